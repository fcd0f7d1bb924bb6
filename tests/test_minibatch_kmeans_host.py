"""Mini-batch k-means on the host: (1) the NumPy restatement (tests/minibatch_kmeans_ref.py) IS scikit-learn's
MiniBatchKMeans.partial_fit / predict -- equal counts, centres within 1e-10 max|centre| (both sides are float64 sums of at most 4096
terms, n eps = 5e-13; measured 3e-16), equal labels -- on Gaussian blobs, duplicated and zero count rows, and three fixtures with
planted outliers that make scikit-learn reassign starved centres; (2) `sisua_amd.MiniBatchKMeans`, `sisua_amd.clustering.minibatch_kmeans`
and `SingleCellOMIC.clustering` with engine.k_mbkmeans_* replaced by the restatement: the draws, the keys, what is kept and dropped,
the matching, `rank_vars_groups(group_by=key)`; (3) every refusal comes before the device is asked for.  The device's side of the
contract is tests/test_gpu_minibatch_kmeans.py."""
import re

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.cluster import MiniBatchKMeans as SkMiniBatchKMeans

import sisua_amd
from sisua_amd import _hip, build, engine
from sisua_amd import clustering as cl
from sisua_amd.data import SingleCellOMIC
from tests import minibatch_kmeans_ref as R

ROOT = build.os.path.dirname(build.HERE)
SEEDS = (1, 2, 3)


def run_both(x, K, batch, seed, init="k-means++", sparse=False, ours=None):
  """(scikit-learn on the float64 copy, scikit-learn on the float32 input, the model under test) after one partial_fit per batch"""
  sk_init = init if isinstance(init, str) else np.array(init, np.float64)
  sk64 = SkMiniBatchKMeans(n_clusters=K, init=sk_init, batch_size=batch, random_state=seed, compute_labels=False)
  sk32 = SkMiniBatchKMeans(n_clusters=K, init=sk_init if isinstance(init, str) else np.array(init, np.float32), batch_size=batch,
                           random_state=seed, compute_labels=False)
  m = ours or R.Model(K, init=init, batch_size=batch, random_state=seed, compute_labels=False)
  wrap = sp.csr_matrix if sparse else (lambda a: a)
  for s in range(0, x.shape[0], batch):
    sk64.partial_fit(wrap(x[s:s + batch].astype(np.float64)))
    sk32.partial_fit(wrap(x[s:s + batch]))
    m.partial_fit(wrap(x[s:s + batch]))
  return sk64, sk32, m


def hold(sk64, sk32, centres, counts, labels, x):
  assert np.array_equal(counts, sk64._counts)
  assert np.abs(centres - sk64.cluster_centers_).max() <= 1e-10 * np.abs(sk64.cluster_centers_).max()
  assert np.array_equal(labels, sk32.predict(x))


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_restatement_is_scikit_learn(name):
  rows, genes, K, batch, kind = R.FIXTURES[name]
  reassigned = 0
  for seed in SEEDS:
    x = R.make(name, seed)
    sk64, sk32, m = run_both(x, K, batch, seed)
    hold(sk64, sk32, m.centres, m.counts, m.predict(x), x)
    assert m.n_steps == sk64.n_steps_ == -(-rows // batch)
    reassigned += any(m.reassigned)
  if name in R.OUTLIER_FIXTURES:
    assert reassigned >= 1   # (the planted outliers starve their centres: scikit-learn's reassignment is on the tested path)


@pytest.mark.parametrize("name", ["wide", "outlier_b"])
def test_restatement_random_and_array_init(name):
  rows, genes, K, batch, _ = R.FIXTURES[name]
  x = R.make(name, 1)
  for init in ("random", x[np.random.RandomState(7).choice(rows, K, replace=False)]):
    sk64, sk32, m = run_both(x, K, batch, 2, init=init)
    hold(sk64, sk32, m.centres, m.counts, m.predict(x), x)


@pytest.mark.parametrize("name", ["counts", "outlier_a"])
def test_restatement_csr_is_scikit_learns_csr_path(name):
  rows, genes, K, batch, _ = R.FIXTURES[name]
  x = R.make(name, 1)
  sk64, sk32, m = run_both(x, K, batch, 1, sparse=True)
  assert np.array_equal(m.counts, sk64._counts)
  assert np.abs(m.centres - sk64.cluster_centers_).max() <= 1e-10 * np.abs(sk64.cluster_centers_).max()
  assert np.array_equal(m.predict(sp.csr_matrix(x)), sk32.predict(sp.csr_matrix(x)))


# ---- the class and the container, on the restatement -------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
  """a refusal must never reach the library"""
  def boom(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", boom)


@pytest.fixture
def ref_driver(monkeypatch, no_device):
  """engine.k_mbkmeans_* replaced by the restatement; counts the calls"""
  calls = dict(seed=0, step=0, predict=0)

  def count(name, f):
    def g(*a, **k):
      calls[name] += 1
      return f(*a, **k)
    return g

  monkeypatch.setattr(engine, "k_mbkmeans_seed", count("seed", R.k_seed))
  monkeypatch.setattr(engine, "k_mbkmeans_step", count("step", R.k_step))
  monkeypatch.setattr(engine, "k_mbkmeans_predict", count("predict", R.k_predict))
  return calls


@pytest.mark.parametrize("name,init", [("wide", "k-means++"), ("outlier_a", "k-means++"), ("outlier_c", "random"), ("tiny", "array"),
                                       ("counts", "k-means++")])
def test_class_draws_what_scikit_learn_draws(ref_driver, name, init):
  rows, genes, K, batch, _ = R.FIXTURES[name]
  x = R.make(name, 2)
  if init == "array":
    init = x[:K].astype(np.float64)
  ours = sisua_amd.MiniBatchKMeans(n_clusters=K, init=init, batch_size=batch, random_state=2)
  sk64, sk32, m = run_both(x, K, batch, 2, init=init, ours=ours)
  hold(sk64, sk32, m.cluster_centers_, m.counts_, m.predict(x), x)
  steps = -(-rows // batch)
  assert m.n_steps_ == steps and m.cluster_centers_.dtype == np.float64
  assert ref_driver == dict(seed=int(isinstance(init, str) and init == "k-means++"), step=steps, predict=steps + 1)
  last = x[(steps - 1) * batch:]
  lab, d = R.k_predict(last, m.cluster_centers_, want_distance=True)
  assert np.array_equal(m.labels_, lab) and m.inertia_ == float(d.sum())
  # the stream after the fit stands where scikit-learn's stands
  assert m._rng.randint(1 << 30) == sk64._random_state.randint(1 << 30)


def test_class_without_labels_and_csr(ref_driver):
  rows, genes, K, batch, _ = R.FIXTURES["wide"]
  x = R.make("wide", 3)
  a = sisua_amd.MiniBatchKMeans(K, batch_size=batch, random_state=5, compute_labels=False)
  b = sisua_amd.MiniBatchKMeans(K, batch_size=batch, random_state=5, compute_labels=False)
  for s in range(0, rows, batch):
    a.partial_fit(x[s:s + batch])
    b.partial_fit(sp.csr_matrix(x[s:s + batch]))
  assert not hasattr(a, "labels_") and ref_driver["predict"] == 0
  assert np.array_equal(a.cluster_centers_, b.cluster_centers_) and np.array_equal(a.counts_, b.counts_)
  assert np.array_equal(a.predict(x), b.predict(sp.csr_matrix(x)))


def test_minibatch_kmeans_function_is_the_recipe(ref_driver):
  x = R.make("outlier_a", 2)
  got = cl.minibatch_kmeans(x, 4, batch_size=128, random_state=3)
  assert np.array_equal(got, R.clustering(x, 4, random_state=3, batch_size=128))
  assert ref_driver == dict(seed=1, step=4, predict=1)
  order = R.batches(400, 128, 3)
  assert sorted(order) == [(0, 128), (128, 256), (256, 384), (384, 400)] and order != sorted(order)


def test_matching_is_an_assignment_not_the_row_argmax():
  # variable 0 is strongest in cluster 0, and so is variable 1: the row-wise argmax would give cluster 0 twice
  labels = np.array([0, 0, 0, 1, 1, 2])
  probs = np.array([[.9, .8, .1], [.9, .8, .1], [.9, .8, .1], [.6, .1, .1], [.6, .1, .1], [.1, .1, .9]])
  corr = np.array([[probs[labels == c, i].sum() for c in range(3)] for i in range(3)])
  assert list(np.argmax(corr, axis=1)) == [0, 0, 2]
  assert list(cl.match_clusters(labels, probs, 3)) == [1, 0, 2] == list(R.match(labels, probs, 3))


def container(sparse=False, seed=2):
  rng = np.random.RandomState(seed)
  group = rng.randint(0, 4, 300)
  x = np.floor(np.abs(rng.normal(0.0, 3.0, (4, 40))[group] * 4 + rng.normal(0.0, 2.0, (300, 40)))).astype(np.float32)
  x[x < 4] = 0.0
  prot = np.eye(4, dtype=np.float32)[(group + 1) % 4]   # (a 0 / 1 omic is its own probability embedding: no mixture is fitted)
  sco = SingleCellOMIC(sp.csr_matrix(x) if sparse else x, var_names=[f"g{i}" for i in range(40)])
  sco.add_omic("proteomic", prot, var_names=["CD3", "CD4", "CD8", "CD19"])
  return sco, x, prot


@pytest.mark.parametrize("sparse", [False, True])
def test_singlecell_clustering_keys_kept_and_dropped(ref_driver, sparse):
  sco, x, prot = container(sparse)
  var = sco.get_var_names("proteomic")
  ids = sco.clustering(n_clusters=4)
  assert ids.dtype == np.int64 and np.array_equal(ids, R.clustering(x, 4, random_state=1))
  assert list(sco._obs) == ["transcriptomic_kmeans4"] and sco._obs["transcriptomic_kmeans4"][:2] == ("transcriptomic", None)
  n = dict(ref_driver)
  assert sco.clustering(n_clusters=4, return_key=True) == "transcriptomic_kmeans4" and ref_driver == n   # kept
  assert sco.clustering(n_clusters=4, random_state=9) is ids                                              # whatever its other arguments
  sco._replace("proteomic", prot[:, ::-1].copy())
  assert "transcriptomic_kmeans4" in sco._obs                                                             # no cluster omic behind it

  sco2, _, _ = container(sparse)
  names = sco2.clustering(n_clusters="proteomic")
  assert np.array_equal(names, R.clustering(x, 4, random_state=1, probs=sco2.get_x_probs("proteomic"), var_names=var))
  assert set(names) <= set(var) and sco2._obs["transcriptomic_kmeans4"][:2] == ("transcriptomic", "proteomic")
  sco2._replace("proteomic", prot[:, ::-1].copy())
  assert not sco2._obs                                                                                    # the cluster omic was replaced
  raw = sco2.clustering(n_clusters="proteomic", matching_labels=False)
  assert np.array_equal(raw, ids)
  sco2._replace("transcriptomic", x * 2)
  assert not sco2._obs
  assert not sco2[np.arange(50)]._obs and not sco.copy()._obs                                            # a subset starts without

  sco3, _, _ = container(sparse)
  own = sco3.clustering("proteomic", random_state=3)   # n_clusters=None: the omic's own width, and the omic names its clusters
  assert list(sco3._obs) == ["proteomic_kmeans4"] and sco3._obs["proteomic_kmeans4"][:2] == ("proteomic", "proteomic")
  assert np.array_equal(own, R.clustering(prot, 4, random_state=3, probs=sco3.get_x_probs("proteomic"), var_names=var))


def test_singlecell_clustering_pca_and_tsne_routes(ref_driver, monkeypatch):
  sco, x, _ = container()
  asked = []

  def reduce(omic=None, n_components=100, algo="pca", random_state=1):
    asked.append((omic, n_components, algo))
    return x[:, :5] if algo == "pca" else x[:, :2]

  monkeypatch.setattr(sco, "dimension_reduce", reduce)
  assert np.array_equal(sco.clustering(n_clusters=3, algo="PCA "), R.clustering(x[:, :5], 3, random_state=1))
  assert np.array_equal(sco.clustering(n_clusters=3, algo="tsne"), R.clustering(x[:, :2], 3, random_state=1))
  assert asked == [("transcriptomic", 100, "pca"), ("transcriptomic", 2, "tsne")]
  assert sorted(sco._obs) == ["transcriptomic_pca3", "transcriptomic_tsne3"]


def test_rank_vars_groups_takes_a_clustering_key(ref_driver, monkeypatch):
  from tests import rank_groups_ref as RG
  monkeypatch.setattr(engine, "k_group_moments", lambda x, labels, n_groups, block_rows=0: RG.group_moments(x, labels, n_groups))
  sco, x, prot = container()
  key = sco.clustering(n_clusters="proteomic", return_key=True)
  rank_key = sco.rank_vars_groups(n_vars=5, group_by=key, method="t-test")
  assert rank_key == "transcriptomic_transcriptomic_kmeans4_rank"
  res = sco.get_rank_vars_groups(rank_key)
  want = RG.rank_genes_groups(x, sco.clustering(n_clusters="proteomic"), method="t-test", n_genes=5, var_names=sco.get_var_names("transcriptomic"))
  for g in want:
    assert list(res["names"][g]) == list(want[g]["names"])
  with pytest.raises(NotImplementedError, match="clustering=None"):
    sco.rank_vars_groups(method="t-test")   # (the reference's default call is still two calls here)
  sco._replace("proteomic", prot[:, ::-1].copy())
  assert key not in sco._obs and rank_key in sco._uns     # the ranking was made from the first omic alone
  sco._replace("transcriptomic", x * 2)
  assert rank_key not in sco._uns


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_never_ask_for_the_device(no_device):
  x = R.make("tiny", 1)
  M = sisua_amd.MiniBatchKMeans
  with pytest.raises(NotImplementedError, match="partial_fit"):
    M(3).fit(x)
  for bad in (1, 257, 2.5, None):
    with pytest.raises(ValueError, match="n_clusters"):
      M(bad)
  with pytest.raises(ValueError, match="init"):
    M(3, init="k-means||")
  with pytest.raises(ValueError, match="init array"):
    M(3, init=np.zeros((4, 5)))
  with pytest.raises(ValueError, match="features"):
    M(3, init=np.zeros((3, 4))).partial_fit(x)
  with pytest.raises(ValueError, match="tol"):
    M(3, tol=1e-3)
  with pytest.raises(ValueError, match="should be >= n_clusters"):
    M(50).partial_fit(x)
  with pytest.raises(ValueError, match="matrix"):
    M(3).partial_fit(x[0])
  with pytest.raises(ValueError, match="partial_fit first"):
    M(3).predict(x)
  with pytest.raises(ValueError, match="matrix"):
    cl.minibatch_kmeans(x[0], 3)
  # the engine's own checks
  c = x[:3].astype(np.float64)
  bad = x.copy()
  bad[4, 1] = np.inf
  for X in (bad, sp.csr_matrix(bad)):
    with pytest.raises(ValueError, match="not finite"):
      engine.k_mbkmeans_predict(X, c)
    with pytest.raises(ValueError, match="not finite"):
      engine.k_mbkmeans_step(X, c, np.zeros(3))
    with pytest.raises(ValueError, match="not finite"):
      engine.k_mbkmeans_seed(X, 3, 0, np.zeros((2, 3)))
  with pytest.raises(ValueError, match="n_clusters"):
    engine.k_mbkmeans_predict(x, c[:1])
  with pytest.raises(ValueError, match="centres"):
    engine.k_mbkmeans_predict(x, c[:, :4])
  with pytest.raises(ValueError, match="counts"):
    engine.k_mbkmeans_step(x, c, np.array([0.0, -1.0, 0.0]))
  with pytest.raises(ValueError, match=r"\[0, 1\)"):
    engine.k_mbkmeans_seed(x, 3, 0, np.ones((2, 3)))
  with pytest.raises(ValueError, match="u must be"):
    engine.k_mbkmeans_seed(x, 3, 0, np.zeros((2, 17)))
  with pytest.raises(ValueError, match="first"):
    engine.k_mbkmeans_seed(x, 3, 37, np.zeros((2, 3)))
  with pytest.raises(ValueError, match="rows"):
    engine.k_mbkmeans_seed(x[:2], 3, 0, np.zeros((2, 3)))
  with pytest.raises(ValueError, match="block_rows"):
    engine.k_mbkmeans_predict(x, c, block_rows=-1)
  # the container
  sco, _, _ = container()
  for algo in ("knn", "umap", "louvain"):
    with pytest.raises(NotImplementedError, match="'kmeans', 'pca' and 'tsne'"):
      sco.clustering(n_clusters=4, algo=algo)
  with pytest.raises(ValueError):
    sco.clustering(n_clusters="epigenomic")
  with pytest.raises(ValueError, match="n_clusters"):
    sco.clustering(n_clusters=1)
  with pytest.raises(ValueError, match="n_clusters"):
    sco.clustering(n_clusters=300)


def test_header_binding_build_list_and_documents_agree():
  hdr = open(build.os.path.join(ROOT, "include", "sisua_hip.h")).read()
  assert int(re.search(r"#define SMX_ABI_VERSION (\d+)", hdr).group(1)) == _hip.SMX_ABI_VERSION >= 16
  assert "smx_mbkmeans.hip" in build.SOURCES
  for name, n_args in (("smx_mbkmeans_seed", 13), ("smx_mbkmeans_step", 11), ("smx_mbkmeans_predict", 11)):
    proto = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
    assert len(proto.split(",")) == n_args == len(_hip.SIGNATURES[name][1])
    assert name in open(build.os.path.join(ROOT, "tools", "asan", "host_driver.cpp")).read()
  assert "MiniBatchKMeans" in dir(sisua_amd)
  for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
    text = open(build.os.path.join(ROOT, doc)).read()
    assert "MiniBatchKMeans" in text and "`SingleCellOMIC.clustering` is not built" not in text, doc
