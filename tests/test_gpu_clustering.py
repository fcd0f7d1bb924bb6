"""Clustering scores on the device (smx_cluster.hip) against the float64 restatement tests/clustering_ref.py: the silhouette sums, the batched
Lloyd iterations, their independence of the batch, the edges, the argument checks, and the route from a model to the reference's score table.

Tolerances.  a, b, inertia and centres to 1e-10 relative: the order of a float64 sum of N terms moves it by about N 2^-53, 1e-13 at N = 1000,
and three decades are left for the square roots.  Labels, iteration counts and the best restart are EQUAL: the restatement's smallest
relative gap between a cell's best and second-best centre is asserted >= 1e-9 first, seven decades above the summation noise, so the label
sequence has one answer."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import clustering_ref as R
from tests.util import make_pair, perturbed_params, synth_counts, synth_labels

pytestmark = pytest.mark.gpu

NAMES = list(R.DATASETS)
RTOL = 1e-10


@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


_KM = {}


def _ref_kmeans(name):
  """the restatement's run of every restart of the data set: made once"""
  if name not in _KM:
    Z, _, idx = R.dataset(name)
    _KM[name] = R.kmeans(Z, idx)
  return _KM[name]


def _close(got, want, what):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0, where=want != 0))
  zero = bool(np.all(got[want == 0] == 0))
  print(f"{what}: max relative error {err:.3e}")
  assert err <= RTOL and zero, (what, err)


def _bits(a):
  return np.ascontiguousarray(a).tobytes()


# ---- 1. silhouette sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_silhouette_sums(api, name):
  from sisua_amd.engine import k_cluster_silhouette
  Z, y, _ = R.dataset(name)
  K = R.DATASETS[name][2]
  a, b = k_cluster_silhouette(Z, y, K)
  ra, rb = R.silhouette_sums(Z, y, K)
  assert a.dtype == np.float64 and a.shape == (Z.shape[0],)
  _close(a, ra, f"{name} a")
  _close(b, rb, f"{name} b")
  a2, b2 = k_cluster_silhouette(Z, y, K)
  assert _bits(a) == _bits(a2) and _bits(b) == _bits(b2)
  # the score the four parts are for
  from sisua_amd.clustering import silhouette_from_sums
  cnt = np.bincount(y, minlength=K)[y]
  assert abs(silhouette_from_sums(a, b, cnt == 1)[0] - R.silhouette(ra, rb, cnt)[0]) <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_silhouette_singleton_unused_class_and_duplicates(api, name):
  from sisua_amd.engine import k_cluster_silhouette
  Z, y, _ = R.dataset(name)
  K = R.DATASETS[name][2]
  Z, y = Z.copy(), y.copy()
  y[y >= 1] += 1       # class id 1 is unused
  y[0] = K + 1         # a singleton class
  Z[5] = Z[7]          # exact duplicates
  a, b = k_cluster_silhouette(Z, y, K + 2)
  ra, rb = R.silhouette_sums(Z, y, K + 2)
  assert a[0] == 0.0 and np.isfinite(b).all()
  _close(a, ra, f"{name} a (edges)")
  _close(b, rb, f"{name} b (edges)")


def test_silhouette_nan_row(api):
  from sisua_amd.engine import k_cluster_silhouette
  Z, y, _ = R.dataset("d5")
  Z = Z.copy()
  Z[3] = np.nan
  a, b = k_cluster_silhouette(Z, y, 3)
  with np.errstate(invalid="ignore"):
    ra, rb = R.silhouette_sums(Z, y, 3)
  own = y == y[3]
  assert np.array_equal(np.isnan(a), own) and np.array_equal(np.isnan(b), ~own | (np.arange(257) == 3))
  assert np.array_equal(np.isnan(a), np.isnan(ra)) and np.array_equal(np.isnan(b), np.isnan(rb))
  _close(a[~own], ra[~own], "a beside a NaN row")
  _close(b[own & (np.arange(257) != 3)], rb[own & (np.arange(257) != 3)], "b beside a NaN row")
  Z[3] = np.inf   # an infinity is read as NaN
  a2, b2 = k_cluster_silhouette(Z, y, 3)
  assert np.array_equal(np.isnan(a2), np.isnan(a)) and np.array_equal(np.isnan(b2), np.isnan(b))


def test_silhouette_with_one_class_in_use(api):
  """the C entry with every cell in one class (the Python layer refuses this before the device): no other class has a cell, so b = +inf"""
  from sisua_amd.engine import k_cluster_silhouette
  Z, _, _ = R.dataset("d5")
  for n in (257, 1):
    a, b = k_cluster_silhouette(Z[:n], np.ones(n, np.int32), 3)
    ra, _ = R.silhouette_sums(Z[:n], np.ones(n, np.int64), 3)
    assert np.isposinf(b).all()
    _close(a, ra, f"a of {n} cell(s) in one class")


# ---- 2. k-means --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_kmeans_is_the_restatement(api, name):
  from sisua_amd.engine import k_cluster_kmeans
  Z, _, idx = R.dataset(name)
  ref = _ref_kmeans(name)
  print(f"{name}: smallest relative gap of the restatement {ref['gap']:.3e}, iterations {ref['n_iter'].tolist()}")
  assert ref["gap"] >= 1e-9   # the condition that makes equality the right demand
  got = k_cluster_kmeans(Z, idx, max_iter=300, all_labels=True)
  assert np.array_equal(got["labels_all"], ref["labels_all"])
  assert np.array_equal(got["n_iter"], ref["n_iter"]) and got["best"] == ref["best"]
  assert np.array_equal(got["labels"], ref["labels_all"][ref["best"]])
  _close(got["inertia"], ref["inertia"], f"{name} inertia")
  _close(got["centres"], ref["centres_all"][ref["best"]], f"{name} centres")
  again = k_cluster_kmeans(Z, idx, max_iter=300, all_labels=True)
  assert all(_bits(got[k]) == _bits(again[k]) for k in ("labels_all", "labels", "centres", "inertia", "n_iter"))


@pytest.mark.parametrize("name", NAMES)
def test_kmeans_restart_alone_and_iteration_limits(api, name):
  from sisua_amd.engine import k_cluster_kmeans
  Z, _, idx = R.dataset(name)
  ref = _ref_kmeans(name)
  batch = k_cluster_kmeans(Z, idx, max_iter=300, all_labels=True)
  for r in sorted({0, len(idx) - 1, batch["best"]}):
    alone = k_cluster_kmeans(Z, idx[r:r + 1], max_iter=300)
    assert alone["best"] == 0 and np.array_equal(alone["labels"], batch["labels_all"][r]) and alone["n_iter"][0] == batch["n_iter"][r]
    assert _bits(alone["inertia"][0]) == _bits(batch["inertia"][r])
    if r == batch["best"]:
      assert _bits(alone["centres"]) == _bits(batch["centres"])
    # max_iter = the iterations it needs: the converged result
    exact = k_cluster_kmeans(Z, idx[r:r + 1], max_iter=int(ref["n_iter"][r]))
    assert np.array_equal(exact["labels"], alone["labels"]) and _bits(exact["inertia"]) == _bits(alone["inertia"]) and \
        _bits(exact["centres"]) == _bits(alone["centres"]) and exact["n_iter"][0] == ref["n_iter"][r]
  # max_iter = 1: the first assignment, against the initial centres
  first = k_cluster_kmeans(Z, idx, max_iter=1, all_labels=True)
  want = [R.lloyd(Z, row, 1) for row in idx]
  assert np.array_equal(first["labels_all"], np.stack([w[0] for w in want])) and (first["n_iter"] == 1).all()
  _close(first["inertia"], [w[2] for w in want], f"{name} inertia of the first assignment")
  assert np.array_equal(first["centres"], Z[idx[first["best"]]].astype(np.float64))


def test_kmeans_empty_cluster_keeps_its_centre(api):
  from sisua_amd.engine import k_cluster_kmeans
  Z, _, _ = R.dataset("d5")
  Z = Z.copy()
  Z[1] = Z[0]
  init = np.array([[0, 1, 200]], np.int32)   # two equal centres: ties go to the lower index, so cluster 1 starts empty
  two = k_cluster_kmeans(Z, init, max_iter=2)
  assert not (R.lloyd(Z, init[0], 1)[0] == 1).any()
  assert np.array_equal(two["centres"][1], Z[0].astype(np.float64)) and two["n_iter"][0] == 2   # kept through the first update
  got = k_cluster_kmeans(Z, init, max_iter=50)
  want = R.lloyd(Z, init[0], 50)
  assert got["n_iter"][0] == want[3] <= 50 and np.array_equal(got["labels"], want[0])
  _close(got["centres"], want[1], "centres after an empty cluster")
  _close(got["inertia"], [want[2]], "inertia after an empty cluster")


def test_invalid_arguments(api):
  from sisua_amd import _hip
  from sisua_amd.engine import k_cluster_kmeans, k_cluster_silhouette
  Z, y, idx = R.dataset("d5")
  wide = np.zeros((257, 129), np.float32)
  bad_y, bad_idx = y.copy(), idx.copy()
  bad_y[9], bad_idx[2, 1] = 3, 257
  calls = [lambda: k_cluster_silhouette(np.zeros((257, 0), np.float32), y, 3), lambda: k_cluster_silhouette(wide, y, 3),
           lambda: k_cluster_silhouette(Z, np.zeros(257, np.int32), 1), lambda: k_cluster_silhouette(Z, bad_y, 3),
           lambda: k_cluster_silhouette(Z, -bad_y, 3), lambda: k_cluster_silhouette(Z, y, 257),
           lambda: k_cluster_kmeans(np.zeros((257, 0), np.float32), idx), lambda: k_cluster_kmeans(wide, idx),
           lambda: k_cluster_kmeans(Z, idx[:, :1]), lambda: k_cluster_kmeans(Z, bad_idx), lambda: k_cluster_kmeans(Z, -bad_idx),
           lambda: k_cluster_kmeans(Z, idx, max_iter=0), lambda: k_cluster_kmeans(Z[:2], idx % 2)]
  for i, call in enumerate(calls):
    with pytest.raises(_hip.SmxError) as err:
      call()
    assert err.value.code == -1, i   # SMX_ERR_INVALID


# ---- 3. from a model ---------------------------------------------------------------------------------------------------------------
N_CELLS, G = 257, 60
_MODELS = {}


def _model(api, kind):
  """an unfitted model whose engine holds the oracle's initial weights moved off the symmetric point (tests.util.perturbed_params)"""
  if kind not in _MODELS:
    from sisua_amd import config
    net = dict(encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
    lat = api.RVmeta(6, "diag", True, "Latents")
    if kind == "scvi":
      m = api.SCVI(outputs=api.RVmeta(G, "zinbd", True, "transcriptomic"), latents=lat, **net)
    elif kind == "dca":
      m = api.DeepCountAutoencoder(outputs=api.RVmeta(G, "zinb", True, "transcriptomic"), **net)
    else:
      m = api.VAE(outputs=api.RVmeta(G, "zinb", True, "transcriptomic"), latents=lat, **net)
    cfg = m._make_config()
    spec, _ = make_pair(model=cfg.model, n_genes=G, likelihood=cfg.likelihood, enc_units=cfg.enc_units, dec_units=cfg.dec_units,
                        latent_dim=cfg.latent_dim, encl_units=cfg.encl_units)
    params = perturbed_params(spec)
    assert list(params) == list(config.init_params(cfg))
    m._ensure_engine(512).set_params(params)
    _MODELS[kind] = m
  return _MODELS[kind]


def _data():
  x = synth_counts(N_CELLS, G, sparsity=0.8, seed=3)
  extras = synth_labels(N_CELLS, ((5, "nb"),))[0].astype(np.float64)
  return x, extras


@pytest.mark.parametrize("kind", ["vae", "dca"])
def test_model_scores_are_the_scores_of_its_latent_means(api, kind):
  from sisua_amd import metrics
  m = _model(api, kind)
  x, extras = _data()
  kw = dict(n_init=10, max_iter=100)
  want = metrics.clustering_scores(np.asarray(m.encode(x).mean()), extras, 5, **kw)
  assert set(want) == {"ASW", "ARI", "NMI", "UCA"} and all(np.isfinite(v) for v in want.values())
  assert -1.0 <= want["ASW"] <= 1.0 and 0.0 <= want["UCA"] <= 1.0
  for inputs in (x, sp.csr_matrix(x)):
    for bs in (8, 64):
      got = m.clustering_scores(inputs, extras, batch_size=bs, **kw)
      assert {k: _bits(np.float64(v)) for k, v in got.items()} == {k: _bits(np.float64(v)) for k, v in want.items()}, (bs, got, want)
  # 1-D labels: n_labels defaults to the number of distinct ones
  y = R.prepare_labels(extras)
  assert m.clustering_scores(x, y, batch_size=64, **kw) == metrics.clustering_scores(np.asarray(m.encode(x).mean()), y, np.unique(y).size, **kw)


def test_clustering_scores_metric(api):
  from sisua_amd import metrics
  x, extras = _data()
  kw = dict(n_init=10, max_iter=100)
  m = _model(api, "vae")
  got = metrics.ClusteringScores(x, extras, batch_size=64, **kw)(m)
  want = metrics.clustering_scores(np.asarray(m.encode(x).mean()), np.argmax(extras, 1), 5, **kw)
  assert set(got) == {"ASW", "ARI", "NMI", "UCA", "ASW_0", "ARI_0", "NMI_0", "UCA_0"}
  for k, v in want.items():
    assert got[k] == got[k + "_0"] == -v, k
  assert got["UCA"] < 0.0
  # scvi: the library latent is the second entry, and the plain keys are the mean of the two
  s = _model(api, "scvi")
  got = metrics.ClusteringScores(x, extras, batch_size=64, **kw)(s)
  qz, ql = s.encode(x)
  assert np.asarray(ql.mean()).shape == (N_CELLS, 1)
  for idx, q in enumerate((qz, ql)):
    want = metrics.clustering_scores(np.asarray(q.mean()), np.argmax(extras, 1), 5, **kw)
    for k, v in want.items():
      assert got[f"{k}_{idx}"] == -v, (k, idx)
  assert set(got) == {f"{k}{sfx}" for k in ("ASW", "ARI", "NMI", "UCA") for sfx in ("", "_0", "_1")}
  for k in ("ASW", "ARI", "NMI", "UCA"):
    assert got[k] == float(np.mean([got[k + "_0"], got[k + "_1"]]))
