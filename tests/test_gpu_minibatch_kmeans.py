"""smx_mbkmeans.hip on the device against the float64 restatement (tests/minibatch_kmeans_ref.py), through engine.k_mbkmeans_*, then
`sisua_amd.MiniBatchKMeans` against scikit-learn itself and `SingleCellOMIC.clustering` against the restatement's recipe.

What is compared, per case: the seeding's indices EQUAL and its potentials within the bound below; a first step from zero counts and a
second from the updated ones: labels and counts EQUAL, inertia within the bound, centres within
4 (m + 2) 2^-53 (|c| count + sum |x|) / (count + m) elementwise (c, count: before the step; m, sum |x|: the centre's rows); predict:
labels EQUAL, distances within the bound.  The bound of a sum of non-negative terms, whatever the order on either side: a squared
distance makes at most G + 2 roundings on its way (the difference, the square, G - 1 additions; one less where the square is fused),
a sum of n of them n - 1 more, so |device - restatement| <= 2 (G + n + 2) 2^-53 x the sum (`chain_bound`).
Equality is honest because the restatement's margins hold for every case (asserted, no row exempted): a row's two smallest distances
differ by more than 1e-9 relative unless the two centres are the same row; every pick's u x pot lies more than 1e-9 pot from the scan
values around it; the two best candidate potentials differ by more than 1e-9 relative unless they are the same row.

Shapes: the host fixtures; n_genes 1 and 255 / 256 / 257 around the kernel's column trip of 256; n_clusters 2, 5 (one above the 4 centres
a wave holds at once) and 256; rows = n_clusters, 63, 65 and 257 around the 16 rows of a workgroup; a block of three distinct rows for
five centres (the potential reaches 0 and the picks fall to row 0); a CSR matrix with empty rows and an empty last column."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import minibatch_kmeans_ref as R

pytestmark = pytest.mark.gpu

# name -> (rows, genes, K, seed); the data seeds were chosen on the CPU so that the margins hold
SHAPES = {
    "g1": (63, 1, 2, 0),
    "g255": (65, 255, 5, 0),
    "g256": (257, 256, 256, 0),
    "g257": (12, 257, 12, 0),
}
DATA_SEED = 2   # of the host fixtures
CASES = list(R.FIXTURES) + list(SHAPES) + ["few_distinct", "csr_holes"]


def _matrix(name):
  if name in R.FIXTURES:
    return R.make(name, DATA_SEED), R.FIXTURES[name][2]
  if name == "few_distinct":
    base = np.array([[0, 1, 2, 3, 4, 5, 6], [9, 8, 7, 6, 5, 4, 3], [2, 2, 30, 2, 2, 2, 2]], np.float32)
    return base[np.random.RandomState(4).randint(0, 3, 40)], 5
  if name == "csr_holes":
    x = np.floor(np.abs(np.random.RandomState(5).normal(0.0, 6.0, (90, 21)))).astype(np.float32)
    x[x < 6] = 0.0
    x[[0, 17, 40, 89]] = 0.0
    x[:, -1] = 0.0
    return x, 4
  rows, genes, K, seed = SHAPES[name]
  rng = np.random.RandomState(2000 + seed)
  return (rng.normal(0.0, 4.0, (K, genes))[np.arange(rows) % K] + rng.normal(0.0, 1.0, (rows, genes))).astype(np.float32), K


@functools.lru_cache(maxsize=None)
def case(name):
  """the matrix, the draws and the restatement's results of a case: computed once, shared, never written to"""
  x, K = _matrix(name)
  rng = np.random.RandomState(11)
  first, u = int(rng.randint(x.shape[0])), rng.uniform(size=(K - 1, 2 + int(np.log(K))))
  mg = R.Margins()
  seed = R.k_seed(x, K, first, u, margins=mg)
  s1 = R.k_step(x, seed["centres"], np.zeros(K), margins=mg)
  s2 = R.k_step(x, s1["centres"], s1["counts"], margins=mg)
  lab, dist = R.k_predict(x, s2["centres"], want_distance=True, margins=mg)
  for a in (x, u, lab, dist, *seed.values(), *[v for s in (s1, s2) for v in s.values() if isinstance(v, np.ndarray)]):
    a.setflags(write=False)
  return dict(x=x, K=K, first=first, u=u, seed=seed, s1=s1, s2=s2, labels=lab, dist=dist, margins=mg)


def sum_bound(n, G, total):
  return R.chain_bound(G + n + 2, total)


def centre_bound(x, c, count, labels):
  """[K, G]: 4 (m + 2) 2^-53 (|c| count + sum |x|) / (count + m); rows of centres without members are 0 (left alone: equal bits)"""
  X = np.abs(x.astype(np.float64))
  out = np.zeros_like(c)
  for k in range(c.shape[0]):
    rows = labels == k
    m = int(rows.sum())
    if m:
      out[k] = 4 * (m + 2) * R.EPS * (np.abs(c[k]) * count[k] + X[rows].sum(axis=0)) / (count[k] + m)
  return out


@pytest.mark.parametrize("name", CASES)
def test_margins_hold(name):
  mg = case(name)["margins"]
  assert mg.ok(), (mg.row, mg.pick, mg.cand)


@pytest.mark.parametrize("name", CASES)
def test_seed(name):
  from sisua_amd import engine
  c = case(name)
  n, G = c["x"].shape
  got = engine.k_mbkmeans_seed(c["x"], c["K"], c["first"], c["u"])
  ref = c["seed"]
  err = np.abs(got["potential"] - ref["potential"])
  print(name, "potential error / bound", float((err / np.maximum(sum_bound(n, G, ref["potential"]), 1e-300)).max()))
  assert np.array_equal(got["indices"], ref["indices"])
  assert np.array_equal(got["centres"], ref["centres"])   # (rows of x)
  assert (err <= sum_bound(n, G, ref["potential"])).all()
  if name == "few_distinct":
    assert ref["potential"][-1] == 0.0 and got["potential"][-1] == 0.0 and got["indices"][-1] == 0
  again, sparse = engine.k_mbkmeans_seed(c["x"], c["K"], c["first"], c["u"]), engine.k_mbkmeans_seed(sp.csr_matrix(c["x"]), c["K"], c["first"], c["u"])
  for k in got:
    assert np.array_equal(got[k], again[k]) and np.array_equal(got[k], sparse[k]), k


@pytest.mark.parametrize("name", CASES)
def test_step(name):
  from sisua_amd import engine
  c = case(name)
  x, K = c["x"], c["K"]
  n, G = x.shape
  centres, counts = c["seed"]["centres"], np.zeros(K)
  for ref in (c["s1"], c["s2"]):
    got = engine.k_mbkmeans_step(x, centres, counts)
    bound = centre_bound(x, centres, counts, ref["labels"])
    err = np.abs(got["centres"] - ref["centres"])
    print(name, "inertia error / bound", abs(got["inertia"] - ref["inertia"]) / max(sum_bound(n, G, ref["inertia"]), 1e-300),
          "centre error / bound", float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    assert np.array_equal(got["labels"], ref["labels"])
    assert np.array_equal(got["counts"], ref["counts"])
    assert abs(got["inertia"] - ref["inertia"]) <= sum_bound(n, G, ref["inertia"])
    assert (err <= bound).all()
    again, sparse = engine.k_mbkmeans_step(x, centres, counts), engine.k_mbkmeans_step(sp.csr_matrix(x), centres, counts)
    for k in ("centres", "counts", "labels"):
      assert np.array_equal(got[k], again[k]) and np.array_equal(got[k], sparse[k]), k
    assert got["inertia"] == again["inertia"] == sparse["inertia"]
    assert engine.k_mbkmeans_step(x, centres, counts, want_labels=False)["labels"] is None
    centres, counts = ref["centres"], ref["counts"]


@pytest.mark.parametrize("name", CASES)
def test_predict(name):
  from sisua_amd import engine
  c = case(name)
  x, centres = c["x"], c["s2"]["centres"]
  lab, dist = engine.k_mbkmeans_predict(x, centres, want_distance=True)
  err, bound = np.abs(dist - c["dist"]), R.chain_bound(x.shape[1] + 2, c["dist"])
  print(name, "distance error / bound", float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
  assert np.array_equal(lab, c["labels"])
  assert (err <= bound).all()
  for X in (x, sp.csr_matrix(x)):
    for block_rows in (1, 7, 64, 0):
      l2, d2 = engine.k_mbkmeans_predict(X, centres, block_rows=block_rows, want_distance=True)
      assert np.array_equal(l2, lab) and np.array_equal(d2, dist), block_rows
  assert np.array_equal(engine.k_mbkmeans_predict(x, centres), lab)


def test_nonfinite_input_is_refused():
  from sisua_amd import engine
  x = np.array(case("tiny")["x"])
  x[3, 2] = np.nan
  with pytest.raises(ValueError, match="not finite"):
    engine.k_mbkmeans_predict(x, case("tiny")["s2"]["centres"])


@pytest.mark.parametrize("name", ["wide", "outlier_a"])
def test_class_against_scikit_learn(name):
  from sklearn.cluster import MiniBatchKMeans as SkMiniBatchKMeans
  from sisua_amd import MiniBatchKMeans
  rows, genes, K, batch, _ = R.FIXTURES[name]
  x = R.make(name, DATA_SEED)
  x64 = x.astype(np.float64)
  sk = SkMiniBatchKMeans(n_clusters=K, batch_size=batch, random_state=1, compute_labels=False)
  ours = MiniBatchKMeans(n_clusters=K, batch_size=batch, random_state=1)
  for s in range(0, rows, batch):
    sk.partial_fit(x64[s:s + batch])
    ours.partial_fit(x[s:s + batch])
  assert np.array_equal(ours.counts_, sk._counts) and ours.n_steps_ == sk.n_steps_
  err = np.abs(ours.cluster_centers_ - sk.cluster_centers_).max()
  print(name, "centres: max error", err, "of", np.abs(sk.cluster_centers_).max())
  assert err <= 1e-10 * np.abs(sk.cluster_centers_).max()
  assert np.array_equal(ours.predict(x), sk.predict(x64))
  assert ours.labels_.shape == (rows - (rows - 1) // batch * batch,) and ours.inertia_ >= 0


@pytest.mark.parametrize("sparse", [False, True])
def test_singlecell_clustering(sparse):
  from sisua_amd.data import SingleCellOMIC
  rng = np.random.RandomState(4)
  group = rng.randint(0, 4, 300)
  x = np.floor(np.abs(rng.normal(0.0, 3.0, (4, 40))[group] * 4 + rng.normal(0.0, 2.0, (300, 40)))).astype(np.float32)
  x[x < 4] = 0.0
  prot, var = np.eye(4, dtype=np.float32)[(group + 1) % 4], np.array(["a", "b", "c", "d"])

  def container():
    return SingleCellOMIC(sp.csr_matrix(x) if sparse else x, omic="transcriptomic").add_omic("proteomic", prot, var_names=var)

  ids = container().clustering(n_clusters=4)
  assert np.array_equal(ids, R.clustering(x, 4, random_state=1)) and ids.dtype == np.int64
  sco = container()
  names = sco.clustering(n_clusters="proteomic")
  assert np.array_equal(names, R.clustering(x, 4, random_state=1, probs=sco.get_x_probs("proteomic"), var_names=var))
  assert sco.clustering(n_clusters="proteomic", return_key=True) == "transcriptomic_kmeans4"
