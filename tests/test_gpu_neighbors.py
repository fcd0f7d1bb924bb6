"""The neighbour graphs on the device (smx_pca.hip, smx_knn.hip through engine.k_pca_cov / k_pca_project / k_knn / k_knn_umap,
sisua_amd/neighbors.py and SingleCellOMIC.dimension_reduce / neighbors) against the float64 restatement tests/neighbors_ref.py.

Shapes are the smallest at which the kernels can still go wrong: rows around the MFMA's group of 4 and the block's slices of 64, columns
around the 16-wide fragment and the 64-wide macro-tile, cells around the workgroup of 256, widths around the register paddings.

Bounds.
  covariance   a sum of n products in two orders differs by at most about 2 n u sum |a b| <= 2 n u (n - 1) sqrt(S_ii S_jj), u = 2^-53;
               the issue sets |dS_ij| <= 4 n 2^-53 sqrt(S_ii S_jj) and mean to n 2^-53 max |x|.  A constant column gives exactly 0.
  projection   the float32 rounding of the float64 restatement: equal or one float32 ulp apart, equal in at least 99 % of the entries.
  kNN          integer coordinates: every d2 is an exact integer, so idx and dist are EQUAL and the tie rule decides most ranks.
               Gaussian data: first the restatement's own relative gap between consecutive sorted d2 must pass 1e-11 (two float64 sums of
               <= 128 terms differ by ~1e-14 relative), then idx EQUAL and dist to rtol 1e-13.  k = n - 1 is run where the entry takes
               it (k <= 256): at n = 600 the largest k, 256, stands in.
  UMAP rows    first the restatement's own branch margins must pass 1e-10, then rho EQUAL, sigma and weights to rtol 1e-12."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from sisua_amd import _hip, engine, neighbors
from sisua_amd.data import SingleCellOMIC, synthetic_8kly
from tests import neighbors_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
COV_N = [2, 3, 4, 5, 63, 64, 65, 257]
COV_G = [1, 15, 16, 17, 33, 100]
PROJECT_SHAPES = [(5, 1, 1), (64, 17, 17), (65, 33, 5), (257, 100, 20), (300, 100, 100), (300, 130, 128)]   # (n, G, C)
KNN_N = [2, 3, 255, 256, 257, 600]
KNN_D = [1, 3, 4, 5, 32, 100, 128]
KNN_GAUSS = [((600, 100, 11), 3), ((257, 5, 11), 4), ((256, 1, 3), 5), ((255, 32, 254), 6)]      # ((n, D, k), seed)
UMAP_CASES = [((300, 10, 12), 7, 0), ((257, 3, 5), 8, 0), ((64, 2, 2), 9, 0), ((200, 4, 12), 10, 20)]   # ((n, D, K), seed, duplicated cells)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _same_graph(a, b):
  return (a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and _same_bits(a.data, b.data))


def _ulp_distance(a, b):
  """float32 arrays -> the distance in units of the last place (finite values)"""
  def ordered(x):
    i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)
  return np.abs(ordered(a) - ordered(b))


@functools.lru_cache(maxsize=None)
def _cov_matrix(n, G):
  """float32 [n, G]: column 0 is 1e4 + small noise (a one-pass covariance fails there), the last column (G >= 2) is constant, some
  entries are 0 so that the CSR twin is sparse; never written to"""
  rng = np.random.default_rng(1000 * n + G)
  x = (3.0 * rng.standard_normal((n, G)) + rng.uniform(-4, 4, G)).astype(np.float32)
  x[rng.uniform(size=(n, G)) < 0.3] = 0.0
  x[:, 0] = (1e4 + 0.01 * rng.standard_normal(n)).astype(np.float32)
  if G >= 2:
    x[:, G - 1] = 2.5
  x.setflags(write=False)
  return x


@pytest.mark.parametrize("G", COV_G)
@pytest.mark.parametrize("n", COV_N)
def test_cov_against_restatement(n, G):
  x = _cov_matrix(n, G)
  mean, S = engine.k_pca_cov(x)
  rmean, rS = R.pca_cov(x)
  assert S.shape == (G, G) and S.dtype == np.float64 and mean.shape == (G,)
  print(n, G, "mean err / bound", float(np.max(np.abs(mean - rmean)) / (n * U * np.abs(x).max())))
  assert np.all(np.abs(mean - rmean) <= n * U * np.abs(x).max())
  scale = np.sqrt(np.outer(np.diag(rS), np.diag(rS)))
  bound = 4 * n * U * scale
  with np.errstate(invalid="ignore", divide="ignore"):
    print(n, G, "max |dS| / bound", float(np.nanmax(np.where(bound > 0, np.abs(S - rS) / bound, 0.0))))
  assert np.all(np.abs(S - rS) <= bound)
  assert np.array_equal(S, S.T)
  if G >= 2:
    assert rS[G - 1, G - 1] == 0 and np.all(S[G - 1] == 0) and np.all(S[:, G - 1] == 0) and mean[G - 1] == 2.5
  assert S[0, 0] > 0 and abs(S[0, 0] / rS[0, 0] - 1) < 1e-9   # the 1e4 column: a one-pass formula loses every digit here


def test_cov_same_bits_for_every_cut():
  x = _cov_matrix(300, 100)
  first = engine.k_pca_cov(x, block_rows=64)
  csr = sp.csr_matrix(x)
  assert csr.nnz < x.size
  for block_rows in (64, 128, 0):
    for m in (x, csr):
      for _ in range(2):
        got = engine.k_pca_cov(m, block_rows=block_rows)
        assert _same_bits(got[0], first[0]) and _same_bits(got[1], first[1]), (block_rows, sp.issparse(m))
  assert np.array_equal(first[1], first[1].T)


@pytest.mark.parametrize("shape", PROJECT_SHAPES)
def test_project_against_restatement(shape):
  n, G, C = shape
  x = R.planted_matrix(n, G, seed=n + G)
  fit = R.pca_fit(x, C)
  want = R.pca_project(x, fit["mean"], fit["components"])
  got = engine.k_pca_project(x, fit["mean"], fit["components"])
  assert got.shape == (n, C) and got.dtype == np.float32
  ulp = _ulp_distance(got, want)
  print(shape, "max ulp", int(ulp.max()), "equal share", float((ulp == 0).mean()))
  assert ulp.max() <= 1 and (ulp == 0).mean() >= 0.99
  csr = sp.csr_matrix(x)
  for block_rows in (64, 128, 0):
    for m in (x, csr):
      assert _same_bits(engine.k_pca_project(m, fit["mean"], fit["components"], block_rows=block_rows), got), (block_rows, sp.issparse(m))


@functools.lru_cache(maxsize=None)
def _grid_cells(n, D):
  z = np.random.default_rng(7 * n + D).integers(-3, 4, size=(n, D)).astype(np.float32)
  z.setflags(write=False)
  return z, R.sq_distances(z)


def _grid_ks(n):
  return sorted({k for k in (1, 11, n - 1) if k < n and k <= 256} | ({256} if n > 257 else set()))


@pytest.mark.parametrize("D", KNN_D)
@pytest.mark.parametrize("n", KNN_N)
def test_knn_integer_grid_is_exact(n, D):
  z, d2 = _grid_cells(n, D)
  for k in _grid_ks(n):
    ridx, rdist, rd2 = R.knn(z, k, d2)
    idx, dist = engine.k_knn(z, k)
    assert idx.dtype == np.int32 and dist.dtype == np.float64 and idx.shape == (n, k)
    assert np.array_equal(idx, ridx), (n, D, k)
    # d2 is an exact integer on both sides and sqrt is correctly rounded: dist EQUAL, and its square rounds back to the integer
    assert np.array_equal(dist, np.sqrt(rd2)) and np.array_equal(dist, rdist) and np.array_equal(np.rint(dist * dist), rd2), (n, D, k)


def _check_gauss(z, k, distinct_only=False):
  d2 = R.sq_distances(z)
  if distinct_only:   # exact ties (duplicated cells) are decided by the index on both sides: guard the gaps between distinct values
    gap = min(float(np.min(np.diff(s) / s[1:])) for s in (np.unique(np.delete(d2[i], i)) for i in range(z.shape[0])) if s.size > 1)
  else:
    gap = R.knn_gap(z, k, d2)
  print(z.shape, k, "smallest relative gap", gap)
  assert gap > 1e-11
  ridx, rdist, _ = R.knn(z, k, d2)
  idx, dist = engine.k_knn(z, k)
  assert np.array_equal(idx, ridx)
  np.testing.assert_allclose(dist, rdist, rtol=1e-13, atol=0)
  return idx, dist


@pytest.mark.parametrize("case,seed", KNN_GAUSS)
def test_knn_gaussian(case, seed):
  n, D, k = case
  _check_gauss(np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32), k)


def test_knn_duplicated_cells():
  z = np.random.default_rng(11).standard_normal((300, 8)).astype(np.float32)
  z[40:60] = z[7]   # 20 copies of cell 7
  idx, dist = _check_gauss(z, 25, distinct_only=True)
  assert np.all(dist[7, :20] == 0) and idx[7, :20].tolist() == list(range(40, 60))
  assert idx[45, :20].tolist() == [7] + [j for j in range(40, 60) if j != 45] and np.all(dist[45, :20] == 0)


def test_knn_same_answers_for_every_slicing():
  cases = [(np.random.default_rng(12).standard_normal((600, 10)).astype(np.float32), 11), (_grid_cells(257, 3)[0], 256)]
  try:
    for z, k in cases:
      _hip.clear_tuning("knn_slices")
      want = engine.k_knn(z, k)
      for slices in (1, 32):
        _hip.set_tuning("knn_slices", slices)
        got = engine.k_knn(z, k)
        assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]), (z.shape, k, slices)
  finally:
    _hip.clear_tuning("knn_slices")


@pytest.mark.parametrize("case,seed,n_dup", UMAP_CASES)
def test_umap_rows(case, seed, n_dup):
  n, D, K = case
  z = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
  if n_dup:
    z[100:100 + n_dup] = z[3]
  idx, dist = R.with_self(*R.knn(z, K - 1)[:2])
  rho, sigma, w, (m_side, m_stop) = R.umap_rows(idx, dist, margins=True)
  print(case, "branch margins", m_side, m_stop)
  assert m_side > 1e-10 and m_stop > 1e-10
  if n_dup:
    assert (rho == 0).sum() >= n_dup   # rows that see only duplicates: the global floor
  grho, gsigma, gw = engine.k_knn_umap(idx, dist)
  assert np.array_equal(grho, rho)
  np.testing.assert_allclose(gsigma, sigma, rtol=1e-12, atol=0)
  np.testing.assert_allclose(gw, w, rtol=1e-12, atol=0)
  assert np.all(gw[:, 0] == 0)
  conn, dd = neighbors.umap_connectivities(idx, dist)
  rconn, rdd = neighbors.assemble_graph(idx, dist, w)
  assert np.array_equal(conn.indices, rconn.indices) and np.allclose(conn.data, rconn.data, rtol=1e-6) and _same_graph(dd, rdd)


@functools.lru_cache(maxsize=None)
def _e2e():
  x = synthetic_8kly(seed=8, n=500, g=300)[0]
  dense = SingleCellOMIC(x).normalize(total=True, log1p=True)
  sparse = SingleCellOMIC(sp.csr_matrix(x)).normalize(total=True, log1p=True)
  return dense, sparse


def test_end_to_end_dense_and_csr():
  dense, sparse = _e2e()
  assert sparse.is_sparse() and not dense.is_sparse()
  X = dense.numpy()
  n, G = X.shape
  sd, ss = dense.dimension_reduce(n_components=20), sparse.dimension_reduce(n_components=20)
  assert sd.shape == (500, 20) and _same_bits(sd, ss)
  md, ms = dense.get_pca(), sparse.get_pca()
  for name in ("mean_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_"):
    assert _same_bits(getattr(md, name), getattr(ms, name)), name
  # the fit within the covariance's bounds: the mean, and (Weyl) every eigenvalue within the spectral norm of the error of S
  rmean, rS = R.pca_cov(X)
  assert np.all(np.abs(md.mean_ - rmean) <= n * U * np.abs(X).max())
  fit = R.pca_fit(X, 20)
  assert np.all(np.abs(md.explained_variance_ - fit["explained_variance"]) <= G * 4 * n * U * np.diag(rS).max())
  # the scores within the projection's bound, for the model's own mean and components
  ulp = _ulp_distance(sd, R.pca_project(X, md.mean_, md.components_))
  print("e2e scores: max ulp", int(ulp.max()), "equal share", float((ulp == 0).mean()))
  assert ulp.max() <= 1 and (ulp == 0).mean() >= 0.99
  assert dense.dimension_reduce(n_components=20) is sd and _same_bits(dense.dimension_reduce(n_components=5), sd[:, :5])
  # the neighbour graph: 300 columns > 100, so the default PCA first; the same bits from the CSR twin
  cd, dd, pd_ = dense.neighbors(n_neighbors=12, n_pcs=30)
  cs, ds, ps = sparse.neighbors(n_neighbors=12, n_pcs=30)
  assert pd_ == ps == {"params": {"n_neighbors": 12, "method": "umap", "metric": "euclidean", "n_pcs": 30,
                                  "use_rep": "transcriptomic_pca"}}
  assert _same_graph(cd, cs) and _same_graph(dd, ds)
  assert cd.dtype == np.float32 and cd.shape == (500, 500) and (cd != cd.T).nnz == 0
  assert np.array_equal(np.diff(dd.indptr), np.full(500, 11))
  rep = dense.dimension_reduce()[:, :30]
  assert rep.shape == (500, 30)
  ridx, rdist, _ = R.knn(rep, 11)
  assert R.knn_gap(rep, 11) > 1e-11
  assert np.array_equal(dd.indices.reshape(500, 11), np.sort(ridx, axis=1))
  again = dense.neighbors(n_neighbors=12, n_pcs=30)
  assert again[0] is cd and again[1] is dd and again[2] is pd_
  twin = dense.copy()
  assert twin.get_pca() is None and not twin._neighbors
  twin.dimension_reduce(n_components=3)
  twin._replace(twin.omics[0], X)
  assert twin.get_pca() is None


def test_latent_space_graph_without_a_container():
  z = np.random.default_rng(13).standard_normal((400, 16)).astype(np.float32)
  conn, dist = neighbors.neighbors(z, n_neighbors=8)
  ridx, rdist, _ = R.knn(z, 7)
  assert np.array_equal(dist.indices.reshape(400, 7), np.sort(ridx, axis=1)) and (conn != conn.T).nnz == 0
  order = np.argsort(ridx, axis=1)
  np.testing.assert_allclose(dist.data.reshape(400, 7), np.take_along_axis(rdist, order, axis=1).astype(np.float32), rtol=1e-6)
  model, scores = neighbors.pca(R.planted_matrix(100, 40, seed=14), 8)
  assert scores.shape == (100, 8) and model.components_.shape == (8, 40) and np.all(np.diff(model.explained_variance_) <= 0)
