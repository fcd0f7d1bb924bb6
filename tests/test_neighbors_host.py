"""CPU-side checks of the neighbour graphs (no device): the NumPy restatement (tests/neighbors_ref.py) against scikit-learn and hand-worked
rows, every refusal (each must fire on the host, before the library is asked for a device), the host assembly of the sparse graphs, and
the container's bookkeeping with the device driver replaced by the restatement."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import sisua_amd
from sisua_amd import _hip, build, engine, neighbors
from sisua_amd.data import SingleCellOMIC
from tests import neighbors_ref as R


@pytest.fixture
def no_device(monkeypatch):
  """a refusal must never reach the library"""
  def boom(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", boom)


@pytest.fixture
def ref_driver(monkeypatch):
  """engine.k_* of the neighbour graphs replaced by the restatement; counts the calls"""
  calls = dict(cov=0, project=0, knn=0, umap=0)

  def dense(x):
    return x.toarray() if sp.issparse(x) else np.asarray(x)

  def cov(x, block_rows=0):
    calls["cov"] += 1
    return R.pca_cov(dense(x))

  def project(x, mean, components, block_rows=0):
    calls["project"] += 1
    return R.pca_project(dense(x), mean, components)

  def knn(Z, k):
    calls["knn"] += 1
    return R.knn(Z, k)[:2]

  def umap(idx, dist):
    calls["umap"] += 1
    return R.umap_rows(idx, dist)

  for name, fn in (("k_pca_cov", cov), ("k_pca_project", project), ("k_knn", knn), ("k_knn_umap", umap)):
    monkeypatch.setattr(engine, name, fn)
  return calls


# ---- the restatement against independent code ----------------------------------------------------------------------------------------
def test_restated_pca_equals_sklearn_full_svd():
  skd = pytest.importorskip("sklearn.decomposition")
  X = R.planted_matrix(400, 60, seed=1)
  fit = R.pca_fit(X, 12)
  sk = skd.PCA(n_components=12, svd_solver="full").fit(X.astype(np.float64))
  print("ev rel", float(np.max(np.abs(fit["explained_variance"] / sk.explained_variance_ - 1))))
  np.testing.assert_allclose(fit["explained_variance"], sk.explained_variance_, rtol=1e-10)
  np.testing.assert_allclose(fit["explained_variance_ratio"], sk.explained_variance_ratio_, rtol=1e-10)
  np.testing.assert_allclose(fit["singular_values"], sk.singular_values_, rtol=1e-10)
  np.testing.assert_allclose(fit["mean"], sk.mean_, rtol=1e-13, atol=1e-13)
  got, want = R.pca_project64(X, fit["mean"], fit["components"]), sk.transform(X.astype(np.float64))
  sign = np.sign((got * want).sum(axis=0))
  err = np.abs(got * sign - want).max(axis=0) / np.abs(want).max(axis=0)
  print("score err / column max", float(err.max()))
  assert err.max() <= 1e-6
  # the sign rule is scikit-learn's svd_flip(u_based_decision=False): the entry of largest magnitude of every component is positive
  assert np.all(fit["components"][np.arange(12), np.argmax(np.abs(fit["components"]), axis=1)] > 0)
  host_comp, host_ev, total = neighbors.components_from_cov(R.pca_cov(X)[1], 12)
  assert np.array_equal(host_comp, fit["components"]) and np.array_equal(host_ev, fit["explained_variance"])
  assert total == np.trace(R.pca_cov(X)[1])


def test_sign_rule_ties_go_to_the_lowest_column():
  assert np.array_equal(R.flip_signs([[-2.0, 2.0, 1.0], [1.0, -3.0, 3.0]]), [[2.0, -2.0, -1.0], [-1.0, 3.0, -3.0]])
  cov = np.array([[1.0, -1.0], [-1.0, 1.0]])   # the leading eigenvector is (1, -1) / sqrt 2 up to sign: |entries| tie
  comp, ev, _ = neighbors.components_from_cov(cov, 2)
  assert comp[0, 0] > 0 and comp[0, 1] < 0 and ev[0] == pytest.approx(2.0) and ev[1] >= 0.0


@pytest.mark.parametrize("shape,k", [((300, 10), 11), ((257, 3), 5), ((64, 1), 3)])
def test_restated_knn_equals_sklearn_brute(shape, k):
  skn = pytest.importorskip("sklearn.neighbors")
  Z = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
  idx, dist, _ = R.knn(Z, k)
  want = skn.NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(Z.astype(np.float64)).kneighbors(Z.astype(np.float64))[0][:, 1:]
  np.testing.assert_allclose(dist, want, rtol=1e-6, atol=1e-7)   # (sklearn's brute force uses the Gram form: it is the less exact one)
  assert np.all(idx != np.arange(shape[0])[:, None]) and np.all(np.diff(dist, axis=1) >= 0)


def test_restated_knn_orders_ties_by_index():
  Z = np.array([[0.0], [1.0], [-1.0], [1.0], [0.0]], np.float32)
  idx, dist, d2 = R.knn(Z, 3)
  assert idx.tolist() == [[4, 1, 2], [3, 0, 4], [0, 4, 1], [1, 0, 4], [0, 1, 2]]
  assert d2.tolist() == [[0, 1, 1], [0, 1, 1], [1, 1, 4], [0, 1, 1], [0, 1, 1]]


def test_umap_rows_by_hand():
  # n_neighbors = 2: target = log2(2) = 1 and the one neighbour sits at rho, so psum = 1 in round 0: sigma stays 1
  idx = np.array([[0, 1], [1, 0], [2, 1]], np.int32)
  dist = np.array([[0.0, 0.5], [0.0, 0.5], [0.0, 2.0]])
  rho, sigma, w = R.umap_rows(idx, dist)
  assert rho.tolist() == [0.5, 0.5, 2.0] and sigma.tolist() == [1.0, 1.0, 1.0] and w.tolist() == [[0.0, 1.0]] * 3
  # ... unless the floor 1e-3 x the row's mean is above 1
  rho, sigma, w = R.umap_rows(idx[:2], np.array([[0.0, 4000.0], [0.0, 4000.0]]))
  assert sigma.tolist() == [2.0, 2.0]
  # an all-duplicates row: rho = 0, psum = K - 1 > log2(K) in every round, sigma halves 64 times and is raised to the GLOBAL floor
  idx = np.array([[0, 1, 2, 3], [1, 0, 2, 3], [2, 0, 1, 3], [3, 4, 0, 1], [4, 3, 0, 1]], np.int32)
  dist = np.array([[0.0, 0, 0, 3.0], [0.0, 0, 0, 3.0], [0.0, 0, 0, 3.0], [0.0, 0, 0, 0], [0.0, 1.0, 3.0, 3.0]])
  rho, sigma, w = R.umap_rows(idx, dist)
  assert rho[3] == 0.0 and sigma[3] == 1e-3 * (dist.sum() / dist.size) and w[3].tolist() == [0.0, 1.0, 1.0, 1.0]
  assert rho[0] == 3.0 and w[0].tolist() == [0.0, 1.0, 1.0, 1.0]   # duplicates in front of the first positive distance
  # a generic row: the weights are exp(-(d - rho) / sigma) and sum to log2(K) within the stop rule
  assert rho[4] == 1.0 and abs(w[4, 1:].sum() - 2.0) < 1e-5 and w[4, 1] == 1.0
  assert w[4, 2] == np.exp(-(2.0 / sigma[4])) and 0 < w[4, 2] < 1


# ---- every refusal, on the host ------------------------------------------------------------------------------------------------------
def test_pca_refusals(no_device):
  wide = sp.csr_matrix((3, 8193), dtype=np.float32)
  with pytest.raises(ValueError, match="filter_highly_variable_genes"):
    neighbors.pca(wide, 10)
  with pytest.raises(ValueError, match="filter_highly_variable_genes"):
    SingleCellOMIC(wide).dimension_reduce()
  with pytest.raises(ValueError, match="filter_highly_variable_genes"):
    engine.k_pca_cov(wide)
  with pytest.raises(ValueError, match="at least 2 cells"):
    neighbors.pca(np.ones((1, 5), np.float32), 2)
  with pytest.raises(ValueError, match="at least 2 cells"):
    engine.k_pca_cov(np.ones((1, 5), np.float32))
  with pytest.raises(ValueError, match="n_components"):
    neighbors.pca(np.ones((4, 5), np.float32), 0)
  with pytest.raises(ValueError):
    engine.k_pca_project(np.ones((4, 5), np.float32), np.zeros(5), np.zeros((129, 5)))
  with pytest.raises(ValueError, match="finite"):
    engine.k_pca_project(np.ones((4, 5), np.float32), np.zeros(5), np.full((2, 5), np.nan))
  om = SingleCellOMIC(np.ones((6, 5), np.float32))
  for algo in ("tsne", "umap"):
    with pytest.raises(NotImplementedError, match="pca"):
      om.dimension_reduce(algo=algo)
  with pytest.raises(ValueError):
    om.dimension_reduce(algo="lda")


def test_knn_refusals(no_device):
  Z = np.random.default_rng(0).standard_normal((6, 3)).astype(np.float32)
  for k in (0, 6, 7, 257):
    with pytest.raises(ValueError, match="k must be"):
      neighbors.knn(Z, k)
    with pytest.raises(ValueError, match="k must be"):
      engine.k_knn(Z, k)
  for bad in (np.nan, np.inf, -np.inf):
    Zb = Z.copy()
    Zb[4, 1] = bad
    with pytest.raises(ValueError, match="not finite"):
      neighbors.knn(Zb, 2)
    with pytest.raises(ValueError, match="not finite"):
      engine.k_knn(Zb, 2)
    with pytest.raises(ValueError, match="not finite"):
      neighbors.neighbors(Zb, 3)
  with pytest.raises(ValueError, match="D <= 128"):
    neighbors.knn(np.zeros((300, 129), np.float32), 2)
  for n_neighbors in (1, 0, 7, 258):
    with pytest.raises(ValueError, match="n_neighbors"):
      neighbors.neighbors(Z, n_neighbors)
    with pytest.raises(ValueError, match="n_neighbors"):
      SingleCellOMIC(Z).neighbors(n_neighbors=n_neighbors)
  with pytest.raises(ValueError):
    engine.k_knn_umap(np.zeros((4, 1), np.int32), np.zeros((4, 1)))
  with pytest.raises(ValueError, match="outside"):
    engine.k_knn_umap(np.full((4, 3), 4, np.int32), np.zeros((4, 3)))
  with pytest.raises(ValueError, match="non-negative"):
    engine.k_knn_umap(np.zeros((4, 3), np.int32), np.full((4, 3), -1.0))


def test_neighbors_unbuilt_options(no_device):
  om = SingleCellOMIC(np.random.default_rng(0).standard_normal((20, 4)).astype(np.float32))
  with pytest.raises(NotImplementedError, match="knn=True"):
    om.neighbors(knn=False)
  for method in ("gauss", "rapids"):
    with pytest.raises(NotImplementedError, match="umap"):
      om.neighbors(method=method)
  for metric in ("cosine", "manhattan", lambda a, b: 0.0):
    with pytest.raises(NotImplementedError, match="euclidean"):
      om.neighbors(metric=metric)


# ---- graph assembly (pure host code) ---------------------------------------------------------------------------------------------------
def test_graph_assembly():
  Z = np.random.default_rng(3).standard_normal((50, 4)).astype(np.float32)
  K = 6
  idx, dist = R.with_self(*R.knn(Z, K - 1)[:2])
  w = R.umap_rows(idx, dist)[2]
  conn, D = neighbors.assemble_graph(idx, dist, w)
  assert conn.dtype == np.float32 and D.dtype == np.float32 and conn.shape == D.shape == (50, 50)
  assert isinstance(conn, sp.csr_matrix) and isinstance(D, sp.csr_matrix)
  assert (conn != conn.T).nnz == 0                        # symmetric
  assert conn.diagonal().max() == 0 and D.diagonal().max() == 0
  assert np.array_equal(np.diff(D.indptr), np.full(50, K - 1))   # no duplicates here: n_neighbors - 1 stored entries per row
  assert (conn.data != 0).all() and (D.data != 0).all()
  A = np.zeros((50, 50))
  A[np.repeat(np.arange(50), K), idx.ravel()] = w.ravel()
  np.testing.assert_array_equal(conn.toarray(), (A + A.T - A * A.T).astype(np.float32))
  assert np.array_equal(D.toarray()[np.arange(50)[:, None], idx[:, 1:]], dist[:, 1:].astype(np.float32))


def test_graph_assembly_duplicate_cells():
  Z = np.random.default_rng(4).standard_normal((30, 3)).astype(np.float32)
  Z[7] = Z[2]   # cells 2 and 7 are duplicates
  idx, dist = R.with_self(*R.knn(Z, 4)[:2])
  w = R.umap_rows(idx, dist)[2]
  conn, D = neighbors.assemble_graph(idx, dist, w)
  assert idx[2, 1] == 7 and idx[7, 1] == 2 and dist[2, 1] == 0 and w[2, 1] == 1
  assert D[2, 7] == 0 and D[7, 2] == 0 and D.getrow(2).nnz == 3   # the duplicate leaves `distances` ...
  assert conn[2, 7] == 1 and conn[7, 2] == 1                       # ... and stays in `connectivities` with weight 1
  with pytest.raises(ValueError):
    neighbors.assemble_graph(idx, dist, w[:, :3])


# ---- the container's bookkeeping, with the restatement as the driver -------------------------------------------------------------------
def test_dimension_reduce_bookkeeping(ref_driver):
  X = R.planted_matrix(80, 30, seed=2)
  om = SingleCellOMIC(X)
  s10 = om.dimension_reduce(n_components=10)
  assert s10.shape == (80, 10) and s10.dtype == np.float32 and ref_driver["cov"] == 1
  model = om.get_pca()
  assert isinstance(model, sisua_amd.PCA) and model.components_.shape == (10, 30) and model.n_samples_seen_ == 80
  for name in ("mean_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_"):
    assert getattr(model, name).dtype == np.float64
  fit = R.pca_fit(X, 10)
  np.testing.assert_array_equal(model.components_, fit["components"])
  np.testing.assert_allclose(model.explained_variance_ratio_, fit["explained_variance_ratio"], rtol=1e-12)
  np.testing.assert_allclose(model.singular_values_, fit["singular_values"], rtol=1e-12)
  assert np.array_equal(model.transform(X), s10)
  s4 = om.dimension_reduce(n_components=4)            # no more components: a column slice of the kept scores
  assert ref_driver["cov"] == 1 and np.array_equal(s4, s10[:, :4])
  assert om.dimension_reduce(n_components=10) is s10
  s20 = om.dimension_reduce(n_components=20)          # more: refits
  assert ref_driver["cov"] == 2 and s20.shape == (80, 20) and om.get_pca() is not model
  assert om.dimension_reduce(n_components=100).shape == (80, 30)   # min(n_components, dim)
  assert om[np.arange(40)].get_pca() is None and om.copy().get_pca() is None
  om._replace(om.omics[0], X * 2)
  assert om.get_pca() is None
  om.dimension_reduce(n_components=3)
  om.add_omic(om.omics[0], X)
  assert om.get_pca() is None


def test_neighbors_bookkeeping(ref_driver):
  X = R.planted_matrix(60, 120, seed=3)   # wider than 100 columns: reduced with PCA first
  om = SingleCellOMIC(X)
  om.add_omic("proteomic", np.random.default_rng(1).standard_normal((60, 7)).astype(np.float32))
  conn, dist, params = om.neighbors(n_neighbors=5, n_pcs=8)
  assert ref_driver == dict(cov=1, project=1, knn=1, umap=1)
  assert params == {"params": {"n_neighbors": 5, "method": "umap", "metric": "euclidean", "n_pcs": 8, "use_rep": "transcriptomic_pca"}}
  assert om.dimension_reduce().shape == (60, 100) and ref_driver["cov"] == 1   # the reference's default PCA was kept
  want = R.knn(om.dimension_reduce()[:, :8], 4)
  assert np.array_equal(np.sort(dist.indices.reshape(60, 4), axis=1), np.sort(want[0], axis=1))
  again = om.neighbors(n_neighbors=5, n_pcs=8)
  assert again[0] is conn and again[1] is dist and again[2] is params and ref_driver["knn"] == 1
  c2, d2, p2 = om.neighbors("proteomic", n_neighbors=12)    # a narrow omic is used as it is
  assert p2["params"]["use_rep"] == "proteomic" and p2["params"]["n_pcs"] == 7 and ref_driver["cov"] == 1
  assert np.array_equal(np.diff(d2.indptr), np.full(60, 11)) and om.neighbors(n_neighbors=5)[0] is conn
  om._replace("proteomic", om.numpy("proteomic") + 1)
  assert "proteomic" not in om._neighbors and om.neighbors()[0] is conn
  assert not om.copy()._neighbors and not om[np.arange(10)]._neighbors


# ---- ABI bookkeeping -------------------------------------------------------------------------------------------------------------------
def test_abi_bookkeeping():
  assert _hip.SMX_ABI_VERSION >= 12 and "smx_pca.hip" in build.SOURCES and "smx_knn.hip" in build.SOURCES
  assert "smx_dist.h" in build.HEADERS and "smx_prep.h" in build.HEADERS   # a change of a shared header rebuilds its users
  header = open(build.HEADERS[-1] if build.HEADERS[-1].startswith("/") else build.os.path.join(build.CSRC, build.HEADERS[-1])).read()
  assert int(re.search(r"#define SMX_ABI_VERSION (\d+)", header).group(1)) == _hip.SMX_ABI_VERSION
  for name in ("smx_pca_cov", "smx_pca_project", "smx_knn", "smx_knn_umap"):
    assert name in _hip.SIGNATURES and re.search(r"\bint %s\(" % name, header)
  assert sisua_amd.PCA is neighbors.PCA
