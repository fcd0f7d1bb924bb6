"""CPU-side checks of the UMAP layout (no device): the NumPy restatement (tests/umap_ref.py) against rows worked by hand, umap-learn's a
and b, the schedule's counts, every refusal (each must fire on the host, before the library is asked for a device), the container's
bookkeeping with the device driver replaced by the restatement, the ABI's bookkeeping, and the per-epoch form against umap-learn's
literal in-place loop."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import sisua_amd
from sisua_amd import _hip, build, engine, neighbors
from sisua_amd.data import SingleCellOMIC
from tests import neighbors_ref as NR
from tests import umap_ref as R


@pytest.fixture
def no_device(monkeypatch):
  """a refusal must never reach the library"""
  def boom(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", boom)


@pytest.fixture
def ref_driver(monkeypatch):
  """engine.k_* of the path replaced by the restatements; counts the calls"""
  calls = dict(cov=0, knn=0, rows=0, layout=0)

  def dense(x):
    return x.toarray() if sp.issparse(x) else np.asarray(x)

  def cov(x, block_rows=0):
    calls["cov"] += 1
    return NR.pca_cov(dense(x))

  def project(x, mean, components, block_rows=0):
    return NR.pca_project(dense(x), mean, components)

  def knn(Z, k):
    calls["knn"] += 1
    return NR.knn(Z, k)[:2]

  def rows(idx, dist):
    calls["rows"] += 1
    return NR.umap_rows(idx, dist)

  def layout(E, Y0, n_epochs, a, b, gamma=1.0, initial_alpha=1.0, negative_sample_rate=5, seed=0, epoch_begin=0, epoch_end=None,
             next_sample=None, next_negative=None):
    calls["layout"] += 1
    engine._umap_problem(E, Y0)
    return R.layout(E, Y0, n_epochs, a, b, gamma, initial_alpha, negative_sample_rate, seed, epoch_begin, min(n_epochs, 3))   # (three epochs)

  for name, fn in (("k_pca_cov", cov), ("k_pca_project", project), ("k_knn", knn), ("k_knn_umap", rows), ("k_umap_layout", layout)):
    monkeypatch.setattr(engine, name, fn)
  return calls


def _pair_graph(w=1.0):
  return sp.csr_matrix(np.array([[0.0, w], [w, 0.0]]))


def _blob_graph(n_per, K=12):
  X = R.blobs(n_per, sep=4.25)
  idx, dist, _ = NR.knn(X, K - 1)
  tab = neighbors.self_table(idx, dist)
  return X, neighbors.assemble_graph(tab[0], tab[1], NR.umap_rows(*tab)[2])[0]


# ---- the restatement against rows worked by hand ---------------------------------------------------------------------------------------
def test_two_cells_by_hand():
  """a = b = 1, no negatives: d2 = 1, pb = 1, g = (-2 x (1 / 1)) / (1 + 1) = -1; cell 0 has d = -1, term 2 clip(1) = 2; cell 1 the mirror.
  n_epochs = 2: nothing is active in epoch 0 (next = e = 1 > 0); in epoch 1 alpha = 1 - 1/2, so the two cells swap places."""
  E = R.prepare(_pair_graph(), 2)
  assert E.data.tolist() == [1.0, 1.0]
  Y0 = np.array([[0.0], [1.0]])
  nxt, neg = R.start_state(E.data, 0)
  Y = R.epoch(E, Y0, 0, 2, 1.0, 1.0, 1.0, 1.0, 0, 0, nxt, neg)
  assert np.array_equal(Y, Y0) and nxt.tolist() == [1.0, 1.0]
  Y = R.epoch(E, Y, 1, 2, 1.0, 1.0, 1.0, 1.0, 0, 0, nxt, neg)
  assert Y.tolist() == [[1.0], [0.0]] and nxt.tolist() == [2.0, 2.0]
  # far apart in two dimensions, a = 2, b = 0.5: d = (3, 4), d2 = 25, pb = 5, g = ((-2 x 2 x 0.5) x (5 / 25)) / (2 x 5 + 1) = -0.4 / 11
  Y0 = np.array([[0.0, 0.0], [3.0, 4.0]])
  nxt, neg = R.start_state(E.data, 0)
  Y = R.epoch(E, Y0, 1, 4, 2.0, 0.5, 1.0, 1.0, 0, 0, nxt, neg)   # alpha = 3/4
  g = (-2.0 * (5.0 / 25.0)) / 11.0
  np.testing.assert_allclose(Y[0], [0.75 * 2 * g * -3.0, 0.75 * 2 * g * -4.0], rtol=1e-15)
  np.testing.assert_allclose(Y[1], [3.0 + 0.75 * 2 * g * 3.0, 4.0 + 0.75 * 2 * g * 4.0], rtol=1e-15)


def test_negatives_and_both_clips_by_hand():
  """two cells 0.01 apart, one negative per activation (S = 1), gamma = 1, a = b = 1: a negative that draws the other cell has
  g = 2 / ((0.001 + 1e-4) (1e-4 + 1)) ~ 1818 and g d = -+18: clipped to -+4; one that draws the cell itself is skipped.  The
  attraction is 2 clip(g d) with g = -2 / (1e-4 + 1): 2 x 0.02 towards the other cell."""
  E = R.prepare(_pair_graph(), 4)
  Y0 = np.array([[0.0], [0.01]])
  nxt, neg = np.array([1.0, 1.0]), np.array([0.0, 0.0])   # entered at epoch 1 with one negative due: m = trunc((1 - 0) / 1) = 1
  Y, A, T, m, _ = R.epoch(E, Y0, 1, 4, 1.0, 1.0, 1.0, 1.0, 1, 7, nxt, neg, detail=True)
  assert m.tolist() == [1, 1] and nxt.tolist() == [2.0, 2.0] and neg.tolist() == [1.0, 1.0]
  k = R.draws(np.array([0, 1], np.uint64), 1, np.array([0, 0], np.uint64), 7, 2)
  att = 2.0 * ((-2.0 * ((0.01 * 0.01) / (0.01 * 0.01))) / (1.0 * (0.01 * 0.01) + 1.0)) * 0.01   # what cell 1 gets; cell 0 the opposite
  want0 = -att + (0.0 if k[0] == 0 else -4.0)
  want1 = att + (0.0 if k[1] == 1 else 4.0)
  np.testing.assert_allclose(Y[:, 0], [0.0 + 0.75 * want0, 0.01 + 0.75 * want1], rtol=1e-14)
  assert T.tolist() == [2, 2]
  # the attraction: a = 1, b = 0.5, d = 1e-3: pb = 1e-3, g = (-1 x (1e-3 / 1e-6)) / (1e-3 + 1) ~ -1000, g d ~ -+1: inside the clip
  Y0 = np.array([[0.0], [1e-3]])
  nxt, neg = R.start_state(E.data, 0)
  Y = R.epoch(E, Y0, 1, 4, 1.0, 0.5, 1.0, 1.0, 0, 0, nxt, neg)
  g = (-1.0 * (1e-3 / 1e-6)) / (1e-3 + 1.0)
  assert abs(g * 1e-3) < 4.0   # ~ -1: not clipped
  np.testing.assert_allclose(Y[:, 0], [0.75 * 2 * g * -1e-3, 1e-3 + 0.75 * 2 * g * 1e-3], rtol=1e-12)
  Y0 = np.array([[0.0], [1e-9]])   # b = 0.25, d = 1e-9: pb = 10^-4.5, g = -0.5 x 10^13.5 / (1 + pb), g d ~ -+1.6e4: clipped to -+4, doubled
  nxt, neg = R.start_state(E.data, 0)
  Y = R.epoch(E, Y0, 1, 4, 1.0, 0.25, 1.0, 1.0, 0, 0, nxt, neg)
  assert Y[:, 0].tolist() == [0.0 + 0.75 * 8.0, 1e-9 + 0.75 * -8.0]


def test_duplicated_pair_by_hand():
  """two cells on top of each other: d2 == 0, so the attraction is 0 and every negative is skipped -- nothing moves, the schedule does"""
  E = R.prepare(_pair_graph(), 10)
  Y0 = np.array([[2.5, -1.0], [2.5, -1.0]])
  out = R.layout(E, Y0, 10, 1.5, 0.9, S=5, seed=3)
  assert np.array_equal(out["Y"], Y0)
  assert out["next_sample"].tolist() == [10.0, 10.0] and np.allclose(out["next_negative"], 9.0 + np.array([0.0, 0.0]), atol=0.2 + 1e-12)
  nxt, neg, acts, negs = R.state_at(E.data, 5, 10, 10, counts=True)
  assert acts.tolist() == [9, 9] and np.array_equal(nxt, out["next_sample"]) and np.array_equal(neg, out["next_negative"])


def test_entry_active_at_epoch_0_with_no_negative():
  """a state entered by hand: next_sample = 0 makes the entry active in epoch 0; next_negative = 0 gives m = trunc((0 - 0) / e_neg) = 0"""
  E = R.prepare(_pair_graph(), 5)
  Y0 = np.array([[0.0], [1.0]])
  nxt, neg = np.zeros(2), np.zeros(2)
  Y, A, T, m, _ = R.epoch(E, Y0, 0, 5, 1.0, 1.0, 1.0, 1.0, 5, 0, nxt, neg, detail=True)
  assert m.tolist() == [0, 0] and T.tolist() == [1, 1] and nxt.tolist() == [1.0, 1.0] and neg.tolist() == [0.0, 0.0]
  assert Y.tolist() == [[2.0], [-1.0]]   # alpha_0 = 1: the attraction's 2 x clip(1) alone
  # the clamp: a stale next_negative bounds m by S x n_epochs
  nxt, neg = np.zeros(2), np.full(2, -1e30)
  m = R.epoch(E, Y0, 0, 5, 1.0, 1.0, 1.0, 1.0, 5, 0, nxt, neg, detail=True)[3]
  assert m.tolist() == [25, 25]


def test_ab_values():
  a, b = neighbors.find_ab_params(1.0, 0.5)
  assert abs(a - 0.58303) <= 1e-3 and abs(b - 1.33417) <= 1e-3
  a, b = neighbors.find_ab_params(1.0, 0.1)
  assert abs(a - 1.577) <= 1e-3 and abs(b - 0.895) <= 1e-3


def test_schedule_counts():
  """over a run an entry of weight w is active floor(n_epochs w / max) times within 1.  Its negatives keep pace with the epochs, not with
  the activations (next_negative is brought up to the epoch at every activation), so an activation draws S of them and the run S x
  activations within one activation's worth (S).  For an entry of the largest weight (e = 1) that is S x n_epochs, short of it by the
  epoch 0 in which nothing is active (S) and by the first activation's S - 1 (1)."""
  rng = np.random.default_rng(0)
  w = np.concatenate([[1.0, 1.0], rng.uniform(0.002, 1.0, 400)])
  for n_epochs, S in ((200, 5), (500, 5), (37, 1), (200, 64)):
    keep = w >= w.max() / n_epochs
    eps = w.max() / w[keep]
    _, _, acts, negs = R.state_at(eps, S, n_epochs, n_epochs, counts=True)
    assert np.abs(acts - np.floor(n_epochs * w[keep] / w.max())).max() <= 1
    assert np.abs(negs - S * acts).max() <= S
    assert abs(negs[0] - S * n_epochs) <= S + 1 and acts[0] == n_epochs - 1   # the largest weight: every epoch but epoch 0


def test_prepare_and_normalise():
  X, conn = _blob_graph(20)
  for n_epochs in (10, 200):
    G = neighbors.umap_prepare_graph(conn, n_epochs)
    want = R.prepare(conn, n_epochs)
    assert G.format == "csr" and G.dtype == np.float64 and G.has_sorted_indices and (G != G.T).nnz == 0
    assert np.array_equal(G.indptr, want.indptr) and np.array_equal(G.indices, want.indices) and np.array_equal(G.data, want.data)
    assert G.data.min() == 1.0 and G.data.max() <= n_epochs
  assert neighbors.umap_prepare_graph(conn, 10).nnz < neighbors.umap_prepare_graph(conn, 200).nnz < conn.nnz + 1
  lonely = sp.lil_matrix((4, 4))
  lonely[0, 1] = lonely[1, 0] = 1.0
  lonely[2, 3] = lonely[3, 2] = 1e-3   # below 1 / 500
  G = neighbors.umap_prepare_graph(lonely.tocsr(), 500)
  assert np.diff(G.indptr).tolist() == [1, 1, 0, 0]
  assert neighbors.umap_n_epochs(10000) == 500 and neighbors.umap_n_epochs(10001) == 200 and neighbors.umap_n_epochs(5, 7) == 7
  Y0 = np.array([[1.0, 3.0, -2.0], [3.0, 3.0, 0.0], [2.0, 3.0, 2.0]])
  assert neighbors.umap_normalise(Y0).tolist() == [[0.0, 5.0, 0.0], [10.0, 5.0, 5.0], [5.0, 5.0, 10.0]]
  assert np.array_equal(neighbors.umap_normalise(Y0), R.normalise(Y0))
  assert np.array_equal(neighbors.umap_init(6, 2, "random", 7), np.random.RandomState(7).uniform(-10, 10, (6, 2)))


# ---- every refusal, on the host ---------------------------------------------------------------------------------------------------------
def test_umap_refusals(no_device):
  X, conn = _blob_graph(10)
  for C in (0, 4, 100, -1, 2.5):
    with pytest.raises(NotImplementedError, match="at most 3 dimensions"):
      neighbors.umap_layout(conn, n_components=C)
    with pytest.raises(NotImplementedError, match="at most 3 dimensions"):
      neighbors.umap(X, n_components=C)
    with pytest.raises(NotImplementedError, match="at most 3 dimensions"):
      SingleCellOMIC(X).umap(n_components=C)
  for init in ("spectral",):
    with pytest.raises(NotImplementedError, match="'pca'"):
      neighbors.umap_layout(conn, init=init)
    with pytest.raises(NotImplementedError, match="'pca'"):
      neighbors.umap(X, init=init)
  with pytest.raises(ValueError, match="needs the cells"):
    neighbors.umap_layout(conn, init="pca")
  for init in ("laplace", np.zeros((30, 3)), np.zeros((29, 2)), np.full((30, 2), np.nan)):
    with pytest.raises(ValueError, match="init"):
      neighbors.umap_layout(conn, init=init)
    with pytest.raises(ValueError, match="init"):
      neighbors.umap(X, init=init)
  for n_epochs in (0, 10001, -3, 2.5):
    with pytest.raises(ValueError, match="n_epochs"):
      neighbors.umap_layout(conn, n_epochs=n_epochs)
    with pytest.raises(ValueError, match="n_epochs"):
      SingleCellOMIC(X).umap(n_epochs=n_epochs)
  for S in (-1, 65, 2.5):
    with pytest.raises(ValueError, match="negative_sample_rate"):
      neighbors.umap_layout(conn, negative_sample_rate=S)
  for alpha in (0.0, -1.0, np.nan, np.inf):
    with pytest.raises(ValueError, match="alpha"):
      neighbors.umap_layout(conn, alpha=alpha)
  for gamma in (-1.0, np.nan, np.inf):
    with pytest.raises(ValueError, match="gamma"):
      neighbors.umap_layout(conn, gamma=gamma)
  for kw in (dict(spread=0.0), dict(spread=np.nan), dict(min_dist=-0.1), dict(min_dist=2.0), dict(min_dist=np.nan)):
    with pytest.raises(ValueError, match="min_dist"):
      neighbors.umap_layout(conn, **kw)
    with pytest.raises(ValueError, match="min_dist"):
      SingleCellOMIC(X).umap(**kw)
  for rs in (-1, 2 ** 32, 1.5, None):
    with pytest.raises(ValueError, match="random_state"):
      neighbors.umap_layout(conn, random_state=rs)
  # the graph
  with pytest.raises(ValueError, match="square scipy.sparse"):
    neighbors.umap_layout(conn.toarray())
  with pytest.raises(ValueError, match="square scipy.sparse"):
    neighbors.umap_layout(conn[:, :20])
  with pytest.raises(ValueError, match="2 .. 2\\^31 - 1 cells"):
    neighbors.umap_layout(sp.csr_matrix((1, 1)))
  oneway = conn.tolil()
  oneway[0, oneway.rows[0][0]] = 0.123
  with pytest.raises(ValueError, match="not symmetric"):
    neighbors.umap_layout(oneway.tocsr())
  for v in (-0.5, np.nan, np.inf):
    bad = conn.astype(np.float64)
    bad.data[3] = v
    with pytest.raises(ValueError, match="finite and not negative"):
      neighbors.umap_layout(bad)
  with pytest.raises(ValueError, match="diagonal"):
    neighbors.umap_layout((conn + sp.identity(30, format="csr")).tocsr())
  # the cells
  with pytest.raises(ValueError, match="pca"):
    neighbors.umap(np.zeros((300, 129), np.float32))
  Xb = X.copy()
  Xb[7, 2] = np.nan
  with pytest.raises(ValueError, match="not finite"):
    neighbors.umap(Xb)
  for k in (1, 31, 258):
    with pytest.raises(ValueError, match="n_neighbors"):
      neighbors.umap(X, n_neighbors=k)
  with pytest.raises(ValueError, match="not one of the omics"):
    SingleCellOMIC(X).umap("proteomic")


def test_engine_refusals(no_device):
  _, conn = _blob_graph(10)
  E = R.prepare(conn, 50)
  n = 30
  Y = np.random.default_rng(0).standard_normal((n, 2))
  a, b = 0.58, 1.33

  def call(E_=E, Y_=Y, n_epochs=50, **kw):
    return engine.k_umap_layout(E_, Y_, n_epochs, kw.pop("a", a), kw.pop("b", b), **kw)

  for Yb in (Y[:, :0], np.zeros((n, 4)), Y[:-1], Y.ravel()):
    with pytest.raises(ValueError, match="Y must be"):
      call(Y_=Yb)
  Yn = Y.copy()
  Yn[3, 1] = np.inf
  with pytest.raises(ValueError, match="not finite"):
    call(Y_=Yn)
  with pytest.raises(ValueError, match="CSR"):
    call(E_=E.toarray())
  with pytest.raises(ValueError, match="CSR"):
    call(E_=E.tocsc())
  with pytest.raises(ValueError, match="2 .. 2\\^31 - 1 cells"):
    call(E_=sp.csr_matrix((1, 1)), Y_=Y[:1])
  lo, hi = E.indptr[2], E.indptr[3]
  unsorted = E.copy()
  unsorted.indices[lo:hi] = unsorted.indices[lo:hi][::-1].copy()
  with pytest.raises(ValueError, match="increase strictly"):
    call(E_=unsorted)
  far = E.copy()
  far.indices[hi - 1] = n
  with pytest.raises(ValueError, match="outside"):
    call(E_=far)
  diag = sp.csr_matrix(np.array([[1.0, 2.0], [2.0, 0.0]]))
  with pytest.raises(ValueError, match="diagonal"):
    call(E_=diag, Y_=Y[:2])
  for v in (0.0, -1.0, np.nan, np.inf):
    bad = E.copy()
    bad.data[5] = v
    with pytest.raises(ValueError, match="finite and positive"):
      call(E_=bad)
  lop = E.copy()
  lop.data[0] = lop.data[0] + 1.0
  with pytest.raises(ValueError, match="not symmetric"):
    call(E_=lop)
  broken = E.copy()
  broken.indptr[4] = broken.indptr[3] - 1
  with pytest.raises(ValueError, match="indptr"):
    call(E_=broken)
  for n_epochs in (0, 10001):
    with pytest.raises(ValueError, match="n_epochs"):
      call(n_epochs=n_epochs)
  for kw in (dict(epoch_begin=-1), dict(epoch_begin=3, epoch_end=2), dict(epoch_end=51)):
    with pytest.raises(ValueError, match="epoch_begin"):
      call(**kw)
  for S in (-1, 65):
    with pytest.raises(ValueError, match="negative_sample_rate"):
      call(negative_sample_rate=S)
  for kw in (dict(a=-1.0), dict(b=np.nan), dict(gamma=np.inf), dict(gamma=-0.5)):
    with pytest.raises(ValueError, match="a, b and gamma"):
      call(**kw)
  with pytest.raises(ValueError, match="initial_alpha"):
    call(initial_alpha=np.nan)
  for seed in (-1, 2 ** 64):
    with pytest.raises(ValueError, match="seed"):
      call(seed=seed)
  with pytest.raises(ValueError, match="come together"):
    call(next_sample=E.data)
  with pytest.raises(ValueError, match="one per entry"):
    call(next_sample=E.data[:-1], next_negative=E.data)
  with pytest.raises(ValueError, match="must be finite"):
    call(next_sample=E.data, next_negative=np.full(E.nnz, np.nan))
  with pytest.raises(ValueError):
    engine.k_umap_pow(np.array([1.0, -1.0]), 1.3)


# ---- the surface and the container's bookkeeping ------------------------------------------------------------------------------------------
def test_umap_surface(ref_driver):
  X = R.blobs(20, sep=4.25)
  model = sisua_amd.UMAP(n_neighbors=5, n_epochs=40, random_state=3)
  Y = model.fit_transform(X)
  assert Y is model.embedding_ and Y.shape == (60, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
  assert model.n_epochs_ == 40 and (model.a_, model.b_) == neighbors.find_ab_params(1.0, 0.5)
  assert sp.issparse(model.graph_) and model.graph_.shape == (60, 60) and model.graph_.dtype == np.float32
  assert ref_driver == dict(cov=1, knn=1, rows=1, layout=1)
  assert sisua_amd.UMAP(n_neighbors=5, init="random").fit(X).n_epochs_ == 500 and ref_driver["cov"] == 1
  Y3, info = neighbors.umap_layout(model.graph_, 3, n_epochs=9, init=np.arange(180.0).reshape(60, 3), return_info=True)
  assert Y3.shape == (60, 3) and info["n_epochs"] == 9 and info["graph"].dtype == np.float64 and info["init"].min() == 0.0 and info["init"].max() == 10.0
  assert sisua_amd.umap(X, n_neighbors=5, n_components=1, init="random").shape == (60, 1)
  # the start handed to the driver is the normalised PCA init
  seen = {}
  real = engine.k_umap_layout

  def spy(E, Y0, *a, **k):
    seen["Y0"], seen["E"] = Y0, E
    return real(E, Y0, *a, **k)

  engine.k_umap_layout = spy   # (ref_driver's monkeypatch restores the attribute)
  neighbors.umap(X, n_neighbors=5, n_epochs=4)
  fit = NR.pca_fit(X, 2)
  assert np.array_equal(seen["Y0"], R.normalise(NR.pca_project(X, fit["mean"], fit["components"])))
  assert np.array_equal(seen["E"].data, R.prepare(model.graph_, 4).data)


def test_singlecell_umap_bookkeeping(ref_driver):
  X = NR.planted_matrix(40, 120, seed=3)   # wider than 100 columns: reduced with PCA first
  om = SingleCellOMIC(X)
  om.add_omic("proteomic", R.blobs(14, sep=4.25)[:40])
  Y = om.umap()
  assert Y.shape == (40, 2) and Y.dtype == np.float32
  assert ref_driver["knn"] == 1 and ref_driver["rows"] == 1 and ref_driver["layout"] == 1
  assert ref_driver["cov"] == 2   # (the omic's PCA-100, kept, and the init's PCA of its scores)
  assert om.get_pca().components_.shape == (100, 120)
  graph = om.neighbors()[0]
  assert om.umap() is Y and om.umap(min_dist=0.1, n_epochs=3) is Y and ref_driver["layout"] == 1
  Y3 = om.umap(n_components=3)
  assert Y3.shape == (40, 3) and ref_driver["layout"] == 2 and ref_driver["knn"] == 1 and ref_driver["cov"] == 3   # the kept graph and PCA are reused
  assert om.neighbors()[0] is graph
  Yp = om.umap("proteomic", n_components=1)
  assert Yp.shape == (40, 1) and ref_driver["layout"] == 3 and ref_driver["knn"] == 2
  assert not om.copy()._umap and not om[np.arange(10)]._umap
  om._replace("proteomic", om.numpy("proteomic") + 1)
  assert set(om._umap) == {("transcriptomic", 2), ("transcriptomic", 3)}
  om.add_omic("transcriptomic", X)
  assert not om._umap
  # the two pinned refusals still raise, and point here
  with pytest.raises(NotImplementedError, match="pca") as e:
    om.dimension_reduce(algo="umap", n_components=2)
  assert "SingleCellOMIC.umap" in str(e.value)
  with pytest.raises(NotImplementedError, match="'kmeans', 'pca' and 'tsne'") as e:
    om.clustering(n_clusters=4, algo="umap")
  assert "SingleCellOMIC.umap" in str(e.value)


# ---- ABI bookkeeping -------------------------------------------------------------------------------------------------------------------------
def test_abi_bookkeeping():
  assert _hip.SMX_ABI_VERSION >= 20 and "smx_umap.hip" in build.SOURCES
  header = open(build.os.path.join(build.CSRC, build.HEADERS[-1])).read()
  assert int(re.search(r"#define SMX_ABI_VERSION (\d+)", header).group(1)) == _hip.SMX_ABI_VERSION
  for name in ("smx_umap_layout", "smx_umap_pow"):
    assert name in _hip.SIGNATURES and re.search(r"\bint %s\(" % name, header)
  decl = re.search(r"\bint smx_umap_layout\(([^;]*)\);", header).group(1)
  assert len(decl.split(",")) == len(_hip.SIGNATURES["smx_umap_layout"][1]) == 18
  source = open(build.os.path.join(build.CSRC, "smx_umap.hip")).read()
  assert "ST_UMAP_NEG = %d" % R.ST_UMAP_NEG in source and "stream id %d" % R.ST_UMAP_NEG in header
  assert sisua_amd.UMAP is neighbors.UMAP and sisua_amd.umap is neighbors.umap
  assert engine.k_umap_layout.__module__ == "sisua_amd.engine._neighbors"


# ---- the per-epoch form against the literal in-place loop ---------------------------------------------------------------------------------
def test_per_epoch_form_against_sequential():
  """3 x 100 Gaussian cells in 10 dimensions, the groups 6 apart, K = 12, 200 epochs, min_dist = 0.5, PCA start.  Measured here:
  trustworthiness 0.9218 (per-epoch) against 0.9242 (sequential); the issue's twelve runs had the per-epoch form at most 0.0076 below."""
  skm = pytest.importorskip("sklearn.manifold")
  X, conn = _blob_graph(100)
  group = np.arange(300) % 3
  E = R.prepare(conn, 200)
  a, b = neighbors.find_ab_params(1.0, 0.5)
  fit = NR.pca_fit(X, 2)
  Y0 = R.normalise(NR.pca_project(X, fit["mean"], fit["components"]))
  per_epoch = R.layout(E, Y0, 200, a, b, seed=1)["Y"]
  sequential = R.layout_sequential(E, Y0, 200, a, b, seed=1)
  t_pe, t_seq = skm.trustworthiness(X, per_epoch, n_neighbors=12), skm.trustworthiness(X, sequential, n_neighbors=12)
  print("trustworthiness: per-epoch", t_pe, "sequential", t_seq)
  assert np.isfinite(per_epoch).all() and np.isfinite(sequential).all()
  assert t_pe >= t_seq - 0.02
  assert R.nearest_in_group(per_epoch, group) and R.nearest_in_group(sequential, group)
