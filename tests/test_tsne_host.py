"""CPU-side checks of t-SNE (no device): the NumPy restatement (tests/tsne_ref.py) against scikit-learn's private functions on data whose
squared distances are exact in float32, the row whose first sum is 0, every refusal (each must fire on the host, before the library is
asked for a device), the host assembly of P, and the container's bookkeeping with the device driver replaced by the restatement."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import sisua_amd
from sisua_amd import _hip, build, engine, neighbors
from sisua_amd.data import SingleCellOMIC
from tests import neighbors_ref as NR
from tests import tsne_ref as R


@pytest.fixture
def no_device(monkeypatch):
  """a refusal must never reach the library"""
  def boom(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", boom)


@pytest.fixture
def ref_driver(monkeypatch):
  """engine.k_* of the path replaced by the restatements; counts the calls"""
  calls = dict(cov=0, knn=0, affinities=0, fit=0)

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

  def affinities(idx, dist, perplexity):
    calls["affinities"] += 1
    return R.affinity_rows(dist, perplexity)

  def fit(P, Y0, max_iter, ee, lr, mgn, nwp):
    calls["fit"] += 1
    return R.fit(P, Y0, min(max_iter, 3), ee, lr, mgn, nwp)   # (three iterations: the bookkeeping is what is looked at)

  for name, fn in (("k_pca_cov", cov), ("k_pca_project", project), ("k_knn", knn), ("k_tsne_affinities", affinities), ("k_tsne_fit", fit)):
    monkeypatch.setattr(engine, name, fn)
  return calls


def _table(X, perplexity):
  idx, dist, d2 = NR.knn(X, R.support(X.shape[0], perplexity))
  return idx, dist, d2


# ---- the restatement against scikit-learn ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,perplexity", [(60, 5.0), (300, 30.0)])
def test_restated_P_equals_sklearn(n, perplexity):
  ts = pytest.importorskip("sklearn.manifold._t_sne")
  X = R.probe_data(n)
  idx, dist, d2 = _table(X, perplexity)
  assert np.array_equal(d2, d2.astype(np.float32).astype(np.float64))   # scikit-learn's float32 cast loses nothing
  k = idx.shape[1]
  graph = sp.csr_matrix((d2.ravel().copy(), idx.ravel().copy(), np.arange(0, n * k + 1, k)), shape=(n, n))   # (it is sorted in place)
  want = ts._joint_probabilities_nn(graph, perplexity, 0).toarray()
  cond_p, beta, margin = R.affinity_rows(dist, perplexity, margins=True)
  got = R.joint(idx, cond_p)
  print(n, "P max abs", float(np.abs(got.toarray() - want).max()), "branch margin", float(margin.min()))
  assert np.abs(got.toarray() - want).max() <= 1e-12
  assert abs(got.sum() - 1.0) < 1e-12 and (got.data > 0).all() and got.has_sorted_indices
  # the package's host assembly is the restatement's
  mine = neighbors.joint_probabilities(idx, cond_p)
  assert np.array_equal(mine.indptr, got.indptr) and np.array_equal(mine.indices, got.indices)
  np.testing.assert_allclose(mine.data, got.data, rtol=1e-14)
  assert mine.dtype == np.float64 and mine.has_sorted_indices


@pytest.mark.parametrize("n,perplexity", [(60, 5.0), (300, 30.0)])
def test_restated_gradient_equals_sklearn(n, perplexity):
  ts = pytest.importorskip("sklearn.manifold._t_sne")
  from scipy.spatial.distance import squareform
  X = R.probe_data(n)
  idx, dist, _ = _table(X, perplexity)
  P = R.joint(idx, R.affinity_rows(dist, perplexity)[0])
  Pd = P.toarray()
  for scale in (1e-4, 1.0, 20.0):
    Y = np.random.default_rng(3).standard_normal((n, 2)) * scale
    kl_sk, g_sk = ts._kl_divergence(Y.ravel().copy(), squareform(Pd, checks=False), 1.0, n, 2)
    g, kl, Z = R.objective(P, Y)
    err = np.abs(g - g_sk.reshape(n, 2)).max() / np.abs(g_sk).max()
    print(n, scale, "grad rel", float(err), "KL", kl, kl_sk)
    assert err <= 1e-12 and abs(kl - kl_sk) <= 1e-12 * abs(kl_sk)
  # the summation order over j moves the gradient by rounding only
  g2 = R.objective(P, Y, order=np.random.default_rng(0).permutation(n))[0]
  assert np.abs(g2 - g).max() <= 1e-12 * np.abs(g).max()
  # exaggeration scales the attractive part alone
  g12 = R.objective(P, Y, 12.0)[0]
  rep = (g - R.objective(P, Y, 2.0)[0])   # = -4 att
  np.testing.assert_allclose(g12, g - 11.0 * rep, rtol=0, atol=1e-12 * np.abs(g12).max())


def test_restated_update_equals_sklearn():
  ts = pytest.importorskip("sklearn.manifold._t_sne")
  n = 60
  X = R.probe_data(n)
  idx, dist, _ = _table(X, 5.0)
  P = R.joint(idx, R.affinity_rows(dist, 5.0)[0])
  Y0 = np.random.RandomState(1).standard_normal((n, 2)) * 1e-4

  def objective(p, compute_error=True):
    g, kl, _ = R.objective(P, p.reshape(n, 2), 12.0)
    return kl, g.ravel()

  want, _, it = ts._gradient_descent(objective, Y0.ravel().copy(), 0, 20, n_iter_check=50, momentum=0.5, learning_rate=50.0)
  Y, update, gains = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
  for _ in range(20):
    R.descent_step(Y, update, gains, R.objective(P, Y, 12.0)[0], 0.5, 50.0)
  assert it == 19 and np.array_equal(Y.ravel(), want)
  got = R.fit(P, Y0, max_iter=20, learning_rate=50.0)
  assert np.array_equal(got["Y"], Y) and np.array_equal(got["gains"], gains) and np.array_equal(got["update"], update)
  assert got["n_iter"] == 20 and np.isfinite(got["kl_trace"][19]) and np.isnan(got["kl_trace"][:19]).all()


def test_restated_schedule():
  """the two phases: each starts from update = 0 and gains = 1; an early end of the first starts the second; the counters"""
  n = 60
  X = R.probe_data(n)
  idx, dist, _ = _table(X, 5.0)
  P = R.joint(idx, R.affinity_rows(dist, 5.0)[0])
  Y0 = np.random.RandomState(1).standard_normal((n, 2)) * 1e-4
  a = R.fit(P, Y0, max_iter=252, learning_rate=50.0)
  assert a["n_iter"] == 252 and np.flatnonzero(~np.isnan(a["kl_trace"])).tolist() == [49, 99, 149, 199, 249, 251]
  assert set(np.unique(a["gains"])) <= {0.8 + 0.2, 0.8 * 0.8}   # two iterations after the reset: 1 -> 0.8 -> 1 or 0.64
  b = R.fit(P, Y0, max_iter=400, learning_rate=50.0, min_grad_norm=1e30)   # every check stops its phase
  assert b["n_iter"] == 100 and np.flatnonzero(~np.isnan(b["kl_trace"])).tolist() == [49, 99]


def test_zero_sum_row():
  """the data times 1000: every exp(-d2) underflows at beta = 1, the sum is replaced by 1e-8f and the search halves beta from there"""
  ut = pytest.importorskip("sklearn.manifold._utils")
  n, perplexity = 60, 5.0
  X = R.probe_data(n, scale=1000.0)
  idx, _, d2 = _table(X, perplexity)
  d2_32 = d2.astype(np.float32)
  assert (np.exp(-d2_32.astype(np.float64)) == 0).all()
  dist = np.sqrt(d2_32.astype(np.float64))
  cond_p, beta, margin = R.affinity_rows(dist, perplexity, margins=True)
  want = ut._binary_search_perplexity(d2_32, perplexity, 0)
  print("cond_p max abs", float(np.abs(cond_p - want).max()), "beta max", float(beta.max()), "margin", float(margin.min()))
  assert np.abs(cond_p - want).max() <= 1e-9 and (beta < 1e-3).all() and np.isfinite(cond_p).all()
  H = -(cond_p * np.log(np.maximum(cond_p, 1e-300))).sum(axis=1)
  assert np.abs(H - np.log(perplexity)).max() <= 2e-5
  # one round by hand: sum = 0 -> 1e-8f, p = 0, H = log(1e-8f) < target, so beta halves
  one = R.affinity_rows(np.full((4, 3), 1e3), 2.0)
  assert np.isfinite(one[0]).all() and (one[1] < 1.0).all()


# ---- every refusal, on the host ---------------------------------------------------------------------------------------------------------
def test_tsne_refusals(no_device):
  Z = np.random.default_rng(0).standard_normal((40, 3)).astype(np.float32)
  for perplexity in (40, 41, 86, 0.5, np.nan):
    with pytest.raises(ValueError, match="perplexity"):
      neighbors.tsne(Z, perplexity=perplexity)
    with pytest.raises(ValueError, match="perplexity"):
      neighbors.tsne_affinities(Z, perplexity)
  with pytest.raises(ValueError, match="perplexity"):
    neighbors.tsne(np.zeros((300, 3), np.float32), perplexity=85.5)
  with pytest.raises(ValueError, match="at least 4 cells"):
    neighbors.tsne(Z[:3], perplexity=1)
  for C in (0, 4, 100, -1, 2.5):
    with pytest.raises(NotImplementedError, match="at most 3 dimensions"):
      neighbors.tsne(Z, n_components=C, perplexity=5)
    with pytest.raises(NotImplementedError, match="n_components=2.*algo='pca'"):
      SingleCellOMIC(Z).dimension_reduce(algo="tsne", n_components=C)
  with pytest.raises(NotImplementedError, match="at most 3 dimensions"):
    SingleCellOMIC(Z).dimension_reduce(algo="tsne")   # the signature's default of 100 belongs to 'pca'
  with pytest.raises(NotImplementedError, match="at most 3 dimensions"):
    SingleCellOMIC(sp.csr_matrix((3, 9000), dtype=np.float32)).dimension_reduce(algo="tsne")   # ... before anything else is looked at
  with pytest.raises(NotImplementedError, match="pca"):
    SingleCellOMIC(Z).dimension_reduce(algo="umap", n_components=2)
  for bad in (np.nan, np.inf, -np.inf):
    Zb = Z.copy()
    Zb[7, 2] = bad
    with pytest.raises(ValueError, match="not finite"):
      neighbors.tsne(Zb, perplexity=5)
    with pytest.raises(ValueError, match="not finite"):
      neighbors.tsne_affinities(Zb, 5)
  with pytest.raises(ValueError, match="pca"):
    neighbors.tsne(np.zeros((300, 129), np.float32))
  with pytest.raises(ValueError, match="pca"):
    neighbors.tsne_affinities(np.zeros((300, 129), np.float32))
  for init in (np.zeros((40, 3)), np.zeros((39, 2)), np.zeros(80), "spectral"):
    with pytest.raises(ValueError, match="init"):
      neighbors.tsne(Z, perplexity=5, init=init)
  with pytest.raises(ValueError, match="init"):
    neighbors.tsne(Z, perplexity=5, init=np.full((40, 2), np.nan))
  with pytest.raises(ValueError, match="learning_rate"):
    neighbors.tsne(Z, perplexity=5, learning_rate="fast")
  with pytest.raises(ValueError, match="learning_rate"):
    neighbors.tsne(Z, perplexity=5, learning_rate=0.0)
  with pytest.raises(ValueError, match="max_iter"):
    neighbors.tsne(Z, perplexity=5, max_iter=0)


def test_engine_refusals(no_device):
  n = 12
  idx, dist, _ = _table(R.probe_data(n), 2.0)
  P = R.joint(idx, R.affinity_rows(dist, 2.0)[0])
  Y = np.random.default_rng(0).standard_normal((n, 2))
  # affinities
  for perplexity in (0.5, 12, 13, np.nan, np.inf):
    with pytest.raises(ValueError, match="perplexity"):
      engine.k_tsne_affinities(idx, dist, perplexity)
  with pytest.raises(ValueError, match="at least 4 cells"):
    engine.k_tsne_affinities(idx[:3, :2] % 3, dist[:3, :2], 1.0)
  with pytest.raises(ValueError, match="k <= 256"):
    engine.k_tsne_affinities(np.zeros((300, 257), np.int32), np.zeros((300, 257)), 5.0)
  with pytest.raises(ValueError, match="outside"):
    engine.k_tsne_affinities(idx + 6, dist, 2.0)
  with pytest.raises(ValueError, match="non-negative"):
    engine.k_tsne_affinities(idx, -dist, 2.0)
  with pytest.raises(ValueError):
    engine.k_tsne_affinities(idx, dist[:, :3], 2.0)
  # the problem of the gradient and of the descent
  for call in (lambda P_, Y_: engine.k_tsne_gradient(P_, Y_), lambda P_, Y_: engine.k_tsne_fit(P_, Y_, 10)):
    for Yb in (Y[:, :0], np.zeros((n, 4)), Y[:-1], Y.ravel()):
      with pytest.raises(ValueError, match="Y must be"):
        call(P, Yb)
    Yn = Y.copy()
    Yn[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
      call(P, Yn)
    with pytest.raises(ValueError, match="CSR"):
      call(P.toarray(), Y)
    with pytest.raises(ValueError, match="CSR"):
      call(P.tocsc(), Y)
    with pytest.raises(ValueError, match="at least 4 cells"):
      call(sp.csr_matrix(np.full((3, 3), 0.1)), Y[:3])
    unsorted = P.copy()
    lo, hi = unsorted.indptr[2], unsorted.indptr[3]
    unsorted.indices[lo:hi] = unsorted.indices[lo:hi][::-1].copy()
    with pytest.raises(ValueError, match="increase strictly"):
      call(unsorted, Y)
    doubled = P.copy()
    doubled.indices[lo + 1] = doubled.indices[lo]
    with pytest.raises(ValueError, match="increase strictly"):
      call(doubled, Y)
    far = P.copy()
    far.indices[hi - 1] = n
    with pytest.raises(ValueError, match="outside"):
      call(far, Y)
    neg = P.copy()
    neg.indices[0] = -1
    with pytest.raises(ValueError, match="outside"):
      call(neg, Y)
    for v in (0.0, -1e-3, np.nan, np.inf):
      bad = P.copy()
      bad.data[5] = v
      with pytest.raises(ValueError, match="finite and positive"):
        call(bad, Y)
    broken = P.copy()
    broken.indptr[4] = broken.indptr[3] - 1
    with pytest.raises(ValueError, match="indptr"):
      call(broken, Y)
  for e in (0.0, -1.0, np.nan):
    with pytest.raises(ValueError, match="exaggeration"):
      engine.k_tsne_gradient(P, Y, e)
    with pytest.raises(ValueError, match="early_exaggeration"):
      engine.k_tsne_fit(P, Y, 10, early_exaggeration=e)
  for kw in (dict(max_iter=0), dict(n_iter_without_progress=-1)):
    with pytest.raises(ValueError, match="max_iter"):
      engine.k_tsne_fit(P, Y, **kw)
  for kw in (dict(learning_rate=0.0), dict(learning_rate=np.inf), dict(min_grad_norm=-1.0), dict(min_grad_norm=np.nan)):
    with pytest.raises(ValueError, match="learning_rate"):
      engine.k_tsne_fit(P, Y, **kw)


# ---- host pieces ---------------------------------------------------------------------------------------------------------------------------
def test_joint_probabilities_keeps_zeros_out():
  idx = np.array([[1, 2], [0, 2], [3, 0], [2, 1]], np.int32)
  cond = np.array([[0.5, 0.5], [1.0, 0.0], [0.25, 0.75], [0.0, 0.0]])
  P = neighbors.joint_probabilities(idx, cond)
  A = np.zeros((4, 4))
  A[np.repeat(np.arange(4), 2), idx.ravel()] = cond.ravel()
  want = (A + A.T) / (A + A.T).sum()
  np.testing.assert_allclose(P.toarray(), want, rtol=1e-15)
  assert (P.data > 0).all() and P.nnz == np.count_nonzero(want) and P.has_sorted_indices and (P != P.T).nnz == 0
  with pytest.raises(ValueError):
    neighbors.joint_probabilities(idx, cond[:, :1])
  with pytest.raises(ValueError, match="outside"):
    neighbors.joint_probabilities(idx + 2, cond)


def test_init_forms(ref_driver):
  Z = NR.planted_matrix(50, 6, seed=1)
  y = neighbors.tsne_init(Z, 2, "pca")
  fit = NR.pca_fit(Z, 2)
  scores = NR.pca_project(Z, fit["mean"], fit["components"]).astype(np.float64)
  assert y.dtype == np.float64 and np.array_equal(y, scores / np.std(scores[:, 0]) * 1e-4)
  assert np.std(y[:, 0]) == pytest.approx(1e-4)
  assert np.array_equal(neighbors.tsne_init(Z, 3, "random", 7), np.random.RandomState(7).standard_normal((50, 3)) * 1e-4)
  given = np.arange(100.0).reshape(50, 2)
  got = neighbors.tsne_init(Z, 2, given)
  assert np.array_equal(got, given) and got is not given
  one = neighbors.tsne_init(Z[:, :1], 2, "pca")   # fewer columns than components: the rest start at 0
  assert one.shape == (50, 2) and (one[:, 1] == 0).all()
  dup = Z.copy()
  dup[10:20] = dup[3]
  yd = neighbors.tsne_init(dup, 2, "pca")
  assert (yd[10:20] == yd[3]).all()   # duplicated cells start on top of each other


def test_tsne_surface(ref_driver):
  X = R.probe_data(60)
  model = sisua_amd.TSNE(perplexity=5.0, init="random", random_state=3)
  Y = model.fit_transform(X)
  assert Y is model.embedding_ and Y.shape == (60, 2) and Y.dtype == np.float32
  assert model.learning_rate_ == 50.0 and model.n_iter_ == 3 and np.isfinite(model.kl_divergence_)
  assert model.kl_divergence_ == model.kl_trace_[2]
  assert ref_driver == dict(cov=0, knn=1, affinities=1, fit=1)
  assert neighbors.TSNE(perplexity=5.0, learning_rate=120).fit(X).learning_rate_ == 120.0
  assert neighbors.TSNE(perplexity=5.0, early_exaggeration=0.25).fit(X).learning_rate_ == 60.0   # 'auto': max(n / exaggeration / 4, 50)
  P = neighbors.tsne_affinities(X, 5.0)
  idx, dist, _ = _table(X, 5.0)
  want = R.joint(idx, R.affinity_rows(dist, 5.0)[0])
  assert np.array_equal(P.indices, want.indices) and np.allclose(P.data, want.data, rtol=1e-14, atol=0)


def test_dimension_reduce_tsne_bookkeeping(ref_driver):
  X = NR.planted_matrix(40, 120, seed=3)   # wider than 100 columns: reduced with PCA first
  om = SingleCellOMIC(X)
  om.add_omic("proteomic", R.probe_data(40))
  Y = om.dimension_reduce(algo="tsne", n_components=2)
  assert Y.shape == (40, 2) and Y.dtype == np.float32
  assert ref_driver["cov"] == 2 and ref_driver["knn"] == 1 and ref_driver["fit"] == 1   # (covariances: the omic's PCA and the init's)
  assert om.get_pca().components_.shape == (100, 120)   # the reference's default PCA was left behind
  assert om.dimension_reduce(algo="tsne", n_components=2) is Y and ref_driver["fit"] == 1
  Y3 = om.dimension_reduce(algo="tsne", n_components=3)
  assert Y3.shape == (40, 3) and ref_driver["fit"] == 2 and ref_driver["cov"] == 3   # the kept PCA is reused
  Yp = om.dimension_reduce("proteomic", algo="tsne", n_components=1)
  assert Yp.shape == (40, 1) and ref_driver["fit"] == 3
  assert not om.copy()._tsne and not om[np.arange(10)]._tsne
  om._replace("proteomic", om.numpy("proteomic") + 1)
  assert set(om._tsne) == {("transcriptomic", 2), ("transcriptomic", 3)}
  om.add_omic("transcriptomic", X)
  assert not om._tsne


# ---- ABI bookkeeping -------------------------------------------------------------------------------------------------------------------------
def test_abi_bookkeeping():
  assert _hip.SMX_ABI_VERSION >= 13 and "smx_tsne.hip" in build.SOURCES
  header = open(build.os.path.join(build.CSRC, build.HEADERS[-1])).read()
  assert int(re.search(r"#define SMX_ABI_VERSION (\d+)", header).group(1)) == _hip.SMX_ABI_VERSION
  for name in ("smx_tsne_affinities", "smx_tsne_gradient", "smx_tsne_fit"):
    assert name in _hip.SIGNATURES and re.search(r"\bint %s\(" % name, header)
  assert sisua_amd.TSNE is neighbors.TSNE
