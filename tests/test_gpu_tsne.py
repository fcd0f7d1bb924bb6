"""t-SNE on the device (smx_tsne.hip through engine.k_tsne_affinities / k_tsne_gradient / k_tsne_fit, sisua_amd/neighbors.py and
SingleCellOMIC.dimension_reduce(algo='tsne')) against the float64 restatement tests/tsne_ref.py.

Shapes are the smallest at which the kernels can still go wrong: cells around the LDS tile of 128 and the workgroup of 256, more than one
workgroup, k = n - 1 and k = 256, one slice of the j range and as many as the library takes (32).

Bounds.
  affinities   the search is a sequence of branches on H - target; a row is GUARDED when the restatement's own margin min(||H - target| -
               tol|, |H - target| where the side is looked at) over its rounds passes 1e-10 (the device's exp and log move H by ~1e-15).
               On guarded rows beta is EQUAL and cond_p is within 1e-12 relative (absolute 1e-300: a relative bound has no meaning among
               subnormals).  The guard may leave out at most 1 % of a case's rows.
  gradient     |d grad_ic| <= (4 n + 32) 2^-53 A_ic, A_ic = 4 (sum_j |attractive term| + sum_j |repulsive term| / Z): six roundings per
               term, a chain of n terms, the relative error of Z.  Z to 2 n 2^-53 relative; KL to (4 n + 32) 2^-53 sum p |log(p Z / w)|.
  trajectory   the dynamics are chaotic, so the tolerance is a measurement: the restatement run with the sums over j in three orders
               (ascending, descending, a random permutation) on exactly these inputs differs, relative to max |Y|, by
                   n = 60:  2.3e-16 after 1 iteration, 3.4e-14 after 10        n = 300:  3.3e-16 after 1, 2.3e-15 after 10
               (update alike; gains: equal).  The tolerance is 100 x that: 2.3e-14, 3.4e-12, 3.3e-14, 2.3e-13, for Y, update and gains
               each relative to its own largest magnitude.  The margin is for the device's exp, log and division.
  whole runs   judged by what they are for: a finite trace, a KL that falls after the exaggeration ends, every cell's nearest neighbour
               in the embedding in its own group, and a trustworthiness no more than 0.02 below that of scikit-learn's own
               TSNE(method='exact') from the same start.  The data are the probe's with the groups 24 apart instead of 8: at 8 the
               groups' boxes [-6, 6] + 8 g overlap and three cells of the 300 have their nearest neighbour IN THE INPUT in another
               group (scikit-learn's exact embedding and the restatement's each show six such cells), so the check would ask the
               embedding for something the data do not have; at 24 the boxes are 12 apart in every coordinate (>= 26.8 between
               groups, above every within-group nearest-neighbour distance)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from sisua_amd import _hip, engine, neighbors
from sisua_amd.data import SingleCellOMIC
from tests import neighbors_ref as NR
from tests import tsne_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
AFF_N = [4, 5, 255, 256, 257, 600]
AFF_PERPLEXITY = [2.0, 5.0, 30.0, 85.0]
AFF_DATA = ["integer", "gauss", "x1000", "duplicates"]
GRAD_N = [4, 5, 63, 64, 65, 255, 256, 257, 600]
GRAD_SCALE = [1e-4, 1.0, 50.0]
MAX_SLICES = 32
SPREAD = {(60, 1): 2.3e-16, (60, 10): 3.4e-14, (300, 1): 3.3e-16, (300, 10): 2.3e-15}   # the restatement's order-to-order spread (CPU)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _cells(kind, n):
  """float32 [n, 5], never written to"""
  if kind == "integer":
    x = R.probe_data(n)
  elif kind == "x1000":
    x = R.probe_data(n, scale=1000.0)
  elif kind == "gauss":
    x = np.random.default_rng(n).standard_normal((n, 5)).astype(np.float32)
  else:   # a block of min(20, n - 1) duplicated cells
    x = R.probe_data(n).copy()
    x[1:min(21, n)] = x[0]
  x.setflags(write=False)
  return x


@functools.lru_cache(maxsize=None)
def _table(kind, n, k):
  idx, dist, _ = NR.knn(_cells(kind, n), k)
  return idx, dist


@functools.lru_cache(maxsize=None)
def _joint(n, perplexity):
  """the restatement's P of the probe data"""
  idx, dist = _table("integer", n, R.support(n, perplexity))
  return R.joint(idx, R.affinity_rows(dist, perplexity)[0])


@pytest.fixture
def slices():
  def set_(s):
    _hip.clear_tuning("tsne_slices") if s is None else _hip.set_tuning("tsne_slices", s)
  yield set_
  _hip.clear_tuning("tsne_slices")


# ---- affinities ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", AFF_DATA)
@pytest.mark.parametrize("n,perplexity", [(n, p) for n in AFF_N for p in AFF_PERPLEXITY if p < n])
def test_affinities_against_restatement(n, perplexity, kind):
  k = R.support(n, perplexity)
  idx, dist = _table(kind, n, k)
  want_p, want_beta, margin = R.affinity_rows(dist, perplexity, margins=True)
  cond_p, beta = engine.k_tsne_affinities(idx, dist, perplexity)
  assert cond_p.shape == (n, k) and cond_p.dtype == np.float64 and beta.shape == (n,)
  guarded = margin > 1e-10
  left_out = int((~guarded).sum())
  rel = np.abs(cond_p - want_p)[guarded] / np.maximum(want_p[guarded], 1e-300)
  print(n, perplexity, kind, "k", k, "left out", left_out, "cond_p rel", float(rel.max()), "beta equal", bool(np.array_equal(beta[guarded], want_beta[guarded])))
  assert left_out <= 0.01 * n
  assert np.array_equal(beta[guarded], want_beta[guarded])
  np.testing.assert_allclose(cond_p[guarded], want_p[guarded], rtol=1e-12, atol=1e-300)
  assert np.isfinite(cond_p).all() and (cond_p >= 0).all()


def test_affinities_surface_and_slices(slices):
  """tsne_affinities: the device's kNN table and rows, the host assembly; the same bits from call to call and for every slice knob"""
  Z = _cells("integer", 300)
  P = neighbors.tsne_affinities(Z, 30.0)
  want = _joint(300, 30.0)
  assert sp.issparse(P) and P.format == "csr" and P.dtype == np.float64 and P.has_sorted_indices
  assert np.array_equal(P.indptr, want.indptr) and np.array_equal(P.indices, want.indices)
  np.testing.assert_allclose(P.data, want.data, rtol=1e-11)
  for knob in ("tsne_slices", "knn_slices"):
    try:
      _hip.set_tuning(knob, 1)
      Q = neighbors.tsne_affinities(Z, 30.0)
    finally:
      _hip.clear_tuning(knob)
    assert np.array_equal(Q.indptr, P.indptr) and np.array_equal(Q.indices, P.indices) and _same_bits(Q.data, P.data)


# ---- the gradient, elementwise ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grad_problem(n):
  return _joint(n, 2.0 if n < 10 else min(30.0, (n - 1) / 3.0))


@functools.lru_cache(maxsize=None)
def _grad_reference(n, C, e, scale):
  Y = np.random.default_rng(100 * n + C).standard_normal((n, C)) * scale
  Y.setflags(write=False)
  return (Y,) + R.objective(_grad_problem(n), Y, e, bounds=True)


@pytest.mark.parametrize("n_slices", [1, MAX_SLICES])
@pytest.mark.parametrize("scale", GRAD_SCALE)
@pytest.mark.parametrize("e", [1.0, 12.0])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("n", GRAD_N)
def test_gradient_against_restatement(n, C, e, scale, n_slices, slices):
  Y, want, want_kl, want_Z, A, B = _grad_reference(n, C, e, scale)
  slices(n_slices)
  grad, kl, Z = engine.k_tsne_gradient(_grad_problem(n), Y, e)
  assert grad.shape == (n, C) and grad.dtype == np.float64
  bound = (4 * n + 32) * U
  with np.errstate(invalid="ignore", divide="ignore"):
    frac = np.where(A > 0, np.abs(grad - want) / (bound * A), np.where(grad == want, 0.0, np.inf))
  print(n, C, e, scale, n_slices, "grad err / bound", float(frac.max()), "Z", abs(Z - want_Z) / (2 * n * U * want_Z),
        "KL", abs(kl - want_kl) / (bound * B))
  assert frac.max() <= 1.0
  assert abs(Z - want_Z) <= 2 * n * U * want_Z
  assert abs(kl - want_kl) <= bound * B


def test_gradient_same_bits_twice(slices):
  Y, *_ = _grad_reference(600, 2, 12.0, 1.0)
  a, b = engine.k_tsne_gradient(_grad_problem(600), Y, 12.0), engine.k_tsne_gradient(_grad_problem(600), Y, 12.0)
  assert _same_bits(a[0], b[0]) and a[1:] == b[1:]


# ---- a short trajectory ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 10])
@pytest.mark.parametrize("n,perplexity", [(60, 5.0), (300, 30.0)])
def test_short_trajectory(n, perplexity, max_iter):
  P = _joint(n, perplexity)
  Y0 = np.random.RandomState(1).standard_normal((n, 2)) * 1e-4
  lr = max(n / 12.0 / 4.0, 50.0)
  want = R.fit(P, Y0, max_iter=max_iter, learning_rate=lr)
  got = engine.k_tsne_fit(P, Y0, max_iter=max_iter, learning_rate=lr)
  tol = 100.0 * SPREAD[(n, max_iter)]
  assert got["n_iter"] == want["n_iter"] == max_iter
  for q in ("Y", "update", "gains"):
    err = np.abs(got[q] - want[q]).max() / np.abs(want[q]).max()
    print(n, max_iter, q, "err", float(err), "tolerance", tol)
    assert err <= tol, q
  assert np.array_equal(np.isnan(got["kl_trace"]), np.isnan(want["kl_trace"]))
  np.testing.assert_allclose(got["kl_trace"][max_iter - 1], want["kl_trace"][max_iter - 1], rtol=1e-11)


# ---- whole runs --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _whole_run():
  X = R.probe_data(300, offset=24.0)
  Y0 = np.random.RandomState(1).standard_normal((300, 2)) * 1e-4
  model = neighbors.TSNE(perplexity=30.0, max_iter=500, init=Y0)
  return X, Y0, model, model.fit_transform(X)


def test_whole_run_embeds_the_groups():
  skm = pytest.importorskip("sklearn.manifold")
  X, Y0, model, Y = _whole_run()
  trace = model.kl_trace_
  reported = np.flatnonzero(~np.isnan(trace))
  assert Y.shape == (300, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
  assert reported.tolist() == list(range(49, 500, 50)) and np.isfinite(trace[reported]).all()
  assert model.n_iter_ == 500 and model.kl_divergence_ == trace[499] and model.learning_rate_ == 50.0
  assert trace[499] < trace[249]
  group = np.arange(300) % 3
  d2 = NR.sq_distances(Y)
  np.fill_diagonal(d2, np.inf)
  assert np.array_equal(group[np.argmin(d2, axis=1)], group)
  ref = skm.TSNE(n_components=2, perplexity=30.0, method="exact", init=Y0.astype(np.float32), max_iter=500, learning_rate="auto").fit_transform(
      X.astype(np.float64))
  mine, theirs = skm.trustworthiness(X, Y, n_neighbors=12), skm.trustworthiness(X, ref, n_neighbors=12)
  print("trustworthiness: device", mine, "scikit-learn exact", theirs, "KL", trace[reported].tolist())
  assert mine >= theirs - 0.02


def test_whole_run_same_bits_twice():
  X, Y0, model, Y = _whole_run()
  again = neighbors.TSNE(perplexity=30.0, max_iter=500, init=Y0)
  assert _same_bits(again.fit_transform(X), Y) and _same_bits(again.kl_trace_, model.kl_trace_)


def test_early_stop_on_grad_norm():
  """a min_grad_norm that every check passes: the first phase ends at iteration 50, the second (from the next iteration, as in scikit-learn) at 100"""
  X, Y0, _, _ = _whole_run()
  model = neighbors.TSNE(perplexity=30.0, max_iter=500, init=Y0, min_grad_norm=1e30)
  model.fit_transform(X)
  assert model.n_iter_ == 100 and np.flatnonzero(~np.isnan(model.kl_trace_)).tolist() == [49, 99]
  assert model.kl_divergence_ == model.kl_trace_[99] and np.isfinite(model.kl_divergence_)
  short = neighbors.TSNE(perplexity=30.0, max_iter=7, init="random", random_state=4)
  assert short.fit_transform(X).shape == (300, 2) and short.n_iter_ == 7 and short.kl_divergence_ == short.kl_trace_[6]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def test_dimension_reduce_tsne_end_to_end():
  rng = np.random.default_rng(11)
  counts = rng.poisson(rng.gamma(0.6, 2.0, size=(1, 300)) * (1.0 + (np.arange(500) % 3)[:, None] * rng.uniform(0, 2, (1, 300)))).astype(np.float32)
  dense = SingleCellOMIC(counts).normalize(total=True, log1p=True)
  sparse = SingleCellOMIC(sp.csr_matrix(counts)).normalize(total=True, log1p=True)
  assert sparse.is_sparse() and not dense.is_sparse()
  Y = dense.dimension_reduce(algo="tsne", n_components=2)
  assert Y.shape == (500, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
  assert dense.dimension_reduce(algo="tsne", n_components=2) is Y
  assert _same_bits(sparse.dimension_reduce(algo="tsne", n_components=2), Y)
  left = dense.get_pca()
  fresh = SingleCellOMIC(counts).normalize(total=True, log1p=True)
  fresh.dimension_reduce(algo="pca")
  assert left.components_.shape == (100, 300) and _same_bits(left.components_, fresh.get_pca().components_)
  assert _same_bits(left.mean_, fresh.get_pca().mean_) and _same_bits(dense.dimension_reduce(algo="pca"), fresh.dimension_reduce(algo="pca"))
