"""The definition of the mutual-information matrix (tests/mutual_info_ref.py) held to scikit-learn, on the host: the three estimators
per pair of columns, the preparation of _estimate_mi around them, the edge cases, the refusals of the public function, and a mutation
check of the restatement itself.  The device is held to the restatement in tests/test_gpu_mutual_info.py.

scikit-learn's cd estimator leaves its k-d tree for the brute-force path in label groups of 2 .. 2k + 1 cells; that path forms distances
as sqrt(x^2 + y^2 - 2xy), which loses the 1e-10 noise, and its result then differs from the exact estimator's by up to 0.17 nats.  The
exact estimator is the definition here, so the comparisons with scikit-learn fold such groups into the largest one (singletons stay)."""
import numpy as np
import pytest

from tests import mutual_info_ref as R

NS = (8, 63, 64, 65, 257, 600)
KS = (1, 3, 5)


def _columns(N, k, ties, seed):
  """(x, y) continuous and d discrete for one grid case; `ties`: the values floored to a grid (heavy ties) before the 1e-10 noise"""
  rng = np.random.RandomState(seed)
  x = rng.standard_normal(N)
  y = 0.6 * x + rng.standard_normal(N)
  if ties:
    x, y = np.floor(x * 2) / 2, np.floor(y * 2) / 2
    x, y = x + 1e-10 * rng.standard_normal(N), y + 1e-10 * rng.standard_normal(N)
  d = np.floor(2 * x + rng.standard_normal(N)).clip(-2, 2)   # five labels that depend on x
  d[:2] = (7, 8)                                             # ... and two singletons
  return x, y, R.fold_small_groups(d, k)


@pytest.mark.parametrize("ties", (False, True))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", NS)
def test_cc_equals_sklearn(N, k, ties):
  from sklearn.feature_selection._mutual_info import _compute_mi_cc
  x, y, _ = _columns(N, k, ties, 100 + N + k)
  assert R.mi_cc(x, y, k) == _compute_mi_cc(x, y, k)


def _cd_by_loops(c, d, k):
  """Ross's estimator written out cell by cell, for the one grid case scikit-learn cannot referee"""
  from scipy.special import digamma
  N = len(c)
  kept = [i for i in range(N) if (d == d[i]).sum() > 1]
  terms = []
  for i in kept:
    group = [j for j in range(N) if d[j] == d[i] and j != i]
    ki = min(k, len(group))
    r = np.nextafter(sorted(abs(c[j] - c[i]) for j in group)[ki - 1], 0.0)
    m = sum(1 for j in kept if abs(c[j] - c[i]) <= r)
    terms.append(digamma(ki) - digamma(len(group) + 1) - digamma(m))
  return max(0.0, float(digamma(len(kept)) + np.mean(terms))) if kept else 0.0


@pytest.mark.parametrize("ties", (False, True))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", NS)
def test_cd_equals_sklearn(N, k, ties):
  from sklearn.feature_selection._mutual_info import _compute_mi_cd
  x, _, d = _columns(N, k, ties, 200 + N + k)
  counts = np.unique(d, return_counts=True)[1]
  if not ((counts == 1) | (counts >= 2 * k + 2)).all():   # (N = 8: one label for every cell)
    d = np.zeros(N)
  if N >= 2 * k + 2:
    assert R.mi_cd(x, d, k) == _compute_mi_cd(x, d, k)
  else:
    # N = 8, k = 5: no labelling has a group of 2k + 2 = 12 cells, so scikit-learn takes its brute-force path whatever the labels; the
    # restatement is held to the estimator written out by loops instead, on labels with small groups and singletons
    d = np.array([0, 0, 0, 0, 0, 1, 1, 2.0])
    assert abs(R.mi_cd(x, d, k) - _cd_by_loops(x, d, k)) <= 1e-14


@pytest.mark.parametrize("N", NS)
def test_dd_close_to_sklearn(N):
  from sklearn.metrics import mutual_info_score
  rng = np.random.RandomState(300 + N)
  a = rng.randint(0, 5, N).astype(np.float64)
  b = np.where(rng.uniform(size=N) < 0.5, a, rng.randint(0, 3, N))
  assert abs(R.mi_dd(a, b) - mutual_info_score(a, b)) <= 1e-12
  c = rng.randint(-2, 2, N).astype(np.float64)   # (independent labels, negative values among them)
  assert abs(R.mi_dd(a, c) - mutual_info_score(a, c)) <= 1e-12


_mixed = R.mixed_problem


def test_preparation_equals_sklearn():
  """The whole of _estimate_mi.  The preparation reproduces scale()'s bits (the block's standard deviation is reduced as scikit-learn
  reduces it), so the comparison is equality up to the closing sums: the estimators' integers are the same, and np.mean of the same
  digamma values is the same."""
  from sklearn.feature_selection import mutual_info_classif, mutual_info_regression
  X, mask, y, yd = _mixed()
  for k in (1, 3):
    got = R.estimate_mi(X, y, mask, False, k, 1)
    want = mutual_info_regression(X, y, discrete_features=mask, n_neighbors=k, random_state=1)
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[~mask], want[~mask])
    got = R.estimate_mi(X, yd, mask, True, k, 1)
    want = mutual_info_classif(X, yd, discrete_features=mask, n_neighbors=k, random_state=1)
    assert np.abs(got - want).max() <= 1e-12


def test_host_preparation_is_the_restatement(monkeypatch):
  """sisua_amd.mutual_info prepares the columns that tests/mutual_info_ref.prepare does, bit for bit, whatever the host chunk and whether
  the noise block is kept or walked: the device entry is replaced by a recorder."""
  from sisua_amd import engine, mutual_info as M
  X, mask, y, yd = _mixed()
  Y = np.stack([y, yd, 2.0 * y + 1.0], axis=1)
  seen = {}

  def record(xcols, xd, ycols, ydm, k, gene_chunk):
    seen.setdefault("x", []).append(np.array(xcols))
    seen["y"], seen["xd"], seen["yd"] = np.array(ycols), seen.get("xd", []) + list(xd), list(ydm)
    return np.zeros((len(xcols), len(ycols)))

  monkeypatch.setattr(engine, "mutual_info", record)
  want_x, want_y = R.prepare(X, y, mask, False, 1)
  for chunk_bytes, keep in ((64 << 20, 256 << 20), (8 * 300 * 2, 256 << 20), (8 * 300, 0)):
    monkeypatch.setattr(M, "_HOST_CHUNK_BYTES", chunk_bytes)
    monkeypatch.setattr(M, "_NOISE_KEEP_BYTES", keep)
    monkeypatch.setattr(M, "_NOISE_ROWS", 700)
    seen.clear()
    M.mutual_information(X, Y, discrete_features=mask, discrete_targets=np.array([False, True, False]))
    got = np.concatenate(seen["x"], axis=0)
    assert np.array_equal(got, want_x.T), (chunk_bytes, keep)
    assert np.array_equal(seen["y"][0], want_y) and np.array_equal(seen["y"][1], yd)
    assert np.array_equal(seen["y"][2], R.prepare(X, Y[:, 2], mask, False, 1)[1])
    assert seen["xd"] == list(mask) and seen["yd"] == [False, True, False]
  seen.clear()   # 'auto': every value an integer
  M.mutual_information(X, Y)
  assert seen["xd"] == list(mask) and seen["yd"] == [False, True, False]
  seen.clear()   # sparse X is taken by columns; genes= is X[:, genes]
  import scipy.sparse as sp
  sel = [4, 0, 0, 5]
  M.mutual_information(sp.csr_matrix(X), Y, discrete_features=mask, genes=sel, noise=False)
  assert np.array_equal(np.concatenate(seen["x"], axis=0), R.prepare(X[:, sel], y, mask[sel], False, 1, noise=False)[0].T)


# ---- edge cases, pinned --------------------------------------------------------------------------------------------------------------
def test_edge_cases():
  from scipy.special import digamma
  rng = np.random.RandomState(11)
  N, k = 40, 3
  x = rng.standard_normal(N)
  const = np.full(N, 2.5)
  # a constant continuous column: every distance along it is 0 <= r, so its count is N and its term psi(N) cancels psi(N); what is left
  # is psi(k) - mean psi(nx + 1) with r_i the k-th distance along x alone -> nx = k - 1: 0 up to the rounding of the two means
  assert R.mi_cc(x, const, k) <= 1e-14
  r, nx, ny = R.mi_cc_cells(x, const, k)
  assert (ny == N - 1).all() and (nx == k - 1).all()
  # all labels unique: no cell is kept
  assert R.mi_cd(x, np.arange(N, dtype=np.float64), k) == 0.0
  assert R.mi_cd_cells(x, np.arange(N), k)[0].sum() == 0
  # a single label: count = N, m_i = the k + 1 cells within the k-th neighbour's distance less one ulp -> k cells
  kept, ki, count, m, _ = R.mi_cd_cells(x, np.zeros(N), k)
  assert kept.all() and (ki == k).all() and (count == N).all() and (m == k).all()
  assert R.mi_cd(x, np.zeros(N), k) <= 1e-14   # psi(N) + psi(k) - psi(N) - psi(k), up to the rounding of the means
  assert R.mi_dd(np.zeros(N), rng.randint(0, 3, N)) == 0.0
  # N = k + 1: every other cell is a neighbour
  xs, ys = rng.standard_normal(k + 1), rng.standard_normal(k + 1)
  r, nx, ny = R.mi_cc_cells(xs, ys, k)
  d = np.maximum(np.abs(xs[:, None] - xs[None]), np.abs(ys[:, None] - ys[None]))
  assert np.array_equal(r, np.nextafter(d.max(1), 0.0)) and (np.minimum(nx, ny) <= k - 1).all()   # (the farthest cell is outside along one axis)
  # labels compare by value: -0.0 is 0.0
  assert R.mi_dd(np.array([0.0, -0.0, 1.0, 1.0]), np.array([0.0, 0.0, 1.0, 1.0])) == pytest.approx(np.log(2.0), abs=1e-15)


def test_refusals_need_no_device():
  from sisua_amd import mutual_info as M
  from sisua_amd.engine import MI_MAX_NEIGHBORS
  assert MI_MAX_NEIGHBORS >= 8
  X, Y = np.random.RandomState(0).standard_normal((10, 3)), np.random.RandomState(1).standard_normal((10, 2))
  with pytest.raises(ValueError, match="below the number of cells"):
    M.mutual_information(X[:6], Y[:6], n_neighbors=6)
  with pytest.raises(ValueError, match="MI_MAX_NEIGHBORS"):
    M.mutual_information(np.zeros((100, 3)), np.zeros((100, 2)), n_neighbors=MI_MAX_NEIGHBORS + 1)
  with pytest.raises(ValueError, match="n_neighbors"):
    M.mutual_information(X, Y, n_neighbors=0)
  bad = X.copy()
  bad[3, 2] = np.nan
  with pytest.raises(ValueError, match="gene column 2 .*not finite"):
    M.mutual_information(bad, Y)
  bad = Y.copy()
  bad[0, 1] = np.inf
  with pytest.raises(ValueError, match="protein column 1 .*not finite"):
    M.mutual_information(X, bad)
  with pytest.raises(ValueError):
    M.mutual_information(X, Y[:5])
  with pytest.raises(IndexError):
    M.mutual_information(X, Y, genes=[3])
  with pytest.raises(ValueError, match="n_neighbors"):
    R.estimate_mi(X[:6], Y[:6, 0], np.zeros(3, bool), False, k=6)


def test_marker_scores_and_plumbing():
  import re
  import sisua_amd
  from sisua_amd import _hip, build, metrics
  m = np.arange(6.0).reshape(3, 2)
  genes, prots, markers = ["CD4", "CD8A", "X"], ["CD4", "CD8"], {"CD8": "CD8A", "CD4": "CD4", "CD19": "CD19"}
  for kind in ("pearson", "spearman", "mi"):
    assert metrics.marker_scores(m, kind, genes, prots, markers) == {f"{kind}_CD8A_CD8": 3.0, f"{kind}_CD4_CD4": 0.0}
  assert metrics.marker_scores(m, "pearson", genes, prots, markers) == metrics.marker_correlations(m, "pearson", genes, prots, markers)
  with pytest.raises(NotImplementedError):
    metrics.marker_scores(m, "lasso", genes, prots, markers)
  with pytest.raises(ValueError):
    metrics.marker_scores(m.T, "mi", genes, prots, markers)
  assert sisua_amd.mutual_information is sisua_amd.mutual_info.mutual_information and sisua_amd.marker_scores is metrics.marker_scores
  assert _hip.SMX_ABI_VERSION >= 14 and "smx_mi.hip" in build.SOURCES
  header = open(build.os.path.join(build.CSRC, build.HEADERS[-1])).read()
  for name in ("smx_mutual_info", "smx_k_mi_cells"):
    assert name in _hip.SIGNATURES and re.search(r"\bint %s\(" % name, header)


# ---- the restatement itself: each rule switched off breaks a named case ------------------------------------------------------------------
def test_mutations_are_seen():
  from sklearn.feature_selection._mutual_info import _compute_mi_cc, _compute_mi_cd
  x, y, d = _columns(257, 3, False, 42)
  cc, cd = _compute_mi_cc(x, y, 3), _compute_mi_cd(x, d, 3)
  assert R.mi_cc(x, y, 3) == cc and R.mi_cd(x, d, 3) == cd
  # without nextafter the k-th neighbour itself is inside the radius: a count of every cell grows
  assert R.mi_cc(x, y, 3, nextafter=False) != cc
  assert R.mi_cd(x, d, 3, nextafter=False) != cd
  a, b = R.mi_cc_cells(x, y, 3, nextafter=False), R.mi_cc_cells(x, y, 3)
  assert (a[1] + a[2] > b[1] + b[2]).all()   # (the k-th neighbour is at the radius along at least one axis)
  # counting without the cell itself
  assert R.mi_cc(x, y, 3, count_self=False) != cc
  assert R.mi_cd(x, d, 3, count_self=False) != cd
  # keeping the two singletons: n' grows by 2
  assert R.mi_cd_cells(x, d, 3, drop_singletons=False)[0].sum() == R.mi_cd_cells(x, d, 3)[0].sum() + 2
  assert R.mi_cd(x, d, 3, drop_singletons=False) != cd
