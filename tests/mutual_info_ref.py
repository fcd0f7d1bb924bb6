"""The definition of the gene x protein mutual-information matrix (smx_mi.hip, sisua_amd/mutual_info.py): scikit-learn's three
estimators restated in NumPy float64, per pair of columns, with every distance the exact |a - b|.

  cc  both continuous        Kraskov et al. (KSG), sklearn.feature_selection._mutual_info._compute_mi_cc
  cd  continuous x discrete  Ross, _compute_mi_cd
  dd  both discrete          sklearn.metrics.mutual_info_score

and the preparation of `_estimate_mi` around them (`prepare`): continuous columns divided by their standard deviation, then
1e-10 max(1, mean|x|) noise from RandomState(seed) in scikit-learn's order of draws.

Two stated deviations from scikit-learn: in a label group of 2 .. 2k + 1 members its NearestNeighbors takes the brute-force path, whose
distances sqrt(x^2 + y^2 - 2xy) lose the 1e-10 noise -- here the distances are exact; and where no cell is kept (every label unique)
cd is 0.0 where scikit-learn raises.

The *_cells functions return the per-cell integers and radii that the device's kernel-level entry returns.  The keywords `nextafter`,
`count_self` and `drop_singletons` exist for the mutation check of tests/test_mutual_info_host.py: each switches one rule of the
definition off."""
import numpy as np
from scipy.special import digamma


def _kth_smallest_others(d, k):
  """d [N, N] distances -> per row the k-th smallest (k [N] or a number, 1-based) over the OTHER columns"""
  N = d.shape[0]
  d = d.copy()
  d[np.arange(N), np.arange(N)] = np.inf
  s = np.sort(d, axis=1)
  return s[np.arange(N), np.broadcast_to(np.asarray(k), (N,)) - 1]


def mi_cc_cells(x, y, k, nextafter=True, count_self=True):
  """-> (r [N] float64, nx [N], ny [N] int64): the radius just inside the k-th nearest Chebyshev neighbour, and how many OTHER cells lie
  within it along each axis"""
  x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
  dx, dy = np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :])
  r = _kth_smallest_others(np.maximum(dx, dy), k)
  if nextafter:
    r = np.nextafter(r, 0.0)
  self_ = 1 if count_self else 0   # (the cell itself is inside its own radius, and the estimator takes it out again)
  nx = (dx <= r[:, None]).sum(1) - 1 - (1 - self_)
  ny = (dy <= r[:, None]).sum(1) - 1 - (1 - self_)
  return r, nx, ny


def mi_cc_from_cells(nx, ny, k):
  return max(0.0, float(digamma(len(nx)) + digamma(k) - np.mean(digamma(nx + 1)) - np.mean(digamma(ny + 1))))


def mi_cc(x, y, k, **mut):
  _, nx, ny = mi_cc_cells(x, y, k, **mut)
  return mi_cc_from_cells(nx, ny, k)


def mi_cd_cells(c, d, k, nextafter=True, count_self=True, drop_singletons=True):
  """-> (kept, k_i, count_i, m_i [N] int64, r [N] float64); k_i, m_i and r are 0 where the cell is not kept"""
  c, d = np.asarray(c, np.float64), np.asarray(d, np.float64)
  N = len(c)
  dist = np.abs(c[:, None] - c[None, :])
  same = d[:, None] == d[None, :]
  count = same.sum(1)
  kept = count > 1 if drop_singletons else np.ones(N, bool)
  ki = np.where(count > 1, np.minimum(k, count - 1), 0)
  r = np.zeros(N)
  rows = np.flatnonzero(count > 1)
  if rows.size:
    within = np.where(same, dist, np.inf)
    r[rows] = _kth_smallest_others(within, np.maximum(ki, 1))[rows]
    if nextafter:
      r[rows] = np.nextafter(r[rows], 0.0)
  m = ((dist <= r[:, None]) & kept[None, :]).sum(1) - (0 if count_self else 1)
  m = np.where(kept, m, 0)
  return kept.astype(np.int64), ki * kept, count, m, r * (count > 1)


def mi_cd(c, d, k, **mut):
  kept, ki, count, m, _ = mi_cd_cells(c, d, k, **mut)
  return mi_cd_from_cells(kept, ki, count, m)


def mi_cd_from_cells(kept, ki, count, m):
  on = kept.astype(bool)
  n = int(on.sum())
  if n == 0:
    return 0.0   # (scikit-learn raises here: a stated deviation)
  with np.errstate(all="ignore"):   # (a mutation may ask for digamma(0))
    v = digamma(n) + np.mean(digamma(ki[on])) - np.mean(digamma(count[on])) - np.mean(digamma(m[on]))
  return max(0.0, float(v))


def mi_dd_triples(a, b):
  """-> (a value, b value, n_ab) [R] of the non-empty cells of the contingency table, sorted by (a, b)"""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  ua, ia = np.unique(a, return_inverse=True)
  ub, ib = np.unique(b, return_inverse=True)
  key, n = np.unique(ia.astype(np.int64) * len(ub) + ib, return_counts=True)
  return ua[key // len(ub)], ub[key % len(ub)], n


def mi_dd(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  N = len(a)
  va, vb, nab = mi_dd_triples(a, b)
  na = np.array([(a == v).sum() for v in va])
  nb = np.array([(b == v).sum() for v in vb])
  terms = nab / N * (((np.log(nab) - np.log(na)) - np.log(nb)) + np.log(N))
  return max(0.0, float(terms.sum()))


def mi_pair(x, y, x_discrete, y_discrete, k):
  """scikit-learn's _compute_mi: the estimator the kinds of the two columns select"""
  if x_discrete and y_discrete:
    return mi_dd(x, y)
  if x_discrete:
    return mi_cd(y, x, k)
  if y_discrete:
    return mi_cd(x, y, k)
  return mi_cc(x, y, k)


def scale_no_mean(x):
  """sklearn.preprocessing.scale(x, with_mean=False) of one column: x / std, a std below 10 eps read as 1"""
  x = np.asarray(x, np.float64)
  s = np.nanstd(x)
  return x / (1.0 if s < 10 * np.finfo(np.float64).eps else s)


def prepare(X, y, discrete_mask, y_discrete, seed=1, noise=True):
  """_estimate_mi's preparation of the features X [N, G] and ONE target y [N] -> (X', y') float64"""
  X = np.array(X, np.float64)
  y = np.array(y, np.float64)
  cont = ~np.asarray(discrete_mask, bool)
  N = X.shape[0]
  rng = np.random.RandomState(seed)
  if cont.any():
    Xc = X[:, cont]   # (the block as scikit-learn reduces it: NumPy adds the rows of several columns in order, one column pairwise)
    s = np.nanstd(Xc, axis=0)
    s[s < 10 * np.finfo(np.float64).eps] = 1.0
    X[:, cont] = Xc / s
    means = np.maximum(1, np.mean(np.abs(X[:, cont]), axis=0))
    z = rng.standard_normal(size=(N, int(cont.sum())))
    if noise:
      X[:, cont] += 1e-10 * means * z
  if not y_discrete:
    y = scale_no_mean(y)
    z = rng.standard_normal(size=N)
    if noise:
      y = y + 1e-10 * np.maximum(1, np.mean(np.abs(y))) * z
  return X, y


def estimate_mi(X, y, discrete_mask, y_discrete, k=3, seed=1, noise=True):
  """mutual_info_regression / mutual_info_classif (y_discrete) of the features against one target -> [G]"""
  if k >= len(y):
    raise ValueError(f"n_neighbors = {k} must be below the number of cells ({len(y)})")
  Xp, yp = prepare(X, y, discrete_mask, y_discrete, seed, noise)
  return np.array([mi_pair(Xp[:, g], yp, bool(discrete_mask[g]), y_discrete, k) for g in range(Xp.shape[1])])


def fold_small_groups(d, k):
  """Labels for a comparison with scikit-learn's cd: groups of 2 .. 2k + 1 members (where its brute-force distances differ from the exact
  ones) are merged into the largest group; singletons stay."""
  d = np.array(d, np.float64)
  vals, counts = np.unique(d, return_counts=True)
  big = vals[np.argmax(counts)]
  for v, c in zip(vals, counts):
    if 2 <= c <= 2 * k + 1 and v != big:
      d[d == v] = big
  return d


def mixed_problem(N=300, seed=5):
  """A small mix for the comparisons with scikit-learn: X [N, 6] (columns 1 and 4 discrete), its mask, a continuous and a discrete target"""
  rng = np.random.RandomState(seed)
  X = rng.standard_normal((N, 6))
  X[:, 1] = rng.poisson(2.0, N)
  X[:, 3] = np.exp(X[:, 0] + 0.3 * rng.standard_normal(N))
  X[:, 4] = rng.randint(0, 3, N)
  mask = np.array([False, True, False, False, True, False])
  y = 0.5 * X[:, 0] + rng.standard_normal(N)
  yd = (X[:, 4] + (rng.uniform(size=N) < 0.3)).astype(np.float64)
  for j in (1, 4):   # (label groups of 2 .. 2k + 1 cells folded away: scikit-learn's distances differ there)
    X[:, j] = fold_small_groups(X[:, j], 3)
  return X, mask, y, fold_small_groups(yd, 3)
