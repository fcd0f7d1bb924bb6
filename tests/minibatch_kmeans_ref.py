"""A float64 NumPy restatement of what the reference's SingleCellOMIC.clustering asks of scikit-learn's MiniBatchKMeans: the k-means++
seeding (`_kmeans_plusplus`, unit weights), one `_mini_batch_step` (assign, incremental centre update, random reassignment of starved
centres), `predict`, the draws of `partial_fit` from `RandomState` in scikit-learn's order, and the `clustering` recipe with its
matching of clusters to variable names.  No scikit-learn here: tests/test_minibatch_kmeans_host.py holds this file to it.

Every squared distance is the direct form sum_j ((double)x_j - c_j)^2.  `k_seed`, `k_step` and `k_predict` have the signatures and the
return values of `sisua_amd.engine.k_mbkmeans_seed / _step / _predict`, so the host tests put them in the engine's place.  Beside the
results they keep what the GPU tests need to hold equality honest: the margins between the two smallest distances of a row, between a
pick's target and the scan values around it, and between the two best candidate potentials (see `Margins`)."""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -53


def dense64(x):
  return np.asarray(x.toarray() if sp.issparse(x) else x, dtype=np.float64)


def sqdist(X, C):
  """[n, K] float64: the direct form, one centre at a time"""
  X = dense64(X)
  out = np.empty((X.shape[0], C.shape[0]), np.float64)
  for k in range(C.shape[0]):
    d = X - C[k]
    out[:, k] = (d * d).sum(axis=1)
  return out


def chain_bound(n_roundings, abs_sum):
  """|device - restatement| of a sum whose every side makes at most n_roundings roundings on its way (the squares and the
  additions of the longest chain, in ANY order of summation): 2 n 2^-53 x (the sum of the absolute terms)"""
  return 2.0 * n_roundings * EPS * abs_sum


class Margins:
  """The smallest margins met so far (1.0: none met).  row: (d2 - d1) / d2 of a row's two smallest distances to DIFFERENT centre rows
  (two centres that are the same row tie exactly on every side and go to the lowest index); pick: the distance of a pick's u x pot
  from the scan values on either side, over pot (pot = 0: every scan value is an exact 0 on every side and the pick is row 0);
  cand: (second - best) / second of the candidate potentials of DIFFERENT rows."""

  def __init__(self):
    self.row = self.pick = self.cand = 1.0

  def ok(self, tol=1e-9):
    return self.row > tol and self.pick > tol and self.cand > tol


def _row_margin(D, C, mg):
  if mg is None or D.shape[1] < 2:
    return
  order = np.argsort(D, axis=1, kind="stable")[:, :2]
  d1, d2 = np.take_along_axis(D, order, axis=1).T
  for r in np.flatnonzero(d2 - d1 <= 1e-6 * d2):   # (only the close calls are looked at one by one)
    if d1[r] == d2[r] and np.array_equal(C[order[r, 0]], C[order[r, 1]]):
      continue
    mg.row = min(mg.row, (d2[r] - d1[r]) / d2[r] if d2[r] > 0 else 0.0)
  far = d2 - d1 > 1e-6 * d2
  if far.any():
    mg.row = min(mg.row, float(((d2 - d1)[far] / d2[far]).min()))


def k_seed(x, K, first, u, margins=None):
  """scikit-learn's _kmeans_plusplus with unit weights: first = the first centre's row, u [K - 1, T] in [0, 1) ->
  dict(indices [K] int32, centres [K, G] float64, potential [K] float64)"""
  X = dense64(x)
  n = X.shape[0]
  u = np.asarray(u, np.float64).reshape(K - 1, -1)
  idx, pot = np.empty(K, np.int32), np.empty(K, np.float64)
  idx[0] = first
  closest = sqdist(X, X[[first]])[:, 0]
  pot[0] = closest.sum()
  for c in range(1, K):
    scan = np.cumsum(closest)
    target = u[c - 1] * pot[c - 1]
    cand = np.minimum(np.searchsorted(scan, target, side="left"), n - 1)
    if margins is not None and pot[c - 1] > 0:
      for t, j in zip(target, cand):
        near = min(abs(scan[j] - t), abs(t - scan[j - 1]) if j > 0 else np.inf)
        margins.pick = min(margins.pick, near / pot[c - 1])
    D = np.minimum(closest[None, :], sqdist(X, X[cand]).T)   # [T, n]
    pots = D.sum(axis=1)
    best = int(np.argmin(pots))
    if margins is not None:
      other = pots[[not np.array_equal(X[j], X[cand[best]]) for j in cand]]
      if other.size:
        margins.cand = min(margins.cand, (other.min() - pots[best]) / other.min() if other.min() > 0 else 0.0)
    idx[c], pot[c], closest = cand[best], pots[best], D[best]
  return dict(indices=idx, centres=X[idx].copy(), potential=pot)


def k_step(x, centres, counts, want_labels=True, margins=None):
  """one _mini_batch_step without the reassignment -> dict(centres, counts (new arrays), inertia, labels or None)"""
  X = dense64(x)
  C, cnt = np.array(centres, np.float64), np.array(counts, np.float64)
  D = sqdist(X, C)
  _row_margin(D, C, margins)
  lab = np.argmin(D, axis=1)
  inertia = float(D[np.arange(X.shape[0]), lab].sum())
  for k in range(C.shape[0]):
    rows = np.flatnonzero(lab == k)
    if rows.size:
      s = np.zeros(X.shape[1])
      for r in rows:   # (row order)
        s += X[r]
      C[k] = (C[k] * cnt[k] + s) / (cnt[k] + rows.size)
      cnt[k] += rows.size
  return dict(centres=C, counts=cnt, inertia=inertia, labels=lab.astype(np.int32) if want_labels else None)


def k_predict(x, centres, block_rows=0, want_distance=False, margins=None):
  C = np.asarray(centres, np.float64)
  D = sqdist(x, C)
  _row_margin(D, C, margins)
  lab = np.argmin(D, axis=1).astype(np.int32)
  return (lab, D[np.arange(D.shape[0]), lab]) if want_distance else lab


def take_rows(x, rows):
  return dense64(x[rows])


class Model:
  """MiniBatchKMeans.partial_fit / predict as the reference uses them, on the k_* above.  `reassigned`: one flag per step, whether
  centres were replaced by rows of the block."""

  def __init__(self, n_clusters=8, init="k-means++", batch_size=1024, compute_labels=True, random_state=None, reassignment_ratio=0.01):
    self.K, self.init, self.batch_size, self.compute_labels = int(n_clusters), init, int(batch_size), compute_labels
    self.random_state, self.ratio = random_state, reassignment_ratio
    self.margins, self.reassigned, self.centres = Margins(), [], None

  def partial_fit(self, X):
    n, K = X.shape[0], self.K
    if self.centres is None:
      self.rng = np.random.RandomState(self.random_state)
      self.bs = min(self.batch_size, n)
      init_size = 3 * self.bs
      if init_size < K:
        init_size = 3 * K
      Xi = X
      if init_size < n:
        Xi = X[self.rng.randint(0, n, init_size)]
      ni = Xi.shape[0]
      if isinstance(self.init, str) and self.init == "k-means++":
        first = self.rng.choice(ni, p=np.ones(ni) / ni)
        u = self.rng.uniform(size=(K - 1, 2 + int(np.log(K))))
        self.centres = k_seed(Xi, K, first, u, margins=self.margins)["centres"]
      elif isinstance(self.init, str) and self.init == "random":
        self.centres = take_rows(Xi, self.rng.choice(ni, size=K, replace=False, p=np.ones(ni) / ni))
      else:
        self.centres = np.array(self.init, np.float64)
      self.counts, self.since, self.n_steps = np.zeros(K), 0, 0
    self.since += self.bs
    reassign = bool((self.counts == 0).any() or self.since >= 10 * K)
    if reassign:
      self.since = 0
    r = k_step(X, self.centres, self.counts, want_labels=False, margins=self.margins)
    self.centres, self.counts = r["centres"], r["counts"]
    did = False
    if reassign and self.ratio > 0:
      to = self.counts < self.ratio * self.counts.max()
      if to.sum() > 0.5 * n:
        to[np.argsort(self.counts)[int(0.5 * n):]] = False
      if to.sum():
        self.centres[to] = take_rows(X, self.rng.choice(n, replace=False, size=int(to.sum())))
        did = True
      self.counts[to] = np.min(self.counts[~to])
    self.reassigned.append(did)
    if self.compute_labels:
      self.labels, d = k_predict(X, self.centres, want_distance=True, margins=self.margins)
      self.inertia = float(d.sum())
    self.n_steps += 1
    return self

  def predict(self, X):
    return k_predict(X, self.centres, margins=self.margins)


def batches(n, batch_size, random_state):
  """the row batches of the `clustering` recipe: (s, min(s + batch_size, n)) in the order RandomState(random_state).permutation"""
  starts = np.arange(0, n, batch_size)
  return [(int(s), int(min(s + batch_size, n))) for s in starts[np.random.RandomState(random_state).permutation(len(starts))]]


def match(labels, probs, K):
  """ids [n_vars]: cluster ids[i] takes variable i -- the linear assignment that maximises sum_i corr[i, ids[i]]"""
  from scipy.optimize import linear_sum_assignment
  corr = np.zeros((probs.shape[1], K), np.float64)
  for lab in range(K):
    corr[:, lab] = np.asarray(probs, np.float64)[labels == lab].sum(axis=0)
  return linear_sum_assignment(corr, maximize=True)[1]


def clustering(X, K, random_state=1, batch_size=4096, probs=None, var_names=None, model=None):
  """labels [n] int64 of the recipe; with probs [n, K] and var_names [K] the names after matching"""
  m = model or Model(K, batch_size=batch_size, compute_labels=False, random_state=random_state)
  for s, e in batches(X.shape[0], batch_size, random_state):
    m.partial_fit(X[s:e])
  labels = m.predict(X).astype(np.int64)
  if probs is None:
    return labels
  ids = match(labels, probs, K)
  names = {int(c): var_names[i] for i, c in enumerate(ids)}
  return np.array([names[int(c)] for c in labels])


# ---- fixtures shared by the host and the GPU tests: name -> (rows, genes, K, batch, kind) ------------------------------------------
FIXTURES = {
    "tiny": (37, 5, 3, 16, "blobs"),
    "wide": (200, 33, 12, 64, "blobs"),
    "one_batch": (300, 7, 5, 4096, "blobs"),
    "counts": (130, 70, 50, 64, "counts"),
    "outlier_a": (400, 6, 4, 256, "outlier"),
    "outlier_b": (300, 9, 5, 128, "outlier"),
    "outlier_c": (700, 4, 3, 4096, "outlier"),
}
OUTLIER_FIXTURES = ("outlier_a", "outlier_b", "outlier_c")


def make(name, seed=0):
  """the float32 matrix of a fixture.  blobs: K Gaussian blobs; counts: floor(|x|) of wide Gaussians, ten rows twice and four rows of zeros;
  outlier: K - 1 blobs, and 1 - 3 rows of the first batch moved by 60, 120, ... on every coordinate, which take a centre each at
  the seeding, then starve, so that a later step reassigns them"""
  rows, genes, K, batch, kind = FIXTURES[name]
  rng = np.random.RandomState(1000 + seed)
  if kind == "counts":
    x = np.floor(np.abs(rng.normal(0.0, 30.0, (rows, genes))))
    x[10:20], x[20:24] = x[0:10], 0.0
    return x.astype(np.float32)
  blobs = K - 1 if kind == "outlier" else K
  x = rng.normal(0.0, 4.0, (blobs, genes))[rng.randint(0, blobs, rows)] + rng.normal(0.0, 1.0, (rows, genes))
  if kind == "outlier":
    n_out = 1 + seed % 3
    for i, r in enumerate(rng.choice(min(batch, rows), n_out, replace=False)):
      x[r] += 60.0 * (i + 1)
  return x.astype(np.float32)
