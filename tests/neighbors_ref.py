"""float64 NumPy restatement of the four definitions of the neighbour-graph entries (include/sisua_hip.h: smx_pca_cov, smx_pca_project,
smx_knn, smx_knn_umap).  Plain loops and NumPy sums, written from the definitions and not from the kernels: what
tests/test_gpu_neighbors.py holds the device to and tests/test_neighbors_host.py holds to scikit-learn."""
import numpy as np


def pca_cov(X):
  """-> (mean [G], S [G, G]): the float64 column means and the two-pass covariance (X - mean)^T (X - mean) / (n - 1)"""
  X = np.asarray(X, dtype=np.float64)
  n = X.shape[0]
  mean = X.sum(axis=0) / n
  Xc = X - mean
  return mean, Xc.T @ Xc / (n - 1)


def flip_signs(comp):
  """each row's entry of largest magnitude positive, ties to the lowest column"""
  comp = np.array(comp, dtype=np.float64)
  for c in range(comp.shape[0]):
    if comp[c, np.argmax(np.abs(comp[c]))] < 0:
      comp[c] = -comp[c]
  return comp


def pca_fit(X, n_components):
  """-> dict(mean, components [C, G], explained_variance, explained_variance_ratio, singular_values): eigh of the covariance, components
  by decreasing eigenvalue, negative eigenvalues clamped to 0, the ratio against trace(S)"""
  mean, S = pca_cov(X)
  w, v = np.linalg.eigh(S)
  order = np.argsort(-w, kind="stable")[:n_components]
  ev = np.maximum(w[order], 0.0)
  n = np.asarray(X).shape[0]
  return dict(mean=mean, components=flip_signs(v[:, order].T), explained_variance=ev, explained_variance_ratio=ev / np.trace(S),
              singular_values=np.sqrt(ev * (n - 1)))


def pca_project64(X, mean, components):
  """(x - mean) . components^T in float64"""
  return (np.asarray(X, dtype=np.float64) - mean) @ np.asarray(components, dtype=np.float64).T


def pca_project(X, mean, components):
  return pca_project64(X, mean, components).astype(np.float32)


def sq_distances(Z):
  """d2 [N, N] float64 in the direct form sum_d (z_i[d] - z_j[d])^2"""
  Z = np.asarray(Z, dtype=np.float64)
  d2 = np.empty((Z.shape[0], Z.shape[0]))
  for i in range(Z.shape[0]):
    d2[i] = np.square(Z - Z[i]).sum(axis=1)
  return d2


def knn(Z, k, d2=None):
  """-> (idx [N, k] int32, dist [N, k], d2 [N, k]): per cell the k others with the smallest (d2, j), ascending"""
  d2 = sq_distances(Z) if d2 is None else d2
  N = d2.shape[0]
  idx = np.empty((N, k), np.int32)
  for i in range(N):
    order = np.argsort(d2[i], kind="stable")   # stable: equal d2 stay in index order = the order (d2, j)
    idx[i] = order[order != i][:k]
  best = np.take_along_axis(d2, idx.astype(np.int64), axis=1)
  return idx, np.sqrt(best), best


def knn_gap(Z, k, d2=None):
  """the smallest relative gap between consecutive sorted d2 among each cell's first k + 1 candidates (all of them when k = N - 1)"""
  d2 = sq_distances(Z) if d2 is None else d2
  N = d2.shape[0]
  gap = np.inf
  for i in range(N):
    s = np.sort(np.delete(d2[i], i))[:k + 1]
    if s.size > 1:
      gap = min(gap, float(np.min(np.diff(s) / s[1:])))
  return gap


def with_self(idx, dist):
  N = idx.shape[0]
  return (np.concatenate([np.arange(N, dtype=np.int32)[:, None], idx], axis=1),
          np.concatenate([np.zeros((N, 1)), np.asarray(dist, dtype=np.float64)], axis=1))


def umap_rows(idx, dist, margins=False):
  """rho [N], sigma [N], weight [N, K] of a table whose column 0 is the cell itself.  margins: also (min |psum - target| over the rounds that go
  on, min ||psum - target| - 1e-5| over every round) of every row -- how far the restatement's own branches are from flipping"""
  idx, dist = np.asarray(idx), np.asarray(dist, dtype=np.float64)
  N, K = dist.shape
  target = np.log2(K)
  table_mean = dist.sum() / (N * K)
  rho, sigma, weight = np.zeros(N), np.zeros(N), np.zeros((N, K))
  m_side, m_stop = np.inf, np.inf
  for i in range(N):
    d = dist[i]
    pos = d[d > 0]
    r = pos[0] if pos.size else 0.0
    lo, hi, mid = 0.0, np.inf, 1.0
    for _ in range(64):
      psum = 0.0
      for c in range(1, K):
        t = d[c] - r
        psum += np.exp(-(t / mid)) if t > 0 else 1.0
      m_stop = min(m_stop, abs(abs(psum - target) - 1e-5))
      if abs(psum - target) < 1e-5:
        break
      m_side = min(m_side, abs(psum - target))   # (the side is only looked at in a round that goes on)
      if psum > target:
        hi = mid
        mid = (lo + hi) / 2
      else:
        lo = mid
        mid = mid * 2 if hi == np.inf else (lo + hi) / 2
    row_sum = 0.0
    for c in range(K):
      row_sum += d[c]
    floor = 1e-3 * (row_sum / K) if r > 0 else 1e-3 * table_mean
    s = max(mid, floor)
    rho[i], sigma[i] = r, s
    for c in range(K):
      t = d[c] - r
      weight[i, c] = 0.0 if idx[i, c] == i else (1.0 if (t <= 0 or s == 0) else np.exp(-(t / s)))
  return (rho, sigma, weight, (m_side, m_stop)) if margins else (rho, sigma, weight)


def planted_matrix(n, G, seed, rank=12):
  """float32 [n, G] with the planted spectrum 30 . 2^(-k/2) on `rank` random directions, a little noise and a column offset"""
  rng = np.random.default_rng(seed)
  r = min(rank, G, n)
  U = rng.standard_normal((n, r))
  V = np.linalg.qr(rng.standard_normal((G, r)))[0]
  X = (U * (30.0 * 2.0 ** (-np.arange(r) / 2.0))) @ V.T + 0.01 * rng.standard_normal((n, G)) + rng.uniform(-5, 5, G)
  return X.astype(np.float32)
