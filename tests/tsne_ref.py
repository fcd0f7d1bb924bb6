"""float64 NumPy restatement of the t-SNE entries (include/sisua_hip.h: smx_tsne_affinities, smx_tsne_gradient, smx_tsne_fit; DESIGN.md
section 4x).  Plain loops and NumPy sums, written from the definitions and not from the kernels: what tests/test_gpu_tsne.py holds the
device to and tests/test_tsne_host.py holds to scikit-learn's private functions."""
import numpy as np
import scipy.sparse as sp

TOL = float(np.float32(1e-5))     # scikit-learn's PERPLEXITY_TOLERANCE, a float32 value
TINY = float(np.float32(1e-8))    # ... and its EPSILON_DBL
EXPLORE, CHECK = 250, 50


def probe_data(n, scale=1.0, seed=0, offset=8.0):
  """integer coordinates in [-6, 6] in 5 dims plus offset x (i mod 3) on every coordinate: three groups whose squared distances are exact
  in float32.  At the offset 8 the groups' boxes overlap (a few cells have their nearest neighbour in another group); from 13 on they are
  disjoint in every coordinate"""
  rng = np.random.default_rng(seed)
  X = rng.integers(-6, 7, size=(n, 5)).astype(np.float64) + float(offset) * (np.arange(n) % 3)[:, None]
  return (X * scale).astype(np.float32)


def support(n, perplexity):
  return min(n - 1, int(3.0 * perplexity + 1.0))


def affinity_rows(dist, perplexity, margins=False):
  """scikit-learn's _binary_search_perplexity on dist [N, k] (d2 = dist x dist) -> (cond_p [N, k], beta [N]); margins: also per row
  min ||H - target| - tol| over the rounds and min |H - target| over the rounds that go on -- how far the row's branches are from
  flipping"""
  dist = np.asarray(dist, dtype=np.float64)
  N, k = dist.shape
  target = np.log(float(np.float32(perplexity)))
  d2 = dist * dist
  P, used, margin = np.zeros((N, k)), np.ones(N), np.full(N, np.inf)
  beta, lo, hi = np.ones(N), np.full(N, -np.inf), np.full(N, np.inf)
  active = np.ones(N, bool)
  for _ in range(100):   # the rows that still search, side by side; every row's own sums run over its columns in order
    a = np.flatnonzero(active)
    if a.size == 0:
      break
    b = beta[a]
    p = np.exp(-d2[a] * b[:, None])
    s = np.cumsum(p, axis=1)[:, -1]   # (cumsum adds from the left, one term at a time)
    s[s == 0.0] = TINY
    p = p / s[:, None]
    sdp = np.cumsum(d2[a] * p, axis=1)[:, -1]
    diff = (np.log(s) + b * sdp) - target
    P[a], used[a] = p, b
    margin[a] = np.minimum(margin[a], np.abs(np.abs(diff) - TOL))
    go = np.abs(diff) > TOL
    active[a[~go]] = False
    a, b, diff = a[go], b[go], diff[go]
    margin[a] = np.minimum(margin[a], np.abs(diff))
    up = diff > 0.0
    au, ad, bu, bd = a[up], a[~up], b[up], b[~up]
    lo[au] = bu
    beta[au] = np.where(hi[au] == np.inf, bu * 2.0, (bu + hi[au]) / 2.0)
    hi[ad] = bd
    beta[ad] = np.where(lo[ad] == -np.inf, bd / 2.0, (bd + lo[ad]) / 2.0)
  return (P, used, margin) if margins else (P, used)


def joint(idx, cond_p):
  """P = (A + A^T) / sum(A + A^T), A the CSR of cond_p at (i, idx): float64 CSR, sorted columns, no explicit zeros"""
  N, k = idx.shape
  A = np.zeros((N, N))
  A[np.repeat(np.arange(N), k), np.asarray(idx).ravel()] = np.asarray(cond_p).ravel()
  S = sp.csr_matrix(A + A.T)
  S.eliminate_zeros()
  S.sort_indices()
  S.data = S.data / S.sum()
  S.eliminate_zeros()
  return S


def objective(P, Y, exaggeration=1.0, order=None, bounds=False):
  """-> (grad [N, C], KL, Z).  order: a permutation of the cells in which the sums over j are taken (None: ascending).  bounds: also
  (A [N, C] = 4 (sum_j |attractive term| + sum_j |repulsive term| / Z), B = sum p |log(p Z / w)|)"""
  Y = np.asarray(Y, dtype=np.float64)
  N, C = Y.shape
  order = np.arange(N) if order is None else np.asarray(order)
  sumw, rep, rep_abs = np.zeros(N), np.zeros((N, C)), np.zeros((N, C))
  for j in order:
    d = Y - Y[j]
    w = 1.0 / (1.0 + np.square(d).sum(axis=1))
    w[j] = 0.0
    sumw += w
    t = (w * w)[:, None] * d
    rep += t
    rep_abs += np.abs(t)
  Z = float(np.sum(sumw))
  rows = np.repeat(np.arange(N), np.diff(P.indptr))   # the entries of P, row by row in column order
  d = Y[rows] - Y[P.indices]
  w = 1.0 / (1.0 + np.square(d).sum(axis=1))
  t = ((exaggeration * P.data) * w)[:, None] * d
  att, att_abs = np.zeros((N, C)), np.zeros((N, C))
  np.add.at(att, rows, t)   # (unbuffered: the entries are added in their order)
  np.add.at(att_abs, rows, np.abs(t))
  terms = P.data * np.log((P.data * Z) / w)
  kl = float(np.sum(terms))
  grad = 4.0 * (att - rep / Z)
  if bounds:
    return grad, kl, Z, 4.0 * (att_abs + rep_abs / Z), float(np.sum(np.abs(terms)))
  return grad, kl, Z


def descent_step(Y, update, gains, grad, momentum, lr):
  """scikit-learn's _gradient_descent, the elementwise part, in place -> the gains-scaled gradient"""
  inc = update * grad < 0.0
  dec = np.invert(inc)
  gains[inc] += 0.2
  gains[dec] *= 0.8
  np.clip(gains, 0.01, np.inf, out=gains)
  grad = grad * gains
  update[...] = momentum * update - lr * grad
  Y += update
  return grad


def fit(P, Y0, max_iter=1000, early_exaggeration=12.0, learning_rate=200.0, min_grad_norm=1e-7, n_iter_without_progress=300, order=None):
  """the header's smx_tsne_fit -> dict(Y, update, gains, kl_trace [max_iter], n_iter)"""
  Y = np.array(Y0, dtype=np.float64)
  update, gains = np.zeros_like(Y), np.ones_like(Y)
  trace, it = np.full(max_iter, np.nan), 0
  for phase in range(2):
    if it >= max_iter:
      break
    end = min(EXPLORE, max_iter) if phase == 0 else max_iter
    update[...], gains[...] = 0.0, 1.0
    best, best_iter = np.finfo(float).max, it
    for i in range(it, end):
      convergence = (i + 1) % CHECK == 0
      grad, kl, _ = objective(P, Y, early_exaggeration if phase == 0 else 1.0, order)
      grad = descent_step(Y, update, gains, grad, 0.5 if phase == 0 else 0.8, learning_rate)
      it = i + 1
      if convergence or i == end - 1:
        trace[i] = kl
      if not convergence:
        continue
      if kl < best:
        best, best_iter = kl, i
      elif phase == 1 and i - best_iter > n_iter_without_progress:
        break
      if np.sqrt(np.sum(grad * grad)) <= min_grad_norm:
        break
  return dict(Y=Y, update=update, gains=gains, kl_trace=trace, n_iter=it)
