"""A NumPy float64 restatement of smx_gbt.hip (include/sisua_hip.h): scikit-learn's GradientBoostingClassifier
(loss='log_loss', criterion='friedman_mse', max_features=None, subsample=1.0, prior init, Newton leaf values, `x <= threshold` goes left)
with four stated deviations that make the result ONE answer, whatever the order of the sums:

  bins        a column (as float32) with at most 256 distinct values has one bin per value and scikit-learn's midpoints a/2 + b/2 (a where
              the midpoint rounds to b) as thresholds; a wider one is cut between the sorted positions p - 1 and p, p = floor(j N / 256),
              j = 1 .. 255, wherever the two values differ.
  statistics  the residual r = y_k - p_k and the curvature h = p_k (1 - p_k) are quantised to rint(v 2^40) as int64: every sum is exact.
  split rule  improvement = SL SL / nL + SR SR / nR - S S / n in float64 from the integers in that order; the largest wins, ties go to
              the lowest feature, then the lowest bin; only improvements > 0 split.
  leaf value  scale * sum r / sum h (0 where sum h is 0), scale = (K - 1) / K, or 1 for two classes.

A tree is kept in heap order: node t has the children 2 t + 1 and 2 t + 2, M = 2^(max_depth + 1) - 1 slots, a slot no cell reaches has n = 0;
feature = -1 marks a leaf (and an empty slot).  The device is held to this file, and this file to scikit-learn (tests/test_gbt_host.py)."""
import numpy as np

QUANTUM = 2.0 ** 40
MAX_BINS = 256
MAX_CELLS, MAX_FEATURES, MAX_CLASSES, MAX_DEPTH = 1 << 20, 32768, 32, 6


# ---- bins ---------------------------------------------------------------------------------------------------------------------------------
def bin_column(col):
  """col [N] (taken as float32) -> (thresholds float32 [n_thr <= 255], bins uint8 [N]): bin(x) <= b exactly where x <= thresholds[b]"""
  v = np.asarray(col, np.float32) + np.float32(0.0)   # (-0 as +0)
  N = v.shape[0]
  order = np.argsort(v, kind="stable")
  s = v[order]
  head = np.zeros(N, bool)
  head[1:] = s[1:] != s[:-1]
  if 1 + int(head.sum()) <= MAX_BINS:
    cut = head
  else:
    cut = np.zeros(N, bool)
    cut[(np.arange(1, MAX_BINS, dtype=np.int64) * N) // MAX_BINS] = True
    cut &= head
  pos = np.flatnonzero(cut)
  a, b = s[pos - 1], s[pos]
  thr = a * np.float32(0.5) + b * np.float32(0.5)
  thr = np.where(thr == b, a, thr).astype(np.float32)
  bins = np.empty(N, np.uint8)
  bins[order] = np.cumsum(cut)
  return thr, bins


def bin_matrix(X):
  """X [N, G] dense or scipy.sparse -> dict(thr float32 [G, 255] (zero behind n_thr), n_thr int32 [G], bins uint8 [G, N])"""
  X = np.asarray(X.todense() if hasattr(X, "todense") else X, np.float32)
  N, G = X.shape
  out = dict(thr=np.zeros((G, MAX_BINS - 1), np.float32), n_thr=np.zeros(G, np.int32), bins=np.zeros((G, N), np.uint8))
  for g in range(G):
    t, out["bins"][g] = bin_column(X[:, g])
    out["n_thr"][g] = len(t)
    out["thr"][g, :len(t)] = t
  return out


# ---- one stage's trees from integer statistics ---------------------------------------------------------------------------------------------
def n_slots(max_depth):
  return 2 ** (max_depth + 1) - 1


def empty_trees(shape, M):
  return dict(feature=np.full(shape + (M,), -1, np.int32), threshold=np.zeros(shape + (M,), np.float32),
              left=np.full(shape + (M,), -1, np.int32), right=np.full(shape + (M,), -1, np.int32), value=np.zeros(shape + (M,), np.float64),
              n=np.zeros(shape + (M,), np.int32), improvement=np.zeros(shape + (M,), np.float64), split_bin=np.full(shape + (M,), -1, np.int32))


def grow(B, q_r, q_h, max_depth=3, min_samples_split=2, min_samples_leaf=1, scale=1.0, margins=None):
  """B: bin_matrix's dict; q_r, q_h int64 [K, N] -> the K trees (arrays [K, M]) and `leaf` int32 [K, N], each cell's leaf slot.
  margins: a list that receives (best - second best) / best of every split node, the second best among the candidates whose sums
  differ from the best one's on both sides (the fit tests' tie check)."""
  bins, n_thr, thr = B["bins"], B["n_thr"], B["thr"]
  G, N = bins.shape
  q_r, q_h = np.asarray(q_r, np.int64).reshape(-1, N), np.asarray(q_h, np.int64).reshape(-1, N)
  K, M = q_r.shape[0], n_slots(max_depth)
  T = empty_trees((K,), M)
  leaf = np.zeros((K, N), np.int32)
  wide = bins.astype(np.int64)
  valid_bin = np.arange(MAX_BINS)[None, :] < n_thr[:, None]   # [G, 256]: a cut behind bin b exists
  for k in range(K):
    for level in range(max_depth + 1):
      base, L = 2 ** level - 1, 2 ** level
      loc = leaf[k] - base
      cells = np.flatnonzero(loc >= 0)   # (a cell in a leaf of an earlier level stays below base)
      if cells.size == 0:
        break
      cnt = np.bincount(loc[cells], minlength=L)
      Sr, Sh = np.zeros(L, np.int64), np.zeros(L, np.int64)
      np.add.at(Sr, loc[cells], q_r[k, cells])
      np.add.at(Sh, loc[cells], q_h[k, cells])
      hs, hc = np.zeros(G * L * MAX_BINS, np.int64), np.zeros(G * L * MAX_BINS, np.int64)
      if level < max_depth:
        idx = ((np.arange(G, dtype=np.int64)[:, None] * L + loc[cells][None, :]) * MAX_BINS + wide[:, cells]).ravel()
        np.add.at(hs, idx, np.broadcast_to(q_r[k, cells], (G, cells.size)).ravel())
        hc = np.bincount(idx, minlength=G * L * MAX_BINS)
      hs, hc = hs.reshape(G, L, MAX_BINS), hc.reshape(G, L, MAX_BINS)
      for j in range(L):
        t, n = base + j, int(cnt[j])
        if n == 0:
          continue
        T["n"][k, t] = n
        split = None
        if level < max_depth and n >= min_samples_split and n >= 2 * min_samples_leaf:
          SL, nL = np.cumsum(hs[:, j, :], axis=1), np.cumsum(hc[:, j, :], axis=1)
          SR, nR = Sr[j] - SL, n - nL
          ok = valid_bin & (np.minimum(nL, nR) >= min_samples_leaf)
          with np.errstate(divide="ignore", invalid="ignore"):
            SLf, SRf, Sf = SL.astype(np.float64), SR.astype(np.float64), np.float64(Sr[j])
            imp = (SLf * SLf / nL.astype(np.float64) + SRf * SRf / nR.astype(np.float64)) - Sf * Sf / np.float64(n)
          imp = np.where(ok, imp, -np.inf)
          flat = int(np.argmax(imp))           # (the first of equal maxima: the lowest feature, then the lowest bin)
          g, b = divmod(flat, MAX_BINS)
          if imp[g, b] > 0.0:
            split = (g, b, float(imp[g, b]))
            if margins is not None:
              same = ((SL == SL[g, b]) & (nL == nL[g, b])) | ((SR == SL[g, b]) & (nR == nL[g, b]))
              other = ok & ~same   # (the same integers on either side: the same cells cut apart, one candidate)
              second = np.max(np.where(other, imp, -np.inf))
              margins.append((imp[g, b] - second) / imp[g, b])
        if split is None:
          T["value"][k, t] = 0.0 if Sh[j] == 0 else scale * (np.float64(Sr[j]) / np.float64(Sh[j]))
          continue
        g, b, best = split
        T["feature"][k, t], T["split_bin"][k, t], T["threshold"][k, t] = g, b, thr[g, b]
        T["left"][k, t], T["right"][k, t] = 2 * t + 1, 2 * t + 2
        T["improvement"][k, t] = best * 2.0 ** -80
        mine = cells[loc[cells] == j]
        leaf[k, mine] = np.where(bins[g, mine] <= b, 2 * t + 1, 2 * t + 2)
  T["leaf"] = leaf
  return T


# ---- the stage loop -------------------------------------------------------------------------------------------------------------------------
def init_raw(y, K):
  """the prior's raw scores [Kz], as scikit-learn's DummyClassifier(strategy='prior') through the loss's link"""
  eps = np.finfo(np.float32).eps
  p = np.clip(np.bincount(y, minlength=K) / np.float64(len(y)), eps, 1 - eps)
  if K == 2:
    return np.array([np.log(p[1] / (1 - p[1]))])
  return np.log(p / np.exp(np.mean(np.log(p))))


def stats(raw, y, K):
  """raw [N, Kz], y [N] -> (q_r, q_h int64 [Kz, N], the losses [N])"""
  N = raw.shape[0]
  if K == 2:
    z = raw[:, 0]
    p = 1.0 / (1.0 + np.exp(-z))
    r, h = (y == 1).astype(np.float64) - p, p * (1.0 - p)
    loss = np.log1p(np.exp(-np.abs(z))) + np.maximum(z, 0.0) - (y == 1) * z
    r, h = r[None, :], h[None, :]
  else:
    m = raw.max(axis=1)
    e = np.exp(raw - m[:, None])
    s = np.zeros(N)
    for k in range(K):   # (in class order: NumPy's own sum is pairwise from 8 terms on)
      s = s + e[:, k]
    p = e / s[:, None]
    r, h = ((np.arange(K)[None, :] == y[:, None]).astype(np.float64) - p).T, (p * (1.0 - p)).T
    loss = (m + np.log(s)) - raw[np.arange(N), y]
  return np.rint(r * QUANTUM).astype(np.int64), np.rint(h * QUANTUM).astype(np.int64), loss


def holdout(y, K, validation_fraction, random_state):
  """-> (train rows, validation rows), both rising: per class in class order, the last ceil(fraction n_c) rows of a permutation of the
  class's rows drawn from ONE RandomState(random_state); at least one row of every class stays in training"""
  rs = np.random.RandomState(random_state)
  held = []
  for c in range(K):
    rows = rs.permutation(np.flatnonzero(y == c))
    n_hold = min(int(np.ceil(validation_fraction * rows.size)), rows.size - 1)
    held.append(rows[rows.size - n_hold:])
  val = np.sort(np.concatenate(held)).astype(np.int64)
  return np.setdiff1d(np.arange(len(y), dtype=np.int64), val), val


def should_stop(history, i, loss, tol):
  """scikit-learn's _fit_stages: `history` [n_iter_no_change] starts at +inf; -> True when stage i is the last one"""
  if np.any(loss + tol < history):
    history[i % len(history)] = loss
    return False
  return True


def tree_apply(T, X):
  """T: arrays [M] of one tree, X float32 [N, G] -> each row's leaf slot, by `x <= threshold` on the float32 values"""
  node = np.zeros(X.shape[0], np.int64)
  for _ in range(MAX_DEPTH + 1):
    f = T["feature"][node]
    go = f >= 0
    if not go.any():
      break
    x = X[np.arange(X.shape[0]), np.maximum(f, 0)]
    node = np.where(go, np.where(x <= T["threshold"][node], T["left"][node], T["right"][node]), node)
  return node


def decision(trees, init, learning_rate, X, n_stages=None):
  """the raw scores float64 [N, Kz] of X (dense or sparse, taken as float32): init, then stage by stage raw + learning_rate * value"""
  X = np.asarray(X.todense() if hasattr(X, "todense") else X, np.float32)
  S, Kz = trees["feature"].shape[:2]
  raw = np.tile(np.asarray(init, np.float64), (X.shape[0], 1))
  for s in range(S if n_stages is None else n_stages):
    for k in range(Kz):
      T = {a: trees[a][s, k] for a in ("feature", "threshold", "left", "right", "value")}
      raw[:, k] = raw[:, k] + learning_rate * T["value"][tree_apply(T, X)]
  return raw


def fit(X, y, K, n_estimators=100, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1, X_val=None, y_val=None,
        n_iter_no_change=None, tol=1e-4, margins=None):
  """-> dict(the tree arrays [n_estimators_, Kz, M], n_estimators_, train_score_ [n_estimators_], val_score [n_estimators_] or None, init
  [Kz], raw [N, Kz] the training rows' final scores).  Early stopping: (X_val, y_val) and n_iter_no_change given."""
  y = np.asarray(y, np.int64)
  Xd = np.asarray(X.todense() if hasattr(X, "todense") else X, np.float32)
  N = Xd.shape[0]
  Kz, M, factor = (1 if K == 2 else K), n_slots(max_depth), (2.0 if K == 2 else 1.0)
  scale = 1.0 if K == 2 else (K - 1.0) / K
  B = bin_matrix(Xd)
  init = init_raw(y, K)
  raw = np.tile(init, (N, 1))
  early = n_iter_no_change is not None
  if early:
    Xv = np.asarray(X_val.todense() if hasattr(X_val, "todense") else X_val, np.float32)
    yv, raw_v, history = np.asarray(y_val, np.int64), np.tile(init, (Xv.shape[0], 1)), np.full(n_iter_no_change, np.inf)
  stages, train_score, val_score = [], [], []
  for i in range(n_estimators):
    q_r, q_h, _ = stats(raw, y, K)
    T = grow(B, q_r, q_h, max_depth, min_samples_split, min_samples_leaf, scale, margins)
    for k in range(Kz):
      raw[:, k] = raw[:, k] + learning_rate * T["value"][k][T["leaf"][k]]
    stages.append(T)
    train_score.append(factor * (np.sum(stats(raw, y, K)[2]) / N))
    if early:
      for k in range(Kz):
        Tk = {a: T[a][k] for a in ("feature", "threshold", "left", "right", "value")}
        raw_v[:, k] = raw_v[:, k] + learning_rate * Tk["value"][tree_apply(Tk, Xv)]
      val_score.append(factor * (np.sum(stats(raw_v, yv, K)[2]) / Xv.shape[0]))
      if should_stop(history, i, val_score[-1], tol):
        break
  out = {a: np.stack([T[a] for T in stages]) for a in ("feature", "threshold", "left", "right", "value", "n", "improvement", "split_bin")}
  out.update(n_estimators_=len(stages), train_score_=np.array(train_score), val_score=np.array(val_score) if early else None, init=init,
             raw=raw, learning_rate=learning_rate)
  return out


def feature_importances(trees, G):
  """scikit-learn's rule: per tree with more than one node the improvements per feature over the root's n; the mean over those trees;
  normalised to sum 1 (zeros if no tree split)"""
  f, imp, n = (trees[a].reshape(-1, trees[a].shape[-1]) for a in ("feature", "improvement", "n"))
  rows = []
  for t in range(f.shape[0]):
    if f[t, 0] < 0:
      continue
    split = f[t] >= 0
    rows.append(np.bincount(f[t][split], weights=imp[t][split], minlength=G) / n[t, 0])
  if not rows:
    return np.zeros(G)
  avg = np.mean(rows, axis=0)
  return avg / avg.sum() if avg.sum() > 0 else np.zeros(G)


def quantile_codes(x, n_bins=10):
  """ordinal KBinsDiscretizer(n_bins, encode='ordinal', strategy='quantile') of one column: edges at the linear-interpolation percentiles,
  edges closer than 1e-8 merged, codes = searchsorted(edges[1:-1], x, side='right')"""
  x = np.asarray(x, np.float64)
  edges = np.percentile(x, np.linspace(0, 100, n_bins + 1))
  keep = np.ones(len(edges), bool)
  keep[1:] = np.ediff1d(edges) > 1e-8
  edges = edges[keep]
  return np.searchsorted(edges[1:-1], x, side="right").astype(np.int64)


# ---- the test matrices ----------------------------------------------------------------------------------------------------------------------
def make_matrix(N, G, seed):
  """float32 [N, G], the column kinds in a cycle of seven: 0 a normal rounded to 0.01 (more than 256 distinct values from about 500 rows on,
  with duplicates that straddle the quantile cuts; negative values), 1 Poisson(3) counts, 2 all zeros, 3 a constant, 4 a copy of column 1
  (identical bins: every tie between the two goes to column 1), 5 a continuous normal, 6 log1p of Poisson(20)"""
  rng = np.random.RandomState(seed)
  X = np.zeros((N, G), np.float32)
  for j in range(G):
    kind = j % 7
    if kind == 0:
      X[:, j] = np.round(rng.normal(size=N) * 100.0) / 100.0
    elif kind == 1:
      X[:, j] = rng.poisson(3.0, N)
    elif kind == 3:
      X[:, j] = 2.5
    elif kind == 4:
      X[:, j] = X[:, 1]
    elif kind == 5:
      X[:, j] = rng.normal(size=N)
    elif kind == 6:
      X[:, j] = np.log1p(rng.poisson(20.0, N))
  return X


def make_labels(X, K, seed, noise=1.0):
  """labels in 0 .. K - 1 that depend on the first columns of X, every class with a row"""
  rng = np.random.RandomState(seed + 1000)
  s = X[:, 0].astype(np.float64) + (0.3 * X[:, 1] if X.shape[1] > 1 else 0.0) + noise * rng.normal(size=X.shape[0])
  y = np.searchsorted(np.quantile(s, np.arange(1, K) / K), s).astype(np.int64)
  y[:K] = np.arange(K)
  return y
