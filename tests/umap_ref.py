"""float64 NumPy restatement of the UMAP layout (include/sisua_hip.h: smx_umap_layout), written from the header
and not from the kernel: what tests/test_gpu_umap.py holds the device to.  `epoch` is the header's per-epoch form, vectorised over the
entries (NumPy rounds every operation, as the header asks); `layout_sequential` is umap-learn's literal in-place loop
(optimize_layout_euclidean: head and tail move, every later force sees the moved positions), in plain Python, which
tests/test_umap_host.py compares the per-epoch form with."""
import math
import random

import numpy as np
import scipy.sparse as sp

from oracle.sisua_oracle import philox4x32_10

ST_UMAP_NEG = 100


def blobs(n_per=100, groups=3, dim=10, sep=6.0, seed=0):
  """groups x n_per standard-normal cells in `dim` dimensions, the centre of group g at sep x e_g (unit vector g): every two groups are
  sqrt(2) sep apart.  Cell i belongs to group i mod groups -> float32 [groups n_per, dim]"""
  rng = np.random.default_rng(seed)
  n = n_per * groups
  X = rng.standard_normal((n, dim))
  X[np.arange(n), np.arange(n) % groups] += sep
  return X.astype(np.float32)


def prepare(graph, n_epochs):
  """the header's prepared graph: CSR float64 of e = max / w, sorted columns, the entries below max / n_epochs dropped"""
  G = sp.csr_matrix(graph, dtype=np.float64, copy=True)   # (sorting below must not reach the caller's arrays)
  G.sum_duplicates()
  G.sort_indices()
  top = G.data.max()
  G.data = np.where(G.data < top / float(n_epochs), 0.0, G.data)
  G.eliminate_zeros()
  G.data = top / G.data
  return G


def normalise(Y0):
  Y0 = np.asarray(Y0, dtype=np.float64)
  out = np.empty_like(Y0)
  for c in range(Y0.shape[1]):
    lo, hi = Y0[:, c].min(), Y0[:, c].max()
    out[:, c] = 5.0 if hi == lo else 10.0 * (Y0[:, c] - lo) / (hi - lo)
  return out


def start_state(eps, S):
  eps = np.asarray(eps, dtype=np.float64)
  return eps.copy(), (eps / float(S) if S > 0 else eps.copy())


def draws(entry, n, p, seed, n_cells):
  """k of negative p of entry `entry` in epoch n (arrays entry and p)"""
  w = philox4x32_10(entry, np.uint64(n), p >> 2, np.uint64(ST_UMAP_NEG), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
  sel = p & 3
  r = np.where(sel == 0, w[0], np.where(sel == 1, w[1], np.where(sel == 2, w[2], w[3]))).astype(np.uint64)
  return (r % np.uint64(n_cells)).astype(np.int64)


def _advance(eps, S, n_epochs, n, nxt, neg, idx=None):
  """the header's schedule step of epoch n, in place on nxt and neg -> m of the active entries idx (None: found here)"""
  dn = float(n)
  if idx is None:
    idx = np.flatnonzero(nxt <= dn)
  m = np.zeros(idx.size, np.int64)
  if S > 0:
    en = eps[idx] / float(S)
    md = np.trunc((dn - neg[idx]) / en)
    md = np.where(md > 0.0, md, 0.0)
    md = np.where(md < float(S) * float(n_epochs), md, float(S) * float(n_epochs))
    neg[idx] = neg[idx] + md * en
    m = md.astype(np.int64)
  nxt[idx] = nxt[idx] + eps[idx]
  return m


def state_at(eps, S, n_epochs, n, counts=False):
  """the schedule state (next_sample, next_negative) at the start of epoch n of a run from epoch 0; counts: also (activations, negatives)
  per entry over the epochs 0 .. n - 1"""
  eps = np.asarray(eps, dtype=np.float64)
  nxt, neg = start_state(eps, S)
  acts, negs = np.zeros(eps.size, np.int64), np.zeros(eps.size, np.int64)
  for e in range(n):
    idx = np.flatnonzero(nxt <= float(e))
    m = _advance(eps, S, n_epochs, e, nxt, neg, idx)
    acts[idx] += 1
    negs[idx] += m
  return (nxt, neg, acts, negs) if counts else (nxt, neg)


def _d2(d):
  s = d[:, 0] * d[:, 0]
  for c in range(1, d.shape[1]):
    s = s + d[:, c] * d[:, c]
  return s


def _clip(x):
  return np.minimum(4.0, np.maximum(-4.0, x))


def epoch(E, Y, n, n_epochs, a, b, gamma, alpha0, S, seed, nxt, neg, order=None, detail=False):
  """one epoch of the header from Y: returns the new Y; nxt and neg (the schedule state) are updated in place.  order: None -- the
  cell's terms are added attraction first, then the negatives by (entry, p); 'reverse'; or a numpy Generator for a random order.
  detail: also (A [N, C] = sum |term|, T [N] = the number of the cell's terms, m [entries] = the negatives drawn, -1 where inactive,
  d2 of every pair that a pow was taken of)"""
  Y = np.asarray(Y, dtype=np.float64)
  N, C = Y.shape
  indptr, cols, eps = E.indptr, E.indices.astype(np.int64), E.data
  rows = np.repeat(np.arange(N), np.diff(indptr))
  dn = float(n)
  alpha = alpha0 * (1.0 - dn / float(n_epochs))
  c_att, c_rep = (-2.0 * a) * b, (2.0 * gamma) * b
  idx = np.flatnonzero(nxt <= dn)
  # attraction
  j, k = rows[idx], cols[idx]
  d = Y[j] - Y[k]
  d2 = _d2(d)
  pos = d2 > 0.0
  t_att = np.zeros((idx.size, C))
  pb = np.power(d2[pos], b)
  g = (c_att * (pb / d2[pos])) / (a * pb + 1.0)
  t_att[pos] = 2.0 * _clip(g[:, None] * d[pos])
  pow_args = [d2[pos]]
  m = _advance(eps, S, n_epochs, n, nxt, neg, idx)
  # negatives
  ent = np.repeat(idx, m)
  p = np.arange(ent.size, dtype=np.int64) - np.repeat(np.cumsum(m) - m, m)
  kn = draws(ent.astype(np.uint64), n, p.astype(np.uint64), seed, N) if ent.size else np.zeros(0, np.int64)
  jn = rows[ent]
  d = Y[jn] - Y[kn]
  d2 = _d2(d) if ent.size else np.zeros(0)
  pos = d2 > 0.0
  t_neg = np.zeros((ent.size, C))
  pb = np.power(d2[pos], b)
  g = c_rep / ((0.001 + d2[pos]) * (a * pb + 1.0))
  t_neg[pos] = _clip(g[:, None] * d[pos])
  pow_args.append(d2[pos])
  who, terms = np.concatenate([j, jn]), np.concatenate([t_att, t_neg])
  if isinstance(order, str) and order == "reverse":
    who, terms = who[::-1], terms[::-1]
  elif order is not None:
    perm = order.permutation(who.size)
    who, terms = who[perm], terms[perm]
  acc = np.zeros((N, C))
  np.add.at(acc, who, terms)   # (unbuffered: the terms are added in their order)
  Ynew = Y + alpha * acc
  if not detail:
    return Ynew
  A = np.zeros((N, C))
  np.add.at(A, who, np.abs(terms))
  mm = np.full(eps.size, -1, np.int64)
  mm[idx] = m
  return Ynew, A, np.bincount(who, minlength=N), mm, np.concatenate(pow_args)


def layout(E, Y0, n_epochs, a, b, gamma=1.0, alpha0=1.0, S=5, seed=0, begin=0, end=None, nxt=None, neg=None, order=None):
  """the header's smx_umap_layout -> dict(Y, next_sample, next_negative)"""
  Y = np.array(Y0, dtype=np.float64)
  if nxt is None:
    nxt, neg = start_state(E.data, S)
  else:
    nxt, neg = np.array(nxt, dtype=np.float64), np.array(neg, dtype=np.float64)
  for n in range(begin, n_epochs if end is None else end):
    Y = epoch(E, Y, n, n_epochs, a, b, gamma, alpha0, S, seed, nxt, neg, order)
  return dict(Y=Y, next_sample=nxt, next_negative=neg)


def layout_sequential(E, Y0, n_epochs, a, b, gamma=1.0, alpha0=1.0, S=5, seed=0):
  """umap-learn's optimize_layout_euclidean (>= 0.5, move_other), the literal in-place loop over the entries in COO order; the negative
  samples come from random.Random(seed) in place of its tau_rand_int -> Y"""
  Y = [list(map(float, r)) for r in np.asarray(Y0, dtype=np.float64)]
  N, C = len(Y), len(Y[0])
  head = np.repeat(np.arange(N), np.diff(E.indptr)).tolist()
  tail = E.indices.tolist()
  eps = E.data.tolist()
  nxt = list(eps)
  eneg = [e / S for e in eps] if S > 0 else None
  nneg = list(eneg) if S > 0 else None
  rng = random.Random(seed)
  rc = range(C)
  for n in range(n_epochs):
    alpha = alpha0 * (1.0 - n / n_epochs)
    for i in range(len(eps)):
      if nxt[i] > n:
        continue
      cur, oth = Y[head[i]], Y[tail[i]]
      d2 = 0.0
      for c in rc:
        d2 += (cur[c] - oth[c]) ** 2
      g = (-2.0 * a * b * d2 ** (b - 1.0)) / (a * d2 ** b + 1.0) if d2 > 0.0 else 0.0
      for c in rc:
        gd = min(4.0, max(-4.0, g * (cur[c] - oth[c])))
        cur[c] += gd * alpha
        oth[c] -= gd * alpha
      nxt[i] += eps[i]
      if S == 0:
        continue
      m = int((n - nneg[i]) / eneg[i])
      for _ in range(m):
        k = rng.randrange(N)
        oth = Y[k]
        d2 = 0.0
        for c in rc:
          d2 += (cur[c] - oth[c]) ** 2
        if d2 > 0.0:
          g = (2.0 * gamma * b) / ((0.001 + d2) * (a * d2 ** b + 1.0))
          for c in rc:
            cur[c] += min(4.0, max(-4.0, g * (cur[c] - oth[c]))) * alpha
      nneg[i] += m * eneg[i]
  return np.array(Y)


def nearest_in_group(Y, group):
  """every cell's nearest other cell in Y is of its own group"""
  Y = np.asarray(Y, dtype=np.float64)
  d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
  np.fill_diagonal(d2, np.inf)
  return bool(np.array_equal(np.asarray(group)[np.argmin(d2, axis=1)], np.asarray(group)))
