"""A float64 / int64 NumPy restatement of the colour-synchronous Louvain method of smx_louvain.hip, and the
test graphs.  The device reproduces it label for label: every degree, total and internal weight is an int64 sum of quantised weights,
gains are float64 from those integers with every operation rounded once, ties go to the lowest community id, and the one float sum
(the modularity over community ids) runs in the halving order of smx_block.h."""
import numpy as np
import scipy.sparse as sp

QUANT = 1 << 30


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def mix32(v):
  """the fixed 32-bit mixer of the colouring's priorities"""
  x = np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
  m = np.uint64(0xFFFFFFFF)
  x ^= x >> np.uint64(16)
  x = (x * np.uint64(0x7FEB352D)) & m
  x ^= x >> np.uint64(15)
  x = (x * np.uint64(0x846CA68B)) & m
  x ^= x >> np.uint64(16)
  return x


def priority(n):
  """the colouring's order: vertices by decreasing (mix32(v), -v), as one uint64 key per vertex (greater = earlier)"""
  v = np.arange(n, dtype=np.uint64)
  return (mix32(v) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - v)


def quantise(adjacency, use_weights=False):
  """CSR (indptr, cols, q int64) of the support (stored zeros are no entries, as in sisua_amd.communities); q = rint(w / wmax * 2^30),
  unit weights 1; entries of q == 0 are dropped"""
  A = sp.csr_matrix(adjacency, copy=True)
  A.eliminate_zeros()
  indptr, cols = A.indptr.astype(np.int64), A.indices.astype(np.int64)
  if use_weights:
    w = A.data.astype(np.float64)
    wmax = w.max() if len(w) else 0.0
    q = np.rint(w / wmax * float(QUANT)).astype(np.int64) if wmax > 0 else np.zeros(len(w), np.int64)
  else:
    q = np.ones(len(cols), np.int64)
  keep = q != 0
  rows = np.repeat(np.arange(A.shape[0]), np.diff(indptr))[keep]
  indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))]).astype(np.int64)
  return indptr, cols[keep], q[keep]


def halving_sum(x):
  """smx_block.h's halving_column_sum: thread t adds x[t], x[t + 256], .. in order; a wave's lanes by halving; the waves (0 + 1) + (2 + 3)"""
  x = np.asarray(x, dtype=np.float64)
  acc = np.zeros(256, np.float64)
  for i in range(0, len(x), 256):
    c = x[i:i + 256]
    acc[:len(c)] += c
  w = acc.reshape(4, 64)
  for o in (32, 16, 8, 4, 2, 1):
    w = w[:, :o] + w[:, o:2 * o]
  return float((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))


def degrees(indptr, q):
  k = np.zeros(len(indptr) - 1, np.int64)
  np.add.at(k, np.repeat(np.arange(len(k)), np.diff(indptr)), q)
  return k


def partition_q(indptr, cols, q, comm, gamma, m2, k=None):
  """Q = sum_c (in_c / m2 - gamma (tot_c / m2)^2) over the ids 0 .. n - 1 in the halving order; a diagonal entry counts once in both"""
  n = len(indptr) - 1
  k = degrees(indptr, q) if k is None else k
  rows = np.repeat(np.arange(n), np.diff(indptr))
  inner = np.zeros(n, np.int64)
  same = comm[rows] == comm[cols]
  np.add.at(inner, comm[rows[same]], q[same])
  tot = np.zeros(n, np.int64)
  np.add.at(tot, comm, k)
  a = inner.astype(np.float64) / np.float64(m2)
  b = tot.astype(np.float64) / np.float64(m2)
  return halving_sum(a - np.float64(gamma) * (b * b))


def colouring(indptr, cols):
  """greedy in decreasing priority: the lowest colour no already coloured neighbour has; self loops are ignored"""
  n = len(indptr) - 1
  pr = priority(n)
  colour = np.full(n, -1, np.int64)
  for v in np.argsort(pr)[::-1]:
    nb = cols[indptr[v]:indptr[v + 1]]
    used = colour[nb[(nb != v) & (pr[nb] > pr[v])]]
    c = 0
    if len(used):
      seen = np.zeros(used.max() + 2, bool)
      seen[used] = True
      c = int(np.argmin(seen))
    colour[v] = c
  return colour


def run_level(indptr, cols, q, gamma, tol, max_sweeps, m2):
  """one level from singletons -> (comm, Q, sweeps, n_colours)"""
  n = len(indptr) - 1
  k = degrees(indptr, q)
  colour = colouring(indptr, cols)
  C = int(colour.max()) + 1
  classes = [np.flatnonzero(colour == c) for c in range(C)]
  comm, tot = np.arange(n, dtype=np.int64), k.copy()
  g, fm2 = np.float64(gamma), np.float64(m2)
  q_old = partition_q(indptr, cols, q, comm, gamma, m2, k)
  sweeps = 0
  while sweeps < max_sweeps:
    comm0, tot0 = comm.copy(), tot.copy()
    moved = 0
    for cls in classes:
      nxt = comm[cls].copy()
      for i, v in enumerate(cls):
        s, e = indptr[v], indptr[v + 1]
        nb, w = cols[s:e], q[s:e]
        other = nb != v
        if not other.any():
          continue
        ids, inv = np.unique(comm[nb[other]], return_inverse=True)
        kin = np.zeros(len(ids), np.int64)
        np.add.at(kin, inv, w[other])
        own = comm[v]
        kv = np.float64(k[v])
        kin_own = kin[ids == own].sum()
        g_own = np.float64(kin_own) - ((g * kv) * np.float64(tot[own] - k[v])) / fm2
        cand = ids != own
        if not cand.any():
          continue
        gain = kin[cand].astype(np.float64) - ((g * kv) * tot[ids[cand]].astype(np.float64)) / fm2
        b = int(np.argmax(gain))   # (ids ascend: the first maximum is the lowest id)
        if gain[b] > g_own:
          nxt[i] = ids[cand][b]
      for v, new in zip(cls, nxt):   # all moves of the colour, then tot
        if new != comm[v]:
          tot[comm[v]] -= k[v]
          tot[new] += k[v]
          comm[v] = new
          moved += 1
    sweeps += 1
    q_new = partition_q(indptr, cols, q, comm, gamma, m2, k)
    if q_new < q_old:
      comm, tot = comm0, tot0
      break
    gained, q_old = q_new - q_old, q_new
    if moved == 0 or gained <= tol:
      break
  return comm, q_old, sweeps, C


def relabel(comm):
  """community ids 0 .. in order of their lowest member"""
  _, first, inv = np.unique(comm, return_index=True, return_inverse=True)
  rank = np.empty(len(first), np.int64)
  rank[np.argsort(first, kind="stable")] = np.arange(len(first))
  return rank[inv]


def aggregate(indptr, cols, q, comm, nc):
  rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
  key = comm[rows] * nc + comm[cols]
  uk, inv = np.unique(key, return_inverse=True)
  val = np.zeros(len(uk), np.int64)
  np.add.at(val, inv, q)
  r, c = uk // nc, uk % nc
  ip = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nc))]).astype(np.int64)
  return ip, c.astype(np.int64), val


def order_by_size(labels):
  """final ids: by decreasing size, ties to the lowest member (= the lower id after `relabel`)"""
  size = np.bincount(labels)
  order = np.lexsort((np.arange(len(size)), -size))
  rank = np.empty(len(size), np.int64)
  rank[order] = np.arange(len(size))
  return rank[labels]


def louvain(adjacency, resolution=1.0, use_weights=False, tol=1e-7, max_sweeps=100, max_levels=32):
  """-> dict(labels int64 [n], n_communities, n_levels, modularity [n_levels], level_size [n_levels], sweeps [n_levels],
  colours [n_levels]); every level run is recorded, the last (which merges nothing) included"""
  indptr, cols, q = quantise(adjacency, use_weights)
  n = len(indptr) - 1
  m2 = int(q.sum())
  out = dict(labels=np.arange(n, dtype=np.int64), n_communities=n, n_levels=0, modularity=[], level_size=[], sweeps=[], colours=[])
  if m2 == 0:
    return _finish(out)
  labels = np.arange(n, dtype=np.int64)
  for _ in range(max_levels):
    nl = len(indptr) - 1
    comm, Q, sweeps, C = run_level(indptr, cols, q, resolution, tol, max_sweeps, m2)
    comm = relabel(comm)
    nc = int(comm.max()) + 1
    labels = comm[labels]
    out["modularity"].append(Q); out["level_size"].append(nc); out["sweeps"].append(sweeps); out["colours"].append(C)
    out["n_levels"] += 1
    if nc == nl:
      break
    indptr, cols, q = aggregate(indptr, cols, q, comm, nc)
  out["labels"] = order_by_size(labels)
  out["n_communities"] = int(labels.max()) + 1
  return _finish(out)


def _finish(out):
  for k, t in (("modularity", np.float64), ("level_size", np.int64), ("sweeps", np.int32), ("colours", np.int32)):
    out[k] = np.asarray(out[k], dtype=t)
  return out


def modularity(adjacency, labels, resolution=1.0, use_weights=False):
  indptr, cols, q = quantise(adjacency, use_weights)
  m2 = int(q.sum())
  if m2 == 0:
    return 0.0
  comm = np.unique(np.asarray(labels), return_inverse=True)[1].astype(np.int64)
  return partition_q(indptr, cols, q, comm, resolution, m2)


# ---- the engine's entries, restated (tests of the Python layer put these in their place) ---------------------------------------------
def k_louvain(indptr, cols, weights, n, resolution=1.0, tol=1e-7, max_sweeps=100, max_levels=32):
  A = sp.csr_matrix((np.ones(len(cols)) if weights is None else weights, cols, indptr), shape=(n, n))
  return louvain(A, resolution, weights is not None, tol, max_sweeps, max_levels)


def k_modularity(indptr, cols, weights, n, labels, resolution=1.0):
  A = sp.csr_matrix((np.ones(len(cols)) if weights is None else weights, cols, indptr), shape=(n, n))
  return modularity(A, labels, resolution, weights is not None)


# ---- test graphs ----------------------------------------------------------------------------------------------------------------------
BLOBS = {   # name: (blobs, cells per blob, dimensions, sd of the centres, k, seed)
    "clean": (6, 50, 8, 6.0, 12, 11),
    "touch": (5, 60, 4, 1.5, 10, 12),
    "cloud": (1, 300, 3, 0.0, 8, 13),
    "ragged": (7, 37, 6, 2.5, 5, 14),
    "wide": (10, 200, 10, 2.0, 12, 15),
}


def blob_cells(name):
  b, m, d, sd, _, seed = BLOBS[name]
  rng = np.random.RandomState(seed)
  centres = rng.normal(0.0, 1.0, (b, d)) * sd
  planted = np.repeat(np.arange(b), m)
  return (centres[planted] + rng.normal(0.0, 1.0, (b * m, d))).astype(np.float32), planted


def knn_graph(x, k, weighted=False):
  """the symmetric union of each cell's k nearest other cells; unit weights, or exp(-distance)"""
  x = np.asarray(x, np.float64)
  n = len(x)
  rows, cols = [], []
  for i in range(n):
    di = ((x - x[i]) ** 2).sum(-1)
    di[i] = np.inf
    nb = np.argsort(di, kind="stable")[:k]
    rows += [i] * k
    cols += list(nb)
  A = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
  A = ((A + A.T) > 0).astype(np.float64).tocsr()
  if weighted:
    r, c = A.nonzero()
    A = sp.csr_matrix((np.exp(-np.sqrt(((x[r] - x[c]) ** 2).sum(-1))), (r, c)), shape=(n, n))
  A.sort_indices()
  return A


def blob_graph(name, weighted=False):
  x, _ = blob_cells(name)
  return knn_graph(x, BLOBS[name][4], weighted)


def _cliques(sizes, n_extra=0):
  n = sum(sizes) + n_extra
  A = sp.lil_matrix((n, n))
  s = 0
  for m in sizes:
    A[s:s + m, s:s + m] = 1.0
    s += m
  A.setdiag(0.0)
  return A


def ring_of_cliques(n_cliques=30, size=5):
  A = _cliques([size] * n_cliques)
  for c in range(n_cliques):
    a, b = c * size, ((c + 1) % n_cliques) * size + 1
    A[a, b] = A[b, a] = 1.0
  A = A.tocsr(); A.eliminate_zeros()
  return A


def two_cliques_and_isolated():
  A = _cliques([7, 5], n_extra=3).tocsr(); A.eliminate_zeros()
  return A


def hub_graph(n_cliques=40, size=128):
  """vertex 0 joined to every vertex of n_cliques cliques of `size`"""
  n = 1 + n_cliques * size
  blocks = sp.block_diag([np.ones((size, size)) - np.eye(size)] * n_cliques, format="csr")
  A = sp.bmat([[None, np.ones((1, n - 1))], [np.ones((n - 1, 1)), blocks]], format="csr")
  A.eliminate_zeros()
  A.sort_indices()
  return A


def empty_graph(n=9):
  return sp.csr_matrix((n, n), dtype=np.float64)


def blob_cases():
  """the blob cases: (name, adjacency, use_weights, gamma) -- the five unit graphs at gamma = 1, weighted "touch" at gamma 0.5, 1 and 2,
  and unit "touch" at gamma 0.5 and 2"""
  out = [(name, blob_graph(name), False, 1.0) for name in BLOBS]
  out += [(f"touch_w_g{g}", blob_graph("touch", weighted=True), True, g) for g in (0.5, 1.0, 2.0)]
  out += [(f"touch_g{g}", blob_graph("touch"), False, g) for g in (0.5, 2.0)]
  return out
