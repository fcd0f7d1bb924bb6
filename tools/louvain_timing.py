"""Wall times of `sisua_amd.louvain` on two graphs: the `neighbors()` graph of the 8kly shape (4697 cells, n_neighbors = 12: about 60 k
entries) and the symmetric 12-nearest-neighbour graph of 131 072 cells in 64 Gaussian blobs (10-D).  Per graph: the call end to end
(the host's checks, the copy, the device's whole multi-level loop, the labels back), the entry `engine.k_louvain` by itself, the entry
`engine.k_modularity` by itself (the same host checks and copy with four launches: what of the entry is NOT the loop), the levels, sweeps
and colours, and networkx's `louvain_communities` on the same host (profiles/louvain_e2e.txt).
usage: python tools/louvain_timing.py [reps=5] [big=131072] [nx_big=1]"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sisua_amd
from sisua_amd import communities, engine
from sisua_amd.data import SingleCellOMIC, synthetic_8kly


def timed(f, reps):
  ts = []
  for _ in range(reps):
    t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)   # (every entry ends in a copy back: the device is idle)
  return ts, r

def show(ts):
  return f"min {min(ts) * 1e3:.1f} ms, median {np.median(ts) * 1e3:.1f} ms, max {max(ts) * 1e3:.1f} ms of {len(ts)}"

def blob_graph(n, k=12, blobs=64, dims=10, seed=3):
  rng = np.random.RandomState(seed)
  x = (rng.normal(0.0, 3.0, (blobs, dims))[rng.randint(0, blobs, n)] + rng.normal(0.0, 1.0, (n, dims))).astype(np.float32)
  idx, _ = engine.k_knn(x, k)
  A = sp.csr_matrix((np.ones(n * k, np.float32), (np.repeat(np.arange(n), k), idx.reshape(-1))), shape=(n, n))
  return ((A + A.T) > 0).astype(np.float32).tocsr()

def measure(name, A, reps, with_networkx):
  n = A.shape[0]
  ip, cj, w, _ = communities.check_adjacency(A)
  print(f"{name}: {n} vertices, {A.nnz} entries, longest row {np.diff(A.indptr).max()}", flush=True)
  ts, (labels, info) = timed(lambda: sisua_amd.louvain(A, return_info=True), reps)
  print(f"{name}: louvain() end to end: {show(ts)}", flush=True)
  print(f"{name}: {info['n_communities']} communities, Q {info['modularity']:.6f}, levels {info['n_levels']}, sizes {info['level_size'].tolist()}, "
        f"sweeps {info['sweeps'].tolist()} (sum {int(info['sweeps'].sum())}), colours {info['colours'].tolist()}", flush=True)
  ts, _ = timed(lambda: communities.check_adjacency(A), reps)
  print(f"{name}: the Python layer's checks (canonical CSR, symmetry) by themselves: {show(ts)}", flush=True)
  ts, _ = timed(lambda: engine.k_louvain(ip, cj, w, n), reps)
  print(f"{name}: smx_louvain by itself (its checks, the copy, the loop): {show(ts)}", flush=True)
  ts, _ = timed(lambda: engine.k_modularity(ip, cj, w, n, labels), reps)
  print(f"{name}: smx_louvain_modularity by itself (the same checks and copy, four launches): {show(ts)}", flush=True)
  if with_networkx:
    import networkx as nx
    G = nx.from_scipy_sparse_array((A > 0).astype(np.float64))   # (unit weights on the support: the problem louvain() solves by default)
    ts, cs = timed(lambda: nx.community.louvain_communities(G, seed=0), 1 if n > 20000 else 3)
    lab = np.empty(n, np.int64)
    for i, c in enumerate(cs):
      lab[list(c)] = i
    print(f"{name}: networkx {nx.__version__} louvain_communities(seed=0) on the host: {show(ts)}; {len(cs)} communities, "
          f"Q {sisua_amd.modularity(A, lab):.6f}", flush=True)

if __name__ == "__main__":
  args = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
  reps, big, nx_big = int(args.get("reps", 5)), int(args.get("big", 131072)), int(args.get("nx_big", 1))
  print(f"host threads {os.environ.get('OMP_NUM_THREADS', '?')} (of {os.cpu_count()} CPUs); networkx's Louvain is one Python thread", flush=True)
  sisua_amd.louvain(blob_graph(2048))   # (a first call: code objects)
  x, _ = synthetic_8kly()
  X = np.log1p(x / x.sum(1, keepdims=True) * 1e4).astype(np.float32)
  A = SingleCellOMIC(X).neighbors(n_neighbors=12)[0]
  measure("8kly neighbors()", A, reps, True)
  if big > 0:
    measure(f"blobs {big}", blob_graph(big), reps, bool(nx_big))
