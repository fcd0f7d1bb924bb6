"""Wall times of `SingleCellOMIC.clustering(algo='kmeans')` at the 8kly shape (4697 cells x 1998 genes, 12 clusters), dense and CSR
containers: the call end to end (two partial_fit batches of 4096 and 601 cells in the permuted order, then predict over all cells; host
draws, copies, the device), the device entries of the same call by themselves (the seeding of the first batch, one step, the
assignment of every cell), and scikit-learn's MiniBatchKMeans run the reference's way (partial_fit per batch, predict per batch) on the
same host (profiles/minibatch_kmeans_e2e.txt).
usage: python tools/minibatch_kmeans_timing.py [reps=5]"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sisua_amd import engine
from sisua_amd.clustering import BATCH_SIZE
from sisua_amd.data import SingleCellOMIC, synthetic_8kly

K = 12

def timed(f, reps):
  ts = []
  for _ in range(reps):
    t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)   # (every entry ends in a copy back: the device is idle)
  return ts, r

def show(ts):
  return f"min {min(ts) * 1e3:.1f} ms, median {np.median(ts) * 1e3:.1f} ms, max {max(ts) * 1e3:.1f} ms of {len(ts)}"

def reference_way(X, random_state=1):
  """scikit-learn as the reference drives it, on the batches of our reading of odin's batching"""
  from sklearn.cluster import MiniBatchKMeans
  n = X.shape[0]
  model = MiniBatchKMeans(n_clusters=K, max_iter=1000, n_init=3 * K, compute_labels=False, batch_size=BATCH_SIZE, random_state=random_state)
  starts = np.arange(0, n, BATCH_SIZE)
  for s in starts[np.random.RandomState(random_state).permutation(len(starts))]:
    model.partial_fit(X[s:s + BATCH_SIZE])
  return np.concatenate([model.predict(X[s:s + BATCH_SIZE]) for s in starts])

if __name__ == "__main__":
  reps = int(dict(a.split("=") for a in sys.argv[1:] if "=" in a).get("reps", 5))
  x, _ = synthetic_8kly()
  X = np.log1p(x / x.sum(1, keepdims=True) * 1e4).astype(np.float32)   # normalised expression, as the clusterings are run on
  N, G = X.shape
  print(f"{N} x {G}, {K} clusters, batches of {BATCH_SIZE}, sparsity {(X == 0).mean():.3f}; host threads "
        f"{os.environ.get('OMP_NUM_THREADS', '?')} (of {os.cpu_count()} CPUs)", flush=True)
  SingleCellOMIC(X[:512, :8]).clustering(n_clusters=3)   # (a first call: code objects)
  rng = np.random.RandomState(1)
  u = rng.uniform(size=(K - 1, 2 + int(np.log(K))))
  for name, M in (("dense", X), ("CSR", sp.csr_matrix(X))):
    ts, labels = timed(lambda: SingleCellOMIC(M).clustering(n_clusters=K), reps)
    print(f"{name}: clustering(algo='kmeans', n_clusters={K}) end to end: {show(ts)}; cluster sizes {np.bincount(labels, minlength=K).tolist()}", flush=True)
    block = M[:BATCH_SIZE]
    ts, seed = timed(lambda: engine.k_mbkmeans_seed(block, K, 7, u), reps)
    print(f"{name}: smx_mbkmeans_seed on {BATCH_SIZE} rows by itself: {show(ts)}", flush=True)
    ts, _ = timed(lambda: engine.k_mbkmeans_step(block, seed["centres"], np.zeros(K), want_labels=False), reps)
    print(f"{name}: smx_mbkmeans_step on {BATCH_SIZE} rows by itself: {show(ts)}", flush=True)
    ts, dev = timed(lambda: engine.k_mbkmeans_predict(M, seed["centres"]), reps)
    print(f"{name}: smx_mbkmeans_predict on all {N} rows by itself: {show(ts)}", flush=True)
    reference_way(M)   # (a first call: scikit-learn's thread pools)
    ts, ref = timed(lambda: reference_way(M), max(3, reps // 2))
    ours = SingleCellOMIC(M).clustering(n_clusters=K)
    print(f"{name}: scikit-learn's MiniBatchKMeans the reference's way on the host: {show(ts)}; labels equal ours: {np.array_equal(ref, ours)}", flush=True)
