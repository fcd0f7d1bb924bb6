"""Wall times of the UMAP path on the device: PCA-100 scores -> umap, split into kNN, connectivities, host preparation and the layout,
the time of one epoch and the pair evaluations per second (profiles/umap_e2e.txt).
usage: python tools/umap_timing.py [small] [large]
(default: both; one `rocprofv3 --kernel-trace --stats -- python tools/umap_timing.py small large` traces the same calls)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sisua_amd import engine, neighbors
from sisua_amd.data import SingleCellOMIC, synthetic_8kly, _counts

K = 12

def timed(f, reps=3):
  ts = []
  for _ in range(reps):
    t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)
  return min(ts), r

def pairs(eps, S, n_epochs, begin, end):
  """pair evaluations of the epochs begin .. end - 1, counted on the host from the schedule alone: activations + negatives"""
  eps = np.asarray(eps, np.float64)
  nxt, neg = eps.copy(), eps / S
  total = 0
  for n in range(end):
    idx = np.flatnonzero(nxt <= n)
    en = eps[idx] / S
    m = np.clip(np.trunc((n - neg[idx]) / en), 0, S * n_epochs)
    neg[idx] += m * en
    nxt[idx] += eps[idx]
    if n >= begin:
      total += idx.size + int(m.sum())
  return total

def device(name, x):
  om = SingleCellOMIC(x).normalize(total=True, log1p=True)
  s = om.dimension_reduce(n_components=100)
  n = s.shape[0]
  neighbors.umap(s[:512], n_epochs=10)   # (a first call: code objects)
  t_knn, (idx, dist) = timed(lambda: engine.k_knn(s, K - 1))
  tab = neighbors.self_table(idx, dist)
  t_rows, (_, _, w) = timed(lambda: engine.k_knn_umap(*tab))
  t_graph, (conn, _) = timed(lambda: neighbors.assemble_graph(tab[0], tab[1], w))
  E = neighbors.umap_n_epochs(n)
  t_prep, G = timed(lambda: neighbors.umap_prepare_graph(conn, 200))
  t_ab, (a, b) = timed(lambda: neighbors.find_ab_params(1.0, 0.5))
  t_init, Y0 = timed(lambda: neighbors.umap_normalise(neighbors.umap_init(n, 2, "pca", 1, s)))
  t_short, _ = timed(lambda: engine.k_umap_layout(G, Y0, 200, a, b, seed=1, epoch_end=50))
  t_long, _ = timed(lambda: engine.k_umap_layout(G, Y0, 200, a, b, seed=1))
  per_epoch = (t_long - t_short) / 150.0   # (uploads, allocation and the result cancel)
  work = pairs(G.data, 5, 200, 50, 200)
  t_all, Y = timed(lambda: neighbors.umap(s, n_neighbors=K), reps=1)
  print(f"{name}: umap(PCA-100 scores), n_neighbors {K}, {E} epochs: {t_all:.2f} s  [smx_knn {t_knn*1e3:.1f} ms, smx_knn_umap {t_rows*1e3:.1f} ms, "
        f"host assembly of the graph ({conn.nnz} entries) {t_graph*1e3:.1f} ms, cut and epochs_per_sample {t_prep*1e3:.1f} ms, curve_fit of a, b "
        f"{t_ab*1e3:.1f} ms, PCA init {t_init*1e3:.1f} ms]", flush=True)
  print(f"{name}: one epoch {per_epoch*1e3:.3f} ms (200 against 50 epochs of smx_umap_layout at n_epochs = 200: {t_long*1e3:.1f} and {t_short*1e3:.1f} ms; "
        f"{G.nnz} entries after the cut) = {work / 150.0 / per_epoch / 1e9:.3f} G pair evaluations / s ({work / 150.0:.0f} per epoch); "
        f"finite: {bool(np.isfinite(Y).all())}", flush=True)

if __name__ == "__main__":
  what = sys.argv[1:] or ["small", "large"]
  if "small" in what:
    device("4697 x 1998 (synthetic_8kly)", synthetic_8kly()[0])
  if "large" in what:
    device("131072 x 2000", _counts(131072, 2000, np.random.default_rng(9), 2.9, 0.28, 0.93))
