"""Wall times of the t-SNE path on the device: PCA-100 scores -> tsne, split into kNN, affinities, host assembly and descent, the time
of one iteration and the pair evaluations per second of the repulsive sweep, with scikit-learn's TSNE(method='barnes_hut') on 16 host
threads beside them for orientation (profiles/tsne_e2e.txt).
usage: python tools/tsne_timing.py [small] [large] [host]
(default: all; `small large` alone is what one `rocprofv3 --kernel-trace --stats -- python tools/tsne_timing.py small large` traces)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sisua_amd import engine, neighbors
from sisua_amd.data import SingleCellOMIC, synthetic_8kly, _counts

PERPLEXITY = 30.0

def timed(f, reps=3):
  ts = []
  for _ in range(reps):
    t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)
  return min(ts), r

def device(name, x):
  om = SingleCellOMIC(x).normalize(total=True, log1p=True)
  s = om.dimension_reduce(n_components=100)
  n = s.shape[0]
  k = min(n - 1, int(3 * PERPLEXITY + 1))
  neighbors.tsne(s[:512], max_iter=10)   # (a first call: code objects)
  t_knn, (idx, dist) = timed(lambda: engine.k_knn(s, k))
  t_aff, (cond_p, _) = timed(lambda: engine.k_tsne_affinities(idx, dist, PERPLEXITY))
  t_host, P = timed(lambda: neighbors.joint_probabilities(idx, cond_p))
  t_init, Y0 = timed(lambda: neighbors.tsne_init(s, 2, "pca"))
  lr = max(n / 12.0 / 4.0, 50.0)
  t_short, _ = timed(lambda: engine.k_tsne_fit(P, Y0, 50, 12.0, lr))
  t_long, fit = timed(lambda: engine.k_tsne_fit(P, Y0, 250, 12.0, lr))
  per_iter = (t_long - t_short) / 200.0   # (uploads, allocation and the result cancel)
  t_grad, _ = timed(lambda: engine.k_tsne_gradient(P, Y0, 12.0))
  t_all, Y = timed(lambda: neighbors.tsne(s), reps=1)
  print(f"{name}: tsne(PCA-100 scores), perplexity {PERPLEXITY:g}, 1000 iterations: {t_all:.2f} s  [smx_knn (k = {k}) {t_knn*1e3:.1f} ms, "
        f"smx_tsne_affinities {t_aff*1e3:.1f} ms, host assembly of P ({P.nnz} entries) {t_host*1e3:.1f} ms, PCA init {t_init*1e3:.1f} ms, "
        f"descent {max(0.0, t_all - t_knn - t_aff - t_host - t_init):.2f} s]", flush=True)
  print(f"{name}: one iteration {per_iter*1e3:.3f} ms (250 against 50 iterations of smx_tsne_fit: {t_long*1e3:.1f} and {t_short*1e3:.1f} ms) = "
        f"{n * float(n) / per_iter / 1e9:.1f} G pair evaluations / s over the whole iteration; smx_tsne_gradient alone, with its copies, "
        f"{t_grad*1e3:.1f} ms; KL after 250 iterations {fit['kl_trace'][249]:.4f}", flush=True)
  return s

def host(name, s):
  from sklearn.manifold import TSNE
  t, _ = timed(lambda: TSNE(n_components=2, perplexity=PERPLEXITY, method="barnes_hut", init="pca", n_jobs=16).fit_transform(s), reps=1)
  print(f"{name} scikit-learn TSNE(method='barnes_hut'), 16 host threads, 1000 iterations: {t:.1f} s", flush=True)

if __name__ == "__main__":
  what = sys.argv[1:] or ["small", "large", "host"]
  mats = {}
  if "small" in what:
    mats["4697 x 1998 (synthetic_8kly)"] = synthetic_8kly()[0]
  if "large" in what:
    mats["32768 x 2000"] = _counts(32768, 2000, np.random.default_rng(9), 2.9, 0.28, 0.93)
  for name, x in mats.items():
    s = device(name, x)
    if "host" in what:
      host(name, s)
