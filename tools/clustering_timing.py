"""End-to-end time of the clustering scores of a latent space [N, 32] with 12 classes: the device route (`sisua_amd.metrics.clustering_scores`:
silhouette sums and 200 k-means restarts on the device, the closing arithmetic on the host) against the route it replaces -- the latents on
the host, then scikit-learn's `silhouette_score` and `KMeans(12, n_init=200, random_state=5218)` with the three label scores, in one process.
Without scikit-learn the host side is the NumPy restatement tests/clustering_ref.py (chunked), and the file says so.  Writes (appends, one
shape per call) profiles/clustering_e2e.txt.

  python tools/clustering_timing.py --cells 8192 [--host-reps 5]     device: median of 5 after a warm-up; host: median of --host-reps
  python tools/clustering_timing.py --cells 65536 --host-reps 1      (the host route takes minutes at this size: one run, no warm-up)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, K = 32, 12


def problem(N):
  rs = np.random.RandomState(3)
  c = rs.randn(K, D) * 0.7
  y = rs.randint(0, K, N)
  return (c[y] + rs.randn(N, D)).astype(np.float32), y


def host_sklearn(Z, y):
  from sklearn.cluster import KMeans
  from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score, silhouette_score
  from sisua_amd.clustering import unsupervised_clustering_accuracy
  p = KMeans(K, n_init=200, random_state=5218).fit_predict(Z)
  return dict(ASW=float(silhouette_score(Z, y)), ARI=adjusted_rand_score(y, p), NMI=normalized_mutual_info_score(y, p),
              UCA=unsupervised_clustering_accuracy(y, p))


def host_numpy(Z, y):
  """the restatement's arithmetic in chunks of rows (the full N x N x D difference tensor does not fit at these sizes)"""
  from sisua_amd import clustering as C
  from tests import clustering_ref as R
  z = Z.astype(np.float64)
  N = z.shape[0]
  sums = np.zeros((N, K))
  onehot = np.eye(K)[y]
  for i0 in range(0, N, 256):
    d = np.sqrt(np.maximum(((z[i0:i0 + 256, None, :] - z[None, :, :]) ** 2).sum(-1), 0.0))
    sums[i0:i0 + 256] = d @ onehot
  cnt = np.bincount(y, minlength=K)
  a = sums[np.arange(N), y] / np.maximum(cnt[y] - 1, 1)
  mean = sums / cnt
  mean[np.arange(N), y] = np.inf
  asw = C.silhouette_from_sums(a, mean.min(1), cnt[y] == 1)[0]
  km = R.kmeans(Z, C.draw_init_idx(N, K, 200))
  p = km["labels_all"][km["best"]]
  return dict(ASW=asw, ARI=C.adjusted_rand(y, p), NMI=C.normalized_mutual_info(y, p), UCA=C.unsupervised_clustering_accuracy(y, p))


def timed(f, reps, warm):
  out = f() if warm else None
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    out = f()
    ts.append(time.perf_counter() - t0)
  return float(np.median(ts)), min(ts), max(ts), out


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--cells", type=int, default=8192)
  ap.add_argument("--host-reps", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clustering_e2e.txt"))
  a = ap.parse_args()
  from sisua_amd import metrics
  from sisua_amd.engine import k_cluster_kmeans, k_cluster_silhouette
  from sisua_amd.clustering import draw_init_idx
  N = a.cells
  Z, y = problem(N)
  dev = timed(lambda: metrics.clustering_scores(Z, y, K), 5, True)
  print(f"device route {dev[0] * 1e3:.2f} ms", flush=True)
  sil = timed(lambda: k_cluster_silhouette(Z, y, K), 5, True)
  idx = draw_init_idx(N, K, 200)
  km = timed(lambda: k_cluster_kmeans(Z, idx), 5, True)
  print(f"  silhouette {sil[0] * 1e3:.2f} ms, k-means {km[0] * 1e3:.2f} ms ({int(km[3]['n_iter'].sum())} assignments)", flush=True)
  try:
    import sklearn
    host_fn, how = host_sklearn, f"scikit-learn {sklearn.__version__}"
  except ImportError:
    host_fn, how = host_numpy, "scikit-learn not importable: the NumPy restatement (tests/clustering_ref.py), float64"
  warm = a.host_reps > 1
  host = timed(lambda: host_fn(Z, y), a.host_reps, warm)
  fmt = lambda s: ", ".join(f"{k} {v:.4f}" for k, v in s.items())
  lines = [f"{N} x {D}, {K} classes, n_init = 200, max_iter = 300; one process, {os.cpu_count()} CPUs visible, OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}",
           f"  device route (clustering_scores)      {dev[0] * 1e3:9.2f} ms [{dev[1] * 1e3:.2f} .. {dev[2] * 1e3:.2f}]   median of 5 after a warm-up",
           f"    of it: silhouette sums              {sil[0] * 1e3:9.2f} ms [{sil[1] * 1e3:.2f} .. {sil[2] * 1e3:.2f}]   (upload, two launches, download)",
           f"           k-means, 200 restarts        {km[0] * 1e3:9.2f} ms [{km[1] * 1e3:.2f} .. {km[2] * 1e3:.2f}]   {int(km[3]['n_iter'].sum())} assignments in all, at most {int(km[3]['n_iter'].max())} per restart",
           f"  host route ({how})  {host[0]:9.3f} s [{host[1]:.3f} .. {host[2]:.3f}]   " +
           (f"median of {a.host_reps} after a warm-up" if warm else "one run, no warm-up"),
           f"  ratio host / device {host[0] / dev[0]:.1f} x",
           f"  scores, device: {fmt(dev[3])}",
           f"  scores, host:   {fmt(host[3])}", ""]
  with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
  print("\n".join(lines))
