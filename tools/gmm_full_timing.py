"""End-to-end time of the Gaussian-mixture labels of a latent space [N, 32] with 12 classes: the device route
(`sisua_amd.clustering.mixture_labels`: 200 k-means restarts, then the full-covariance EM loop of smx_gmm_full_fit from the best partition
and its final E-step) against the route it replaces, scikit-learn's `GaussianMixture(12, random_state=5218).fit_predict` on the host, in one
process.  The device route is split into its k-means call, the EM loop and the final E-step (a call of smx_gmm_full_predict, which is that
launch with its upload and download); the loop's launches are counted against its host round trips (4 launches and one copy of the flags per
iteration, 4 launches and a copy for the start).  Writes (appends, one shape per call) profiles/gaussian_mixture_e2e.txt.

  python tools/gmm_full_timing.py --cells 8192        device and host: median of 5 after a warm-up
  python tools/gmm_full_timing.py --cells 65536"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, K = 32, 12


def problem(N):
  rs = np.random.RandomState(3)
  c = rs.randn(K, D) * 0.7
  y = rs.randint(0, K, N)
  return (c[y] + rs.randn(N, D)).astype(np.float32), y


def timed(f, reps=5):
  out = f()
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    out = f()
    ts.append(time.perf_counter() - t0)
  return float(np.median(ts)), min(ts), max(ts), out


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--cells", type=int, default=8192)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussian_mixture_e2e.txt"))
  a = ap.parse_args()
  from sisua_amd import clustering as C
  from sisua_amd.engine import k_cluster_kmeans, k_gmm_full_fit, k_gmm_full_predict
  from sisua_amd.mixture import starts_from_kmeans
  N = a.cells
  Z, y = problem(N)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    dev = timed(lambda: C.mixture_labels(Z, K))
  print(f"device route {dev[0] * 1e3:.2f} ms", flush=True)
  idx = C.draw_init_idx(N, K, 200)
  km = timed(lambda: k_cluster_kmeans(Z, idx, all_labels=True))
  start = starts_from_kmeans(km[3], 1)
  fit = timed(lambda: k_gmm_full_fit(Z, start, n_components=K))
  res = fit[3]
  n_iter = int(res["n_iter"][0])
  one = timed(lambda: k_gmm_full_fit(Z, start, n_components=K, max_iter=1))
  pred = timed(lambda: k_gmm_full_predict(Z, res["weights"], res["means"], res["chol_inv"]))
  per_iter = (fit[0] - one[0]) / max(n_iter - 1, 1)
  ari = lambda p: C.adjusted_rand(y, p)
  lines = [f"{N} x {D}, {K} components, full covariances, max_iter = 100, tol = 1e-3, reg_covar = 1e-6; one process, {os.cpu_count()} CPUs visible, OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}",
           f"  device route (mixture_labels)          {dev[0] * 1e3:9.2f} ms [{dev[1] * 1e3:.2f} .. {dev[2] * 1e3:.2f}]   median of 5 after a warm-up",
           f"    of it: k-means, 200 restarts         {km[0] * 1e3:9.2f} ms [{km[1] * 1e3:.2f} .. {km[2] * 1e3:.2f}]",
           f"           smx_gmm_full_fit, 1 restart   {fit[0] * 1e3:9.2f} ms [{fit[1] * 1e3:.2f} .. {fit[2] * 1e3:.2f}]   {n_iter} EM iterations, converged {int(res['converged'][0])}, lower bound {res['lower_bound'][0]:.6f}",
           f"             its loop: {4 + 4 * n_iter + 1} launches ({4 * n_iter} in the {n_iter} iterations) against {n_iter + 1} host round trips (one 8 R byte copy each); the same call held to one iteration {one[0] * 1e3:.2f} ms, so {per_iter * 1e3:.3f} ms per further iteration (E-step, three M-step launches, the copy)",
           f"           the final E-step alone (smx_gmm_full_predict: upload, one launch, download) {pred[0] * 1e3:9.2f} ms [{pred[1] * 1e3:.2f} .. {pred[2] * 1e3:.2f}]",
           f"    ARI against the true classes: mixture {ari(dev[3]['labels']):.4f}, k-means {ari(dev[3]['kmeans_labels']):.4f}"]
  try:
    import sklearn
    from sklearn.mixture import GaussianMixture
    z64 = Z.astype(np.float64)

    def host():
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm = GaussianMixture(K, random_state=5218)
        return gm.fit_predict(z64), gm
    h = timed(host)
    gm = h[3][1]
    lines += [f"  host route (scikit-learn {sklearn.__version__}, GaussianMixture({K}, random_state=5218).fit_predict)  {h[0] * 1e3:9.2f} ms [{h[1] * 1e3:.2f} .. {h[2] * 1e3:.2f}]   median of 5 after a warm-up; {gm.n_iter_} EM iterations from its k-means++ start, lower bound {gm.lower_bound_:.6f}, ARI {ari(h[3][0]):.4f}",
              f"  ratio host / device {h[0] / dev[0]:.2f} x (whole routes); host / (device EM call alone) {h[0] / fit[0]:.2f} x"]
  except ImportError:
    lines.append("  scikit-learn not importable: no host route")
  lines.append("")
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
  print("\n".join(lines))
