"""End-to-end time of the probabilistic embedding of a protein panel [N, 12]: the device route (`ProbabilisticEmbedding.fit` + `predict_proba`:
all 12 x 8 restarts of the mixtures in one call of smx_gmm1d_fit, one call of smx_gmm1d_predict) against the route it replaces -- the
reference's settings on scikit-learn, one `GaussianMixture(2, covariance_type='diag', n_init=8, max_iter=120, random_state=8)` per column on
the reference's float32 normalisation, then `predict_proba` per column -- in one process.  Also the EM iterations in all and where the fit's
time goes: its launches (between two events around each iteration's pair) against the host round trips that read the stop flags.  Writes
(appends, one shape per call) profiles/probabilistic_embedding_e2e.txt.

  python tools/gmm_timing.py --cells 8192        device and host: median of 5 after a warm-up
  python tools/gmm_timing.py --cells 65536"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, K = 12, 2


def problem(N):
  """a synthetic two-population protein panel: counts, about a third of the cells in the high population, 30 % zeros in every other column"""
  rs = np.random.RandomState(3)
  cols = []
  for c in range(C):
    high = rs.uniform(size=N) < 0.35
    x = (rs.poisson(np.where(high, 180.0, 14.0) * rs.gamma(6.0, 1.0 / 6.0, size=N)) + 1).astype(np.float32)
    if c % 2:
      x[rs.uniform(size=N) < 0.3] = 0.0
    cols.append(x)
  return np.stack(cols, axis=1)


def host_sklearn(X):
  from sklearn.mixture import GaussianMixture
  out = np.empty(X.shape, np.float64)
  iters = 0
  for c in range(X.shape[1]):
    x = X[:, c]
    norm = lambda v: np.log1p(v / (np.sum(v) + np.finfo(np.float32).eps) * 10000)   # (float32 throughout, as the reference has it)
    tr = x[x > 0]
    tr = tr if tr.size == x.size else np.concatenate([np.zeros(1, np.float32), tr])
    with warnings.catch_warnings():
      warnings.simplefilter("ignore")
      gmm = GaussianMixture(K, covariance_type="diag", init_params="kmeans", n_init=8, max_iter=120, random_state=8).fit(norm(tr)[:, None])
    iters += gmm.n_iter_
    order = np.argsort(gmm.means_.ravel())
    out[:, c] = gmm.predict_proba(norm(x)[:, None]).T[order][1:].mean(axis=0)
  return out, iters


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
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probabilistic_embedding_e2e.txt"))
  a = ap.parse_args()
  from sisua_amd import ProbabilisticEmbedding
  from sisua_amd.engine import k_gmm1d_fit
  from sisua_amd.label_threshold import draw_init_raw
  N = a.cells
  X = problem(N)

  def device():
    pbe = ProbabilisticEmbedding().fit(X)
    return pbe, pbe.predict_proba(X)
  dev = timed(device)
  print(f"device route {dev[0] * 1e3:.2f} ms", flush=True)
  seeds = draw_init_raw(X, K, 8, 8)
  seed_t = timed(lambda: draw_init_raw(X, K, 8, 8))
  fit = timed(lambda: k_gmm1d_fit(X, seeds, stats=True))
  res = fit[3]
  st = res["stats"]
  pbe, prob = dev[3]
  pred = timed(lambda: pbe.predict_proba(X))
  try:
    import sklearn
    host = timed(lambda: host_sklearn(X))
    how = f"scikit-learn {sklearn.__version__}"
    diff = float(np.max(np.abs(host[3][0] - prob)))
  except ImportError:
    host, how, diff = None, "scikit-learn not importable: no host route", float("nan")
  lines = [f"{N} x {C}, {K} components, n_init = 8, max_iter = 120, tol = 1e-3; one process, {os.cpu_count()} CPUs visible, OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}",
           f"  device route (fit + predict_proba)     {dev[0] * 1e3:9.2f} ms [{dev[1] * 1e3:.2f} .. {dev[2] * 1e3:.2f}]   median of 5 after a warm-up",
           f"    of it: seeding on the host           {seed_t[0] * 1e3:9.2f} ms [{seed_t[1] * 1e3:.2f} .. {seed_t[2] * 1e3:.2f}]",
           f"           smx_gmm1d_fit, 96 jobs        {fit[0] * 1e3:9.2f} ms [{fit[1] * 1e3:.2f} .. {fit[2] * 1e3:.2f}]   {int(res['n_iter'].sum())} EM iterations in all, at most {int(res['n_iter'].max())} per job, {int(res['converged'].sum())} of {res['converged'].size} jobs converged",
           f"             its loop: {st['round_trips']} round trips, {st['launches']} launches in the call; {st['loop_ms']:.2f} ms, of which {st['kernel_ms']:.2f} ms ({st['kernel_ms'] / max(st['loop_ms'], 1e-9):.0%}) between the events around the launches and {st['loop_ms'] - st['kernel_ms']:.2f} ms in host round trips; the call {st['call_ms']:.2f} ms (the last of the timed calls)",
           f"           predict_proba                 {pred[0] * 1e3:9.2f} ms [{pred[1] * 1e3:.2f} .. {pred[2] * 1e3:.2f}]"]
  if host is not None:
    lines += [f"  host route ({how}, one GaussianMixture per column)  {host[0] * 1e3:9.2f} ms [{host[1] * 1e3:.2f} .. {host[2] * 1e3:.2f}]   median of 5 after a warm-up; {host[3][1]} EM iterations of its best restarts",
              f"  ratio host / device {host[0] / dev[0]:.2f} x",
              f"  largest |y_prob device - y_prob host| {diff:.3e}"]
  lines.append("")
  with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
  print("\n".join(lines))
