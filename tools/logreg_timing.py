"""Wall times of `sisua_amd.LogisticRegression` on the log-normalised 4697 x 1998 benchmark matrix with 12 classes from
`SingleCellOMIC.clustering(n_clusters=12)` (MiniBatchKMeans), dense and CSR, tol = 1e-4: the fit end to end (the host's checks, the copy of
the matrix, the whole L-BFGS solve on the device, the coefficients back), `rank_genes_groups_logreg` end to end, one evaluation
(`engine.k_logreg_eval`: the same checks and copy with four launches -- what of the entry is NOT the solve), the iterations, evaluations
and launches per iteration, and scikit-learn on the same host with `lbfgs` (tol = 1e-4) and with the reference's `saga`
(profiles/logreg_e2e.txt).  The objective of every solution is recomputed here in float64.
usage: python tools/logreg_timing.py [reps=5] [sk_reps=1] [saga_epochs=1000]"""
import os, sys, time, warnings
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sisua_amd
from sisua_amd import engine
from sisua_amd.data import SingleCellOMIC, synthetic_8kly


def timed(f, reps):
  ts = []
  for _ in range(reps):
    t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)   # (every entry ends in a copy back: the device is idle)
  return ts, r

def show(ts):
  return f"min {min(ts) * 1e3:.1f} ms, median {np.median(ts) * 1e3:.1f} ms, max {max(ts) * 1e3:.1f} ms of {len(ts)}"

def objective(X64, y, W, b):
  """the mean-form objective at C = 1 and max|g|, float64 NumPy"""
  N = len(y)
  Z = X64 @ W.T + b
  m = Z.max(1)
  E = np.exp(Z - m[:, None])
  s = E.sum(1)
  R = E / s[:, None]
  R[np.arange(N), y] -= 1.0
  F = (m + np.log(s) - Z[np.arange(N), y]).sum() / N + (W * W).sum() / (2.0 * N)
  return F, max(np.abs(R.T @ X64 / N + W / N).max(), np.abs(R.sum(0) / N).max())

if __name__ == "__main__":
  args = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
  reps, sk_reps, saga_epochs = int(args.get("reps", 5)), int(args.get("sk_reps", 1)), int(args.get("saga_epochs", 1000))
  print(f"host threads {os.environ.get('OMP_NUM_THREADS', '?')} (of {os.cpu_count()} CPUs)", flush=True)
  x, _ = synthetic_8kly()
  X = np.log1p(x / x.sum(1, keepdims=True) * 1e4).astype(np.float32)
  y = np.unique(SingleCellOMIC(X).clustering(n_clusters=12), return_inverse=True)[1].astype(np.int32)
  K, X64 = int(y.max()) + 1, X.astype(np.float64)
  print(f"matrix {X.shape}, {K} classes of sizes {np.bincount(y).tolist()}, {100.0 * (X != 0).mean():.1f} % non-zero", flush=True)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    sisua_amd.LogisticRegression(max_iter=2).fit(X[:512], y[:512] % 3)   # (a first call: code objects)
  for name, M in (("dense", X), ("CSR", sp.csr_matrix(X))):
    ts, m = timed(lambda: sisua_amd.LogisticRegression(tol=1e-4, max_iter=1000).fit(M, y), reps)
    it, ev = int(m.n_iter_[0]), m.n_eval_
    launches = 4 * ev + (ev - 1) + 3 * it + 1   # an evaluation's four, a trial's step, per iteration the direction, the pair and the dot products
    F, gmax = objective(X64, y, m.coef_, m.intercept_)
    print(f"{name}: LogisticRegression(tol=1e-4).fit end to end: {show(ts)}", flush=True)
    print(f"{name}: {it} iterations, {ev} evaluations, {launches} launches = {launches / max(it, 1):.2f} per iteration; device max|g| {m.max_grad_:.3e}; "
          f"recomputed F {F:.12f}, max|g| {gmax:.3e}", flush=True)
    ts, _ = timed(lambda: engine.k_logreg_eval(M, y, K, m.coef_, m.intercept_), reps)
    print(f"{name}: smx_logreg_eval by itself (the same checks and copy, four launches): {show(ts)}", flush=True)
    ts, _ = timed(lambda: sisua_amd.rank_genes_groups_logreg(M, y, tol=1e-4, max_iter=1000), reps)
    print(f"{name}: rank_genes_groups_logreg end to end: {show(ts)}", flush=True)
    ts, _ = timed(lambda: m.decision_function(M), reps)
    print(f"{name}: decision_function: {show(ts)}", flush=True)
  ours = m.coef_
  import sklearn
  from sklearn.linear_model import LogisticRegression as Sk
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    ts, sk = timed(lambda: Sk(C=1.0, tol=1e-4, max_iter=1000, solver="lbfgs").fit(X, y), sk_reps)
    F, gmax = objective(X64, y, sk.coef_, sk.intercept_)
    print(f"scikit-learn {sklearn.__version__} lbfgs(tol=1e-4, max_iter=1000) on the float32 matrix, this host: {show(ts)}; {int(sk.n_iter_[0])} iterations; "
          f"recomputed F {F:.12f}, max|g| {gmax:.3e}; max |coef - ours| {np.abs(sk.coef_ - ours).max():.3e}", flush=True)
    if saga_epochs > 0:
      ts, sk = timed(lambda: Sk(C=1.0, max_iter=saga_epochs, solver="saga").fit(X, y), 1)
      F, gmax = objective(X64, y, sk.coef_, sk.intercept_)
      note = "the reference's setting" if saga_epochs == 1000 else "the reference's setting is max_iter=1000: NOT run here"
      print(f"scikit-learn saga(max_iter={saga_epochs}; {note}), this host: {show(ts)}; {int(sk.n_iter_[0])} epochs; "
            f"recomputed F {F:.12f}, max|g| {gmax:.3e}; max |coef - ours| {np.abs(sk.coef_ - ours).max():.3e}", flush=True)
