#!/usr/bin/env python3
"""Wall time of SingleCellModel.imputation_scores (medians selected on the device, smx_impute.hip) against the route it replaces:
mean_over_samples() of the count distribution to the host, then the reference's NumPy lines (np.median over all entries, np.median per
cell).  One process, median of 5 runs after a warm-up, and the bytes that leave the device on each route.

usage: python tools/imputation_timing.py [out.txt]      (default: profiles/imputation_scores_e2e.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_route(original, corrupted, imputed):
  d = np.abs(original - imputed)
  cells = [np.median(r) for o, c, r in zip(original, corrupted, d) if np.sum(o) != np.sum(c)]
  return {"imputation_med": float(np.median(d)), "imputation_mean": float(np.mean(cells)) if cells else 0.0,
          "imputation_std": float(np.std(cells)) if cells else 0.0}


def timed(fn, n=5):
  fn()
  ts = []
  for _ in range(n):
    t0 = time.perf_counter()
    r = fn()
    ts.append((time.perf_counter() - t0) * 1e3)
  return r, ts


def main():
  import sisua_amd.models as M
  from sisua_amd.data import SingleCellOMIC, corrupt
  out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "imputation_scores_e2e.txt")
  lines = []
  for n, g, draws in ((8192, 1998, (1, 10)), (8192, 20000, (1,))):
    rng = np.random.default_rng(8)
    x = (rng.poisson(2.0, size=(n, g)) * (rng.uniform(size=(n, g)) < 0.1)).astype(np.float32)
    cor = x.copy()
    cor[: n // 2] = corrupt(x[: n // 2], dropout_rate=0.25, retain_rate=0.2, seed=8)
    sco = SingleCellOMIC(x, name="timing")
    m = M.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), latents=M.RVmeta(16, "diag", True, "Latents"),
              encoder=M.NetConf([128], batchnorm=True, dropout=0.1), decoder=M.NetConf([128], batchnorm=True, dropout=0.1))
    m.fit(sco.create_dataset(["transcriptomic"], batch_size=128, drop_remainder=True), metadata=sco, epochs=1, verbose=False)
    for S in draws:
      buf = np.empty((n, g), np.float32)

      def old():
        h = m._imputation_handle(cor, None, S, 128)
        return numpy_route(x, cor, h.count_distribution.mean_over_samples(out=buf))

      def old_copy_only():
        return m._imputation_handle(cor, None, S, 128).count_distribution.mean_over_samples(out=buf)

      new, t_new = timed(lambda: m.imputation_scores(cor, x, sample_shape=S, batch_size=128))
      _, t_copy = timed(old_copy_only)
      ref, t_old = timed(old)
      same = all(np.float64(new[k]).tobytes() == np.float64(ref[k]).tobytes() for k in ref)
      lines.append(f"shape {n} x {g}, S = {S}: scores {'identical' if same else 'DIFFER'} on the two routes: {new}")
      lines.append(f"  device route  model.imputation_scores:                 median {np.median(t_new):9.1f} ms  min {min(t_new):9.1f}  max {max(t_new):9.1f}  (n=5)"
                   f"  leaves the device: {n * 8 + (2048 + 2 * 1024 + 1 + 2 * 2 * 1024) * 8} bytes")
      lines.append(f"  parent route  mean_over_samples(out=buf) + NumPy lines: median {np.median(t_old):9.1f} ms  min {min(t_old):9.1f}  max {max(t_old):9.1f}  (n=5)"
                   f"  leaves the device: {n * g * 4} bytes")
      lines.append(f"    of which the walk and the [N, G] copy alone:          median {np.median(t_copy):9.1f} ms  min {min(t_copy):9.1f}  max {max(t_copy):9.1f}  (n=5)")
      print("\n".join(lines[-4:]), flush=True)
  with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
