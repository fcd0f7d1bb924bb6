"""End-to-end time of the gene x protein correlation matrices: the device route (Engine.predict_correlate + the closing arithmetic) against
the route without it (the [N, G] mean to the host, then one pearsonr and one spearmanr per pair in one process).  VAE / zinb, hidden 128,
batch 128, 12 proteins; median of 5 calls after a warm-up, with ranges.  Writes profiles/correlation_e2e.txt.

  python tools/correlation_timing.py                   the table (the SciPy loop runs once per shape, on `--genes` genes scaled to all at
                                                       the wide shape: it takes seconds to minutes, its noise does not matter)
  python tools/correlation_timing.py --once 1998 1     one device call, to run under `rocprofv3 --kernel-trace --stats`
  python tools/correlation_timing.py --split DIR       walk / rank / correlate split from the kernel statistics written under DIR"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, P = 8192, 12
OURS = {"col_rank2_kernel": "rank", "col_correlate_kernel": "correlate", "keep_cols_kernel": "keep"}


def problem(G):
  from sisua_amd.config import ModelConfig
  from sisua_amd.engine import Engine
  rng = np.random.default_rng(0)
  x = (rng.poisson(2.0, size=(N, G)) * (rng.uniform(size=(N, G)) < 0.15)).astype(np.float32)
  prot = rng.poisson(rng.uniform(2.0, 40.0, size=P), size=(N, P)).astype(np.float64)
  e = Engine(ModelConfig(model="vae", n_genes=G, likelihood="zinb", enc_units=(128,), dec_units=(128,), latent_dim=16), max_batch=512)
  return e, x, prot


def device_route(e, x, prot, S):
  from sisua_amd.distributions import correlations_from_sums, protein_operands
  ops = protein_operands(prot)
  r = e.predict_correlate(x, ops["rank2"], ops["unit"], n_samples=S, batch=128, count_only=True)
  return correlations_from_sums(N, r["sp_Sa"], r["sp_Saa"], r["sp_Sab"], ops["Sb"], ops["Sbb"], r["pe_Sxx"], r["pe_Sxy"], r["nonfinite"], ops["constant"])


def scipy_loop(mean, prot, genes):
  from scipy.stats import pearsonr, spearmanr
  for g in genes:
    for p in range(prot.shape[1]):
      pearsonr(mean[:, g], prot[:, p])
      spearmanr(mean[:, g], prot[:, p], nan_policy="omit")


def med(f, reps=5):
  f()
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    f()
    ts.append(time.perf_counter() - t0)
  return float(np.median(ts)), min(ts), max(ts)


def table(n_sub):
  lines = [f"N = {N} cells, P = {P} proteins, VAE / zinb, hidden 128, batch 128, one process; median of 5 after a warm-up [min .. max]", ""]
  for G, S in ((1998, 1), (1998, 10), (20000, 1)):
    e, x, prot = problem(G)
    buf = np.empty((N, G), np.float32)
    dev = med(lambda: device_route(e, x, prot, S))
    down = med(lambda: e.predict_stat(x, "mean_over_samples", n_samples=S, batch=128, count_only=True, out=buf))
    genes = range(G) if G <= 2000 else range(0, G, G // n_sub)
    t0 = time.perf_counter()
    scipy_loop(buf, prot, genes)
    sci = (time.perf_counter() - t0) * G / len(genes)
    how = "all pairs, one run" if len(genes) == G else f"{len(genes)} genes (every {G // n_sub}th), one run, scaled to {G}"
    new_b, old_b = G * ((2 + P) * 16 + 4), N * G * 4
    lines += [f"{N} x {G} x {P}, S = {S}",
              f"  device route (ranks + sums on the device, closing on the host)  {dev[0] * 1e3:9.1f} ms [{dev[1] * 1e3:.1f} .. {dev[2] * 1e3:.1f}]",
              f"  host route: mean_over_samples(out=buf) to the host             {down[0] * 1e3:9.1f} ms [{down[1] * 1e3:.1f} .. {down[2] * 1e3:.1f}]",
              f"              + SciPy loop ({how})  {sci:9.1f} s",
              f"  speed-up {(down[0] + sci) / dev[0]:.0f} x;  bytes off the device {new_b} / {old_b} ({old_b / new_b:.0f} x fewer)", ""]
    print("\n".join(lines[-6:]), flush=True)
    e.close()
  return lines


def split(d):
  files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
  if not files:
    return [f"no kernel statistics under {d}"]
  tot = {"walk": 0.0, "keep": 0.0, "rank": 0.0, "correlate": 0.0}
  for row in csv.DictReader(open(files[0])):
    part = next((v for k, v in OURS.items() if k in row["Name"]), "walk")
    tot[part] += float(row["TotalDurationNs"]) * 1e-6
  return ["kernel time of one call at 8192 x 1998 x 12, S = 1 (rocprofv3 --kernel-trace --stats): " +
          ", ".join(f"{k} {v:.2f} ms" for k, v in tot.items())]


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--once", nargs=2, type=int, metavar=("G", "S"))
  ap.add_argument("--split")
  ap.add_argument("--genes", type=int, default=100)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlation_e2e.txt"))
  a = ap.parse_args()
  if a.once:
    e, x, prot = problem(a.once[0])
    device_route(e, x, prot, a.once[1])
    e.close()
  else:
    lines = split(a.split) if a.split else table(a.genes)
    with open(a.out, "a" if a.split else "w") as f:
      f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
