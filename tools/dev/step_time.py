#!/usr/bin/env python3
"""Microseconds per optimiser step of a bench workload, timed as bench.py times it (evaluation passes to bring the clocks up, warm-up steps, the
timed steps' ids staged, all of them queued by ONE library call) -- without the rest of the bench line: the quick A/B of a knob or a build.
    SMX_TUNING=no_fold_dz python tools/dev/step_time.py 8kly            # knobs: docs/LAB_NOTES.md
    python tools/dev/step_time.py c5-shard --storage u16 --steps 100
    python tools/dev/step_time.py 8kly --draws 4                           # fit(sample_shape=4): 4 x 128 stacked rows per step
    python tools/dev/step_time.py 8kly --latent both                       # 'diag' and 'mvntril' at the workload's D, alternately
Prints three repetitions; under rocprofv3 (`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/dev/step_time.py ...`)
`tools/prof_summary.py DIR` gives the per-kernel table and one step's timeline."""
import argparse
import dataclasses
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("workload", nargs="?", default="8kly")
  ap.add_argument("--storage", default=None, help="f32 / u16 / csr (default: f32, u16 at the c5-shard width as bench.py's secondary entry)")
  ap.add_argument("--steps", type=int, default=0)
  ap.add_argument("--warmup", type=int, default=30)
  ap.add_argument("--draws", type=int, default=1, help="Monte-Carlo draws per cell (fit(sample_shape), smx_set_train_draws)")
  ap.add_argument("--latent", default="diag", choices=("diag", "mvntril", "both"),
                  help="latent posterior at the workload's latent_dim: the diagonal Gaussian, the full-covariance one, or both alternately")
  args = ap.parse_args()
  import bench
  from sisua_amd.engine import Engine
  cfg, x, b, extra = bench.build_workload(0, 1, args.workload)
  extra.pop("cell_id_base", None)
  steps = args.steps or (100 if args.workload.startswith("c5") else 300)
  o = bench.make_order(x.shape[0], b, steps + args.warmup)
  runs = []
  for kind in (("diag", "mvntril") if args.latent == "both" else (args.latent,)):
    e = Engine(dataclasses.replace(cfg, latent_tril=kind == "mvntril"), max_batch=b, device=0)
    e.set_train_draws(args.draws)
    e.upload(x, storage=args.storage or ("u16" if args.workload.startswith("c5") else "f32"), **extra)
    for _ in range(50):
      e.eval_step(o[:b])
    e.train_steps(o[: args.warmup * b], args.warmup, b, graph=False)
    runs.append((kind, e))
  for _ in range(3):
    for kind, e in runs:
      e.stage_steps(o[args.warmup * b:], steps, b)
      e.synchronize()
      t = time.perf_counter()
      e.train_steps(None, steps, b, graph=False)
      e.synchronize()
      name = args.workload if args.latent == "diag" else "%s (%s latent)" % (args.workload, kind)
      print("%s: %.1f us per step (%d steps of %d cells, %d draws)" % (name, 1e6 * (time.perf_counter() - t) / steps, steps, b, args.draws),
            flush=True)
  for _, e in runs:
    e.close()


if __name__ == "__main__":
  main()
