"""Step time of a VAE whose gene output is 'nb', 'normal' or 'bernoulli', at the 8kly shape (1998 genes, B 128, H 128, D 32: bench.py's
workload, its counts binarised for 'bernoulli' and log1p-scaled for 'normal') or at 128 x 20 000 (bench.py's c5-shard matrix, the same
transforms).  Timed as tools/dev/step_time.py times it: evaluation passes, 30 warm-up steps, then 300 steps staged and queued by ONE call,
three repetitions.
    python tools/output_kind_profile.py                        # every kind at both shapes
    python tools/output_kind_profile.py normal wide --reps 1   # one of them, e.g. for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/output_kind_profile.py bernoulli 8kly --reps 1"""
import argparse
import dataclasses
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def data(kind, shape):
  import bench
  cfg, x, b, extra = bench.build_workload(0, 1, "8kly" if shape == "8kly" else "c5-shard")
  extra.pop("cell_id_base", None)
  x = np.asarray(x)
  if kind == "bernoulli":
    x = (x > 0).astype(np.float32)
  elif kind == "normal":
    x = np.log1p(x).astype(np.float32)
  return dataclasses.replace(cfg, likelihood=kind), x, b, extra


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("kind", nargs="?", default=None, choices=("nb", "normal", "bernoulli"))
  ap.add_argument("shape", nargs="?", default=None, choices=("8kly", "wide"))
  ap.add_argument("--steps", type=int, default=300)
  ap.add_argument("--warmup", type=int, default=30)
  ap.add_argument("--reps", type=int, default=3)
  args = ap.parse_args()
  import bench
  from sisua_amd.engine import Engine
  for shape in ((args.shape,) if args.shape else ("8kly", "wide")):
    for kind in ((args.kind,) if args.kind else ("nb", "normal", "bernoulli")):
      cfg, x, b, extra = data(kind, shape)
      o = bench.make_order(x.shape[0], b, args.steps + args.warmup)
      e = Engine(cfg, max_batch=b, device=0)
      e.upload(x, storage="f32", **extra)
      for _ in range(50):
        e.eval_step(o[:b])
      e.train_steps(o[: args.warmup * b], args.warmup, b, graph=False)
      for _ in range(args.reps):
        e.stage_steps(o[args.warmup * b:], args.steps, b)
        e.synchronize()
        t = time.perf_counter()
        e.train_steps(None, args.steps, b, graph=False)
        e.synchronize()
        print("%s %s: %.1f us per step (%d steps of %d cells, %d genes; head_fused %s)" % (
            shape, kind, 1e6 * (time.perf_counter() - t) / args.steps, args.steps, b, x.shape[1], "on" if e.head_fused_bytes(b) else "off"), flush=True)
      e.close()


if __name__ == "__main__":
  main()
