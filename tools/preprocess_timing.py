"""Wall time of the loaders' preprocessing chain -- filter_cells(min_counts=1), filter_genes(min_cells=3), normalize(total=True,
log1p=True), filter_highly_variable_genes(n_top_genes) -- on a SingleCellOMIC: the device route (smx_prep.hip behind the container's
methods) against the NumPy restatement of the same chain (tests/preprocess_ref.py, dense float32 / float64 on the host), in one process.
Each stage of the device route is timed too.  Every stage moves the matrix over PCIe once or twice, so this is a measurement of copies
more than of kernels.  Writes (appends) profiles/preprocess_e2e.txt.

  python tools/preprocess_timing.py                     the 4697 x 1998 benchmark matrix, dense and CSR
  python tools/preprocess_timing.py --cells 32768 --genes 4000 --density 0.07      one larger CSR matrix"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(f, reps):
  f()
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    out = f()
    ts.append(time.perf_counter() - t0)
  return float(np.median(ts)), min(ts), max(ts), out


def big_csr(n, g, density, seed=3):
  rng = np.random.default_rng(seed)
  keep = rng.uniform(size=g) ** 3 * 3 * density   # per-gene density: a few dense genes, many sparse ones
  rows, cols = [], []
  for j in range(g):
    r = np.flatnonzero(rng.uniform(size=n) < min(keep[j], 0.9))
    rows.append(r)
    cols.append(np.full(len(r), j))
  rows, cols = np.concatenate(rows), np.concatenate(cols)
  return sp.csr_matrix((rng.geometric(0.4, size=len(rows)).astype(np.float32), (rows, cols)), shape=(n, g))


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--cells", type=int, default=0)
  ap.add_argument("--genes", type=int, default=4000)
  ap.add_argument("--density", type=float, default=0.07)
  ap.add_argument("--top", type=int, default=1000)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_e2e.txt"))
  a = ap.parse_args()
  from sisua_amd import data
  from sisua_amd.data import SingleCellOMIC
  from tests import preprocess_ref as R
  if a.cells:
    X = big_csr(a.cells, a.genes, a.density)
    forms = [("CSR", X)]
  else:
    x, _ = data.synthetic_8kly()
    forms = [("dense", x), ("CSR", sp.csr_matrix(x))]
    X = forms[1][1]
  N, G = X.shape
  lines = [f"{N} x {G}, {X.nnz} non-zeros ({100.0 * X.nnz / (N * G):.1f} %), top {a.top} genes of 20 bins; one process, OMP_NUM_THREADS = "
           f"{os.environ.get('OMP_NUM_THREADS', 'unset')}; median of {a.reps} after a warm-up [min .. max]"]
  stages = [("filter_cells(min_counts=1)", lambda om: om.filter_cells(min_counts=1)),
            ("filter_genes(min_cells=3)", lambda om: om.filter_genes(min_cells=3)),
            ("normalize(total, log1p)", lambda om: om.normalize(total=True, log1p=True)),
            (f"filter_highly_variable_genes({a.top})", lambda om: om.filter_highly_variable_genes(n_top_genes=a.top))]
  genes = {}
  for form, m in forms:
    def chain():
      om = SingleCellOMIC(m, var_names=np.arange(G))
      for _, f in stages:
        f(om)
      return om
    t = timed(chain, a.reps)
    genes[form] = np.asarray(t[3].get_var_names("transcriptomic"))
    lines.append(f"  device route, {form:5s} container          {t[0] * 1e3:9.2f} ms [{t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f}]   (with the container's copy of the input)")
    om = SingleCellOMIC(m, var_names=np.arange(G))
    for name, f in stages:
      shape = om.numpy().shape
      s = timed(lambda: f(om.copy()), a.reps)
      c = timed(lambda: om.copy(), a.reps)
      lines.append(f"    {name:38s} {max(s[0] - c[0], 0) * 1e3:9.2f} ms on {shape[0]} x {shape[1]}   (the stage's call less a copy of the container, {c[0] * 1e3:.2f} ms)")
      f(om)
  dense = X.toarray()
  h = timed(lambda: R.chain(dense, a.top, 20), 1 if a.cells else a.reps)
  same = all(np.array_equal(g, h[3]["genes"]) for g in genes.values())
  lines.append(f"  host restatement (NumPy, dense float32 in, float64 sums) {h[0] * 1e3:9.2f} ms [{h[1] * 1e3:.2f} .. {h[2] * 1e3:.2f}]   same gene set as the device route: {same}")
  lines.append("")
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "a") as f:
    f.write("\n".join(lines) + "\n")
  print("\n".join(lines))
