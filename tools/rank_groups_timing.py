"""Wall times of ranking genes between groups at the 8kly shape (4697 cells x 1998 genes, 12 groups), dense and CSR: every method of
`sisua_amd.rank_genes_groups` end to end (host preparation, copies, the device, the closing formulas), the two device entries by
themselves, and the vectorised SciPy route of the Wilcoxon rank sums (tests/rank_groups_ref.py: one rankdata over the columns, one
product) on the same host (profiles/rank_groups_e2e.txt).
usage: python tools/rank_groups_timing.py [reps=5]"""
import os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sisua_amd import engine, rank_genes_groups
from sisua_amd.data import synthetic_8kly
from sisua_amd.rank_groups import METHODS
from tests import rank_groups_ref as R

K = 12

def timed(f, reps):
  ts = []
  for _ in range(reps):
    t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)   # (every entry ends in a copy back: the device is idle)
  return ts, r

def show(ts):
  return f"min {min(ts) * 1e3:.1f} ms, median {np.median(ts) * 1e3:.1f} ms, max {max(ts) * 1e3:.1f} ms of {len(ts)}"

if __name__ == "__main__":
  reps = int(dict(a.split("=") for a in sys.argv[1:] if "=" in a).get("reps", 5))
  x, y = synthetic_8kly()
  X = np.log1p(x / x.sum(1, keepdims=True) * 1e4).astype(np.float32)   # normalised expression, as the rankings are run on
  lab = np.argmax(y, axis=1)                                           # 12 groups: the protein with the highest level
  N, G = X.shape
  print(f"{N} x {G}, {K} groups of {np.bincount(lab, minlength=K).min()} .. {np.bincount(lab, minlength=K).max()} cells, sparsity "
        f"{(X == 0).mean():.3f}; host threads {os.environ.get('OMP_NUM_THREADS', '?')} (of {os.cpu_count()} CPUs)", flush=True)
  rank_genes_groups(X[:512, :8], lab[:512] % 2, method="wilcoxon")   # (a first call: code objects)
  for name, M in (("dense", X), ("CSR", sp.csr_matrix(X))):
    for method in METHODS:
      ts, _ = timed(lambda: rank_genes_groups(M, lab, method=method), reps)
      print(f"{name}: rank_genes_groups(method={method!r}) end to end: {show(ts)}", flush=True)
    ts, _ = timed(lambda: rank_genes_groups(M, lab, method="wilcoxon", reference=0, tie_correct=True), reps)
    print(f"{name}: rank_genes_groups(method='wilcoxon', reference=0, tie_correct=True) end to end: {show(ts)}", flush=True)
    ts, _ = timed(lambda: engine.k_group_moments(M, lab, K), reps)
    print(f"{name}: smx_group_moments by itself: {show(ts)}", flush=True)
  cols = np.ascontiguousarray(X.T)
  ts, dev = timed(lambda: engine.k_group_ranksums(cols, lab, K), reps)
  print(f"smx_group_ranksums on prepared columns, against the rest: {show(ts)} ({G / min(ts):.0f} genes / s)", flush=True)
  ts, _ = timed(lambda: engine.k_group_ranksums(cols, lab, K, reference=0), reps)
  print(f"smx_group_ranksums on prepared columns, against group 0: {show(ts)}", flush=True)
  ts, ref = timed(lambda: R.ranksums_vectorised(X, lab, K), max(2, reps // 2))
  print(f"SciPy on the host (rankdata(axis=0) and a [12, N] x [N, G] product): {show(ts)}; doubled rank sums equal the device's: "
        f"{np.array_equal(np.rint(2 * ref).astype(np.int64), dev[0])}", flush=True)
