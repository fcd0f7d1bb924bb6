"""Measured accuracy of every matrix-product form reachable through smx_k_gemm and of the fused output head's two products,
beside the figures the tests size their bounds from (tests/product_ref.py, tests/test_gpu_product_accuracy.py).  Needs an MI355X.

  python tools/product_accuracy.py [--out profiles/product_accuracy.txt]

Per form and shape: the relative Frobenius error against float64 on N(0, 1) operands and on operands whose rows / columns are
scaled by powers of two, e_seq32 (a float32 product accumulated sequentially), e_drop (the smallest error of the six-term
arithmetic with one term left out), the bound min(2 e_seq32, e_drop / 3), and the worst error of the known-answer term probe in
float32 ulp.  Then power-of-two scaling (elements that are not bit-identical), subnormal and wide-range operands, containment
of a NaN / infinity, and the head."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  from sisua_amd import engine
  from tests import product_ref as pr
  lines = []

  def emit(s=""):
    print(s, flush=True)
    lines.append(s)

  name = lambda f: "%-5s tile %3d A%s B%s split %d  %4d x %4d x %5d" % (f[0], f[1], "[K][M]" if f[2] else "[M][K]", "[N][K]" if f[3] else "[K][N]", f[4], *f[5])
  cache = {}
  emit("relative Frobenius error against float64; bound = min(2 e_seq32, e_drop / 3); probe: worst |C - ref64| in float32 ulp (allowed: 4)")
  emit("%-62s %9s %9s %9s %9s %9s %6s" % ("form", "N(0,1)", "scaled", "e_seq32", "e_drop", "bound", "probe"))
  for f in pr.forms():
    e, es, ed = pr.random_figures(engine.k_gemm, f, False, cache)
    e2, es2, ed2 = pr.random_figures(engine.k_gemm, f, True, cache)
    emit("%-62s %9.2e %9.2e %9.2e %9.2e %9.2e %6.2f" % (name(f), e, e2, es, ed, pr.bound(es, ed), pr.probe_worst_ulp(engine.k_gemm, f)))
    if e2 > pr.bound(es2, ed2):
      emit("    scaled operands: error %.2e over their bound %.2e" % (e2, pr.bound(es2, ed2)))
  emit()
  emit("power-of-two scaling C(2^p A, 2^q B) against 2^(p+q) C(A, B): elements whose bits differ, per (p, q) of %s" % (pr.SCALINGS,))
  emit("subnormals mixed in: ||C - ref||_F / allowed;  |A| <= 2^126 against |B| >= 2^-103, then >= 2^-126: error / bound;  containment: failures of 8")
  seen = set()
  for f in pr.forms():
    if (f[1], f[2], f[3], f[4]) in seen:   # the smallest (ragged) shape of each form
      continue
    seen.add((f[1], f[2], f[3], f[4]))
    mism = [pr.scaling_mismatches(engine.k_gemm, f, p, q) for p, q in pr.SCALINGS]
    fin, err, allowed = pr.subnormal_figures(engine.k_gemm, f, cache)
    ew, es, ed = pr.wide_range_figures(engine.k_gemm, f, pr.SPLIT_MIN_EXPONENT, cache)
    ew2, es2, ed2 = pr.wide_range_figures(engine.k_gemm, f, -126, cache)
    cont = pr.containment(engine.k_gemm, f)
    bad = [c[0] for c in cont if not (c[1] and c[2])]
    emit("%-62s scaling %s  subnormal %s %.2e / %.2e  wide(2^-103) %.2e / %.2e  wide(2^-126) %.2e / %.2e  containment %d %s" %
         (name(f), mism, "finite" if fin else "NOT FINITE", err, allowed, ew, pr.bound(es, ed), ew2, pr.bound(es2, ed2), len(bad), bad[:2] if bad else ""))
  emit()
  emit("fused output head, G = %d: dW of the 128-cell launch against d[b*] (x) db2, dd of the one-cell launch against db2 W^T" % pr.HEAD_G)
  emit("%-22s %9s %9s %9s %9s   %9s %9s %9s %9s" % ("", "dW err", "e_seq32", "e_drop", "bound", "dd err", "e_seq32", "e_drop", "bound"))
  for lk, k in (("zinb", 3), ("nbd", 2)):
    for b in pr.HEAD_ROWS:
      h = pr.head_figures(engine.k_head_fused, lk, k, b)
      w, d = h["dW"], h["dd"]
      emit("%-5s b* = %3d %s %9.2e %9.2e %9.2e %9.2e   %9.2e %9.2e %9.2e %9.2e" %
           (lk, b, "      " if h["finite"] else "NONFIN", w[0], w[1], w[2], pr.bound(w[1], w[2]), d[0], d[1], d[2], pr.bound(d[1], d[2])))
  if args.out:
    with open(args.out, "w") as fh:
      fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
