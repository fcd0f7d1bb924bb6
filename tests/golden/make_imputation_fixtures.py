#!/usr/bin/env python3
"""Generate tests/golden/imputation_fixture.npz by EXECUTING the reference's own functions imputation_score, imputation_mean_score and
imputation_std_score (sisua/analysis/imputation_benchmarks.py:102-127).  Their module imports plotting packages at module level, so each
function's source is lifted out of the file with `ast` and run against NumPy only; nothing of the reference is copied into the
repository -- the fixture holds inputs and outputs.

usage: python tests/golden/make_imputation_fixtures.py <path to the reference checkout>"""
import ast
import os
import sys
import warnings

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "imputation_fixture.npz")
PATH = "sisua/analysis/imputation_benchmarks.py"


def lift(ref, name, namespace):
  tree = ast.parse(open(os.path.join(ref, PATH)).read())
  for node in ast.walk(tree):
    if isinstance(node, ast.FunctionDef) and node.name == name:
      exec(compile(ast.Module(body=[node], type_ignores=[]), PATH, "exec"), namespace)
      return namespace[name]
  raise KeyError(name)


def cases():
  rng = np.random.default_rng(20261016)
  out = {}
  for name, (n, g) in (("odd", (9, 33)), ("even", (10, 32)), ("even_rows_odd_total", (7, 31)), ("wide", (4, 200))):
    org = (rng.poisson(2.0, size=(n, g)) * (rng.uniform(size=(n, g)) < 0.5)).astype(np.float32)
    crt = org.copy()
    rows = rng.choice(n, size=n // 2, replace=False)   # some rows changed, the others untouched
    for r in rows:
      nz = np.nonzero(crt[r])[0]
      crt[r, nz[: max(1, nz.size // 3)]] = 0.0
    imp = (org * rng.uniform(0.5, 1.5, size=(n, g)) + rng.gamma(1.0, 0.3, size=(n, g))).astype(np.float32)
    out[name] = (org, crt, imp)
  org, crt, imp = (a.copy() for a in out["even"])
  out["unchanged"] = (org, org.copy(), imp)                      # no cell changed: the mean / std scores are 0
  imp_t = np.round(imp * 2.0) / 2.0                              # many ties among the differences
  out["ties"] = (org, crt, imp_t.astype(np.float32))
  imp_n = imp.copy()
  imp_n[3, 5] = np.nan                                           # a NaN: its cell's median and the global median are NaN
  out["nan"] = (org, crt, imp_n)
  one = np.array([[3.0], [0.0], [2.0]], np.float32)              # a single gene
  out["one_gene"] = (one, np.array([[0.0], [0.0], [2.0]], np.float32), np.array([[1.5], [0.25], [2.0]], np.float32))
  return out


def main():
  ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SISUA_REFERENCE", "")
  if not os.path.exists(os.path.join(ref, PATH)):
    sys.exit(__doc__)
  ns = dict(np=np)
  fns = {k: lift(ref, k, ns) for k in ("imputation_score", "imputation_mean_score", "imputation_std_score")}
  rec = {}
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for name, (org, crt, imp) in cases().items():
      rec[f"{name}/original"], rec[f"{name}/corrupted"], rec[f"{name}/imputed"] = org, crt, imp
      # each result as the reference returns it: its dtype is part of the record (np.asarray of a float / np.float32 / int 0)
      rec[f"{name}/med"] = np.asarray(fns["imputation_score"](org, imp))
      rec[f"{name}/mean"] = np.asarray(fns["imputation_mean_score"](org, crt, imp))
      rec[f"{name}/std"] = np.asarray(fns["imputation_std_score"](org, crt, imp))
  np.savez_compressed(OUT, **rec)
  print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(cases()), "cases")


if __name__ == "__main__":
  main()
