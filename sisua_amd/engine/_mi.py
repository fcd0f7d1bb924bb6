"""Gene x protein mutual information by scikit-learn's kNN estimators (smx_mi.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _ip, _ptr

MI_MAX_NEIGHBORS = 8       # smx_mutual_info: the register list of the cc sweep
MI_MAX_CELLS = 1 << 20


def _mi_tables(N):
  """(digamma(n), log(n)) for n = 0 .. N, float64: the two tables the device adds entries of (entry 0 is never read)"""
  from scipy.special import digamma
  n = np.arange(N + 1, dtype=np.float64)
  psi, logn = np.zeros(N + 1), np.zeros(N + 1)
  psi[1:], logn[1:] = digamma(n[1:]), np.log(n[1:])
  return psi, logn


def _mi_check(N, n_neighbors):
  k = int(n_neighbors)
  if not 2 <= N <= MI_MAX_CELLS:
    raise ValueError(f"mutual information takes 2 .. 2^20 cells, got {N}")
  if k < 1 or k > MI_MAX_NEIGHBORS:
    raise ValueError(f"n_neighbors must be in 1 .. {MI_MAX_NEIGHBORS} (MI_MAX_NEIGHBORS: the register list of the device's sweep), got {k}")
  if k >= N:
    raise ValueError(f"n_neighbors = {k} must be below the number of cells ({N})")
  return k


def _mi_cols(cols, discrete, what):
  c = np.ascontiguousarray(cols, dtype=np.float64)
  d = np.ascontiguousarray(discrete, dtype=bool).astype(np.uint8)
  if c.ndim != 2 or c.shape[0] < 1 or d.shape != (c.shape[0],):
    raise ValueError(f"{what} columns must be [columns >= 1, cells] with one discrete flag each, got {c.shape} and {d.shape}")
  bad = np.flatnonzero(~np.isfinite(c).all(axis=1))
  if bad.size:
    raise ValueError(f"{what} column {int(bad[0])} holds a value that is not finite")
  return c, d


def mutual_info(xcols, x_discrete, ycols, y_discrete, n_neighbors: int = 3, gene_chunk: int = 0):
  """smx_mutual_info: prepared columns xcols [G, N] and ycols [P, N] float64 (gene-major) with their discrete flags -> the mutual
  information [G, P] float64 of every pair, by scikit-learn's three kNN estimators.  gene_chunk: genes on the device at a time (0: the
  library's choice); it changes no bit."""
  x, xd = _mi_cols(xcols, x_discrete, "gene")
  y, yd = _mi_cols(ycols, y_discrete, "protein")
  if x.shape[1] != y.shape[1]:
    raise ValueError(f"genes and proteins must share their cells, got {x.shape[1]} and {y.shape[1]}")
  N = x.shape[1]
  k = _mi_check(N, n_neighbors)
  if int(gene_chunk) < 0:
    raise ValueError(f"gene_chunk must be >= 0, got {gene_chunk}")
  lib = _hip.require_gpu()
  psi, logn = _mi_tables(N)
  mi = np.empty((x.shape[0], y.shape[0]), np.float64)
  check(lib.smx_mutual_info(_dp(x), _ptr(xd), _dp(y), _ptr(yd), N, x.shape[0], y.shape[0], k, int(gene_chunk), _dp(psi), _dp(logn), _dp(mi)))
  return mi


def k_mi_cells(x, x_discrete: bool, y, y_discrete: bool, n_neighbors: int = 3) -> dict:
  """smx_k_mi_cells: ONE pair of prepared columns x, y [N] -> the per-cell quantities of its estimator and its value `mi`:
  cc: r [N] float64, nx, ny [N] int32;  cd (either discrete): kept, k, count, m [N] int32 (k and m 0 where not kept), r;
  dd: a, b (the labels' values), n_ab [R]: the non-empty cells of the contingency table sorted by (a, b)"""
  xv, yv = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
  if xv.ndim != 1 or xv.shape != yv.shape:
    raise ValueError(f"x and y must both be [cells], got {xv.shape} and {yv.shape}")
  if not (np.isfinite(xv).all() and np.isfinite(yv).all()):
    raise ValueError("x or y holds a value that is not finite")
  N = xv.shape[0]
  k = _mi_check(N, n_neighbors)
  lib = _hip.require_gpu()
  psi, logn = _mi_tables(N)
  cells, radius, mi = np.empty((4, N), np.int32), np.empty((N,), np.float64), C.c_double()
  check(lib.smx_k_mi_cells(_dp(xv), int(bool(x_discrete)), _dp(yv), int(bool(y_discrete)), N, k, _dp(psi), _dp(logn), _ip(cells), _dp(radius),
                           C.byref(mi)))
  if x_discrete and y_discrete:
    heads = np.flatnonzero(cells[2] > 0)
    at = cells[3][heads]
    return dict(a=xv[at], b=yv[at], n_ab=cells[2][heads].copy(), mi=mi.value)
  if not x_discrete and not y_discrete:
    return dict(r=radius, nx=cells[0] - 1, ny=cells[1] - 1, mi=mi.value)
  return dict(kept=(cells[1] > 0).astype(np.int32), k=cells[0].copy(), count=cells[3].copy(), m=cells[2].copy(), r=radius, mi=mi.value)
