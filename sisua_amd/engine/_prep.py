"""Count-matrix preprocessing (smx_prep.hip): statistics of a view f(x / row_div) and the view written out.  `_prep_input` is the
"dense or scipy.sparse matrix" check of every model-free entry that takes one."""
from __future__ import annotations

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _csr3, _dp, _f32, _fp, _ip, _matrix_ptrs, _ptr, _sparse

PREP_FUNCS = {None: 0, "identity": 0, "log1p": 1, "expm1": 2}   # smx_prep_*: the f of a view f(x / row_div)


def _prep_input(x, func, row_div, block_rows):
  """The shared arguments of smx_prep_stats / smx_prep_apply, checked here so that a refusal never asks for the device:
  -> (dense float32 [N, G] or None, (indptr, cols, vals) or None, N, G, func id, row_div float32 [N] or None)"""
  if func not in PREP_FUNCS:
    raise ValueError(f"func must be one of 'identity', 'log1p', 'expm1', got {func!r}")
  if getattr(x, "ndim", 0) != 2 or x.shape[0] < 1 or x.shape[1] < 1:
    raise ValueError(f"expected a matrix [cells >= 1, genes >= 1], got shape {getattr(x, 'shape', None)}")
  if int(block_rows) < 0:
    raise ValueError(f"block_rows must be >= 0 (0: the library's choice), got {block_rows}")
  N, G = x.shape
  dense, csr = (None, _csr3(x, G)) if _sparse(x) else (_f32(x), None)
  rd = None if row_div is None else _f32(row_div, (N,))
  if rd is not None and not (np.isfinite(rd).all() and (rd != 0).all()):
    raise ValueError("row_div must be finite and non-zero")
  return dense, csr, N, G, PREP_FUNCS[func], rd


def k_prep_stats(x, func=None, row_div=None, col_mask=None, row_thresh=None, block_rows: int = 0) -> dict:
  """smx_prep_stats: the statistics of the view f(x / row_div) of a dense or scipy.sparse matrix [N, G] -> dict(total [N] float64 (over the
  genes col_mask keeps), n_genes [N] int32, sum / sumsq [G] float64, n_cells [G] int64, and with row_thresh [N]: n_above [G] int64)"""
  dense, csr, N, G, f, rd = _prep_input(x, func, row_div, block_rows)
  mask = None if col_mask is None else np.ascontiguousarray(col_mask, dtype=np.uint8)
  if mask is not None and mask.shape != (G,):
    raise ValueError(f"col_mask must be [{G}], got {mask.shape}")
  thr = None if row_thresh is None else _f32(row_thresh, (N,))
  if thr is not None and np.isnan(thr).any():
    raise ValueError("row_thresh holds a NaN")
  lib = _hip.require_gpu()
  out = dict(total=np.empty((N,), np.float64), n_genes=np.empty((N,), np.int32), sum=np.empty((G,), np.float64),
             sumsq=np.empty((G,), np.float64), n_cells=np.empty((G,), np.int64))
  if thr is not None:
    out["n_above"] = np.empty((G,), np.int64)
  check(lib.smx_prep_stats(*_matrix_ptrs(dense, csr), N, G, int(block_rows), f, _fp(rd), _ptr(mask), _fp(thr), _dp(out["total"]),
                           _ip(out["n_genes"]), _dp(out["sum"]), _dp(out["sumsq"]), _ptr(out["n_cells"]), _ptr(out.get("n_above"))))
  return out


def k_prep_apply(x, func=None, row_div=None, mean=None, std=None, max_value=None, block_rows: int = 0):
  """smx_prep_apply: the view f(x / row_div) written out as float32, then (v - mean) / std and the clip from above at max_value where
  given.  A scipy.sparse matrix without mean / std / max_value comes back as CSR of the same structure (only the stored values cross);
  everything else comes back dense [N, G]."""
  dense, csr, N, G, f, rd = _prep_input(x, func, row_div, block_rows)
  if (mean is None) != (std is None):
    raise ValueError("mean and std go together")
  mu, sd = (None, None) if mean is None else (_f32(mean, (G,)), _f32(std, (G,)))
  if max_value is not None and np.isnan(max_value):
    raise ValueError("max_value is NaN")
  clip, mv = (0, 0.0) if max_value is None else (1, float(max_value))
  lib = _hip.require_gpu()
  if csr is not None and mu is None and not clip:
    import scipy.sparse as sp
    vals = np.empty_like(csr[2])
    check(lib.smx_prep_apply(*_matrix_ptrs(dense, csr), N, G, int(block_rows), f, _fp(rd), None, None, 0, 0.0, None, _fp(vals)))
    return sp.csr_matrix((vals, csr[1].copy(), csr[0].copy()), shape=(N, G))
  out = np.empty((N, G), np.float32)
  check(lib.smx_prep_apply(*_matrix_ptrs(dense, csr), N, G, int(block_rows), f, _fp(rd), _fp(mu), _fp(sd), clip, mv, _fp(out), None))
  return out
