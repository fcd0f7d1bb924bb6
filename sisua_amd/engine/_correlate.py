"""Gene x protein correlation sums (smx_correlate.hip): the kernels of Engine.predict_correlate on host columns."""
import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _f32, _fp, _ip, _ptr


def _col_operands(prot_rank2, prot_unit, N):
  pr, pu = np.ascontiguousarray(prot_rank2, dtype=np.int32), np.ascontiguousarray(prot_unit, dtype=np.float64)
  if pr.ndim != 2 or pr.shape[0] < 1 or pr.shape[1] != N or pu.shape != pr.shape:
    raise ValueError(f"prot_rank2 and prot_unit must both be [P >= 1, {N}], got {pr.shape} and {pu.shape}")
  return pr, pu


def _col_outputs(n, P):
  """The result arrays of the correlation sums for n genes and P proteins, and their pointers in the order of smx_predict_correlate's outputs"""
  out = dict(sp_Sa=np.empty((n,), np.int64), sp_Saa=np.empty((n,), np.int64), sp_Sab=np.empty((n, P), np.int64),
             pe_mean=np.empty((n,), np.float64), pe_Sxx=np.empty((n,), np.float64), pe_Sxy=np.empty((n, P), np.float64),
             nonfinite=np.empty((n,), np.int32))
  return out, tuple(_ptr(a) for a in out.values())   # (the dict is in the order of the C arguments)


def k_col_rank2(cols):
  """smx_k_col_rank2: cols [n_cols, N] (gene-major) -> (rank2 [n_cols, N] int32 = 2 x the average ranks of every column, nonfinite [n_cols] int32)"""
  lib = _hip.require_gpu()
  c = _f32(cols)
  n, N = c.shape
  rank2, nonfinite = np.empty((n, N), np.int32), np.empty((n,), np.int32)
  check(lib.smx_k_col_rank2(_fp(c), n, N, _ip(rank2), _ip(nonfinite)))
  return rank2, nonfinite


def k_col_correlate(cols, prot_rank2, prot_unit):
  """smx_k_col_correlate: the kernels of Engine.predict_correlate on host columns cols [n_cols, N] -> its dict of sums"""
  lib = _hip.require_gpu()
  c = _f32(cols)
  n, N = c.shape
  pr, pu = _col_operands(prot_rank2, prot_unit, N)
  out, res = _col_outputs(n, pr.shape[0])
  check(lib.smx_k_col_correlate(_fp(c), n, N, _ip(pr), _dp(pu), pr.shape[0], *res))
  return out
