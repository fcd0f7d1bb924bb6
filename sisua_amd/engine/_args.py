"""The argument plumbing of every wrapper: numpy arrays to C pointers, and the argument checks that more than one kernel family shares."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

_CTYPES = {np.dtype(np.float32): C.c_float, np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32,
           np.dtype(np.int64): C.c_int64, np.dtype(np.uint8): C.c_uint8, np.dtype(np.uint16): C.c_uint16}


def _ptr(a, dtype=None):
  """The pointer to an array's data, typed by its dtype (float32, float64, int32, int64, uint8, uint16; anything else is a TypeError);
  None stays None (NULL).  dtype: the one the C argument takes -- an array of another is a TypeError instead of a reinterpretation."""
  if a is None:
    return None
  if dtype is not None and a.dtype != dtype:
    raise TypeError(f"expected a {np.dtype(dtype).name} array, got {a.dtype}")
  if a.dtype not in _CTYPES:
    raise TypeError(f"no pointer type for dtype {a.dtype}")
  return a.ctypes.data_as(C.POINTER(_CTYPES[a.dtype]))


def _fp(a: Optional[np.ndarray]):
  return _ptr(a, np.float32)


def _ip(a):
  return _ptr(a, np.int32)


def _dp(a):
  return _ptr(a, np.float64)


def _f32(a, shape=None):
  a = np.ascontiguousarray(a, dtype=np.float32)
  if shape is not None and tuple(a.shape) != tuple(shape):
    raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
  return a


def _csr3(x, n_genes: int, n_rows: Optional[int] = None):
  """scipy.sparse rows -> (indptr int64, cols int32, vals float32) of their canonical float32 CSR (data.as_csr), shape-checked."""
  from sisua_amd.data import as_csr
  if x.ndim != 2 or x.shape[1] != n_genes or (n_rows is not None and x.shape[0] != n_rows):
    raise ValueError(f"expected sparse rows [{'n_cells' if n_rows is None else n_rows}, {n_genes}], got {x.shape}")
  c = as_csr(x, copy=False)
  return (np.ascontiguousarray(c.indptr, dtype=np.int64), np.ascontiguousarray(c.indices, dtype=np.int32),
          np.ascontiguousarray(c.data, dtype=np.float32))


def _csr_ptrs(t):
  return (_ptr(t[0], np.int64), _ip(t[1]), _fp(t[2]))


def _matrix_ptrs(dense, csr):
  """The four pointers (x, indptr, cols, vals) of a host matrix in the rows convention of include/sisua_hip.h, for a (dense, csr) pair: one
  of the two is None (both: a matrix the entry lets the caller leave out)."""
  return (_fp(dense), *((None, None, None) if csr is None else _csr_ptrs(csr)))


def _fps(arrays):
  """A C array of float pointers to `arrays` (label heads), None without any; the caller keeps `arrays` alive through the call."""
  return (C.POINTER(C.c_float) * max(1, len(arrays)))(*[_fp(a) for a in arrays]) if arrays else None


def _sparse(x) -> bool:
  from sisua_amd.data import is_sparse
  return is_sparse(x)


def _label_ids(labels, N, K, expected):
  """labels [N] of integers in 0 .. K - 1 -> int32; `expected`: the entry's own wording of what it takes, for its refusal"""
  lab = np.asarray(labels)
  if lab.shape != (N,) or lab.dtype.kind not in "iu":
    raise ValueError(f"labels must be {expected}, got {lab.dtype} {lab.shape}")
  if lab.min() < 0 or lab.max() >= K:
    raise ValueError(f"labels must lie in 0 .. {K - 1}")
  return np.ascontiguousarray(lab, dtype=np.int32)
