"""Multinomial logistic regression (smx_logreg.hip): objective and gradient, the L-BFGS fit, the logits."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _ip, _label_ids, _matrix_ptrs
from sisua_amd.engine._prep import _prep_input

LR_MAX_CLASSES = 256       # smx_logreg_*
LR_MAX_GENES = 32768
LR_MAX_RESIDENT = 1 << 31    # the matrix is held whole: rows (rounded up to 64) x (genes rounded up to 4)


def _lr_input(x, labels, n_classes, block_rows=0, resident=True, every_class=False):
  """The shared arguments of smx_logreg_*, checked here so that a refusal never asks for the device -> (dense, csr, N, G, K, form, labels
  int32 or None).  Two classes take the binary form (one logit row), three and more the multinomial one."""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  K = int(n_classes)
  if not 2 <= K <= LR_MAX_CLASSES:
    raise ValueError(f"logistic regression takes 2 .. {LR_MAX_CLASSES} classes, got {n_classes}")
  if G > LR_MAX_GENES or N >= 2 ** 31:
    raise ValueError(f"logistic regression takes up to {LR_MAX_GENES} columns and fewer than 2^31 rows, got {(N, G)}")
  if resident and (N + 63) // 64 * 64 * ((G + 3) // 4 * 4) > LR_MAX_RESIDENT:
    raise ValueError(f"a matrix of {N} x {G} passes the {LR_MAX_RESIDENT} entries held on the device at once")
  if not np.isfinite(dense if csr is None else csr[2]).all():
    raise ValueError("x holds an entry that is not finite")
  lab = None if labels is None else _label_ids(labels, N, K, f"[{N}] integers")
  if lab is not None and every_class:
    empty = np.flatnonzero(np.bincount(lab, minlength=K) == 0)
    if empty.size:
      raise ValueError(f"class {int(empty[0])} has no row")
  return dense, csr, N, G, K, int(K == 2), lab


def _lr_params(W, b, Kz, G, what="W"):
  w, bb = np.ascontiguousarray(W, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
  if w.shape != (Kz, G) or bb.shape != (Kz,):
    raise ValueError(f"{what} must be [{Kz}, {G}] and its intercept [{Kz}], got {w.shape} and {bb.shape}")
  if not (np.isfinite(w).all() and np.isfinite(bb).all()):
    raise ValueError(f"{what} or its intercept holds a value that is not finite")
  return w, bb


def _lr_penalty(C_):
  c = float(C_)
  if not (np.isfinite(c) and c > 0):
    raise ValueError(f"C must be finite and > 0, got {C_}")
  return c


def k_logreg_eval(x, labels, n_classes: int, W, b, C_: float = 1.0, fit_intercept: bool = True) -> dict:
  """smx_logreg_eval: the mean-form objective F = (1/N) sum_i loss_i + ||W||^2 / (2 C N) and its gradient at (W [Kz, G], b [Kz]) float64,
  Kz = 1 logit row for two classes (the binary form), n_classes otherwise; x dense or scipy.sparse [N, G] (taken as float32), labels [N]
  integers in 0 .. n_classes - 1 (not every class needs a row) -> dict(F, gW [Kz, G], gb [Kz]).  fit_intercept=False: b is taken as 0 and gb is 0."""
  dense, csr, N, G, K, form, lab = _lr_input(x, labels, n_classes)
  Kz = 1 if form else K
  w, bb = _lr_params(W, b, Kz, G)
  c = _lr_penalty(C_)
  lib = _hip.require_gpu()
  F, gW, gb = C.c_double(), np.empty((Kz, G), np.float64), np.empty((Kz,), np.float64)
  check(lib.smx_logreg_eval(*_matrix_ptrs(dense, csr), N, G, _ip(lab), K, form, c, int(bool(fit_intercept)), _dp(w), _dp(bb), C.byref(F),
                            _dp(gW), _dp(gb)))
  return dict(F=F.value, gW=gW, gb=gb)


def k_logreg_fit(x, labels, n_classes: int, C_: float = 1.0, fit_intercept: bool = True, tol: float = 1e-4, max_iter: int = 100,
                 W0=None, b0=None) -> dict:
  """smx_logreg_fit: the minimiser of k_logreg_eval's F by L-BFGS (memory 10, Armijo backtracking) on the device, from zero or from the
  warm start (W0, b0); every class needs a row; stops at max|g| <= tol or after max_iter iterations ->
  dict(W [Kz, G], b [Kz], F, gmax, n_iter, n_eval, converged)"""
  dense, csr, N, G, K, form, lab = _lr_input(x, labels, n_classes, every_class=True)
  Kz = 1 if form else K
  c = _lr_penalty(C_)
  if not float(tol) > 0 or not np.isfinite(float(tol)):
    raise ValueError(f"tol must be finite and > 0, got {tol}")
  if int(max_iter) < 1:
    raise ValueError(f"max_iter must be >= 1, got {max_iter}")
  if (W0 is None) != (b0 is None):
    raise ValueError("the warm start is W0 and b0, or neither")
  w0, bb0 = (None, None) if W0 is None else _lr_params(W0, b0, Kz, G, "W0")
  lib = _hip.require_gpu()
  W, b = np.empty((Kz, G), np.float64), np.empty((Kz,), np.float64)
  F, gmax, n_iter, n_eval, conv = C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
  check(lib.smx_logreg_fit(*_matrix_ptrs(dense, csr), N, G, _ip(lab), K, form, c, int(bool(fit_intercept)), float(tol), int(max_iter),
                           _dp(w0), _dp(bb0), _dp(W), _dp(b), C.byref(F), C.byref(gmax), C.byref(n_iter), C.byref(n_eval), C.byref(conv)))
  return dict(W=W, b=b, F=F.value, gmax=gmax.value, n_iter=n_iter.value, n_eval=n_eval.value, converged=bool(conv.value))


def k_logreg_decision(x, W, b, n_classes: int, block_rows: int = 0):
  """smx_logreg_decision: the logits x.w + b of every row, float64 [N, n_classes], or [N] for two classes (W [1, G]); the matrix is
  streamed in blocks of block_rows rows (0: the library's choice; it changes no bit)"""
  dense, csr, N, G, K, form, _ = _lr_input(x, None, n_classes, block_rows, resident=False)
  Kz = 1 if form else K
  w, bb = _lr_params(W, b, Kz, G)
  lib = _hip.require_gpu()
  z = np.empty((N, Kz), np.float64)
  check(lib.smx_logreg_decision(*_matrix_ptrs(dense, csr), N, G, int(block_rows), K, form, _dp(w), _dp(bb), _dp(z)))
  return z[:, 0] if form else z
