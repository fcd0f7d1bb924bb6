"""The two Gaussian mixtures: one 1-D mixture per column (smx_gmm.hip) and scikit-learn's full-covariance EM (smx_gmm_full.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _f32, _fp, _ip, _ptr


def _gmm_matrix(X, K=None):
  """X [cells, C] as contiguous float32, within the limits of smx_gmm.hip (checked here so that a refusal never asks for the device)"""
  x = np.asarray(X)
  if x.ndim != 2 or x.shape[0] < 1:
    raise ValueError(f"X must be [cells >= 1, C], got {x.shape}")
  if not (1 <= x.shape[1] <= 4096):
    raise ValueError(f"the number of columns must be 1 .. 4096, got {x.shape[1]}")
  if x.shape[0] >= 2 ** 31:
    raise ValueError(f"n_cells must be below 2^31, got {x.shape[0]}")
  if K is not None and not (2 <= int(K) <= 8):
    raise ValueError(f"the number of components must be 2 .. 8, got {K}")
  x = _f32(x)
  if not np.all(np.isfinite(x)) or np.any(x < 0):
    raise ValueError("Only support non-negative values: X holds a negative or non-finite entry")
  return x


def gmm_n_train(x, remove_zeros: bool = True) -> np.ndarray:
  """int64 [C]: the size of every column's training set -- with remove_zeros the positive cells plus ONE sample 0 if any cell was zero"""
  if not remove_zeros:
    return np.full((x.shape[1],), x.shape[0], np.int64)
  n_pos = np.count_nonzero(x > 0, axis=0).astype(np.int64)
  return n_pos + (n_pos < x.shape[0])


def k_gmm1d_fit(X, init_raw, max_iter: int = 120, tol: float = 1e-3, reg_covar: float = 1e-6, remove_zeros: bool = True,
                log_norm: bool = True, all_params: bool = False, stats: bool = False) -> dict:
  """smx_gmm1d_fit: one 1-D mixture of K Gaussians per column of X [cells, C] (non-negative), restart r of column c started from the raw
  values init_raw [C, R, K] of K training cells -> dict(lower_bound, n_iter, converged [C, R]; best, n_train, col_sum [C]; weights, means,
  variances [C, K] of the best restart; params_all [C, R, 3, K] when asked; stats: launches, round_trips, kernel_ms, loop_ms, call_ms)"""
  seeds = np.asarray(init_raw)
  if seeds.ndim != 3:
    raise ValueError(f"init_raw must be [C, R, K], got {seeds.shape}")
  Cn, R, K = seeds.shape
  x = _gmm_matrix(X, K)
  if Cn != x.shape[1]:
    raise ValueError(f"init_raw is for {Cn} columns and X has {x.shape[1]}")
  if not (1 <= R <= 64):
    raise ValueError(f"the number of restarts must be 1 .. 64, got {R}")
  max_iter, tol, reg_covar = int(max_iter), float(tol), float(reg_covar)
  if max_iter < 1 or not (tol > 0 and np.isfinite(tol)) or not (reg_covar >= 0 and np.isfinite(reg_covar)):
    raise ValueError(f"max_iter >= 1, tol > 0 and reg_covar >= 0 are required, got {max_iter}, {tol} and {reg_covar}")
  seeds = _f32(seeds)
  if not np.all(np.isfinite(seeds)) or np.any(seeds < 0):
    raise ValueError("init_raw holds a negative or non-finite value")
  n_train = gmm_n_train(x, remove_zeros)
  if np.any(n_train < K):
    c = int(np.argmax(n_train < K))
    raise ValueError(f"column {c} has {int(n_train[c])} training samples, fewer than the {K} components")
  lib = _hip.require_gpu()
  N, Cn = x.shape
  out = dict(lower_bound=np.empty((Cn, R), np.float64), n_iter=np.empty((Cn, R), np.int32), converged=np.empty((Cn, R), np.int32),
             best=np.empty((Cn,), np.int32), weights=np.empty((Cn, K), np.float64), means=np.empty((Cn, K), np.float64),
             variances=np.empty((Cn, K), np.float64), n_train=np.empty((Cn,), np.int64), col_sum=np.empty((Cn,), np.float64))
  every = np.empty((Cn, R, 3, K), np.float64) if all_params else None
  st = np.zeros((5,), np.float64) if stats else None
  check(lib.smx_gmm1d_fit(_fp(x), N, Cn, K, _fp(seeds), R, max_iter, tol, reg_covar, int(bool(remove_zeros)), int(bool(log_norm)),
                          _dp(out["lower_bound"]), _ip(out["n_iter"]), _ip(out["converged"]), _ip(out["best"]), _dp(out["weights"]),
                          _dp(out["means"]), _dp(out["variances"]), _ptr(out["n_train"]), _dp(out["col_sum"]), _dp(every), _dp(st)))
  if every is not None:
    out["params_all"] = every
  if st is not None:
    out["stats"] = dict(launches=int(st[0]), round_trips=int(st[1]), kernel_ms=float(st[2]), loop_ms=float(st[3]), call_ms=float(st[4]))
  return out


def k_gmm1d_predict(X, weights, means, variances, order, positive_component: int, threshold, log_norm: bool = True, score: bool = False):
  """smx_gmm1d_predict: X [cells, C] under the mixtures weights, means, variances [C, K] -> (prob [cells, C] float64, the mean responsibility
  of the components order[c, positive_component:]; bin [cells, C] float32, normalised value >= threshold[c]; score [cells, C] float64, the
  log-likelihood, or None)"""
  w, m, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (weights, means, variances))
  if w.ndim != 2 or m.shape != w.shape or v.shape != w.shape:
    raise ValueError(f"weights, means and variances must all be [C, K], got {w.shape}, {m.shape} and {v.shape}")
  Cn, K = w.shape
  x = _gmm_matrix(X, K)
  o = np.ascontiguousarray(order, dtype=np.int32)
  thr = np.ascontiguousarray(threshold, dtype=np.float64)
  if x.shape[1] != Cn:
    raise ValueError(f"Number of classes mis-match: fitted with {Cn} columns, X has {x.shape[1]}")
  if o.shape != (Cn, K) or not np.array_equal(np.sort(o, axis=1), np.tile(np.arange(K, dtype=np.int32), (Cn, 1))):
    raise ValueError("order must be [C, K], a permutation of 0 .. K - 1 per column")
  if thr.shape != (Cn,) or np.any(np.isnan(thr)):
    raise ValueError("threshold must be [C] without NaN")
  if not (1 <= int(positive_component) < K):
    raise ValueError(f"positive_component must be 1 .. K - 1 = {K - 1}, got {positive_component}")
  if not (np.all(np.isfinite(w)) and np.all(w > 0) and np.all(np.isfinite(m)) and np.all(np.isfinite(v)) and np.all(v > 0)):
    raise ValueError("weights and variances must be positive and finite, means finite")
  lib = _hip.require_gpu()
  N = x.shape[0]
  prob, bins = np.empty((N, Cn), np.float64), np.empty((N, Cn), np.float32)
  sc = np.empty((N, Cn), np.float64) if score else None
  check(lib.smx_gmm1d_predict(_fp(x), N, Cn, K, _dp(w), _dp(m), _dp(v), _ip(o), int(positive_component), _dp(thr), int(bool(log_norm)),
                              _dp(prob), _fp(bins), _dp(sc)))
  return prob, bins, sc


ILL_DEFINED_COVARIANCE = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance "
                          "caused by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or "
                          "scale the input data.")


def k_gmm_full_fit(Z, init_labels, max_iter: int = 100, tol: float = 1e-3, reg_covar: float = 1e-6, all_params: bool = False,
                   n_components=None) -> dict:
  """smx_gmm_full_fit: scikit-learn's full-covariance EM loop on cells Z [N, D] from the starting labelings init_labels [R, N] (or [N]), K =
  n_components (default: the largest label + 1) -> dict(lower_bound, n_iter, converged, status [R]; best; weights [K], means [K, D],
  covariances, chol_inv [K, D, D] and labels [N] of the best restart; with all_params weights_all [R, K], means_all [R, K, D],
  covariances_all [R, K, D, D]).  A restart with status 1 met an ill-defined covariance; ValueError when every restart did."""
  z = _f32(Z)
  lab = np.asarray(init_labels)
  if lab.ndim == 1:
    lab = lab[None, :]
  if z.ndim != 2 or lab.ndim != 2 or lab.shape[1] != z.shape[0]:
    raise ValueError(f"Z must be [cells, D] and init_labels [R, cells], got {z.shape} and {lab.shape}")
  lab = np.ascontiguousarray(lab, dtype=np.int32)
  K = (int(lab.max()) + 1 if lab.size else 0) if n_components is None else int(n_components)
  (N, D), R = z.shape, lab.shape[0]
  lib = _hip.require_gpu()
  out = dict(lower_bound=np.empty((R,), np.float64), n_iter=np.empty((R,), np.int32), converged=np.empty((R,), np.int32),
             status=np.zeros((R,), np.int32), weights=np.empty((max(K, 0),), np.float64), means=np.empty((max(K, 0), D), np.float64),
             covariances=np.empty((max(K, 0), D, D), np.float64), chol_inv=np.empty((max(K, 0), D, D), np.float64), labels=np.empty((N,), np.int32))
  best = C.c_int32(-1)
  every = np.empty((R, max(K, 0) * (1 + D + D * D)), np.float64) if all_params else None
  rc = lib.smx_gmm_full_fit(_fp(z), N, D, K, _ip(lab), R, int(max_iter), float(tol), float(reg_covar), _dp(out["lower_bound"]), _ip(out["n_iter"]),
                            _ip(out["converged"]), _ip(out["status"]), C.byref(best), _dp(out["weights"]), _dp(out["means"]),
                            _dp(out["covariances"]), _dp(out["chol_inv"]), _ip(out["labels"]), _dp(every))
  if rc == -1 and R >= 1 and bool(np.all(out["status"] == 1)):   # (SMX_ERR_INVALID with every status set: every restart failed)
    raise ValueError(ILL_DEFINED_COVARIANCE)
  check(rc)
  out["best"] = int(best.value)
  if every is not None:
    out["weights_all"] = every[:, :K].copy()
    out["means_all"] = every[:, K:K + K * D].reshape(R, K, D).copy()
    out["covariances_all"] = every[:, K + K * D:].reshape(R, K, D, D).copy()
  return out


def k_gmm_full_predict(Z, weights, means, chol_inv, resp: bool = False, score: bool = False) -> dict:
  """smx_gmm_full_predict: cells Z [N, D] under the mixture weights [K], means [K, D], chol_inv [K, D, D] (lower triangular: the inverse of
  the Cholesky factor of every covariance) -> dict(labels [N] int32; resp [N, K] and score [N] float64 when asked)"""
  w, m, li = (np.ascontiguousarray(a, dtype=np.float64) for a in (weights, means, chol_inv))
  if w.ndim != 1 or m.ndim != 2 or m.shape[0] != w.shape[0] or li.shape != (m.shape[0], m.shape[1], m.shape[1]):
    raise ValueError(f"weights, means and chol_inv must be [K], [K, D] and [K, D, D], got {w.shape}, {m.shape} and {li.shape}")
  K, D = m.shape
  z = _f32(Z)
  if z.ndim != 2 or z.shape[1] != D:
    raise ValueError(f"the mixture has {D} features, Z is {z.shape}")
  lib = _hip.require_gpu()
  N = z.shape[0]
  out = dict(labels=np.empty((N,), np.int32))
  if resp:
    out["resp"] = np.empty((N, K), np.float64)
  if score:
    out["score"] = np.empty((N,), np.float64)
  check(lib.smx_gmm_full_predict(_fp(z), N, D, K, _dp(w), _dp(m), _dp(li), _ip(out["labels"]), _dp(out["resp"]) if resp else None,
                                 _dp(out["score"]) if score else None))
  return out
