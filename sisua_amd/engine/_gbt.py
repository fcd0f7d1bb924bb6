"""Gradient-boosted classification trees (smx_gbt.hip): the bins, one stage's trees from integer statistics, the stage loop, the raw scores."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _fp, _ip, _label_ids, _matrix_ptrs, _ptr
from sisua_amd.engine._prep import _prep_input

GBT_MAX_CELLS = 1 << 20      # smx_gbt_*
GBT_MAX_GENES = 32768
GBT_MAX_CLASSES = 32
GBT_MAX_DEPTH = 6
GBT_MAX_BINS = 256
GBT_MAX_PASS = 16            # (class, node) pairs of one pass of the sweep
GBT_MAX_RESIDENT = 1 << 31   # the float32 matrix is held whole while it is binned: rows (rounded up to 64) x (genes rounded up to 4)
GBT_MAX_Q = 1 << 41          # |q_r| and q_h of k_gbt_grow

_TREE_ARRAYS = (("feature", np.int32), ("threshold", np.float32), ("left", np.int32), ("right", np.int32), ("value", np.float64),
                ("n", np.int32), ("improvement", np.float64))


def _gbt_input(x, block_rows=0, resident=True):
  """The matrix of smx_gbt_*, checked here so that a refusal never asks for the device -> (dense, csr, N, G)"""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  if N > GBT_MAX_CELLS:
    raise ValueError(f"gradient boosting takes N <= 2^20 rows (the statistics are exact integers), got {N}")
  if G > GBT_MAX_GENES:
    raise ValueError(f"gradient boosting takes G <= {GBT_MAX_GENES} columns, got {G}")
  if resident and (N + 63) // 64 * 64 * ((G + 3) // 4 * 4) > GBT_MAX_RESIDENT:
    raise ValueError(f"a matrix of {N} x {G} passes the {GBT_MAX_RESIDENT} entries held on the device at once")
  if not np.isfinite(dense if csr is None else csr[2]).all():
    raise ValueError("x holds an entry that is not finite")
  return dense, csr, N, G


def _gbt_tree_params(max_depth, min_samples_split, min_samples_leaf, pass_pairs):
  d, mss, msl, pp = int(max_depth), int(min_samples_split), int(min_samples_leaf), int(pass_pairs)
  if not 1 <= d <= GBT_MAX_DEPTH:
    raise ValueError(f"max_depth must be 1 .. {GBT_MAX_DEPTH}, got {max_depth}")
  if mss < 2 or msl < 1:
    raise ValueError(f"min_samples_split must be >= 2 and min_samples_leaf >= 1, got {min_samples_split} and {min_samples_leaf}")
  if not 0 <= pp <= GBT_MAX_PASS:
    raise ValueError(f"pass_pairs must be 0 (the library's choice) or 1 .. {GBT_MAX_PASS}, got {pass_pairs}")
  return d, mss, msl, pp


def _gbt_tree_outputs(shape):
  return {name: np.empty(shape, dtype) for name, dtype in _TREE_ARRAYS}


def _gbt_tree_ptrs(t):
  return (_ip(t["feature"]), _fp(t["threshold"]), _ip(t["left"]), _ip(t["right"]), _dp(t["value"]), _ip(t["n"]), _dp(t["improvement"]))


def k_gbt_bin(x) -> dict:
  """smx_gbt_bin: every column of x (dense or scipy.sparse [N, G], taken as float32) sorted and binned -> dict(thr float32 [G, 255] (zero
  behind n_thr), n_thr int32 [G], bins uint8 [G, N]): a bin per distinct value up to 256 of them, cuts at the 256-quantile positions beyond"""
  dense, csr, N, G = _gbt_input(x)
  lib = _hip.require_gpu()
  out = dict(thr=np.empty((G, GBT_MAX_BINS - 1), np.float32), n_thr=np.empty((G,), np.int32), bins=np.empty((G, N), np.uint8))
  check(lib.smx_gbt_bin(*_matrix_ptrs(dense, csr), N, G, _fp(out["thr"]), _ip(out["n_thr"]), _ptr(out["bins"])))
  return out


def k_gbt_grow(B, q_r, q_h, max_depth: int = 3, min_samples_split: int = 2, min_samples_leaf: int = 1, scale: float = 1.0,
               pass_pairs: int = 0) -> dict:
  """smx_gbt_grow: the K trees of one stage from integer statistics q_r, q_h int64 [K, N] over the bins B (k_gbt_bin's dict) -> dict(feature,
  threshold, left, right, value, n, improvement [K, M = 2^(max_depth + 1) - 1] in heap order, leaf int32 [K, N]).  pass_pairs (tests): the
  (class, node) pairs one workgroup of the sweep holds in LDS; it changes no bit."""
  bins = np.ascontiguousarray(B["bins"], dtype=np.uint8)
  n_thr, thr = np.ascontiguousarray(B["n_thr"], dtype=np.int32), np.ascontiguousarray(B["thr"], dtype=np.float32)
  if bins.ndim != 2 or bins.shape[0] < 1 or bins.shape[1] < 1:
    raise ValueError(f"bins must be [G >= 1, N >= 1], got {bins.shape}")
  G, N = bins.shape
  if N > GBT_MAX_CELLS or G > GBT_MAX_GENES:
    raise ValueError(f"gradient boosting takes N <= 2^20 rows and G <= {GBT_MAX_GENES} columns, got {(N, G)}")
  if n_thr.shape != (G,) or thr.shape != (G, GBT_MAX_BINS - 1):
    raise ValueError(f"n_thr must be [{G}] and thr [{G}, {GBT_MAX_BINS - 1}], got {n_thr.shape} and {thr.shape}")
  if n_thr.min() < 0 or n_thr.max() > GBT_MAX_BINS - 1 or (bins > n_thr[:, None]).any():
    raise ValueError("a threshold count outside 0 .. 255, or a bin beyond its column's thresholds")
  qr, qh = np.ascontiguousarray(q_r, dtype=np.int64), np.ascontiguousarray(q_h, dtype=np.int64)
  if qr.ndim != 2 or qr.shape[1] != N or qh.shape != qr.shape or not 1 <= qr.shape[0] <= GBT_MAX_CLASSES:
    raise ValueError(f"q_r and q_h must be [1 .. {GBT_MAX_CLASSES}, {N}], got {qr.shape} and {qh.shape}")
  if np.abs(qr).max() > GBT_MAX_Q or qh.min() < 0 or qh.max() > GBT_MAX_Q:
    raise ValueError("the statistics must satisfy |q_r| <= 2^41 and 0 <= q_h <= 2^41")
  d, mss, msl, pp = _gbt_tree_params(max_depth, min_samples_split, min_samples_leaf, pass_pairs)
  if not np.isfinite(float(scale)):
    raise ValueError(f"scale must be finite, got {scale}")
  K, M = qr.shape[0], 2 ** (d + 1) - 1
  lib = _hip.require_gpu()
  out = _gbt_tree_outputs((K, M))
  out["leaf"] = np.empty((K, N), np.int32)
  check(lib.smx_gbt_grow(_ptr(bins), _ip(n_thr), _fp(thr), _ptr(qr), _ptr(qh), N, G, K, d, mss, msl, float(scale), pp, *_gbt_tree_ptrs(out),
                         _ip(out["leaf"])))
  return out


def gbt_init_raw(labels, n_classes: int):
  """the prior's raw scores float64 [Kz]: scikit-learn's DummyClassifier(strategy='prior') through the loss's link -- logit(p_1) for two
  classes, log p_k - mean log p for more; p clipped to [eps, 1 - eps] of float32"""
  eps = np.finfo(np.float32).eps
  p = np.clip(np.bincount(labels, minlength=n_classes) / np.float64(len(labels)), eps, 1 - eps)
  if n_classes == 2:
    return np.array([np.log(p[1] / (1 - p[1]))])
  return np.log(p / np.exp(np.mean(np.log(p))))


def k_gbt_fit(x, labels, n_classes: int, n_estimators: int = 100, learning_rate: float = 0.1, max_depth: int = 3, min_samples_split: int = 2,
              min_samples_leaf: int = 1, x_val=None, labels_val=None, n_iter_no_change=None, tol: float = 1e-4, pass_pairs: int = 0) -> dict:
  """smx_gbt_fit: the stage loop on the device.  x dense or scipy.sparse [N, G], labels [N] integers in 0 .. n_classes - 1, every class
  with a row.  n_iter_no_change: scikit-learn's early stopping on (x_val, labels_val), which take no part in the bins or the trees ->
  dict(the tree arrays [n_estimators_, Kz, M], n_estimators_, train_score_ [n_estimators_], val_score [n_estimators_] or None, init [Kz],
  learning_rate, max_depth)"""
  dense, csr, N, G = _gbt_input(x)
  K = int(n_classes)
  if not 2 <= K <= GBT_MAX_CLASSES:
    raise ValueError(f"gradient boosting takes 2 .. {GBT_MAX_CLASSES} classes, got {n_classes}")
  lab = _label_ids(labels, N, K, f"[{N}] integers")
  empty = np.flatnonzero(np.bincount(lab, minlength=K) == 0)
  if empty.size:
    raise ValueError(f"class {int(empty[0])} has no row")
  d, mss, msl, pp = _gbt_tree_params(max_depth, min_samples_split, min_samples_leaf, pass_pairs)
  S, lr = int(n_estimators), float(learning_rate)
  if S < 1:
    raise ValueError(f"n_estimators must be >= 1, got {n_estimators}")
  if not (np.isfinite(lr) and lr > 0):
    raise ValueError(f"learning_rate must be finite and > 0, got {learning_rate}")
  early = n_iter_no_change is not None
  vd = vc = vlab = None
  Nv, patience = 0, 0
  if early:
    patience = int(n_iter_no_change)
    if patience < 1 or not np.isfinite(float(tol)):
      raise ValueError(f"n_iter_no_change must be >= 1 and tol finite, got {n_iter_no_change} and {tol}")
    if x_val is None or labels_val is None:
      raise ValueError("early stopping takes x_val and labels_val")
    vd, vc, Nv, Gv = _gbt_input(x_val)
    if Gv != G:
      raise ValueError(f"x_val must have {G} columns, got {Gv}")
    vlab = _label_ids(labels_val, Nv, K, f"[{Nv}] integers")
  Kz, M = (1 if K == 2 else K), 2 ** (d + 1) - 1
  init = gbt_init_raw(lab, K)
  lib = _hip.require_gpu()
  out = _gbt_tree_outputs((S, Kz, M))
  done, train, val = C.c_int32(), np.zeros((S,), np.float64), np.zeros((S,), np.float64)
  check(lib.smx_gbt_fit(*_matrix_ptrs(dense, csr), N, G, _ip(lab), K, *(_matrix_ptrs(vd, vc) if early else (None,) * 4), Nv, _ip(vlab), S, lr, d,
                        mss, msl, patience, float(tol), pp, _dp(init), *_gbt_tree_ptrs(out), C.byref(done), _dp(train),
                        _dp(val) if early else None))
  s = done.value
  out = {name: a[:s].copy() for name, a in out.items()}
  out.update(n_estimators_=s, train_score_=train[:s].copy(), val_score=val[:s].copy() if early else None, init=init, learning_rate=lr,
             max_depth=d)
  return out


def k_gbt_decision(x, trees, init, learning_rate: float, block_rows: int = 0, n_stages=None):
  """smx_gbt_decision: the raw scores float64 [N, Kz] of the rows of x (dense or scipy.sparse) under the tree arrays [S, Kz, M] of `trees`
  (k_gbt_fit's dict): init, then stage by stage + learning_rate * the leaf value.  n_stages: the first stages only.  The matrix is
  streamed in blocks of block_rows rows (0: the library's choice; it changes no bit)."""
  dense, csr, N, G = _gbt_input(x, block_rows, resident=False)
  f = np.ascontiguousarray(trees["feature"], dtype=np.int32)
  if f.ndim != 3 or not 1 <= f.shape[1] <= GBT_MAX_CLASSES:
    raise ValueError(f"the tree arrays must be [stages, 1 .. {GBT_MAX_CLASSES}, M], got {f.shape}")
  S, Kz, M = f.shape
  d = int(M + 1).bit_length() - 2
  if M != 2 ** (d + 1) - 1 or not 1 <= d <= GBT_MAX_DEPTH:
    raise ValueError(f"a tree has 2^(max_depth + 1) - 1 slots, max_depth 1 .. {GBT_MAX_DEPTH}, got {M}")
  s = S if n_stages is None else int(n_stages)
  if not 0 <= s <= S:
    raise ValueError(f"n_stages must be 0 .. {S}, got {n_stages}")
  arr = {name: np.ascontiguousarray(trees[name], dtype=dtype) for name, dtype in _TREE_ARRAYS[:5]}
  if any(a.shape != f.shape for a in arr.values()):
    raise ValueError("the tree arrays differ in shape")
  node = np.arange(M)[None, None, :]
  split = f >= 0
  if f.min(initial=0) < -1 or f.max(initial=-1) >= G:
    raise ValueError(f"a tree splits on a feature outside 0 .. {G - 1}")
  for side in ("left", "right"):
    if ((arr[side] <= node) | (arr[side] >= M))[split].any():
      raise ValueError("a tree's child lies outside the tree")
  b = np.ascontiguousarray(init, dtype=np.float64)
  if b.shape != (Kz,) or not np.isfinite(b).all() or not np.isfinite(float(learning_rate)):
    raise ValueError(f"init must be [{Kz}] and finite, and learning_rate finite")
  lib = _hip.require_gpu()
  raw = np.empty((N, Kz), np.float64)
  check(lib.smx_gbt_decision(*_matrix_ptrs(dense, csr), N, G, int(block_rows), s, Kz, d, _ip(arr["feature"]), _fp(arr["threshold"]),
                             _ip(arr["left"]), _ip(arr["right"]), _dp(arr["value"]), _dp(b), float(learning_rate), _dp(raw)))
  return raw
