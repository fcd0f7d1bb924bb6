"""Mini-batch k-means (smx_mbkmeans.hip): k-means++ seeding, one mini-batch step, nearest-centre prediction."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _ip, _matrix_ptrs
from sisua_amd.engine._prep import _prep_input

MBK_MAX_CLUSTERS = 256      # smx_mbkmeans_*
MBK_MAX_GENES = 32768
MBK_MAX_SEED_ROWS = 65536    # smx_mbkmeans_seed: one workgroup scans the block
MBK_MAX_TRIALS = 16
MBK_MAX_RESIDENT = 1 << 31   # smx_mbkmeans_seed / _step hold their block whole: rows x (genes rounded up to 4)


def _mbk_input(x, n_clusters, block_rows=0, resident=False):
  """The shared arguments of smx_mbkmeans_*, checked here so that a refusal never asks for the device -> (dense, csr, N, G, K)"""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  K = int(n_clusters)
  if not 2 <= K <= MBK_MAX_CLUSTERS:
    raise ValueError(f"n_clusters must be in 2 .. {MBK_MAX_CLUSTERS}, got {n_clusters}")
  if G > MBK_MAX_GENES or N >= 2 ** 31:
    raise ValueError(f"mini-batch k-means takes up to {MBK_MAX_GENES} columns and fewer than 2^31 rows, got {(N, G)}")
  if resident and (N + 63) // 64 * 64 * ((G + 3) // 4 * 4) > MBK_MAX_RESIDENT:
    raise ValueError(f"a block of {N} x {G} passes the {MBK_MAX_RESIDENT} entries held on the device at once; take fewer rows per block")
  if not np.isfinite(dense if csr is None else csr[2]).all():
    raise ValueError("x holds an entry that is not finite")
  return dense, csr, N, G, K


def _mbk_centres(centres, K, G):
  c = np.ascontiguousarray(centres, dtype=np.float64)
  if c.ndim != 2 or c.shape[1] != G:
    raise ValueError(f"centres must be [n_clusters, {G}], got {c.shape}")
  return c


def k_mbkmeans_seed(x, K: int, first: int, u) -> dict:
  """smx_mbkmeans_seed: scikit-learn's k-means++ seeding of a dense or scipy.sparse block x [n, G] (taken as float32) with unit weights;
  first: the first centre's row, u [K - 1, T] float64 in [0, 1): the draws of every further centre's T local trials ->
  dict(indices [K] int32, centres [K, G] float64 (the chosen rows), potential [K] float64 (after each pick))"""
  dense, csr, N, G, K = _mbk_input(x, K, resident=True)
  uu = np.ascontiguousarray(u, dtype=np.float64)
  if uu.ndim != 2 or uu.shape[0] != K - 1 or not 1 <= uu.shape[1] <= MBK_MAX_TRIALS:
    raise ValueError(f"u must be [{K - 1}, 1 .. {MBK_MAX_TRIALS}], got {uu.shape}")
  if not ((uu >= 0) & (uu < 1)).all():
    raise ValueError("u must lie in [0, 1)")
  if not K <= N <= MBK_MAX_SEED_ROWS:
    raise ValueError(f"the seeding takes a block of n_clusters = {K} .. {MBK_MAX_SEED_ROWS} rows, got {N}")
  if not 0 <= int(first) < N:
    raise ValueError(f"first must be a row 0 .. {N - 1}, got {first}")
  lib = _hip.require_gpu()
  out = dict(indices=np.empty((K,), np.int32), centres=np.empty((K, G), np.float64), potential=np.empty((K,), np.float64))
  check(lib.smx_mbkmeans_seed(*_matrix_ptrs(dense, csr), N, G, K, uu.shape[1], int(first), _dp(uu), _ip(out["indices"]),
                              _dp(out["centres"]), _dp(out["potential"])))
  return out


def k_mbkmeans_step(x, centres, counts, want_labels: bool = True) -> dict:
  """smx_mbkmeans_step: one mini-batch step of a block x [n, G] without the reassignment: the labels against centres [K, G], then for every
  centre with m > 0 rows centre = (centre * count + the sum of its rows in row order) / (count + m) and count += m ->
  dict(centres [K, G], counts [K] float64 (new arrays), inertia (of the labels, before the update), labels [n] int32 or None)"""
  c = np.array(centres, dtype=np.float64, order="C", ndmin=2)
  dense, csr, N, G, K = _mbk_input(x, c.shape[0], resident=True)
  c = _mbk_centres(c, K, G)
  cnt = np.array(counts, dtype=np.float64, order="C")
  if cnt.shape != (K,) or not (np.isfinite(cnt).all() and (cnt >= 0).all()):
    raise ValueError(f"counts must be [{K}], finite and >= 0")
  lib = _hip.require_gpu()
  labels, inertia = (np.empty((N,), np.int32) if want_labels else None), C.c_double()
  check(lib.smx_mbkmeans_step(*_matrix_ptrs(dense, csr), N, G, K, _dp(c), _dp(cnt), _ip(labels), C.byref(inertia)))
  return dict(centres=c, counts=cnt, inertia=inertia.value, labels=labels)


def k_mbkmeans_predict(x, centres, block_rows: int = 0, want_distance: bool = False):
  """smx_mbkmeans_predict: the nearest of centres [K, G] for every row of a dense or scipy.sparse x [N, G], streamed in blocks of block_rows
  rows (0: the library's choice; it changes no bit) -> labels [N] int32, or (labels, squared distance [N] float64) with want_distance"""
  c = np.ascontiguousarray(centres, dtype=np.float64)
  dense, csr, N, G, K = _mbk_input(x, c.shape[0] if c.ndim == 2 else 0, block_rows)
  c = _mbk_centres(c, K, G)
  lib = _hip.require_gpu()
  labels, dist = np.empty((N,), np.int32), (np.empty((N,), np.float64) if want_distance else None)
  check(lib.smx_mbkmeans_predict(*_matrix_ptrs(dense, csr), N, G, int(block_rows), K, _dp(c), _ip(labels), _dp(dist)))
  return (labels, dist) if want_distance else labels
