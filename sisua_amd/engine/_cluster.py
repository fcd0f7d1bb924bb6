"""Clustering scores of a latent space (smx_cluster.hip): silhouette distances and Lloyd's k-means."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _f32, _fp, _ip


def k_cluster_silhouette(Z, labels, n_labels: int):
  """smx_cluster_silhouette: cells Z [N, D] float32, classes labels [N] in 0 .. n_labels - 1 -> (a [N], b [N]) float64, the mean distance of
  every cell to its own class and to the nearest other one"""
  lib = _hip.require_gpu()
  z = _f32(Z)
  y = np.ascontiguousarray(labels, dtype=np.int32)
  if z.ndim != 2 or y.shape != (z.shape[0],):
    raise ValueError(f"Z must be [cells, D] and labels [cells], got {z.shape} and {y.shape}")
  a, b = np.empty((z.shape[0],), np.float64), np.empty((z.shape[0],), np.float64)
  check(lib.smx_cluster_silhouette(_fp(z), z.shape[0], z.shape[1], _ip(y), int(n_labels), _dp(a), _dp(b)))
  return a, b


def k_cluster_kmeans(Z, init_idx, max_iter: int = 300, all_labels: bool = False):
  """smx_cluster_kmeans: Lloyd's iterations on cells Z [N, D] float32 from the initial centres Z[init_idx [n_init, K]], every restart in one
  call -> dict(labels [N], centres [K, D], inertia [n_init], n_iter [n_init], best, and labels_all [n_init, N] when asked)"""
  lib = _hip.require_gpu()
  z = _f32(Z)
  idx = np.ascontiguousarray(init_idx, dtype=np.int32)
  if z.ndim != 2 or idx.ndim != 2:
    raise ValueError(f"Z must be [cells, D] and init_idx [n_init, K], got {z.shape} and {idx.shape}")
  (N, D), (R, K) = z.shape, idx.shape
  out = dict(labels=np.empty((N,), np.int32), centres=np.empty((K, D), np.float64), inertia=np.empty((R,), np.float64),
             n_iter=np.empty((R,), np.int32))
  best = C.c_int32(-1)
  every = np.empty((R, N), np.int32) if all_labels else None
  check(lib.smx_cluster_kmeans(_fp(z), N, D, K, _ip(idx), R, int(max_iter), _ip(out["labels"]), _dp(out["centres"]), _dp(out["inertia"]),
                               _ip(out["n_iter"]), C.byref(best), _ip(every)))
  out["best"] = int(best.value)
  if every is not None:
    out["labels_all"] = every
  return out
