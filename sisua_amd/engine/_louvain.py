"""Louvain communities of a symmetric CSR graph and the modularity of a partition (smx_louvain.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _ip, _ptr

LOUVAIN_MAX_VERTICES, LOUVAIN_MAX_ENTRIES = 2 ** 24, 2 ** 31 - 1


def louvain_table_degree() -> int:
  """smx_louvain_table_degree: rows of up to this many stored entries are moved by one wave with a hash table in LDS, longer ones by one
  workgroup with a sort.  Needs no device."""
  return int(_hip.load().smx_louvain_table_degree())


def _louvain_graph(indptr, cols, weights, n):
  """The CSR arguments of smx_louvain*, shape- and range-checked so that a refusal never asks for the device; symmetry is the caller's
  (sisua_amd.communities) and the library's to check"""
  n = int(n)
  ip, cj = np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(cols, dtype=np.int32)
  if not 1 <= n <= LOUVAIN_MAX_VERTICES:
    raise ValueError(f"the graph must have 1 .. 2^24 vertices, got {n}")
  if ip.shape != (n + 1,) or ip[0] != 0 or (np.diff(ip) < 0).any() or cj.shape != (int(ip[-1]),) or ip[-1] > LOUVAIN_MAX_ENTRIES:
    raise ValueError(f"indptr must be [{n + 1}] from 0, not decreasing, and cols [indptr[-1] <= 2^31 - 1]")
  if cj.size and (cj.min() < 0 or cj.max() >= n):
    raise ValueError("cols holds an index outside 0 .. n - 1")
  w = None
  if weights is not None:
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != cj.shape or not (np.isfinite(w).all() and (w >= 0).all()):
      raise ValueError("weights must be one per entry, finite and >= 0")
  return ip, cj, w, n


def k_louvain(indptr, cols, weights, n, resolution: float = 1.0, tol: float = 1e-7, max_sweeps: int = 100, max_levels: int = 32) -> dict:
  """smx_louvain: the communities of the symmetric CSR graph (indptr [n + 1], cols, weights float64 or None for unit weights) ->
  dict(labels int64 [n] (ids by decreasing size, ties to the lowest member), n_communities, n_levels, and per level run modularity,
  level_size, sweeps, colours)"""
  ip, cj, w, n = _louvain_graph(indptr, cols, weights, n)
  resolution, tol, max_sweeps, max_levels = float(resolution), float(tol), int(max_sweeps), int(max_levels)
  if not (np.isfinite(resolution) and resolution >= 0 and np.isfinite(tol) and tol >= 0):
    raise ValueError(f"resolution and tol must be finite and >= 0, got {resolution} and {tol}")
  if max_sweeps < 1 or not 1 <= max_levels <= 4096:
    raise ValueError(f"max_sweeps >= 1 and 1 <= max_levels <= 4096 are required, got {max_sweeps} and {max_levels}")
  lib = _hip.require_gpu()
  labels, nc, nl = np.empty((n,), np.int32), C.c_int32(), C.c_int32()
  q, size = np.zeros((max_levels,), np.float64), np.zeros((max_levels,), np.int64)
  sweeps, colours = np.zeros((max_levels,), np.int32), np.zeros((max_levels,), np.int32)
  check(lib.smx_louvain(_ptr(ip), _ip(cj), _dp(w), n, resolution, tol, max_sweeps, max_levels, _ip(labels), C.byref(nc), C.byref(nl), _dp(q),
                        _ptr(size), _ip(sweeps), _ip(colours)))
  L = nl.value
  return dict(labels=labels.astype(np.int64), n_communities=int(nc.value), n_levels=int(L), modularity=q[:L], level_size=size[:L],
              sweeps=sweeps[:L], colours=colours[:L])


def k_modularity(indptr, cols, weights, n, labels, resolution: float = 1.0) -> float:
  """smx_louvain_modularity: Q of the partition labels [n] (ids in 0 .. n - 1) of the graph, with smx_louvain's integers and sum order"""
  ip, cj, w, n = _louvain_graph(indptr, cols, weights, n)
  lab = np.ascontiguousarray(labels, dtype=np.int32)
  if lab.shape != (n,) or lab.min() < 0 or lab.max() >= n:
    raise ValueError(f"labels must be [{n}] ids in 0 .. {n - 1}")
  resolution = float(resolution)
  if not (np.isfinite(resolution) and resolution >= 0):
    raise ValueError(f"resolution must be finite and >= 0, got {resolution}")
  lib = _hip.require_gpu()
  q = C.c_double()
  check(lib.smx_louvain_modularity(_ptr(ip), _ip(cj), _dp(w), n, _ip(lab), resolution, C.byref(q)))
  return float(q.value)
