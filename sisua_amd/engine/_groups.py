"""Moments and rank sums of genes between cell groups (smx_rankgroups.hip): what the t-test and Wilcoxon rankings close on the host."""
from __future__ import annotations

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _f32, _fp, _ip, _label_ids, _matrix_ptrs, _ptr
from sisua_amd.engine._prep import _prep_input

RANK_MAX_CELLS = 1 << 20    # smx_group_ranksums: 2 N^2 and N^3 stay inside int64
RANK_MAX_GROUPS = 256        # smx_group_ranksums: the LDS accumulators
MOMENT_MAX_GROUPS = 65535    # smx_group_moments
MOMENT_MAX_ACC = 1 << 26     # smx_group_moments: n_groups x (n_genes rounded up to 4)


def _group_labels(labels, N, n_groups, max_groups):
  """labels [N] of integers in 0 .. n_groups - 1 -> int32, checked here so that a refusal never asks for the device"""
  K = int(n_groups)
  if not 1 <= K <= max_groups:
    raise ValueError(f"n_groups must be in 1 .. {max_groups}, got {n_groups}")
  return _label_ids(labels, N, K, f"integers [{N}]"), K


def k_group_moments(x, labels, n_groups: int, block_rows: int = 0) -> dict:
  """smx_group_moments: a dense or scipy.sparse matrix [N, G] and labels [N] in 0 .. n_groups - 1 -> dict(count [K] int64, and per group
  and gene sum [K, G] float64, css [K, G] float64 (the centred sum of squares about sum / count) and nnz [K, G] int64 (values != 0))"""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  lab, K = _group_labels(labels, N, n_groups, MOMENT_MAX_GROUPS)
  if K * ((G + 3) // 4 * 4) > MOMENT_MAX_ACC:
    raise ValueError(f"{K} groups x {G} genes pass the {MOMENT_MAX_ACC} accumulators of the group moments; take the genes in parts")
  lib = _hip.require_gpu()
  out = dict(count=np.empty((K,), np.int64), sum=np.empty((K, G), np.float64), css=np.empty((K, G), np.float64),
             nnz=np.empty((K, G), np.int64))
  check(lib.smx_group_moments(*_matrix_ptrs(dense, csr), N, G, int(block_rows), _ip(lab), K, _ptr(out["count"]), _dp(out["sum"]),
                              _dp(out["css"]), _ptr(out["nnz"])))
  return out


def k_group_ranksums(cols, labels, n_groups: int, reference: int = -1):
  """smx_group_ranksums: cols [n_cols, N] float32 (gene-major, finite) and labels [N] in 0 .. n_groups - 1 -> (rank2_sum [K, n_cols] int64,
  tie_term int64: [n_cols] against the rest (reference = -1), [K, n_cols] against a reference group, whose own rows are 0)"""
  c = _f32(cols)
  if c.ndim != 2 or c.shape[0] < 1 or not 1 <= c.shape[1] <= RANK_MAX_CELLS:
    raise ValueError(f"cols must be [n_cols >= 1, 1 .. {RANK_MAX_CELLS} cells], got {c.shape}")
  n, N = c.shape
  lab, K = _group_labels(labels, N, n_groups, RANK_MAX_GROUPS)
  ref = int(reference)
  if not -1 <= ref < K:
    raise ValueError(f"reference must be -1 (the rest) or a group 0 .. {K - 1}, got {reference}")
  bad = np.flatnonzero(~np.isfinite(c).all(axis=1))
  if bad.size:
    raise ValueError(f"column {int(bad[0])} holds a value that is not finite")
  lib = _hip.require_gpu()
  rank2, tie = np.empty((K, n), np.int64), np.empty((n,) if ref < 0 else (K, n), np.int64)
  check(lib.smx_group_ranksums(_fp(c), n, N, _ip(lab), K, ref, _ptr(rank2), _ptr(tie)))
  return rank2, tie
