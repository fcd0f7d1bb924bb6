"""Louvain communities of a symmetric graph on the device (smx_louvain.hip: `engine.k_louvain`, `engine.k_modularity`) -- what the
reference's `SingleCellOMIC.louvain` asks of scanpy.tl.louvain (_single_cell_analysis.py:732-835), without scanpy, igraph or the louvain
package.  The method is deterministic: synchronous within the colour classes of a fixed colouring, every sum an exact integer of weights
quantised to 2^-30 of the largest (tests/louvain_ref.py restates it in NumPy, and the device reproduces that label
for label).  It makes no random choice, so there is no seed."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def check_adjacency(adjacency, use_weights: bool = False):
  """Any scipy.sparse matrix -> (indptr int64, cols int32, weights float64 or None, n) of its canonical CSR (duplicates summed, stored
  zeros dropped).  Refused with ValueError: not sparse, not square, an entry that is negative or not finite, a stored non-zero diagonal
  entry, a matrix that is not symmetric."""
  if not sp.issparse(adjacency):
    raise ValueError(f"adjacency must be a scipy.sparse matrix, got {type(adjacency).__name__}")
  if adjacency.ndim != 2 or adjacency.shape[0] != adjacency.shape[1]:
    raise ValueError(f"adjacency must be square, got {adjacency.shape}")
  if adjacency.shape[0] < 1:
    raise ValueError("adjacency has no vertex")
  A = sp.csr_matrix(adjacency, dtype=np.float64, copy=True)
  A.sum_duplicates()
  if not np.isfinite(A.data).all() or (A.data < 0).any():
    raise ValueError("adjacency holds an entry that is negative or not finite")
  A.eliminate_zeros()
  if A.diagonal().any():
    raise ValueError("adjacency holds a non-zero diagonal entry (a self loop)")
  if (A != A.T).nnz:
    raise ValueError("adjacency is not symmetric")
  A.sort_indices()
  return (np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32),
          np.ascontiguousarray(A.data, dtype=np.float64) if use_weights else None, int(A.shape[0]))


def _check_settings(resolution, tol=0.0, max_sweeps=1, max_levels=1):
  resolution, tol = float(resolution), float(tol)
  if not (np.isfinite(resolution) and resolution >= 0):
    raise ValueError(f"resolution must be finite and >= 0, got {resolution}")
  if not (np.isfinite(tol) and tol >= 0):
    raise ValueError(f"tol must be finite and >= 0, got {tol}")
  if int(max_sweeps) < 1 or not 1 <= int(max_levels) <= 4096:
    raise ValueError(f"max_sweeps >= 1 and 1 <= max_levels <= 4096 are required, got {max_sweeps} and {max_levels}")
  return resolution, tol, int(max_sweeps), int(max_levels)


def louvain(adjacency, resolution=1.0, use_weights=False, tol=1e-7, max_sweeps=100, max_levels=32, return_info=False):
  """The communities of the graph `adjacency` (any scipy.sparse matrix: symmetric, entries finite and >= 0, no self loop) -> int64 labels
  [n], the ids by decreasing size with ties to the lowest member.  use_weights=False takes unit weights on the stored support.
  resolution: the gamma of Q = sum_c (in_c / m2 - gamma (tot_c / m2)^2); a level ends when a sweep moves nothing, gains at most tol, or
  lowers Q, or after max_sweeps.  return_info: also dict(modularity, n_communities, n_levels, and per level run level_modularity,
  level_size, sweeps, colours)."""
  resolution, tol, max_sweeps, max_levels = _check_settings(resolution, tol, max_sweeps, max_levels)
  ip, cj, w, n = check_adjacency(adjacency, use_weights)
  from sisua_amd import engine
  out = engine.k_louvain(ip, cj, w, n, resolution=resolution, tol=tol, max_sweeps=max_sweeps, max_levels=max_levels)
  labels = np.asarray(out["labels"], dtype=np.int64)
  if not return_info:
    return labels
  L = int(out["n_levels"])
  return labels, dict(modularity=float(out["modularity"][L - 1]) if L else 0.0, n_communities=int(out["n_communities"]), n_levels=L,
                      level_modularity=np.asarray(out["modularity"], dtype=np.float64), level_size=np.asarray(out["level_size"], dtype=np.int64),
                      sweeps=np.asarray(out["sweeps"], dtype=np.int32), colours=np.asarray(out["colours"], dtype=np.int32))


def modularity(adjacency, labels, resolution=1.0, use_weights=False) -> float:
  """Q of the partition `labels` [n] (any values) of the graph, with `louvain`'s quantised integers and sum order"""
  resolution = _check_settings(resolution)[0]
  ip, cj, w, n = check_adjacency(adjacency, use_weights)
  lab = np.asarray(labels)
  if lab.shape != (n,):
    raise ValueError(f"labels must be [{n}], got {lab.shape}")
  from sisua_amd import engine
  return float(engine.k_modularity(ip, cj, w, n, np.unique(lab, return_inverse=True)[1].astype(np.int32), resolution=resolution))


def threshold_variables(x, nmin: int = 2, nmax: int = 5) -> np.ndarray:
  """The reference's `_threshold(x, 2, 5)` (_single_cell_analysis.py:47-61) with `sisua_amd.GaussianMixture`: 1-D mixtures of nmin ..
  nmax - 1 components on the values x [V], the model of highest AIC, the entries the component of highest mean takes -> bool [V]"""
  from sisua_amd.mixture import GaussianMixture
  x = np.asarray(x, dtype=np.float32).reshape(-1, 1)
  models = [GaussianMixture(n_components=k, random_state=1).fit(x) for k in range(int(nmin), int(nmax))]
  best = models[int(np.argmax([m.aic(x) for m in models]))]
  return best.predict(x) == int(np.argmax(best.means_.ravel()))


def community_names(ids, probs, var_names) -> dict:
  """id -> name, the reference's rule: the omic's probabilities summed over each community's cells, thresholded, the chosen variables'
  names joined with '_'.  An omic of fewer than 5 variables (fewer values than the mixtures need) names a community str(id)."""
  ids, var_names = np.asarray(ids), np.asarray(var_names)
  out = {}
  for c in np.unique(ids):
    if len(var_names) < 5:
      out[int(c)] = str(int(c))
    else:
      out[int(c)] = "_".join(str(v) for v in var_names[threshold_variables(np.asarray(probs)[ids == c].sum(axis=0, dtype=np.float64))])
  return out
