"""Neighbour graphs on the device: exact PCA, exact k nearest neighbours and UMAP's fuzzy connectivities -- what the reference's
`SingleCellOMIC.dimension_reduce(algo='pca')` and `SingleCellOMIC.neighbors` compute through scikit-learn and scanpy
(sisua/data/_single_cell_analysis.py:385-451, 546-630).  Host code here is NumPy and SciPy only; everything of size N x G, N x C or N^2
runs in libsisua_hip.so (smx_pca.hip, smx_knn.hip; definitions in include/sisua_hip.h and DESIGN.md section 4v).

  pca(X, n_components)         -> (PCA, scores [N, C] float32)
  knn(Z, k)                    -> (idx [N, k] int32, dist [N, k] float64): the k OTHER cells nearest to each
  umap_connectivities(idx, dist) -> (connectivities, distances): the table's column 0 is the cell itself
  neighbors(Z, n_neighbors)    -> (connectivities, distances) of a latent space, e.g. model.encode's

PCA here is EXACT: the eigen-decomposition of the two-pass float64 covariance.  The reference's IncrementalPCA over batches of 4096 rows
is exact PCA for one batch and an approximation of it for several.

Not built: t-SNE and UMAP embeddings, method='gauss', knn=False, metrics other than Euclidean, approximate neighbour search, PCA of
matrices wider than 8192 columns."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

MAX_PCA_GENES = 8192     # smx_pca_cov: the covariance takes 8 G^2 bytes
MAX_KNN_DIM = 128        # smx_knn
MAX_NEIGHBORS = 257      # smx_knn: k <= 256 others, plus the cell itself


def _engine():
  from sisua_amd import engine
  return engine


def _check_matrix(X):
  if getattr(X, "ndim", 0) != 2 or X.shape[0] < 1 or X.shape[1] < 1:
    raise ValueError(f"expected a matrix [cells, features], got shape {getattr(X, 'shape', None)}")
  if X.shape[1] > MAX_PCA_GENES:
    raise ValueError(f"PCA of {X.shape[1]} columns is not built: the covariance route takes at most {MAX_PCA_GENES} (8 G^2 bytes); "
                     "select genes first, e.g. with filter_highly_variable_genes")


def components_from_cov(cov, n_components: int):
  """The host part of the fit: numpy.linalg.eigh of the covariance -> (components [C, G], explained_variance [C], total variance).
  Components by decreasing eigenvalue; the sign of each makes its entry of largest magnitude positive, ties to the lowest column
  (scikit-learn's svd_flip(u_based_decision=False)); negative eigenvalues are clamped to 0."""
  cov = np.asarray(cov, dtype=np.float64)
  w, v = np.linalg.eigh(cov)
  w, v = w[::-1], v[:, ::-1]
  C = int(n_components)
  comp = np.ascontiguousarray(v[:, :C].T)
  big = np.argmax(np.abs(comp), axis=1)   # (the first of equals)
  comp *= np.where(comp[np.arange(C), big] < 0, -1.0, 1.0)[:, None]
  return comp, np.maximum(w[:C], 0.0), float(np.trace(cov))


class PCA:
  """A fitted exact PCA: mean_ [G], components_ [C, G], explained_variance_, explained_variance_ratio_, singular_values_ [C] (float64),
  n_samples_seen_; transform(X) projects on the device."""

  def __init__(self, mean, components, explained_variance, total_variance, n_samples):
    self.mean_ = np.ascontiguousarray(mean, dtype=np.float64)
    self.components_ = np.ascontiguousarray(components, dtype=np.float64)
    self.explained_variance_ = np.asarray(explained_variance, dtype=np.float64)
    self.n_samples_seen_ = int(n_samples)
    self.n_components_ = self.components_.shape[0]
    self.singular_values_ = np.sqrt(self.explained_variance_ * (self.n_samples_seen_ - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
      self.explained_variance_ratio_ = self.explained_variance_ / float(total_variance)

  def transform(self, X, block_rows: int = 0):
    """(X - mean_) . components_^T in float64, rounded once -> [cells, C] float32; X dense or scipy.sparse"""
    _check_matrix(X)
    if X.shape[1] != self.mean_.shape[0]:
      raise ValueError(f"the model has {self.mean_.shape[0]} features, X is {X.shape}")
    eng = _engine()
    step = eng.PCA_MAX_COMPONENTS
    parts = [eng.k_pca_project(X, self.mean_, self.components_[c:c + step], block_rows) for c in range(0, self.n_components_, step)]
    return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=1)

  def __repr__(self):
    return f"<PCA n_components={self.n_components_} n_features={self.mean_.shape[0]} n_samples={self.n_samples_seen_}>"


def pca(X, n_components: int = 100, block_rows: int = 0):
  """Exact PCA of a dense or scipy.sparse matrix [cells >= 2, features <= 8192] -> (PCA, scores [cells, min(n_components, features)])"""
  _check_matrix(X)
  if X.shape[0] < 2:
    raise ValueError(f"PCA needs at least 2 cells, got {X.shape[0]}")
  if int(n_components) < 1:
    raise ValueError(f"n_components must be >= 1, got {n_components}")
  C = min(int(n_components), X.shape[1])
  mean, cov = _engine().k_pca_cov(X, block_rows)
  comp, ev, total = components_from_cov(cov, C)
  model = PCA(mean, comp, ev, total, X.shape[0])
  return model, model.transform(X, block_rows)


def _check_cells(Z):
  Z = np.ascontiguousarray(Z, dtype=np.float32)
  if Z.ndim != 2 or not 1 <= Z.shape[1] <= MAX_KNN_DIM:
    raise ValueError(f"Z must be [cells, 1 <= D <= {MAX_KNN_DIM}], got {Z.shape}")
  if not np.isfinite(Z).all():
    raise ValueError("Z holds an entry that is not finite")
  return Z


def knn(Z, k: int):
  """The k other cells nearest to each cell of Z [cells, D <= 128] by (squared Euclidean distance in float64, index): exact, all pairs"""
  Z = _check_cells(Z)
  if not 1 <= int(k) <= MAX_NEIGHBORS - 1 or int(k) >= Z.shape[0]:
    raise ValueError(f"k must be in 1 .. {MAX_NEIGHBORS - 1} and below the number of cells ({Z.shape[0]}), got {k}")
  return _engine().k_knn(Z, int(k))


def assemble_graph(idx, dist, weight):
  """The sparse graphs of a neighbour table idx / dist / weight [N, K] (host only) -> (connectivities, distances), float32 CSR [N, N].
  A = the CSR of the weights; connectivities = A + A^T - A o A^T (the fuzzy union, set_op_mix_ratio = 1), distances = dist at (i, idx);
  explicit zeros are removed from both, as scanpy does: a duplicate at distance 0 leaves `distances` and stays in `connectivities`."""
  idx, dist, weight = np.asarray(idx), np.asarray(dist, dtype=np.float64), np.asarray(weight, dtype=np.float64)
  if idx.ndim != 2 or dist.shape != idx.shape or weight.shape != idx.shape:
    raise ValueError(f"idx, dist and weight must share one shape [cells, K], got {idx.shape}, {dist.shape} and {weight.shape}")
  N, K = idx.shape
  if idx.size and (idx.min() < 0 or idx.max() >= N):
    raise ValueError("idx holds an index outside 0 .. cells - 1")
  rows = np.repeat(np.arange(N), K)
  A = sp.coo_matrix((weight.ravel(), (rows, idx.ravel())), shape=(N, N)).tocsr()
  A.eliminate_zeros()
  T = A.T.tocsr()
  conn = (A + T - A.multiply(T)).tocsr()
  conn.eliminate_zeros()
  D = sp.coo_matrix((dist.ravel(), (rows, idx.ravel())), shape=(N, N)).tocsr()
  D.eliminate_zeros()
  return conn.astype(np.float32), D.astype(np.float32)


def umap_connectivities(idx, dist):
  """UMAP's fuzzy simplicial set (local_connectivity = 1, set_op_mix_ratio = 1) of a neighbour table idx / dist [N, K] whose column 0 is
  the cell itself at distance 0 and whose other columns are `knn`'s -> (connectivities, distances)"""
  _, _, weight = _engine().k_knn_umap(idx, dist)
  return assemble_graph(idx, dist, weight)


def check_n_neighbors(n_neighbors, n_cells: int) -> int:
  k = int(n_neighbors)
  if not 2 <= k <= min(MAX_NEIGHBORS, int(n_cells)):
    raise ValueError(f"n_neighbors must be in 2 .. min({MAX_NEIGHBORS}, cells = {n_cells}), got {n_neighbors}")
  return k


def self_table(idx, dist):
  """knn's table with the cell itself in front, at distance 0: the row UMAP's weights are defined on (width n_neighbors)"""
  N = idx.shape[0]
  return (np.concatenate([np.arange(N, dtype=np.int32)[:, None], idx], axis=1),
          np.concatenate([np.zeros((N, 1), np.float64), dist], axis=1))


def neighbors(Z, n_neighbors: int = 12):
  """The neighbour graph of the cells Z [cells, D <= 128], e.g. a latent space: each cell's n_neighbors - 1 nearest other cells, exact,
  weighted by UMAP's connectivities -> (connectivities, distances), scipy.sparse CSR float32 [cells, cells]"""
  Z = _check_cells(Z)
  K = check_n_neighbors(n_neighbors, Z.shape[0])
  return umap_connectivities(*self_table(*knn(Z, K - 1)))
