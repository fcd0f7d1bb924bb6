"""Neighbour graphs on the device: exact PCA, exact k nearest neighbours and UMAP's fuzzy connectivities -- what the reference's
`SingleCellOMIC.dimension_reduce(algo='pca')` and `SingleCellOMIC.neighbors` compute through scikit-learn and scanpy
(sisua/data/_single_cell_analysis.py:385-451, 546-630).  Host code here is NumPy and SciPy only; everything of size N x G, N x C or N^2
runs in libsisua_hip.so (smx_pca.hip, smx_knn.hip; definitions in include/sisua_hip.h and DESIGN.md section 4v).

  pca(X, n_components)         -> (PCA, scores [N, C] float32)
  knn(Z, k)                    -> (idx [N, k] int32, dist [N, k] float64): the k OTHER cells nearest to each
  umap_connectivities(idx, dist) -> (connectivities, distances): the table's column 0 is the cell itself
  neighbors(Z, n_neighbors)    -> (connectivities, distances) of a latent space, e.g. model.encode's
  tsne_affinities(Z, perplexity) -> P, t-SNE's joint affinities, CSR float64
  tsne(Z, n_components, ...) / TSNE -> Y [N, C <= 3] float32: scikit-learn's t-SNE with the EXACT repulsive sum (smx_tsne.hip, section 4x)
  umap_layout(graph, ...)      -> Y [N, C <= 3] float32: UMAP's layout of a fuzzy graph, the per-epoch form (smx_umap.hip, section 4zd)
  umap(Z, n_neighbors, ...) / UMAP -> Y: kNN, connectivities and the layout

PCA here is EXACT: the eigen-decomposition of the two-pass float64 covariance.  The reference's IncrementalPCA over batches of 4096 rows
is exact PCA for one batch and an approximation of it for several.

Not built: UMAP's spectral init, `transform` of new cells, output metrics other than Euclidean, UMAP into more than 3 dimensions, parity
with umap-learn's random stream; Barnes-Hut / FFT approximations of t-SNE, t-SNE into more than 3 dimensions or with a perplexity above 85,
method='gauss', knn=False, metrics other than Euclidean, approximate neighbour search, PCA of matrices wider than 8192 columns."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

MAX_PCA_GENES = 8192     # smx_pca_cov: the covariance takes 8 G^2 bytes
MAX_KNN_DIM = 128        # smx_knn
MAX_NEIGHBORS = 257      # smx_knn: k <= 256 others, plus the cell itself
MAX_TSNE_COMPONENTS = 3  # smx_tsne_fit
MAX_PERPLEXITY = 85.0    # floor(3 perplexity + 1) <= 256 neighbours
MAX_UMAP_COMPONENTS = 3  # smx_umap_layout
MAX_UMAP_EPOCHS = 10000
MAX_UMAP_NEGATIVES = 64


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


# ---- t-SNE (smx_tsne.hip; definitions in include/sisua_hip.h and DESIGN.md section 4x) ----
def check_tsne_components(n_components) -> int:
  if isinstance(n_components, bool) or n_components != int(n_components) or not 1 <= int(n_components) <= MAX_TSNE_COMPONENTS:
    raise NotImplementedError(f"t-SNE embeds into at most {MAX_TSNE_COMPONENTS} dimensions here (n_components = 1, 2 or 3), got "
                              f"{n_components}: pass n_components=2, or use algo='pca' for wider representations")
  return int(n_components)


def _check_tsne_cells(Z, perplexity):
  """-> (Z float32 [cells, D], k): scikit-learn's support k = min(cells - 1, floor(3 perplexity + 1))"""
  if getattr(Z, "ndim", 0) == 2 and Z.shape[1] > MAX_KNN_DIM:
    raise ValueError(f"t-SNE of {Z.shape[1]} columns is not built: the exact neighbour search takes at most D <= {MAX_KNN_DIM}; reduce "
                     "the matrix first with pca(X, n_components)")
  Z = _check_cells(Z)
  n, perplexity = Z.shape[0], float(perplexity)
  if n < 4:
    raise ValueError(f"t-SNE needs at least 4 cells, got {n}")
  if not (np.isfinite(perplexity) and 1.0 <= perplexity <= MAX_PERPLEXITY):
    raise ValueError(f"perplexity must be in 1 .. {MAX_PERPLEXITY:g} (the support of 3 perplexity + 1 neighbours is at most "
                     f"{MAX_NEIGHBORS - 1} cells), got {perplexity}")
  if perplexity >= n:
    raise ValueError(f"perplexity must be below the number of cells ({n}), got {perplexity}")
  return Z, min(n - 1, int(3.0 * perplexity + 1.0))


def joint_probabilities(idx, cond_p):
  """The joint P of a table of conditional affinities (host only): A = the CSR of cond_p [N, k] at (i, idx), P = (A + A^T) / sum(A + A^T),
  float64 CSR [N, N] with sorted columns; explicit zeros are kept out."""
  idx, cond_p = np.asarray(idx), np.asarray(cond_p, dtype=np.float64)
  if idx.ndim != 2 or cond_p.shape != idx.shape:
    raise ValueError(f"idx and cond_p must share one shape [cells, k], got {idx.shape} and {cond_p.shape}")
  N, k = idx.shape
  if idx.size and (idx.min() < 0 or idx.max() >= N):
    raise ValueError("idx holds an index outside 0 .. cells - 1")
  A = sp.csr_matrix((cond_p.ravel(), idx.ravel().astype(np.int64), np.arange(0, N * k + 1, k)), shape=(N, N))
  P = (A + A.T).tocsr()
  P.sum_duplicates()
  P.eliminate_zeros()
  P.sort_indices()
  P /= P.sum()
  P.eliminate_zeros()   # (an entry that the division took below the smallest float64)
  return P


def tsne_affinities(Z, perplexity: float = 30.0):
  """The joint affinities P of t-SNE for the cells Z [cells >= 4, D <= 128], scikit-learn's: conditional Gaussians of the given perplexity
  on each cell's min(cells - 1, floor(3 perplexity + 1)) exact nearest neighbours, symmetrised -> scipy.sparse CSR float64"""
  Z, k = _check_tsne_cells(Z, perplexity)
  idx, dist = _engine().k_knn(Z, k)
  cond_p, _ = _engine().k_tsne_affinities(idx, dist, float(perplexity))
  return joint_probabilities(idx, cond_p)


def tsne_init(Z, n_components: int, init="pca", random_state=1):
  """The start of the descent, float64 [cells, C].  'pca': the first C exact-PCA scores of Z over the standard deviation of the first,
  times 1e-4 (scikit-learn's default; fewer than C columns in Z: the rest start at 0); 'random': RandomState(random_state)
  .standard_normal times 1e-4; or an array [cells, C]"""
  n, C = Z.shape[0], int(n_components)
  if isinstance(init, str):
    if init == "random":
      return np.random.RandomState(random_state).standard_normal((n, C)) * 1e-4
    if init != "pca":
      raise ValueError(f"init must be 'pca', 'random' or an array [cells, {C}], got {init!r}")
    scores = pca(Z, C)[1].astype(np.float64)
    if scores.shape[1] < C:
      scores = np.concatenate([scores, np.zeros((n, C - scores.shape[1]))], axis=1)
    sd = np.std(scores[:, 0])
    return scores / sd * 1e-4 if sd > 0 else scores
  Y0 = np.array(init, dtype=np.float64)
  if Y0.shape != (n, C):
    raise ValueError(f"init must be 'pca', 'random' or an array [{n}, {C}], got an array of shape {Y0.shape}")
  if not np.isfinite(Y0).all():
    raise ValueError("init holds an entry that is not finite")
  return Y0


class TSNE:
  """t-SNE with scikit-learn's objective, schedule and attribute names, the Barnes-Hut tree replaced by the exact sum over all pairs,
  float64 on the device (smx_tsne.hip).  After fit_transform: embedding_ [cells, C] float32 (the float64 result rounded once),
  kl_divergence_ (the last reported KL), n_iter_ (iterations run), learning_rate_, kl_trace_ [max_iter] (NaN where an iteration did not
  report).  Duplicated cells under init='pca' start and stay on top of each other, as in scikit-learn: equal positions get equal
  forces in the exact form."""

  def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
               n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", random_state=1):
    self.n_components, self.perplexity, self.early_exaggeration = n_components, perplexity, early_exaggeration
    self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, max_iter, n_iter_without_progress
    self.min_grad_norm, self.init, self.random_state = min_grad_norm, init, random_state

  def fit_transform(self, Z):
    C = check_tsne_components(self.n_components)
    Z, k = _check_tsne_cells(Z, self.perplexity)
    n, ee = Z.shape[0], float(self.early_exaggeration)
    if isinstance(self.learning_rate, str):
      if self.learning_rate != "auto":
        raise ValueError(f"learning_rate must be 'auto' or a positive number, got {self.learning_rate!r}")
      lr = max(n / ee / 4.0, 50.0)
    else:
      lr = float(self.learning_rate)
    if not (np.isfinite(ee) and ee > 0 and np.isfinite(lr) and lr > 0):
      raise ValueError(f"early_exaggeration and learning_rate must be finite and positive, got {ee} and {lr}")
    if int(self.max_iter) < 1 or int(self.n_iter_without_progress) < 0 or not float(self.min_grad_norm) >= 0:
      raise ValueError("max_iter must be >= 1, n_iter_without_progress >= 0 and min_grad_norm >= 0")
    if not isinstance(self.init, str):
      tsne_init(Z, C, self.init)   # (a refusal comes before any device work)
    elif self.init not in ("pca", "random"):
      raise ValueError(f"init must be 'pca', 'random' or an array [cells, {C}], got {self.init!r}")
    eng = _engine()
    idx, dist = eng.k_knn(Z, k)
    P = joint_probabilities(idx, eng.k_tsne_affinities(idx, dist, float(self.perplexity))[0])
    Y0 = tsne_init(Z, C, self.init, self.random_state)
    fit = eng.k_tsne_fit(P, Y0, int(self.max_iter), ee, lr, float(self.min_grad_norm), int(self.n_iter_without_progress))
    reported = fit["kl_trace"][~np.isnan(fit["kl_trace"])]
    self.embedding_ = fit["Y"].astype(np.float32)
    self.kl_divergence_ = float(reported[-1]) if reported.size else float("nan")
    self.kl_trace_, self.n_iter_, self.learning_rate_ = fit["kl_trace"], fit["n_iter"], lr
    return self.embedding_

  def fit(self, Z):
    self.fit_transform(Z)
    return self


def tsne(Z, n_components: int = 2, perplexity: float = 30.0, early_exaggeration: float = 12.0, learning_rate="auto", max_iter: int = 1000,
         n_iter_without_progress: int = 300, min_grad_norm: float = 1e-7, init="pca", random_state=1):
  """The t-SNE embedding of the cells Z [cells >= 4, D <= 128], e.g. a latent space or PCA scores -> Y [cells, n_components <= 3] float32
  (see `TSNE`)"""
  return TSNE(n_components, perplexity, early_exaggeration, learning_rate, max_iter, n_iter_without_progress, min_grad_norm, init,
              random_state).fit_transform(Z)


# ---- UMAP (smx_umap.hip; definitions in include/sisua_hip.h and DESIGN.md section 4zd) ----
def check_umap_components(n_components) -> int:
  if isinstance(n_components, bool) or n_components != int(n_components) or not 1 <= int(n_components) <= MAX_UMAP_COMPONENTS:
    raise NotImplementedError(f"UMAP embeds into at most {MAX_UMAP_COMPONENTS} dimensions here (n_components = 1, 2 or 3), got "
                              f"{n_components}: pass n_components=2, or use pca(X, n_components) for wider representations")
  return int(n_components)


def find_ab_params(spread: float = 1.0, min_dist: float = 0.5):
  """umap-learn's find_ab_params: a, b of 1 / (1 + a x^(2b)) fitted (scipy.optimize.curve_fit, its defaults) to the curve that is 1 up to
  min_dist and exp(-(x - min_dist) / spread) after, on 300 points of [0, 3 spread] -> (a, b) floats"""
  from scipy.optimize import curve_fit
  spread, min_dist = float(spread), float(min_dist)
  if not (np.isfinite(spread) and spread > 0 and np.isfinite(min_dist) and 0 <= min_dist <= spread):
    raise ValueError(f"spread must be finite and positive and 0 <= min_dist <= spread, got spread = {spread} and min_dist = {min_dist}")

  def curve(x, a, b):
    return 1.0 / (1.0 + a * x ** (2 * b))

  xv = np.linspace(0, spread * 3, 300)
  yv = np.zeros(xv.shape)
  yv[xv < min_dist] = 1.0
  yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
  params, _ = curve_fit(curve, xv, yv)
  return float(params[0]), float(params[1])


def umap_n_epochs(n_cells: int, n_epochs=None) -> int:
  """umap-learn's default: 500 epochs up to 10000 cells, 200 above; a given n_epochs must be in 1 .. 10000"""
  if n_epochs is None:
    return 500 if int(n_cells) <= 10000 else 200
  if isinstance(n_epochs, bool) or n_epochs != int(n_epochs) or not 1 <= int(n_epochs) <= MAX_UMAP_EPOCHS:
    raise ValueError(f"n_epochs must be None or a whole number in 1 .. {MAX_UMAP_EPOCHS}, got {n_epochs}")
  return int(n_epochs)


def umap_prepare_graph(graph, n_epochs: int):
  """The graph as the layout takes it (host only; umap-learn's simplicial_set_embedding): a symmetric scipy.sparse matrix [cells, cells]
  of weights > 0 without diagonal -> CSR float64 [cells, cells] of epochs_per_sample = max / w, columns sorted, duplicates summed, the
  entries below max / n_epochs dropped (the cut is symmetric; a row may become empty: that cell never moves)"""
  if not sp.issparse(graph) or graph.ndim != 2 or graph.shape[0] != graph.shape[1]:
    raise ValueError(f"the graph must be a square scipy.sparse matrix over the cells, got {type(graph).__name__} of shape "
                     f"{getattr(graph, 'shape', None)}")
  n = graph.shape[0]
  if not 2 <= n < 2 ** 31:
    raise ValueError(f"a UMAP layout needs 2 .. 2^31 - 1 cells, got {n}")
  G = sp.csr_matrix(graph, dtype=np.float64, copy=True)
  G.sum_duplicates()
  G.sort_indices()
  if not np.isfinite(G.data).all() or (G.data < 0).any():
    raise ValueError("the graph's weights must be finite and not negative")
  G.eliminate_zeros()
  if (G.diagonal() != 0).any():
    raise ValueError("the graph holds entries on its diagonal: a cell is not its own neighbour")
  if (G != G.T).nnz:
    raise ValueError("the graph is not symmetric: symmetrise it first, e.g. with umap_connectivities")
  if G.nnz >= 2 ** 31:
    raise ValueError(f"the graph holds {G.nnz} entries, at most 2^31 - 1 are taken")
  if G.nnz:
    top = float(G.data.max())
    G.data[G.data < top / float(n_epochs)] = 0.0
    G.eliminate_zeros()
    G.data = top / G.data
  return G


def umap_normalise(Y0):
  """The start mapped per axis to [0, 10]: 10 (Y - min) / (max - min); an axis with max == min becomes 5 (float64)"""
  Y0 = np.asarray(Y0, dtype=np.float64)
  lo, hi = Y0.min(axis=0), Y0.max(axis=0)
  flat = hi == lo
  out = 10.0 * (Y0 - lo) / np.where(flat, 1.0, hi - lo)
  out[:, flat] = 5.0
  return out


def umap_init(n_cells: int, n_components: int, init="random", random_state=1, Z=None):
  """The start of the layout before umap_normalise, float64 [cells, C].  'random': RandomState(random_state).uniform(-10, 10); 'pca' (needs
  the cells Z): the first C exact-PCA scores (fewer than C columns in Z: the rest start at 0); or an array [cells, C]"""
  n, C = int(n_cells), int(n_components)
  if isinstance(init, str):
    if init == "spectral":
      raise NotImplementedError("init='spectral' is not built: use init='pca' (the default of `umap`), 'random' or an array")
    if init == "random":
      return np.random.RandomState(random_state).uniform(-10.0, 10.0, size=(n, C))
    if init != "pca":
      raise ValueError(f"init must be 'pca', 'random' or an array [cells, {C}], got {init!r}")
    if Z is None:
      raise ValueError("init='pca' needs the cells, which a graph does not hold: call umap(Z, ...) or pass the PCA scores as init")
    scores = pca(Z, C)[1].astype(np.float64)
    if scores.shape[1] < C:
      scores = np.concatenate([scores, np.zeros((n, C - scores.shape[1]))], axis=1)
    return scores
  Y0 = np.array(init, dtype=np.float64)
  if Y0.shape != (n, C):
    raise ValueError(f"init must be 'pca', 'random' or an array [{n}, {C}], got an array of shape {Y0.shape}")
  if not np.isfinite(Y0).all():
    raise ValueError("init holds an entry that is not finite")
  return Y0


def _umap_params(n_cells, n_components, min_dist, spread, n_epochs, alpha, gamma, negative_sample_rate, random_state):
  """every scalar of the layout, checked on the host -> (C, n_epochs, alpha, gamma, S, seed)"""
  C = check_umap_components(n_components)
  E = umap_n_epochs(n_cells, n_epochs)
  alpha, gamma = float(alpha), float(gamma)
  if not (np.isfinite(alpha) and alpha > 0):
    raise ValueError(f"alpha (the initial learning rate) must be finite and positive, got {alpha}")
  if not (np.isfinite(gamma) and gamma >= 0):
    raise ValueError(f"gamma (the repulsion strength) must be finite and >= 0, got {gamma}")
  S = negative_sample_rate
  if isinstance(S, bool) or S != int(S) or not 0 <= int(S) <= MAX_UMAP_NEGATIVES:
    raise ValueError(f"negative_sample_rate must be a whole number in 0 .. {MAX_UMAP_NEGATIVES}, got {negative_sample_rate}")
  if isinstance(random_state, bool) or not isinstance(random_state, (int, np.integer)) or not 0 <= int(random_state) < 2 ** 32:
    raise ValueError(f"random_state must be an integer in 0 .. 2^32 - 1 (it seeds RandomState and the negative samples), got {random_state!r}")
  spread, min_dist = float(spread), float(min_dist)
  if not (np.isfinite(spread) and spread > 0 and np.isfinite(min_dist) and 0 <= min_dist <= spread):
    raise ValueError(f"spread must be finite and positive and 0 <= min_dist <= spread, got spread = {spread} and min_dist = {min_dist}")
  return C, E, alpha, gamma, int(S), int(random_state)


def umap_layout(graph, n_components: int = 2, min_dist: float = 0.5, spread: float = 1.0, n_epochs=None, alpha: float = 1.0,
                gamma: float = 1.0, negative_sample_rate: int = 5, init="random", random_state=1, return_info: bool = False):
  """UMAP's layout of a symmetric fuzzy graph (e.g. `neighbors(Z)[0]`), umap-learn's simplicial_set_embedding with the optimiser in its
  PER-EPOCH form (every force of an epoch from the positions at its start; float64 on the device, smx_umap.hip) -> Y [cells, C <= 3]
  float32 (the float64 result rounded once).  init: 'random' (the default: a graph holds no cells to take a PCA of) or an array
  [cells, C]; the start is mapped per axis to [0, 10].  return_info: (Y, dict(n_epochs, a, b, graph = the prepared CSR of
  epochs_per_sample, init = the normalised start))"""
  n = graph.shape[0] if hasattr(graph, "shape") and len(graph.shape) == 2 else 0
  C, E, alpha, gamma, S, seed = _umap_params(n, n_components, min_dist, spread, n_epochs, alpha, gamma, negative_sample_rate, random_state)
  G = umap_prepare_graph(graph, E)
  Y0 = umap_normalise(umap_init(n, C, init, seed))
  a, b = find_ab_params(spread, min_dist)
  fit = _engine().k_umap_layout(G, Y0, E, a, b, gamma, alpha, S, seed)
  Y = fit["Y"].astype(np.float32)
  return (Y, dict(n_epochs=E, a=a, b=b, graph=G, init=Y0)) if return_info else Y


class UMAP:
  """UMAP with umap-learn's graph, schedule and attribute names and scanpy's defaults (min_dist = 0.5, spread = 1): exact neighbours,
  the fuzzy union, and the layout in its per-epoch form (smx_knn.hip, smx_umap.hip).  After fit_transform: embedding_ [cells, C]
  float32, graph_ (the connectivities, CSR float32), n_epochs_, a_, b_.  init='pca' (the default, as `TSNE` here), 'random' or an array."""

  def __init__(self, n_neighbors=12, n_components=2, min_dist=0.5, spread=1.0, n_epochs=None, alpha=1.0, gamma=1.0,
               negative_sample_rate=5, init="pca", random_state=1):
    self.n_neighbors, self.n_components, self.min_dist, self.spread, self.n_epochs = n_neighbors, n_components, min_dist, spread, n_epochs
    self.alpha, self.gamma, self.negative_sample_rate, self.init, self.random_state = alpha, gamma, negative_sample_rate, init, random_state

  def fit_transform(self, Z):
    if getattr(Z, "ndim", 0) == 2 and Z.shape[1] > MAX_KNN_DIM:
      raise ValueError(f"UMAP of {Z.shape[1]} columns is not built: the exact neighbour search takes at most D <= {MAX_KNN_DIM}; reduce "
                       "the matrix first with pca(X, n_components)")
    Z = _check_cells(Z)
    n = Z.shape[0]
    C, _, _, _, _, seed = _umap_params(n, self.n_components, self.min_dist, self.spread, self.n_epochs, self.alpha, self.gamma,
                                       self.negative_sample_rate, self.random_state)
    K = check_n_neighbors(self.n_neighbors, n)
    if not isinstance(self.init, str) or self.init != "pca":
      umap_init(n, C, self.init, seed)   # (a refusal comes before any device work)
    conn, _ = neighbors(Z, K)
    Y0 = umap_init(n, C, self.init, seed, Z)
    Y, info = umap_layout(conn, C, self.min_dist, self.spread, self.n_epochs, self.alpha, self.gamma, self.negative_sample_rate, Y0, seed,
                          return_info=True)
    self.embedding_, self.graph_, self.n_epochs_, self.a_, self.b_ = Y, conn, info["n_epochs"], info["a"], info["b"]
    return Y

  def fit(self, Z):
    self.fit_transform(Z)
    return self


def umap(Z, n_neighbors: int = 12, n_components: int = 2, min_dist: float = 0.5, spread: float = 1.0, n_epochs=None, alpha: float = 1.0,
         gamma: float = 1.0, negative_sample_rate: int = 5, init="pca", random_state=1):
  """The UMAP embedding of the cells Z [cells, D <= 128], e.g. a latent space or PCA scores -> Y [cells, n_components <= 3] float32 (see
  `UMAP`)"""
  return UMAP(n_neighbors, n_components, min_dist, spread, n_epochs, alpha, gamma, negative_sample_rate, init, random_state).fit_transform(Z)
