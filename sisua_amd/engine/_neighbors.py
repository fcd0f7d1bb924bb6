"""Neighbour graphs and embeddings: PCA (smx_pca.hip), exact kNN and UMAP connectivities (smx_knn.hip), t-SNE (smx_tsne.hip), the UMAP
layout (smx_umap.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sisua_amd import _hip
from sisua_amd._hip import check
from sisua_amd.engine._args import _dp, _f32, _fp, _ip, _matrix_ptrs, _ptr
from sisua_amd.engine._prep import _prep_input

PCA_MAX_GENES = 8192       # smx_pca_cov / smx_pca_project: the covariance takes 8 G^2 bytes
PCA_MAX_COMPONENTS = 128    # smx_pca_project, per call
KNN_MAX_D, KNN_MAX_K = 128, 256


def _pca_input(x, block_rows):
  """The matrix of smx_pca_cov / smx_pca_project, checked here so that a refusal never asks for the device"""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  if G > PCA_MAX_GENES:
    raise ValueError(f"PCA of {G} columns is not built: the covariance route takes at most {PCA_MAX_GENES} "
                     "(8 G^2 bytes); select genes first, e.g. with filter_highly_variable_genes")
  return dense, csr, N, G


def k_pca_cov(x, block_rows: int = 0):
  """smx_pca_cov: a dense or scipy.sparse matrix [N >= 2, G <= 8192] -> (mean [G], cov [G, G]) float64, the two-pass covariance with
  n - 1 in the denominator"""
  dense, csr, N, G = _pca_input(x, block_rows)
  if N < 2:
    raise ValueError(f"a covariance needs at least 2 cells, got {N}")
  lib = _hip.require_gpu()
  mean, cov = np.empty((G,), np.float64), np.empty((G, G), np.float64)
  check(lib.smx_pca_cov(*_matrix_ptrs(dense, csr), N, G, int(block_rows), _dp(mean), _dp(cov)))
  return mean, cov


def k_pca_project(x, mean, components, block_rows: int = 0):
  """smx_pca_project: (x - mean) . components^T for mean [G] and components [C <= 128, G] float64 -> [N, C] float32"""
  dense, csr, N, G = _pca_input(x, block_rows)
  mu, w = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(components, dtype=np.float64)
  if mu.shape != (G,) or w.ndim != 2 or w.shape[1] != G or not 1 <= w.shape[0] <= PCA_MAX_COMPONENTS:
    raise ValueError(f"mean must be [{G}] and components [1 .. {PCA_MAX_COMPONENTS}, {G}], got {mu.shape} and {w.shape}")
  if not (np.isfinite(mu).all() and np.isfinite(w).all()):
    raise ValueError("mean and components must be finite")
  lib = _hip.require_gpu()
  out = np.empty((N, w.shape[0]), np.float32)
  check(lib.smx_pca_project(*_matrix_ptrs(dense, csr), N, G, int(block_rows), _dp(mu), _dp(w), w.shape[0], _fp(out)))
  return out


def k_knn(Z, k: int):
  """smx_knn: cells Z [N, D] float32 -> (idx [N, k] int32, dist [N, k] float64), the k other cells nearest to each by (d2, index)"""
  z = _f32(Z)
  k = int(k)
  if z.ndim != 2 or not 1 <= z.shape[1] <= KNN_MAX_D:
    raise ValueError(f"Z must be [cells, 1 <= D <= {KNN_MAX_D}], got {z.shape}")
  if not 1 <= k <= KNN_MAX_K or k >= z.shape[0]:
    raise ValueError(f"k must be in 1 .. {KNN_MAX_K} and below the number of cells ({z.shape[0]}), got {k}")
  if not np.isfinite(z).all():
    raise ValueError("Z holds an entry that is not finite")
  lib = _hip.require_gpu()
  idx, dist = np.empty((z.shape[0], k), np.int32), np.empty((z.shape[0], k), np.float64)
  check(lib.smx_knn(_fp(z), z.shape[0], z.shape[1], k, _ip(idx), _dp(dist)))
  return idx, dist


def k_knn_umap(idx, dist):
  """smx_knn_umap: a neighbour table idx / dist [N, K] whose column 0 is the cell itself -> (rho [N], sigma [N], weight [N, K]) float64"""
  ix, d = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float64)
  if ix.ndim != 2 or d.shape != ix.shape or not 2 <= ix.shape[1] <= KNN_MAX_K + 1 or ix.shape[0] < 1:
    raise ValueError(f"idx and dist must both be [cells, 2 <= K <= {KNN_MAX_K + 1}], got {ix.shape} and {d.shape}")
  N, K = ix.shape
  if ix.min() < 0 or ix.max() >= N:
    raise ValueError("idx holds an index outside 0 .. cells - 1")
  if not (np.isfinite(d).all() and (d >= 0).all()):
    raise ValueError("dist must be finite and non-negative")
  lib = _hip.require_gpu()
  rho, sigma, weight = np.empty((N,), np.float64), np.empty((N,), np.float64), np.empty((N, K), np.float64)
  check(lib.smx_knn_umap(_ip(ix), _dp(d), N, K, _dp(rho), _dp(sigma), _dp(weight)))
  return rho, sigma, weight


TSNE_MAX_COMPONENTS = 3


def k_tsne_affinities(idx, dist, perplexity: float):
  """smx_tsne_affinities: smx_knn's table idx / dist [N, k] (the k other cells) -> (cond_p [N, k], beta [N]) float64, scikit-learn's
  binary search for the perplexity, per row"""
  ix, d = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float64)
  if ix.ndim != 2 or d.shape != ix.shape or not 1 <= ix.shape[1] <= KNN_MAX_K:
    raise ValueError(f"idx and dist must both be [cells, 1 <= k <= {KNN_MAX_K}], got {ix.shape} and {d.shape}")
  N, k = ix.shape
  if N < 4 or k >= N:
    raise ValueError(f"t-SNE needs at least 4 cells and k below their number, got {N} cells and k = {k}")
  perplexity = float(perplexity)
  if not (np.isfinite(perplexity) and 1.0 <= perplexity < N):
    raise ValueError(f"perplexity must be in 1 .. below the number of cells ({N}), got {perplexity}")
  if ix.min() < 0 or ix.max() >= N:
    raise ValueError("idx holds an index outside 0 .. cells - 1")
  if not (np.isfinite(d).all() and (d >= 0).all()):
    raise ValueError("dist must be finite and non-negative")
  lib = _hip.require_gpu()
  cond_p, beta = np.empty((N, k), np.float64), np.empty((N,), np.float64)
  check(lib.smx_tsne_affinities(_ip(ix), _dp(d), N, k, perplexity, _dp(cond_p), _dp(beta)))
  return cond_p, beta


def _tsne_problem(P, Y):
  """The joint P (scipy.sparse CSR [N, N], sorted columns, entries > 0) and an embedding Y [N, 1 .. 3] as the t-SNE entries take them,
  checked here so that a refusal never asks for the device -> (indptr int64, cols int32, p float64, y float64)"""
  import scipy.sparse as sp
  if not sp.issparse(P) or P.format != "csr" or P.ndim != 2 or P.shape[0] != P.shape[1]:
    raise ValueError(f"P must be a square scipy.sparse CSR matrix, got {type(P).__name__} of shape {getattr(P, 'shape', None)}")
  N = P.shape[0]
  if not 4 <= N < 2 ** 31:
    raise ValueError(f"t-SNE needs at least 4 cells, got {N}")
  y = np.ascontiguousarray(Y, dtype=np.float64)
  if y.ndim != 2 or y.shape[0] != N or not 1 <= y.shape[1] <= TSNE_MAX_COMPONENTS:
    raise ValueError(f"Y must be [{N}, 1 .. {TSNE_MAX_COMPONENTS}], got {y.shape}")
  if not np.isfinite(y).all():
    raise ValueError("Y holds an entry that is not finite")
  indptr, cols = np.ascontiguousarray(P.indptr, dtype=np.int64), np.ascontiguousarray(P.indices, dtype=np.int32)
  p = np.ascontiguousarray(P.data, dtype=np.float64)
  if indptr.shape != (N + 1,) or indptr[0] != 0 or (np.diff(indptr) < 0).any() or indptr[-1] != cols.size or p.size != cols.size:
    raise ValueError("P's indptr does not describe its entries")
  if cols.size and (cols.min() < 0 or cols.max() >= N):
    raise ValueError("P holds a column outside 0 .. cells - 1")
  inner = np.ones(cols.size, bool)
  inner[indptr[:-1][indptr[:-1] < cols.size]] = False   # (the first entry of a row has no entry in front of it)
  if (np.diff(cols.astype(np.int64), prepend=-1)[inner] <= 0).any():
    raise ValueError("the columns of a row of P must increase strictly (sort_indices, sum_duplicates)")
  if not (np.isfinite(p).all() and (p > 0).all()):
    raise ValueError("every stored entry of P must be finite and positive (eliminate_zeros)")
  return indptr, cols, p, y


def k_tsne_gradient(P, Y, exaggeration: float = 1.0):
  """smx_tsne_gradient: one evaluation of the exact t-SNE objective at Y [N, C] for the joint P (CSR) -> (grad [N, C], KL, Z) float64"""
  indptr, cols, p, y = _tsne_problem(P, Y)
  exaggeration = float(exaggeration)
  if not (np.isfinite(exaggeration) and exaggeration > 0):
    raise ValueError(f"exaggeration must be finite and positive, got {exaggeration}")
  lib = _hip.require_gpu()
  grad, kl, Z = np.empty_like(y), C.c_double(), C.c_double()
  check(lib.smx_tsne_gradient(_ptr(indptr), _ip(cols), _dp(p), y.shape[0], y.shape[1], _dp(y), exaggeration,
                              _dp(grad), C.byref(kl), C.byref(Z)))
  return grad, kl.value, Z.value


def k_tsne_fit(P, Y0, max_iter: int = 1000, early_exaggeration: float = 12.0, learning_rate: float = 200.0, min_grad_norm: float = 1e-7,
               n_iter_without_progress: int = 300):
  """smx_tsne_fit: scikit-learn's descent of the exact objective from Y0 [N, C], resident on the device -> dict(Y, update, gains
  [N, C] float64, kl_trace [max_iter] (NaN where the iteration did not report), n_iter)"""
  indptr, cols, p, y0 = _tsne_problem(P, Y0)
  max_iter, nwp = int(max_iter), int(n_iter_without_progress)
  ee, lr, mgn = float(early_exaggeration), float(learning_rate), float(min_grad_norm)
  if max_iter < 1 or nwp < 0:
    raise ValueError(f"max_iter must be >= 1 and n_iter_without_progress >= 0, got {max_iter} and {nwp}")
  if not (np.isfinite(ee) and ee > 0 and np.isfinite(lr) and lr > 0 and mgn >= 0):
    raise ValueError(f"early_exaggeration and learning_rate must be finite and positive and min_grad_norm >= 0, got {ee}, {lr}, {mgn}")
  lib = _hip.require_gpu()
  Y, update, gains = np.empty_like(y0), np.empty_like(y0), np.empty_like(y0)
  trace, n_iter = np.empty((max_iter,), np.float64), np.zeros((1,), np.int32)
  check(lib.smx_tsne_fit(_ptr(indptr), _ip(cols), _dp(p), y0.shape[0], y0.shape[1], _dp(y0), max_iter, ee, lr,
                         mgn, nwp, _dp(Y), _dp(trace), _ip(n_iter), _dp(update), _dp(gains)))
  return dict(Y=Y, update=update, gains=gains, kl_trace=trace, n_iter=int(n_iter[0]))


UMAP_MAX_COMPONENTS = 3
UMAP_MAX_EPOCHS = 10000
UMAP_MAX_NEGATIVES = 64


def _umap_problem(E, Y):
  """The prepared graph E (scipy.sparse CSR [N, N] of epochs_per_sample: symmetric support and values, sorted columns, no diagonal,
  entries > 0) and an embedding Y [N, 1 .. 3] as smx_umap_layout takes them, checked here so that a refusal never asks for the device
  -> (indptr int64, cols int32, eps float64, y float64)"""
  import scipy.sparse as sp
  if not sp.issparse(E) or E.format != "csr" or E.ndim != 2 or E.shape[0] != E.shape[1]:
    raise ValueError(f"the graph must be a square scipy.sparse CSR matrix, got {type(E).__name__} of shape {getattr(E, 'shape', None)}")
  N = E.shape[0]
  if not 2 <= N < 2 ** 31:
    raise ValueError(f"a UMAP layout needs 2 .. 2^31 - 1 cells, got {N}")
  y = np.ascontiguousarray(Y, dtype=np.float64)
  if y.ndim != 2 or y.shape[0] != N or not 1 <= y.shape[1] <= UMAP_MAX_COMPONENTS:
    raise ValueError(f"Y must be [{N}, 1 .. {UMAP_MAX_COMPONENTS}], got {y.shape}")
  if not np.isfinite(y).all():
    raise ValueError("Y holds an entry that is not finite")
  indptr, cols = np.ascontiguousarray(E.indptr, dtype=np.int64), np.ascontiguousarray(E.indices, dtype=np.int32)
  eps = np.ascontiguousarray(E.data, dtype=np.float64)
  if indptr.shape != (N + 1,) or indptr[0] != 0 or (np.diff(indptr) < 0).any() or indptr[-1] != cols.size or eps.size != cols.size:
    raise ValueError("the graph's indptr does not describe its entries")
  if cols.size >= 2 ** 31:
    raise ValueError(f"the graph holds {cols.size} entries, at most 2^31 - 1 are taken")
  if cols.size and (cols.min() < 0 or cols.max() >= N):
    raise ValueError("the graph holds a column outside 0 .. cells - 1")
  inner = np.ones(cols.size, bool)
  inner[indptr[:-1][indptr[:-1] < cols.size]] = False   # (the first entry of a row has no entry in front of it)
  if (np.diff(cols.astype(np.int64), prepend=-1)[inner] <= 0).any():
    raise ValueError("the columns of a row of the graph must increase strictly (sort_indices, sum_duplicates)")
  if (cols == np.repeat(np.arange(N), np.diff(indptr))).any():
    raise ValueError("the graph holds an entry on the diagonal")
  if not (np.isfinite(eps).all() and (eps > 0).all()):
    raise ValueError("every epochs_per_sample must be finite and positive")
  if (E != E.T).nnz:
    raise ValueError("the graph is not symmetric")
  return indptr, cols, eps, y


def k_umap_layout(E, Y0, n_epochs: int, a: float, b: float, gamma: float = 1.0, initial_alpha: float = 1.0, negative_sample_rate: int = 5,
                  seed: int = 0, epoch_begin: int = 0, epoch_end=None, next_sample=None, next_negative=None):
  """smx_umap_layout: the epochs epoch_begin .. epoch_end - 1 (None: n_epochs) of the per-epoch UMAP layout from Y0 [N, C] on the prepared
  graph E (CSR of epochs_per_sample).  next_sample / next_negative [entries]: the schedule state at epoch_begin (None: the start of a
  run, e and e / negative_sample_rate) -> dict(Y [N, C], next_sample, next_negative [entries]) float64, the state at epoch_end"""
  indptr, cols, eps, y0 = _umap_problem(E, Y0)
  n_epochs, S, seed = int(n_epochs), int(negative_sample_rate), int(seed)
  if not 1 <= n_epochs <= UMAP_MAX_EPOCHS:
    raise ValueError(f"n_epochs must be in 1 .. {UMAP_MAX_EPOCHS}, got {n_epochs}")
  begin, end = int(epoch_begin), n_epochs if epoch_end is None else int(epoch_end)
  if not 0 <= begin <= end <= n_epochs:
    raise ValueError(f"the epochs must obey 0 <= epoch_begin <= epoch_end <= n_epochs = {n_epochs}, got {begin} and {end}")
  if not 0 <= S <= UMAP_MAX_NEGATIVES:
    raise ValueError(f"negative_sample_rate must be in 0 .. {UMAP_MAX_NEGATIVES}, got {S}")
  a, b, gamma, alpha = float(a), float(b), float(gamma), float(initial_alpha)
  if not (np.isfinite(a) and a >= 0 and np.isfinite(b) and b >= 0 and np.isfinite(gamma) and gamma >= 0):
    raise ValueError(f"a, b and gamma must be finite and >= 0, got {a}, {b} and {gamma}")
  if not np.isfinite(alpha):
    raise ValueError(f"initial_alpha must be finite, got {alpha}")
  if not 0 <= seed < 2 ** 64:
    raise ValueError(f"seed must be in 0 .. 2^64 - 1, got {seed}")
  if (next_sample is None) != (next_negative is None):
    raise ValueError("next_sample and next_negative come together or not at all")
  if next_sample is None:
    nxt, neg = eps.copy(), (eps / S if S > 0 else eps.copy())
  else:
    nxt, neg = np.array(next_sample, dtype=np.float64), np.array(next_negative, dtype=np.float64)
    if nxt.shape != eps.shape or neg.shape != eps.shape:
      raise ValueError(f"next_sample and next_negative must be [{eps.size}], one per entry, got {nxt.shape} and {neg.shape}")
    if not (np.isfinite(nxt).all() and np.isfinite(neg).all()):
      raise ValueError("next_sample and next_negative must be finite")
  lib = _hip.require_gpu()
  Y = np.empty_like(y0)
  check(lib.smx_umap_layout(_ptr(indptr), _ip(cols), _dp(eps), y0.shape[0], y0.shape[1], _dp(y0), n_epochs, begin, end, a, b, gamma, alpha, S,
                            seed, _dp(nxt), _dp(neg), _dp(Y)))
  return dict(Y=Y, next_sample=nxt, next_negative=neg)


def k_umap_pow(x, b: float):
  """smx_umap_pow: the device's pow(x, b) for x [n] float64, finite and > 0 -- the function the UMAP forces use (tests)"""
  x, b = np.ascontiguousarray(x, dtype=np.float64), float(b)
  if x.ndim != 1 or x.size < 1 or not (np.isfinite(x).all() and (x > 0).all()) or not np.isfinite(b):
    raise ValueError("x must be [n >= 1], finite and positive, and b finite")
  lib = _hip.require_gpu()
  out = np.empty_like(x)
  check(lib.smx_umap_pow(_dp(x), b, x.size, _dp(out)))
  return out
