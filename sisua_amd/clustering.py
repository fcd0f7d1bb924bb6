"""Clustering scores of a latent space (the reference's `clustering_scores`, sisua/analysis/latent_benchmarks.py:69-117): ASW on the true
labels, ARI / NMI / UCA between the true labels and k-means labels.  The two dense parts -- all N^2 distances of the silhouette and the
restarts of Lloyd's algorithm -- run on the device (smx_cluster.hip: `engine.k_cluster_silhouette`, `engine.k_cluster_kmeans`); what is here
is the small host arithmetic on their results, pure NumPy (UCA's assignment problem: SciPy's `linear_sum_assignment`), written after
scikit-learn's definitions of the four scores."""
from __future__ import annotations

from math import comb
from typing import Dict

import numpy as np

DEFAULT_SEED = 5218   # the reference's random_state


def prepare_labels(labels) -> np.ndarray:
  """The reference's label preparation: a 2-D `labels` (one-hot, or levels per class) is min-max normalised per column, then argmax; a 1-D
  one is taken as it is.  Returns int64 [cells]."""
  y = np.asarray(labels)
  if y.ndim == 2:
    y = y.astype(np.float64)
    lo, hi = y.min(axis=0, keepdims=True), y.max(axis=0, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
      y = (y - lo) / (hi - lo)
    return np.argmax(y, axis=-1).astype(np.int64)
  if y.ndim != 1:
    raise ValueError(f"labels must be [cells] or [cells, classes], got {y.shape}")
  if not np.issubdtype(y.dtype, np.integer):
    if not np.all(y == np.round(y)):
      raise ValueError("1-D labels must be whole numbers (class indices)")
    y = np.round(y)
  return y.astype(np.int64)


def silhouette_from_sums(a, b, singleton=None):
  """(score, samples) from the mean distances a (own class) and b (nearest other class) of every cell: s_i = (b - a) / max(a, b); s_i = 0
  where the cell's class is a singleton (`singleton` [cells] bool) or max(a, b) == 0.  The score is the mean of the samples."""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  if a.shape != b.shape or a.ndim != 1:
    raise ValueError(f"a and b must both be [cells], got {a.shape} and {b.shape}")
  m = np.maximum(a, b)
  with np.errstate(divide="ignore", invalid="ignore"):
    s = (b - a) / m
  s = np.where(m == 0.0, 0.0, s)
  if singleton is not None:
    s = np.where(np.asarray(singleton, bool), 0.0, s)
  return float(np.mean(s)), s


def contingency(y, y_pred) -> np.ndarray:
  """int64 table [classes of y, classes of y_pred] over the distinct values of each, in sorted order"""
  y, p = np.asarray(y).ravel(), np.asarray(y_pred).ravel()
  if y.shape != p.shape:
    raise ValueError(f"y and y_pred differ in length: {y.shape} and {p.shape}")
  _, yi = np.unique(y, return_inverse=True)
  _, pi = np.unique(p, return_inverse=True)
  t = np.zeros((int(yi.max()) + 1 if y.size else 0, int(pi.max()) + 1 if y.size else 0), np.int64)
  np.add.at(t, (yi, pi), 1)
  return t


def adjusted_rand(y, y_pred) -> float:
  """sklearn.metrics.adjusted_rand_score: the pair counts in Python integers, one float64 division"""
  t = contingency(y, y_pred)
  n = int(t.sum())
  pairs = comb(n, 2)
  both = sum(comb(int(v), 2) for v in t.ravel())               # pairs together in both
  same_y = sum(comb(int(v), 2) for v in t.sum(axis=1))
  same_p = sum(comb(int(v), 2) for v in t.sum(axis=0))
  tn, fp, fn, tp = pairs - same_y - same_p + both, same_p - both, same_y - both, both   # (of the pair confusion matrix, each halved)
  if fn == 0 and fp == 0:
    return 1.0
  return 2 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def _entropy(counts) -> float:
  c = np.asarray(counts, np.float64)
  c = c[c > 0]
  if c.size <= 1:
    return 0.0
  n = c.sum()
  return float(-np.sum((c / n) * (np.log(c) - np.log(n))))


def normalized_mutual_info(y, y_pred) -> float:
  """sklearn.metrics.normalized_mutual_info_score with its default arithmetic-mean normalisation"""
  t = contingency(y, y_pred)
  if t.shape[0] <= 1 and t.shape[1] <= 1:   # (both one class: a perfect match, as scikit-learn has it)
    return 1.0
  n = float(t.sum())
  ri, ci = np.nonzero(t)
  v = t[ri, ci].astype(np.float64)
  pi, pj = t.sum(axis=1).astype(np.float64), t.sum(axis=0).astype(np.float64)
  outer = pi[ri] * pj[ci]
  mi = float(np.sum((v / n) * (np.log(v) - np.log(n)) + (v / n) * (-np.log(outer) + 2.0 * np.log(n))))
  mi = max(mi, 0.0)
  if abs(mi) < np.finfo(np.float64).eps:
    return 0.0
  return mi / ((_entropy(pi) + _entropy(pj)) / 2.0)


def unsupervised_clustering_accuracy(y, y_pred) -> float:
  """The reference's UCA (latent_benchmarks.py:48-66, after scVI): the reward matrix [predicted, true] over the UNION of both label sets,
  the best one-to-one matching of predicted to true labels, the share of cells it gets right."""
  from scipy.optimize import linear_sum_assignment
  y, p = np.asarray(y).ravel(), np.asarray(y_pred).ravel()
  if y.shape != p.shape:
    raise ValueError(f"y and y_pred differ in length: {y.shape} and {p.shape}")
  u, inv = np.unique(np.concatenate((y, p)), return_inverse=True)
  reward = np.zeros((u.size, u.size), np.int64)
  np.add.at(reward, (inv[y.size:], inv[:y.size]), 1)
  rows, cols = linear_sum_assignment(reward.max() - reward)
  return float(int(reward[rows, cols].sum()) / p.size)


def draw_init_idx(n_cells: int, n_clusters: int, n_init: int, seed: int = DEFAULT_SEED) -> np.ndarray:
  """The starts of the restarts: n_init rows of n_clusters DISTINCT cells, row after row from one np.random.RandomState(seed).  int32"""
  rs = np.random.RandomState(seed)
  return np.stack([rs.choice(n_cells, n_clusters, replace=False) for _ in range(n_init)]).astype(np.int32)


def _check_latent(latent, labels, n_labels):
  z = np.asarray(latent)
  if z.ndim != 2 or z.shape[0] < 2:
    raise ValueError(f"latent must be [cells >= 2, D], got {z.shape}")
  if not (1 <= z.shape[1] <= 128):
    raise ValueError(f"the latent width must be 1 .. 128, got {z.shape[1]}")
  y = prepare_labels(labels)
  if y.shape[0] != z.shape[0]:
    raise ValueError(f"latent has {z.shape[0]} cells and labels {y.shape[0]}")
  n_labels = int(n_labels)
  if not (2 <= n_labels <= 256):
    raise ValueError(f"n_labels must be 2 .. 256, got {n_labels}")
  if n_labels > z.shape[0]:
    raise ValueError(f"n_labels = {n_labels} clusters need at least as many cells, got {z.shape[0]}")
  if y.min() < 0 or y.max() >= n_labels:
    raise ValueError(f"labels must lie in 0 .. n_labels - 1 = {n_labels - 1}, got {int(y.min())} .. {int(y.max())}")
  if np.unique(y).size < 2:
    raise ValueError("the silhouette needs at least two classes with cells")
  return np.ascontiguousarray(z, dtype=np.float32), y


def clustering_scores(latent, labels, n_labels, prediction_algorithm="knn", n_init=200, seed=DEFAULT_SEED, max_iter=300) -> Dict[str, float]:
  """{'ASW', 'ARI', 'NMI', 'UCA'} of a latent space [cells, D] (latent_benchmarks.py:69-117; higher is better for all four): the silhouette
  on the TRUE labels, the other three between the true labels and the labels of k-means with n_labels clusters -- `n_init` restarts of
  Lloyd's algorithm from random cells (np.random.RandomState(seed), see `draw_init_idx`), the restart of lowest inertia.  Distances and
  restarts run on the device.  labels: [cells] class indices, or 2-D (see `prepare_labels`).  Only prediction_algorithm='knn' (the
  reference's name for k-means) is built."""
  if prediction_algorithm in ("gmm", "both"):
    raise NotImplementedError(f"prediction_algorithm={prediction_algorithm!r} needs the Gaussian-mixture predictor, which is not built: "
                              "only 'knn' (k-means) is")
  if prediction_algorithm != "knn":
    raise ValueError(f"Not support for prediction_algorithm: '{prediction_algorithm}'")
  z, y = _check_latent(latent, labels, n_labels)
  n_init, max_iter = int(n_init), int(max_iter)
  if not (1 <= n_init <= 4096) or max_iter < 1:
    raise ValueError(f"n_init must be 1 .. 4096 and max_iter >= 1, got {n_init} and {max_iter}")
  from sisua_amd.engine import k_cluster_kmeans, k_cluster_silhouette
  a, b = k_cluster_silhouette(z, y, int(n_labels))
  counts = np.bincount(y, minlength=int(n_labels))
  asw, _ = silhouette_from_sums(a, b, singleton=counts[y] == 1)
  km = k_cluster_kmeans(z, draw_init_idx(z.shape[0], int(n_labels), n_init, seed), max_iter=max_iter)
  pred = km["labels"]
  return dict(ASW=asw, ARI=adjusted_rand(y, pred), NMI=normalized_mutual_info(y, pred), UCA=unsupervised_clustering_accuracy(y, pred))


# ---- the reference's complete function: k-means, the Gaussian mixture, or both -------------------------------------------------------
def _mixture_labels(z, n_labels, seed, n_init, max_iter):
  from sisua_amd.engine import k_cluster_kmeans
  from sisua_amd.mixture import GaussianMixture, starts_from_kmeans
  km = k_cluster_kmeans(z, draw_init_idx(z.shape[0], n_labels, n_init, seed), max_iter=max_iter, all_labels=True)
  gm = GaussianMixture(n_labels, random_state=seed, kmeans_n_init=n_init, kmeans_max_iter=max_iter)
  labels = gm._fit_from_labels(z, starts_from_kmeans(km, 1))
  return dict(labels=labels, kmeans_labels=km["labels"], mixture=gm)


def mixture_labels(latent, n_labels, seed=DEFAULT_SEED, n_init=200, max_iter=300) -> dict:
  """The two predicted labelings of the reference's `clustering_scores` from ONE run of the k-means restarts: dict(kmeans_labels -- the
  restart of lowest inertia --, labels -- those of `mixture.GaussianMixture(n_labels)` (full covariances, max_iter 100, tol 1e-3, reg_covar
  1e-6) started from that partition --, mixture: the fitted instance).  n_init, seed, max_iter: of the k-means restarts."""
  from sisua_amd.mixture import check_cells, check_settings
  n_labels, n_init, max_iter = int(n_labels), int(n_init), int(max_iter)
  check_settings(n_labels, 1e-3, 1e-6, 100, 1, n_init, max_iter)   # (the mixture's own settings are its defaults)
  z = check_cells(latent, n_labels)
  return _mixture_labels(z, n_labels, seed, n_init, max_iter)


def latent_scores(latent, labels, n_labels, prediction_algorithm="both", n_init=200, seed=DEFAULT_SEED, max_iter=300) -> Dict[str, float]:
  """The reference's `clustering_scores` with its default (latent_benchmarks.py:69-117): {'ASW', 'ARI', 'NMI', 'UCA'} of a latent space with
  the predicted labels of 'knn' (k-means: exactly `clustering_scores`), 'gmm' (the full-covariance Gaussian mixture, `mixture_labels`) or
  'both': the per-key average (v1 + v2) / 2 of the two, ASW included as the reference has it.  The silhouette sums and the k-means restarts
  run once.  The mixture is built for a latent width of 1 .. 64."""
  if prediction_algorithm == "knn":
    return clustering_scores(latent, labels, n_labels, "knn", n_init=n_init, seed=seed, max_iter=max_iter)
  if prediction_algorithm not in ("gmm", "both"):
    raise ValueError(f"Not support for prediction_algorithm: '{prediction_algorithm}'")
  from sisua_amd.mixture import check_cells, check_settings
  z, y = _check_latent(latent, labels, n_labels)
  n_init, max_iter = int(n_init), int(max_iter)
  check_settings(int(n_labels), 1e-3, 1e-6, 100, 1, n_init, max_iter)
  z = check_cells(z, int(n_labels))   # (the mixture's limits: a width of 1 .. 64, no non-finite entry)
  from sisua_amd.engine import k_cluster_silhouette
  a, b = k_cluster_silhouette(z, y, int(n_labels))
  counts = np.bincount(y, minlength=int(n_labels))
  asw, _ = silhouette_from_sums(a, b, singleton=counts[y] == 1)
  both = _mixture_labels(z, int(n_labels), seed, n_init, max_iter)
  score = lambda pred: dict(ASW=asw, ARI=adjusted_rand(y, pred), NMI=normalized_mutual_info(y, pred),
                            UCA=unsupervised_clustering_accuracy(y, pred))
  s2 = score(both["labels"])
  if prediction_algorithm == "gmm":
    return s2
  s1 = score(both["kmeans_labels"])
  return {k: (s1[k] + s2[k]) / 2 for k in s1}


# ---- mini-batch k-means of a whole matrix (the reference's SingleCellOMIC.clustering: _single_cell_analysis.py:679-700, 714-726) -----
BATCH_SIZE = 4096   # the reference's


def minibatch_kmeans(X, n_clusters, batch_size: int = BATCH_SIZE, random_state=1) -> np.ndarray:
  """The k-means part of the reference's `clustering` for a matrix without a container (an omic, a latent space): a
  `sisua_amd.MiniBatchKMeans(n_clusters, batch_size, compute_labels=False, random_state)` takes one `partial_fit` per batch of rows
  (s, min(s + batch_size, n)) in the order `RandomState(random_state).permutation(n_batches)` -- our reading of the reference's
  `odin.utils.batching(seed=...)`, which is not at hand -- and then predicts every row.  X: dense or scipy.sparse, never densified whole.
  Returns the labels [rows] int32.  The distance sweeps run on the device (smx_mbkmeans.hip)."""
  from sisua_amd.minibatch_kmeans import MiniBatchKMeans
  if getattr(X, "ndim", 0) != 2:
    raise ValueError(f"X must be a matrix [rows, features], got shape {getattr(X, 'shape', None)}")
  model = MiniBatchKMeans(n_clusters=n_clusters, batch_size=batch_size, compute_labels=False, random_state=random_state)
  n = X.shape[0]
  starts = np.arange(0, n, model.batch_size)
  for s in starts[np.random.RandomState(random_state).permutation(len(starts))]:
    model.partial_fit(X[int(s):int(min(s + model.batch_size, n))])
  return model.predict(X)


def match_clusters(labels, probs, n_clusters) -> np.ndarray:
  """ids [n_vars]: the cluster that takes each variable's name.  corr[i, c] = the float64 sum of probs[:, i] over the cells of cluster c;
  the linear assignment that maximises sum_i corr[i, ids[i]] -- our reading of the reference's `diagonal_linear_assignment`, which is
  not at hand."""
  from scipy.optimize import linear_sum_assignment
  p, lab = np.asarray(probs, np.float64), np.asarray(labels)
  corr = np.zeros((p.shape[1], int(n_clusters)), np.float64)
  for c in range(int(n_clusters)):
    corr[:, c] = p[lab == c].sum(axis=0)
  return linear_sum_assignment(corr, maximize=True)[1]
