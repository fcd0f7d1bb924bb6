"""Evaluation metrics of a fitted model as plain callables `metric(model) -> dict` (the reference's training-time metrics,
sisua/analysis/sc_metrics.py:244-402, without its callback machinery): `ImputationError`, `CorrelationScores`, `MutualInformation` and
`ClusteringScores` (with `clustering_scores`, the function it is made of); and the views of the full gene x protein matrices of
`SingleCellModel.correlation` / `mutual_information` that the reference's analysis reads (`correlation_list`, `marker_correlations`, and
`marker_scores`, which also takes the 'mi' matrix).  What needs the [cells, genes] mean of the gene output is reduced on the device (smx_impute.hip); the correlations over a few marker columns are SciPy's,
called as the reference calls them."""
from __future__ import annotations

from typing import Dict, Iterable, List, Mapping, Sequence, Tuple

import numpy as np

from sisua_amd.clustering import clustering_scores, latent_scores   # noqa: F401  (latent_benchmarks.py:69-117; distances, restarts and EM on the device)
from sisua_amd.data import SingleCellOMIC, corrupt as _corrupt, is_sparse


def _matrix(a):
  """The first omic of a SingleCellOMIC, or the array / scipy.sparse matrix itself."""
  return a.numpy() if isinstance(a, SingleCellOMIC) else a


def _handle(model, x, sample_shape, batch_size):
  return model._imputation_handle(x, None, sample_shape, batch_size)


class ImputationError:
  """`{'imp_med', 'imp_mean'}` of a model (sc_metrics.py:244-284): the cells are predicted from the corrupted counts with `sample_shape`
  draws, and the mean of the count distribution is compared with the original counts `inputs` -- the median absolute difference over all
  entries, and the mean over the changed cells of the per-cell medians.  corrupted=None: `data.corrupt(inputs)` with its defaults
  (dropout_rate 0.2, retain_rate 0.2, seed 8), made once."""

  def __init__(self, inputs, corrupted=None, sample_shape=1, batch_size=64):
    self.original = _matrix(inputs)
    self.corrupted = _matrix(corrupted) if corrupted is not None else _corrupt(self.original, inplace=False)
    if tuple(self.original.shape) != tuple(self.corrupted.shape):
      raise ValueError(f"inputs {tuple(self.original.shape)} and corrupted {tuple(self.corrupted.shape)} differ in shape")
    self.sample_shape, self.batch_size = sample_shape, int(batch_size)

  def __call__(self, model) -> Dict[str, float]:
    s = _handle(model, self.corrupted, self.sample_shape, self.batch_size).imputation_scores(self.original)
    return {"imp_med": s["imputation_med"], "imp_mean": s["imputation_mean"]}


def marker_pairs(gene_names: Sequence[str], protein_names: Sequence[str], markers: Mapping[str, str]) -> List[Tuple[int, int]]:
  """(gene index, extras column) of every protein in `protein_names` whose marker gene -- `markers[protein name]`, a mapping the CALLER
  supplies -- is in `gene_names`; in the order of the proteins."""
  where = {str(g): i for i, g in enumerate(gene_names)}
  return [(where[str(markers[str(p)])], j) for j, p in enumerate(protein_names) if str(p) in markers and str(markers[str(p)]) in where]


class CorrelationScores:
  """The four keys of sc_metrics.py:287-348: the NEGATED Pearson / Spearman correlations between the imputed expression of a marker gene
  and the level of its protein, mean and median over the pairs ({} without pairs).  inputs: the counts the prediction is made from;
  extras: the protein matrix [cells, proteins]; pairs: a list of (gene index, extras column) (see `marker_pairs`).  Only the marker genes'
  columns of the mean leave the device (`LazyCountOutput.mean_over_samples(genes=...)`)."""

  def __init__(self, inputs, extras, pairs: Iterable[Tuple[int, int]], sample_shape=1, batch_size=64):
    self.inputs = _matrix(inputs)
    ex = _matrix(extras)
    self.extras = np.asarray(ex.toarray() if is_sparse(ex) else ex, np.float64)
    self.pairs = [(int(g), int(p)) for g, p in pairs]
    if self.extras.ndim != 2 or self.extras.shape[0] != self.inputs.shape[0]:
      raise ValueError("extras must be [cells, proteins] for the cells of inputs")
    for g, p in self.pairs:
      if not (0 <= g < self.inputs.shape[1]) or not (0 <= p < self.extras.shape[1]):
        raise IndexError(f"pair {(g, p)} is outside genes 0 .. {self.inputs.shape[1] - 1} / extras columns 0 .. {self.extras.shape[1] - 1}")
    self.sample_shape, self.batch_size = sample_shape, int(batch_size)

  def __call__(self, model) -> Dict[str, float]:
    from scipy.stats import pearsonr, spearmanr
    if not self.pairs:
      return {}
    h = _handle(model, self.inputs, self.sample_shape, self.batch_size)
    if h.is_zero_inflated:
      h = h.count_distribution
    cols = h.mean_over_samples(genes=[g for g, _ in self.pairs])
    spearman, pearson = [], []
    for j, (_, p) in enumerate(self.pairs):
      spearman.append(-spearmanr(cols[:, j], self.extras[:, p]).correlation)
      pearson.append(-pearsonr(cols[:, j], self.extras[:, p])[0])
    return {"pearson_mean": float(np.mean(pearson)), "spearman_mean": float(np.mean(spearman)),
            "pearson_med": float(np.median(pearson)), "spearman_med": float(np.median(spearman))}


class ClusteringScores:
  """The scores of sc_metrics.py:351-402: `clustering_scores` of the mean of every latent posterior of the model against the protein
  levels `extras` [cells, proteins] -- labels = argmax(extras, 1), n_labels = the number of proteins.  One entry per latent (`ASW_0`, ...;
  `_1` is SCVI's library latent), plus the plain keys as the mean over the latents; all values NEGATED, as the reference does (a loss:
  lower is better).  inputs: the counts the cells are encoded from; prediction_algorithm: 'knn' (k-means, `clustering_scores`), or 'gmm' /
  'both' through `latent_scores`; kw: keywords of `clustering_scores` (n_init, seed, max_iter)."""

  def __init__(self, inputs, extras, batch_size=64, prediction_algorithm="knn", **kw):
    self.inputs = _matrix(inputs)
    ex = _matrix(extras)
    ex = np.asarray(ex.toarray() if is_sparse(ex) else ex)
    if ex.ndim != 2 or ex.shape[0] != self.inputs.shape[0] or ex.shape[1] < 2:
      raise ValueError("extras must be [cells, proteins >= 2] for the cells of inputs")
    self.labels, self.n_labels = np.argmax(ex, axis=1), int(ex.shape[1])
    self.batch_size, self.kw, self.prediction_algorithm = int(batch_size), dict(kw), prediction_algorithm

  def __call__(self, model) -> Dict[str, float]:
    scores, avg = {}, {}
    knn = self.prediction_algorithm == "knn"
    for idx, z in enumerate(model._latent_means(self.inputs, None, self.batch_size)):
      found = clustering_scores(z, self.labels, self.n_labels, **self.kw) if knn else \
          latent_scores(z, self.labels, self.n_labels, self.prediction_algorithm, **self.kw)
      for key, val in found.items():
        scores[f"{key}_{idx}"] = -val
        avg.setdefault(key, []).append(-val)
    scores.update({k: float(np.mean(v)) for k, v in avg.items()})
    return scores


class MutualInformation:
  """`{'mi_mean', 'mi_med'}` of a model, beside `CorrelationScores` and with its arguments: the NEGATED mutual information (nats;
  `sisua_amd.mutual_information`, scikit-learn's kNN estimators on the device) between the imputed expression of a marker gene and the
  level of its protein, mean and median over the pairs ({} without pairs).  Only the marker genes' columns of the mean leave the device."""

  def __init__(self, inputs, extras, pairs: Iterable[Tuple[int, int]], sample_shape=1, batch_size=64, n_neighbors=3):
    c = CorrelationScores(inputs, extras, pairs, sample_shape, batch_size)   # (the same checks)
    self.inputs, self.extras, self.pairs = c.inputs, c.extras, c.pairs
    self.sample_shape, self.batch_size, self.n_neighbors = sample_shape, int(batch_size), int(n_neighbors)

  def __call__(self, model) -> Dict[str, float]:
    if not self.pairs:
      return {}
    genes = [g for g, _ in self.pairs]
    mat = model.mutual_information(self.inputs, self.extras, sample_shape=self.sample_shape, batch_size=self.batch_size, genes=genes,
                                   n_neighbors=self.n_neighbors)
    mi = [-float(mat[j, p]) for j, (_, p) in enumerate(self.pairs)]
    return {"mi_mean": float(np.mean(mi)), "mi_med": float(np.median(mi))}


def correlation_list(pearson, spearman) -> List[Tuple[int, int, float, float]]:
  """`SingleCellOMIC.get_correlation`'s return (_single_cell_analysis.py:1199-1245) from the two [G, P] matrices: (gene index, protein
  index, pearson, spearman) of every pair, sorted by decreasing average of the two (the reference's `sorted(...)[::-1]`: among equal averages the later pair first); pairs whose
  average is NaN go last, in index order."""
  pe, sp = np.asarray(pearson, np.float64), np.asarray(spearman, np.float64)
  if pe.ndim != 2 or pe.shape != sp.shape:
    raise ValueError(f"pearson and spearman must be the same [genes, proteins], got {pe.shape} and {sp.shape}")
  avg = ((pe + sp) / 2.0).ravel()
  nan = np.isnan(avg)
  order = np.concatenate([np.flatnonzero(~nan)[np.argsort(avg[~nan], kind="stable")[::-1]], np.flatnonzero(nan)])
  P = pe.shape[1]
  return [(int(i // P), int(i % P), float(pe.flat[i]), float(sp.flat[i])) for i in order]


def marker_correlations(matrix, kind: str, gene_names: Sequence[str], protein_names: Sequence[str], markers: Mapping[str, str]) -> Dict[str, float]:
  """`Posterior._matrix_scores` (posterior.py:996-1024) of a 'pearson' or 'spearman' matrix [genes, proteins]: {f"{kind}_{gene}_{protein}":
  matrix[gene, protein]} for every protein of `markers` (protein name -> marker gene name, supplied by the caller) whose two names are known."""
  if kind not in ("pearson", "spearman"):
    raise NotImplementedError(f"No support for score_type='{kind}'")
  m = np.asarray(matrix, np.float64)
  if m.shape != (len(gene_names), len(protein_names)):
    raise ValueError(f"matrix must be [{len(gene_names)}, {len(protein_names)}], got {m.shape}")
  var1 = {str(n): i for i, n in enumerate(gene_names)}
  var2 = {str(n): i for i, n in enumerate(protein_names)}
  return {f"{kind}_{g}_{p}": float(m[var1[str(g)], var2[str(p)]]) for p, g in markers.items() if str(g) in var1 and str(p) in var2}


def marker_scores(matrix, kind: str, gene_names: Sequence[str], protein_names: Sequence[str], markers: Mapping[str, str]) -> Dict[str, float]:
  """`Posterior._matrix_scores` (posterior.py:996-1024) of a 'pearson', 'spearman', 'mi' or 'importance' matrix [genes, proteins]:
  `marker_correlations` (which refuses 'mi' and 'importance') with the third and fourth kinds: {f"{kind}_{gene}_{protein}": matrix[gene,
  protein]}.  'lasso' is not built."""
  if kind not in ("mi", "importance"):
    return marker_correlations(matrix, kind, gene_names, protein_names, markers)
  found = marker_correlations(matrix, "pearson", gene_names, protein_names, markers)   # (the same view; only the keys' prefix differs)
  return {kind + key[len("pearson"):]: value for key, value in found.items()}


def dci_scores(matrix, test_acc=None) -> Dict[str, float]:
  """Disentanglement, completeness and informativeness (Eastwood & Williams 2018, as disentanglement_lib states them) of an importance
  matrix [n_codes, n_factors] (`sisua_amd.importance_matrix`) -> dict(disentanglement, completeness, informativeness).
  disentanglement: per code 1 - entropy(row + 1e-11, base=n_factors), weighted by the row's share of the matrix's total;
  completeness: the mean over the factors of 1 - entropy(column + 1e-11, base=n_codes); informativeness: the mean of test_acc over the
  factors that have one (NaN without test_acc, or where every accuracy is NaN).  Entropies are scipy.stats.entropy's.  Defined without a
  NaN at the edges: with one factor (or one code) the logarithm's base is 1, and the score is 1 -- a single factor cannot be entangled
  with another; an all-zero matrix gives every row the weight 0, so disentanglement 0, and uniform columns, so completeness 0."""
  from scipy.stats import entropy
  m = np.abs(np.asarray(matrix, np.float64))
  if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1 or not np.isfinite(m).all():
    raise ValueError(f"matrix must be a finite [n_codes >= 1, n_factors >= 1], got {m.shape}")
  n_codes, n_factors = m.shape
  per_code = 1.0 - entropy(m.T + 1e-11, base=n_factors) if n_factors > 1 else np.ones(n_codes)
  total = m.sum()
  weight = m.sum(axis=1) / total if total > 0 else np.zeros(n_codes)
  per_factor = 1.0 - entropy(m + 1e-11, base=n_codes) if n_codes > 1 else np.ones(n_factors)
  info = float("nan")
  if test_acc is not None:
    acc = np.asarray(test_acc, np.float64).reshape(-1)
    if acc.shape != (n_factors,):
      raise ValueError(f"test_acc must be [{n_factors}], got {acc.shape}")
    info = float(np.nanmean(acc)) if np.isfinite(acc).any() else float("nan")
  return dict(disentanglement=float(np.sum(per_code * weight)), completeness=float(np.mean(per_factor)), informativeness=info)
