"""The reference's `ProbabilisticEmbedding` (sisua/label_threshold.py): one 1-D Gaussian mixture per protein column, whose posterior gives the
probability embedding (`predict_proba`, the `y_prob` SISUA trains on) and whose positive component's confidence interval gives the binary
one (`predict`, `y_bin`).  The mixtures are fitted and evaluated on the device (smx_gmm.hip: `engine.k_gmm1d_fit`, `engine.k_gmm1d_predict`),
every restart of every column in one call; what is here is the host's part: the seeds of the restarts, the order of the components, the
threshold.  A fitted instance holds NumPy arrays only.

Seeding is NOT scikit-learn's k-means start: restart r of column c starts from K distinct cells of the column's training vector, drawn by
ONE np.random.RandomState(random_state), column after column, restart after restart (`draw_init_raw`).  Not built: clip_quartile, the
one-component fallback for an ill-defined covariance (with reg_covar > 0 and diagonal covariances scikit-learn never raises it), the plots."""
from __future__ import annotations

import numpy as np


def training_vector(x, remove_zeros: bool = True) -> np.ndarray:
  """The raw training set of one column, as the reference's normalize(test_mode=False) forms it before the log: the positive cells in cell
  order, with ONE 0 in front if any cell was zero"""
  x = np.asarray(x, np.float32).ravel()
  if not remove_zeros:
    return x
  pos = x[x > 0]
  return pos if pos.size == x.size else np.concatenate([np.zeros((1,), np.float32), pos])


def draw_init_raw(X, n_components: int, n_init: int, random_state=8, remove_zeros: bool = True) -> np.ndarray:
  """float32 [C, n_init, K]: the raw values of the K distinct training cells every restart starts from"""
  X = np.asarray(X, np.float32)
  rs = np.random.RandomState(random_state)
  out = np.empty((X.shape[1], n_init, n_components), np.float32)
  for c in range(X.shape[1]):
    tv = training_vector(X[:, c], remove_zeros)
    if tv.size < n_components:
      raise ValueError(f"column {c} has {tv.size} training samples, fewer than the {n_components} components")
    for r in range(n_init):
      out[c, r] = tv[rs.choice(tv.size, n_components, replace=False)]
  return out


def ci_bound(loc, scale, ci_threshold: float):
  """The end of scipy.stats.norm.interval(|ci_threshold|, loc, scale) the reference thresholds at: the lower one for ci_threshold < 0"""
  from scipy.stats import norm
  z = float(norm.ppf(0.5 + abs(float(ci_threshold)) / 2.0))
  return loc - z * scale if ci_threshold < 0 else loc + z * scale


class ProbabilisticEmbedding:
  """fit(X [cells, classes]) -> predict_proba / predict / score_samples of matrices with the same columns"""

  def __init__(self, n_components_per_class=2, positive_component=1, log_norm=True, clip_quartile=0., remove_zeros=True, ci_threshold=-0.68,
               random_state=8, verbose=False, n_init=8, max_iter=120, tol=1e-3, reg_covar=1e-6):
    self.n_components_per_class = int(n_components_per_class)
    self.positive_component = int(positive_component)
    self.remove_zeros, self.log_norm, self.clip_quartile = bool(remove_zeros), bool(log_norm), float(clip_quartile)
    self.ci_threshold = float(ci_threshold)
    self.verbose, self.random_state = bool(verbose), random_state
    self.n_init, self.max_iter, self.tol, self.reg_covar = int(n_init), int(max_iter), float(tol), float(reg_covar)
    if self.clip_quartile > 0:
      raise ValueError("clip_quartile > 0 is not built: only clip_quartile = 0 is")
    if not (2 <= self.n_components_per_class <= 8):
      raise ValueError(f"n_components_per_class must be 2 .. 8, got {self.n_components_per_class}")
    if not (1 <= self.positive_component < self.n_components_per_class):
      raise ValueError(f"positive_component must be 1 .. n_components_per_class - 1, got {self.positive_component}")
    if not (0 <= abs(self.ci_threshold) <= 1):
      raise ValueError(f"|ci_threshold| must be at most 1, got {self.ci_threshold}")
    if not (1 <= self.n_init <= 64) or self.max_iter < 1 or not self.tol > 0 or not self.reg_covar >= 0:
      raise ValueError("n_init must be 1 .. 64, max_iter >= 1, tol > 0 and reg_covar >= 0")
    self._fit = None

  # ---- the fitted state -------------------------------------------------------------------------------------------------------------
  @classmethod
  def from_parameters(cls, weights, means, variances, **kwargs):
    """An instance that holds given mixtures [classes, K] (components in any order) without fitting"""
    w, m, v = (np.array(a, dtype=np.float64, ndmin=2) for a in (weights, means, variances))
    if w.ndim != 2 or m.shape != w.shape or v.shape != w.shape:
      raise ValueError(f"weights, means and variances must all be [classes, K], got {w.shape}, {m.shape} and {v.shape}")
    self = cls(n_components_per_class=w.shape[1], **kwargs)
    self._set(dict(weights=w, means=m, variances=v))
    return self

  def _set(self, res):
    keep = ("weights", "means", "variances", "lower_bound", "n_iter", "converged", "best", "n_train", "col_sum")
    self._fit = {k: np.array(res[k]) for k in keep if k in res}
    self._fit["order"] = np.argsort(self._fit["means"], axis=1, kind="stable").astype(np.int32)

  def _fitted(self):
    if self._fit is None:
      raise ValueError("this ProbabilisticEmbedding is not fitted: call fit(X) first")
    return self._fit

  @property
  def n_classes(self):
    return 0 if self._fit is None else int(self._fit["means"].shape[0])

  @property
  def means(self):
    """[n_components, n_classes], the components by increasing mean"""
    f = self._fitted()
    return np.take_along_axis(f["means"], f["order"], axis=1).T.copy()

  @property
  def precisions(self):
    """[n_components, n_classes], in the order of `means`"""
    f = self._fitted()
    return (1.0 / np.take_along_axis(f["variances"], f["order"], axis=1)).T

  @property
  def thresholds(self):
    """[n_classes]: the normalised value from which `predict` gives 1"""
    f = self._fitted()
    pos = f["order"][:, self.positive_component]
    rows = np.arange(pos.size)
    return ci_bound(f["means"][rows, pos], np.sqrt(f["variances"][rows, pos]), self.ci_threshold)

  # ---- main -------------------------------------------------------------------------------------------------------------------------
  def fit(self, X):
    from sisua_amd.engine import _gmm_matrix, k_gmm1d_fit
    x = _gmm_matrix(X, self.n_components_per_class)
    seeds = draw_init_raw(x, self.n_components_per_class, self.n_init, self.random_state, self.remove_zeros)
    res = k_gmm1d_fit(x, seeds, max_iter=self.max_iter, tol=self.tol, reg_covar=self.reg_covar, remove_zeros=self.remove_zeros,
                      log_norm=self.log_norm)
    rows = np.arange(x.shape[1])
    for k in ("lower_bound", "n_iter", "converged"):   # (of the best restart)
      res[k] = res[k][rows, res["best"]]
    self._set(res)
    if self.verbose:
      print(f"ProbabilisticEmbedding: {x.shape[1]} mixtures of {self.n_components_per_class}, {int(np.sum(res['converged']))} converged")
    return self

  def fit_transform(self, X, return_probabilities=True):
    self.fit(X)
    return self.predict_proba(X) if return_probabilities else self.predict(X)

  def _predict(self, X, score=False):
    from sisua_amd.engine import _gmm_matrix, k_gmm1d_predict
    f = self._fitted()
    x = _gmm_matrix(X)
    if x.shape[1] != self.n_classes:
      raise ValueError(f"Number of classes mis-match: fitted with {self.n_classes}, given {x.shape[1]}")
    return k_gmm1d_predict(x, f["weights"], f["means"], f["variances"], f["order"], self.positive_component, self.thresholds,
                           log_norm=self.log_norm, score=score)

  def predict(self, X):
    """float32 [cells, classes]: 1 where the normalised value reaches the threshold, else 0"""
    return self._predict(X)[1]

  def predict_proba(self, X):
    """float64 [cells, classes]: the mean responsibility of the components from `positive_component` up"""
    return self._predict(X)[0]

  def score_samples(self, X):
    """[cells]: the log-likelihood of every cell, averaged over the classes"""
    return np.mean(self._predict(X, score=True)[2], axis=1)

  def score(self, X, y=None):
    return float(np.mean(self.score_samples(X)))
