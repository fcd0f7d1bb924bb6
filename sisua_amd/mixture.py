"""`GaussianMixture`: scikit-learn's full-covariance Gaussian mixture with its EM loop on the device (smx_gmm_full.hip:
`engine.k_gmm_full_fit`, `engine.k_gmm_full_predict`).  It is the second predictor of the reference's clustering scores
(sisua/analysis/latent_benchmarks.py:69-117: `GaussianMixture(n_labels, random_state=5218)`).  The seeding is the host's: restarts of
Lloyd's algorithm from random cells (`clustering.draw_init_idx`, `engine.k_cluster_kmeans`), the `n_init` partitions of lowest inertia as
starting labelings.  Parity with scikit-learn's own k-means++ start and its random stream is not built; from the same starting labelling the
loop is scikit-learn's (tests/test_mixture_host.py)."""
from __future__ import annotations

import warnings

import numpy as np

from sisua_amd.clustering import DEFAULT_SEED, draw_init_idx

MAX_WIDTH, MAX_COMPONENTS, MAX_RESTARTS = 64, 256, 8


class ConvergenceWarning(UserWarning):
  """the EM loop ended at max_iter without meeting tol (scikit-learn's warning of the same name)"""


def check_cells(X, n_components) -> np.ndarray:
  """X [cells, D] as contiguous float32 within the limits of smx_gmm_full.hip, checked before the device is asked for"""
  x = np.asarray(X)
  if x.ndim != 2:
    raise ValueError(f"X must be [cells, D], got {x.shape}")
  if not (1 <= x.shape[1] <= MAX_WIDTH):
    raise ValueError(f"the full-covariance mixture is built for a width of 1 .. {MAX_WIDTH}, got {x.shape[1]}")
  if not (n_components <= x.shape[0] < 2 ** 31):
    raise ValueError(f"n_components = {n_components} needs at least as many cells (and fewer than 2^31), got {x.shape[0]}")
  x = np.ascontiguousarray(x, dtype=np.float32)
  if not np.all(np.isfinite(x)):
    raise ValueError("X holds a non-finite entry")
  return x


def check_settings(n_components, tol, reg_covar, max_iter, n_init, kmeans_n_init=1, kmeans_max_iter=1):
  n_components, max_iter, n_init, kmeans_n_init, kmeans_max_iter = (int(v) for v in (n_components, max_iter, n_init, kmeans_n_init, kmeans_max_iter))
  tol, reg_covar = float(tol), float(reg_covar)
  if not (2 <= n_components <= MAX_COMPONENTS):
    raise ValueError(f"n_components must be 2 .. {MAX_COMPONENTS}, got {n_components}")
  if max_iter < 1 or not (tol > 0 and np.isfinite(tol)) or not (reg_covar >= 0 and np.isfinite(reg_covar)):
    raise ValueError(f"max_iter >= 1, tol > 0 and reg_covar >= 0 are required, got {max_iter}, {tol} and {reg_covar}")
  if not (1 <= n_init <= MAX_RESTARTS):
    raise ValueError(f"n_init must be 1 .. {MAX_RESTARTS}, got {n_init}")
  if not (n_init <= kmeans_n_init <= 4096) or kmeans_max_iter < 1:
    raise ValueError(f"kmeans_n_init must be n_init .. 4096 and the k-means max_iter >= 1, got {kmeans_n_init} and {kmeans_max_iter}")


def starts_from_kmeans(km, n_init: int) -> np.ndarray:
  """int32 [n_init, cells]: the k-means restarts of lowest inertia, by increasing inertia with ties to the lower index (NaN last)"""
  inertia = np.where(np.isnan(km["inertia"]), np.inf, km["inertia"])
  return np.ascontiguousarray(km["labels_all"][np.argsort(inertia, kind="stable")[:n_init]], dtype=np.int32)


class GaussianMixture:
  """sklearn.mixture.GaussianMixture(covariance_type='full') with the EM loop on the device.  n_init: the number of EM restarts (1 .. 8),
  started from the `n_init` best of `kmeans_n_init` k-means restarts from random cells of np.random.RandomState(random_state); the restart
  of highest lower bound is kept.  Attributes after `fit`, NumPy arrays only: weights_ [K], means_ [K, D], covariances_ [K, D, D],
  precisions_cholesky_ [K, D, D] (upper triangular, scikit-learn's layout), lower_bound_, n_iter_, converged_.  Only covariance_type='full'
  and the k-means start are built: other covariance types, weights_init / means_init / precisions_init, init_params and warm_start are
  refused.  Two limits scikit-learn does not have: a width of 1 .. 64, and `predict`, `predict_proba`, `score_samples` and `score` refuse
  an X with fewer rows than components, as `fit` does (the limit of smx_gmm_full_predict: K <= n_cells)."""

  def __init__(self, n_components, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, random_state=DEFAULT_SEED,
               kmeans_n_init=200, kmeans_max_iter=300, **not_built):
    if covariance_type != "full":
      raise ValueError(f"covariance_type={covariance_type!r} is not built: only 'full' is (1-D diagonal mixtures: ProbabilisticEmbedding)")
    for name, value in not_built.items():
      if name in ("weights_init", "means_init", "precisions_init", "warm_start", "init_params"):
        if value is None or value is False or (name == "init_params" and value == "kmeans"):
          continue
        raise ValueError(f"{name} is not built: only covariance_type='full' from a k-means start (kmeans_n_init random-cell restarts) is")
      raise TypeError(f"GaussianMixture() got an unexpected keyword argument {name!r}")
    check_settings(n_components, tol, reg_covar, max_iter, n_init, kmeans_n_init, kmeans_max_iter)
    self.n_components, self.covariance_type = int(n_components), "full"
    self.tol, self.reg_covar, self.max_iter, self.n_init = float(tol), float(reg_covar), int(max_iter), int(n_init)
    self.random_state, self.kmeans_n_init, self.kmeans_max_iter = int(random_state), int(kmeans_n_init), int(kmeans_max_iter)

  # ---- fitting -----------------------------------------------------------------------------------------------------------------------
  def fit(self, X, y=None):
    self.fit_predict(X)
    return self

  def fit_predict(self, X, y=None) -> np.ndarray:
    x = check_cells(X, self.n_components)
    from sisua_amd.engine import k_cluster_kmeans
    km = k_cluster_kmeans(x, draw_init_idx(x.shape[0], self.n_components, self.kmeans_n_init, self.random_state),
                          max_iter=self.kmeans_max_iter, all_labels=True)
    return self._fit_from_labels(x, starts_from_kmeans(km, self.n_init))

  def _fit_from_labels(self, x, init_labels) -> np.ndarray:
    """the EM restarts from given starting labelings [R, cells]; returns the labels of the best one"""
    from sisua_amd.engine import k_gmm_full_fit
    out = k_gmm_full_fit(x, init_labels, max_iter=self.max_iter, tol=self.tol, reg_covar=self.reg_covar, n_components=self.n_components)
    b = out["best"]
    self.weights_, self.means_, self.covariances_ = out["weights"], out["means"], out["covariances"]
    self.precisions_cholesky_ = np.ascontiguousarray(np.swapaxes(out["chol_inv"], 1, 2))
    self.lower_bound_, self.n_iter_, self.converged_ = float(out["lower_bound"][b]), int(out["n_iter"][b]), bool(out["converged"][b])
    self.n_features_in_ = int(x.shape[1])
    if not self.converged_:
      warnings.warn(f"Best performing initialization did not converge. Try different init parameters, or increase max_iter, tol, or check "
                    f"for degenerate data. (max_iter = {self.max_iter}, tol = {self.tol})", ConvergenceWarning, stacklevel=3)
    return out["labels"].astype(np.int64)

  # ---- a fitted mixture ----------------------------------------------------------------------------------------------------------------
  def _e_step(self, X, **want):
    if not hasattr(self, "weights_"):
      raise RuntimeError("This GaussianMixture instance is not fitted yet: call fit first")
    x = check_cells(X, self.n_components)
    if x.shape[1] != self.n_features_in_:
      raise ValueError(f"X has {x.shape[1]} features, the mixture was fitted on {self.n_features_in_}")
    from sisua_amd.engine import k_gmm_full_predict
    return k_gmm_full_predict(x, self.weights_, self.means_, np.swapaxes(self.precisions_cholesky_, 1, 2), **want)

  def predict(self, X) -> np.ndarray:
    return self._e_step(X)["labels"].astype(np.int64)

  def predict_proba(self, X) -> np.ndarray:
    return self._e_step(X, resp=True)["resp"]

  def score_samples(self, X) -> np.ndarray:
    return self._e_step(X, score=True)["score"]

  def score(self, X, y=None) -> float:
    return float(np.mean(self.score_samples(X)))

  def _n_parameters(self) -> int:
    d = self.n_features_in_
    return int(self.n_components * d * (d + 1) // 2 + d * self.n_components + self.n_components - 1)

  def bic(self, X) -> float:
    n = np.asarray(X).shape[0]
    return float(-2.0 * self.score(X) * n + self._n_parameters() * np.log(n))

  def aic(self, X) -> float:
    return float(-2.0 * self.score(X) * np.asarray(X).shape[0] + 2.0 * self._n_parameters())
