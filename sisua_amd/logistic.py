"""scikit-learn's LogisticRegression as far as the reference leans on it (scanpy's rank_genes_groups(method='logreg') under
SingleCellOMIC.rank_vars_groups): the L2-penalised fit, multinomial for three and more classes and the one-logit binary form for two,
solved on the device by a deterministic full-batch L-BFGS (smx_logreg.hip through `engine.k_logreg_*`).  The
penalised objective is strictly convex in the coefficients, so the fit is defined by its optimum, not by a solver's path: with a small
`tol` the coefficients agree with scikit-learn's converged solvers to their own disagreement.
Not built: the L1 and elastic-net penalties, no penalty, class and sample weights, one-vs-rest fits, stochastic solvers."""
import warnings

import numpy as np

from sisua_amd import engine

BUILT = ("LogisticRegression here is built for penalty='l2', solver=None or 'lbfgs', class_weight=None and no sample_weight: "
         "C, fit_intercept, tol, max_iter and warm_start are its settings")


class LogisticRegression:
  """LogisticRegression(C=1.0, fit_intercept=True, tol=1e-4, max_iter=100, warm_start=False).  tol bounds max|gradient| of the mean-form
  objective (1/N) sum_i loss_i + ||W||^2 / (2 C N).  X is dense or scipy.sparse (never densified on the host) and is taken as float32.
  After `fit`: classes_ (sorted), coef_ [K, G] float64 ([1, G] for two classes), intercept_ [K] ([1]), n_iter_ [1] int32.  A fit that
  ends above tol raises a RuntimeWarning that gives the final max|g|, never an exception."""

  def __init__(self, C=1.0, fit_intercept=True, tol=1e-4, max_iter=100, warm_start=False, penalty="l2", solver=None, class_weight=None,
               **other):
    if other:
      raise ValueError(f"{BUILT}; got {sorted(other)}")
    if penalty != "l2" or solver not in (None, "lbfgs") or class_weight is not None:
      raise ValueError(f"{BUILT}; got penalty={penalty!r}, solver={solver!r}, class_weight={class_weight!r}")
    if not (np.isfinite(float(C)) and float(C) > 0):
      raise ValueError(f"C must be finite and > 0, got {C}")
    if not (np.isfinite(float(tol)) and float(tol) > 0):
      raise ValueError(f"tol must be finite and > 0, got {tol}")
    if int(max_iter) < 1:
      raise ValueError(f"max_iter must be >= 1, got {max_iter}")
    self.C, self.fit_intercept, self.tol, self.max_iter, self.warm_start = float(C), bool(fit_intercept), float(tol), int(max_iter), bool(warm_start)
    self.penalty, self.solver, self.class_weight = penalty, solver, class_weight

  @staticmethod
  def _check(X):
    if getattr(X, "ndim", 0) != 2 or X.shape[0] < 1 or X.shape[1] < 1:
      raise ValueError(f"X must be a matrix [rows >= 1, features >= 1], got shape {getattr(X, 'shape', None)}")
    return X

  def fit(self, X, y, sample_weight=None):
    if sample_weight is not None:
      raise ValueError(f"{BUILT}; got sample_weight")
    X = self._check(X)
    y = np.asarray(y)
    if y.shape != (X.shape[0],):
      raise ValueError(f"y must be [{X.shape[0]}], got {y.shape}")
    classes, codes = np.unique(y, return_inverse=True)
    K = len(classes)
    if K < 2:
      raise ValueError(f"a fit needs at least 2 classes, y holds {K}: {classes[:1].tolist()}")
    W0 = b0 = None
    if self.warm_start and getattr(self, "coef_", None) is not None and self.coef_.shape == ((1 if K == 2 else K), X.shape[1]):
      W0, b0 = self.coef_, self.intercept_
    r = engine.k_logreg_fit(X, codes.reshape(-1).astype(np.int32), K, self.C, self.fit_intercept, self.tol, self.max_iter, W0, b0)
    self.classes_, self.coef_, self.intercept_ = classes, r["W"], r["b"]
    self.n_iter_, self.n_eval_, self.objective_, self.max_grad_ = np.array([r["n_iter"]], np.int32), int(r["n_eval"]), float(r["F"]), float(r["gmax"])
    self.n_features_in_ = X.shape[1]
    if not r["converged"]:
      warnings.warn(f"LogisticRegression stopped after {r['n_iter']} iterations ({r['n_eval']} evaluations) with max|g| = {r['gmax']:.3e} "
                    f"> tol = {self.tol:g}: raise max_iter", RuntimeWarning, stacklevel=2)
    return self

  def _fitted(self, X):
    if getattr(self, "coef_", None) is None:
      raise ValueError("this LogisticRegression is not fitted yet: call fit first")
    X = self._check(X)
    if X.shape[1] != self.coef_.shape[1]:
      raise ValueError(f"X has {X.shape[1]} features, the fit had {self.coef_.shape[1]}")
    return X

  def decision_function(self, X):
    """the logits [N, K] float64, or [N] for two classes (positive: classes_[1])"""
    return engine.k_logreg_decision(self._fitted(X), self.coef_, self.intercept_, len(self.classes_))

  def predict(self, X):
    z = self.decision_function(X)
    return self.classes_[(z > 0).astype(np.int64) if z.ndim == 1 else np.argmax(z, axis=1)]

  def predict_log_proba(self, X):
    z = self.decision_function(X)
    if z.ndim == 1:
      z = np.stack([np.zeros_like(z), z], axis=1)   # (the implicit zero logit of classes_[0])
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))

  def predict_proba(self, X):
    return np.exp(self.predict_log_proba(X))

  def score(self, X, y, sample_weight=None):
    if sample_weight is not None:
      raise ValueError(f"{BUILT}; got sample_weight")
    return float(np.mean(self.predict(X) == np.asarray(y)))
