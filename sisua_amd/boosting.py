"""scikit-learn's GradientBoostingClassifier as far as the reference leans on it (odin's `representative_importance_matrix` under
SingleCellOMIC.get_importance_matrix, Posterior.cal_importance and Posterior.cal_dci): log-loss boosting of depth-limited regression trees
with the friedman_mse criterion, prior init and Newton leaf values, fitted on the device over a one-byte histogram of the matrix
(smx_gbt.hip through `engine.k_gbt_*`; tests/gbt_ref.py restates it in NumPy).

It deviates from scikit-learn in four stated ways, which make a fit ONE answer, independent of the order of any sum: columns with more than
256 distinct values are cut at the 256-quantile positions (the histogram approximation; narrower columns keep every distinct value and so
scikit-learn's candidate partitions); residuals and curvatures are quantised to 2^-40; ties between candidates go to the lowest feature,
then the lowest bin, and a split needs an improvement > 0 (scikit-learn breaks ties by its seeded feature order and takes
zero-improvement splits); the holdout rows of early stopping are chosen per class by this build's own rule.  A threshold is the midpoint of
the two neighbouring values of the WHOLE column, where scikit-learn takes the neighbours among the node's own cells: the training cells are
cut apart identically, a new row between the two may go the other way.
Not built: random forests, regression, subsample < 1, max_features, sample weights, more than 256 bins, exact (non-histogram) splits of
wide-valued columns, loss='exponential', warm_start, ccp_alpha, max_leaf_nodes."""
import warnings

import numpy as np

from sisua_amd import engine

BUILT = ("GradientBoostingClassifier here is built for loss='log_loss', criterion='friedman_mse', subsample=1.0, max_features=None, "
         "init=None, no sample_weight, warm_start=False, ccp_alpha=0 and max_leaf_nodes=None: n_estimators, learning_rate, max_depth, "
         "min_samples_split, min_samples_leaf, n_iter_no_change, validation_fraction, tol and random_state are its settings")
_TREE_ARRAYS = ("feature", "threshold", "left", "right", "value", "n", "improvement")


class Tree:
  """One regression tree of a fit, read-only: arrays [M] in heap order (the children of slot t are 2 t + 1 and 2 t + 2) -- feature (-1: a
  leaf, or a slot no cell reached), threshold, children_left / children_right (-1 on a leaf), value, n_node_samples (0: unreached),
  improvement (residual units); node_count: the slots that cells reached."""

  def __init__(self, arrays):
    for name, a in arrays.items():
      a = a.copy()
      a.setflags(write=False)
      object.__setattr__(self, {"left": "children_left", "right": "children_right", "n": "n_node_samples"}.get(name, name), a)
    object.__setattr__(self, "node_count", int((self.n_node_samples > 0).sum()))

  def __setattr__(self, name, value):
    raise AttributeError("a fitted tree is read-only")


def feature_importances(trees, n_features):
  """scikit-learn's rule over the tree arrays [.., M]: per tree with more than one node the improvements per feature over the root's n, the
  mean over those trees, normalised to sum 1 (zeros if no tree split)"""
  f, imp, n = (np.asarray(trees[a]).reshape(-1, np.asarray(trees[a]).shape[-1]) for a in ("feature", "improvement", "n"))
  rows = []
  for t in range(f.shape[0]):
    if f[t, 0] < 0:
      continue
    split = f[t] >= 0
    rows.append(np.bincount(f[t][split], weights=imp[t][split], minlength=n_features) / n[t, 0])
  if not rows:
    return np.zeros(n_features)
  avg = np.mean(rows, axis=0)
  return avg / avg.sum() if avg.sum() > 0 else np.zeros(n_features)


def holdout_rows(codes, n_classes, validation_fraction, random_state):
  """The rows early stopping holds out -> (training rows, validation rows), both rising.  Per class, in class order, the last
  ceil(validation_fraction * n_c) rows of a permutation of the class's rows, all drawn from one RandomState(random_state); at least one row
  of every class stays in training.  (scikit-learn draws a stratified train_test_split: a stated deviation.)"""
  rs = np.random.RandomState(random_state)
  held = []
  for c in range(n_classes):
    rows = rs.permutation(np.flatnonzero(codes == c))
    n_hold = min(int(np.ceil(validation_fraction * rows.size)), rows.size - 1)
    held.append(rows[rows.size - n_hold:])
  val = np.sort(np.concatenate(held)).astype(np.int64)
  return np.setdiff1d(np.arange(len(codes), dtype=np.int64), val), val


def quantile_codes(column, n_bins=10):
  """One column cut into quantile bins, int64 codes: the ordinal `KBinsDiscretizer(n_bins, encode='ordinal', strategy='quantile')` of
  scikit-learn restated -- edges at the linearly interpolated percentiles 0, 100 / n_bins, .., 100; an edge closer than 1e-8 to the one
  before it is dropped; code = the number of inner edges <= x."""
  x = np.asarray(column, np.float64).reshape(-1)
  edges = np.percentile(x, np.linspace(0, 100, int(n_bins) + 1))
  keep = np.ones(len(edges), bool)
  keep[1:] = np.ediff1d(edges) > 1e-8
  edges = edges[keep]
  return np.searchsorted(edges[1:-1], x, side="right").astype(np.int64)


class GradientBoostingClassifier:
  """GradientBoostingClassifier(n_estimators=100, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1,
  n_iter_no_change=None, validation_fraction=0.1, tol=1e-4, random_state=None).  X is dense or scipy.sparse (never densified on the host)
  and is taken as float32.  After `fit`: classes_ (sorted), n_classes_, n_estimators_, train_score_ [n_estimators_], feature_importances_
  [G], estimators_ [n_estimators_, Kz] of `Tree` (Kz = 1 for two classes, the class-1 logit; n_classes_ otherwise).  random_state only
  chooses the holdout rows of early stopping: the trees themselves have no random part."""

  def __init__(self, n_estimators=100, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1, n_iter_no_change=None,
               validation_fraction=0.1, tol=1e-4, random_state=None, loss="log_loss", criterion="friedman_mse", subsample=1.0,
               max_features=None, init=None, warm_start=False, ccp_alpha=0.0, max_leaf_nodes=None, **other):
    if other:
      raise ValueError(f"{BUILT}; got {sorted(other)}")
    if (loss != "log_loss" or criterion != "friedman_mse" or float(subsample) != 1.0 or max_features is not None or init is not None or warm_start
        or float(ccp_alpha) != 0.0 or max_leaf_nodes is not None):
      raise ValueError(f"{BUILT}; got loss={loss!r}, criterion={criterion!r}, subsample={subsample!r}, max_features={max_features!r}, "
                       f"init={init!r}, warm_start={warm_start!r}, ccp_alpha={ccp_alpha!r}, max_leaf_nodes={max_leaf_nodes!r}")
    if int(n_estimators) < 1:
      raise ValueError(f"n_estimators must be >= 1, got {n_estimators}")
    if not (np.isfinite(float(learning_rate)) and float(learning_rate) > 0):
      raise ValueError(f"learning_rate must be finite and > 0, got {learning_rate}")
    engine._gbt_tree_params(max_depth, min_samples_split, min_samples_leaf, 0)
    if n_iter_no_change is not None and int(n_iter_no_change) < 1:
      raise ValueError(f"n_iter_no_change must be None or >= 1, got {n_iter_no_change}")
    if not 0.0 < float(validation_fraction) < 1.0:
      raise ValueError(f"validation_fraction must lie in (0, 1), got {validation_fraction}")
    if not np.isfinite(float(tol)):
      raise ValueError(f"tol must be finite, got {tol}")
    self.n_estimators, self.learning_rate, self.max_depth = int(n_estimators), float(learning_rate), int(max_depth)
    self.min_samples_split, self.min_samples_leaf = int(min_samples_split), int(min_samples_leaf)
    self.n_iter_no_change = None if n_iter_no_change is None else int(n_iter_no_change)
    self.validation_fraction, self.tol, self.random_state = float(validation_fraction), float(tol), random_state

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
    codes, K = codes.reshape(-1).astype(np.int32), len(classes)
    if K < 2:
      raise ValueError(f"a fit needs at least 2 classes, y holds {K}: {classes[:1].tolist()}")
    kw = dict(n_estimators=self.n_estimators, learning_rate=self.learning_rate, max_depth=self.max_depth,
              min_samples_split=self.min_samples_split, min_samples_leaf=self.min_samples_leaf)
    if self.n_iter_no_change is None:
      r = engine.k_gbt_fit(X, codes, K, **kw)
    else:
      if K > engine.GBT_MAX_CLASSES:
        raise ValueError(f"gradient boosting takes 2 .. {engine.GBT_MAX_CLASSES} classes, got {K}")
      if engine._sparse(X):
        X = X.tocsr()   # (rows are taken by index)
      train, val = holdout_rows(codes, K, self.validation_fraction, self.random_state)
      if val.size == 0:
        raise ValueError("early stopping found no row to hold out: every class has a single row")
      r = engine.k_gbt_fit(X[train], codes[train], K, x_val=X[val], labels_val=codes[val], n_iter_no_change=self.n_iter_no_change,
                           tol=self.tol, **kw)
      self.validation_score_ = r["val_score"]
    self._trees = {a: r[a] for a in _TREE_ARRAYS}
    self._init = r["init"]
    self.classes_, self.n_classes_, self.n_features_in_ = classes, K, X.shape[1]
    self.n_estimators_, self.train_score_ = int(r["n_estimators_"]), r["train_score_"]
    self.feature_importances_ = feature_importances(self._trees, X.shape[1])
    self.estimators_ = np.empty(r["feature"].shape[:2], dtype=object)
    for s in range(self.estimators_.shape[0]):
      for k in range(self.estimators_.shape[1]):
        self.estimators_[s, k] = Tree({a: r[a][s, k] for a in _TREE_ARRAYS})
    return self

  def _fitted(self, X):
    if getattr(self, "_trees", None) is None:
      raise ValueError("this GradientBoostingClassifier is not fitted yet: call fit first")
    X = self._check(X)
    if X.shape[1] != self.n_features_in_:
      raise ValueError(f"X has {X.shape[1]} features, the fit had {self.n_features_in_}")
    return X

  def _squeeze(self, raw):
    return raw[:, 0] if self.n_classes_ == 2 else raw

  def decision_function(self, X):
    """the raw scores [N, K] float64, or [N] for two classes (positive: classes_[1])"""
    return self._squeeze(engine.k_gbt_decision(self._fitted(X), self._trees, self._init, self.learning_rate))

  def staged_decision_function(self, X):
    """the raw scores after each stage (one pass of the trees per stage)"""
    X = self._fitted(X)
    for s in range(1, self.n_estimators_ + 1):
      yield self._squeeze(engine.k_gbt_decision(X, self._trees, self._init, self.learning_rate, n_stages=s))

  def predict_proba(self, X):
    z = self.decision_function(X)
    if z.ndim == 1:
      p = 1.0 / (1.0 + np.exp(-z))
      return np.stack([1.0 - p, p], axis=1)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)

  def predict(self, X):
    z = self.decision_function(X)
    return self.classes_[(z > 0).astype(np.int64) if z.ndim == 1 else np.argmax(z, axis=1)]

  def score(self, X, y, sample_weight=None):
    if sample_weight is not None:
      raise ValueError(f"{BUILT}; got sample_weight")
    return float(np.mean(self.predict(X) == np.asarray(y)))


def importance_matrix(repr_train, factor_train, repr_test, factor_test, random_state=1234, n_iter_no_change=100, **gbt_kw):
  """odin's `representative_importance_matrix`: one GradientBoostingClassifier per factor (a column of discrete factor values) on the
  representations; column f of the matrix is abs(feature_importances_) of factor f's fit ->
  (matrix [n_repr, n_factors] float64, train_acc [n_factors], test_acc [n_factors]).

  [3P-recall] odin is not available to this build; from recall it constructs `GradientBoostingClassifier(random_state=random_state,
  n_iter_no_change=100)` and everything else at scikit-learn's defaults.  That default is kept here, and what follows from it: 10 % of the
  training rows are held out of every fit (validation_fraction=0.1), and with n_estimators=100 there is effectively no early stop -- a fit
  ends early only if no stage at all improves on the ones before.  Pass n_iter_no_change=None to fit on all training rows.

  A factor whose training rows hold a single class cannot be fitted: its column is zero, its accuracies NaN, and a RuntimeWarning says so."""
  ft, fe = np.asarray(factor_train), np.asarray(factor_test)
  if ft.ndim != 2 or fe.ndim != 2 or ft.shape[1] != fe.shape[1]:
    raise ValueError(f"the factors must be [rows, n_factors] with the same n_factors, got {ft.shape} and {fe.shape}")
  if repr_train.shape[0] != ft.shape[0] or repr_test.shape[0] != fe.shape[0] or repr_train.shape[1] != repr_test.shape[1]:
    raise ValueError(f"representations {repr_train.shape} / {repr_test.shape} do not match the factors {ft.shape} / {fe.shape}")
  n_repr, n_factors = repr_train.shape[1], ft.shape[1]
  matrix, train_acc, test_acc = np.zeros((n_repr, n_factors)), np.full(n_factors, np.nan), np.full(n_factors, np.nan)
  for f in range(n_factors):
    if len(np.unique(ft[:, f])) < 2:
      warnings.warn(f"factor {f} holds a single class in the training rows: its importance column is zero", RuntimeWarning, stacklevel=2)
      continue
    model = GradientBoostingClassifier(random_state=random_state, n_iter_no_change=n_iter_no_change, **gbt_kw).fit(repr_train, ft[:, f])
    matrix[:, f] = np.abs(model.feature_importances_)
    train_acc[f], test_acc[f] = model.score(repr_train, ft[:, f]), model.score(repr_test, fe[:, f])
  return matrix, train_acc, test_acc
