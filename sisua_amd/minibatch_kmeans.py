"""scikit-learn's MiniBatchKMeans as far as the reference's SingleCellOMIC.clustering uses it: `partial_fit` per batch of rows, then
`predict`.  The distance sweeps -- the k-means++ seeding of the first batch, every mini-batch step, the assignment of every row -- run on
the device (smx_mbkmeans.hip through `engine.k_mbkmeans_*`), in float64 and the direct form of the squared distance; the host draws from
`np.random.RandomState` exactly what scikit-learn 1.7 draws, in its order, and reassigns starved centres as `_mini_batch_step` does.  With
the same data, batches and seed the counts equal scikit-learn's and the centres agree to rounding.
Not built: `fit` (its sampled loop with early stopping), sample weights, a callable init."""
import numbers

import numpy as np

from sisua_amd import engine
from sisua_amd.data import is_sparse


def _rows(X, rows):
  """the rows of a dense or CSR block as float64 [len(rows), G]"""
  r = X[rows]
  return np.asarray(r.toarray() if is_sparse(r) else r, dtype=np.float64)


class MiniBatchKMeans:
  """MiniBatchKMeans(n_clusters=8, init='k-means++', max_iter=100, batch_size=1024, compute_labels=True, random_state=None,
  n_init='auto', reassignment_ratio=0.01).  init: 'k-means++', 'random' or an [n_clusters, n_features] array.  max_iter and n_init are
  accepted and unused: `partial_fit` never reads them in scikit-learn either.  X is dense or scipy.sparse and is taken as float32.
  After `partial_fit`: cluster_centers_ [n_clusters, n_features] float64, counts_ [n_clusters], n_steps_, and with compute_labels
  labels_ and inertia_ of the last batch against the updated centres."""

  def __init__(self, n_clusters=8, init="k-means++", max_iter=100, batch_size=1024, compute_labels=True, random_state=None, n_init="auto",
               reassignment_ratio=0.01, **other):
    if other:
      raise ValueError(f"MiniBatchKMeans here takes none of {sorted(other)}: only what partial_fit and predict read is built")
    if not isinstance(n_clusters, numbers.Integral) or not 2 <= int(n_clusters) <= engine.MBK_MAX_CLUSTERS:
      raise ValueError(f"n_clusters must be an integer in 2 .. {engine.MBK_MAX_CLUSTERS}, got {n_clusters!r}")
    if not isinstance(batch_size, numbers.Integral) or int(batch_size) < 1:
      raise ValueError(f"batch_size must be an integer >= 1, got {batch_size!r}")
    if isinstance(init, str):
      if init not in ("k-means++", "random"):
        raise ValueError(f"init must be 'k-means++', 'random' or an [n_clusters, n_features] array, got {init!r}")
    else:
      init = np.array(init, dtype=np.float64)
      if init.ndim != 2 or init.shape[0] != int(n_clusters) or not np.isfinite(init).all():
        raise ValueError(f"an init array must be [{int(n_clusters)}, n_features] and finite, got shape {init.shape}")
    if not float(reassignment_ratio) >= 0:
      raise ValueError(f"reassignment_ratio should be >= 0, got {reassignment_ratio}")
    self.n_clusters, self.init, self.max_iter, self.batch_size = int(n_clusters), init, max_iter, int(batch_size)
    self.compute_labels, self.random_state, self.n_init, self.reassignment_ratio = bool(compute_labels), random_state, n_init, float(reassignment_ratio)

  def fit(self, X, y=None, sample_weight=None):
    raise NotImplementedError("MiniBatchKMeans.fit (the sampled loop with early stopping) is not built: call partial_fit per batch of rows, "
                              "as the reference's SingleCellOMIC.clustering does")

  @staticmethod
  def _check(X, n_features=None):
    if getattr(X, "ndim", 0) != 2 or X.shape[0] < 1 or X.shape[1] < 1:
      raise ValueError(f"X must be a matrix [rows >= 1, features >= 1], got shape {getattr(X, 'shape', None)}")
    if n_features is not None and X.shape[1] != n_features:
      raise ValueError(f"X has {X.shape[1]} features, the centres have {n_features}")
    return X

  def _seed(self, X):
    """the first call's centres, consuming the stream as _init_centroids and _kmeans_plusplus do"""
    n, K, rng = X.shape[0], self.n_clusters, self._rng
    init_size = 3 * self._batch_size
    if init_size < K:
      init_size = 3 * K
    if init_size < n:
      X = X[rng.randint(0, n, init_size)]
      n = init_size
    if isinstance(self.init, str) and self.init == "k-means++":
      first = rng.choice(n, p=np.ones(n) / n)
      u = rng.uniform(size=(K - 1, 2 + int(np.log(K))))
      return engine.k_mbkmeans_seed(X, K, first, u)["centres"]
    if isinstance(self.init, str):
      return _rows(X, rng.choice(n, size=K, replace=False, p=np.ones(n) / n))
    return self.init.copy()

  def partial_fit(self, X, y=None, sample_weight=None):
    if sample_weight is not None:
      raise ValueError("sample_weight is not built")
    first_call = not hasattr(self, "cluster_centers_")
    X = self._check(np.asarray(X) if not is_sparse(X) and not isinstance(X, np.ndarray) else X, None if first_call else self.cluster_centers_.shape[1])
    n, K = X.shape[0], self.n_clusters
    if first_call:
      if n < K:
        raise ValueError(f"n_samples={n} should be >= n_clusters={K}.")
      if not isinstance(self.init, str) and self.init.shape[1] != X.shape[1]:
        raise ValueError(f"the init array has {self.init.shape[1]} features, X has {X.shape[1]}")
      self._rng = np.random.RandomState(self.random_state)
      self._batch_size = min(self.batch_size, n)
      centres = self._seed(X)
      self.cluster_centers_, self.counts_, self._n_since_last_reassign, self.n_steps_ = centres, np.zeros(K), 0, 0
    self._n_since_last_reassign += self._batch_size
    reassign = bool((self.counts_ == 0).any() or self._n_since_last_reassign >= 10 * K)
    if reassign:
      self._n_since_last_reassign = 0
    r = engine.k_mbkmeans_step(X, self.cluster_centers_, self.counts_, want_labels=False)
    centres, counts = r["centres"], r["counts"]
    if reassign and self.reassignment_ratio > 0:
      to = counts < self.reassignment_ratio * counts.max()
      if to.sum() > 0.5 * n:   # (at most half the block's rows become centres)
        to[np.argsort(counts)[int(0.5 * n):]] = False
      if to.sum():
        centres[to] = _rows(X, self._rng.choice(n, replace=False, size=int(to.sum())))
      counts[to] = np.min(counts[~to])   # (on every reassigning step, as scikit-learn does)
    self.cluster_centers_, self.counts_ = centres, counts
    if self.compute_labels:
      self.labels_, d = engine.k_mbkmeans_predict(X, centres, want_distance=True)
      self.inertia_ = float(d.sum())
    self.n_steps_ += 1
    return self

  def predict(self, X):
    if not hasattr(self, "cluster_centers_"):
      raise ValueError("this MiniBatchKMeans has no centres yet: call partial_fit first")
    X = self._check(np.asarray(X) if not is_sparse(X) and not isinstance(X, np.ndarray) else X, self.cluster_centers_.shape[1])
    return engine.k_mbkmeans_predict(X, self.cluster_centers_)
