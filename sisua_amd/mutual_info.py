"""Gene x protein mutual-information matrices (the reference's third association score beside Pearson and Spearman:
`SingleCellOMIC.get_mutual_information`, data/_single_cell_analysis.py:1148-1196; `Posterior.get_correlation_matrix(corr_type='mi')`,
analysis/posterior.py:896-912): scikit-learn's `mutual_info_regression` / `mutual_info_classif`, one call per protein with the same
seed, as one matrix.  The preparation of `_estimate_mi` -- a continuous column divided by its standard deviation, then 1e-10 max(1,
mean|x|) noise from `RandomState(random_state)` in scikit-learn's order of draws -- is NumPy, per chunk of genes; the three estimators
(Kraskov's for two continuous columns, Ross's for a continuous and a discrete one, the contingency table for two discrete ones) run on
the device (smx_mi.hip; definitions in include/sisua_hip.h, restated in tests/mutual_info_ref.py).

Two deviations from scikit-learn, both stated there: distances are exact also in label groups of 2 .. 2k + 1 cells, and a pair in which
no cell is kept (every label unique) scores 0.0 where scikit-learn raises."""
from __future__ import annotations

import numpy as np

from sisua_amd.engine import MI_MAX_CELLS, MI_MAX_NEIGHBORS   # noqa: F401

_NOISE_ROWS = 1 << 22          # normals drawn at a time
_HOST_CHUNK_BYTES = 64 << 20   # prepared gene columns on the host at a time
_NOISE_KEEP_BYTES = 256 << 20  # the whole [cells, continuous genes] noise is kept when it is no larger


def _engine():
  from sisua_amd import engine
  return engine


def is_discrete(column) -> bool:
  """This build's rule for discrete_features / discrete_targets = 'auto' (the reference's `odin.stats.is_discrete` is not part of its
  tree): a column is discrete when every value is an integer."""
  v = np.asarray(column)
  if v.dtype.kind in "biu":
    return True
  v = v.astype(np.float64, copy=False)
  return bool(np.isfinite(v).all() and (v == np.floor(v)).all())


def _dense(a):
  return np.asarray(a.toarray() if hasattr(a, "toarray") else a)


def _mask(spec, cols, n, what):
  """'auto', a bool, or a boolean array [n] -> bool [n]; cols(j) gives column j"""
  if isinstance(spec, str):
    if spec != "auto":
      raise ValueError(f"{what} must be 'auto', a bool or a boolean array, got {spec!r}")
    return np.array([is_discrete(cols(j)) for j in range(n)], bool)
  if isinstance(spec, (bool, np.bool_)):
    return np.full(n, bool(spec))
  m = np.asarray(spec)
  if m.dtype != bool or m.shape != (n,):
    raise ValueError(f"{what} must be 'auto', a bool or a boolean array [{n}], got {m.dtype} {m.shape}")
  return m.copy()


class _FeatureNoise:
  """The standard_normal((N, n_cont)) block of _estimate_mi, row-major from RandomState(seed), by columns; `target()` is the
  standard_normal(N) that follows it in the stream."""

  def __init__(self, seed, N, n_cont):
    self.seed, self.N, self.n = seed, int(N), int(n_cont)
    self._all = self._target = None
    self._keep = 0 < self.N * self.n * 8 <= _NOISE_KEEP_BYTES

  def _walk(self, c0, c1):
    """the columns c0 .. c1 - 1 of the block, drawn in row blocks, and the generator after the whole block"""
    rng = np.random.RandomState(self.seed)
    out = np.empty((self.N, c1 - c0))
    rows = max(1, _NOISE_ROWS // max(self.n, 1))
    for r0 in range(0, self.N if self.n else 0, rows):
      r1 = min(self.N, r0 + rows)
      out[r0:r1] = rng.standard_normal(size=(r1 - r0, self.n))[:, c0:c1]
    return out, rng

  def columns(self, c0, c1):
    """[N, c1 - c0]: the noise of the continuous features c0 .. c1 - 1 (counted among the continuous ones)"""
    if not self._keep:
      return self._walk(c0, c1)[0]
    if self._all is None:
      self._all, rng = self._walk(0, self.n)
      self._target = rng.standard_normal(size=self.N)
    return self._all[:, c0:c1]

  def target(self):
    if self._target is None and self._keep:
      self.columns(0, 0)   # (one walk of the stream leaves both)
    if self._target is None:
      self._target = self._walk(0, 0)[1].standard_normal(size=self.N)
    return self._target


def prepare_targets(Y, discrete, noise_z, noise=True):
  """Y [N, P] -> protein-major prepared columns [P, N] float64: a continuous target scaled and noised as scale(y) of ONE target is
  (every protein is its own scikit-learn call with the same seed: the same noise vector)"""
  Y = np.asarray(Y, np.float64)
  out = np.empty((Y.shape[1], Y.shape[0]))
  for p in range(Y.shape[1]):
    y = np.ascontiguousarray(Y[:, p])
    if not discrete[p]:
      s = np.nanstd(y)
      y = y / (1.0 if s < 10 * np.finfo(np.float64).eps else s)
      if noise:
        y = y + 1e-10 * np.maximum(1, np.mean(np.abs(y))) * noise_z()
    out[p] = y
  return out


def mutual_information(X, Y, discrete_features="auto", discrete_targets="auto", n_neighbors=3, random_state=1, genes=None, noise=True,
                       gene_chunk=0):
  """The mutual information [G, P] float64 (nats, clipped at 0) between every column of X [N, G] (dense or scipy.sparse; sparse is taken
  per chunk of genes and never densified whole) and every column of Y [N, P]: column p is scikit-learn's
  `mutual_info_classif` (a discrete target) or `mutual_info_regression(X, Y[:, p], discrete_features=mask, n_neighbors=n_neighbors,
  random_state=random_state)`.  discrete_features / discrete_targets: 'auto' (`is_discrete`: every value an integer), a bool, or a boolean
  array.  genes: a list of gene indices (any order, repeats allowed): the result is that of X[:, genes].  noise=False leaves the 1e-10
  noise out: a pure function of the data.  gene_chunk: genes on the device at a time (0: the library's choice); no bit depends on it."""
  eng = _engine()
  if getattr(X, "ndim", 0) != 2 or getattr(Y, "ndim", 0) != 2 or X.shape[0] != Y.shape[0] or X.shape[1] < 1 or Y.shape[1] < 1:
    raise ValueError(f"X must be [cells, genes] and Y [cells, proteins], got {getattr(X, 'shape', None)} and {getattr(Y, 'shape', None)}")
  N = X.shape[0]
  k = eng._mi_check(N, n_neighbors)
  sparse = hasattr(X, "tocsc")
  if sparse:
    X = X.tocsc()
  sel = np.arange(X.shape[1]) if genes is None else np.asarray(genes, np.int64).ravel()
  if sel.size < 1 or sel.min() < 0 or sel.max() >= X.shape[1]:
    raise IndexError(f"genes must name columns 0 .. {X.shape[1] - 1}")
  G = sel.size
  take = lambda idx: np.asarray(_dense(X[:, idx]), np.float64).reshape(N, -1)
  Yd = np.asarray(_dense(Y), np.float64)
  if not np.isfinite(Yd).all():
    raise ValueError(f"protein column {int(np.flatnonzero(~np.isfinite(Yd).all(axis=0))[0])} holds a value that is not finite")
  hostc = max(1, min(G, _HOST_CHUNK_BYTES // (8 * N)))
  if isinstance(discrete_features, str) and discrete_features == "auto":
    xd = np.concatenate([[is_discrete(c) for c in take(sel[g0:g0 + hostc]).T] for g0 in range(0, G, hostc)]).astype(bool)
  else:
    xd = _mask(discrete_features, None, X.shape[1], "discrete_features")[sel]   # (the mask names X's columns)
  yd = _mask(discrete_targets, lambda j: Yd[:, j], Yd.shape[1], "discrete_targets")
  n_cont = int((~xd).sum())
  z = _FeatureNoise(random_state, N, n_cont)
  ycols = prepare_targets(Yd, yd, z.target, noise)
  cont_rank = np.cumsum(~xd) - 1   # a continuous gene's column in the noise block
  out = np.empty((G, Yd.shape[1]))
  for g0 in range(0, G, hostc):
    g1 = min(G, g0 + hostc)
    block = take(sel[g0:g1])
    bad = np.flatnonzero(~np.isfinite(block).all(axis=0))
    if bad.size:
      raise ValueError(f"gene column {g0 + int(bad[0])} holds a value that is not finite")
    cols = np.ascontiguousarray(block.T)   # gene-major [genes, N]: a gene's cells are contiguous, as a column of scikit-learn's block is
    cont = np.flatnonzero(~xd[g0:g1])
    if cont.size:
      c = cols[cont]
      sd = np.nanstd(c, axis=1)
      sd[sd < 10 * np.finfo(np.float64).eps] = 1.0
      c /= sd[:, None]
      if noise:
        means = np.maximum(1, np.mean(np.abs(c), axis=1))
        c0, c1 = int(cont_rank[g0 + cont[0]]), int(cont_rank[g0 + cont[-1]]) + 1
        c += ((1e-10 * means)[None, :] * z.columns(c0, c1)).T
      cols[cont] = c
    out[g0:g1] = eng.mutual_info(cols, xd[g0:g1], ycols, yd, k, gene_chunk)
  return out
