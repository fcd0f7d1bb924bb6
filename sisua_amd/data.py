"""Host-side data semantics of the training path (NumPy; runs once per fit, not
per step): the pieces of the reference's data layer that decide WHICH cells and
WHICH values reach the step.

  split_indices      SingleCellOMIC.split            sisua/data/single_cell_dataset.py:43-81
  corrupt            apply_artificial_corruption     sisua/data/utils.py:168-228 (via _single_cell_analysis.py:78-111)
  library_size       get_library_size                sisua/data/utils.py:231-263
  label_mask / epoch_order / iter_batches
                     _OMICbase.create_dataset        sisua/data/_single_cell_base.py:539-602
  synthetic_*        shape/sparsity-matched stand-ins for the datasets of
                     description/dataset.html (the real ones need S3 downloads)

Bit-exactness of the first three against the reference's own code is pinned by
tests/golden/reference_data_fixtures.npz.

Sparse counts: every function here also takes a scipy.sparse matrix, held as canonical float32 CSR (`as_csr`: sorted
column indices, duplicates summed, explicit zeros dropped) and never densified whole.  `corrupt` and `library_size` give
the dense twin's bits (for library_size: integer counts with row sums below 2**24, which float32 holds exactly).
"""
from __future__ import annotations

import numbers
from typing import List, Optional, Sequence, Tuple

import ctypes as _C

import numpy as np
import scipy.sparse as sp


def is_sparse(x) -> bool:
  return sp.issparse(x)


def as_csr(x, copy: bool = True) -> sp.csr_matrix:
  """Any scipy.sparse matrix (COO, CSC, CSR, any dtype) -> canonical float32 CSR: indices sorted within a row, duplicates
  summed (in the input's dtype, as its toarray() would), explicit zeros dropped.  copy=False returns `x` itself when it is
  canonical float32 CSR already."""
  if (not copy and isinstance(x, sp.csr_matrix) and x.dtype == np.float32 and x.has_canonical_format
      and not (x.data == 0).any()):
    return x
  x = sp.csr_matrix(x, copy=True)
  x.sum_duplicates()   # (sorts the indices too)
  x = x.astype(np.float32, copy=False)
  x.eliminate_zeros()
  x.sort_indices()
  return x


def row_sums(x) -> np.ndarray:
  """float32 row sums: dense `x.sum(axis=1)`; CSR from its non-zeros (fp64 accumulation, exact -- and so equal to the dense
  float32 sum -- for integer counts with row sums below 2**24)."""
  if not is_sparse(x):
    return x.sum(axis=1)
  x = as_csr(x, copy=False)
  rows = np.repeat(np.arange(x.shape[0]), np.diff(x.indptr))
  return np.bincount(rows, weights=x.data, minlength=x.shape[0]).astype(np.float32)


def split_indices(n_obs: int, train_percent: float = 0.8, seed: int = 1) -> Tuple[np.ndarray, np.ndarray]:
  train_percent = np.clip(train_percent, 0.0, 1.0)
  ids = np.random.RandomState(seed=seed).permutation(n_obs).astype("int32")
  n_train = int(train_percent * n_obs)
  return ids[:n_train], ids[n_train:]


def corrupt(x: np.ndarray, dropout_rate: float = 0.2, retain_rate: float = 0.2, distribution: str = "binomial",
            seed: int = 8, inplace: bool = False) -> np.ndarray:
  """x sparse: canonical CSR (`as_csr`) in, CSR out (inplace: `x` itself), the dense twin's values bit for bit -- its non-zeros
  are np.nonzero's row-major order, so the same RandomState picks the same entries; entries set to 0 leave the structure."""
  distribution = str(distribution).lower()
  dropout_rate = float(dropout_rate)
  if not 0 <= dropout_rate < 1:
    raise ValueError(f"dropout value must be >= 0 and < 1, given: {dropout_rate}")
  if is_sparse(x):
    return _corrupt_csr(x, dropout_rate, retain_rate, distribution, seed, inplace)
  out = x if inplace else np.array(x, copy=True)
  if not (0.0 < dropout_rate < 1.0 or 0.0 < retain_rate < 1.0):
    return out
  rand = np.random.RandomState(seed=seed)
  i, j = np.nonzero(x)
  n_sel = int(np.floor(dropout_rate * len(i)))
  if n_sel == 0:   # nothing to corrupt (the reference's rand.choice / fancy indexing fails on this empty case)
    if distribution not in ("binomial", "uniform"):
      raise ValueError("Only support 2 corruption distribution: 'uniform' and 'binomial', "
                       f"but given: '{distribution}'")
    return out
  ix = rand.choice(range(len(i)), size=n_sel, replace=False)
  i, j = i[ix], j[ix]
  if distribution == "binomial":
    vals = rand.binomial(n=(x[i, j]).astype(np.int32), p=retain_rate)
  elif distribution == "uniform":
    vals = np.multiply(x[i, j], rand.binomial(n=np.ones(len(ix), dtype=np.int32), p=retain_rate))
  else:
    raise ValueError("Only support 2 corruption distribution: 'uniform' and 'binomial', "
                     f"but given: '{distribution}'")
  out[i, j] = vals
  return out


def _corrupt_csr(x, dropout_rate, retain_rate, distribution, seed, inplace):
  if not (isinstance(x, sp.csr_matrix) and x.dtype == np.float32 and x.has_canonical_format):
    if inplace:
      raise ValueError("in-place corruption of a sparse matrix needs canonical float32 CSR (data.as_csr)")
    x = as_csr(x)
  out = x if inplace else x.copy()
  if not (0.0 < dropout_rate < 1.0 or 0.0 < retain_rate < 1.0):
    return out
  rand = np.random.RandomState(seed=seed)
  nz = np.flatnonzero(out.data != 0)   # (the stored entries in row-major order: np.nonzero of the dense twin)
  n_sel = int(np.floor(dropout_rate * len(nz)))
  if distribution not in ("binomial", "uniform"):
    raise ValueError("Only support 2 corruption distribution: 'uniform' and 'binomial', "
                     f"but given: '{distribution}'")
  if n_sel == 0:
    return out
  ix = nz[rand.choice(range(len(nz)), size=n_sel, replace=False)]
  if distribution == "binomial":
    vals = rand.binomial(n=out.data[ix].astype(np.int32), p=retain_rate)
  else:
    vals = np.multiply(out.data[ix], rand.binomial(n=np.ones(len(ix), dtype=np.int32), p=retain_rate))
  out.data[ix] = vals
  out.eliminate_zeros()
  return out


def library_size(x: np.ndarray):
  """-> (log_counts [N], local_mean, local_var); the model receives
  library = [[local_mean, local_var]] * N (data/_single_cell_base.py:568-570).  x may be sparse (row sums: `row_sums`)."""
  if x.ndim != 2:
    raise ValueError("Only support 2-D matrix")
  total = row_sums(x)
  log_counts = np.log(total + 1e-8)
  return log_counts, np.float32(np.mean(log_counts)), np.float32(np.var(log_counts))


def library_matrix(x: np.ndarray) -> np.ndarray:
  _, m, v = library_size(x)
  return np.tile(np.array([[m, v]], dtype=np.float32), (x.shape[0], 1))


def label_mask(n_obs: int, labels_percent: float, n_omics: int, seed: int = 1) -> np.ndarray:
  """Per-cell 'labelled' flag drawn once (the reference draws it in a tf.data map and
  freezes it with .cache(''); forced False with a single omic)."""
  labels_percent = float(np.clip(labels_percent, 0.0, 1.0))
  if n_omics <= 1 or labels_percent <= 0.0:
    return np.zeros(n_obs, dtype=bool)
  return np.random.RandomState(seed).uniform(size=n_obs) < labels_percent


_SHUFFLE_LIB = [False]


def _shuffle_lib():
  """libsisua_hip.so when it is built (its smx_shuffle_order is host-only code); None otherwise: the Python walk below
  is the definition, the library only runs it faster (tests/test_data.py checks they agree)."""
  if _SHUFFLE_LIB[0] is False:
    try:
      from sisua_amd import _hip
      _SHUFFLE_LIB[0] = _hip.load()
    except Exception:
      _SHUFFLE_LIB[0] = None
  return _SHUFFLE_LIB[0]


def epoch_order(n_obs: int, epoch: int, shuffle: int = 1000, seed: int = 1) -> np.ndarray:
  """Visit order of one epoch under a streaming shuffle buffer of size `shuffle`
  (tf.data .shuffle(1000) after .cache, before .batch)."""
  if not shuffle or shuffle <= 0:
    return np.arange(n_obs, dtype=np.int32)
  rng = np.random.RandomState(seed + epoch)
  out = np.empty(n_obs, dtype=np.int32)
  picks = rng.randint(0, 2 ** 31 - 1, size=n_obs)
  lib = _shuffle_lib()
  if lib is not None:   # the sequential walk in C (smx_shuffle_order): ~10 us instead of 2.3 ms per 3381-cell epoch
    p64 = np.ascontiguousarray(picks, dtype=np.int64)
    rc = lib.smx_shuffle_order(int(n_obs), int(shuffle), p64.ctypes.data_as(_C.POINTER(_C.c_int64)), out.ctypes.data_as(_C.POINTER(_C.c_int32)))
    if rc == 0:
      return out
  buf = list(range(min(shuffle, n_obs)))
  nxt = len(buf)
  for t in range(n_obs):
    k = picks[t] % len(buf)
    out[t] = buf[k]
    if nxt < n_obs:
      buf[k] = nxt
      nxt += 1
    else:
      buf[k] = buf[-1]
      buf.pop()
  return out


def iter_batches(order: np.ndarray, batch_size: int, drop_remainder: bool = True) -> List[np.ndarray]:
  n = len(order)
  end = (n // batch_size) * batch_size if drop_remainder else n
  return [order[s:s + batch_size] for s in range(0, end, batch_size)]


def shard_for_rank(ids: np.ndarray, rank: int, world: int) -> np.ndarray:
  """Data-parallel partition of the cells: rank r owns ids[r::world] truncated to a
  common length, so every rank runs the same number of steps (no data-path collective)."""
  n = (len(ids) // world) * world
  return ids[:n][rank::world]


def shard_range(n_obs: int, rank: int, world: int) -> Tuple[int, int]:
  """Contiguous data-parallel partition [lo, hi) of the cells (rank r owns N / world cells resident in
  its HBM), every rank the same count.  Contiguous so that a cell's GLOBAL id (the Philox key of its dropout masks
  and eps) is `lo + local row`: the noise of a cell does not depend on how the cells are sharded."""
  n = n_obs // world
  return rank * n, (rank + 1) * n


# ---------------------------------------------------------------------------
# synthetic stand-ins; generator seed 8 = the repo's habitual seed
# ---------------------------------------------------------------------------
def _counts(n, g, rng, gene_sd, size_sd, target_sparsity):
  m_g = rng.normal(0.0, gene_sd, size=g)
  s_c = rng.lognormal(0.0, size_sd, size=n)
  lo, hi = -14.0, 6.0
  gam = rng.gamma(2.0, 0.5, size=(n, g)).astype(np.float32)
  base = (s_c[:, None] * np.exp(m_g)[None, :]).astype(np.float32) * gam
  for _ in range(30):  # bisection on a global offset until P(x == 0) hits the target
    mid = 0.5 * (lo + hi)
    p0 = float(np.exp(-base * np.exp(mid)).mean())
    lo, hi = (lo, mid) if p0 < target_sparsity else (mid, hi)
  x = rng.poisson(base * np.exp(0.5 * (lo + hi))).astype(np.float32)
  return x


def synthetic_8kly(seed: int = 8, n: int = 4697, g: int = 1998, n_proteins: int = 12):
  """pbmc8k_ly-shaped: 4697 x 1998, sparsity ~0.93, mean non-zero count ~4.2, 12
  real-valued protein levels in [0.5, 9.1] (description/dataset.html:187)."""
  rng = np.random.default_rng(seed)
  x = _counts(n, g, rng, 2.9, 0.28, 0.93)
  x[x.sum(1) == 0, 0] = 1.0
  y = np.clip(rng.lognormal(0.9, 0.7, size=(n, n_proteins)), 0.5, 9.1).astype(np.float32)
  return x, y


def synthetic_eccly(seed: int = 8):
  """pbmcecc_ly-shaped: 2941 x 2000, sparsity ~0.89, 38 proteins (dataset.html:217)."""
  rng = np.random.default_rng(seed + 1)
  x = _counts(2941, 2000, rng, 2.6, 0.3, 0.89)
  x[x.sum(1) == 0, 0] = 1.0
  y = np.clip(rng.lognormal(0.9, 0.7, size=(2941, 38)), 0.5, 9.1).astype(np.float32)
  return x, y


def synthetic_cortex(seed: int = 8):
  """cortex-shaped: 3005 x 558, sparsity ~0.29, heavy tail, 7 one-hot cell types
  (dataset.html:31)."""
  rng = np.random.default_rng(seed + 2)
  x = _counts(3005, 558, rng, 1.8, 0.5, 0.29)
  x[rng.integers(0, 3005), rng.integers(0, 558)] = 10738.0
  x[x.sum(1) == 0, 0] = 1.0
  y = np.eye(7, dtype=np.float32)[rng.integers(0, 7, 3005)]
  return x, y


def synthetic_scalability(n: int, seed: int = 8):
  """The reference's own scalability shape: randint(0,100,(n,500)) genes and
  randint(0,10,(n,10)) proteins (tests/test_scalability.py:22-27)."""
  rng = np.random.default_rng(seed)
  return rng.integers(0, 100, size=(n, 500)).astype(np.float32), rng.integers(0, 10, size=(n, 10)).astype(np.float32)


# ---------------------------------------------------------------------------
# Minimal multi-omic container + minibatch description: what SingleCellModel.fit /
# predict need from SingleCellOMIC (data/_single_cell_base.py) without AnnData.
# ---------------------------------------------------------------------------
class BatchDataset:
  """What `SingleCellOMIC.create_dataset` returns in the reference (a tf.data pipeline of
  dict(inputs, library, mask) batches, _single_cell_base.py:539-602), as plain arrays plus
  the batching recipe; the arrays are uploaded to HBM once and minibatches are row ids."""

  def __init__(self, arrays: Sequence[np.ndarray], omics: Sequence[str], library: np.ndarray, mask: np.ndarray,
               batch_size: int = 64, drop_remainder: bool = False, shuffle: int = 1000, seed: int = 1):
    # the counts (arrays[0]) may be sparse: kept as canonical float32 CSR, batches are CSR row blocks; other omics are dense
    self.arrays = [as_csr(a, copy=False) if (i == 0 and is_sparse(a)) else
                   np.ascontiguousarray(a.toarray() if is_sparse(a) else a, dtype=np.float32) for i, a in enumerate(arrays)]
    self.omics = list(omics)
    self.library = np.ascontiguousarray(library, dtype=np.float32)
    self.mask = np.ascontiguousarray(mask, dtype=bool)
    self.batch_size, self.drop_remainder, self.shuffle, self.seed = int(batch_size), bool(drop_remainder), int(shuffle or 0), int(seed)

  @property
  def n_obs(self):
    return self.arrays[0].shape[0]

  def epoch_batches(self, epoch: int) -> List[np.ndarray]:
    return iter_batches(epoch_order(self.n_obs, epoch, self.shuffle, self.seed), self.batch_size, self.drop_remainder)

  def steps_per_epoch(self) -> int:
    n = self.n_obs
    return n // self.batch_size if self.drop_remainder else -(-n // self.batch_size)

  def __iter__(self):
    for ids in self.epoch_batches(0):
      inputs = [a[ids] for a in self.arrays]
      yield dict(inputs=inputs[0] if len(inputs) == 1 else inputs, library=self.library[ids], mask=self.mask[ids])


class SingleCellOMIC:
  """Multi-omic cells x features container with the methods the training path calls on the
  reference's SingleCellOMIC: split, corrupt, library statistics, create_dataset, get_rv, and the preprocessing its loaders call first:
  filter_cells, filter_genes, normalize, expm1, filter_highly_variable_genes."""

  def __init__(self, X, var_names=None, name: str = "scOMICS", omic: str = "transcriptomic"):
    self.name = name
    self._data, self._vars = {}, {}
    self._embeddings = {}   # omic -> (pbe, prob, bin) of probabilistic_embedding; a subset or a copy starts without
    self._pca = {}          # omic -> (PCA, scores) of dimension_reduce; likewise
    self._neighbors = {}    # omic -> (connectivities, distances, params) of neighbors; likewise
    self._tsne = {}         # (omic, n_components) -> the embedding of dimension_reduce(algo='tsne'); likewise
    self._umap = {}         # (omic, n_components) -> the embedding of umap; likewise
    self._uns = {}          # the reference's .uns: 'mutualinfo_{omic}_{target}' -> (omic, target, matrix) of get_mutual_information and
                            # '{omic}_{group_by}_rank' -> (omic, grouping omic or None, dict) of rank_vars_groups; likewise
    self._obs = {}          # the reference's .obs: '{omic}_{algo}{n_clusters}' -> (omic, cluster omic or None, labels) of clustering, and
                            # '{omic}_louvain' / '{omic}_louvain_labels' -> (omic, None, ids / names) of louvain; likewise
    self.add_omic(omic, X, var_names)

  def add_omic(self, omic: str, X, var_names=None):
    """X: dense (stored as float32) or any scipy.sparse matrix (stored as canonical float32 CSR, never densified)."""
    X = as_csr(X) if is_sparse(X) else np.ascontiguousarray(X, dtype=np.float32)
    if self._data and X.shape[0] != self.n_obs:
      raise ValueError(f"Number of cell mismatch {self.n_obs} and {X.shape[0]}")
    self._data[str(omic)] = X
    self._drop_derived(str(omic))
    self._vars[str(omic)] = np.array([f"{omic}{i}" for i in range(X.shape[1])]) if var_names is None else np.asarray(var_names)
    return self

  @property
  def omics(self):
    return list(self._data)

  @property
  def n_omics(self):
    return len(self._data)

  @property
  def n_obs(self):
    return next(iter(self._data.values())).shape[0]

  @property
  def n_vars(self):
    """Number of variables of the first OMIC (AnnData's n_vars; tests/test_singlecell_models.py:127)."""
    return next(iter(self._data.values())).shape[1]

  def get_omic(self, omic):
    return self._data[str(omic)]

  def numpy(self, omic=None):
    return self._data[str(omic) if omic is not None else self.omics[0]]

  def is_sparse(self, omic=None) -> bool:
    return is_sparse(self.numpy(omic))

  def get_dim(self, omic):
    return self._data[str(omic)].shape[1]

  def get_var_names(self, omic):
    return self._vars[str(omic)]

  def __getitem__(self, ids):
    out = None
    for om in self.omics:
      if out is None:
        out = SingleCellOMIC(self._data[om][ids], self._vars[om], name=self.name, omic=om)
      else:
        out.add_omic(om, self._data[om][ids], self._vars[om])
    return out

  def copy(self):
    return self[np.arange(self.n_obs)]

  def split(self, train_percent=0.8, copy=True, seed=1):
    tr, te = split_indices(self.n_obs, train_percent, seed)
    return (None if len(tr) == 0 else self[tr]), (None if len(te) == 0 else self[te])

  def corrupt(self, dropout_rate=0.2, retain_rate=0.2, distribution="binomial", omic=None, inplace=True, seed=8):
    om = self if inplace else self.copy()
    key = str(omic) if omic is not None else om.omics[0]
    corrupt(om._data[key], dropout_rate, retain_rate, distribution, seed, inplace=True)
    return om

  def sparsity(self, omic=None):
    x = self.numpy(omic)
    if is_sparse(x):   # (canonical CSR: every stored entry is non-zero)
      return float((x.shape[0] * x.shape[1] - x.nnz) / (x.shape[0] * x.shape[1]))
    return float((x == 0).mean())

  def library_size(self, omic=None):
    return library_matrix(self.numpy(omic))

  # ---- preprocessing (sisua_amd/preprocess.py; the matrix work runs on the device: smx_prep.hip) ----
  def _first(self, omic=None) -> str:
    return str(omic) if omic is not None else self.omics[0]

  def _drop_derived(self, key: str):
    for cache in (self._embeddings, self._pca, self._neighbors):
      cache.pop(key, None)
    for cache in (self._tsne, self._umap):
      for kc in [kc for kc in cache if kc[0] == key]:
        del cache[kc]
    for store in (self._uns, self._obs):
      for kc in [kc for kc, v in store.items() if key in v[:2]]:
        del store[kc]

  def _replace(self, key: str, X, var_names=None):
    """A new matrix for an omic already held (same cells); its embedding, PCA and neighbour graph, if any, no longer describe it"""
    self._data[key] = as_csr(X) if is_sparse(X) else np.ascontiguousarray(X, dtype=np.float32)
    self._drop_derived(key)
    if var_names is not None:
      self._vars[key] = np.asarray(var_names)

  def filter_cells(self, min_counts=None, max_counts=None, min_genes=None, max_genes=None, inplace=True):
    """The reference's filter_cells (scanpy.pp.filter_cells on the first omic): exactly one bound; a cell is kept when its total count
    (`*_counts`) or its number of expressed genes (`*_genes`) is >= the minimum or <= the maximum.  The cells leave every omic."""
    from sisua_amd import preprocess
    keep, _ = preprocess.filter_cells(self.numpy(), min_counts, max_counts, min_genes, max_genes)
    om = self if inplace else self.copy()
    for key in om.omics:
      om._replace(key, om._data[key][keep])
    om.name += "_filtercell"
    return om

  def filter_genes(self, min_counts=None, max_counts=None, min_cells=None, max_cells=None, inplace=True):
    """The reference's filter_genes (scanpy.pp.filter_genes on the first omic): exactly one bound on a gene's total count or on the number
    of cells that express it.  The genes leave the first omic and its var_names."""
    from sisua_amd import preprocess
    keep, _ = preprocess.filter_genes(self.numpy(), min_counts, max_counts, min_cells, max_cells)
    om = self if inplace else self.copy()
    key = om.omics[0]
    om._replace(key, om._data[key][:, keep], om._vars[key][keep])
    om.name += "_filtergene"
    return om

  def filter_highly_variable_genes(self, min_disp=1.0, max_disp=np.inf, min_mean=0.01, max_mean=8, n_top_genes=1000, n_bins=20,
                                   flavor="seurat", inplace=True):
    """The reference's filter_highly_variable_genes (scanpy.pp.highly_variable_genes, subset=True; expects logarithmised data): the first
    omic keeps its highly variable genes.  `highly_variable_features` of the result holds highly_variable, means, dispersions and
    dispersions_norm of every gene it had before."""
    from sisua_amd import preprocess
    res = preprocess.highly_variable_genes(self.numpy(), min_disp, max_disp, min_mean, max_mean, n_top_genes, n_bins, flavor)
    om = self if inplace else self.copy()
    key, keep = om.omics[0], res["highly_variable"]
    om._replace(key, om._data[key][:, keep], om._vars[key][keep])
    om.highly_variable_features = {k: res[k] for k in ("highly_variable", "means", "dispersions", "dispersions_norm")}
    om.name += "_vargene"
    return om

  def expm1(self, omic=None, inplace=True):
    from sisua_amd import preprocess
    key = self._first(omic)
    X = preprocess.apply_view(self.numpy(key), func="expm1")
    om = self if inplace else self.copy()
    om._replace(key, X)
    return om

  def normalize(self, omic=None, total=False, log1p=False, scale=False, target_sum=None, exclude_highly_expressed=False,
                max_fraction=0.05, max_value=None, inplace=True):
    """The reference's normalize (scanpy.pp.normalize_total, log1p, scale, in this order, each where asked).  The stages are composed into
    one view f(x / c) of the matrix, so it crosses to the device once per pass; a sparse omic stays sparse unless it is scaled.
    max_value clips from above only."""
    from sisua_amd import preprocess
    preprocess.check_normalize(target_sum, max_fraction, max_value)
    key = self._first(omic)
    X = self.numpy(key)
    suffix = ("_total" if total else "") + ("_log1p" if log1p else "") + ("_scale" if scale else "")
    if suffix:
      c = preprocess.total_size_factors(X, target_sum, exclude_highly_expressed, max_fraction) if total else None
      X = preprocess.apply_view(X, func="log1p" if log1p else None, row_div=c, scale=bool(scale), max_value=max_value)
    om = self if inplace else self.copy()
    if suffix:
      om._replace(key, X)
      om.name += suffix
    return om

  def probabilistic_embedding(self, omic=None, n_components_per_class=2, positive_component=1, log_norm=True, clip_quartile=0.,
                              remove_zeros=True, ci_threshold=-0.68, seed=1, pbe=None):
    """The reference's SingleCellOMIC.probabilistic_embedding (_single_cell_analysis.py:311-383): one Gaussian mixture per column of the
    omic, fitted on the device -> (the `ProbabilisticEmbedding`, prob [cells, C] clipped to [1e-8, 1 - 1e-8], bin [cells, C]).  A matrix
    that holds only 0 / 1 is its own embedding (pbe None).  A given `pbe` is used without fitting.  The first result of an omic is kept on
    the object and returned from then on; a sparse omic is densified for the call (a protein panel is narrow)."""
    import warnings
    from sisua_amd.label_threshold import ProbabilisticEmbedding
    key = str(omic) if omic is not None else self.omics[0]
    if pbe is not None and not isinstance(pbe, ProbabilisticEmbedding):
      raise TypeError("pbe, if given, must be instance of sisua_amd.ProbabilisticEmbedding")
    if float(clip_quartile) > 0:
      raise ValueError("clip_quartile > 0 is not built: only clip_quartile = 0 is")
    if key in self._embeddings:
      return self._embeddings[key]
    X = self.numpy(key)
    X = X.toarray() if is_sparse(X) else X
    if X.shape[1] >= 100:
      warnings.warn("%d GMM will be trained!" % X.shape[1])
    if np.all((X == 0) | (X == 1)):
      self._embeddings[key] = (None, X, X)
      return self._embeddings[key]
    if pbe is None:
      pbe = ProbabilisticEmbedding(n_components_per_class=n_components_per_class, positive_component=positive_component, log_norm=log_norm,
                                   clip_quartile=clip_quartile, remove_zeros=remove_zeros, ci_threshold=ci_threshold, random_state=seed)
      pbe.fit(X)
    prob = np.clip(pbe.predict_proba(X), 0. + 1e-8, 1. - 1e-8)
    self._embeddings[key] = (pbe, prob, pbe.predict(X))
    return self._embeddings[key]

  def get_x_probs(self, omic=None):
    """The probability embedding of an omic (`probabilistic_embedding` with its defaults, or what an earlier call left)"""
    return self.probabilistic_embedding(omic=omic)[1]

  def get_x_bins(self, omic=None):
    return self.probabilistic_embedding(omic=omic)[2]

  # ---- analysis (sisua_amd/neighbors.py; the matrix work runs on the device: smx_pca.hip, smx_knn.hip) ----
  def dimension_reduce(self, omic=None, n_components=100, algo="pca", random_state=1):
    """The reference's dimension_reduce(algo='pca'): the scores [cells, min(n_components, dim)] float32 of an EXACT PCA of the omic (the
    reference's IncrementalPCA over batches of 4096 rows is exact for one batch and approximates it for several).  The model
    (`sisua_amd.PCA`) and its scores are kept on the object: a later call that asks for no more components returns a column slice, one
    that asks for more refits.  PCA is deterministic: random_state is accepted and unused.
    algo='tsne': the t-SNE embedding [cells, n_components] float32 of the omic (`sisua_amd.TSNE` with its defaults: scikit-learn's
    objective with the exact repulsive sum).  n_components must be 1, 2 or 3 -- the signature's default of 100 belongs to 'pca' and is
    refused.  As in `neighbors`, an omic wider than 100 columns goes through dimension_reduce(algo='pca') first (its 100 scores; a kept
    PCA is reused).  The start is the PCA init, so random_state is unused.  The result is kept per omic and n_components.
    'umap' is not built under this name: the UMAP embedding is `SingleCellOMIC.umap`."""
    from sisua_amd import neighbors as nb
    algo = str(algo).lower().strip()
    if algo == "umap":
      raise NotImplementedError(f"dimension_reduce(algo={algo!r}) is not built: only algo='pca' and algo='tsne' are; the UMAP embedding "
                                "is SingleCellOMIC.umap")
    if algo == "tsne":
      C = nb.check_tsne_components(n_components)   # (before anything else is looked at)
      key = self._first(omic)
      if (key, C) not in self._tsne:
        if self.get_dim(key) > 100:
          rep = self.dimension_reduce(key, algo="pca", random_state=random_state)
        else:
          rep = self.numpy(key)
          rep = rep.toarray() if is_sparse(rep) else rep
        self._tsne[(key, C)] = nb.tsne(rep, n_components=C, random_state=random_state)
      return self._tsne[(key, C)]
    if algo != "pca":
      raise ValueError(f"Only support algorithm: 'pca', 'tsne', 'umap'; but given: '{algo}'")
    key = self._first(omic)
    X = self.numpy(key)
    if int(n_components) < 1:
      raise ValueError(f"n_components must be >= 1, got {n_components}")
    C = min(int(n_components), X.shape[1])
    if key not in self._pca or self._pca[key][1].shape[1] < C:
      self._pca[key] = nb.pca(X, C)
    scores = self._pca[key][1]
    return scores if scores.shape[1] == C else scores[:, :C]

  def get_mutual_information(self, omic="transcriptomic", target_omic="proteomic", n_neighbors=3, random_state=1):
    """The reference's get_mutual_information (_single_cell_analysis.py:1148-1196): the mutual information [n_vars of omic, n_vars of
    target_omic] float64 between every feature of one omic and every feature of another, scikit-learn's kNN estimators
    (`sisua_amd.mutual_information`: discrete columns are those whose every value is an integer; the estimators run on the device,
    smx_mi.hip).  As in the reference the seed is fixed at 1 whatever `random_state`, the two omics must differ, and the matrix is kept
    under 'mutualinfo_{omic}_{target_omic}' until one of the two omics is replaced: a later call returns it whatever its n_neighbors."""
    from sisua_amd.mutual_info import mutual_information
    n_neighbors, random_state = int(n_neighbors), 1
    om1, om2 = self._first(omic), self._first(target_omic)
    assert om1 != om2, "Mutual information only for 2 different OMIC type"
    uns_key = f"mutualinfo_{om1}_{om2}"
    if uns_key not in self._uns:
      self._uns[uns_key] = (om1, om2, mutual_information(self.numpy(om1), self.numpy(om2), n_neighbors=n_neighbors, random_state=random_state))
    return self._uns[uns_key][2]

  def get_importance_matrix(self, omic="transcriptomic", target_omic="proteomic", random_state=1):
    """The reference's get_importance_matrix (_single_cell_analysis.py:1107-1145): the importance [n_vars of omic, n_vars of target_omic]
    float64 of every feature of one omic for every feature of another -- per target feature one gradient-boosted tree classifier on the
    device (`sisua_amd.importance_matrix`, smx_gbt.hip), whose feature_importances_ are the column.  As in the reference: the two omics
    must differ; a target that is not discrete (`mutual_info.is_discrete` of the whole matrix) is cut into 10 quantile bins per column
    (`boosting.quantile_codes`: the ordinal KBinsDiscretizer(strategy='quantile')); the seed is 1 whatever `random_state`; the cells are
    split 75 / 25 by RandomState(1).permutation and the fits take random_state=rand.randint(1e8).  A sparse omic stays CSR.  A target
    feature with a single class among the training cells gives a zero column (with a RuntimeWarning).  The matrix is kept under
    'importance_{omic}_{target_omic}' until one of the two omics is replaced."""
    from sisua_amd.boosting import importance_matrix, quantile_codes
    from sisua_amd.mutual_info import is_discrete
    random_state = 1
    om1, om2 = self._first(omic), self._first(target_omic)
    assert om1 != om2, "Mutual information only for 2 different OMIC type"
    uns_key = f"importance_{om1}_{om2}"
    if uns_key not in self._uns:
      X, y = self.numpy(om1), self.numpy(om2)
      X = X.tocsr() if is_sparse(X) else X
      y = np.asarray(y.toarray() if is_sparse(y) else y)
      if not is_discrete(y):
        y = np.stack([quantile_codes(y[:, j], 10) for j in range(y.shape[1])], axis=1)
      rand = np.random.RandomState(random_state)
      ids = rand.permutation(X.shape[0])
      cut = int(0.75 * X.shape[0])
      train, test = ids[:cut], ids[cut:]
      matrix, _, _ = importance_matrix(X[train], y[train], X[test], y[test], random_state=rand.randint(1e8))
      self._uns[uns_key] = (om1, om2, matrix)
    return self._uns[uns_key][2]

  def rank_vars_groups(self, n_vars=100, group_by="proteomic", clustering="kmeans", method="logreg", corr_method="benjamini-hochberg",
                       max_iter=1000, reference="rest"):
    """The reference's rank_vars_groups (_single_cell_analysis.py:862-918, scanpy.tl.rank_genes_groups there): the variables of the FIRST
    omic ranked for characterising groups of cells (`sisua_amd.rank_genes_groups`; the matrix work runs on the device, smx_rankgroups.hip).
    group_by: a [cells] array of labels, or the name of an omic with clustering=None -- each cell's label is then the variable name at
    the argmax of `get_x_probs(omic)`, as the reference's '{omic}_labels'.  method: 't-test', 't-test_overestim_var', 'wilcoxon', or
    'logreg' (the reference's default: `sisua_amd.rank_genes_groups_logreg`, one L2-penalised logistic regression solved on the device,
    smx_logreg.hip, with at most max_iter iterations; its dict holds 'params', 'names' and 'scores' only, and corr_method is ignored).
    The result is kept under '{omic}_{group_by}_rank' ('labels' for an array) until an omic it was made from is replaced; a later call
    returns what is kept, whatever its other arguments.  Returns the key, as the reference does: `get_rank_vars_groups(key)` gives the dict.
    group_by may also be a key that `clustering(..., return_key=True)` or `louvain` ('{omic}_louvain') left (the reference's `if
    str(group_by) in self.obs`): its labels
    are ranked, under '{omic}_{that key}_rank', until the first omic or the clustered one is replaced.  The reference's default --
    an omic's name with clustering='kmeans' -- takes two calls here: `key = sco.clustering(first omic, n_clusters=group_by,
    return_key=True)`, then `sco.rank_vars_groups(group_by=key, ...)`.
    Deviations: there is no use_raw (the omic is ranked as it stands); an omic's name with clustering='kmeans' (the reference's
    default) raises NotImplementedError naming clustering=None, whatever the method; max_iter belongs to method='logreg' and is unused
    by the others."""
    from sisua_amd.rank_groups import METHODS, rank_genes_groups, rank_genes_groups_logreg
    built = (f"rank_vars_groups is built for method in {METHODS} with group_by a [cells] label array or an omic's name with "
             "clustering=None")
    om1 = self.omics[0]
    kept = None
    if isinstance(group_by, str) and group_by in self._obs:
      kept, (om2, name) = self._obs[group_by][2], (self._obs[group_by][0], group_by)
    elif isinstance(group_by, str):
      if group_by not in self._data:
        raise ValueError(f"group_by={group_by!r} is neither a [cells] label array, one of the omics {self.omics} nor a key that "
                         f"clustering(return_key=True) left ({sorted(self._obs)})")
      if clustering is not None:
        raise NotImplementedError(f"clustering={clustering!r} is not built (SingleCellOMIC.clustering): {built}")
      om2, name = group_by, group_by
    else:
      om2, name = None, "labels"
    key = f"{om1}_{name}_rank"
    if key not in self._uns:
      if kept is not None:
        labels = kept
      elif om2 is None:
        labels = np.asarray(group_by)
        if labels.shape != (self.n_obs,):
          raise ValueError(f"group_by must be [{self.n_obs}] labels, got {labels.shape}")
      else:
        labels = np.asarray(self._vars[om2])[np.argmax(self.get_x_probs(om2), axis=1)]
      if method == "logreg":   # (corr_method is ignored, as in the reference: a logistic fit has no p-values)
        res = rank_genes_groups_logreg(self.numpy(om1), labels, reference=reference, n_genes=int(n_vars), var_names=self._vars[om1],
                                       max_iter=int(max_iter))
      else:
        res = rank_genes_groups(self.numpy(om1), labels, reference=reference, method=method, corr_method=corr_method, n_genes=int(n_vars),
                                var_names=self._vars[om1])
      self._uns[key] = (om1, om2, res)
    return key

  def get_rank_vars_groups(self, key):
    """The dict `rank_vars_groups` left under `key`"""
    if key not in self._uns or not str(key).endswith("_rank"):
      raise KeyError(f"no ranked groups under {key!r}: call rank_vars_groups first")
    return self._uns[key][2]

  def clustering(self, omic=None, n_clusters=None, n_init="auto", algo="kmeans", matching_labels=True, return_key=False, random_state=1):
    """The reference's clustering (_single_cell_analysis.py:632-730) for algo in ('kmeans', 'pca', 'tsne'): `sisua_amd.MiniBatchKMeans`
    (n_clusters, batch_size=4096, compute_labels=False, random_state) -- scikit-learn's class there, its distance sweeps on the device
    here (smx_mbkmeans.hip) -- takes one `partial_fit` per batch of 4096 cells and then predicts every cell.
    n_clusters: None -> the omic's own width, a number as given, an omic's name -> that omic's width; None and a name make that omic
    the cluster omic.  algo='kmeans' clusters the omic as it stands (dense or CSR, never densified whole), 'pca' its
    dimension_reduce(n_components=100, algo='pca') and 'tsne' its dimension_reduce(n_components=2, algo='tsne') (the reference's 100 is
    refused there).  With a cluster omic and matching_labels each cluster is named after one of its variables: corr[i, c] = the float64
    sum of get_x_probs(cluster omic)[:, i] over the cells of cluster c, `scipy.optimize.linear_sum_assignment(corr, maximize=True)`
    gives every variable i its cluster ids[i], and cluster ids[i] takes the name of variable i.
    The labels [cells] (int64 ids, or names) are kept under '{omic}_{algo}{n_clusters}' until the omic or the cluster omic is replaced; a
    later call returns what is kept, whatever its other arguments.  return_key: the key instead of the labels (for
    `rank_vars_groups(group_by=key)`).
    Two readings of code that is not at hand, stated as such: the reference's `odin.utils.batching(4096, n, seed=random_state)` is
    taken as the batches (s, min(s + 4096, n)) in the order RandomState(random_state).permutation(n_batches), and its
    `diagonal_linear_assignment` as the assignment above.  n_init is accepted and unused (partial_fit never reads it).
    Not built: algo='knn' (spectral clustering) and 'umap' raise NotImplementedError, as does any other algo."""
    from sisua_amd.clustering import BATCH_SIZE, match_clusters, minibatch_kmeans
    algo = str(algo).strip().lower()
    key = self._first(omic)
    if key not in self._data:
      raise ValueError(f"omic={omic!r} is not one of the omics {self.omics}")
    cluster_omic = None
    if n_clusters is None:
      cluster_omic = key
    elif isinstance(n_clusters, numbers.Number):
      n_clusters = int(n_clusters)
    else:
      cluster_omic = str(n_clusters)
      if cluster_omic not in self._data:
        raise ValueError(f"n_clusters={n_clusters!r} is neither a number nor one of the omics {self.omics}")
    K = self.get_dim(cluster_omic) if cluster_omic is not None else n_clusters
    name = f"{key}_{algo}{K}"
    if name in self._obs:
      return name if return_key else self._obs[name][2]
    if algo not in ("kmeans", "pca", "tsne"):
      raise NotImplementedError(f"clustering(algo={algo!r}) is not built: only algo='kmeans', 'pca' and 'tsne' are (the UMAP embedding "
                                "itself is SingleCellOMIC.umap)")
    if algo == "kmeans":
      X = self.numpy(key)
    else:
      X = self.dimension_reduce(omic=key, n_components=100 if algo == "pca" else 2, algo=algo)
    labels = minibatch_kmeans(X, K, batch_size=BATCH_SIZE, random_state=random_state).astype(np.int64)
    if cluster_omic is not None and matching_labels:
      ids = match_clusters(labels, self.get_x_probs(cluster_omic), K)
      names = {int(c): n for c, n in zip(ids, self._vars[cluster_omic])}
      labels = np.array([names[int(c)] for c in labels])
    self._obs[name] = (key, cluster_omic, labels)
    return name if return_key else labels

  def louvain(self, omic=None, resolution=None, restrict_to=None, adjacency=None, flavor="vtraag", directed=True, use_weights=False,
              partition_type=None, partition_kwargs={}, random_state=1):
    """The reference's louvain (_single_cell_analysis.py:732-835, scanpy.tl.louvain there): the Louvain communities of the omic's
    neighbour graph -- `self.neighbors(omic)[0]`, or `adjacency` (any symmetric scipy.sparse matrix over the cells) -- found on the
    device (`sisua_amd.louvain`, smx_louvain.hip) -> (y float32 [cells], y_labels str [cells]).  resolution=None is 1.0; use_weights takes
    the graph's weights instead of unit weights on its support.  y: the ids by decreasing size.  y_labels: each community named as in the
    reference -- `get_x_probs(omic)` summed over its cells, thresholded (`sisua_amd.communities.threshold_variables`), the chosen
    variables' names joined with '_'; an omic of fewer than 5 variables names a community str(id).  The ids (int64) are kept under
    '{omic}_louvain' and the names under '{omic}_louvain_labels' until the omic is replaced, and a later call returns what is kept,
    whatever its arguments; `rank_vars_groups(group_by='{omic}_louvain')` ranks the communities.
    Deviations: the method is deterministic, so random_state is accepted and unused; a symmetric graph has one
    modularity, so `directed` is accepted either way; flavor 'vtraag' and 'igraph' are the same call; restrict_to, partition_type and a
    non-empty partition_kwargs raise NotImplementedError; the names come from `sisua_amd.GaussianMixture`, not scikit-learn's."""
    from sisua_amd import communities
    if restrict_to is not None or partition_type is not None or partition_kwargs:
      raise NotImplementedError("louvain(restrict_to=, partition_type=, partition_kwargs=) are not built: only the modularity partition "
                                "of all cells is")
    if flavor not in ("vtraag", "igraph"):
      raise ValueError(f"flavor must be 'vtraag' or 'igraph', got {flavor!r}")
    key = self._first(omic)
    if key not in self._data:
      raise ValueError(f"omic={omic!r} is not one of the omics {self.omics}")
    name, name_labels = f"{key}_louvain", f"{key}_louvain_labels"
    if name not in self._obs:
      if adjacency is not None and (not hasattr(adjacency, "shape") or tuple(adjacency.shape) != (self.n_obs, self.n_obs)):
        raise ValueError(f"adjacency must be a sparse matrix [{self.n_obs}, {self.n_obs}] over the cells")
      graph = self.neighbors(key)[0] if adjacency is None else adjacency
      ids = communities.louvain(graph, resolution=1.0 if resolution is None else resolution, use_weights=bool(use_weights))
      self._obs[name] = (key, None, ids)
      self._obs.pop(name_labels, None)
    ids = self._obs[name][2]
    if name_labels not in self._obs:
      names = communities.community_names(ids, self.get_x_probs(key), self._vars[key])
      self._obs[name_labels] = (key, None, np.array([names[int(c)] for c in ids]))
    return ids.astype(np.float32), self._obs[name_labels][2]

  def umap(self, omic=None, n_components=2, min_dist=0.5, spread=1.0, n_epochs=None, random_state=1):
    """The UMAP embedding [cells, n_components] float32 of the omic (the reference's dimension_reduce(algo='umap'), which calls cuML or
    umap-learn; scanpy's tl.umap defaults min_dist = 0.5, spread = 1): the layout (`sisua_amd.neighbors.umap_layout`, the per-epoch form
    on the device, smx_umap.hip) of `self.neighbors(omic)`'s connectivities -- the kept graph, or the one a first call of neighbors with
    its defaults leaves.  n_components must be 1, 2 or 3.  The start is the PCA init as in dimension_reduce(algo='tsne'): the first
    n_components exact-PCA scores of the representation (an omic wider than 100 columns goes through dimension_reduce(algo='pca') first;
    a kept PCA is reused), mapped per axis to [0, 10]; random_state seeds the negative samples.  The result is kept per omic and
    n_components until the omic is replaced, and a later call returns it whatever its other arguments.
    Not built: spectral init, transform of new cells, other output metrics; dimension_reduce(algo='umap') and clustering(algo='umap')
    keep raising NotImplementedError."""
    from sisua_amd import neighbors as nb
    C = nb.check_umap_components(n_components)   # (before anything else is looked at)
    key = self._first(omic)
    if key not in self._data:
      raise ValueError(f"omic={omic!r} is not one of the omics {self.omics}")
    if (key, C) not in self._umap:
      nb._umap_params(self.n_obs, C, min_dist, spread, n_epochs, 1.0, 1.0, 5, random_state)   # (refusals before any device work)
      graph = self.neighbors(key)[0]
      if self.get_dim(key) > 100:
        rep = self.dimension_reduce(key, algo="pca")
      else:
        rep = self.numpy(key)
        rep = rep.toarray() if is_sparse(rep) else rep
      Y0 = nb.umap_init(self.n_obs, C, "pca", random_state, rep)
      self._umap[(key, C)] = nb.umap_layout(graph, C, min_dist, spread, n_epochs, init=Y0, random_state=random_state)
    return self._umap[(key, C)]

  def get_pca(self, omic=None):
    """The fitted `sisua_amd.PCA` of an omic (what `dimension_reduce` left), or None"""
    return self._pca.get(self._first(omic), (None, None))[0]

  def neighbors(self, omic=None, n_neighbors=12, n_pcs=100, knn=True, method="umap", metric="euclidean", random_state=1):
    """The reference's neighbors (scanpy.pp.neighbors there): each cell's n_neighbors - 1 nearest other cells, EXACT over all pairs, with
    UMAP's connectivities -> (connectivities, distances, {'params': ...}), the graphs scipy.sparse CSR float32 [cells, cells].  As in the
    reference an omic wider than 100 columns is first reduced with dimension_reduce(algo='pca'); the first min(n_pcs, width) columns of
    the representation are used.  The first result of an omic is kept on the object and returned from then on.  Only knn=True,
    method='umap' and metric='euclidean' are built; 2 <= n_neighbors <= min(257, cells)."""
    from sisua_amd import neighbors as nb
    if not knn:
      raise NotImplementedError("neighbors(knn=False) is not built: only the hard k-nearest-neighbour graph (knn=True) is")
    if str(method).lower() != "umap":
      raise NotImplementedError(f"neighbors(method={method!r}) is not built: only method='umap' is")
    if not isinstance(metric, str) or metric.lower() != "euclidean":
      raise NotImplementedError(f"neighbors(metric={metric!r}) is not built: only metric='euclidean' is")
    K = nb.check_n_neighbors(n_neighbors, self.n_obs)
    if int(n_pcs) < 1:
      raise ValueError(f"n_pcs must be >= 1, got {n_pcs}")
    key = self._first(omic)
    if key in self._neighbors:
      return self._neighbors[key]
    if self.get_dim(key) > 100:
      rep, use_rep = self.dimension_reduce(key, algo="pca", random_state=random_state), key + "_pca"
    else:
      rep, use_rep = self.numpy(key), key
      rep = rep.toarray() if is_sparse(rep) else rep
    width = min(int(n_pcs), rep.shape[1])
    conn, dist = nb.neighbors(np.ascontiguousarray(rep[:, :width]), K)
    params = {"params": {"n_neighbors": K, "method": "umap", "metric": "euclidean", "n_pcs": width, "use_rep": use_rep}}
    self._neighbors[key] = (conn, dist, params)
    return self._neighbors[key]

  def get_rv(self, omic, distribution=None):
    from sisua_amd.config import RVmeta
    omic = str(omic)
    if distribution is None:
      if omic in ("transcriptomic", "atac", "chromatin"):
        distribution = "zinb"
      elif omic == "proteomic":
        distribution = "nb"
      elif omic in ("celltype", "disease", "progenitor"):
        distribution = "onehot"
      else:
        raise ValueError(f"No default distribution for OMIC {omic}")
    return RVmeta(event_shape=self.get_dim(omic), posterior=distribution, projection=True, name=omic)

  create_rv = get_rv

  def create_dataset(self, omics=None, labels_percent=0, batch_size=64, drop_remainder=False, shuffle=1000, seed=1):
    if omics is None:
      omics = [self.omics[0]]
    if isinstance(omics, str):
      omics = [omics]
    omics = [str(o) for o in omics]
    arrays = [self.get_omic(o) for o in omics]
    return BatchDataset(arrays, omics, self.library_size(omics[0]), label_mask(self.n_obs, labels_percent, len(omics), seed),
                        batch_size, drop_remainder, shuffle, seed)

  def __repr__(self):
    return f"<SingleCellOMIC '{self.name}' n_obs={self.n_obs} " + " ".join(f"{o}:{self.get_dim(o)}" for o in self.omics) + ">"
