"""Sparse count matrices on the host (no GPU): SingleCellOMIC holds any scipy.sparse input as canonical float32 CSR, every
method gives its dense twin's values (corrupt and library_size bit for bit, also against the reference's own fixtures), no
whole matrix is densified on the way to the device, and the C entry points for CSR host rows are declared and exported."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from sisua_amd import data
from sisua_amd.data import SingleCellOMIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = np.load(os.path.join(ROOT, "tests", "golden", "reference_data_fixtures.npz"))


def _dense(n=60, g=23, seed=0):
  rng = np.random.default_rng(seed)
  x = rng.poisson(1.5, size=(n, g)).astype(np.float32) * (rng.uniform(size=(n, g)) < 0.3)
  x[3] = 0.0
  return x


def _inputs(x):
  """The same counts in every form the constructor must take."""
  i, j = np.nonzero(x)
  v = x[i, j]
  half = v // 2
  dup = sp.coo_matrix((np.concatenate([v - half, half]).astype(np.int64), (np.concatenate([i, i]), np.concatenate([j, j]))), shape=x.shape)
  zeros = sp.csr_matrix((np.concatenate([v, [0.0, 0.0]]), (np.concatenate([i, [3, 3]]), np.concatenate([j, [0, 1]]))),
                        shape=x.shape)   # explicit zeros in the empty row 3
  assert zeros.nnz == len(v) + 2
  unsorted = sp.csr_matrix(x)
  for r in range(x.shape[0]):
    a, b = unsorted.indptr[r], unsorted.indptr[r + 1]
    unsorted.indices[a:b] = unsorted.indices[a:b][::-1].copy()
    unsorted.data[a:b] = unsorted.data[a:b][::-1].copy()
  unsorted.has_sorted_indices = False
  return dict(csr=sp.csr_matrix(x), csc=sp.csc_matrix(x), coo=sp.coo_matrix(x), int=sp.csr_matrix(x.astype(np.int32)),
              unsorted=unsorted, duplicates=dup, explicit_zeros=zeros, csr_array=sp.csr_array(x))


FORMS = list(_inputs(_dense()))


def _canonical(m):
  assert isinstance(m, sp.csr_matrix) and m.dtype == np.float32
  assert m.has_sorted_indices and m.has_canonical_format and not (m.data == 0).any()


@pytest.mark.parametrize("form", FORMS)
def test_constructor_stores_canonical_csr(form):
  x = _dense()
  src = _inputs(x)[form]
  before = src.copy()
  s = SingleCellOMIC(src)
  m = s.numpy()
  _canonical(m)
  assert s.is_sparse() and s.get_omic("transcriptomic") is m
  assert np.array_equal(m.toarray(), x)
  assert (src != before).nnz == 0   # (the caller's matrix is left alone)
  s.add_omic("proteomic", _inputs(x)["coo"])
  _canonical(s.numpy("proteomic"))
  assert not SingleCellOMIC(x).is_sparse()


@pytest.mark.parametrize("form", FORMS)
def test_methods_equal_dense_twin(form):
  x = _dense()
  s, d = SingleCellOMIC(_inputs(x)[form]).add_omic("celltype", np.eye(3, dtype=np.float32)[np.arange(60) % 3]), \
      SingleCellOMIC(x).add_omic("celltype", np.eye(3, dtype=np.float32)[np.arange(60) % 3])
  for a, b in zip(s.split(0.7), d.split(0.7)):
    _canonical(a.numpy())
    assert np.array_equal(a.numpy().toarray(), b.numpy()) and np.array_equal(a.numpy("celltype"), b.numpy("celltype"))
  assert np.array_equal(s.copy().numpy().toarray(), x)
  ids = np.array([5, 3, 3, 59, 0])
  assert np.array_equal(s[ids].numpy().toarray(), x[ids])
  assert s.sparsity() == d.sparsity()
  assert np.array_equal(s.library_size(), d.library_size())
  for shuffle in (0, 1000):
    ds, dd = (o.create_dataset(["transcriptomic", "celltype"], labels_percent=0.5, batch_size=16, shuffle=shuffle) for o in (s, d))
    assert sp.issparse(ds.arrays[0]) and isinstance(ds.arrays[1], np.ndarray)
    assert np.array_equal(ds.library, dd.library) and np.array_equal(ds.mask, dd.mask)
    for bs, bd in zip(ds, dd):
      assert sp.issparse(bs["inputs"][0]) and np.array_equal(bs["inputs"][0].toarray(), bd["inputs"][0])
      assert np.array_equal(bs["inputs"][1], bd["inputs"][1]) and np.array_equal(bs["library"], bd["library"])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dist", ["binomial", "uniform"])
def test_corrupt_bitwise_equals_dense(form, dist):
  x = _dense()
  for rate, keep, seed in ((0.2, 0.2, 8), (0.35, 0.5, 1), (0.0, 1.0, 8)):
    s = SingleCellOMIC(_inputs(x)[form]).corrupt(rate, keep, dist, seed=seed)
    d = SingleCellOMIC(x).corrupt(rate, keep, dist, seed=seed)
    _canonical(s.numpy())
    assert np.array_equal(s.numpy().toarray(), d.numpy())
  out = data.corrupt(sp.csr_matrix(x), 0.3, 0.1, dist, seed=2)
  _canonical(out)
  assert np.array_equal(out.toarray(), data.corrupt(x, 0.3, 0.1, dist, seed=2))


def test_corrupt_and_library_against_reference_fixtures():
  x = sp.csr_matrix(FX["x"])
  assert np.array_equal(data.corrupt(x, 0.2, 0.2, seed=8).toarray(), FX["corrupt_seed8"])
  assert np.array_equal(data.corrupt(x, 0.35, 0.5, seed=8).toarray(), FX["corrupt_d35_r50_seed8"])
  y = data.as_csr(x)
  out = data.corrupt(y, 0.2, 0.2, seed=1, inplace=True)
  assert out is y and np.array_equal(y.toarray(), FX["corrupt_seed1"])
  lc, lm, lv = data.library_size(sp.csr_matrix(FX["lib_x"]))
  assert np.array_equal(lc.reshape(-1, 1).astype(np.float64), FX["lib_log_counts"])
  assert np.all(FX["lib_local_mean"] == lm) and np.all(FX["lib_local_var"] == lv)


def test_library_size_exact_below_2_24():
  """Integer counts whose row sums reach 2**24 - 1: still the dense float32 sums exactly."""
  x = np.zeros((4, 300), np.float32)
  x[0, :256] = 65535.0
  x[0, 256] = 2 ** 24 - 1 - 256 * 65535
  x[1, ::3] = 7.0
  assert data.row_sums(sp.csr_matrix(x))[0] == 2 ** 24 - 1
  assert np.array_equal(data.row_sums(sp.csr_matrix(x)), x.sum(axis=1))
  assert np.array_equal(data.library_matrix(sp.csr_matrix(x)), data.library_matrix(x))


@pytest.fixture
def no_densify(monkeypatch):
  """toarray / todense of every scipy class raise on more rows than a row block (the engine's batches: <= 512 rows)."""
  for cls in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix, sp.csr_array, sp.spmatrix):
    for name in ("toarray", "todense"):
      orig = getattr(cls, name, None)
      if orig is None:
        continue

      def guarded(self, *a, _orig=orig, **kw):
        if self.shape[0] > 512:
          raise AssertionError(f"whole-matrix densification of {self.shape}")
        return _orig(self, *a, **kw)
      monkeypatch.setattr(cls, name, guarded)


def _big():
  rng = np.random.default_rng(1)
  return sp.random(3000, 400, density=0.1, format="csr", random_state=2, data_rvs=lambda k: rng.integers(1, 9, k)).astype(np.float32)


def test_no_densification_create_dataset(no_densify):
  x = _big()
  s = SingleCellOMIC(x).add_omic("celltype", np.eye(4, dtype=np.float32)[np.arange(3000) % 4])
  tr, va = s.split(0.9)
  tr.corrupt(0.2, 0.2)
  ds = tr.create_dataset(["transcriptomic", "celltype"], labels_percent=0.1, batch_size=64, shuffle=1000)
  assert sp.issparse(ds.arrays[0]) and s.sparsity() > 0.8
  for i, b in enumerate(ds):
    assert b["inputs"][0].shape[0] <= 64
    if i > 3:
      break
  with pytest.raises(AssertionError):
    x.toarray()


def test_no_densification_fit_preparation(no_densify, monkeypatch):
  """The host side of fit on a sparse container, up to the device: the counts reach Engine.upload as CSR (train and validation rows
  joined), by default into the sparse store."""
  import sisua_amd.models as M
  seen = {}

  class Stop(Exception):
    pass

  class FakeEngine:
    max_batch = 64
    world = 1
    step = 0

    def set_train_draws(self, n):
      pass

    def upload(self, X, labels, library, mask, cell_id_base=0, storage="f32"):
      seen.update(X=X, storage=storage, library=library)
      raise Stop()

  x = _big()
  tr, va = SingleCellOMIC(x).split(0.8)
  monkeypatch.setattr(M.SingleCellModel, "_ensure_engine", lambda self, b: FakeEngine())
  # (the default encoder has input dropout, which the sparse store cannot key: the float32 store, filled from the CSR rows on the device)
  for enc, storage in ((M.NetConf([32], batchnorm=True), "csr"), (None, "f32")):
    m = M.VAE(outputs=M.RVmeta(400, "zinb", True, "transcriptomic"), latents=M.RVmeta(6, "diag", True, "Latents"),
              **(dict(encoder=enc) if enc is not None else {}))
    with pytest.raises(Stop):
      m.fit(tr, valid=va, epochs=1, batch_size=64, verbose=False, distributed=False)
    assert sp.issparse(seen["X"]) and seen["X"].shape == (3000, 400) and seen["storage"] == storage
    assert (seen["X"] != sp.vstack([tr.numpy(), va.numpy()])).nnz == 0
    assert np.array_equal(seen["library"][:tr.n_obs], tr.library_size())


def test_csr_symbols_declared_and_exported():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd import _hip
  lib = _hip.load()
  hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sisua_hip.h")).read(), flags=re.S)
  declared = set(re.findall(r"\b(smx_[a-z_0-9]+)\s*\(", hdr))
  for name in ("smx_predict", "smx_predict_stat", "smx_marginal_llk", "smx_dataset_upload_csr", "smx_dataset_upload_csr_dense",
               "smx_pad_audit", "smx_pad_poke"):
    assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name)
