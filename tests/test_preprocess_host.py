"""CPU-side checks of the count-matrix preprocessing (no device): the NumPy restatement (tests/preprocess_ref.py) against pandas and
scikit-learn, sisua_amd/preprocess.py's host functions against the restatement, the argument checks (which must fire before the library is
even loaded), and the container's bookkeeping with the device driver replaced by the restatement."""
import numpy as np
import pytest
import scipy.sparse as sp

from sisua_amd import _hip, preprocess
from sisua_amd.data import SingleCellOMIC
from tests import preprocess_ref as R

# (shape, seed, n_bins, n_top_genes): seeds at which the top-n selection is no near tie (tests/test_gpu_preprocess.py asserts the guards)
CASES = {"seurat": [((300, 96), 2, 5, 24), ((257, 70), 1, 20, 16), ((1000, 200), 11, 20, 50)],
         "cell_ranger": [((300, 96), 16, 5, 24), ((257, 70), 1, 20, 14), ((1000, 200), 28, 20, 50)]}


def _log_matrix(shape, seed):
  return R.normalize(R.counts(*shape, seed), total=True, log1p=True)


def test_counts_family_is_mostly_zeros():
  for shape in ((300, 96), (1000, 200)):
    z = float((R.counts(*shape, 3) == 0).mean())
    assert 0.6 < z < 0.75, z


@pytest.mark.parametrize("n_bins", [5, 20])
def test_restated_bins_equal_pandas_cut(n_bins):
  pd = pytest.importorskip("pandas")
  for shape, seed in (((300, 96), 2), ((257, 70), 1), ((1000, 200), 11)):
    hv = R.highly_variable(R.view(_log_matrix(shape, seed), "expm1"), "seurat", n_bins, 10)
    want = pd.cut(hv["means"], bins=n_bins).codes
    assert np.array_equal(hv["mean_bin"], want)
    assert np.array_equal(preprocess.equal_width_bins(hv["means"], n_bins)[0], want)
  const = np.full(7, 2.5)   # a constant vector: pandas widens the range instead
  assert np.array_equal(preprocess.equal_width_bins(const, n_bins)[0], pd.cut(const, bins=n_bins).codes)
  assert np.array_equal(R.codes_of(const, R.cut_edges(const, n_bins)), pd.cut(const, bins=n_bins).codes)


def test_percentile_bins_equal_pandas_cut():
  pd = pytest.importorskip("pandas")
  hv = R.highly_variable(R.view(_log_matrix((1000, 200), 28), "expm1"), "cell_ranger", 20, 50)
  edges = np.r_[-np.inf, np.percentile(hv["means"], np.arange(10, 105, 5)), np.inf]
  want = pd.cut(hv["means"], edges).codes
  assert np.array_equal(hv["mean_bin"], want)
  assert np.array_equal(preprocess.percentile_bins(hv["means"])[0], want)


def test_restated_scale_equals_standard_scaler():
  skp = pytest.importorskip("sklearn.preprocessing")
  v = _log_matrix((300, 96), 2)
  got, mean, std = R.scale(v)
  n = v.shape[0]
  sk = skp.StandardScaler().fit(v.astype(np.float64))
  np.testing.assert_allclose(mean, sk.mean_, rtol=1e-12, atol=1e-15)
  live = sk.var_ > 0
  np.testing.assert_allclose(std[live], np.sqrt(sk.var_[live] * n / (n - 1)), rtol=1e-10)   # (ddof 0 there, 1 here)
  assert np.all(std[~live] == 1) and (~live).any()   # the all-zero gene
  want = (v.astype(np.float64) - sk.mean_) / np.where(live, np.sqrt(sk.var_ * n / (n - 1)), 1.0)
  np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)   # (float32 arithmetic on float32-rounded moments)
  assert got.dtype == np.float32
  clipped, _, _ = R.scale(v, max_value=1.5)
  assert clipped.max() == np.float32(1.5) and clipped.min() == got.min()   # from above only


@pytest.mark.parametrize("flavor", ["seurat", "cell_ranger"])
def test_host_functions_reproduce_the_restatement(flavor):
  for shape, seed, n_bins, n_top in CASES[flavor]:
    e = R.view(_log_matrix(shape, seed), "expm1")
    want = R.highly_variable(e, flavor, n_bins, n_top)
    st = R.stats(e)
    got = preprocess.highly_variable(st["sum"], st["sumsq"], e.shape[0], flavor, n_bins, n_top)
    np.testing.assert_allclose(got["means"], want["means"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["dispersions"], want["dispersions"], rtol=1e-13, atol=0, equal_nan=True)
    np.testing.assert_allclose(got["dispersions_norm"], want["dispersions_norm"], rtol=0, atol=1e-10, equal_nan=True)
    assert np.array_equal(got["mean_bin"], want["mean_bin"])
    assert np.array_equal(got["highly_variable"], want["highly_variable"]) and got["highly_variable"].sum() == n_top
    cut = preprocess.highly_variable(st["sum"], st["sumsq"], e.shape[0], flavor, n_bins, None, min_disp=0.5, max_disp=3.0, min_mean=0.05,
                                     max_mean=4.0)
    ref = R.highly_variable(e, flavor, n_bins, None, 0.5, 3.0, 0.05, 4.0)
    assert np.array_equal(cut["highly_variable"], ref["highly_variable"]) and 0 < ref["highly_variable"].sum() < e.shape[1]


def test_single_gene_bins_normalise_to_exactly_one():
  shape, seed, n_bins, n_top = CASES["seurat"][1]
  e = R.view(_log_matrix(shape, seed), "expm1")
  st = R.stats(e)
  for hv in (R.highly_variable(e, "seurat", n_bins, n_top), preprocess.highly_variable(st["sum"], st["sumsq"], e.shape[0], "seurat", n_bins, n_top)):
    size = np.bincount(hv["mean_bin"], minlength=n_bins)
    alone = (size[hv["mean_bin"]] == 1) & ~np.isnan(hv["dispersions"])
    assert alone.any() and np.all(hv["dispersions_norm"][alone] == 1.0)


def test_size_factors_and_filters_reproduce_the_restatement():
  x = R.counts(300, 96, 2)
  st = R.stats(x)
  for target in (None, 1e4):
    assert np.array_equal(preprocess.size_factors(st["total"], target), R.size_factors(x, target))
  c = preprocess.size_factors(st["total"])
  assert c.dtype == np.float32 and c[150] == np.float32(1) / np.median(st["total"][st["total"] > 0]).astype(np.float32)   # the empty cell
  masked = R.stats(x, col_mask=R.stats(x, row_thresh=st["total"].astype(np.float32) * np.float32(0.05))["n_above"] == 0)
  assert np.array_equal(preprocess.size_factors(masked["total"]), R.size_factors(x, None, True, 0.05))
  assert np.array_equal(preprocess.keep_by_bound(st["total"], "min_counts", 1), R.filter_cells(x, min_counts=1))
  assert np.array_equal(preprocess.keep_by_bound(st["n_genes"], "max_genes", 30), R.filter_cells(x, max_genes=30))
  assert np.array_equal(preprocess.keep_by_bound(st["n_cells"], "min_cells", 3), R.filter_genes(x, min_cells=3))
  assert np.array_equal(preprocess.keep_by_bound(st["sum"], "max_counts", 100), R.filter_genes(x, max_counts=100))
  mean, std = preprocess.scale_params(st["sum"], st["sumsq"], x.shape[0])
  _, rmean, rstd = R.scale(x)
  assert np.array_equal(mean, rmean.astype(np.float32)) and np.array_equal(std, rstd.astype(np.float32))


# ---- every argument check raises before the library is loaded ----
@pytest.fixture
def no_library(monkeypatch):
  def refuse(*a, **k):
    raise AssertionError("the library was asked for before the arguments were checked")
  monkeypatch.setattr(_hip, "load", refuse)
  monkeypatch.setattr(_hip, "require_gpu", refuse)


def _container(sparse=False, seed=2):
  x = R.counts(60, 40, seed)
  y = np.arange(60 * 3, dtype=np.float32).reshape(60, 3)
  om = SingleCellOMIC(sp.csr_matrix(x) if sparse else x, var_names=[f"g{i}" for i in range(40)], name="toy")
  return om.add_omic("proteomic", y), x


def test_argument_checks_fire_before_the_library(no_library):
  om, x = _container()
  with pytest.raises(ValueError, match="Only provide one"):
    om.filter_cells()
  with pytest.raises(ValueError, match="Only provide one"):
    om.filter_cells(min_counts=1, min_genes=2)
  with pytest.raises(ValueError, match="Only provide one"):
    om.filter_genes(min_cells=1, max_cells=20)
  with pytest.raises(ValueError, match="flavor"):
    om.filter_highly_variable_genes(flavor="svr")
  with pytest.raises(ValueError, match="n_bins"):
    om.filter_highly_variable_genes(n_bins=0)
  with pytest.raises(ValueError, match="n_top_genes"):
    om.filter_highly_variable_genes(n_top_genes=0)
  with pytest.raises(ValueError, match="n_top_genes"):
    om.filter_highly_variable_genes(n_top_genes=2.5)
  with pytest.raises(ValueError, match="target_sum"):
    om.normalize(total=True, target_sum=0)
  with pytest.raises(ValueError, match="max_fraction"):
    om.normalize(total=True, exclude_highly_expressed=True, max_fraction=1.0)
  with pytest.raises(ValueError, match="max_value"):
    om.normalize(scale=True, max_value=float("nan"))
  with pytest.raises(ValueError, match="MAX_GENES"):
    preprocess.filter_genes(sp.csr_matrix((1, preprocess.MAX_GENES + 1), dtype=np.float32), min_cells=1)
  with pytest.raises(ValueError, match="MAX_CELLS"):
    preprocess.check_shape(preprocess.MAX_CELLS + 1, 5)
  with pytest.raises(ValueError, match="at least 2 cells"):
    preprocess.highly_variable_genes(x[:1], n_top_genes=3)
  from sisua_amd import engine
  with pytest.raises(ValueError, match="func"):
    engine.k_prep_stats(x, func="sqrt")
  with pytest.raises(ValueError, match="block_rows"):
    engine.k_prep_stats(x, block_rows=-1)
  with pytest.raises(ValueError, match="row_div"):
    engine.k_prep_apply(x, row_div=np.zeros(60, np.float32))
  with pytest.raises(ValueError, match="expected shape"):
    engine.k_prep_apply(x, row_div=np.ones(59, np.float32))
  with pytest.raises(ValueError, match="col_mask"):
    engine.k_prep_stats(x, col_mask=np.ones(39, np.uint8))
  with pytest.raises(ValueError, match="row_thresh"):
    engine.k_prep_stats(x, row_thresh=np.full(60, np.nan, np.float32))
  with pytest.raises(ValueError, match="mean and std"):
    engine.k_prep_apply(x, mean=np.zeros(40, np.float32))
  assert om.name == "toy" and om.numpy().shape == (60, 40)   # a refusal changes nothing


def test_library_refuses_before_device_work():
  """The C entry points themselves: SMX_ERR_INVALID with a message, on a machine with or without a device"""
  import ctypes as C
  from sisua_amd import build
  build.build(verbose=False)
  lib = _hip.load()
  fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
  assert _hip.SMX_ABI_VERSION >= 11 and "smx_prep.hip" in build.SOURCES
  x, out = np.ones((2, 3), np.float32), np.empty((2, 3), np.float32)
  div0 = np.array([1, 0], np.float32)
  assert lib.smx_prep_apply(fp(x), None, None, None, 2, 3, 0, 7, None, None, None, 0, 0.0, fp(out), None) == -1
  assert b"func" in lib.smx_last_error()
  assert lib.smx_prep_apply(fp(x), None, None, None, 2, 3, 0, 0, fp(div0), None, None, 0, 0.0, fp(out), None) == -1
  assert b"divisor" in lib.smx_last_error()
  assert lib.smx_prep_apply(fp(x), None, None, None, 2, 3, 0, 0, None, None, None, 0, 0.0, fp(out), fp(out)) == -1
  assert lib.smx_prep_apply(fp(x), None, None, None, 2, 3, 0, 0, None, None, None, 0, 0.0, None, fp(out)) == -1   # out_vals needs CSR input
  assert lib.smx_prep_apply(fp(x), None, None, None, 2, 3, -1, 0, None, None, None, 0, 0.0, fp(out), None) == -1
  assert lib.smx_prep_apply(None, None, None, None, 2, 3, 0, 0, None, None, None, 0, 0.0, fp(out), None) == -1
  indptr, cols = np.array([0, 1, 2], np.int64), np.array([0, 3], np.int32)   # column 3 of 3 genes
  vals = np.ones(2, np.float32)
  assert lib.smx_prep_apply(None, indptr.ctypes.data_as(C.POINTER(C.c_int64)), cols.ctypes.data_as(C.POINTER(C.c_int32)), fp(vals), 2, 3, 0, 0,
                            None, None, None, 0, 0.0, fp(out), None) == -1
  assert b"column" in lib.smx_last_error()
  assert lib.smx_prep_stats(fp(x), None, None, None, 2, 3, 0, 0, None, None, None, None, None, None, None, None, None) == -1


# ---- the container, with the device driver replaced by the restatement ----
@pytest.fixture
def host_engine(monkeypatch):
  from sisua_amd import engine

  def dense(x):
    return x.toarray() if sp.issparse(x) else np.asarray(x, np.float32)

  def k_prep_stats(x, func=None, row_div=None, col_mask=None, row_thresh=None, block_rows=0):
    return R.stats(R.view(dense(x), func, row_div), col_mask, row_thresh)

  def k_prep_apply(x, func=None, row_div=None, mean=None, std=None, max_value=None, block_rows=0):
    v = R.view(dense(x), func, row_div)
    if mean is not None:
      v = (v - mean[None, :]) / std[None, :]
    if max_value is not None:
      v[v > max_value] = max_value
    return sp.csr_matrix(v) if (sp.issparse(x) and mean is None and max_value is None) else v
  monkeypatch.setattr(engine, "k_prep_stats", k_prep_stats)
  monkeypatch.setattr(engine, "k_prep_apply", k_prep_apply)


@pytest.mark.parametrize("sparse", [False, True])
def test_container_bookkeeping(host_engine, no_library, sparse):
  om, x = _container(sparse)
  keep_c = R.filter_cells(x, min_counts=1)
  assert not keep_c.all()
  out = om.filter_cells(min_counts=1, inplace=False)
  assert out is not om and om.name == "toy" and om.n_obs == 60 and out.name == "toy_filtercell"
  assert out.n_obs == keep_c.sum() and out.get_omic("proteomic").shape == (keep_c.sum(), 3)   # the cells leave every omic
  assert np.array_equal(out.get_omic("proteomic"), om.get_omic("proteomic")[keep_c])
  assert out.is_sparse() == sparse
  x1 = x[keep_c]
  keep_g = R.filter_genes(x1, min_cells=3)
  assert not keep_g.all()
  same = out.filter_genes(min_cells=3)
  assert same is out and out.name == "toy_filtercell_filtergene" and out.n_vars == keep_g.sum()
  assert list(out.get_var_names("transcriptomic")) == [f"g{i}" for i in np.flatnonzero(keep_g)]
  assert out.get_dim("proteomic") == 3 and len(out.get_var_names("proteomic")) == 3   # the genes leave the filtered omic only
  x2 = x1[:, keep_g]
  out.normalize(total=True, log1p=True)
  assert out.name.endswith("_filtergene_total_log1p") and out.is_sparse() == sparse
  want = R.normalize(x2, total=True, log1p=True)
  got = out.numpy().toarray() if sparse else out.numpy()
  assert np.array_equal(got, want)
  hv = out.filter_highly_variable_genes(n_top_genes=0.25, n_bins=5, inplace=False)
  ref = R.highly_variable(R.view(want, "expm1"), "seurat", 5, 0.25)
  assert hv.name.endswith("_vargene") and not out.name.endswith("_vargene")
  assert np.array_equal(hv.highly_variable_features["highly_variable"], ref["highly_variable"])
  assert set(hv.highly_variable_features) == {"highly_variable", "means", "dispersions", "dispersions_norm"}
  assert hv.n_vars == ref["highly_variable"].sum() >= int(0.25 * x2.shape[1])
  assert list(hv.get_var_names("transcriptomic")) == list(out.get_var_names("transcriptomic")[ref["highly_variable"]])
  back = hv.expm1(inplace=False)
  assert back is not hv and back.name == hv.name   # (the reference's expm1 adds no suffix)
  sc = out.normalize(scale=True, max_value=2.0, inplace=False)
  assert sc.name.endswith("_log1p_scale") and not sc.is_sparse() and sc.numpy().max() <= 2.0 and sc.numpy().min() < -0.1
  assert np.array_equal(sc.numpy(), R.scale(want, 2.0)[0])
  assert out.normalize(inplace=False).name == out.name   # nothing asked: nothing changes
  ds = hv.create_dataset(batch_size=16)   # a filtered container still feeds fit / predict
  assert ds.n_obs == hv.n_obs and ds.arrays[0].shape == (hv.n_obs, hv.n_vars) and ds.library.shape == (hv.n_obs, 2)
  assert sum(len(b) for b in ds.epoch_batches(0)) == hv.n_obs


def test_product_does_not_import_pandas():
  import subprocess
  import sys
  code = "import sys; import sisua_amd.preprocess, sisua_amd.data; assert 'pandas' not in sys.modules and 'scanpy' not in sys.modules"
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  subprocess.run([sys.executable, "-c", code], check=True, cwd=root)
