"""Count-matrix preprocessing on the device (smx_prep.hip through engine.k_prep_stats / k_prep_apply and SingleCellOMIC's methods) against
the NumPy restatement tests/preprocess_ref.py.

Shapes: ragged rows and columns, more than one tile of 256 genes (1030), one row (1, 33); block_rows 64 cuts every shape but the last
two into several blocks, 0 leaves one.  Every matrix has an all-zero cell and an all-zero gene (the one-row shape: the gene only).

Bounds.  Sums of non-negative float64 terms in two orders differ by at most 2 N 2^-53 relative (N <= 1024: 2.3e-13), so 1e-12 holds
the sums; counts are integers and EQUAL.  Division, subtraction and the clip are IEEE float32 operations: BITS.  log1pf / expm1f are the
device library's: the largest distance from the correctly rounded result over these inputs was measured as 1 ulp for both (DESIGN.md
section 4q); the test allows the measured value plus one and never more than 4 (OpenCL's full-profile bound for expm1 is 3 ulp)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from sisua_amd import engine, preprocess
from sisua_amd.data import SingleCellOMIC
from tests import preprocess_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(300, 96), (257, 70), (1000, 200), (64, 1030), (1, 33)]
SEEDS = {(300, 96): 2, (257, 70): 1, (1000, 200): 11, (64, 1030): 4, (1, 33): 5}
VIEWS = [(None, False), (None, True), ("log1p", False), ("log1p", True), ("expm1", False), ("expm1", True)]
MEASURED_ULP = {"log1p": 1, "expm1": 1}   # the largest distance seen on the device over the inputs of test_apply_log1p_expm1_ulp
ULP_CAP = 4
# (shape, seed, n_bins, n_top_genes) per flavour: seeds picked on the CPU so that both guards of test_variable_genes hold with room
HVG_CASES = {"seurat": [((300, 96), 2, 5, 24), ((257, 70), 1, 20, 16), ((1000, 200), 11, 20, 50), ((64, 1030), 4, 20, 100)],
             "cell_ranger": [((300, 96), 16, 5, 24), ((257, 70), 1, 20, 14), ((1000, 200), 28, 20, 50), ((64, 1030), 388, 20, 80)]}
E2E_SEED = 10


@functools.lru_cache(maxsize=None)
def _data(shape, seed):
  """counts x, their size factors c, the log-normalised matrix L (the input of the expm1 views: expm1f of a raw count overflows), its
  own factors cl -- computed once and shared; nobody writes to them"""
  x = R.counts(*shape, seed)
  c = R.size_factors(x)
  L = R.normalize(x, total=True, log1p=True)
  out = dict(x=x, c=c, L=L, cl=R.size_factors(L))
  for a in out.values():
    a.setflags(write=False)
  return out


def _view_input(shape, func, div):
  d = _data(shape, SEEDS[shape])
  return (d["L"], d["cl"] if div else None) if func == "expm1" else (d["x"], d["c"] if div else None)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
  if isinstance(a, dict):
    return set(a) == set(b) and all(_same_bits(a[k], b[k]) for k in a)
  return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _dense(m):
  return m.toarray() if sp.issparse(m) else m


@pytest.mark.parametrize("block_rows", [64, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_stats_identity_view(shape, block_rows):
  x = _data(shape, SEEDS[shape])["x"]
  N, G = shape
  mask = (np.arange(G) % 3 != 1).astype(np.uint8)
  thr = (R.stats(x)["total"].astype(np.float32) * np.float32(0.05)).astype(np.float32)
  got = engine.k_prep_stats(x, col_mask=mask, row_thresh=thr, block_rows=block_rows)
  want = R.stats(x, col_mask=mask, row_thresh=thr)
  if N > 2:
    assert (want["n_genes"] == 0).any()   # the all-zero cell
  assert (want["n_cells"] == 0).any()     # the all-zero gene
  for k in ("sum", "sumsq", "total"):
    print(shape, block_rows, k, "max rel", float(np.max(np.abs(got[k] - want[k]) / np.maximum(want[k], 1e-300))))
    np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0)
    assert np.all(got[k][want[k] == 0] == 0)
  for k in ("n_genes", "n_cells", "n_above"):
    assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
  L = _data(shape, SEEDS[shape])["L"]   # non-integer values: the order of the sums shows in the last bits
  got, want = engine.k_prep_stats(L, block_rows=block_rows), R.stats(L)
  for k in ("sum", "sumsq", "total"):
    print(shape, block_rows, "log matrix", k, "max rel", float(np.max(np.abs(got[k] - want[k]) / np.maximum(want[k], 1e-300))))
    np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0)
    assert np.all(got[k][want[k] == 0] == 0)
  assert np.array_equal(got["n_genes"], want["n_genes"]) and np.array_equal(got["n_cells"], want["n_cells"])
  plain = engine.k_prep_stats(x, block_rows=block_rows)
  np.testing.assert_allclose(plain["total"], R.stats(x)["total"], rtol=1e-12, atol=0)
  assert "n_above" not in plain


@pytest.mark.parametrize("func,div", VIEWS)
@pytest.mark.parametrize("shape", SHAPES)
def test_stats_same_bits(shape, func, div):
  """dense against CSR, block_rows 64 against 0, two calls, and the view of X against the identity view of apply(view, X)"""
  m, c = _view_input(shape, func, div)
  base = engine.k_prep_stats(m, func=func, row_div=c)
  assert np.isfinite(base["sum"]).all() and np.isfinite(base["sumsq"]).all() and base["sum"].max() > 0
  assert _same_bits(base, engine.k_prep_stats(m, func=func, row_div=c)), "two calls"
  assert _same_bits(base, engine.k_prep_stats(m, func=func, row_div=c, block_rows=64)), "block_rows"
  csr = sp.csr_matrix(m)
  assert _same_bits(base, engine.k_prep_stats(csr, func=func, row_div=c)), "CSR"
  assert _same_bits(base, engine.k_prep_stats(csr, func=func, row_div=c, block_rows=64)), "CSR, block_rows"
  made = engine.k_prep_apply(m, func=func, row_div=c, block_rows=64)
  assert _same_bits(base, engine.k_prep_stats(made)), "identity view of the applied matrix"
  assert _same_bits(base, engine.k_prep_stats(engine.k_prep_apply(csr, func=func, row_div=c), block_rows=64)), "... of the applied CSR"


@pytest.mark.parametrize("func,div", VIEWS)
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_same_bits(shape, func, div):
  m, c = _view_input(shape, func, div)
  G = shape[1]
  mean = np.linspace(-0.5, 1.5, G).astype(np.float32)
  std = np.linspace(0.25, 3.0, G).astype(np.float32)
  csr = sp.csr_matrix(m)
  base = engine.k_prep_apply(m, func=func, row_div=c)
  assert base.dtype == np.float32 and base.shape == m.shape
  assert _same_bits(base, engine.k_prep_apply(m, func=func, row_div=c)), "two calls"
  assert _same_bits(base, engine.k_prep_apply(m, func=func, row_div=c, block_rows=64)), "block_rows"
  for br in (0, 64):
    out = engine.k_prep_apply(csr, func=func, row_div=c, block_rows=br)
    assert sp.issparse(out) and np.array_equal(out.indptr, csr.indptr) and np.array_equal(out.indices, csr.indices)   # sparse stays sparse
    assert _same_bits(base, out.toarray()), "CSR"
  scaled = engine.k_prep_apply(m, func=func, row_div=c, mean=mean, std=std, max_value=1.25)
  assert scaled.max() == np.float32(1.25) and scaled.min() < 0
  assert _same_bits(scaled, engine.k_prep_apply(m, func=func, row_div=c, mean=mean, std=std, max_value=1.25, block_rows=64))
  for br in (0, 64):
    out = engine.k_prep_apply(csr, func=func, row_div=c, mean=mean, std=std, max_value=1.25, block_rows=br)
    assert not sp.issparse(out) and _same_bits(scaled, out), "centred output of CSR input is dense"
  want = (base - mean[None, :]) / std[None, :]   # centring and clip of the device's own view values: float32 IEEE operations, BITS
  want[want > np.float32(1.25)] = np.float32(1.25)
  assert _same_bits(scaled, want)


@pytest.mark.parametrize("shape", SHAPES)
def test_apply_division_subtraction_clip_bits(shape):
  """A view made of division, subtraction and clip only has the restatement's bits"""
  d = _data(shape, SEEDS[shape])
  x, c = d["x"], d["c"]
  assert _same_bits(engine.k_prep_apply(x, row_div=c, block_rows=64), R.view(x, None, c))
  assert _same_bits(engine.k_prep_apply(x), x.copy())
  mean, std = (x.mean(axis=0) / 2).astype(np.float32), (1 + x.std(axis=0)).astype(np.float32)
  want = (R.view(x, None, c) - mean[None, :]) / std[None, :]
  want[want > np.float32(0.75)] = np.float32(0.75)
  assert _same_bits(engine.k_prep_apply(x, row_div=c, mean=mean, std=std, max_value=0.75), want)
  assert _same_bits(engine.k_prep_apply(sp.csr_matrix(x), row_div=c, mean=mean, std=std, max_value=0.75, block_rows=64), want)
  if shape[0] > 1:   # scale end to end: the moments from the device's statistics of the view
    got = preprocess.apply_view(x, row_div=c, scale=True, max_value=3.0)
    ref, _, _ = R.scale(R.view(x, None, c), 3.0)
    st = engine.k_prep_stats(x, row_div=c)
    rs = R.stats(R.view(x, None, c))
    if _same_bits(st["sum"], rs["sum"]) and _same_bits(st["sumsq"], rs["sumsq"]):
      assert _same_bits(got, ref)
    else:   # float64 sums in another order: moments within 1e-12, float32 results within a few ulp of O(1) values
      np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)
    assert got.max() <= 3.0 and np.isfinite(got).all()


@pytest.mark.parametrize("func", ["log1p", "expm1"])
def test_apply_log1p_expm1_ulp(func):
  worst = 0
  for shape in SHAPES:
    for div in (False, True):
      m, c = _view_input(shape, func, div)
      got = engine.k_prep_apply(m, func=func, row_div=c)
      want = R.exact(func)(R.view_argument(m, c))   # the float64 function of the same float32 argument, rounded to float32
      assert np.isfinite(want).all()
      worst = max(worst, int(R.ulp_distance(got, want).max()))
      assert np.all(got[R.view_argument(m, c) == 0] == 0)
  print(f"{func}: largest distance from the correctly rounded float32 result: {worst} ulp")
  assert worst <= min(MEASURED_ULP[func] + 1, ULP_CAP)


def _inner_edges(edges, flavor):
  """The edges a mean could cross: not the lowest (below every mean) nor the highest finite one (the largest mean itself)"""
  return edges[1:-1] if flavor == "seurat" else edges[1:-2]


@pytest.mark.parametrize("flavor", ["seurat", "cell_ranger"])
@pytest.mark.parametrize("case", range(4))
def test_variable_genes(flavor, case):
  shape, seed, n_bins, n_top = HVG_CASES[flavor][case]
  L = _data(shape, seed)["L"]
  e = engine.k_prep_apply(L, func="expm1")   # the restatement is fed the device's own expm1 matrix
  want = R.highly_variable(e, flavor, n_bins, n_top)
  gap = R.top_gap(want["dispersions_norm"], n_top)
  dist = np.abs(want["means"][:, None] - _inner_edges(want["edges"], flavor)[None, :])
  if flavor == "cell_ranger":
    dist = dist[dist > 0]   # a percentile at a whole rank IS one of the means, on both sides alike (right-closed: it stays below its edge)
  margin = dist.min() / (want["means"].max() - want["means"].min())
  print(shape, flavor, "gap", float(gap), "edge margin", float(margin))
  assert gap >= 1e-3 and margin >= 1e-6, "the case is a near tie: pick another seed"
  for sparse in (False, True):
    got = preprocess.highly_variable_genes(sp.csr_matrix(L) if sparse else L, n_top_genes=n_top, n_bins=n_bins, flavor=flavor)
    np.testing.assert_allclose(got["means"], want["means"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(got["dispersions"], want["dispersions"], rtol=1e-10, atol=1e-10, equal_nan=True)
    assert np.array_equal(np.isnan(got["dispersions_norm"]), np.isnan(want["dispersions_norm"]))
    np.testing.assert_allclose(got["dispersions_norm"], want["dispersions_norm"], rtol=0, atol=1e-9, equal_nan=True)
    assert np.array_equal(got["mean_bin"], want["mean_bin"])
    assert np.array_equal(got["highly_variable"], want["highly_variable"]) and got["highly_variable"].sum() == n_top
    if flavor == "seurat":
      size = np.bincount(want["mean_bin"], minlength=n_bins)
      alone = (size[want["mean_bin"]] == 1) & ~np.isnan(want["dispersions"])
      if (shape, n_bins) == ((257, 70), 20):
        assert alone.any()   # the matrix whose bins include single-gene bins
      assert np.all(got["dispersions_norm"][alone] == 1.0)
  cut = preprocess.highly_variable_genes(L, n_top_genes=None, n_bins=n_bins, flavor=flavor, min_disp=0.5, max_disp=3.0, min_mean=0.05, max_mean=4.0)
  ref = R.highly_variable(e, flavor, n_bins, None, 0.5, 3.0, 0.05, 4.0)
  z = np.nan_to_num(ref["dispersions_norm"])
  near = min(np.abs(z - 0.5).min(), np.abs(z - 3.0).min(), np.abs(ref["means"] - 0.05).min(), np.abs(ref["means"] - 4.0).min())
  if near > 1e-8:   # (no gene sits on a cut-off)
    assert np.array_equal(cut["highly_variable"], ref["highly_variable"])


def _chain(om):
  return (om.filter_cells(min_counts=1).filter_genes(min_cells=3).normalize(total=True, log1p=True)
          .filter_highly_variable_genes(n_top_genes=50))


def test_end_to_end_dense_and_sparse():
  x = _data((1000, 200), E2E_SEED)["x"]
  want = R.chain(x, 50, 20)
  assert R.top_gap(want["hv"]["dispersions_norm"], 50) >= 1e-3
  names = np.array([f"gene{i}" for i in range(200)])
  y = np.arange(1000 * 4, dtype=np.float32).reshape(1000, 4)
  outs = []
  for m in (x.copy(), sp.csr_matrix(x)):
    om = SingleCellOMIC(m, var_names=names, name="e2e").add_omic("proteomic", y)
    out = _chain(om)
    assert out is om and om.name == "e2e_filtercell_filtergene_total_log1p_vargene"
    assert list(om.get_var_names("transcriptomic")) == list(names[want["genes"]])   # the gene set is the restatement's
    assert np.array_equal(om.get_omic("proteomic"), y[want["cells"]])
    assert om.is_sparse() == sp.issparse(m) and om.numpy().shape == (len(want["cells"]), 50)
    outs.append(om)
  a, b = _dense(outs[0].numpy()), _dense(outs[1].numpy())
  assert _same_bits(a, b)   # dense and sparse containers: the same bits
  for k, v in outs[0].highly_variable_features.items():
    assert _same_bits(v, outs[1].highly_variable_features[k]), k
  assert R.ulp_distance(a, want["x"]).max() <= min(MEASURED_ULP["log1p"] + 1, ULP_CAP)
  ds = outs[1].create_dataset(batch_size=64)
  assert ds.n_obs == len(want["cells"]) and ds.arrays[0].shape[1] == 50


def test_exclude_highly_expressed_and_target_sum():
  x = _data((300, 96), SEEDS[(300, 96)])["x"]
  for kw in (dict(target_sum=1e4), dict(exclude_highly_expressed=True, max_fraction=0.05), dict(exclude_highly_expressed=True, max_fraction=0.2, target_sum=50)):
    c = preprocess.total_size_factors(x, **kw)
    assert _same_bits(c, R.size_factors(x, **kw))
    assert _same_bits(c, preprocess.total_size_factors(sp.csr_matrix(x), **kw))
  om = SingleCellOMIC(x.copy()).normalize(total=True, exclude_highly_expressed=True, max_fraction=0.2, target_sum=50)
  assert _same_bits(om.numpy(), R.normalize(x, total=True, exclude_highly_expressed=True, max_fraction=0.2, target_sum=50))
  assert om.name.endswith("_total")


def test_limits_raise_value_error_naming_the_limit():
  x = _data((300, 96), SEEDS[(300, 96)])["x"]
  om = SingleCellOMIC(x.copy())
  wide = SingleCellOMIC(sp.csr_matrix((2, preprocess.MAX_GENES + 1), dtype=np.float32))
  with pytest.raises(ValueError, match=r"2\^20 \(MAX_GENES\)"):
    wide.filter_genes(min_cells=1)
  with pytest.raises(ValueError, match=r"2\^20 \(MAX_GENES\)"):
    wide.normalize(log1p=True)
  with pytest.raises(ValueError, match=r"2\^31 - 1 \(MAX_CELLS\)"):
    preprocess.check_shape(2 ** 31, 10)
  with pytest.raises(ValueError, match=r"n_cells >= 2"):
    SingleCellOMIC(x[:1].copy()).filter_highly_variable_genes(n_top_genes=5)
  with pytest.raises(ValueError, match=r"n_cells >= 2"):
    SingleCellOMIC(x[:1].copy()).normalize(scale=True)
  with pytest.raises(ValueError, match=r"n_top_genes.*>= 1"):
    om.filter_highly_variable_genes(n_top_genes=0)
  with pytest.raises(ValueError, match=r"n_bins.*>= 1"):
    om.filter_highly_variable_genes(n_bins=0)
  with pytest.raises(ValueError, match=r"target_sum.*> 0"):
    om.normalize(total=True, target_sum=-1)
  with pytest.raises(ValueError, match=r"max_fraction.*\(0, 1\)"):
    om.normalize(total=True, exclude_highly_expressed=True, max_fraction=0)
  with pytest.raises(ValueError, match=r"block_rows must be >= 0"):
    engine.k_prep_stats(x, block_rows=-64)
  assert om.name == "scOMICS" and _same_bits(om.numpy(), x)
