"""Gene x protein correlation matrices on the device (smx_correlate.hip): the column ranks against scipy.stats.rankdata (equal integers),
the integer sums against NumPy int64 (equal), Pearson against scipy.stats.pearsonr on the float64 casts, fitted models against the
reference's per-pair SciPy calls on the device's own mean (tests/correlation_ref.py), invariance to batching / input form / gene chunking /
the form of the extras, and the edges.

Tolerance of the Pearson comparisons, 1e-9: a two-pass centred float64 sum of N <= 20001 terms has relative error of order N 2^-53, about
2e-12; the bound leaves more than 100 x over that.  The finite non-constant test columns have std / |mean| >= 1e-3, so centring does not
amplify the error."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import correlation_ref as R
from tests.util import synth_counts, synth_labels

pytestmark = pytest.mark.gpu

N, G = 300, 120
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 20001]   # one form for every N: 20001 x 8 bytes is more than a CU's LDS
N_FINITE = 14   # of the 16 columns of _columns


@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


_COLS = {}


def _columns(n):
  """(cols [16, n] float32, rank2 of the 14 finite ones by SciPy): made once per n"""
  if n not in _COLS:
    rng = np.random.default_rng(n)
    cols = [rng.normal(size=n) * 10.0 ** rng.integers(-30, 31, size=n) for _ in range(6)]               # 60 decades, both signs
    cols += [rng.integers(0, 3, size=n).astype(np.float64) for _ in range(3)]                            # counts 0..2: long tie runs
    cols += [np.full(n, -3.5)]                                                                           # all equal
    cols += [np.where(rng.uniform(size=n) < 0.5, 0.0, -0.0) for _ in range(2)]                           # +0 / -0 mixed
    cols += [rng.integers(-2, 3, size=n) * np.float64(1e-42), rng.integers(1, 9, size=n) * np.float64(3e-45)]   # denormals
    nan, inf = rng.normal(size=n), rng.normal(size=n)
    nan[rng.integers(n)], inf[rng.integers(n)] = np.nan, -np.inf if n % 2 else np.inf
    c = np.stack(cols + [nan, inf]).astype(np.float32)
    c.setflags(write=False)
    want = np.stack([R.rank2(col) for col in c[:N_FINITE]])
    want.setflags(write=False)
    _COLS[n] = (c, want)
  return _COLS[n]


# ---- 1. kernel: ranks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_col_rank2_is_rankdata(api, n):
  from sisua_amd.engine import k_col_rank2
  cols, want = _columns(n)
  rank2, nonfinite = k_col_rank2(cols)
  assert rank2.dtype == np.int32 and rank2.shape == cols.shape
  assert list(nonfinite) == [0] * N_FINITE + [1, 1]
  for j in range(N_FINITE):
    assert np.array_equal(rank2[j], want[j]), (n, j)


# ---- 2. kernel: sums -----------------------------------------------------------------------------------------------------------
def _proteins(n, P, seed=0):
  """Poisson counts; with more than one column the last is constant"""
  rng = np.random.default_rng(1000 * P + n + seed)
  prot = rng.poisson(rng.uniform(1.0, 30.0, size=P), size=(n, P)).astype(np.float64)
  if P > 1:
    prot[:, -1] = 4.0
  return prot


@pytest.mark.parametrize("P", [1, 9, 33])
@pytest.mark.parametrize("n", SIZES)
def test_col_correlate_sums(api, n, P):
  from sisua_amd.distributions import correlations_from_sums, protein_operands
  from sisua_amd.engine import k_col_correlate
  cols, _ = _columns(n)
  prot = _proteins(n, P)
  ops = protein_operands(prot)
  got = k_col_correlate(cols, ops["rank2"], ops["unit"])
  want = R.numpy_sums(cols[:N_FINITE], prot)
  assert list(got["nonfinite"]) == [0] * N_FINITE + [1, 1]
  for k in ("sp_Sa", "sp_Saa", "sp_Sab"):
    assert got[k].dtype == np.int64 and np.array_equal(got[k][:N_FINITE], want[k]), (k, n, P)
  assert ops["Sb"] == want["sp_Sb"] and ops["Sbb"] == want["sp_Sbb"]
  res = correlations_from_sums(n, got["sp_Sa"], got["sp_Saa"], got["sp_Sab"], ops["Sb"], ops["Sbb"], got["pe_Sxx"], got["pe_Sxy"],
                               got["nonfinite"], ops["constant"])
  pe, spm = R.pair_matrices(cols[:N_FINITE].T.astype(np.float64), prot)
  assert np.isnan(res["pearson"][N_FINITE:]).all() and np.isnan(res["spearman"][N_FINITE:]).all()   # the NaN and the inf column
  for key, ref in (("pearson", pe), ("spearman", spm)):
    g = res[key][:N_FINITE]
    assert np.array_equal(np.isnan(g), np.isnan(ref)), (key, n, P)
    ok = ~np.isnan(ref)
    delta = float(np.abs(g[ok] - ref[ok]).max()) if ok.any() else 0.0
    print(f"N={n} P={P} {key}: max |delta| {delta:.3e} over {int(ok.sum())} pairs")
    assert delta <= 1e-9, (key, n, P, delta)
  if n == 1:
    assert np.isnan(res["pearson"]).all() and np.isnan(res["spearman"]).all()
  if P > 1 and n > 2:
    assert np.isnan(res["pearson"][:, -1]).all() and np.isfinite(res["pearson"][:9, 0]).all()


# ---- fitted models -------------------------------------------------------------------------------------------------------------
KINDS = {"vae_zinb": ("vae", "zinb"), "vae_nb": ("vae", "nb"), "vae_normal": ("vae", "normal"), "scvi_zinbd": ("scvi", "zinbd"),
         "sisua_nb": ("sisua", "nb"), "dca_zinb": ("dca", "zinb")}
_FITTED = {}


def _extras():
  return synth_labels(N, ((9, "nb"),))[0].astype(np.float64)


def fitted(api, kind):
  if kind in _FITTED:
    return _FITTED[kind]
  from sisua_amd.data import SingleCellOMIC
  from tests.output_kinds_ref import synth_continuous
  model, llk = KINDS[kind]
  x = synth_continuous(N, G, seed=7) if llk == "normal" else synth_counts(N, G, sparsity=0.8, seed=3)
  lat = api.RVmeta(8, "diag", True, "Latents")
  net = dict(encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  sco = SingleCellOMIC(x, name="toy")
  if model == "sisua":
    sco.add_omic("proteomic", synth_labels(N, ((9, "nb"),))[0])
    m = api.SISUA(outputs=sco.get_rv("transcriptomic", llk), labels=[api.RVmeta(9, "nb", True, "proteomic")], latents=lat, **net)
    m.fit(sco, epochs=3, batch_size=64, verbose=False)
  else:
    if model == "scvi":
      m = api.SCVI(outputs=sco.get_rv("transcriptomic", llk), latents=lat, **net)
    elif model == "dca":
      m = api.DeepCountAutoencoder(outputs=sco.get_rv("transcriptomic", llk), **net)
    elif llk == "normal":
      m = api.VAE(outputs=api.RVmeta(G, "normal", name="transcriptomic"), latents=lat, **net)
    else:
      m = api.VAE(outputs=sco.get_rv("transcriptomic", llk), latents=lat, **net)
    m.fit(sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True), metadata=sco, epochs=3, learning_rate=2e-3)
  _FITTED[kind] = (m, x)
  return _FITTED[kind]


def _handle(m, x, S, batch_size=50):
  h = m._imputation_handle(x, None, S, batch_size)
  return h.count_distribution if h.is_zero_inflated else h


def _same(a, b):
  """the same bits, NaN where NaN"""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _same_result(a, b):
  return set(a) == set(b) == {"pearson", "spearman"} and _same(a["pearson"], b["pearson"]) and _same(a["spearman"], b["spearman"])


# ---- 3. fitted models ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("kind", ["vae_zinb", "vae_nb", "vae_normal", "scvi_zinbd", "sisua_nb"])
def test_model_correlation_is_scipy_on_the_device_mean(api, kind, S):
  from sisua_amd.distributions import protein_operands
  m, x = fitted(api, kind)
  extras = _extras()
  got = m.correlation(x, extras, sample_shape=S, batch_size=50)
  assert got["pearson"].shape == (G, 9) and got["spearman"].shape == (G, 9) and got["pearson"].dtype == np.float64
  h = _handle(m, x, S)
  mean = h.mean_over_samples()
  assert mean.shape == (N, G) and mean.dtype == np.float32
  if kind == "vae_normal":
    assert (mean < 0).any()
  # Spearman through the exact integer sums; the final values against the per-pair SciPy calls
  ops = protein_operands(extras)
  sums, want = h.correlation_sums(ops), R.numpy_sums(mean.T, extras)
  for k in ("sp_Sa", "sp_Saa", "sp_Sab"):
    assert np.array_equal(sums[k], want[k]), (kind, S, k)
  assert not sums["nonfinite"].any()
  pe, spm = R.pair_matrices(mean.astype(np.float64), extras)
  for key, ref in (("pearson", pe), ("spearman", spm)):
    assert np.array_equal(np.isnan(got[key]), np.isnan(ref)) and np.isfinite(ref).sum() > G
    ok = ~np.isnan(ref)
    delta = float(np.abs(got[key][ok] - ref[ok]).max())
    print(f"{kind} S={S} {key}: max |delta| {delta:.3e}")
    assert delta <= 1e-9, (kind, S, key, delta)
  idx = [5, 5, 119, 0]
  sub = m.correlation(x, extras, sample_shape=S, batch_size=50, genes=idx)
  assert _same(sub["pearson"], got["pearson"][idx]) and _same(sub["spearman"], got["spearman"][idx])


# ---- 4. invariance -----------------------------------------------------------------------------------------------------------------
def test_invariance_to_batching_forms_and_gene_chunks(api):
  """Batch sizes on a model with deterministic latents (a cell's planes do not depend on its minibatch; with a stochastic posterior a
  cell's noise id is its index within the minibatch, so other batch sizes are other draws); input form, gene chunking, staging chunks and
  the form of the extras on that model and on a stochastic one with several draws."""
  from sisua_amd import _hip
  extras = _extras()
  m, x = fitted(api, "dca_zinb")
  ref = m.correlation(x, extras, sample_shape=1, batch_size=50)
  assert np.isfinite(ref["pearson"]).sum() > G
  try:
    for keep in (None, 7 * 16.0 * N, 1e18):   # the default; 7 genes per chunk (18 walks); "everything fits"
      if keep is not None:
        _hip.set_tuning("correlate_keep_bytes", keep)
      for bs in (8, 64, 512):
        assert _same_result(m.correlation(x, extras, sample_shape=1, batch_size=bs), ref), (keep, bs)
      assert _same_result(m.correlation(sp.csr_matrix(x), extras, sample_shape=1, batch_size=50), ref), keep
      assert _same_result(m.correlation(x, sp.csr_matrix(extras), sample_shape=1, batch_size=50), ref), keep
    _hip.set_tuning("predict_stage_floats", 40000.0)   # several staging chunks of the walk
    assert _same_result(m.correlation(x, extras, sample_shape=1, batch_size=50), ref)
  finally:
    _hip.clear_tuning("")
  m2, x2 = fitted(api, "vae_zinb")
  ref = m2.correlation(x2, extras, sample_shape=3, batch_size=50)
  try:
    for keep in (7 * 16.0 * N, 1e18):
      _hip.set_tuning("correlate_keep_bytes", keep)
      _hip.set_tuning("predict_stage_floats", 40000.0)
      assert _same_result(m2.correlation(x2, extras, sample_shape=3, batch_size=50), ref), keep
      assert _same_result(m2.correlation(sp.csr_matrix(x2), sp.csr_matrix(extras), sample_shape=3, batch_size=50), ref), keep
      _hip.clear_tuning("")
  finally:
    _hip.clear_tuning("")


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------
def test_constant_gene_constant_protein_and_one_cell(api):
  from sisua_amd.distributions import correlations_from_sums, protein_operands
  from sisua_amd.engine import k_col_correlate
  rng = np.random.default_rng(4)
  cols = rng.gamma(2.0, 2.0, size=(5, 777)).astype(np.float32)
  cols[2] = np.float32(0.1)   # a gene whose mean is the same in every cell
  prot = _proteins(777, 4)
  ops = protein_operands(prot)
  r = k_col_correlate(cols, ops["rank2"], ops["unit"])
  assert r["pe_Sxx"][2] == 0.0 and r["pe_mean"][2] == np.float64(np.float32(0.1))   # (the float64 sum of N equal float32 is exact)
  res = correlations_from_sums(777, r["sp_Sa"], r["sp_Saa"], r["sp_Sab"], ops["Sb"], ops["Sbb"], r["pe_Sxx"], r["pe_Sxy"], r["nonfinite"], ops["constant"])
  for key in ("pearson", "spearman"):
    want = np.zeros((5, 4), bool)
    want[2], want[:, 3] = True, True
    assert np.array_equal(np.isnan(res[key]), want), key
  # a fitted model: a constant protein gives a NaN column; one cell gives all NaN
  m, x = fitted(api, "vae_nb")
  ex = _extras()
  ex[:, 4] = 2.0
  got = m.correlation(x, ex, sample_shape=1, batch_size=50)
  for key in ("pearson", "spearman"):
    assert np.isnan(got[key][:, 4]).all() and np.isfinite(np.delete(got[key], 4, axis=1)).all()
  one = m.correlation(x[:1], ex[:1], sample_shape=1, batch_size=50)
  assert one["pearson"].shape == (G, 9) and np.isnan(one["pearson"]).all() and np.isnan(one["spearman"]).all()


def test_argument_errors(api):
  from sisua_amd import _hip
  from sisua_amd.config import ModelConfig
  from sisua_amd.engine import Engine, k_col_rank2
  m, x = fitted(api, "vae_nb")
  ex = _extras()
  bad = ex.copy()
  bad[3, 2] = np.nan
  with pytest.raises(ValueError):
    m.correlation(x, bad)
  with pytest.raises(ValueError):
    m.correlation(x, ex[:-1])
  with pytest.raises(IndexError):
    m.correlation(x, ex, genes=[0, G])
  # more than 2^20 cells: refused with an error code before any device work
  n_big = (1 << 20) + 1
  e = Engine(ModelConfig(model="vae", n_genes=4, likelihood="nb", enc_units=(8,), dec_units=(8,), latent_dim=2), max_batch=64)
  try:
    with pytest.raises(_hip.SmxError) as err:
      e.predict_correlate(np.zeros((n_big, 4), np.float32), np.full((1, n_big), 2, np.int32), np.zeros((1, n_big)))
    assert err.value.code != 0 and "2^20" in str(err.value)
  finally:
    e.close()
  with pytest.raises(_hip.SmxError):
    k_col_rank2(np.zeros((1, n_big), np.float32))
