"""Imputation scores reduced on the device (smx_impute.hip): the row selection against np.partition bit for bit, the scores as exact
functions of the device's own mean (tests/imputation_ref.py, which tests/test_imputation_host.py ties to the reference's functions), the
float64 oracle within the movement of the mean, invariance to batching / chunking / input form / second-pass form, the column gather."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import imputation_ref as R
from tests.util import make_pair, perturbed_params, synth_counts, synth_labels

pytestmark = pytest.mark.gpu

N, G = 300, 120


@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
  """bit for bit, any NaN standing for any NaN"""
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- 2. kernel level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 2, 31, 32, 33, 1998, 2000, 4097, 20000])
def test_row_select_is_np_partition(api, g):
  from sisua_amd.engine import k_row_select
  rng = np.random.default_rng(g)
  rows = [np.abs(rng.normal(size=g)) * 10.0 ** rng.integers(-30, 30, size=g) for _ in range(6)]      # random, 60 decades
  rows += [rng.integers(0, 3, size=g).astype(np.float64) for _ in range(4)]                            # ties
  rows += [np.zeros(g), np.where(rng.uniform(size=g) < 0.5, 0.0, -0.0)]                                # all zero, +0 / -0
  rows += [rng.integers(0, 2, size=g) * np.float64(1e-42), np.where(rng.uniform(size=g) < 0.5, np.inf, rng.uniform(size=g))]   # denormals, inf
  rows += [np.where(rng.uniform(size=g) < 0.3, np.nan, rng.uniform(size=g)), np.full(g, np.nan), np.full(g, 7.25)]            # NaN rows, one value
  x = np.stack(rows).astype(np.float32)
  for ld in (g, g + 7):
    buf = np.full((x.shape[0], ld), np.nan, np.float32)   # garbage beyond G: NaN and negative values
    buf[:, g::2] = -1.0
    buf[:, :g] = x
    lo, hi = k_row_select(buf, g)
    canon = np.where(x == 0, np.float32(0.0), x)   # (-0 counts as +0)
    elo, ehi = R.middle_two(canon)
    assert _same(lo, elo) and _same(hi, ehi), (g, ld)


# ---- fitted models ---------------------------------------------------------------------------------------------------------
def _data(kind):
  from sisua_amd.data import corrupt
  x = synth_counts(N, G, sparsity=0.8, seed=3)
  x[5] = 0.0
  if kind == "bernoulli":
    x = (x > 0).astype(np.float32)
  cor = x.copy()
  cor[40:200] = corrupt(x[40:200], dropout_rate=0.3, retain_rate=0.2, seed=8)   # a subset of the rows only
  return x, cor


def _fit(api, kind):
  from sisua_amd.data import SingleCellOMIC
  x, cor = _data(kind)
  lat = api.RVmeta(8, "diag", True, "Latents")
  net = dict(encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  sco = SingleCellOMIC(x, name="toy")
  if kind == "scvi":
    m = api.SCVI(outputs=sco.get_rv("transcriptomic", "zinbd"), latents=lat, **net)
  elif kind == "sisua":
    sco.add_omic("proteomic", synth_labels(N, ((9, "nb"),))[0])
    m = api.SISUA(outputs=sco.get_rv("transcriptomic", "nb"), labels=[api.RVmeta(9, "nb", True, "proteomic")], latents=lat, **net)
    m.fit(sco, epochs=3, batch_size=64, verbose=False)
    return m, x, cor
  else:
    m = api.VAE(outputs=sco.get_rv("transcriptomic", {"vae": "zinb"}.get(kind, kind)), latents=lat, **net)
  m.fit(sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True), metadata=sco, epochs=3, learning_rate=2e-3)
  return m, x, cor


_FITTED = {}


def fitted(api, kind):
  if kind not in _FITTED:
    _FITTED[kind] = _fit(api, kind)
  return _FITTED[kind]


def _lazy(m, inputs, S=(), batch_size=50):
  lX, _ = m.predict(inputs, sample_shape=S, batch_size=batch_size, verbose=False, lazy=True)
  return lX[0] if isinstance(lX, tuple) else lX


# ---- 3. exact functions of the device's own mean ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", [(), 3])
@pytest.mark.parametrize("kind", ["vae", "sisua", "scvi", "bernoulli"])
def test_scores_are_exact_functions_of_the_device_mean(api, kind, S):
  m, x, cor = fitted(api, kind)
  changed = R.cell_changed(x, cor)
  assert changed.any() and not changed.all()
  lz = _lazy(m, cor, S)
  mean = (lz.count_distribution if lz.is_zero_inflated else lz).mean_over_samples()
  assert mean.shape == (N, G) and mean.dtype == np.float32
  cells = lz.imputation_cells(x)
  got = lz.imputation_scores(x)
  want = R.scores(x, cor, mean)
  print(f"exact {kind} S={S}: device {got} reference {want}")
  assert _same(cells["cell_median"], R.cell_medians(x, mean))
  assert np.array_equal(cells["cell_changed"].astype(bool), changed)
  lo, hi = R.middle_two(R.abs_diff(x, mean).reshape(1, -1))
  assert _same(cells["global_lohi"], [lo[0], hi[0]])
  assert set(got) == {"imputation_med", "imputation_mean", "imputation_std"} and all(isinstance(v, float) for v in got.values())
  for k in want:
    assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
  # the model's method: the same scores from the same draws
  S_n = S if S else 1
  assert m.imputation_scores(cor, x, sample_shape=S_n, batch_size=50) == got


# ---- 4. against the float64 oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
def test_scores_against_the_float64_oracle(api, S):
  from oracle import sisua_oracle as so
  from sisua_amd.engine import Engine
  spec, cfg = make_pair(model="vae", n_genes=G, likelihood="zinb", enc_units=(32,), dec_units=(32,), latent_dim=8)
  params, bn = perturbed_params(spec), so.init_bn_state(spec)
  x, cor = _data("vae")
  B = 100
  x, cor = x[:B], cor[:B]
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  ref = np.zeros((B, G), np.float64)
  for s in range(S):   # one minibatch: a cell's noise id is its index
    r = so.forward_backward(spec, params, bn, cor, so.PhiloxNoise(spec.seed, 0, np.arange(B), sample=s), training=False, backward=False)
    ref += np.exp(np.asarray(r["x_params"][0], np.float64)) * np.exp(np.asarray(r["x_params"][1], np.float64))   # the count distribution's mean
  ref /= S
  mean = e.predict_stat(cor, "mean_over_samples", n_samples=S, batch=B, count_only=True)
  bound = float(np.abs(mean.astype(np.float64) - ref).max())
  got = e.predict_impute(cor, x, n_samples=S, batch=B, count_only=True)
  d = np.abs(x.astype(np.float64) - ref)
  med = 0.5 * (float(got["global_lohi"][0]) + float(got["global_lohi"][1]))
  err_med, err_cells = abs(med - np.median(d)), np.abs(got["cell_median"].astype(np.float64) - np.median(d, axis=1)).max()
  print(f"oracle S={S}: max |mean - oracle| {bound:.3e}; |imputation_med - oracle| {err_med:.3e}; max |cell_median - oracle| {err_cells:.3e}")
  e.close()
  assert bound < 1e-2 * max(1.0, float(ref.max()))   # (the two forward passes are the same model at all)
  assert err_med <= bound and err_cells <= bound


# ---- 5. invariance -------------------------------------------------------------------------------------------------------------
def test_invariance_to_batching_chunking_and_forms(api):
  """a model with deterministic latents: a cell's planes do not depend on its minibatch, so every form gives the same bits"""
  from sisua_amd import _hip
  from sisua_amd.data import SingleCellOMIC
  x, cor = _data("vae")
  sco = SingleCellOMIC(x, name="toy")
  m = api.DeepCountAutoencoder(outputs=sco.get_rv("transcriptomic", "zinb"), encoder=api.NetConf([32], batchnorm=True, dropout=0.1),
                               decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  m.fit(sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True), metadata=sco, epochs=3, learning_rate=2e-3)
  ref = _lazy(m, cor, (), 50).imputation_cells(x)

  def same(r):
    return _same(r["cell_median"], ref["cell_median"]) and np.array_equal(r["cell_changed"], ref["cell_changed"]) and \
        _same(r["global_lohi"], ref["global_lohi"])
  try:
    for keep in (None, 0.0, 1e18):   # the default, the repeated walk, "everything fits"
      if keep is not None:
        _hip.set_tuning("impute_keep_bytes", keep)
      for stage in (None, 40000.0):   # several chunks of the walk
        if stage is not None:
          _hip.set_tuning("predict_stage_floats", stage)
        for bs in (8, 64, 512):
          assert same(_lazy(m, cor, (), bs).imputation_cells(x)), (keep, stage, bs)
        assert same(_lazy(m, sp.csr_matrix(cor), (), 50).imputation_cells(x)), (keep, stage)
        assert same(_lazy(m, cor, (), 50).imputation_cells(sp.csr_matrix(x))), (keep, stage)
        assert same(_lazy(m, sp.csr_matrix(cor), (), 50).imputation_cells(sp.csr_matrix(x))), (keep, stage)
        _hip.clear_tuning("predict_stage_floats")
  finally:
    _hip.clear_tuning("")
  # a stochastic model, several draws: the two second-pass forms and the chunking at ONE batch size
  m2, x2, cor2 = fitted(api, "vae")
  ref = _lazy(m2, cor2, 3, 50).imputation_cells(x2)
  try:
    for keep in (0.0, 1e18):
      _hip.set_tuning("impute_keep_bytes", keep)
      _hip.set_tuning("predict_stage_floats", 40000.0)
      assert same(_lazy(m2, cor2, 3, 50).imputation_cells(x2)), keep
      assert same(_lazy(m2, sp.csr_matrix(cor2), 3, 50).imputation_cells(sp.csr_matrix(x2))), keep
      _hip.clear_tuning("")
  finally:
    _hip.clear_tuning("")


def test_nan_gives_nan(api):
  m, x, cor = fitted(api, "vae")
  xn = x.copy()
  xn[7, 3] = np.nan
  r = _lazy(m, cor, (), 50).imputation_cells(xn)
  assert np.isnan(r["cell_median"][7]) and np.isnan(r["cell_median"]).sum() == 1 and np.isnan(r["global_lohi"]).all()
  assert np.isnan(_lazy(m, cor, (), 50).imputation_scores(xn)["imputation_med"])


# ---- 6. column gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [(), 3])
def test_column_gather(api, S):
  from scipy.stats import pearsonr, spearmanr
  from sisua_amd import _hip
  from sisua_amd.metrics import CorrelationScores, ImputationError
  m, x, cor = fitted(api, "vae")
  lz = _lazy(m, x, S)
  full = lz.mean_over_samples()
  idx = [17, 3, 119, 3, 0, 64]
  assert np.array_equal(lz.mean_over_samples(genes=idx), full[:, idx])
  assert np.array_equal(_lazy(m, sp.csr_matrix(x), S).mean_over_samples(genes=idx), full[:, idx])
  _hip.set_tuning("predict_stage_floats", 40000.0)
  assert np.array_equal(lz.mean_over_samples(genes=np.array(idx)), full[:, idx])
  _hip.clear_tuning("")
  buf = np.empty((N, len(idx)), np.float32)
  assert lz.mean_over_samples(genes=idx, out=buf) is buf and np.array_equal(buf, full[:, idx])
  cfull = lz.count_distribution.mean_over_samples()
  assert np.array_equal(lz.count_distribution.mean_over_samples(genes=idx), cfull[:, idx])
  with pytest.raises(IndexError):
    lz.mean_over_samples(genes=[0, G])
  # the metric classes on the real model
  S_n = S if S else 1
  prot = np.random.default_rng(1).gamma(2.0, 1.0, size=(N, 3)) + x[:, [17, 3, 64]]
  pairs = [(17, 0), (3, 1), (64, 2)]
  got = CorrelationScores(x, prot, pairs, sample_shape=S_n, batch_size=50)(m)
  pe = [-pearsonr(cfull[:, g], prot[:, p])[0] for g, p in pairs]
  spm = [-spearmanr(cfull[:, g], prot[:, p]).correlation for g, p in pairs]
  assert got == {"pearson_mean": float(np.mean(pe)), "spearman_mean": float(np.mean(spm)), "pearson_med": float(np.median(pe)),
                 "spearman_med": float(np.median(spm))}
  ie = ImputationError(x, corrupted=cor, sample_shape=S_n, batch_size=50)(m)
  sc = m.imputation_scores(cor, x, sample_shape=S_n, batch_size=50)
  assert ie == {"imp_med": sc["imputation_med"], "imp_mean": sc["imputation_mean"]}


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_stale_handle(api):
  from sisua_amd.data import SingleCellOMIC
  x, cor = _data("vae")
  sco = SingleCellOMIC(x, name="toy")
  m = api.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), latents=api.RVmeta(8, "diag", True, "Latents"),
              encoder=api.NetConf([32]), decoder=api.NetConf([32]))
  ds = sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True)
  m.fit(ds, metadata=sco, epochs=1)
  lz = _lazy(m, cor, (), 50)
  with pytest.raises(ValueError):
    lz.imputation_scores(x[:, :-1])
  with pytest.raises(ValueError):
    lz.imputation_scores(x[:-1])
  with pytest.raises(ValueError):
    lz.imputation_scores(None)
  assert set(lz.imputation_scores(x)) == {"imputation_med", "imputation_mean", "imputation_std"}
  same = _lazy(m, x, (), 50).imputation_scores(x)   # nothing corrupted: no changed cell
  assert same["imputation_mean"] == 0.0 and same["imputation_std"] == 0.0
  m.fit(ds, metadata=sco, epochs=1)
  with pytest.raises(RuntimeError):
    lz.imputation_scores(x)
  with pytest.raises(RuntimeError):
    lz.mean_over_samples(genes=[1])
  with pytest.raises(NotImplementedError, match="imputation_scores"):
    m.create_posterior()
