"""Posterior-predictive sampling of the gene output on the device (smx_sample.hip): the law of the draws per parameter point against the
float64 closed forms (tests/predictive_sample_ref.py: bounds derived there, none tuned), determinism and independence of the batching,
and `LazyCountOutput.sample` through fitted models.  SEED was written here before the first GPU run."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import predictive_sample_ref as R
from tests.util import synth_counts

pytestmark = pytest.mark.gpu

SEED = 20261016
ROWS, G = 64, 1024   # N = 2^16 draws per parameter point
LK = {"nb": 0, "zinb": 1, "nbd": 2, "zinbd": 3, "mse": 4, "bernoulli": 5, "normal": 6}
_FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


def plane_sample(lk, planes, direct=False, count_only=False, seed=SEED, n_k=1):
  """smx_k_plane_sample on planes [k][rows][G] -> [n_k][rows][G]"""
  from sisua_amd import _hip, build
  build.build(verbose=False)
  lib = _hip.require_gpu()
  pl = np.ascontiguousarray(planes, np.float32)
  k, rows, g = pl.shape
  out = np.empty((n_k, rows, g), np.float32)
  _hip.check(lib.smx_k_plane_sample(LK[lk], int(direct), int(count_only), pl.ctypes.data_as(_FP), rows, g, seed, n_k, out.ctypes.data_as(_FP)))
  return out


POINTS = [(r, m) for r in R.SHAPES for m in R.MEANS]


@functools.lru_cache(maxsize=None)
def _grid_draws(param, pi):
  """one launch per (parameterisation, gate): ROWS rows of constant planes per (shape, mean) point"""
  k = 2 if pi is None else 3
  planes = np.empty((k, len(POINTS) * ROWS, G), np.float32)
  for i, (r, m) in enumerate(POINTS):
    for c, v in enumerate(R.count_planes(param, r, m, pi)):
      planes[c, i * ROWS:(i + 1) * ROWS] = v
  lk = ("zinb" if pi is not None else "nb") if param == "nb" else ("zinbd" if pi is not None else "nbd")
  return plane_sample(lk, planes, direct=(param == "nbd_direct"))[0]


@pytest.mark.parametrize("m", R.MEANS)
@pytest.mark.parametrize("r", R.SHAPES)
@pytest.mark.parametrize("pi", R.GATES)
@pytest.mark.parametrize("param", R.PARAMETERISATIONS)
def test_count_law(param, pi, r, m):
  i = POINTS.index((r, m))
  x = _grid_draws(param, pi)[i * ROWS:(i + 1) * ROWS]
  law = R.CountLaw(*R.count_params(param, R.count_planes(param, r, m, pi)))
  ok_m, zm, zv = R.moments_check(x, law)
  ok_c, stat, crit, bins = R.chi2_check(x, law)
  print(f"count_law {param} pi={pi} r={r} m={m}: z_mean {zm:+.2f} z_var {zv:+.2f} chi2 {stat:.1f} / {crit:.1f} ({bins} bins)")
  assert x.dtype == np.float32 and R.integer_valued(x)
  assert ok_m, (zm, zv)
  assert ok_c, (stat, crit, bins)


def test_count_only_drops_the_gate():
  r, m, pi = 3.0, 2.0, 0.7
  for param in R.PARAMETERISATIONS:
    planes = np.stack([np.full((ROWS, G), v, np.float32) for v in R.count_planes(param, r, m, pi)])
    lk = "zinb" if param == "nb" else "zinbd"
    x = plane_sample(lk, planes, direct=(param == "nbd_direct"), count_only=True)[0]
    rr, mm, _ = R.count_params(param, R.count_planes(param, r, m, pi))
    law = R.CountLaw(rr, mm, None)
    assert R.moments_check(x, law)[0] and R.chi2_check(x, law)[0], param


@pytest.mark.parametrize("logits", R.BERNOULLI_LOGITS)
def test_bernoulli_law(logits):
  x = plane_sample("bernoulli", np.full((1, ROWS, G), logits, np.float32))[0]
  law = R.BernoulliLaw(logits)
  ok_m, zm, zv = R.moments_check(x, law)
  ok_c, stat, crit, _ = R.chi2_check(x, law)
  print(f"bernoulli_law {logits}: z_mean {zm:+.2f} z_var {zv:+.2f} chi2 {stat:.1f} / {crit:.1f}")
  assert set(np.unique(x)) <= {0.0, 1.0} and ok_m and ok_c


@pytest.mark.parametrize("loc,raw", R.NORMAL_POINTS)
def test_normal_law(loc, raw):
  x = plane_sample("normal", np.stack([np.full((ROWS, G), loc, np.float32), np.full((ROWS, G), raw, np.float32)]))[0]
  law = R.NormalLaw(loc, raw)
  ok_m, zm, zv = R.moments_check(x, law)
  ok_k, d, crit = R.ks_check(x, law)
  print(f"normal_law {loc} {raw}: z_mean {zm:+.2f} z_var {zv:+.2f} ks {d:.5f} / {crit:.5f}")
  assert ok_m and ok_k


def test_mse_is_the_location():
  loc = np.random.default_rng(0).normal(size=(1, 8, 100)).astype(np.float32)
  assert np.array_equal(plane_sample("mse", loc, n_k=2), np.stack([loc[0], loc[0]]))


# ---- determinism -----------------------------------------------------------------------------------------------
def _mixed_planes(rows=48, g=200):
  rng = np.random.default_rng(5)
  return np.stack([rng.normal(0.5, 1.5, (rows, g)), rng.normal(0.0, 1.0, (rows, g)), rng.normal(-1.0, 1.0, (rows, g))]).astype(np.float32)


def test_kernel_is_deterministic_in_the_seed():
  planes = _mixed_planes()
  a, b = plane_sample("zinb", planes, seed=7, n_k=3), plane_sample("zinb", planes, seed=7, n_k=3)
  assert np.array_equal(a, b)
  c = plane_sample("zinb", planes, seed=8, n_k=3)
  nb7, nb8 = plane_sample("nb", planes[:2], seed=7)[0], plane_sample("nb", planes[:2], seed=8)[0]
  nondeg = np.exp(planes[0]) * np.exp(planes[1]) > 3.0   # the non-degenerate elements: mean above 3, P(two independent draws agree) well under 1 / 2
  assert nondeg.sum() > 1000 and (nb7[nondeg] != nb8[nondeg]).mean() > 0.5
  assert (a[0][nondeg] != c[0][nondeg]).mean() > 0.3
  # the n_k samples of one call are different draws, and sample k does not depend on n_k
  assert (nb7[nondeg] != plane_sample("nb", planes[:2], seed=7, n_k=2)[1][nondeg]).mean() > 0.5
  assert np.array_equal(a[:2], plane_sample("zinb", planes, seed=7, n_k=2))


@pytest.fixture(scope="module")
def fitted(api):
  from sisua_amd.data import SingleCellOMIC
  x = synth_counts(300, 120, sparsity=0.8, seed=3)
  x[5] = 0.0
  x[40:104] = np.maximum(x[40:104], 1.0)
  sco = SingleCellOMIC(x, name="toy")
  m = api.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), latents=api.RVmeta(8, "diag", True, "Latents"),
              encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  m.fit(sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True), metadata=sco, epochs=3, learning_rate=2e-3)
  return m, sco, x


def _lazy(m, inputs, S=(), batch_size=50):
  lX, _ = m.predict(inputs, sample_shape=S, batch_size=batch_size, verbose=False, lazy=True)
  return lX[0] if isinstance(lX, tuple) else lX


@pytest.mark.parametrize("S", [(), 3])
def test_samples_do_not_depend_on_batching_or_input_form(api, fitted, S):
  from sisua_amd import _hip
  from sisua_amd.data import SingleCellOMIC
  m, sco, x = fitted
  ref = _lazy(m, sco, S, 50).sample(2, seed=SEED)
  lead = (S,) if S else ()
  assert ref.shape == (2,) + lead + (300, 120) and ref.dtype == np.float32
  # Another batch size: the sampler's counters do not know it, but the latent draws of a stochastic model do (a cell's noise id is its
  # index within its minibatch), so the planes themselves move with batch_size for every cell past the first minibatch.  Wherever the
  # planes are the same bits (the three statistics below determine the three planes), the samples are.
  def stats(lz):
    return np.stack([lz.mean(), lz.variance(), lz.count_distribution.mean()])
  ref_stats = stats(_lazy(m, sco, S, 50))
  for bs in (32, 512):
    lz = _lazy(m, sco, S, bs)
    same = np.all(stats(lz) == ref_stats, axis=(0, -1))   # [S,] N: the cell's planes are those of the reference
    same = same.all(axis=0) if same.ndim > 1 else same
    print(f"batching S={S} batch_size={bs}: {int(same.sum())} of 300 cells have the reference's planes")
    assert same[:min(bs, 50)].all()
    assert np.array_equal(lz.sample(2, seed=SEED)[..., same, :], ref[..., same, :]), bs
  assert np.array_equal(_lazy(m, sp.csr_matrix(x), S, 50).sample(2, seed=SEED), ref)                      # scipy.sparse input: the CSR walk
  assert np.array_equal(_lazy(m, SingleCellOMIC(sp.csr_matrix(x), name="toy"), S, 50).sample(2, seed=SEED), ref)
  _hip.set_tuning("predict_stage_floats", 40000.0)   # several chunks of the walk
  assert np.array_equal(_lazy(m, sco, S, 50).sample(2, seed=SEED), ref)
  assert np.array_equal(_lazy(m, sp.csr_matrix(x), S, 50).sample(2, seed=SEED), ref)
  _hip.clear_tuning("")
  # the seed: reproducible, and another seed / another sample index is another draw
  lz = _lazy(m, sco, S, 50)
  s3 = lz.sample(3, seed=SEED)
  assert np.array_equal(s3, lz.sample(3, seed=SEED)) and np.array_equal(s3[:2], ref)
  # the non-degenerate elements: two independent draws of the element's law agree with probability sum_k p(k)^2 < 0.4
  e = lz.materialize()
  ks = np.arange(64.0).reshape((64,) + (1,) * lz.mean().ndim)
  agree = (np.exp(e.distribution.log_prob(ks)) ** 2).sum(0)
  live = agree < 0.4
  print(f"determinism S={S}: {int(live.sum())} non-degenerate elements of {live.size}")
  # independent draws differ in a fraction mean(1 - agree) of ALL elements, within 6 standard errors of a mean of independent indicators
  want, bound = float((1.0 - agree).mean()), 6.0 * np.sqrt(0.25 / agree.size)
  for other in (s3[1], lz.sample(seed=SEED + 1)):
    got = float((s3[0] != other).mean())
    print(f"determinism S={S}: {got:.4f} of the elements differ, expected {want:.4f} +- {bound:.4f}")
    assert abs(got - want) <= bound
    if live.sum() > 200:
      assert (s3[0][live] != other[live]).mean() > 0.5
  assert not np.array_equal(lz.sample(), lz.sample())   # seed=None: fresh entropy
  buf = np.empty(s3.shape, np.float32)
  assert lz.sample(3, seed=SEED, out=buf) is buf and np.array_equal(buf, s3)
  assert lz.sample((2, 2), seed=SEED).shape == (2, 2) + lead + (300, 120)


def test_samples_do_not_depend_on_the_batch_size(api):
  """a fitted model with deterministic latents (the planes of a cell do not depend on its minibatch): batch_size 32 / 50 / 512 give
  the same samples bit for bit, dense and sparse"""
  from sisua_amd.data import SingleCellOMIC
  x = synth_counts(300, 120, sparsity=0.8, seed=3)
  sco = SingleCellOMIC(x, name="toy")
  m = api.DeepCountAutoencoder(outputs=sco.get_rv("transcriptomic", "zinb"), encoder=api.NetConf([32], batchnorm=True, dropout=0.1),
                               decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  m.fit(sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True), metadata=sco, epochs=3, learning_rate=2e-3)
  ref = _lazy(m, sco, (), 50).sample(2, seed=SEED)
  assert R.integer_valued(ref) and ref.shape == (2, 300, 120)
  for bs in (32, 512):
    assert np.array_equal(_lazy(m, sco, (), bs).sample(2, seed=SEED), ref), bs
    assert np.array_equal(_lazy(m, sp.csr_matrix(x), (), bs).sample(2, seed=SEED), ref), bs


@pytest.mark.parametrize("storage", ["u16", "csr"])
def test_samples_do_not_depend_on_the_resident_store(api, fitted, storage, tmp_path):
  """the same parameters in a model whose counts are resident as uint16 / CSR: the same samples"""
  from sisua_amd.data import SingleCellOMIC
  m, sco, x = fitted
  ref = _lazy(m, sco, 2, 50).sample(2, seed=SEED)
  m.save_weights(os.path.join(tmp_path, "w"))
  other = api.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), latents=api.RVmeta(8, "diag", True, "Latents"),
                  encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  src = SingleCellOMIC(sp.csr_matrix(x), name="toy") if storage == "csr" else sco
  other.fit(src, epochs=1, batch_size=64, storage=storage, verbose=False)
  other.load_weights(os.path.join(tmp_path, "w"))
  lz = _lazy(other, src, 2, 50)
  assert np.array_equal(lz.mean(), _lazy(m, sco, 2, 50).mean())
  assert np.array_equal(lz.sample(2, seed=SEED), ref)


# ---- end to end -----------------------------------------------------------------------------------------------
def _model(api, kind, sco):
  lat = api.RVmeta(8, "diag", True, "Latents")
  net = dict(encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  if kind == "scvi":
    return api.SCVI(outputs=sco.get_rv("transcriptomic", "zinbd"), latents=lat, **net)
  return api.VAE(outputs=sco.get_rv("transcriptomic", {"vae": "zinb"}.get(kind, kind)), latents=lat, **net)


@pytest.mark.parametrize("kind", ["vae", "scvi", "bernoulli", "normal"])
def test_lazy_sample_end_to_end(api, kind):
  from sisua_amd import distributions as D
  from sisua_amd.data import SingleCellOMIC
  x = synth_counts(300, 120, sparsity=0.8, seed=3)
  if kind == "bernoulli":
    x = (x > 0).astype(np.float32)
  elif kind == "normal":
    x = np.log1p(x) - 0.5
  sco = SingleCellOMIC(x, name="toy")
  m = _model(api, kind, sco)
  m.fit(sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True), metadata=sco, epochs=3, learning_rate=2e-3)
  K = 64
  for S in ((), 2):
    lz = _lazy(m, sco, S, 50)
    assert isinstance(lz, D.LazyCountOutput)
    lead = (S,) if S else ()
    x1 = lz.sample(seed=SEED)
    assert x1.shape == lead + (300, 120) and x1.dtype == np.float32
    xs = lz.sample(K, seed=SEED)
    assert xs.shape == (K,) + lead + (300, 120) and np.array_equal(xs[0], x1)
    if kind in ("vae", "scvi"):
      assert R.integer_valued(xs)
    elif kind == "bernoulli":
      assert set(np.unique(xs)) <= {0.0, 1.0}
    # pooled over the cells (and the latent draws) and the K samples, per gene: the sample mean against mean(), within 6 standard errors
    # from variance() (the elements are independent draws of their own laws: the pooled mean has variance sum(var) / n^2)
    mean, var = lz.mean().astype(np.float64), lz.variance().astype(np.float64)
    ax = tuple(range(xs.ndim - 1))
    n = xs.size // 120
    got = xs.astype(np.float64).mean(axis=ax)
    want = mean.mean(axis=tuple(range(mean.ndim - 1)))
    se = np.sqrt(var.sum(axis=tuple(range(var.ndim - 1))) * K) / n
    z = (got - want) / se
    print(f"end_to_end {kind} S={S}: max |z| of the per-gene pooled mean {np.abs(z).max():.2f}")
    assert np.all(np.abs(z) <= 6.0), np.abs(z).max()
    if lz.is_zero_inflated:
      xc = lz.count_distribution.sample(K, seed=SEED + 1)
      assert xc.shape == xs.shape and R.integer_valued(xc)
      # P(sample = 0) - P(count sample = 0) = pi (1 - p_count(0)) per element; both zero fractions are means of independent
      # indicators, each of variance <= 1 / 4: the difference of the two fractions within 6 sqrt(2 * 1 / 4 / n_total) of its expectation
      e = lz.materialize()
      pi = np.broadcast_to(e.distribution.probs, mean.shape)
      p0c = np.exp(e.distribution.count_distribution.log_prob(np.zeros(mean.shape)))
      expect = float((pi * (1.0 - p0c)).mean())
      diff = float((xs == 0).mean() - (xc == 0).mean())
      bound = 6.0 * np.sqrt(0.5 / xs.size)
      print(f"end_to_end {kind} S={S}: zero fraction gap {diff:.5f}, expected {expect:.5f} +- {bound:.5f}, mean gate {float(pi.mean()):.4f}")
      assert expect > 2 * bound and abs(diff - expect) <= bound
  # a stale handle raises
  m.fit(sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True), metadata=sco, epochs=1)
  with pytest.raises(RuntimeError):
    lz.sample(seed=SEED)


# ---- robustness --------------------------------------------------------------------------------------------------
def test_degenerate_planes_return():
  """NaN, +-inf, an overflowing mean (p0 = 80) and a shape of 1e-6 in every plane combination: every rejection loop is bounded, the call
  returns, and each result is NaN or finite (counts: a non-negative integer).  Run once, under the suite's normal time limit."""
  bad = np.array([np.nan, np.inf, -np.inf, 80.0, np.log(1e-6), 0.0], np.float32)
  nb = bad.size
  for lk, k in (("nb", 2), ("zinb", 3), ("nbd", 2), ("zinbd", 3), ("bernoulli", 1), ("normal", 2)):
    for direct in ((False, True) if lk in ("nbd", "zinbd") else (False,)):
      planes = np.zeros((k, nb ** k, 64), np.float32)
      idx = np.indices((nb,) * k).reshape(k, -1)
      for c in range(k):
        planes[c] = bad[idx[c]][:, None]
      x = plane_sample(lk, planes, direct=direct, n_k=2)
      assert np.all(np.isnan(x) | np.isfinite(x)), (lk, direct)
      fin = x[np.isfinite(x)]
      if lk not in ("normal",):
        assert np.all(fin == np.floor(fin)) and np.all(fin >= 0), (lk, direct)
      any_nan_plane = np.isnan(planes).any(axis=0)
      if lk in ("nb", "nbd", "bernoulli", "normal"):   # (a zero-inflated draw gated to 0 never reads the count planes)
        assert np.all(np.isnan(x[:, any_nan_plane])), (lk, direct)
