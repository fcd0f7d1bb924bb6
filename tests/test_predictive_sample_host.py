"""Predictive sampling, host side: the acceptance functions of tests/predictive_sample_ref.py pass on the host reference (the eager
NumPy distributions' `sample`, fixed seed) at every point of the grid the device sampler is held to, and fail on deliberately wrong
samplers -- so the bounds separate right from wrong before any GPU run.  And the shape / seed contract of `LazyCountOutput.sample`
against a stand-in engine."""
import types

import numpy as np
import pytest

from sisua_amd import distributions as D
from tests import predictive_sample_ref as R

N = 1 << 16
SEED = 20261016


def _eager(param, r, m, pi):
  planes = [np.full((N,), v, np.float32) for v in R.count_planes(param, r, m, pi)]
  lk = ("zinb" if pi is not None else "nb") if param == "nb" else ("zinbd" if pi is not None else "nbd")
  return D.count_distribution(lk, [p[None, :] for p in planes], "x", activated=(param == "nbd_direct")), R.CountLaw(*R.count_params(param, [p[0] for p in planes]))


@pytest.mark.parametrize("param", R.PARAMETERISATIONS)
@pytest.mark.parametrize("pi", R.GATES)
def test_host_reference_passes_at_every_grid_point(param, pi):
  for r in R.SHAPES:
    for m in R.MEANS:
      dist, law = _eager(param, r, m, pi)
      x = np.asarray(dist.sample(seed=SEED))
      ok_m, zm, zv = R.moments_check(x, law)
      ok_c, stat, crit, bins = R.chi2_check(x, law)
      assert R.integer_valued(x)
      assert ok_m, (param, r, m, pi, zm, zv)
      assert ok_c, (param, r, m, pi, stat, crit, bins)


def test_fourth_moment_closed_form_against_a_pmf_sum():
  """where the pmf sum converges (moderate shape and mean) it agrees with the factorial-moment form"""
  for r, m, pi in ((3.0, 2.0, None), (0.5, 15.0, 0.1), (50.0, 0.3, 0.7)):
    law = R.CountLaw(r, m, pi)
    k = np.arange(0, 20000)
    p = law.pmf(k)
    mean = (k * p).sum()
    var = ((k - mean) ** 2 * p).sum()
    mu4 = ((k - mean) ** 4 * p).sum()
    assert np.allclose(law.moments(), (mean, var, mu4), rtol=1e-8)


def test_bernoulli_and_normal_references_pass():
  for l in R.BERNOULLI_LOGITS:
    x = D.Bernoulli(logits=np.full((N,), l, np.float32)).sample(seed=SEED)
    law = R.BernoulliLaw(l)
    assert R.moments_check(x, law)[0] and R.chi2_check(x, law)[0], l
  for loc, raw in R.NORMAL_POINTS:
    law = R.NormalLaw(loc, raw)
    x = D.Normal(np.full((N,), law.loc), np.full((N,), law.scale)).sample(seed=SEED)
    assert R.moments_check(x, law)[0] and R.ks_check(x, law)[0], (loc, raw)


@pytest.mark.parametrize("wrong", ["no_mixing", "gate_swapped", "shape_scale_swapped", "bernoulli_complement", "normal_variance_for_scale"])
def test_wrong_samplers_fail(wrong):
  rng = np.random.default_rng(SEED)
  if wrong == "no_mixing":   # Poisson of the mean, without the Gamma
    law = R.CountLaw(0.5, 2.0)
    x = rng.poisson(2.0, N)
    assert not R.moments_check(x, law)[0] and not R.chi2_check(x, law)[0]
  elif wrong == "gate_swapped":   # kept with probability pi instead of 1 - pi
    law = R.CountLaw(3.0, 2.0, 0.1)
    x = rng.poisson(rng.gamma(3.0, 2.0 / 3.0, N)) * (rng.uniform(size=N) < 0.1)
    assert not R.moments_check(x, law)[0] and not R.chi2_check(x, law)[0]
  elif wrong == "shape_scale_swapped":   # the same mean, another variance
    law = R.CountLaw(3.0, 15.0)
    x = rng.poisson(rng.gamma(5.0, 3.0, N))
    assert abs(x.mean() - 15.0) < 0.5
    assert not R.moments_check(x, law)[0] and not R.chi2_check(x, law)[0]
  elif wrong == "bernoulli_complement":
    law = R.BernoulliLaw(-1.0)
    x = (rng.uniform(size=N) >= law.p).astype(np.float32)
    assert not R.moments_check(x, law)[0] and not R.chi2_check(x, law)[0]
  else:   # softplus1(raw)^2 used as the standard deviation
    law = R.NormalLaw(0.25, 1.5)
    x = law.loc + law.scale ** 2 * rng.standard_normal(N)
    assert not R.moments_check(x, law)[0] and not R.ks_check(x, law)[0]


def test_a_small_bias_is_seen():
  """a rate off by 3 % (far above the float32 perturbation of the parameters, ~1e-6) is rejected at 2^16 draws"""
  rng = np.random.default_rng(SEED)
  law = R.CountLaw(50.0, 15.0)
  x = rng.poisson(rng.gamma(50.0, 1.03 * 15.0 / 50.0, N))
  assert not R.moments_check(x, law)[0]


# ---- LazyCountOutput.sample against a stand-in engine ------------------------------------------------
class _Engine:

  def __init__(self):
    self.calls = []

  def predict_stat(self, x, stat, library=None, n_samples=1, batch=None, count_only=False, target=None, out=None, seed=0, n=1):
    self.calls.append(dict(stat=stat, n_samples=n_samples, batch=batch, count_only=count_only, seed=seed, n=n))
    shape = (n, n_samples, x.shape[0], x.shape[1])
    r = np.random.default_rng(seed).poisson(1.0, shape).astype(np.float32)
    if out is not None:
      assert out.shape == shape
      out[...] = r
      return out
    return r


def _lazy(S, lk="zinb", n=5, g=7):
  eng = _Engine()
  model = types.SimpleNamespace(_cfg=types.SimpleNamespace(likelihood=lk, n_genes=g), step=3, _param_version=0, _ensure_engine=lambda b: eng)
  return D.LazyCountOutput(model, np.zeros((n, g), np.float32), None, S, 4, "x"), eng, model


def test_engine_knows_the_sample_stat():
  from sisua_amd.engine import Engine
  assert Engine.STATS["sample"] == 4 and Engine.STATS["log_prob"] == 3


@pytest.mark.parametrize("S", [1, 3])
def test_lazy_sample_shape_and_seed_contract(S):
  lz, eng, model = _lazy(S)
  lead = (S,) if S > 1 else ()
  assert lz.sample(seed=1).shape == lead + (5, 7) and lz.sample(seed=1).dtype == np.float32
  assert lz.sample(3, seed=1).shape == (3,) + lead + (5, 7)
  assert lz.sample((2, 3), seed=1).shape == (2, 3) + lead + (5, 7)
  assert eng.calls[-1] == dict(stat="sample", n_samples=S, batch=4, count_only=False, seed=1, n=6)
  assert np.array_equal(lz.sample(3, seed=11), lz.sample(3, seed=11))
  # seed=None: fresh entropy, an integer handed to the engine
  lz.sample(); a = eng.calls[-1]["seed"]
  lz.sample(); b = eng.calls[-1]["seed"]
  assert isinstance(a, int) and isinstance(b, int) and a != b and 0 <= a < 2 ** 64
  # the count distribution samples without the gate
  lz.count_distribution.sample(2, seed=5)
  assert eng.calls[-1]["count_only"] is True and eng.calls[-1]["n"] == 2
  # out=: written in place
  buf = np.empty((3,) + lead + (5, 7), np.float32)
  assert lz.sample(3, seed=11, out=buf) is buf and np.array_equal(buf, lz.sample(3, seed=11))
  with pytest.raises(ValueError):
    lz.sample(3, seed=11, out=np.empty((5, 7), np.float32))
  with pytest.raises(ValueError):
    lz.sample((0,), seed=1)
  # a stale handle raises
  model.step = 4
  with pytest.raises(RuntimeError):
    lz.sample(seed=1)
