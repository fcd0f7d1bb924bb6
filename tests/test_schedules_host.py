"""Step-dependent weights on the host (sisua_amd.interpolation; include/sisua_hip.h: smx_set_schedule): every interpolation and Keras
learning-rate schedule against its closed form, the library's evaluator (smx_schedule_eval) against the Python one, the parsing of every
accepted form and every refusal, and the model surface that takes a schedule as `beta`.  CPU only."""
import ctypes as C
import math
import pickle

import numpy as np
import pytest

from sisua_amd import interpolation as I
from sisua_amd import optimizers

F32 = lambda v: float(np.float32(v))


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def test_interpolations_closed_form():
  lin = I.linear(vmin=0.5, vmax=3.0, norm=20, delayIn=5, delayOut=4)
  for s in range(0, 60):
    a = 0.0 if s < 5 else min((s - 5) / 20.0, 1.0)
    assert lin.value(s) == pytest.approx(0.5 + 2.5 * a, rel=0, abs=1e-15), s
  pw = I.power(vmin=1.0, vmax=2.0, norm=8, power=3)
  cs = I.cosine(vmin=-1.0, vmax=1.0, norm=8)
  for s in range(0, 12):
    a = min(s / 8.0, 1.0)
    assert pw.value(s) == pytest.approx(1.0 + a ** 3, abs=1e-15)
    assert cs.value(s) == pytest.approx(-1.0 + 2.0 * (0.5 - 0.5 * math.cos(math.pi * a)), abs=1e-15)
  assert I.const(0.25).value(123456) == 0.25 and I.const(vmax=1).value(0) == 1.0


def test_ramp_ends_are_the_end_points_bit_for_bit():
  vmin, vmax = 0.3, 0.9   # (vmin + (vmax - vmin) * 1 is not vmax in float64)
  assert vmin + (vmax - vmin) * 1.0 != vmax
  for f in (I.linear, I.cosine, I.power):
    sch = f(vmin=vmin, vmax=vmax, norm=10, delayIn=3)
    assert sch.value(0) == vmin and sch.value(3) == vmin and sch.value(13) == vmax and sch.value(10 ** 6) == vmax
    assert sch(3) == F32(vmin) and sch(13) == F32(vmax)


def test_cyclical_wrap():
  sch = I.linear(vmin=0, vmax=10, norm=20, cyclical=True, delayOut=5, delayIn=5)   # the reference tutorial's KL weight
  P = 30
  for s in range(0, 3 * P):
    p = s % P
    a = 0.0 if p < 5 else min((p - 5) / 20.0, 1.0)
    assert sch.value(s) == pytest.approx(10 * a, abs=1e-14), s
  assert sch.value(P) == 0.0 and sch.value(P + 25) == 10.0 and sch.value(2 * P + 29) == 10.0


def test_keras_closed_forms():
  ed = I.as_schedule({"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=0.1, decay_steps=7, decay_rate=0.5)})
  eds = I.as_schedule({"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=0.1, decay_steps=7, decay_rate=0.5, staircase=True)})
  it = I.as_schedule({"class_name": "InverseTimeDecay", "config": dict(initial_learning_rate=0.1, decay_steps=4, decay_rate=0.3)})
  its = I.as_schedule({"class_name": "InverseTimeDecay", "config": dict(initial_learning_rate=0.1, decay_steps=4, decay_rate=0.3, staircase=True)})
  pd = I.as_schedule({"class_name": "PolynomialDecay", "config": dict(initial_learning_rate=0.1, decay_steps=10)})
  pdc = I.as_schedule({"class_name": "PolynomialDecay", "config": dict(initial_learning_rate=0.1, decay_steps=10, end_learning_rate=0.01,
                                                                         power=2.0, cycle=True)})
  cd = I.as_schedule({"class_name": "CosineDecay", "config": dict(initial_learning_rate=0.1, decay_steps=10, alpha=0.2)})
  for s in range(0, 40):
    assert ed.value(s) == pytest.approx(0.1 * 0.5 ** (s / 7), rel=1e-14)
    assert eds.value(s) == pytest.approx(0.1 * 0.5 ** (s // 7), rel=1e-14)
    assert it.value(s) == pytest.approx(0.1 / (1 + 0.3 * s / 4), rel=1e-14)
    assert its.value(s) == pytest.approx(0.1 / (1 + 0.3 * (s // 4)), rel=1e-14)
    t = min(s, 10)
    assert pd.value(s) == pytest.approx((0.1 - 0.0001) * (1 - t / 10) + 0.0001, rel=1e-14)   # (defaults: end 1e-4, power 1)
    ds = 10 * (1 if s == 0 else math.ceil(s / 10))
    assert pdc.value(s) == pytest.approx((0.1 - 0.01) * (1 - s / ds) ** 2 + 0.01, rel=1e-14)
    assert cd.value(s) == pytest.approx(0.1 * ((1 - 0.2) * 0.5 * (1 + math.cos(math.pi * t / 10)) + 0.2), rel=1e-14)
  pw = I.as_schedule({"class_name": "PiecewiseConstantDecay", "config": dict(boundaries=[10, 20], values=[1.0, 0.5, 0.1])})
  assert [pw.value(s) for s in (0, 10, 11, 20, 21, 10 ** 6)] == [1.0, 1.0, 0.5, 0.5, 0.1, 0.1]   # (inclusive boundaries)


# ---- the library's evaluator ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
  from sisua_amd import _hip, build
  build.build(verbose=False)
  return _hip.load()


def _lib_eval(lib, sch, first, count):
  p = np.ascontiguousarray(sch.params, np.float64)
  out = np.empty(count, np.float32)
  rc = lib.smx_schedule_eval(sch.kind, p.ctypes.data_as(C.POINTER(C.c_double)), len(p), int(first), count,
                             out.ctypes.data_as(C.POINTER(C.c_float)))
  return rc, out


SCHEDULES = {
    "const": I.const(0.37),
    "linear": I.linear(vmin=0.1, vmax=0.7, norm=20, delayIn=5),
    "linear_cyc": I.linear(vmin=0, vmax=10, norm=20, cyclical=True, delayOut=5, delayIn=5),
    "power": I.power(vmin=0.2, vmax=1.3, norm=333, cyclical=True, delayIn=7, delayOut=2, power=3),
    "cosine": I.cosine(vmin=0.0, vmax=1.0, norm=1000, cyclical=True, delayOut=50),
    "exp": I.as_schedule({"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=1e-3, decay_steps=1000, decay_rate=0.9)}),
    "exp_stair": I.as_schedule({"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=1e-3, decay_steps=977, decay_rate=0.5,
                                                                                staircase=True)}),
    "invtime": I.as_schedule({"class_name": "InverseTimeDecay", "config": dict(initial_learning_rate=1e-2, decay_steps=10, decay_rate=0.5)}),
    "piecewise": I.as_schedule({"class_name": "PiecewiseConstantDecay", "config": dict(boundaries=[100, 5000, 70000],
                                                                                      values=[1e-3, 5e-4, 1e-4, 3e-5])}),
    "poly": I.as_schedule({"class_name": "PolynomialDecay", "config": dict(initial_learning_rate=1e-3, decay_steps=30000, power=0.5)}),
    "poly_cycle": I.as_schedule({"class_name": "PolynomialDecay", "config": dict(initial_learning_rate=1e-3, decay_steps=777, cycle=True)}),
    "cosdecay": I.as_schedule({"class_name": "CosineDecay", "config": dict(initial_learning_rate=1e-3, decay_steps=50000, alpha=0.1)}),
}


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_library_evaluator_matches_python(lib, name):
  sch = SCHEDULES[name]
  for first, count in ((0, 100001), (2 ** 31 - 5000, 5000)):
    rc, got = _lib_eval(lib, sch, first, count)
    assert rc == 0
    want = np.array([sch.value(first + i) for i in range(count)], np.float64).astype(np.float32)
    if sch.kind in (I.CONST, I.PIECEWISE):
      assert np.array_equal(got, want)
    else:
      ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
      assert ulp.max() <= 1, (first, int(ulp.argmax()), int(ulp.max()))
  if sch.kind in (I.LINEAR, I.POWER, I.COSINE):   # the ramp's ends: exactly vmin / vmax
    vmin, vmax, norm, _, din, _ = sch.params[:6]
    rc, got = _lib_eval(lib, sch, 0, int(din + norm) + 3)
    assert got[0] == np.float32(vmin) and got[int(din + norm)] == np.float32(vmax)


def test_library_refusals(lib):
  for kind, p in ((I.LINEAR, [0, 1, 0, 0, 0, 0]), (I.LINEAR, [0, 1, 5, 0, -1, 0]), (I.EXP_DECAY, [1e-3, 0, 0.5, 0]),
                  (I.PIECEWISE, [5, 5, 1, 2, 3]), (I.PIECEWISE, [1, 2]), (99, [1.0]), (I.CONST, [float("nan")])):
    sch = I.Schedule.__new__(I.Schedule)
    sch.kind, sch.params = kind, tuple(float(v) for v in p)
    assert _lib_eval(lib, sch, 0, 4)[0] != 0, (kind, p)


# ---- parsing, refusals, pickling ----------------------------------------------------------------------------------------------------
class ExponentialDecay:   # what a tf.keras schedule is to this code: a class name and get_config()
  def __init__(self, **cfg):
    self.cfg = cfg

  def get_config(self):
    return dict(self.cfg, name="ExponentialDecay")


class CosineDecay(ExponentialDecay):
  pass


def test_resolve_forms():
  ed = dict(initial_learning_rate=0.01, decay_steps=100, decay_rate=0.9)
  want = I.Schedule(I.EXP_DECAY, (0.01, 100, 0.9, 0))
  assert optimizers.resolve("adam", {"class_name": "ExponentialDecay", "config": ed}, 1.0)[2] == want
  assert optimizers.resolve({"class_name": "adam", "config": {"learning_rate": {"class_name": "ExponentialDecay", "config": ed}}}, 1e-3, 1.0)[2] == want
  assert optimizers.resolve({"class_name": "sgd", "config": {"lr": ExponentialDecay(**ed)}}, 1e-3, 1.0)[2] == want
  assert optimizers.resolve("rmsprop", ExponentialDecay(**ed), None)[2] == want
  lin = I.linear(vmin=0, vmax=1e-3, norm=10)
  assert optimizers.resolve("adam", lin, 1.0)[2] == lin   # (either kind serves either target)
  n, hp, lr, clip = optimizers.resolve("adam", 2e-3, 5.0)
  assert lr == 2e-3 and float(lr) == 2e-3 and lr.kind == I.CONST and clip == 5.0
  cd = I.as_schedule(CosineDecay(initial_learning_rate=1.0, decay_steps=5, warmup_target=None, warmup_steps=0))
  assert cd == I.Schedule(I.COSINE_DECAY, (1.0, 5.0, 0.0))


REFUSED = [
    (lambda s: s * 0.1, "callable"),
    ({"class_name": "ReduceLROnPlateau", "config": {}}, "not built"),
    ({"class_name": "CosineDecayRestarts", "config": dict(initial_learning_rate=1.0, first_decay_steps=10)}, "not built"),
    ({"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=1.0, decay_steps=0, decay_rate=0.5)}, "decay_steps"),
    ({"class_name": "PolynomialDecay", "config": dict(initial_learning_rate=1.0, decay_steps=-3)}, "decay_steps"),
    ({"class_name": "PiecewiseConstantDecay", "config": dict(boundaries=[10, 10], values=[1, 2, 3])}, "increase"),
    ({"class_name": "PiecewiseConstantDecay", "config": dict(boundaries=[10, 20], values=[1, 2])}, "len"),
    ({"class_name": "CosineDecay", "config": dict(initial_learning_rate=1.0, decay_steps=10, warmup_steps=5)}, "warm"),
    ({"class_name": "CosineDecay", "config": dict(initial_learning_rate=1.0, decay_steps=10, warmup_target=0.1)}, "warm"),
    ({"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=1.0, decay_steps=10)}, "needs decay_rate"),
    ({"config": {}}, "class_name"),
    ("fast", "not a number"),
]


@pytest.mark.parametrize("value,msg", REFUSED)
def test_refusals(value, msg):
  with pytest.raises(ValueError, match=msg):
    optimizers.resolve("adam", value, 1.0)
  with pytest.raises(ValueError, match=msg):
    I.as_schedule(value, "beta")


def test_interpolation_refusals():
  with pytest.raises(ValueError, match="norm"):
    I.linear(norm=0)
  with pytest.raises(ValueError, match="delay"):
    I.cosine(norm=3, delayIn=-1)
  with pytest.raises(ValueError, match="delay"):
    I.power(norm=3, delayOut=-2)


def test_pickle_round_trip():
  for sch in list(SCHEDULES.values()) + [I.const(2.0)]:
    back = pickle.loads(pickle.dumps(sch))
    assert back == sch and type(back) is type(sch)
    assert [back(s) for s in (0, 7, 99, 12345)] == [sch(s) for s in (0, 7, 99, 12345)]


def test_model_takes_a_beta_schedule():
  import sisua_amd.models as M
  assert M.interpolation is I
  from sisua_amd.config import RVmeta
  sch = I.linear(vmin=0, vmax=10, norm=20, cyclical=True, delayOut=5, delayIn=5)
  m = M.VAE(outputs=RVmeta(50, "zinb", True, "Transcriptomic"), beta=sch)
  assert m.beta_schedule == sch and m.beta == 0.0   # (the value at the model's step: 0 before any fit)
  assert m._make_config().beta == 0.0 and isinstance(m._make_config().beta, float)
  assert pickle.loads(pickle.dumps(m.init_args))["beta"] == sch
  assert M.VAE(outputs=RVmeta(50, "zinb", True, "Transcriptomic"), beta=0.5).beta == 0.5
  assert M.DeepCountAutoencoder(outputs=RVmeta(50, "zinb", True, "Transcriptomic"), beta=sch).beta_schedule == sch
  with pytest.raises(ValueError, match="callable"):
    M.VAE(outputs=RVmeta(50, "zinb", True, "Transcriptomic"), beta=lambda s: 1.0)
