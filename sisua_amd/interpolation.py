"""Step-dependent weights: the KL weight `beta` of a model and the learning rate of `fit` (include/sisua_hip.h: smx_set_schedule).

Interpolations ([3P-recall] odin's `interpolation`, which the reference re-exports from sisua.models for its KL weight and builds as
`interpolation.const(vmax=1)` / `interpolation.linear(vmin=0, vmax=10, norm=20, cyclical=True, delayOut=5, delayIn=5)`), keyed by the
model's global step -- the 0-based index of the update in flight, the step that keys the Philox noise and is saved in checkpoints:

- `const(vmax)` is `vmax`.
- `linear`, `power` (`power=2`) and `cosine` take `(vmin=0, vmax=1, norm, cyclical=False, delayIn=0, delayOut=0)`.  With
  P = delayIn + norm + delayOut, p = step % P when cyclical, else step; a = 0 while p < delayIn, else min((p - delayIn) / norm, 1).
  The value is vmin + (vmax - vmin) f(a) with f(a) = a, a ** power or 0.5 - 0.5 cos(pi a); at a == 0 it is vmin and at a == 1 vmax
  exactly (no arithmetic on the end points).

Learning-rate schedules, the tf.keras 2.x formulas and defaults ([3P-recall] keras.optimizers.schedules), keyed by the optimiser's own
iteration count step - t0 (t0: the step at which the rule's state began, smx_get_optimizer): ExponentialDecay, InverseTimeDecay,
PiecewiseConstantDecay (value i while step <= boundaries[i]), PolynomialDecay (`cycle`) and CosineDecay.  They are given in the Keras
registry's dict form `{'class_name': ..., 'config': {...}}` or as any object whose class name is one of these and whose `get_config()`
returns that config (a tf.keras schedule).  Either kind may be given for either target: `as_schedule` lowers every form to one record.

Every value is computed in float64 and rounded once to float32, here and in the library's evaluator (smx_schedule_eval), operation for
operation.  Python callables are refused: a step function cannot run on the device."""
import math
from typing import Sequence, Tuple

import numpy as np

__all__ = ["Interpolation", "Schedule", "const", "linear", "power", "cosine", "as_schedule", "KERAS"]

# smx_schedule_kind
CONST, LINEAR, POWER, COSINE, EXP_DECAY, INVTIME_DECAY, PIECEWISE, POLY_DECAY, COSINE_DECAY = range(9)
KERAS = ("ExponentialDecay", "InverseTimeDecay", "PiecewiseConstantDecay", "PolynomialDecay", "CosineDecay")
BUILT = "built: const, linear, power, cosine (sisua_amd.interpolation); " + ", ".join(KERAS) + " (tf.keras)"


def _value(kind: int, p: Sequence[float], step: float) -> float:
  """the float64 value at `step` -- smx_schedule.hip's sched_value, operation for operation"""
  if kind == CONST:
    return p[0]
  if kind in (LINEAR, POWER, COSINE):
    vmin, vmax, norm, din, dout = p[0], p[1], p[2], p[4], p[5]
    x = math.fmod(step, din + norm + dout) if p[3] != 0.0 else step
    if x < din:
      return vmin
    a = (x - din) / norm
    if a >= 1.0:
      return vmax
    if a == 0.0:
      return vmin
    f = a if kind == LINEAR else math.pow(a, p[6]) if kind == POWER else 0.5 - 0.5 * math.cos(math.pi * a)
    return vmin + (vmax - vmin) * f
  if kind in (EXP_DECAY, INVTIME_DECAY):
    q = step / p[1]
    if p[3] != 0.0:
      q = math.floor(q)
    return p[0] * math.pow(p[2], q) if kind == EXP_DECAY else p[0] / (1.0 + p[2] * q)
  if kind == PIECEWISE:
    k = (len(p) - 1) // 2
    for i in range(k):
      if step <= p[i]:
        return p[k + i]
    return p[2 * k]
  if kind == POLY_DECAY:
    s, ds = step, p[1]
    if p[4] != 0.0:
      ds = ds * (1.0 if s == 0.0 else math.ceil(s / ds))
    else:
      s = min(s, ds)
    return (p[0] - p[2]) * math.pow(1.0 - s / ds, p[3]) + p[2]
  if kind == COSINE_DECAY:
    s = min(step, p[1])
    c = 0.5 * (1.0 + math.cos(math.pi * (s / p[1])))
    return p[0] * ((1.0 - p[2]) * c + p[2])
  raise ValueError(f"schedule kind {kind!r} is not built; {BUILT}")


def _check(kind: int, p: Tuple[float, ...]):
  """smx_schedule.hip's sched_check: ValueError naming what is wrong"""
  if not all(math.isfinite(v) for v in p):
    raise ValueError(f"schedule parameters must be finite: {p}")
  if kind in (LINEAR, POWER, COSINE):
    if not p[2] > 0:
      raise ValueError(f"interpolation: norm must be > 0, given {p[2]!r}")
    if p[4] < 0 or p[5] < 0:
      raise ValueError(f"interpolation: delayIn / delayOut must be >= 0, given {p[4]!r} / {p[5]!r}")
  elif kind in (EXP_DECAY, INVTIME_DECAY, POLY_DECAY, COSINE_DECAY):
    if not p[1] > 0:
      raise ValueError(f"learning-rate schedule: decay_steps must be > 0, given {p[1]!r}")
  elif kind == PIECEWISE:
    k = (len(p) - 1) // 2
    if any(not p[i] > p[i - 1] for i in range(1, k)):
      raise ValueError(f"PiecewiseConstantDecay: boundaries must increase, given {list(p[:k])}")


class Schedule:
  """One schedule record: smx_schedule_kind and its float64 parameters in smx_set_schedule's order.  Picklable; equal records compare
  equal, and a const record equals (and converts to) its number.  `value(step)` is the float64 value, `__call__(step)` the float32 one a training step uses."""

  def __init__(self, kind: int, params: Sequence[float]):
    self.kind = int(kind)
    self.params = tuple(float(v) for v in params)
    _check(self.kind, self.params)

  def value(self, step) -> float:
    return _value(self.kind, self.params, float(step))

  def __call__(self, step) -> float:
    return float(np.float32(self.value(step)))

  def record(self) -> "Schedule":
    return self

  def __eq__(self, other):   # (a const record is its value: it equals that number)
    if isinstance(other, Schedule):
      return (self.kind, self.params) == (other.kind, other.params)
    if self.kind == CONST and isinstance(other, (int, float, np.integer, np.floating)) and not isinstance(other, (bool, np.bool_)):
      return self.params[0] == float(other)
    return NotImplemented

  def __hash__(self):
    return hash(self.params[0]) if self.kind == CONST else hash((self.kind, self.params))

  def __float__(self):
    if self.kind != CONST:
      raise TypeError(f"{self!r} depends on the step: evaluate it at a step")
    return self.params[0]

  def __repr__(self):
    return f"Schedule(kind={self.kind}, params={self.params})"


class Interpolation(Schedule):
  """An interpolation of `interpolation.const / linear / power / cosine` (the odin names)."""

  def __init__(self, name: str, kind: int, params: Sequence[float], **kw):
    self.name = name
    self.kwargs = kw
    super().__init__(kind, params)

  @property
  def vmin(self):
    return self.kwargs.get("vmin", self.kwargs.get("vmax"))

  @property
  def vmax(self):
    return self.kwargs["vmax"]

  def __repr__(self):
    return f"interpolation.{self.name}(" + ", ".join(f"{k}={v!r}" for k, v in self.kwargs.items()) + ")"


def const(vmax=1.0) -> Interpolation:
  return Interpolation("const", CONST, (vmax,), vmax=vmax)


def _ramp(name, kind, vmin, vmax, norm, cyclical, delayIn, delayOut, extra=()):
  kw = dict(vmin=vmin, vmax=vmax, norm=norm, cyclical=bool(cyclical), delayIn=delayIn, delayOut=delayOut)
  if extra:
    kw["power"] = extra[0]
  return Interpolation(name, kind, (vmin, vmax, norm, 1.0 if cyclical else 0.0, delayIn, delayOut) + tuple(extra), **kw)


def linear(vmin=0.0, vmax=1.0, norm=1, cyclical=False, delayIn=0, delayOut=0) -> Interpolation:
  return _ramp("linear", LINEAR, vmin, vmax, norm, cyclical, delayIn, delayOut)


def power(vmin=0.0, vmax=1.0, norm=1, cyclical=False, delayIn=0, delayOut=0, power=2) -> Interpolation:
  return _ramp("power", POWER, vmin, vmax, norm, cyclical, delayIn, delayOut, (power,))


def cosine(vmin=0.0, vmax=1.0, norm=1, cyclical=False, delayIn=0, delayOut=0) -> Interpolation:
  return _ramp("cosine", COSINE, vmin, vmax, norm, cyclical, delayIn, delayOut)


# ---- the Keras learning-rate schedules -------------------------------------------------------------------------------------------
# class name -> (kind, (key, default or _REQ) in smx_set_schedule's order)
_REQ = object()
_KERAS_SPEC = {
    "ExponentialDecay": (EXP_DECAY, (("initial_learning_rate", _REQ), ("decay_steps", _REQ), ("decay_rate", _REQ),
                                     ("staircase", False))),
    "InverseTimeDecay": (INVTIME_DECAY, (("initial_learning_rate", _REQ), ("decay_steps", _REQ), ("decay_rate", _REQ),
                                         ("staircase", False))),
    "PolynomialDecay": (POLY_DECAY, (("initial_learning_rate", _REQ), ("decay_steps", _REQ), ("end_learning_rate", 0.0001),
                                     ("power", 1.0), ("cycle", False))),
    "CosineDecay": (COSINE_DECAY, (("initial_learning_rate", _REQ), ("decay_steps", _REQ), ("alpha", 0.0))),
}
# settings of a newer CosineDecay that are not built: refused unless at their defaults
_COSINE_WARMUP = {"warmup_target": None, "warmup_steps": 0}


def _keras(class_name: str, config: dict) -> Schedule:
  cfg = dict(config or {})
  cfg.pop("name", None)
  if class_name == "PiecewiseConstantDecay":
    extra = set(cfg) - {"boundaries", "values"}
    if extra or "boundaries" not in cfg or "values" not in cfg:
      raise ValueError(f"PiecewiseConstantDecay takes boundaries and values, given {sorted(config or {})}")
    b = [float(v) for v in np.asarray(cfg["boundaries"], np.float64).ravel()]
    v = [float(x) for x in np.asarray(cfg["values"], np.float64).ravel()]
    if len(v) != len(b) + 1:
      raise ValueError(f"PiecewiseConstantDecay: len(values) must be len(boundaries) + 1, given {len(v)} and {len(b)}")
    return Schedule(PIECEWISE, b + v)
  if class_name not in _KERAS_SPEC:
    raise ValueError(f"learning-rate schedule {class_name!r} is not built; {BUILT}")
  kind, spec = _KERAS_SPEC[class_name]
  if class_name == "CosineDecay":
    for k, d in _COSINE_WARMUP.items():
      if k in cfg and cfg.pop(k) not in (d, None if d is None else float(d)):
        raise ValueError(f"CosineDecay: {k} is not built (warm-up); {BUILT}")
  known = {k for k, _ in spec}
  extra = set(cfg) - known
  if extra:
    raise ValueError(f"{class_name} has no setting {sorted(extra)} (it takes {', '.join(k for k, _ in spec)})")
  out = []
  for k, d in spec:
    if k not in cfg and d is _REQ:
      raise ValueError(f"{class_name} needs {k}")
    v = cfg.get(k, d)
    out.append(float(bool(v)) if isinstance(v, (bool, np.bool_)) else float(v))
  return Schedule(kind, out)


def as_schedule(value, what: str = "value") -> Schedule:
  """Every accepted form -> a Schedule record: a number (const), an interpolation, a Schedule, the Keras registry's dict form or an
  object with a Keras schedule's class name and `get_config()`.  ValueError for anything else, Python callables included."""
  if isinstance(value, Schedule):
    return value
  if isinstance(value, (bool, np.bool_)):
    raise ValueError(f"{what}: {value!r} is not a number or a schedule; {BUILT}")
  if isinstance(value, (int, float, np.integer, np.floating)) or (isinstance(value, np.ndarray) and value.ndim == 0):
    return Schedule(CONST, (float(value),))
  if isinstance(value, dict):
    if "class_name" not in value:
      raise ValueError(f"{what}: a schedule dict needs 'class_name' (the Keras registry's form {{'class_name': ..., 'config': {{...}}}})")
    extra = set(value) - {"class_name", "config"}
    if extra:
      raise ValueError(f"{what}: unexpected keys {sorted(extra)} in the schedule dict")
    return _keras(str(value["class_name"]), value.get("config") or {})
  name = type(value).__name__
  if hasattr(value, "get_config") and name in KERAS:
    return _keras(name, value.get_config())
  if callable(value):
    raise ValueError(f"{what}: a Python callable ({name}) cannot run on the device; {BUILT}")
  raise ValueError(f"{what}: {value!r} is not a number or a schedule; {BUILT}")
