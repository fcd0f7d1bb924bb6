"""The optimiser rules of `fit(optimizer=...)` / `Engine.set_optimizer` (include/sisua_hip.h: smx_set_optimizer).

The reference hands `train.optimizer` of configs/base.yaml to the Keras optimiser registry through odin's trainer: a name or the
registry's dict form `{"class_name": ..., "config": {...}}`.  The rules built on the device are tf.keras 2.x's Adam, SGD, RMSprop,
Adagrad and Adamax with their defaults; every other name, and every setting these rules take in Keras but the device does not
(centered RMSprop, AMSGrad, clipvalue, decay), is refused here, before any device work.  Host code only."""
from typing import Dict, Optional, Tuple

import numpy as np

from sisua_amd import interpolation

# name -> (smx_optimizer, ordered hyper-parameters with the tf.keras 2.x defaults; Adam's defaults are smx_config's)
RULES: Dict[str, Tuple[int, Tuple[Tuple[str, float], ...]]] = {
    "adam": (0, (("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7))),
    "sgd": (1, (("momentum", 0.0), ("nesterov", False))),
    "rmsprop": (2, (("rho", 0.9), ("momentum", 0.0), ("epsilon", 1e-7))),
    "adagrad": (3, (("initial_accumulator_value", 0.1), ("epsilon", 1e-7))),
    "adamax": (4, (("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7))),
}
NAMES = {v[0]: k for k, v in RULES.items()}
# settings Keras has that the device rules do not: refused when they would change the update
_UNBUILT = {"centered": False, "amsgrad": False, "clipvalue": None, "decay": 0.0, "global_clipnorm": None}


def _refuse_unbuilt(name: str, key: str, value):
  if key in _UNBUILT and value is not None and value != _UNBUILT[key] and not (key == "decay" and float(value) == 0.0):
    raise ValueError(f"optimizer {name!r}: {key}={value!r} is not built (out of scope: centered RMSprop, AMSGrad, clipvalue, "
                     "decay schedules)")


def canonical(name: str, **hp) -> Tuple[str, Dict[str, float]]:
  """(rule name, every hyper-parameter of the rule with defaults filled in) -- ValueError for a rule that is not built or a key the
  rule does not have."""
  if not isinstance(name, str):
    raise ValueError(f"optimizer {name!r}: give a name or the registry's dict form; built: {', '.join(RULES)}")
  key = name.lower()
  if key not in RULES:
    raise ValueError(f"optimizer {name!r} is not built; built: {', '.join(RULES)}")
  _, spec = RULES[key]
  known = dict(spec)
  out = dict(spec)
  for k, v in hp.items():
    _refuse_unbuilt(key, k, v)
    if k in _UNBUILT:
      continue
    if k not in known:
      raise ValueError(f"optimizer {key!r} has no hyper-parameter {k!r} (it takes {', '.join(known)})")
    out[k] = bool(v) if isinstance(known[k], bool) else float(v)
  for k, v in out.items():
    if not isinstance(v, bool) and not np.isfinite(v):
      raise ValueError(f"optimizer {key!r}: {k}={v!r} is not finite")
  # (at epsilon 0, or a denormal float32 whose reciprocal is inf, the device's update makes 0 * inf = NaN of every tensor's zero padding,
  # whatever Adagrad's accumulator starts at: its initial value goes into the logical elements only)
  if "epsilon" in out and not np.float32(out["epsilon"]) >= np.finfo(np.float32).tiny:
    raise ValueError(f"optimizer {key!r}: epsilon={out['epsilon']!r} must be a normal float32 (>= 2^-126)")
  return key, out


def resolve(optimizer, learning_rate, clipnorm: Optional[float]):
  """fit()'s `optimizer` argument -> (rule name, hyper-parameters, learning-rate schedule, clipnorm).  The dict form's `learning_rate` (or
  `lr`) and `clipnorm` override fit's own arguments.  The learning rate is a number or a schedule (sisua_amd.interpolation: a Keras
  schedule in the registry's dict form or as a tf.keras object, or an interpolation); it comes back as an interpolation.Schedule record,
  a const one for a number (equal to that number)."""
  if isinstance(optimizer, dict):
    if "class_name" not in optimizer:
      raise ValueError("optimizer dict needs 'class_name' (the Keras registry's form {'class_name': ..., 'config': {...}})")
    extra = set(optimizer) - {"class_name", "config"}
    if extra:
      raise ValueError(f"optimizer dict: unexpected keys {sorted(extra)}")
    cfg = dict(optimizer.get("config") or {})
    cfg.pop("name", None)   # (the Keras object's display name)
    for k in ("learning_rate", "lr"):
      if k in cfg:
        learning_rate = cfg.pop(k)
    if "clipnorm" in cfg:
      clipnorm = cfg.pop("clipnorm")
    name, hp = canonical(optimizer["class_name"], **cfg)
  else:
    name, hp = canonical(optimizer)
  return name, hp, interpolation.as_schedule(learning_rate, "learning_rate"), clipnorm


def hp_vector(name: str, hp: Dict[str, float]) -> np.ndarray:
  """the hyper-parameters in smx_set_optimizer's order (float32)"""
  return np.array([float(hp[k]) for k, _ in RULES[name][1]], np.float32)


def hp_dict(name: str, vec) -> Dict[str, float]:
  """smx_get_optimizer's vector -> {key: value} of the rule"""
  spec = RULES[name][1]
  return {k: (bool(vec[i]) if isinstance(d, bool) else float(vec[i])) for i, (k, d) in enumerate(spec)}


def same_rule(a: Tuple[str, Dict[str, float]], b: Tuple[str, Dict[str, float]]) -> bool:
  """the same rule with the same hyper-parameters at float32 precision (what the device holds)"""
  return a[0] == b[0] and np.array_equal(hp_vector(a[0], a[1]), hp_vector(b[0], b[1]))


# ---- checkpoints (models.save_weights / load_weights) ----------------------------------------------------------------------------
def to_npz(name: str, hp: Dict[str, float], t0: int) -> Dict[str, np.ndarray]:
  """the optimiser's entries of a checkpoint (beside m/ and v/, which hold the rule's slots 2 / 3)"""
  return {"opt/name": np.array(name), "opt/hp": hp_vector(name, hp), "opt/t0": np.array(int(t0), np.int64)}


def from_npz(z) -> Tuple[str, Optional[Dict[str, float]], int]:
  """(rule name, hyper-parameters, t0) of a checkpoint; one without the entries (every checkpoint written before the rules) is Adam
  from step 0 with the model's own betas (hyper-parameters None)."""
  files = set(z.files if hasattr(z, "files") else z.keys())
  if "opt/name" not in files:
    return "adam", None, 0
  name = str(np.asarray(z["opt/name"]).item())
  name, hp = canonical(name, **hp_dict(name, np.asarray(z["opt/hp"], np.float64)))
  return name, hp, int(np.asarray(z["opt/t0"]).item())
