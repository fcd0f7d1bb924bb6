"""The optimiser rules of fit(optimizer=...) (sisua_amd.optimizers; include/sisua_hip.h: smx_set_optimizer) on the host: the parsing of a
name / the Keras registry's dict form and every refusal (before any engine is made), the float64 reference of the rules that the GPU tests
compose with oracle.forward_backward -- checked against torch.optim where torch has the same form --, and the checkpoint entries.  CPU only."""
import os
import re

import numpy as np
import pytest
import torch

from sisua_amd import _hip, optimizers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every rule and setting the device builds (name, hyper-parameters)
SETTINGS = {
    "sgd": ("sgd", {}),
    "sgd_momentum": ("sgd", dict(momentum=0.9)),
    "sgd_nesterov": ("sgd", dict(momentum=0.9, nesterov=True)),
    "rmsprop": ("rmsprop", {}),
    "rmsprop_momentum": ("rmsprop", dict(momentum=0.9)),
    "adagrad": ("adagrad", {}),
    "adamax": ("adamax", {}),
}


# ---- the float64 reference --------------------------------------------------------------------------------------------------------
def init_opt(name, params, **hp):
  """The state of a rule that starts fresh: t = 0, slots 2 / 3 ('m' / 'v') zero -- Adagrad's accumulator at initial_accumulator_value."""
  name, full = optimizers.canonical(name, **hp)
  v0 = full["initial_accumulator_value"] if name == "adagrad" else 0.0
  return {"rule": name, "hp": full, "t": 0, "m": {k: np.zeros_like(v) for k, v in params.items()},
          "v": {k: np.full_like(v, v0) for k, v in params.items()}}


def rule_apply(name, hp, lr, t, g, m, v, w):
  """One update of one tensor in float64 (tf.keras 2.x's training ops): (m, v, w) after the clipped gradient g at the rule's step t."""
  if name == "adam":
    m = hp["beta_1"] * m + (1 - hp["beta_1"]) * g
    v = hp["beta_2"] * v + (1 - hp["beta_2"]) * g * g
    lr_t = lr * np.sqrt(1 - hp["beta_2"] ** t) / (1 - hp["beta_1"] ** t)
    return m, v, w - lr_t * m / (np.sqrt(v) + hp["epsilon"])
  if name == "sgd":
    mu = hp["momentum"]
    if mu == 0:
      return m, v, w - lr * g
    m = mu * m - lr * g
    return m, v, (w + mu * m - lr * g) if hp["nesterov"] else (w + m)
  if name == "rmsprop":
    v = hp["rho"] * v + (1 - hp["rho"]) * g * g
    if hp["momentum"] == 0:
      return m, v, w - lr * g / (np.sqrt(v) + hp["epsilon"])
    m = hp["momentum"] * m + lr * g / np.sqrt(v + hp["epsilon"])
    return m, v, w - m
  if name == "adagrad":
    v = v + g * g
    return m, v, w - lr * g / (np.sqrt(v) + hp["epsilon"])
  if name == "adamax":
    m = hp["beta_1"] * m + (1 - hp["beta_1"]) * g
    v = np.maximum(hp["beta_2"] * v, np.abs(g))
    return m, v, w - lr / (1 - hp["beta_1"] ** t) * m / (v + hp["epsilon"])
  raise ValueError(name)


def opt_update(spec, params, grads, opt):
  """oracle.adam_update's contract under the rule of `opt` (init_opt): per-tensor clipnorm (SCALE's tied tensors: the shared variable's
  norm) in front of the rule, in place; returns the pre-clip norms."""
  opt["t"] += 1
  norms = {}
  for name in params:
    g = grads[name]
    nrm = float(np.sqrt((g * g).sum()))
    if spec.model == "scale" and ((name == "prior/loc" and spec.tie_loc) or (name == "prior/scale" and spec.tie_scale)):
      nrm /= np.sqrt(spec.n_components)
    norms[name] = nrm
    if spec.clipnorm > 0 and nrm > spec.clipnorm:
      g = g * (spec.clipnorm / nrm)
    opt["m"][name], opt["v"][name], params[name] = rule_apply(opt["rule"], opt["hp"], spec.lr, opt["t"], g, opt["m"][name],
                                                              opt["v"][name], params[name])
  return norms


# ---- parsing and refusals ---------------------------------------------------------------------------------------------------------
def test_names_and_dict_form():
  for name in ("adam", "Adam", "SGD", "sgd", "RMSprop", "adagrad", "Adamax"):
    assert optimizers.resolve(name, 1e-3, 100.0)[0] == name.lower()
  n, hp, lr, clip = optimizers.resolve({"class_name": "SGD", "config": {"learning_rate": 0.05, "momentum": 0.5, "nesterov": True,
                                                                      "clipnorm": 3.0, "name": "SGD"}}, 1e-3, 100.0)
  assert (n, hp, lr, clip) == ("sgd", dict(momentum=0.5, nesterov=True), 0.05, 3.0)
  n, hp, lr, clip = optimizers.resolve({"class_name": "RMSprop", "config": {"rho": 0.8, "centered": False, "decay": 0.0}}, 2e-3, None)
  assert (n, hp, lr, clip) == ("rmsprop", dict(rho=0.8, momentum=0.0, epsilon=1e-7), 2e-3, None)
  assert optimizers.resolve("adagrad", 1e-3, 1.0)[1] == dict(initial_accumulator_value=0.1, epsilon=1e-7)
  assert optimizers.resolve("adamax", 1e-3, 1.0)[1] == dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7)
  # the device's order of the hyper-parameters (smx_set_optimizer)
  assert list(optimizers.hp_vector("rmsprop", dict(rho=0.8, momentum=0.5, epsilon=1e-6))) == [np.float32(0.8), np.float32(0.5), np.float32(1e-6)]
  assert optimizers.same_rule(("adam", optimizers.hp_dict("adam", np.float32([0.9, 0.999, 1e-7]))), optimizers.canonical("adam"))


BAD = [
    ("nadam", "not built; built: adam, sgd, rmsprop, adagrad, adamax"),
    ("adadelta", "not built"),
    ("ftrl", "not built"),
    (torch.optim.SGD, "give a name"),
    ({"class_name": "Nadam", "config": {}}, "not built"),
    ({"class_name": "RMSprop", "config": {"centered": True}}, "centered"),
    ({"class_name": "Adam", "config": {"amsgrad": True}}, "amsgrad"),
    ({"class_name": "SGD", "config": {"clipvalue": 1.0}}, "clipvalue"),
    ({"class_name": "Adagrad", "config": {"decay": 0.01}}, "decay"),
    ({"class_name": "SGD", "config": {"rho": 0.9}}, "no hyper-parameter 'rho'"),
    ({"class_name": "Adamax", "config": {"momentum": 0.9}}, "no hyper-parameter 'momentum'"),
    ({"config": {}}, "class_name"),
    # epsilon 0 (or a denormal float32, whose reciprocal is inf) makes 0 * inf = NaN of every tensor's zero padding
    ({"class_name": "Adam", "config": {"epsilon": 0.0}}, "epsilon=0.0 must be a normal float32"),
    ({"class_name": "RMSprop", "config": {"epsilon": 0.0}}, "epsilon=0.0 must be a normal float32"),
    ({"class_name": "RMSprop", "config": {"momentum": 0.9, "epsilon": 0.0}}, "epsilon=0.0 must be a normal float32"),
    ({"class_name": "Adagrad", "config": {"epsilon": 0.0}}, "epsilon=0.0 must be a normal float32"),
    ({"class_name": "Adagrad", "config": {"initial_accumulator_value": 0.0, "epsilon": 0.0}}, "epsilon=0.0 must be a normal float32"),
    ({"class_name": "Adamax", "config": {"epsilon": 0.0}}, "epsilon=0.0 must be a normal float32"),
    ({"class_name": "Adam", "config": {"epsilon": 1e-39}}, "must be a normal float32"),
    ({"class_name": "Adamax", "config": {"epsilon": -1e-7}}, "must be a normal float32"),
]


def _toy_fit(monkeypatch, engine_cls, optimizer):
  import sisua_amd.models as M
  from sisua_amd.data import SingleCellOMIC
  from tests.util import synth_counts
  monkeypatch.setattr(M, "Engine", engine_cls)
  sco = SingleCellOMIC(synth_counts(80, 40, seed=5), name="toy")
  model = M.get_model("vae")(outputs=sco.get_rv("transcriptomic", "zinb"), encoder=M.NetConf([16]), decoder=M.NetConf([16]))
  ds = sco.create_dataset(["transcriptomic"], batch_size=16, drop_remainder=True)
  model.fit(ds, metadata=sco, epochs=1, optimizer=optimizer)


class _NoEngine:
  """Fails the test if `fit` reaches the device."""

  def __init__(self, *a, **k):
    raise AssertionError("an engine was made before the optimiser was checked")


class _Reached(Exception):
  pass


class _ReachedEngine:
  def __init__(self, *a, **k):
    raise _Reached()


@pytest.mark.parametrize("optimizer,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_refusals_come_before_any_engine(monkeypatch, optimizer, match):
  """The refusal is raised by fit before an engine (and so any device work) exists: the stub engine must never be built."""
  with pytest.raises(ValueError, match=re.escape(match)):
    _toy_fit(monkeypatch, _NoEngine, optimizer)


@pytest.mark.parametrize("optimizer", ["rmsprop", "SGD", {"class_name": "SGD", "config": {"momentum": 0.9, "nesterov": True}},
                                       {"class_name": "Adamax", "config": {"learning_rate": 0.01}}])
def test_a_built_rule_reaches_the_engine(monkeypatch, optimizer):
  """The control of the refusals: a built rule passes the checks and meets the stub engine."""
  with pytest.raises(_Reached):
    _toy_fit(monkeypatch, _ReachedEngine, optimizer)


def test_entry_points_are_declared_bound_and_exported():
  hdr = open(os.path.join(ROOT, "include", "sisua_hip.h")).read()
  assert re.search(r"int\s+smx_set_optimizer\s*\(\s*smx_model\s*\*\s*m\s*,\s*int32_t\s+rule\s*,\s*const\s+float\s*\*\s*hp\s*,\s*int32_t\s+n_hp\s*\)", hdr)
  for name in ("smx_set_optimizer", "smx_get_optimizer", "smx_k_opt", "smx_k_opt_carrier"):
    assert name in _hip.SIGNATURES
  lib = os.path.join(ROOT, "sisua_amd", "libsisua_hip.so")
  if not os.path.exists(lib):
    pytest.skip("library not built")
  import subprocess
  syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
  for name in ("smx_set_optimizer", "smx_get_optimizer", "smx_k_opt", "smx_k_opt_carrier"):
    assert re.search(rf"\bT {name}\b", syms), name


# ---- the float64 reference against torch.optim ------------------------------------------------------------------------------------
TORCH = {
    "sgd": lambda p, lr: torch.optim.SGD(p, lr=lr),
    "sgd_momentum": lambda p, lr: torch.optim.SGD(p, lr=lr, momentum=0.9),
    "sgd_nesterov": lambda p, lr: torch.optim.SGD(p, lr=lr, momentum=0.9, nesterov=True),
    "rmsprop": lambda p, lr: torch.optim.RMSprop(p, lr=lr, alpha=0.9, eps=1e-7),
    "adagrad": lambda p, lr: torch.optim.Adagrad(p, lr=lr, initial_accumulator_value=0.1, eps=1e-7),
}


@pytest.mark.parametrize("setting", list(TORCH))
def test_reference_rules_match_torch(setting):
  """50 random steps of the float64 rules against torch.optim (float64) to 1e-12.  torch's SGD momentum buffer is the Keras accumulator
  up to the factor -lr (b = mu b + g; a = -lr b), and its Nesterov step w -= lr (g + mu b) is Keras's w += mu a - lr g; torch's RMSprop
  (alpha = rho) and Adagrad take eps outside the square root as Keras does at momentum 0."""
  name, hp = SETTINGS[setting]
  rng = np.random.default_rng(7)
  lr = 0.01
  w = rng.normal(size=(5, 7))
  tw = torch.tensor(w.copy(), dtype=torch.float64, requires_grad=True)
  topt = TORCH[setting]([tw], lr)
  _, full = optimizers.canonical(name, **hp)
  m = np.zeros_like(w)
  v = np.full_like(w, 0.1 if name == "adagrad" else 0.0)
  for t in range(1, 51):
    g = rng.normal(size=w.shape) * (1 + t % 3)
    tw.grad = torch.tensor(g, dtype=torch.float64)
    topt.step()
    m, v, w = rule_apply(name, full, lr, t, g, m, v, w)
    np.testing.assert_allclose(w, tw.detach().numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("setting", ["rmsprop_momentum", "adamax"])
def test_reference_rules_without_a_torch_twin(setting):
  """Adamax and RMSprop with momentum put eps where torch does not (Adamax: m / (u + eps) with u = max(b2 u, |g|), torch: max(b2 u, |g| +
  eps); RMSprop with momentum: lr g / sqrt(ms + eps), torch: g / (sqrt(ms) + eps)), so they are checked against their written formulas,
  element by element over 20 steps."""
  name, hp = SETTINGS[setting]
  _, full = optimizers.canonical(name, **hp)
  rng = np.random.default_rng(3)
  lr, w = 0.01, rng.normal(size=(4, 3))
  m, v = np.zeros_like(w), np.zeros_like(w)
  for t in range(1, 21):
    g = rng.normal(size=w.shape)
    m1, v1, w1 = rule_apply(name, full, lr, t, g, m, v, w)
    for i in np.ndindex(w.shape):
      if name == "adamax":
        em = 0.9 * m[i] + 0.1 * g[i]
        ev = max(0.999 * v[i], abs(g[i]))
        ew = w[i] - (lr / (1 - 0.9 ** t)) * em / (ev + 1e-7)
      else:
        ev = 0.9 * v[i] + 0.1 * g[i] ** 2
        em = 0.9 * m[i] + lr * g[i] / np.sqrt(ev + 1e-7)
        ew = w[i] - em
      assert np.isclose(m1[i], em, rtol=1e-12, atol=0) and np.isclose(v1[i], ev, rtol=1e-12, atol=0) and np.isclose(w1[i], ew, rtol=1e-12, atol=0)
    m, v, w = m1, v1, w1


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------
def test_checkpoint_without_optimiser_entries_reads_as_adam(tmp_path):
  """Every checkpoint written before the rules holds p/ m/ v/ bn/ step only: it is Adam from step 0 with the model's own betas."""
  f = tmp_path / "old.npz"
  np.savez(f, **{"p/enc/0/W": np.zeros((3, 2), np.float32), "m/enc/0/W": np.zeros((3, 2), np.float32),
                 "v/enc/0/W": np.zeros((3, 2), np.float32), "step": np.array(12, np.int64)})
  assert optimizers.from_npz(np.load(f)) == ("adam", None, 0)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_checkpoint_entries_round_trip(tmp_path, setting):
  name, hp = SETTINGS[setting]
  name, full = optimizers.canonical(name, **hp)
  f = tmp_path / "ck.npz"
  np.savez(f, step=np.array(40, np.int64), **optimizers.to_npz(name, full, 17))
  got = optimizers.from_npz(np.load(f))
  assert got[0] == name and got[2] == 17 and optimizers.same_rule(got[:2], (name, full))
