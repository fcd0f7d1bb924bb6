"""Hidden-layer activations without a GPU: the float64 closed forms and derivatives of tests/activations_ref.py against torch autograd
and finite differences, the reference reproducing the unpatched oracle under ReLU, NetConf / ModelConfig parsing, and the sidecar."""
import dataclasses
import pickle

import numpy as np
import pytest
import torch

from oracle import sisua_oracle as so
from tests import activations_ref as ref
from tests.util import make_pair, perturbed_params, synth_counts

Y = np.concatenate([np.linspace(-6.0, 6.0, 241), [-30.0, -12.5, -1e-3, 1e-3, 12.5, 30.0]])

TORCH = {
    "relu": torch.relu, "linear": lambda t: t, "leaky_relu": lambda t: torch.nn.functional.leaky_relu(t, 0.2),
    "elu": torch.nn.functional.elu, "selu": torch.selu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
    "softplus": torch.nn.functional.softplus,
}


@pytest.mark.parametrize("name", ref.NAMES)
def test_closed_forms_against_autograd(name):
  y = Y[np.abs(Y) > 1e-9]   # (the kinks themselves excluded)
  t = torch.tensor(y, dtype=torch.float64, requires_grad=True)
  out = TORCH[name](t)
  if name == "softplus":   # (torch's softplus is linear beyond threshold 20: compare with the exact form there)
    out = torch.logaddexp(torch.zeros_like(t), t)
  (g,) = torch.autograd.grad(out.sum(), t)
  h = ref.act_fwd(name, y)
  assert np.allclose(h, out.detach().numpy(), rtol=1e-12, atol=1e-14)
  assert np.allclose(ref.act_grad(name, h), g.numpy(), rtol=1e-9, atol=1e-12)
  assert np.isfinite(h).all() and np.isfinite(ref.act_grad(name, h)).all()


@pytest.mark.parametrize("name", ref.NAMES)
def test_derivative_against_finite_differences(name):
  y = Y[np.abs(Y) > 1e-2]
  eps = 1e-6
  fd = (ref.act_fwd(name, y + eps) - ref.act_fwd(name, y - eps)) / (2 * eps)
  assert np.allclose(ref.act_grad(name, ref.act_fwd(name, y)), fd, rtol=1e-6, atol=1e-8)


SPECS = {
    "bn": dict(model="vae", n_genes=60, likelihood="zinb", enc_units=(24, 16), dec_units=(20,), latent_dim=5, dropout_enc=0.2,
               dropout_dec=0.2, input_dropout=0.1),
    "nobn": dict(model="scvi", n_genes=50, likelihood="zinbd", enc_units=(24,), dec_units=(20,), latent_dim=4, encl_units=(8,),
                 batchnorm=False, dropout_enc=0.2, dropout_dec=0.2),
}


def _pass(spec, x, rows):
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]]), (len(rows), 1))
  res = so.forward_backward(spec, params, bn, x[rows], so.PhiloxNoise(spec.seed, 0, rows), library=lib)
  return res, bn


@pytest.mark.parametrize("name", list(SPECS))
def test_relu_reference_is_the_oracle_bit_for_bit(monkeypatch, name):
  spec, _ = make_pair(**SPECS[name])
  x = synth_counts(40, spec.n_genes, seed=2)
  rows = np.arange(32)
  a, bn_a = _pass(spec, x, rows)
  with monkeypatch.context() as mp:
    ref.install(mp)
    assert so._mlp_fwd is ref._mlp_fwd
    b, bn_b = _pass(spec, x, rows)
  assert a["loss"] == b["loss"]
  assert set(a["grads"]) == set(b["grads"])
  for k in a["grads"]:
    assert np.array_equal(a["grads"][k], b["grads"][k]), k
  for k in bn_a:
    assert np.array_equal(bn_a[k], bn_b[k]), k


def test_reference_changes_with_the_activation(monkeypatch):
  spec, _ = make_pair(**SPECS["bn"])
  x = synth_counts(40, spec.n_genes, seed=2)
  a, _ = _pass(spec, x, np.arange(32))
  ref.install(monkeypatch, enc="tanh", dec="elu")
  b, _ = _pass(spec, x, np.arange(32))
  assert a["loss"] != b["loss"] and np.isfinite(b["loss"])


def test_reference_gradient_against_finite_differences(monkeypatch):
  """The patched backward is the derivative of the patched forward (eval mode, one coordinate per tensor of each network)."""
  ref.install(monkeypatch, enc="selu", dec="softplus")
  spec, _ = make_pair(**dict(SPECS["bn"], dropout_enc=0.0, dropout_dec=0.0, input_dropout=0.0))
  x = synth_counts(24, spec.n_genes, seed=4)
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]]), (24, 1))
  noise = so.PhiloxNoise(spec.seed, 0, np.arange(24))
  f = lambda p: so.forward_backward(spec, p, bn, x, noise, library=lib, training=False)
  g = f(params)["grads"]
  for key in ("enc0/gamma", "enc1/W", "dec0/beta"):
    idx = (0,) * params[key].ndim
    h = 1e-6
    pp, pm = {k: v.copy() for k, v in params.items()}, {k: v.copy() for k, v in params.items()}
    pp[key][idx] += h
    pm[key][idx] -= h
    fd = (f(pp)["loss"] - f(pm)["loss"]) / (2 * h)
    assert np.isclose(g[key][idx], fd, rtol=1e-5, atol=1e-7), (key, g[key][idx], fd)


# ---- names ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given,want", [("relu", "relu"), ("ReLU", "relu"), ("linear", "linear"), (None, "linear"), ("identity", "linear"),
                                        ("Leaky_ReLU", "leaky_relu"), ("elu", "elu"), ("SELU", "selu"), ("tanh", "tanh"),
                                        ("sigmoid", "sigmoid"), ("Softplus", "softplus")])
def test_netconf_names(given, want):
  from sisua_amd.config import NetConf
  assert NetConf([8], activation=given).activation == want


@pytest.mark.parametrize("given", ["swish", "silu", "gelu", "softmax", "relu6", "", np.tanh, torch.relu, 3])
def test_netconf_refuses_what_is_not_built(given):
  from sisua_amd.config import NetConf
  with pytest.raises(ValueError, match="relu, linear, leaky_relu, elu, selu, tanh, sigmoid, softplus"):
    NetConf([8], activation=given)


def test_model_config_carries_the_activations():
  from sisua_amd.config import ModelConfig
  a = ModelConfig(n_genes=10)
  assert (a.enc_activation, a.dec_activation, a.encl_activation) == ("relu", "relu", "relu")
  for f in ("enc_activation", "dec_activation", "encl_activation"):
    b = dataclasses.replace(a, **{f: "elu"})
    assert b != a and getattr(b, f) == "elu"
  assert ModelConfig(n_genes=10, dec_activation="TANH").dec_activation == "tanh"
  with pytest.raises(ValueError):
    ModelConfig(n_genes=10, enc_activation="gelu")


def test_models_pass_each_networks_activation():
  import sisua_amd.models as M
  from sisua_amd.config import NetConf, RVmeta
  m = M.VAE(RVmeta(30, "zinb", name="x"), encoder=NetConf([16], activation="elu"), decoder=NetConf([16], activation="tanh"))
  c = m._make_config()
  assert (c.enc_activation, c.dec_activation) == ("elu", "tanh")
  s = M.SCVI(RVmeta(30, "zinbd", name="x"), encoder=NetConf([16], activation="selu"), encoder_l=NetConf([8], activation="sigmoid"),
             decoder=NetConf([16], activation="softplus"))
  c = s._make_config()
  assert (c.enc_activation, c.dec_activation, c.encl_activation) == ("selu", "softplus", "sigmoid")
  assert M.VAE(RVmeta(30, "zinb", name="x"))._make_config().enc_activation == "relu"


def test_experiment_passes_the_activation():
  from sisua_amd import train
  from sisua_amd.config import NetConf
  n = train._from_config({"units": [32], "batchnorm": True, "dropout": 0.1, "activation": "tanh"}, NetConf)
  assert n.activation == "tanh"


# ---- the sidecar ----------------------------------------------------------------------------------------------------------------------
def test_metamodel_round_trip_keeps_each_networks_activation(tmp_path):
  import sisua_amd.models as M
  from sisua_amd.config import NetConf, RVmeta
  kw = dict(outputs=RVmeta(30, "zinbd", name="x"), encoder=NetConf([16], activation="elu"), encoder_l=NetConf([8], activation="tanh"),
            decoder=NetConf([16], activation="leaky_relu"))
  plain = M._to_plain(kw)
  assert plain["encoder"]["activation"] == "elu" and plain["decoder"]["activation"] == "leaky_relu"
  back = M._from_plain(pickle.loads(pickle.dumps(plain)))
  s = M.SCVI(**back)
  c = s._make_config()
  assert (c.enc_activation, c.dec_activation, c.encl_activation) == ("elu", "leaky_relu", "tanh")


def test_reference_written_netconf_keeps_its_activation():
  """An odin NetConf in a sidecar the reference wrote: the shim's attribute dict carries activation='tanh'."""
  import sisua_amd.models as M
  Shim = type("NetConf", (M._Shim,), {"_shim_name": "NetConf"})
  v = Shim()
  v.__setstate__(dict(units=(32, 16), batchnorm=True, dropout=0.1, input_dropout=0.0, activation="tanh", name="Encoder"))
  rec = M._shim_to_record({"encoder": v})["encoder"]
  assert rec.activation == "tanh" and rec.units == (32, 16)
  w = Shim()
  w.__setstate__(dict(units=(8,)))
  assert M._shim_to_record(w).activation == "relu"


def test_to_dict_stays_a_spec_while_relu():
  from sisua_amd.config import ModelConfig
  a = ModelConfig(n_genes=10)
  assert so.Spec(**a.to_dict()).n_genes == 10
  d = dataclasses.replace(a, enc_activation="elu").to_dict()
  assert d["enc_activation"] == "elu" and "dec_activation" not in d
  with pytest.raises(TypeError):
    so.Spec(**d)
