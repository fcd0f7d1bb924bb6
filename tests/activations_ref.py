"""Float64 hidden-layer activations for the oracle, without touching oracle/.

oracle.sisua_oracle's forward_backward, train_step, dp_train_step, marginal_log_prob and posterior_llk call the module globals
_mlp_fwd / _mlp_bwd when they run.  The copies below are the oracle's, with the activation looked up by layer prefix ('enc', 'encl',
'dec'); `install(monkeypatch, enc=..., dec=..., encl=...)` puts them in place for one test.  With every network on 'relu' they compute
exactly what the oracle's own functions compute.

  name         h = act(y)                                  d h / d y from h
  relu         max(y, 0)                                   h > 0
  linear       y                                           1
  leaky_relu   y > 0 ? y : 0.2 y      ([3P-recall] tf.nn.leaky_relu's default slope)   h > 0 ? 1 : 0.2
  elu          y > 0 ? y : exp(y) - 1                      h > 0 ? 1 : h + 1
  selu         lam (y > 0 ? y : alpha (exp(y) - 1))        h > 0 ? lam : h + lam alpha
  tanh         tanh(y)                                     1 - h^2
  sigmoid      1 / (1 + exp(-y))                           h (1 - h)
  softplus     log(1 + exp(y))                             1 - exp(-h)
lam = 1.0507009873554805, alpha = 1.6732632423543772 ([3P-recall] the Keras SELU constants).  The kink log (oracle _log_kink) takes
the pre-activations of the activations with a kink only: relu, leaky_relu, selu.
"""
import numpy as np
from scipy.special import expit

from oracle import sisua_oracle as so

NAMES = ("relu", "linear", "leaky_relu", "elu", "selu", "tanh", "sigmoid", "softplus")
KINKED = ("relu", "leaky_relu", "selu")
LEAKY_SLOPE = 0.2
SELU_LAMBDA = 1.0507009873554805
SELU_ALPHA = 1.6732632423543772

_ACTS = {"enc": "relu", "encl": "relu", "dec": "relu"}


def act_fwd(name, y):
  y = np.asarray(y, dtype=np.float64)
  if name == "relu":
    return np.maximum(y, 0.0)
  if name == "linear":
    return y.copy()
  if name == "leaky_relu":
    return np.where(y > 0, y, LEAKY_SLOPE * y)
  if name == "elu":
    return np.where(y > 0, y, np.expm1(np.minimum(y, 0.0)))
  if name == "selu":
    return SELU_LAMBDA * np.where(y > 0, y, SELU_ALPHA * np.expm1(np.minimum(y, 0.0)))
  if name == "tanh":
    return np.tanh(y)
  if name == "sigmoid":
    return expit(y)
  if name == "softplus":
    return np.logaddexp(0.0, y)
  raise ValueError(name)


def act_grad(name, h):
  """d act / d y, from the output h = act_fwd(name, y)."""
  h = np.asarray(h, dtype=np.float64)
  if name == "relu":
    return (h > 0).astype(np.float64)
  if name == "linear":
    return np.ones_like(h)
  if name == "leaky_relu":
    return np.where(h > 0, 1.0, LEAKY_SLOPE)
  if name == "elu":
    return np.where(h > 0, 1.0, h + 1.0)
  if name == "selu":
    return np.where(h > 0, SELU_LAMBDA, h + SELU_LAMBDA * SELU_ALPHA)
  if name == "tanh":
    return 1.0 - h * h
  if name == "sigmoid":
    return h * (1.0 - h)
  if name == "softplus":
    return -np.expm1(-h)
  raise ValueError(name)


def _mlp_fwd(spec, params, bn_state, prefix, units, h, training, noise, stream0, p_drop, new_bn):
  name = _ACTS[prefix]
  caches = []
  for i, _ in enumerate(units):
    W = params[f"{prefix}{i}/W"]
    pre = h @ W
    c = {"h_in": h}
    if spec.batchnorm:
      mm, mv = bn_state[f"{prefix}{i}/moving_mean"], bn_state[f"{prefix}{i}/moving_var"]
      if training:
        mu, var = pre.mean(0), pre.var(0)
        new_bn[f"{prefix}{i}/moving_mean"] = mm * spec.bn_momentum + mu * (1 - spec.bn_momentum)
        new_bn[f"{prefix}{i}/moving_var"] = mv * spec.bn_momentum + var * (1 - spec.bn_momentum)
        new_bn[f"{prefix}{i}/batch_mean"] = mu
        new_bn[f"{prefix}{i}/batch_var"] = var
      else:
        mu, var = mm, mv
      inv = 1.0 / np.sqrt(var + spec.bn_eps)
      xhat = (pre - mu) * inv
      y = params[f"{prefix}{i}/gamma"] * xhat + params[f"{prefix}{i}/beta"]
      c.update(xhat=xhat, inv=inv)
    else:
      y = pre + params[f"{prefix}{i}/b"]
    if name == "relu":   # (the oracle's own lines)
      act = np.maximum(y, 0.0)
      so._log_kink(y)
    else:
      act = act_fwd(name, y)
      if name in KINKED:
        so._log_kink(y)
    mask = noise.dropout(stream0 + i, y.shape[1], p_drop) if training else 1.0
    h = act * mask
    c.update(pos=(y > 0) if name == "relu" else act_grad(name, act), mask=mask)
    caches.append(c)
  return h, caches


def _mlp_bwd(spec, params, prefix, units, caches, dh, grads, training):
  for i in reversed(range(len(units))):
    c = caches[i]
    dy = dh * c["mask"] * c["pos"]
    if spec.batchnorm:
      gamma = params[f"{prefix}{i}/gamma"]
      grads[f"{prefix}{i}/gamma"] = (dy * c["xhat"]).sum(0)
      grads[f"{prefix}{i}/beta"] = dy.sum(0)
      dxh = dy * gamma
      if training:
        B = dy.shape[0]
        dpre = c["inv"] / B * (B * dxh - dxh.sum(0) - c["xhat"] * (dxh * c["xhat"]).sum(0))
      else:
        dpre = dxh * c["inv"]
    else:
      grads[f"{prefix}{i}/b"] = dy.sum(0)
      dpre = dy
    grads[f"{prefix}{i}/W"] = c["h_in"].T @ dpre
    dh = dpre @ params[f"{prefix}{i}/W"].T
  return dh


def install(monkeypatch, enc="relu", dec="relu", encl="relu"):
  """Give the oracle these hidden-layer activations for the duration of one test."""
  for n in (enc, dec, encl):
    if n not in NAMES:
      raise ValueError(n)
  monkeypatch.setitem(_ACTS, "enc", enc)
  monkeypatch.setitem(_ACTS, "dec", dec)
  monkeypatch.setitem(_ACTS, "encl", encl)
  monkeypatch.setattr(so, "_mlp_fwd", _mlp_fwd)
  monkeypatch.setattr(so, "_mlp_bwd", _mlp_bwd)
