"""Float64 closed forms of the 'bernoulli' and 'normal' heads for the oracle, without touching oracle/.

oracle.sisua_oracle's train_step, forward_backward and marginal_log_prob look up LABEL_LIKELIHOODS, label_planes and label_llk
as module globals when they run.  The wrappers below handle the two kinds themselves and hand every other kind to the
oracle's own functions; `install(monkeypatch)` puts them in place for one test.

  'bernoulli'  1 plane, logits l:                  log p(y) = y l - softplus(l)                       d l = y - sigmoid(l)
  'normal'     2 planes, loc m | raw scale s:      sigma = softplus(s + softplus^-1(1))  ([3P-recall] odin's softplus1)
               log p(y) = -z^2 / 2 - log sigma - log(2 pi) / 2,  z = (y - m) / sigma
               d m = z / sigma,  d s = (z^2 - 1) / sigma * sigmoid(s + softplus^-1(1))
"""
import numpy as np
from scipy.special import expit

from oracle import sisua_oracle as so

KINDS = ("bernoulli", "normal")
_LABEL_LIKELIHOODS = so.LABEL_LIKELIHOODS
_label_planes = so.label_planes
_label_llk = so.label_llk


def bernoulli_llk(y, logits):
  """Elementwise log p(y) and d / d logits."""
  y, l = np.asarray(y, np.float64), np.asarray(logits, np.float64)
  return y * l - np.logaddexp(0.0, l), y - expit(l)


def normal_llk(y, loc, raw_scale):
  """Elementwise log p(y), d / d loc and d / d raw_scale."""
  y, m, s = (np.asarray(a, np.float64) for a in (y, loc, raw_scale))
  t = s + so.SOFTPLUS_INV_1
  sg = np.logaddexp(0.0, t)
  z = (y - m) / sg
  return -0.5 * z * z - np.log(sg) - 0.5 * np.log(2.0 * np.pi), z / sg, (z * z - 1.0) / sg * expit(t)


def label_planes(llk, P=0):
  if llk in KINDS:
    return 1 if llk == "bernoulli" else 2
  return _label_planes(llk, P)


def label_llk(y, raw, llk_kind):
  """Per-cell log-likelihood of one head and its gradient wrt the raw head outputs [B, planes * P]."""
  if llk_kind == "bernoulli":
    ell, d = bernoulli_llk(y, raw)
    return ell.sum(1), d
  if llk_kind == "normal":
    P = raw.shape[1] // 2
    ell, dm, ds = normal_llk(y, raw[:, :P], raw[:, P:])
    return ell.sum(1), np.concatenate([dm, ds], axis=1)
  return _label_llk(y, raw, llk_kind)


def install(monkeypatch):
  """Teach the oracle module the two kinds for the duration of one test."""
  monkeypatch.setattr(so, "LABEL_LIKELIHOODS", tuple(_LABEL_LIKELIHOODS) + KINDS)
  monkeypatch.setattr(so, "label_planes", label_planes)
  monkeypatch.setattr(so, "label_llk", label_llk)


def synth_targets(n, heads, seed=1, probabilities=False):
  """Target arrays in head order: the new kinds' own (0/1 markers, or marker probabilities; bimodal continuous levels),
  every other kind from tests.util.synth_labels."""
  from tests.util import synth_labels
  rng = np.random.default_rng(seed + 100)
  ys = []
  for j, (P, kind) in enumerate(heads):
    if kind == "bernoulli":
      act = rng.normal(size=(n, 1)) * 1.5 + rng.normal(size=(1, P))
      p = expit(act + 0.5 * rng.normal(size=(n, P)))
      ys.append((p if probabilities else (p > 0.5)).astype(np.float32))
    elif kind == "normal":
      on = rng.uniform(size=(n, P)) < 0.4
      ys.append(np.where(on, rng.normal(2.0, 0.5, size=(n, P)), rng.normal(-0.5, 0.8, size=(n, P))).astype(np.float32))
    else:
      ys.append(synth_labels(n, ((P, kind),), seed=seed + j)[0])
  return ys
