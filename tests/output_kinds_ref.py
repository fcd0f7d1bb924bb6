"""Float64 closed forms of the 'bernoulli' and 'normal' gene outputs for the oracle, without touching oracle/.

oracle.sisua_oracle's Spec, forward_backward, marginal_log_prob and posterior_llk look up OUTPUT_POSTERIORS, n_params_per_gene and
count_llk as module globals when they run.  The wrappers below handle the two kinds themselves (through head_kinds_ref's element forms,
the ones the label heads are checked against) and hand every other likelihood to the oracle's own functions; `install(monkeypatch)`
puts them in place for one test.  Neither kind has the count constant -lgamma(x + 1): count_llk returns the density itself.

  'bernoulli'  1 plane, logits l:                  log p(x) = x l - softplus(l)
  'normal'     2 planes, loc m | raw scale s:      sigma = softplus(s + softplus^-1(1)),  log p(x) = -z^2 / 2 - log sigma - log(2 pi) / 2
"""
import numpy as np
from scipy.special import expit

from oracle import sisua_oracle as so
from tests import head_kinds_ref as hk

KINDS = ("bernoulli", "normal")
_OUTPUT_POSTERIORS = so.OUTPUT_POSTERIORS
_n_params_per_gene = so.n_params_per_gene
_count_llk = so.count_llk


def n_params_per_gene(likelihood):
  if likelihood in KINDS:
    return 1 if likelihood == "bernoulli" else 2
  return _n_params_per_gene(likelihood)


def count_llk(x, p, likelihood, direct=False):
  """Elementwise log p(x | planes) and its gradients wrt each raw plane."""
  if likelihood == "bernoulli":
    ell, d = hk.bernoulli_llk(x, p[0])
    return ell, [d]
  if likelihood == "normal":
    ell, dm, ds = hk.normal_llk(x, p[0], p[1])
    return ell, [dm, ds]
  return _count_llk(x, p, likelihood, direct)


def install(monkeypatch):
  """Teach the oracle module the two gene-output kinds (and, through head_kinds_ref, the two head kinds) for one test."""
  hk.install(monkeypatch)
  monkeypatch.setattr(so, "OUTPUT_POSTERIORS", tuple(_OUTPUT_POSTERIORS) + KINDS)
  monkeypatch.setattr(so, "n_params_per_gene", n_params_per_gene)
  monkeypatch.setattr(so, "count_llk", count_llk)


def synth_binary(n, G, seed=0, probabilities=False):
  """Binarised accessibility: a per-cell depth times a per-peak openness, thresholded (or the probabilities themselves)."""
  rng = np.random.default_rng(seed)
  act = rng.normal(size=(n, 1)) * 1.2 + rng.normal(-1.0, 1.0, size=(1, G))
  p = expit(act + 0.7 * rng.normal(size=(n, G)))
  return (p if probabilities else (p > 0.5)).astype(np.float32)


def synth_continuous(n, G, seed=0):
  """Continuous bimodal levels with negative entries (scaled expression / CLR panels): 'on' around 2, 'off' around -0.4, kept above -0.9
  (log1p of the encoder input stays defined)."""
  rng = np.random.default_rng(seed)
  on = rng.uniform(size=(n, G)) < rng.uniform(0.2, 0.6, size=(1, G))
  x = np.where(on, rng.normal(2.0, 0.6, size=(n, G)), rng.normal(-0.4, 0.3, size=(n, G)))
  return np.maximum(x, -0.9).astype(np.float32)


def synth_x(kind, n, G, seed=0):
  return synth_binary(n, G, seed) if kind == "bernoulli" else synth_continuous(n, G, seed)
