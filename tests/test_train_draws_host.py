"""Several Monte-Carlo draws per cell in training (fit(sample_shape=S), smx_set_train_draws): the C-ABI entry, the parsing
and refusals of `fit`, and the float64 identity the GPU tests rest on -- the multi-draw step (encoder once, S draws of
the latent, decoder on the S x B stacked rows, mean loss) IS the oracle's unchanged step on the minibatch repeated S
times (draw-major) with a noise source keyed by draw on the draw side.  CPU only."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import sisua_oracle as so
from sisua_amd import _hip
from tests.test_oracle_torch import count_log_prob, mlp, softplus1
from tests.util import perturbed_params, synth_counts

torch.set_default_dtype(torch.float64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAW_STREAMS_FROM = so.STREAM_DEC_DROPOUT   # decoder dropout (48 + i), eps_z (64), eps_l (65), the mixture pick (67)


class DrawNoise:
  """Noise of a step on S x B stacked rows (row r = draw r // B of cell r % B): the encoder-side streams of every row are
  its cell's (sample index 0), the draw-side streams take sample index r // B."""

  def __init__(self, seed, step, cell_ids, S):
    self.cell_ids, self.S = np.asarray(cell_ids), S
    self.src = [so.PhiloxNoise(seed, step, cell_ids, sample=s) for s in range(S)]

  def _get(self, what, stream, *args):
    if stream < DRAW_STREAMS_FROM:
      return np.tile(getattr(self.src[0], what)(stream, *args), (self.S, 1))
    return np.concatenate([getattr(n, what)(stream, *args) for n in self.src], 0)

  def dropout(self, stream, n_cols, p):
    return self._get("dropout", stream, n_cols, p)

  def normal(self, stream, n_cols):
    return self._get("normal", stream, n_cols)

  def uniform(self, stream, n_cols):
    return self._get("uniform", stream, n_cols)


def test_set_train_draws_is_declared_bound_and_exported():
  hdr = open(os.path.join(ROOT, "include", "sisua_hip.h")).read()
  assert re.search(r"int\s+smx_set_train_draws\s*\(\s*smx_model\s*\*\s*m\s*,\s*int32_t\s+n_draws\s*\)\s*;", hdr)
  assert "smx_set_train_draws" in _hip.SIGNATURES
  lib = os.path.join(ROOT, "sisua_amd", "libsisua_hip.so")
  if not os.path.exists(lib):
    pytest.skip("library not built")
  import subprocess
  syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
  assert re.search(r"\bT smx_set_train_draws\b", syms)


def test_sample_shape_parsing():
  from sisua_amd.models import train_draws
  for shape, S in (((), 1), ([], 1), (1, 1), ((1,), 1), (3, 3), ([5], 5), ((2, 3), 6), (np.int64(4), 4)):
    assert train_draws(shape) == S, shape
  for bad in (0, -2, (2, 0), (3, -1), (1.5,), "3"):
    with pytest.raises(ValueError):
      train_draws(bad)


class _NoEngine:
  """Fails the test if `fit` reaches the device."""

  def __init__(self, *a, **k):
    raise AssertionError("an engine was created before the refusal")


class _World2:
  rank, world = 0, 2


def _toy_fit(monkeypatch, cls_name, sample_shape, distributed=False, **kw):
  import sisua_amd.models as M
  from sisua_amd.data import SingleCellOMIC
  monkeypatch.setattr(M, "Engine", _NoEngine)
  sco = SingleCellOMIC(synth_counts(80, 40, seed=5), name="toy")
  sco.add_omic("proteomic", np.eye(3, dtype=np.float32)[np.arange(80) % 3])
  cls = M.get_model(cls_name)
  args = dict(outputs=sco.get_rv("transcriptomic", "zinb"), encoder=M.NetConf([16]), decoder=M.NetConf([16]))
  args.update(kw)
  if cls_name == "semifvae":
    args["labels"] = [sco.get_rv("proteomic", "onehot")]
  model = cls(**args)
  omics = ["transcriptomic"] + (["proteomic"] if cls_name == "semifvae" else [])
  ds = sco.create_dataset(omics, labels_percent=0.5, batch_size=16, drop_remainder=True)
  model.fit(ds, metadata=sco, epochs=1, sample_shape=sample_shape, distributed=distributed)


@pytest.mark.parametrize("cls_name", ["fvae", "semifvae"])
def test_fit_refuses_several_draws_for_factor_vae(monkeypatch, cls_name):
  with pytest.raises(ValueError, match="one draw"):
    _toy_fit(monkeypatch, cls_name, 3)


@pytest.mark.parametrize("shape", [0, -1, (2, 0)])
def test_fit_refuses_non_positive_sample_shape(monkeypatch, shape):
  with pytest.raises(ValueError, match="positive"):
    _toy_fit(monkeypatch, "vae", shape)


def test_fit_refuses_several_draws_data_parallel(monkeypatch):
  with pytest.raises(ValueError, match="single-GPU"):
    _toy_fit(monkeypatch, "vae", (2,), distributed=_World2())


def test_fit_with_one_draw_reaches_the_engine(monkeypatch):
  """The control: sample_shape = () / 1 passes the checks (and so meets the stub engine)."""
  for shape in ((), 1, [1]):
    with pytest.raises(AssertionError, match="engine was created"):
      _toy_fit(monkeypatch, "vae", shape)


def _torch_multidraw_step(spec, params, bn, x, seed, step, cells, S):
  """VAE step with the encoder run ONCE on the B cells and S draws of z (torch autograd, float64)."""
  P = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
  B, G, D = x.shape[0], spec.n_genes, spec.latent_dim
  n0 = so.PhiloxNoise(seed, step, cells, sample=0)
  new_bn = {}
  h0 = torch.log1p(torch.as_tensor(np.asarray(x, np.float64))) * torch.as_tensor(n0.dropout(so.STREAM_INPUT_DROPOUT, G, spec.input_dropout))
  h = mlp(spec, P, bn, "enc", spec.enc_units, h0, n0, so.STREAM_ENC_DROPOUT, spec.dropout_enc, new_bn)
  lat = h @ P["lat/W"] + P["lat/b"]
  mu, sig = lat[:, :D], softplus1(lat[:, D:])
  kl = torch.distributions.kl_divergence(torch.distributions.Normal(mu, sig), torch.distributions.Normal(torch.zeros_like(mu), torch.ones_like(sig))).sum(1)
  eps = torch.as_tensor(np.concatenate([so.PhiloxNoise(seed, step, cells, sample=s).normal(so.STREAM_EPS_Z, D) for s in range(S)], 0))
  z = mu.repeat(S, 1) + sig.repeat(S, 1) * eps   # draw-major
  d = mlp(spec, P, bn, "dec", spec.dec_units, z, DrawNoise(seed, step, cells, S), so.STREAM_DEC_DROPOUT, spec.dropout_dec, new_bn)
  raw = d @ P["out/W"] + P["out/b"]
  xs = torch.as_tensor(np.tile(np.asarray(x, np.float64), (S, 1)))
  llk = count_log_prob(xs, [raw[:, c * G:(c + 1) * G] for c in range(spec.k)], spec.likelihood, False).sum(1)
  loss = (-llk).mean() + spec.beta * kl.mean()   # mean over cells and draws (the KL is the same for every draw of a cell)
  loss.backward()
  return float(loss.detach()), {k: v.grad.numpy() for k, v in P.items()}, new_bn


def test_multidraw_step_is_the_oracle_on_the_repeated_batch():
  spec = so.Spec(model="vae", n_genes=37, likelihood="zinb", enc_units=(24, 20), dec_units=(18, 22), latent_dim=5,
                 dropout_enc=0.3, dropout_dec=0.25, input_dropout=0.2, beta=1.5)
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  x = synth_counts(50, spec.n_genes, seed=2)
  rows = np.random.default_rng(4).choice(50, size=12, replace=False)
  cells, S, step = rows + 1000, 3, 7
  loss_t, grads_t, bn_t = _torch_multidraw_step(spec, params, bn, x[rows], spec.seed, step, cells, S)
  rep = np.tile(rows, S)
  res = so.forward_backward(spec, params, bn, x[rep], DrawNoise(spec.seed, step, cells, S))
  assert abs(res["metrics"]["loss"] - loss_t) <= 1e-10 * abs(loss_t)
  for k, g in grads_t.items():
    ref = res["grads"][k]
    assert np.linalg.norm(ref - g) <= 1e-10 * max(np.linalg.norm(g), 1e-8), k
  for k, v in bn_t.items():   # moving statistics: the encoder's over B cells equal those over the S copies
    assert np.allclose(res["new_bn"][k], v, rtol=1e-12, atol=1e-14), k
  # and S draws are not one: the stacked step differs from the single-draw step
  one = so.forward_backward(spec, params, bn, x[rows], so.PhiloxNoise(spec.seed, step, cells))
  assert abs(one["metrics"]["loss"] - loss_t) > 1e-6 * abs(loss_t)
