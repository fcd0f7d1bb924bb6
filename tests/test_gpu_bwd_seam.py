"""The decoder's BatchNorm-backward launch (the output head's dW carrier) and the encoder's (with the d z product folded in) as ONE launch whose
encoder workgroups wait inside it for the decoder's d pre-activation (smx_bn.hip: bn_bwd_seam_kernel; smx_handoff.h; smx_backward.hip: the seam
form) against the two launches (knob no_bwd_seam): the same device functions, so EVERYTHING is equal bit for bit -- at the
smallest shapes at which the block indexing and the counter's target can go wrong, not the workload's.

The form needs the fold of the d z product, which exists for a first decoder layer of 128 units only: the grid's hidden width of 64 is the
ENCODER's (8 waiting workgroups instead of 16) beside a decoder of 128 (128 publishing workgroups); with a decoder of 64 units there is no
fold, the form is not taken and the query says so (test_outside_the_predicate_the_two_launches_stay)."""
import itertools
import os
import sys

import numpy as np
import pytest

from oracle import sisua_oracle as so

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

KNOB = {"no_bwd_seam": 1}


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _run(Engine, kw, B, knobs, calls=(3,), n=256, storage="f32", setup=None):
  """train_steps calls of `calls` steps each on a fresh engine under `knobs`: (metrics_history of every call, gradients, parameters, both
  moments, moving statistics, the loss of an eval_step behind them, smx_bwd_seam_steps after every call, smx_lazy_adam_steps after every call)."""
  from sisua_amd import _hip
  from tests.util import make_pair, synth_counts, synth_labels
  spec, cfg = make_pair(**kw)
  x = synth_counts(n, spec.n_genes, sparsity=0.85, seed=spec.n_genes + 3, max_count=400)
  ys = synth_labels(n, spec.extra_outputs + spec.labels)
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]], dtype=np.float32), (n, 1))
  mask = so.label_mask(n, 0.4, n_omics=1 + len(spec.labels), seed=1)
  rng = np.random.default_rng(7)
  try:
    for k, v in knobs.items():
      _hip.set_tuning(k, v)
    e = Engine(cfg, max_batch=128, init=False)
    e.set_flag("bf16x3", True)   # (by default from the workload's width on: these shapes are far below it)
    e.set_params(so.init_params(spec))
    e.upload(x, ys, lib, mask, cell_id_base=5, storage=storage)
    if setup:
      setup(e)
    hist, seam, lazy = [], [], []
    for K in calls:
      order = np.concatenate([rng.permutation(n)[:B] for _ in range(K)]).astype(np.int32)
      m = e.train_steps(order, K, B, metrics=True)
      assert m["nan_flag"] == 0
      hist.append(e.metrics_history(K))
      seam.append(e.bwd_seam_steps())
      lazy.append(e.lazy_adam_steps())
    grads, params, m1, m2 = e.get_params(1), e.get_params(0), e.get_params(2), e.get_params(3)
    bn = {f"{i}/{k}": v for i, d in e.get_bn().items() for k, v in d.items()}
    ev = e.eval_step(np.arange(B, dtype=np.int32))["loss"]
    e.close()
  finally:
    for k in knobs:
      _hip.set_tuning(k, 0)
  return hist, grads, params, m1, m2, bn, ev, seam, lazy


def _assert_same(a, b):
  assert len(a[0]) == len(b[0])
  for ha, hb in zip(a[0], b[0]):   # the ELBO scalars of every step of every call
    for k in ha:
      assert np.array_equal(ha[k], hb[k]), (k, ha[k], hb[k])
  for which in (1, 2, 3, 4, 5):
    assert a[which].keys() == b[which].keys()
    for k in a[which]:
      assert np.array_equal(a[which][k], b[which][k]), (which, k)
  assert a[6] == b[6]   # the evaluation loss behind the calls


def _pair(Engine, kw, B, calls=(3,), knobs=None, **opts):
  on, off = _run(Engine, kw, B, dict(knobs or {}), calls, **opts), _run(Engine, kw, B, dict(knobs or {}, **KNOB), calls, **opts)
  _assert_same(on, off)
  return on, off


def _vae(G, lk, H, dec=(128,), **kw):
  return dict(model="vae", n_genes=G, likelihood=lk, enc_units=(H,), dec_units=dec, latent_dim=10, **kw)


# cells: ragged inside one wave's 16-cell slice / ragged across slices / full.  genes: 70 -> 3 gene tiles of the carried dW (the XCD map pads
# to 8), 330 -> 11: a second round.  zinb: 3 planes, nb: 2.  encoder 128 / 64: 16 / 8 waiting workgroups behind the decoder's 128 columns.
GRID = list(itertools.product((5, 37, 128), (70, 330), ("zinb", "nb"), (128, 64)))


@pytest.mark.parametrize("B,G,lk,H", GRID)
def test_one_launch_equals_the_two_launches_bitwise(Engine, B, G, lk, H):
  """Three steps of one call (two of them with the lazy encoder update: the step's close and W_enc's chunks ride in the fused launch)."""
  on, off = _pair(Engine, _vae(G, lk, H), B)
  assert on[7] == [3] and off[7] == [0]   # (the two forms are what ran)
  assert on[8] == off[8] == [2]


@pytest.mark.parametrize("calls", [(1,), (2,), (5,), (3, 3), (1, 4, 1)])
def test_epochs_within_a_call_and_between_calls(Engine, calls):
  """The counter counts within a library call (target = columns x steps so far) and the call's first step zeroes it: K = 1, 2, 5 and calls
  back to back."""
  on, off = _pair(Engine, _vae(330, "zinb", 128), 37, calls)
  assert on[7] == list(calls) and off[7] == [0] * len(calls)


@pytest.mark.parametrize("case,kw,knobs,opts", [
    ("no_lazy_update", _vae(330, "zinb", 128), {"no_lazy_adam": 1}, {}),        # every step keeps its optimiser launch: no close, no W_enc chunks in the fused launch
    ("clipnorm_bites", _vae(330, "zinb", 128, clipnorm=1e-3), {}, {}),          # the head's chunks left the backward chain: their clip factor comes from the slots the tiles wrote
    ("no_clipnorm", _vae(330, "nb", 64, clipnorm=0.0), {}, {}),
    ("dropout", _vae(330, "zinb", 128, dropout_enc=0.3, dropout_dec=0.2), {}, {}),
    ("no_dropout", _vae(70, "nb", 64, dropout_enc=0.0, dropout_dec=0.0), {}, {}),
    ("uint16_store", _vae(598, "zinb", 128), {}, dict(storage="u16")),
    ("consumers_first", _vae(330, "zinb", 64), {"bwd_seam_cons_first": 1}, {}),  # the waiting workgroups AHEAD of the columns in block order: no dependence on dispatch order
    ("preread", _vae(330, "zinb", 128), {"bwd_seam_preread": 1}, {}),            # the waiting workgroups plain-load every line of d pre_dec before they wait: an L1-warm consumer
    ("preread_consumers_first", _vae(70, "nb", 128), {"bwd_seam_preread": 1, "bwd_seam_cons_first": 1}, {}),
])
def test_variants(Engine, case, kw, knobs, opts):
  on, off = _pair(Engine, kw, 37, (4,), knobs=knobs, **opts)
  assert on[7] == [4] and off[7] == [0], case
  if case == "no_lazy_update":
    assert on[8] == off[8] == [0]


def test_consumer_position_and_preread_change_nothing(Engine):
  """The same four steps with the waiting workgroups behind / ahead of the columns and L1-warm: one result."""
  kw = _vae(330, "zinb", 128)
  a = _run(Engine, kw, 128, {}, (4,))
  b = _run(Engine, kw, 128, {"bwd_seam_cons_first": 1}, (4,))
  c = _run(Engine, kw, 128, {"bwd_seam_preread": 1}, (4,))
  assert a[7] == b[7] == c[7] == [4]
  _assert_same(a, b)
  _assert_same(a, c)


def _timing(e):
  e.timing_enable("bn_bwd")


def _sync_bn(e):
  e.set_sync_bn(True)


@pytest.mark.parametrize("case,kw,opts", [
    ("decoder_of_64", _vae(330, "zinb", 64, dec=(64,)), {}),             # no fold of the d z product: 64 columns never publish to anybody
    ("two_layer_decoder", _vae(330, "zinb", 128, dec=(64, 128)), {}),    # the carrier's d pre is not the fold's operand
    ("wide_encoder", _vae(330, "zinb", 256), {}),                        # 32 chain workgroups: more than may wait
    ("scvi", dict(model="scvi", n_genes=160, likelihood="zinbd", enc_units=(48,), dec_units=(48,), latent_dim=6, encl_units=(16,)), {}),
    ("sync_bn", _vae(330, "zinb", 128), dict(setup=_sync_bn)),
    ("timed_step", _vae(330, "zinb", 128), dict(setup=_timing)),
])
def test_outside_the_predicate_the_two_launches_stay(Engine, case, kw, opts):
  on, off = _pair(Engine, kw, 37, (3,), **opts)
  assert on[7] == [0] and off[7] == [0], case
