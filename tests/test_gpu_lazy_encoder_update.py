"""The lazy encoder update (smx_step.hip): inside a train_steps call every step but the last leaves its optimiser launch
out -- the next step's first launch, the gathered encoder product, updates its block of W_enc in registers while staging it (gemm_body's
RIDE form) and carries the other pending chunks as riders, the latent head's product carries W_enc's own chunks, and the ELBO scalars and the
step's close ride with the encoder's BatchNorm-backward launch -- against the optimiser launch of every step (knob no_lazy_adam).  The same
device functions on both sides, so EVERYTHING is equal bit for bit: parameters, both moments, the last step's gradients, the BatchNorm
moving statistics, every step's metrics_history.  smx_lazy_adam_steps tells which form ran: K - 1 of a call's K steps, 0 under the knob.

Gene widths and what launch_gemm's eff_split is for the first layer's product there (Gp = G rounded up to 32; suggest_split_k gives one slab
below 512 rows and 128-row slabs above, at every cell count and hidden width of the grid):
  G =  70: Gp =  96, eff_split 1 -- one slab, ONE K tile of 96 live rows (rows 96..127 of the tile zeroed behind the update);
  G = 330: Gp = 352, eff_split 1 -- one slab whose workgroups walk THREE K tiles (128, 128, 96): the update is applied to every tile loaded;
  G = 600: Gp = 608, eff_split 5 -- four full slabs and a last one of 96 rows;
  G = 598: Gp = 608, eff_split 5 -- the same with a gene count that is no multiple of 4 (two more zero-padded rows of W_enc, which must stay zero)."""
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

KNOB = {"no_lazy_adam": 1}


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _run(Engine, kw, B, knobs, calls=(3,), n=256, storage="f32", setup=None, draws=1):
  """train_steps calls of `calls` steps each on a fresh engine under `knobs`: (metrics_history of every call, gradients, parameters, both
  moments, moving statistics, the loss of an eval_step behind them, smx_lazy_adam_steps after every call)."""
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
    if draws > 1:
      e.set_train_draws(draws)
    if setup:
      setup(e)
    hist, lazy = [], []
    for K in calls:
      order = np.concatenate([rng.permutation(n)[:B] for _ in range(K)]).astype(np.int32)
      m = e.train_steps(order, K, B, metrics=True)
      assert m["nan_flag"] == 0
      hist.append(e.metrics_history(K))
      lazy.append(e.lazy_adam_steps())
    grads, params, m1, m2 = e.get_params(1), e.get_params(0), e.get_params(2), e.get_params(3)
    bn = {f"{i}/{k}": v for i, d in e.get_bn().items() for k, v in d.items()}
    ev = e.eval_step(np.arange(B, dtype=np.int32))["loss"]
    e.close()
  finally:
    for k in knobs:
      _hip.set_tuning(k, 0)
  return hist, grads, params, m1, m2, bn, ev, lazy


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


def _pair(Engine, kw, B, calls=(3,), **opts):
  on, off = _run(Engine, kw, B, {}, calls, **opts), _run(Engine, kw, B, KNOB, calls, **opts)
  _assert_same(on, off)
  return on, off


def _vae(G, H, enc=None, **kw):
  return dict(model="vae", n_genes=G, likelihood="zinb", enc_units=enc or (H,), dec_units=(H,), latent_dim=10, **kw)


# cells: ragged inside one 32-row tile / ragged across tiles / full.  hidden 128 / 64: four / two N tiles.  genes: the module docstring.
GRID = list(itertools.product((5, 37, 128), (128, 64), (70, 600, 598)))


@pytest.mark.parametrize("B,H,G", GRID)
def test_lazy_update_equals_the_optimiser_launch_bitwise(Engine, B, H, G):
  """Three steps in one call: two of them leave their optimiser launch to the next step's forward launches; everything equal bit for bit."""
  on, off = _pair(Engine, _vae(G, H), B)
  assert on[7] == [2] and off[7] == [0]
  init = so.init_params(so.Spec(**_vae(G, H)))
  w = "enc0/W"
  assert on[2][w].shape == (G, H)
  assert np.any(on[2][w] != init[w].astype(np.float32)) and np.any(on[1][w] != 0)   # (it was updated, from a gradient that is there)


@pytest.mark.parametrize("calls,lazy", [((1,), [0]), ((2,), [1]), ((5,), [4]), ((3, 3), [2, 2]), ((1, 4, 1), [0, 3, 0])])
def test_call_shapes(Engine, calls, lazy):
  """K = 1 defers nothing; K = 2 and 5; two calls back to back (the last step of a call keeps its launch: nothing pending outlives the call,
  and the next call starts afresh at parity 0); a workgroup walking three K tiles (G = 330)."""
  on, off = _pair(Engine, _vae(330, 128), 37, calls)
  assert on[7] == lazy and off[7] == [0] * len(calls)


@pytest.mark.parametrize("B,G,H", [(128, 600, 128), (37, 70, 64)])
def test_both_carriers_of_w_enc_chunks(Engine, B, G, H):
  """W_enc's own chunks ride with the decoder's BatchNorm-backward launch where it is the head's dW carrier (these shapes: head_dw_late) and
  with the latent head's product otherwise (knob lazy_w_fwd forces that one): both equal the optimiser launch bit for bit."""
  kw = _vae(G, H)
  late, fwd, off = _run(Engine, kw, B, {}, (4,)), _run(Engine, kw, B, {"lazy_w_fwd": 1}, (4,)), _run(Engine, kw, B, KNOB, (4,))
  assert late[7] == [3] and fwd[7] == [3] and off[7] == [0]
  _assert_same(late, off)
  _assert_same(fwd, off)


@pytest.mark.parametrize("B,H", [(128, 128), (37, 64), (5, 128)])
def test_xcd_aware_block_map_of_the_first_launch(Engine, B, H):
  """G = 500: Gp = 512, eff_split 4 -- with 4 / 2 N tiles the 16 / 8 blocks of W_enc are a multiple of 8 and the riding launch maps the
  workgroups that share a block onto one XCD (4, 2 and 1 M tiles); the plain order under the knob lazy_no_xcd_map.  Both equal the optimiser launch."""
  kw = _vae(500, H)
  xm, plain, off = _run(Engine, kw, B, {}), _run(Engine, kw, B, {"lazy_no_xcd_map": 1}), _run(Engine, kw, B, KNOB)
  assert xm[7] == [2] and plain[7] == [2] and off[7] == [0]
  _assert_same(xm, off)
  _assert_same(plain, off)


def _sched(e):
  from sisua_amd import interpolation as I
  e.set_schedule("beta", I.linear(vmin=0.2, vmax=1.5, norm=3))
  e.set_schedule("lr", {"class_name": "InverseTimeDecay", "config": dict(initial_learning_rate=3e-3, decay_steps=1, decay_rate=2.0)})


@pytest.mark.parametrize("case,kw,opts", [
    ("clipnorm_bites", _vae(600, 128, clipnorm=1e-3), {}),      # every tensor's norm far above it: the tile workgroups' clip factor decides W_enc
    ("no_clipnorm", _vae(330, 64, clipnorm=0.0), {}),
    ("schedules", _vae(600, 64), dict(setup=_sched)),           # lr halves from step to step: the deferred update must take the PENDING step's lr_t
    ("two_layer_encoder", _vae(330, 128, enc=(128, 64)), {}),   # the second layer's tensors are riders of the first launch
    ("uint16_store", _vae(598, 128), dict(storage="u16")),      # XF == 2
    ("csr_store", _vae(330, 64), dict(storage="csr")),
    ("two_draws", _vae(330, 128), dict(draws=2)),               # 74 stacked rows
    ("input_dropout", _vae(330, 128, input_dropout=0.3), {}),
])
def test_variants(Engine, case, kw, opts):
  on, off = _pair(Engine, kw, 37, (4,), **opts)
  assert on[7] == [3] and off[7] == [0], case


def _rmsprop(e):
  assert e.set_optimizer("rmsprop")


def _timing(e):
  e.timing_enable("adam")


@pytest.mark.parametrize("case,kw,opts", [
    ("rmsprop", _vae(330, 128), dict(setup=_rmsprop)),   # the riders carry Adam only
    ("scvi", dict(model="scvi", n_genes=160, likelihood="zinbd", enc_units=(48,), dec_units=(48,), latent_dim=6, encl_units=(16,)), {}),   # two encoders read X
    ("timing_adam", _vae(330, 128), dict(setup=_timing)),   # per-kernel timings keep the optimiser launch
])
def test_outside_the_predicate_the_optimiser_launch_stays(Engine, case, kw, opts):
  on, off = _pair(Engine, kw, 37, (3,), **opts)
  assert on[7] == [0] and off[7] == [0], case
