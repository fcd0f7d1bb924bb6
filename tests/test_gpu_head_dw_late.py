"""The output head's dW / db / sum-of-squares slots in the decoder's BatchNorm-backward launch (smx_bn.hip: bn_wide_bwd_dw_kernel carrying
smx_headdw.h's role-0 body; smx_backward.hip: dw_late) against the head's own two-role launch (knob no_dw_late): the same
body, so EVERYTHING is equal bit for bit -- at the smallest shapes at which the carrier's block indexing can go wrong, not the workload's."""
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


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _run(Engine, kw, B, knobs, steps=3, n=256):
  """`steps` training steps of a fresh engine under `knobs`: (per-step metrics, gradients, parameters, both moments, moving statistics, the
  form the last step took)."""
  from sisua_amd import _hip
  from tests.util import make_pair, synth_counts, synth_labels
  spec, cfg = make_pair(**kw)
  x = synth_counts(n, spec.n_genes, sparsity=0.85, seed=spec.n_genes + 3, max_count=400)
  ys = synth_labels(n, spec.extra_outputs + spec.labels)
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]], dtype=np.float32), (n, 1))
  mask = so.label_mask(n, 0.4, n_omics=1 + len(spec.labels), seed=1)
  order = np.concatenate([np.random.default_rng(7).permutation(n)[:B] for _ in range(steps)]).astype(np.int32)
  try:
    for k, v in knobs.items():
      _hip.set_tuning(k, v)
    e = Engine(cfg, max_batch=128, init=False)
    e.set_flag("bf16x3", True)   # (by default from the workload's width on: these shapes are far below it)
    e.set_params(so.init_params(spec))
    e.upload(x, ys, lib, mask, cell_id_base=5)
    metrics = []
    for s in range(steps):
      m = e.train_step(order[s * B:(s + 1) * B])
      assert m["nan_flag"] == 0
      metrics.append({k: v for k, v in m.items() if isinstance(v, (int, float))})
    late = e.head_dw_late()
    bn = {f"{i}/{k}": v for i, d in e.get_bn().items() for k, v in d.items()}
    out = (metrics, e.get_params(1), e.get_params(0), e.get_params(2), e.get_params(3), bn, late)
    e.close()
  finally:
    for k in knobs:
      _hip.set_tuning(k, 0)
  return out


def _assert_same(a, b):
  assert a[0] == b[0], (a[0], b[0])   # the ELBO scalars and gradient norms of every step
  for which in (1, 2, 3, 4, 5):
    assert a[which].keys() == b[which].keys()
    for k in a[which]:
      assert np.array_equal(a[which][k], b[which][k]), (which, k)


def _vae(G, lk, H, dec=None, **kw):
  return dict(model="vae", n_genes=G, likelihood=lk, enc_units=(H,), dec_units=dec or (H,), latent_dim=10, **kw)


# cells: ragged inside one wave's 16-cell slice / ragged across slices / full.  genes: 70 -> 3 gene tiles, the XCD map pads to 8 (blocks with
# gt >= n_gt return); 330 -> 11 tiles, a second round of the map.  zinb: 3 planes, nb: 2.  hidden 128 / 64: 4 / 2 H tiles.
GRID = list(itertools.product((5, 37, 128), (70, 330), ("zinb", "nb"), (128, 64)))


@pytest.mark.parametrize("B,G,lk,H", GRID)
def test_carried_dw_equals_the_heads_own_launch_bitwise(Engine, B, G, lk, H):
  """Three training steps with the head's dW carried by the decoder's BatchNorm-backward launch and with the knob no_dw_late: every gradient,
  parameters, both moments, the BatchNorm moving statistics and every step's metrics are equal bit for bit."""
  kw = _vae(G, lk, H)
  on, off = _run(Engine, kw, B, {}), _run(Engine, kw, B, {"no_dw_late": 1})
  assert on[6] and not off[6]   # (the two forms are what ran)
  _assert_same(on, off)


@pytest.mark.parametrize("case,kw", [("two_layer_decoder", _vae(330, "zinb", 128, dec=(64, 128))),   # the carrier is the LAST decoder layer's launch; the riders' next one is the decoder's
                                     ("clipnorm_bites", _vae(330, "zinb", 128, clipnorm=1e-3)),      # every tensor's norm is far above it: the slots the carrier writes decide the update
                                     ("no_clipnorm", _vae(330, "nb", 64, clipnorm=0.0))])
def test_carried_dw_decoder_depth_and_clipnorm(Engine, case, kw):
  on, off = _run(Engine, kw, 37, {}), _run(Engine, kw, 37, {"no_dw_late": 1})
  assert on[6] and not off[6]
  _assert_same(on, off)
  if case == "clipnorm_bites":
    assert max(m["grad_norm_max"] for m in on[0]) > 10 * 1e-3


@pytest.mark.parametrize("B,G,lk,H", [(128, 330, "zinb", 128), (37, 70, "nb", 64)])
def test_the_heads_riders_left_the_carrying_launch(Engine, B, G, lk, H):
  """The carrier WRITES dW_out and its slots, so no optimiser rider of the head may read them in that launch: they start at the next
  BatchNorm-backward launch.  One step with the riders equals one step without any (knob no_adam_early: the optimiser launch updates the
  head) bit for bit -- a rider beside the carrier would have read the previous step's gradient (zeros here) or a torn one."""
  kw = _vae(G, lk, H)
  ride, none = _run(Engine, kw, B, {}, steps=1), _run(Engine, kw, B, {"no_adam_early": 1}, steps=1)
  assert ride[6] and none[6]
  _assert_same(ride, none)
  from tests.util import make_pair
  init = so.init_params(make_pair(**kw)[0])
  head = max(ride[2], key=lambda k: ride[2][k].size)   # W_out: the largest tensor
  assert np.any(ride[2][head] != init[head].astype(np.float32)) and np.any(ride[1][head] != 0)   # (it was updated, from a gradient that is there)


@pytest.mark.parametrize("case,kw", [("sisua_label_head", dict(model="sisua", n_genes=180, likelihood="zinb", enc_units=(64,), dec_units=(64,), latent_dim=9,
                                                               labels=((12, "nb"),))),
                                     ("scvi", dict(model="scvi", n_genes=160, likelihood="zinbd", enc_units=(48,), dec_units=(48,), latent_dim=6,
                                                   encl_units=(16,)))])
def test_outside_the_predicate_the_knob_changes_nothing(Engine, case, kw):
  """A label head (its d d rides with the head's launch) and scvi (separate plane tensors) keep the head's own launch either way."""
  on, off = _run(Engine, kw, 37, {}), _run(Engine, kw, 37, {"no_dw_late": 1})
  assert not on[6] and not off[6]
  _assert_same(on, off)
