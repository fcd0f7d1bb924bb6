"""Several Monte-Carlo draws per cell in training (fit(sample_shape=S), smx_set_train_draws) against the float64 oracle's
unchanged step on the minibatch repeated S times, draw-major, with the draw-keyed noise source of
tests/test_train_draws_host.py (that identity is checked there with torch autograd).  Tolerances of test_gpu_step.py."""
import numpy as np
import pytest

from oracle import sisua_oracle as so
from tests.test_gpu_step import CASES, _problem
from tests.test_train_draws_host import DrawNoise
from tests.util import adam_state_errors, grad_errors, perturbed_params

pytestmark = pytest.mark.gpu
RTOL = 1e-4
BASE = 1000


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _oracle(spec, params, bn, opt, x, ys, lib, mask, rows, step, S, training=True):
  rep = np.tile(rows, S)
  noise = DrawNoise(spec.seed, step, rows + BASE, S)
  kw = dict(y=[y[rep] for y in ys], library=lib[rep], mask=mask[rep])
  if training:
    return so.train_step(spec, params, bn, opt, x[rep], noise, **kw)
  return so.forward_backward(spec, params, bn, x[rep], noise, training=False, backward=False, **kw)


def _engine(Engine, cfg, params, x, ys, lib, mask, max_batch=128):
  e = Engine(cfg, max_batch=max_batch, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=BASE)
  return e


def _check_step(e, m, res, spec, bn, opt):
  assert m["nan_flag"] == 0
  keys = ["loss", "nllk_x", "kl"] + (["nllk_y"] if spec.labels else []) + (["kl_l"] if spec.model == "scvi" else [])
  for key in keys:
    assert np.isclose(m[key], res["metrics"][key], rtol=RTOL, atol=1e-5), (key, m[key], res["metrics"][key])
  worst = grad_errors(e.get_params(which=1), res["grads"])
  assert max(worst.values()) < RTOL, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  em, ev, where = adam_state_errors(e, opt)
  assert em < 2e-4 and ev < 4e-4, (em, ev, where)
  names = [p for p, _ in so.bn_manifest(spec)]
  for i, st in e.get_bn().items():
    assert np.allclose(st["moving_mean"], bn[f"{names[i]}/moving_mean"], rtol=1e-4, atol=1e-6)
    assert np.allclose(st["moving_var"], bn[f"{names[i]}/moving_var"], rtol=1e-4, atol=1e-6)


def _same(a, b):
  """Bitwise equality of arrays, or of lists of arrays (forward's y_params: one array per label head, of different widths)."""
  if isinstance(a, (list, tuple)):
    return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
  return np.array_equal(a, b)


DRAW_CASES = ["vae_zinb", "vae_zinbd", "dca_zinb", "sisua", "misa", "scvi_zinbd", "scvi_share_both", "scale", "scale_tril", "scale_post"]


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("name", DRAW_CASES)
def test_one_step_with_draws_matches_oracle(Engine, name, S):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  e.set_train_draws(S)
  rows = np.random.default_rng(1).choice(x.shape[0], size=64, replace=False).astype(np.int32)
  res = _oracle(spec, params, bn, opt, x, ys, lib, mask, rows, 0, S)
  m = e.train_step(rows)
  assert m["step"] == 1
  _check_step(e, m, res, spec, bn, opt)
  e.close()


def test_trajectory_with_four_draws(Engine):
  """20-step seeded trajectory at S = 4 from the oracle's initial parameters (as test_gpu_step.py's trajectory test): ELBO per step
  within 1e-4 relative, and it trains."""
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_zinbd"], n=512)
  params = {k: v.copy() for k, v in so.init_params(spec).items()}
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  B, n = 64, 20
  e = _engine(Engine, cfg, params, x, ys, lib, mask, max_batch=B)
  e.set_train_draws(4)
  order = np.concatenate([so.epoch_order(x.shape[0], ep, shuffle=100, seed=1) for ep in range(3)])[: n * B].astype(np.int32)
  e.train_steps(order, n, B)
  got = np.asarray(e.metrics_history(n)["loss"], np.float64)
  ref = np.array([_oracle(spec, params, bn, opt, x, ys, lib, mask, order[t * B:(t + 1) * B], t, 4)["metrics"]["loss"] for t in range(n)])
  assert np.allclose(got, ref, rtol=RTOL), np.abs(got / ref - 1).max()
  assert ref[-5:].mean() < ref[:5].mean()      # and it trains
  e.close()


@pytest.mark.parametrize("name", ["vae_zinb", "sisua", "scvi_zinbd"])
def test_graph_replay_is_the_eager_step_with_draws(Engine, name):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  engines = [_engine(Engine, cfg, params, x, ys, lib, mask) for _ in range(2)]
  B, n = 64, 4
  order = np.concatenate([np.random.default_rng(30 + t).choice(x.shape[0], size=B, replace=False) for t in range(n)]).astype(np.int32)
  for e, graph in zip(engines, (False, True)):
    e.set_train_draws(3)
    e.train_steps(order, n, B, graph=graph)
  h0, h1 = engines[0].metrics_history(n), engines[1].metrics_history(n)
  assert all(np.array_equal(h0[k], h1[k]) for k in h0)
  p0, p1 = engines[0].get_params(), engines[1].get_params()
  assert all(np.array_equal(p0[k], p1[k]) for k in p0)
  for e in engines:
    e.close()


# wide_panel_128 at max_batch 64: 64 x 128 floats per slab row -- its scratch capacities at one draw are below the 128 x 128 column-major
# slabs' need, three draws' are not; the routing at one draw must be the fresh engine's
@pytest.mark.parametrize("name,max_batch,B", [("sisua", 128, 96), ("wide_panel_128", 64, 64)])
def test_one_draw_after_three_is_todays_step(Engine, name, max_batch, B):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  e, e0 = (_engine(Engine, cfg, params, x, ys, lib, mask, max_batch=max_batch) for _ in range(2))
  rows = np.random.default_rng(1).choice(x.shape[0], size=B, replace=False).astype(np.int32)
  e.set_train_draws(3)
  f, f0 = e.forward(rows), e0.forward(rows)   # (predict is not a multi-draw pass: the max_batch routing whatever the draw count)
  assert f.keys() == f0.keys() and all(_same(f[k], f0[k]) for k in f0)
  m3 = e.eval_step(rows)
  e.train_step(rows); e0.set_train_draws(3); e0.train_step(rows)   # (both engines through one step at three draws)
  e.set_train_draws(1); e0.set_train_draws(1)
  e1 = _engine(Engine, cfg, e0.get_params(), x, ys, lib, mask, max_batch=max_batch)   # a fresh engine at one draw from the same point ...
  e1.set_bn(e0.get_bn()); e1.set_params(e0.get_params(which=2), which=2); e1.set_params(e0.get_params(which=3), which=3); e1.step = e0.step
  for r in (rows, (rows + 5) % x.shape[0]):   # ... and the grown engine set back to one draw take today's steps, bit for bit
    m, m1 = e.train_step(r), e1.train_step(r)
    assert m == m1
  g, g1 = e.get_params(which=1), e1.get_params(which=1)
  assert all(np.array_equal(g[k], g1[k]) for k in g)
  p, p1 = e.get_params(), e1.get_params()
  assert all(np.array_equal(p[k], p1[k]) for k in p)
  assert e.eval_step(rows) == e1.eval_step(rows)
  assert m3["loss"] != e0.eval_step(rows)["loss"]   # (three draws are not one)
  e.close(); e0.close(); e1.close()


def test_failed_grow_leaves_the_model_as_it_was(Engine):
  """An out-of-memory grow (knob alloc_rows_fail: the n-th allocation fails) is all or nothing: the model keeps its buffers and its
  draw count, steps as before, and a later grow succeeds."""
  from sisua_amd import _hip
  spec, cfg, x, ys, lib, mask = _problem(CASES["sisua"])
  params = perturbed_params(spec)
  e, e0 = (_engine(Engine, cfg, params, x, ys, lib, mask) for _ in range(2))
  rows = np.random.default_rng(1).choice(x.shape[0], size=96, replace=False).astype(np.int32)
  for fail_at in (1, 12, 28):   # (sisua: 29 allocations -- the first, one in the middle, the one before the last)
    _hip.set_tuning("alloc_rows_fail", fail_at)
    try:
      with pytest.raises(Exception, match="out of memory"):
        e.set_train_draws(4)
    finally:
      _hip.clear_tuning("alloc_rows_fail")
  e.set_train_draws(1)   # (still one draw)
  m, m0 = e.train_step(rows), e0.train_step(rows)
  assert m == m0
  r2 = (rows + 5) % x.shape[0]
  e.set_train_draws(4); e0.set_train_draws(4)
  assert e.train_step(r2) == e0.train_step(r2)
  p, p0 = e.get_params(), e0.get_params()
  assert all(np.array_equal(p[k], p0[k]) for k in p)
  e.close(); e0.close()


@pytest.mark.parametrize("name", ["vae_zinb", "sisua", "scvi_zinbd", "scale_post"])
def test_eval_step_with_draws_matches_oracle(Engine, name):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  e.set_train_draws(3)
  rows = np.random.default_rng(2).choice(x.shape[0], size=80, replace=False).astype(np.int32)
  res = _oracle(spec, params, bn, None, x, ys, lib, mask, rows, 0, 3, training=False)
  m = e.eval_step(rows)
  for key in ("loss", "nllk_x", "kl"):
    assert np.isclose(m[key], res["metrics"][key], rtol=RTOL, atol=1e-5), (key, m[key], res["metrics"][key])
  e.close()


@pytest.mark.parametrize("B,S", [(64, 3), (100, 3)])   # 192 stacked rows: the one-launch output head; 300: beyond its 256-row bound
def test_wide_panel_with_draws_matches_oracle(Engine, B, S):
  spec, cfg, x, ys, lib, mask = _problem(CASES["wide_panel_128"])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  e.set_train_draws(S)
  rows = np.random.default_rng(1).choice(x.shape[0], size=B, replace=False).astype(np.int32)
  res = _oracle(spec, params, bn, opt, x, ys, lib, mask, rows, 0, S)
  m = e.train_step(rows)
  _check_step(e, m, res, spec, bn, opt)
  e.close()


def test_set_train_draws_refusals(Engine):
  spec, cfg, x, ys, lib, mask = _problem(CASES["fvae"])
  e = _engine(Engine, cfg, perturbed_params(spec), x, ys, lib, mask)
  e.set_train_draws(1)
  with pytest.raises(Exception, match="FactorVAE"):
    e.set_train_draws(2)
  e.close()
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_zinb"])
  e = _engine(Engine, cfg, perturbed_params(spec), x, ys, lib, mask)
  with pytest.raises(Exception, match=">= 1"):
    e.set_train_draws(0)
  e.close()


@pytest.mark.parametrize("storage", ["f32", "csr"])
def test_fit_sample_shape_is_the_engine_with_draws(Engine, storage):
  """VAE.fit(sample_shape=3) is an explicit Engine.set_train_draws(3) + train_steps loop over fit's own minibatch order
  (data.epoch_order / iter_batches of the dataset, a ragged last batch included), bit for bit, and differs from the single-draw fit."""
  from sisua_amd import data as _data
  from sisua_amd import models as api
  from sisua_amd.data import SingleCellOMIC
  from tests.util import synth_counts
  sco = SingleCellOMIC(synth_counts(400, 150, sparsity=0.85, seed=3, max_count=500), name="toy")
  train, test = sco.split(0.8)

  def model():
    return api.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), latents=api.RVmeta(8, "diag", True, "Latents"),
                   encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))

  def datasets():
    return train.create_dataset(batch_size=64, drop_remainder=False), test.create_dataset(batch_size=40, drop_remainder=True)

  epochs = 3
  ds, vs = datasets()
  a = model().fit(ds, valid=vs, metadata=sco, epochs=epochs, valid_freq=4, sample_shape=3, storage=storage)
  c = model().fit(ds, valid=vs, metadata=sco, epochs=epochs, valid_freq=4, sample_shape=(), storage=storage)
  # the same engine, data and initial state through fit with no step, then the steps by hand
  b = model().fit(ds, valid=vs, metadata=sco, epochs=0, sample_shape=(), storage=storage)
  e = b._engine
  assert e.step == 0
  e.set_train_draws(3)
  for ep in range(epochs):
    for batch in _data.iter_batches(_data.epoch_order(ds.n_obs, ep, ds.shuffle, ds.seed), ds.batch_size, ds.drop_remainder):
      ids = np.asarray(batch, np.int32)
      e.train_steps(ids, 1, ids.size)
  pa, pb, pc = a._engine.get_params(), e.get_params(), c._engine.get_params()
  assert all(np.array_equal(pa[k], pb[k]) for k in pa)
  assert not all(np.array_equal(pa[k], pc[k]) for k in pa)
  assert not np.array_equal(a.train_history["loss"], c.train_history["loss"])
  for mdl in (a, b, c):
    mdl._engine.close()
