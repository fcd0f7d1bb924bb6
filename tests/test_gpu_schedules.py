"""Step-dependent KL weight and learning rate on the device (include/sisua_hip.h: smx_set_schedule) against the unchanged oracle stepped one
step at a time with that step's beta / lr (dataclasses.replace(spec, beta=..., lr=...)), and bitwise agreement of the launch forms that
must not change a step's bits: the const schedule and the float, graph replay and eager launches, the heads' background sweep and the
riders, a resumed fit and an uninterrupted one."""
import dataclasses
import os

import numpy as np
import pytest

from oracle import sisua_oracle as so
from sisua_amd import interpolation as I
from tests.test_gpu_optimizers import CASES, SETTINGS, _problem, _set_rule, with_rule   # noqa: F401 (fixture)
from tests.test_optimizers_host import init_opt
from tests.util import grad_errors, make_pair, perturbed_params, synth_counts

pytestmark = pytest.mark.gpu
RTOL = 1e-4
EXP = {"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=2e-3, decay_steps=10, decay_rate=0.5)}


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _bitwise(a, b):
  for k in a:
    assert np.array_equal(a[k], b[k]), k


def test_default_path_unchanged(Engine):
  """C2 shape, 20 steps: const(1.0) as beta and ExponentialDecay(decay_rate=1) as lr give the bits of the floats."""
  spec, cfg, x, ys, lib, mask = _problem(dict(model="vae", n_genes=1998, likelihood="zinb", enc_units=(128,), dec_units=(128,), latent_dim=32), n=1024)
  order = np.concatenate([so.epoch_order(x.shape[0], ep, shuffle=100, seed=1) for ep in range(3)])[: 20 * 128].astype(np.int32)
  runs = []
  for sched in (False, True):
    e = Engine(cfg, max_batch=128, init=False)
    e.set_params(so.init_params(spec))
    if sched:
      e.set_schedule("beta", I.const(1.0))
      e.set_schedule("lr", {"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=cfg.lr, decay_steps=7, decay_rate=1.0)})
    e.upload(x, ys, lib, mask)
    e.train_steps(order, 20, 128, graph=False)
    runs.append((e.get_params(0), e.get_params(2), e.get_params(3), e.metrics_history(20)))
    e.close()
  for i in range(4):
    _bitwise(runs[0][i], runs[1][i])


def test_vae_zinb_trajectory_matches_reference(Engine):
  """40 steps with a delayed linear KL warm-up and an exponentially decaying lr: the loss of every step, the final parameters, and beta
  recovered from the per-step ELBO scalars."""
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_zinb"], n=400)
  beta = I.linear(vmin=0, vmax=1, norm=20, delayIn=5)
  lr = I.as_schedule(EXP)
  B, steps = 64, 40
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=B, init=False)
  e.set_params(params)
  e.set_schedule("beta", beta)
  e.set_schedule("lr", EXP)
  e.upload(x, ys, lib, mask)
  rng = np.random.default_rng(2)
  order = np.concatenate([rng.permutation(x.shape[0])[:B] for _ in range(steps)]).astype(np.int32)
  e.train_steps(order, steps, B, graph=False)
  h = e.metrics_history(steps)
  ref = []
  for s in range(steps):
    rows = order[s * B:(s + 1) * B]
    sp = dataclasses.replace(spec, beta=beta(s), lr=lr(s))
    ref.append(so.train_step(sp, params, bn, opt, x[rows], so.PhiloxNoise(spec.seed, s, rows))["loss"])
  assert np.allclose(h["loss"], ref, rtol=RTOL, atol=1e-5), np.abs(h["loss"] / np.array(ref) - 1).max()
  worst = grad_errors(e.get_params(0), params)
  assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  kl = h["kl"].astype(np.float64) + h["kl_l"]
  got_beta = (h["loss"] - h["nllk_x"] - h["nllk_o"] - spec.alpha * h["nllk_y"]) / kl
  want = np.array([beta(s) for s in range(steps)])
  assert np.allclose(got_beta, want, atol=2e-3 * max(1.0, np.abs(h["loss"]).max() / kl.min())), (got_beta, want)
  assert want[0] == 0.0 and want[30] == 1.0
  e.close()


KL_CASES = {
    "vae_fold": dict(model="vae", n_genes=300, likelihood="zinb", enc_units=(128,), dec_units=(128,), latent_dim=32),
    "vae_generic": CASES["vae_zinb"],
    "scale_diag": dict(model="scale", n_genes=100, likelihood="zinb", enc_units=(32,), dec_units=(32,), latent_dim=7, n_components=4),
    "scale_tril": dict(model="scale", n_genes=100, likelihood="zinb", enc_units=(32,), dec_units=(32,), latent_dim=7, n_components=4,
                       covariance="tril"),
    "scale_mixture": dict(model="scale", n_genes=100, likelihood="zinb", enc_units=(32,), dec_units=(32,), latent_dim=7, n_components=4,
                          latent_mixture=True),
    "scvi": CASES["scvi"],
    "fvae": CASES["fvae"],
    "sisua": CASES["sisua"],
}


@pytest.mark.parametrize("case", list(KL_CASES))
def test_one_step_at_a_scheduled_beta(Engine, case):
  """One step at step 13 of a cosine KL weight (beta 0.3 .. 2.5, not 1) with a piecewise lr, against the oracle at that step's values."""
  spec, cfg, x, ys, lib, mask = _problem(KL_CASES[case])
  beta = I.cosine(vmin=0.3, vmax=2.5, norm=20, delayIn=2)
  lr = I.as_schedule({"class_name": "PiecewiseConstantDecay", "config": dict(boundaries=[5, 12], values=[1e-3, 5e-4, 3e-3])})
  step, B = 13, 64
  assert beta(step) not in (0.3, 1.0, 2.5)
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  opt["t"] = step
  e = Engine(cfg, max_batch=B, init=False)
  e.set_params(params)
  e.set_schedule("beta", beta)
  e.set_schedule("lr", lr)
  e.upload(x, ys, lib, mask)
  e.step = step
  rows = (np.arange(B, dtype=np.int32) * 3 + 1) % x.shape[0]
  got = e.train_steps(rows, 1, B, graph=False, metrics=True)
  sp = dataclasses.replace(spec, beta=beta(step), lr=lr(step))
  res = so.train_step(sp, params, bn, opt, x[rows], so.PhiloxNoise(spec.seed, step, rows), y=[y[rows] for y in ys], library=lib[rows],
                      mask=mask[rows])
  assert np.isclose(got["loss"], res["loss"], rtol=RTOL, atol=1e-5), (got["loss"], res["loss"])
  worst = grad_errors(e.get_params(0), params)
  assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  e.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_lr_schedule_under_every_rule_restarts_at_t0(Engine, with_rule, setting):
  """Two Adam steps, then the rule (t0 = 2): the lr schedule is keyed by step - t0, so the rule's first step takes the schedule's value at 0."""
  name, hp = SETTINGS[setting]
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_zinb"])
  lr = I.as_schedule(EXP)
  B = 64
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), init_opt("adam", params)
  e = Engine(cfg, max_batch=B, init=False)
  e.set_params(params)
  e.set_schedule("lr", EXP)
  e.upload(x, ys, lib, mask)
  order = (np.arange(B * 8, dtype=np.int32) * 7 + 5) % x.shape[0]
  losses, ref = [], []
  e.train_steps(order[:2 * B], 2, B, graph=False)
  losses += list(e.metrics_history(2)["loss"])
  _set_rule(e, name, hp)
  assert e.get_optimizer()[2] == 2
  e.train_steps(order[2 * B:], 6, B, graph=False)
  losses += list(e.metrics_history(6)["loss"])
  for s in range(8):
    if s == 2:
      opt = init_opt(name, params, **hp)
    rows = order[s * B:(s + 1) * B]
    sp = dataclasses.replace(spec, lr=lr(s if s < 2 else s - 2))
    ref.append(so.train_step(sp, params, bn, opt, x[rows], so.PhiloxNoise(spec.seed, s, rows))["loss"])
  assert np.allclose(losses, ref, rtol=RTOL, atol=1e-5), (losses, ref)
  worst = grad_errors(e.get_params(0), params)
  assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  e.close()


def test_wide_panel_sweep_takes_its_own_steps_lr(Engine):
  """128 cells x 20 000 genes zinb, head_fused: with both schedules the background sweep (head_sweep on) gives the bits of the riders."""
  spec, cfg = make_pair(model="vae", n_genes=20000, likelihood="zinb", enc_units=(128,), dec_units=(128,), latent_dim=32)
  x = synth_counts(256, 20000, sparsity=0.93, seed=11, max_count=500)
  rng = np.random.default_rng(3)
  order = np.concatenate([rng.permutation(256)[:128] for _ in range(4)]).astype(np.int32)
  runs = []
  for sweep in (False, True):
    e = Engine(cfg, max_batch=128, init=False)
    e.set_params(so.init_params(spec))
    e.set_flag("head_fused", True)
    e.set_flag("head_sweep", sweep)
    e.set_schedule("beta", I.linear(vmin=0.2, vmax=1.5, norm=3))
    e.set_schedule("lr", {"class_name": "InverseTimeDecay", "config": dict(initial_learning_rate=3e-3, decay_steps=1, decay_rate=2.0)})
    e.upload(x, cell_id_base=7, storage="u16")
    assert e.head_fused_bytes(128) > 0
    e.train_steps(order, 4, 128, graph=False)
    runs.append((e.metrics_history(4), e.get_params(0), e.get_params(2), e.get_params(3)))
    e.close()
  for i in range(4):
    _bitwise(runs[0][i], runs[1][i])


def test_graph_replay_equals_eager_bitwise(Engine):
  spec, cfg, x, ys, lib, mask = _problem(CASES["sisua"])
  outs = []
  for graph in (False, True):
    e = Engine(cfg, max_batch=64)
    e.set_schedule("beta", I.linear(vmin=0, vmax=2, norm=4, cyclical=True, delayIn=1, delayOut=1))
    e.set_schedule("lr", EXP)
    e.upload(x, ys, lib, mask)
    for call in range(2):   # (a second call replays the captured graph with a fresh table)
      order = (np.arange(64 * 5, dtype=np.int32) + 17 * call) % x.shape[0]
      e.train_steps(order, 5, 64, graph=graph)
      outs.append(e.metrics_history(5))
    outs.append((e.get_params(0), e.get_params(2), e.get_params(3)))
    e.close()
  _bitwise(outs[0], outs[3])
  _bitwise(outs[1], outs[4])
  for i in range(3):
    _bitwise(outs[2][i], outs[5][i])


@pytest.mark.parametrize("world,shard", [(2, False), (4, True)])
def test_data_parallel_matches_reference(Engine, world, shard):
  from tests.test_gpu_dp import run_ranks
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_zinb"], n=400)
  beta = I.linear(vmin=0.5, vmax=2.0, norm=3)
  lr = I.as_schedule(EXP)
  B, steps, base = 32, 4, 1000
  rng = np.random.default_rng(5)
  rows = [rng.permutation(x.shape[0])[: B * world].astype(np.int32).reshape(world, B) for _ in range(steps)]
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  engines = []
  for r in range(world):
    e = Engine(cfg, max_batch=64, init=False)
    e.set_params(params)
    e.set_schedule("beta", beta)
    e.set_schedule("lr", EXP)
    e.upload(x, ys, lib, mask, cell_id_base=base)
    engines.append(e)
  Engine.comm_init_local(engines)
  for e in engines:
    e.set_flag("opt_shard", shard)
  refs = [so.dp_train_step(dataclasses.replace(spec, beta=beta(s), lr=lr(s)), params, bn, opt, x, list(rows[s]), s, cell_base=base)
          for s in range(steps)]
  orders = [np.concatenate([rows[s][r] for s in range(steps)]) for r in range(world)]
  run_ranks([lambda r=r: engines[r].train_steps(orders[r], steps, B, graph=False, metrics=True) for r in range(world)])
  for r in range(world):
    h = engines[r].metrics_history(steps)["loss"]
    for s in range(steps):
      assert np.isclose(h[s], refs[s]["metrics"]["loss"], rtol=RTOL, atol=1e-5), (r, s)
  if shard:
    run_ranks([lambda r=r: engines[r].opt_gather() for r in range(world)])
  worst = grad_errors(engines[0].get_params(0), params)
  assert max(worst.values()) < 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  for r in range(1, world):
    _bitwise(engines[0].get_params(0), engines[r].get_params(0))
  for e in engines:
    e.close()


# ---- the model surface ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


def test_resume_with_schedules_is_bitwise_an_uninterrupted_run(api, tmp_path):
  from sisua_amd.data import SingleCellOMIC
  sco = SingleCellOMIC(synth_counts(600, 120, sparsity=0.8, seed=3), name="toy")
  ds = sco.create_dataset(batch_size=64, drop_remainder=True)
  beta = api.interpolation.linear(vmin=0, vmax=2, norm=5, cyclical=True, delayIn=2, delayOut=1)
  lr = {"class_name": "PolynomialDecay", "config": dict(initial_learning_rate=3e-3, decay_steps=12, end_learning_rate=1e-4, cycle=True)}

  def vae():
    return api.VAE(outputs=sco.get_rv("transcriptomic"), latents=api.RVmeta(6, "diag", True, "Latents"),
                   encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True), beta=beta)

  whole = vae()
  whole.fit(ds, metadata=sco, epochs=4, learning_rate=lr)
  first = vae()
  first.fit(ds, metadata=sco, epochs=2, learning_rate=lr)
  path = os.path.join(tmp_path, "model")
  first.save_weights(path)
  resumed = api.load_model(path)
  assert resumed.beta_schedule == beta and resumed.beta == beta(resumed.step)
  resumed.fit(ds, metadata=sco, epochs=2, learning_rate=lr)
  assert resumed.step == whole.step and whole.beta == beta(whole.step)
  a, b = whole._engine.snapshot(), resumed._engine.snapshot()
  for key in ("params", "m", "v"):
    _bitwise(a[key], b[key])
  assert np.array_equal(whole.train_history["loss"][-1], resumed.train_history["loss"][-1])
  # validation loss takes beta at the model's step: the eval pass of the engine by hand, at two steps of different beta
  e = whole._engine
  rows = np.arange(64, dtype=np.int32)
  s0 = e.step
  vals = []
  for s in (s0, s0 + 2):
    e.step = s
    vals.append((beta(s), e.eval_step(rows)))
  e.step = s0
  (b0, m0), (b1, m1) = vals
  assert b0 != b1
  for bb, m in vals:
    assert np.isclose(m["loss"], m["nllk_x"] + bb * (m["kl"] + m["kl_l"]), rtol=1e-5), (bb, m)
