"""The optimiser rules on the device (smx_set_optimizer; smx_adam.h: opt_apply4) against the float64 reference of
tests/test_optimizers_host.py composed with oracle.forward_backward (oracle.train_step / dp_train_step with the rule in place of Adam):
one step of every rule and setting on several model families from non-trivial slots, 100-step trajectories at the C2 shape, the same
bits across every launch that carries chunks, data parallel with and without opt_shard, checkpoints, switching rules, and fit."""
import os

import numpy as np
import pytest

from oracle import sisua_oracle as so
from tests.test_optimizers_host import SETTINGS, init_opt, opt_update, rule_apply
from tests.util import grad_errors, make_pair, masked_move_error, perturbed_params, rel_l2, synth_counts, synth_labels

pytestmark = pytest.mark.gpu
RTOL = 1e-4


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


@pytest.fixture
def with_rule(monkeypatch):
  """oracle.train_step / dp_train_step compose forward_backward with the rule of their `opt` state (init_opt) instead of Adam"""
  monkeypatch.setattr(so, "adam_update", opt_update)


CASES = {
    "vae_zinb": dict(model="vae", n_genes=203, likelihood="zinb", enc_units=(48, 40), dec_units=(40,), latent_dim=10),
    "sisua": dict(model="sisua", n_genes=180, likelihood="zinb", enc_units=(64,), dec_units=(64,), latent_dim=9,
                  labels=((12, "nb"), (7, "onehot"))),
    "scvi": dict(model="scvi", n_genes=160, likelihood="zinbd", enc_units=(48,), dec_units=(48,), latent_dim=6, encl_units=(16,)),
    "scale_tied": dict(model="scale", n_genes=100, likelihood="zinb", enc_units=(32,), dec_units=(32,), latent_dim=7, n_components=4,
                       tie_loc=True),
    "fvae": dict(model="fvae", n_genes=110, likelihood="zinb", enc_units=(32,), dec_units=(32,), latent_dim=8, disc_units=60, disc_layers=2),
    "vae_clip": dict(model="vae", n_genes=120, likelihood="nb", enc_units=(32,), dec_units=(32,), latent_dim=6, clipnorm=0.05, lr=5e-3),
}


def _problem(kw, n=300):
  spec, cfg = make_pair(**kw)
  x = synth_counts(n, spec.n_genes, sparsity=0.85, seed=0)
  ys = synth_labels(n, spec.extra_outputs + spec.labels)
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]], dtype=np.float32), (n, 1))
  mask = so.label_mask(n, 0.4, n_omics=1 + len(spec.labels), seed=1)
  return spec, cfg, x, ys, lib, mask


def _slots(name, params, seed=9):
  """non-trivial slots, fp32-representable: momentum accumulators of either sign, positive second-moment / accumulator slots"""
  rng = np.random.default_rng(seed)
  f32 = lambda a: a.astype(np.float32).astype(np.float64)
  m = {k: f32(1e-3 * rng.normal(size=v.shape)) for k, v in params.items()}
  v = {k: f32(rng.uniform(1e-6, 1e-4, size=v.shape)) for k, v in params.items()}
  return m, v


def _set_rule(e, name, hp, m=None, v=None):
  assert e.set_optimizer(name, **hp)
  if m is not None:
    e.set_params(m, 2)
    e.set_params(v, 3)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_single_launch_matches_reference(Engine, setting):
  """smx_k_opt: the optimiser launch by itself over several tensors (one of them clipped) at the rule's 5th step."""
  from sisua_amd.engine import k_opt
  name, hp = SETTINGS[setting]
  from sisua_amd.optimizers import canonical
  _, full = canonical(name, **hp)
  rng = np.random.default_rng(2)
  shapes = [(70, 33), (129,), (5000,), (4, 4)]
  f32 = lambda a: a.astype(np.float32).astype(np.float64)
  P = [f32(rng.normal(size=s)) for s in shapes]
  G = [f32(rng.normal(size=s) * (50.0 if i == 2 else 0.01)) for i, s in enumerate(shapes)]
  M = [f32(1e-3 * rng.normal(size=s)) for s in shapes]
  V = [f32(rng.uniform(1e-6, 1e-4, size=s)) for s in shapes]
  lr, clip, t = 1e-2, 5.0, 5
  p, m, v, norms = k_opt(name, P, G, M, V, t, lr=lr, clipnorm=clip, **hp)
  for i in range(len(shapes)):
    n = np.linalg.norm(G[i])
    assert np.isclose(norms[i], n, rtol=1e-5)
    g = G[i] * (clip / n if n > clip else 1.0)
    rm, rv, rw = rule_apply(name, full, lr, t, g, M[i], V[i], P[i])
    assert rel_l2(m[i], rm, floor=1e-12) < RTOL and rel_l2(v[i], rv, floor=1e-12) < RTOL, (i, rel_l2(m[i], rm), rel_l2(v[i], rv))
    # (the move next to the float32 rounding of the weights themselves: lr g is 1e-4 of |w| for the small gradients)
    tol = RTOL * np.abs(rw - P[i]).max() + 2 * np.finfo(np.float32).eps * np.abs(P[i]).max()
    assert np.abs(p[i] - rw).max() <= tol, (i, np.abs(p[i] - rw).max(), tol)
  assert np.linalg.norm(G[2]) > clip


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("case", list(CASES))
def test_one_step_matches_reference(Engine, with_rule, case, setting):
  name, hp = SETTINGS[setting]
  spec, cfg, x, ys, lib, mask = _problem(CASES[case])
  params = perturbed_params(spec)
  m0, v0 = _slots(name, params)
  opt = init_opt(name, params, **hp)
  opt["m"], opt["v"] = {k: a.copy() for k, a in m0.items()}, {k: a.copy() for k, a in v0.items()}
  bn = so.init_bn_state(spec)
  e = Engine(cfg, max_batch=64, init=False)
  e.set_params(params)
  _set_rule(e, name, hp, m0, v0)
  e.upload(x, ys, lib, mask, cell_id_base=1000)
  rows = np.random.default_rng(1).choice(x.shape[0], size=64, replace=False).astype(np.int32)
  p0 = {k: a.copy() for k, a in params.items()}
  res = so.train_step(spec, params, bn, opt, x[rows], so.PhiloxNoise(spec.seed, 0, rows + 1000), y=[y[rows] for y in ys],
                      library=lib[rows], mask=mask[rows])
  got = e.train_step(rows)
  assert got["nan_flag"] == 0 and np.isclose(got["loss"], res["metrics"]["loss"], rtol=RTOL, atol=1e-5)
  worst = grad_errors(e.get_params(1), res["grads"])
  assert max(worst.values()) < RTOL, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  uses = {"m": name in ("adamax",) or (name in ("sgd", "rmsprop") and hp.get("momentum", 0) > 0), "v": name in ("rmsprop", "adagrad", "adamax")}
  for which, key, start in ((2, "m", m0), (3, "v", v0)):
    dev = e.get_params(which)
    if not uses[key]:   # a slot the rule does not use is left as it was
      for k in dev:
        assert np.array_equal(dev[k], start[k].astype(np.float32)), (key, k)
      continue
    err = {k: rel_l2(dev[k] - start[k], opt[key][k] - start[k], floor=max(1e-3 * np.linalg.norm(opt[key][k] - start[k]), 1e-12))
           for k in dev}
    assert max(err.values()) < 4e-4, (key, sorted(err.items(), key=lambda kv: -kv[1])[:3])
  newp = e.get_params()
  top = max(np.linalg.norm(g) for g in res["grads"].values())
  for k in newp:
    if np.linalg.norm(res["grads"][k]) > 1e-3 * top:
      err = masked_move_error(newp[k], p0[k], params[k], res["grads"][k], spec.lr)
      assert err is None or err < 2e-3, (k, err)
  assert e.get_optimizer()[0] == name
  e.close()


@pytest.mark.parametrize("setting", ["sgd_momentum", "adamax"])
def test_engine_switch_matches_reference(Engine, with_rule, setting):
  """Three Adam steps, then the rule: fresh slots, t0 = 3, and the next two steps are the float64 composition from the Adam-trained weights
  (Adamax's bias correction counts from the switch)."""
  name, hp = SETTINGS[setting]
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_zinb"])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=64, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask)
  rows = [np.arange(s * 50, s * 50 + 64, dtype=np.int32) % x.shape[0] for s in range(5)]
  for s in range(3):
    e.train_step(rows[s])
  params = {k: v.astype(np.float64) for k, v in e.get_params(0).items()}   # (the reference continues from the device's weights)
  bn = {f"{nm}/{w}": st[w].astype(np.float64) for (nm, _), st in zip(so.bn_manifest(spec), e.get_bn().values()) for w in ("moving_mean", "moving_var")}
  assert e.set_optimizer(name, **hp) and e.get_optimizer()[2] == 3
  for which in (2, 3):
    assert all(not np.any(a) for a in e.get_params(which).values())
  opt = init_opt(name, params, **hp)
  for s in (3, 4):
    res = so.train_step(spec, params, bn, opt, x[rows[s]], so.PhiloxNoise(spec.seed, s, rows[s]), y=[y[rows[s]] for y in ys],
                        library=lib[rows[s]], mask=mask[rows[s]])
    got = e.train_step(rows[s])
    assert np.isclose(got["loss"], res["metrics"]["loss"], rtol=RTOL, atol=1e-5), s
  err = grad_errors(e.get_params(2), opt["m"])
  assert max(err.values()) < 2e-3, sorted(err.items(), key=lambda kv: -kv[1])[:3]
  e.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_c2_trajectory_matches_reference(Engine, with_rule, setting):
  """100 steps at the C2 shape (B 128, 1998 genes, H 128, D 32, zinb) from the oracle's initial weights: the loss of every step within 1e-4."""
  name, hp = SETTINGS[setting]
  spec, cfg, x, ys, lib, mask = _problem(dict(model="vae", n_genes=1998, likelihood="zinb", enc_units=(128,), dec_units=(128,), latent_dim=32), n=1024)
  params = {k: v.copy() for k, v in so.init_params(spec).items()}
  bn, opt = so.init_bn_state(spec), init_opt(name, params, **hp)
  B, steps = 128, 100
  e = Engine(cfg, max_batch=B, init=False)
  e.set_params(params)
  _set_rule(e, name, hp)
  e.upload(x, ys, lib, mask)
  order = np.concatenate([so.epoch_order(x.shape[0], ep, shuffle=100, seed=1) for ep in range(13)])[: steps * B].astype(np.int32)
  e.train_steps(order, steps, B, graph=False)
  got = np.asarray(e.metrics_history(steps)["loss"], np.float64)
  ref = np.array([so.train_step(spec, params, bn, opt, x[order[s * B:(s + 1) * B]], so.PhiloxNoise(spec.seed, s, order[s * B:(s + 1) * B]))["loss"]
                  for s in range(steps)])
  assert np.allclose(got, ref, rtol=RTOL), (np.abs(got / ref - 1).max(), int(np.abs(got / ref - 1).argmax()))
  assert ref[-10:].mean() < ref[:10].mean()
  e.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_graph_replay_equals_eager_bitwise(Engine, setting):
  name, hp = SETTINGS[setting]
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_zinb"])
  outs = []
  for graph in (False, True):
    e = Engine(cfg, max_batch=64)
    e.upload(x, ys, lib, mask)
    e.train_steps(np.arange(64 * 2, dtype=np.int32) % x.shape[0], 2, 64, graph=graph)   # two Adam steps, then the rule from step 2
    e.set_optimizer(name, **hp)
    assert e.get_optimizer()[2] == 2
    order = (np.arange(64 * 6, dtype=np.int32) + 17) % x.shape[0]
    e.train_steps(order, 6, 64, graph=graph)
    outs.append((e.get_params(0), e.get_params(2), e.get_params(3), e.metrics_history(6)["loss"].copy()))
    e.close()
  for which in range(3):
    for k in outs[0][which]:
      assert np.array_equal(outs[0][which][k], outs[1][which][k]), (which, k)
  assert np.array_equal(outs[0][3], outs[1][3])


@pytest.mark.parametrize("setting", ["sgd", "sgd_nesterov", "rmsprop_momentum", "adagrad", "adamax"])
def test_head_sweep_equals_riders_bitwise(Engine, setting):
  """128 cells x 20 000 genes nb under head_fused: the heads' update as the background sweep (head_sweep 1) and as riders + the optimiser
  launch (head_sweep 0) give the same bits under every rule."""
  name, hp = SETTINGS[setting]
  spec, cfg = make_pair(model="vae", n_genes=20000, likelihood="nb", enc_units=(128,), dec_units=(128,), latent_dim=32)
  x = synth_counts(256, 20000, sparsity=0.93, seed=11, max_count=500)
  rng = np.random.default_rng(3)
  order = np.concatenate([rng.permutation(256)[:128] for _ in range(4)]).astype(np.int32)
  runs = []
  for sweep in (False, True):
    e = Engine(cfg, max_batch=128, init=False)
    e.set_params(so.init_params(spec))
    e.set_flag("head_fused", True)
    e.set_flag("head_sweep", sweep)
    _set_rule(e, name, hp)
    e.upload(x, cell_id_base=7, storage="u16")
    assert e.head_fused_bytes(128) > 0
    e.train_steps(order, 4, 128, graph=False)
    runs.append((e.metrics_history(4)["loss"].copy(), e.get_params(0), e.get_params(2), e.get_params(3)))
    e.close()
  assert np.array_equal(runs[0][0], runs[1][0])
  for which in (1, 2, 3):
    for k in runs[0][which]:
      assert np.array_equal(runs[0][which][k], runs[1][which][k]), (which, k)


@pytest.mark.parametrize("shard", [False, True])
@pytest.mark.parametrize("setting", ["sgd_momentum", "rmsprop_momentum", "adagrad", "adamax"])
def test_data_parallel_world4_matches_reference(Engine, with_rule, setting, shard):
  """World 4 over the loopback communicator, with and without opt_shard (the heads' slots sharded over the ranks): losses of every step
  and, after smx_opt_gather, the parameters and both slots of every rank against the float64 data-parallel contract."""
  from tests.test_gpu_dp import run_ranks
  name, hp = SETTINGS[setting]
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_zinb"], n=400)
  world, B, steps, base = 4, 32, 4, 1000
  rng = np.random.default_rng(5)
  rows = [rng.permutation(x.shape[0])[: B * world].astype(np.int32).reshape(world, B) for _ in range(steps)]
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), init_opt(name, params, **hp)
  engines = []
  for r in range(world):
    e = Engine(cfg, max_batch=64, init=False)
    e.set_params(params)
    _set_rule(e, name, hp)
    e.upload(x, ys, lib, mask, cell_id_base=base)
    engines.append(e)
  Engine.comm_init_local(engines)
  for e in engines:
    e.set_flag("opt_shard", shard)
  refs = [so.dp_train_step(spec, params, bn, opt, x, list(rows[s]), s, cell_base=base) for s in range(steps)]
  orders = [np.concatenate([rows[s][r] for s in range(steps)]) for r in range(world)]
  run_ranks([lambda r=r: engines[r].train_steps(orders[r], steps, B, graph=False, metrics=True) for r in range(world)])
  for r in range(world):
    h = engines[r].metrics_history(steps)["loss"]
    for s in range(steps):
      assert np.isclose(h[s], refs[s]["metrics"]["loss"], rtol=RTOL, atol=1e-5), (r, s)
  if shard:
    run_ranks([lambda r=r: engines[r].opt_gather() for r in range(world)])
  finals = [(e.get_params(0), e.get_params(2), e.get_params(3)) for e in engines]
  worst = grad_errors(finals[0][0], params)
  assert max(worst.values()) < 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  for which, key in ((1, "m"), (2, "v")):
    if (key == "m" and name == "adagrad"):
      continue
    err = grad_errors(finals[0][which], opt[key])
    assert max(err.values()) < 4e-3, (key, sorted(err.items(), key=lambda kv: -kv[1])[:3])
  for which in range(3):
    for k in finals[0][which]:
      for r in range(1, world):
        assert np.array_equal(finals[0][which][k], finals[r][which][k]), (which, k, r)
  for e in engines:
    e.close()


# ---- the model surface ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


def _sco(n=600, g=120):
  from sisua_amd.data import SingleCellOMIC
  return SingleCellOMIC(synth_counts(n, g, sparsity=0.8, seed=3), name="toy")


def _vae(api, sco):
  return api.VAE(outputs=sco.get_rv("transcriptomic"), latents=api.RVmeta(6, "diag", True, "Latents"),
                 encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True))


def test_resume_under_rmsprop_is_bitwise_an_uninterrupted_run(api, tmp_path):
  sco = _sco()
  ds = sco.create_dataset(batch_size=64, drop_remainder=True)
  opt = {"class_name": "RMSprop", "config": {"momentum": 0.5, "rho": 0.8}}
  whole = _vae(api, sco)
  whole.fit(ds, metadata=sco, epochs=4, optimizer=opt)
  first = _vae(api, sco)
  first.fit(ds, metadata=sco, epochs=2, optimizer=opt)
  path = os.path.join(tmp_path, "model")
  first.save_weights(path)
  z = np.load(path + ".npz")
  assert str(z["opt/name"]) == "rmsprop" and int(z["opt/t0"]) == 0
  resumed = api.load_model(path)
  name, hp, t0 = resumed._engine.get_optimizer()
  assert name == "rmsprop" and np.isclose(hp["momentum"], 0.5) and np.isclose(hp["rho"], 0.8) and t0 == 0
  resumed.fit(ds, metadata=sco, epochs=2, optimizer=opt)
  assert resumed.step == whole.step
  a, b = whole._engine.snapshot(), resumed._engine.snapshot()
  for key in ("params", "m", "v"):
    for k in a[key]:
      assert np.array_equal(a[key][k], b[key][k]), (key, k)
  assert np.array_equal(whole.train_history["loss"][-1], resumed.train_history["loss"][-1])


def test_switching_rules_starts_fresh(api):
  """fit with Adam, then with SGD (momentum): the slots start at zero and t0 is the step of the switch (the float64 composition of a
  switch: test_graph_replay_equals_eager_bitwise starts its rule at step 2, test_engine_switch_matches_reference below)."""
  sco = _sco()
  ds = sco.create_dataset(batch_size=64, drop_remainder=True, shuffle=0)
  model = _vae(api, sco)
  model.fit(ds, metadata=sco, epochs=1)
  e = model._engine
  n1 = e.step
  assert e.get_optimizer()[0] == "adam" and n1 > 0
  assert any(np.abs(a).max() > 0 for a in e.get_params(2).values())
  assert e.set_optimizer("sgd", momentum=0.9)
  assert e.get_optimizer()[2] == n1 and not e.set_optimizer("sgd", momentum=0.9)   # the same rule again: nothing changes
  for which in (2, 3):
    assert all(not np.any(a) for a in e.get_params(which).values()), which
  model.fit(ds, metadata=sco, epochs=1, optimizer={"class_name": "SGD", "config": {"momentum": 0.9}})
  assert e is model._engine and e.get_optimizer()[:1] == ("sgd",) and e.get_optimizer()[2] == n1
  assert e.step > n1 and any(np.abs(a).max() > 0 for a in e.get_params(2).values())
  assert e.set_optimizer("adamax") and e.get_optimizer()[2] == e.step
  assert all(not np.any(a) for a in e.get_params(2).values())


def test_fit_rule_is_the_engine_rule_and_not_adam(api):
  sco = _sco()
  ds = sco.create_dataset(batch_size=64, drop_remainder=True)
  a = _vae(api, sco)
  a.fit(ds, metadata=sco, epochs=2, optimizer="adagrad")
  b = _vae(api, sco)
  b._ensure_engine(64)
  assert b._engine.set_optimizer("adagrad")   # the engine's own rule first: fit then finds it in force and continues it
  b.fit(ds, metadata=sco, epochs=2, optimizer="Adagrad")
  c = _vae(api, sco)
  c.fit(ds, metadata=sco, epochs=2)
  pa, pb, pc = a._engine.get_params(), b._engine.get_params(), c._engine.get_params()
  for k in pa:
    assert np.array_equal(pa[k], pb[k]), k
  assert any(not np.array_equal(pa[k], pc[k]) for k in pa)
  assert np.array_equal(a.train_history["loss"], b.train_history["loss"])
  acc = a._engine.get_params(3)
  assert all(np.all(v >= np.float32(0.1)) for v in acc.values())   # Adagrad's accumulator: from 0.1 upwards


def test_adamax_fit_resumes_and_experiment_passes_the_rule(api, tmp_path):
  """train.optimizer=adamax of an Experiment reaches fit; re-running the experiment resumes the rule from its checkpoint."""
  from sisua_amd import train as T
  import inspect
  src = inspect.getsource(T.Experiment.on_train)
  assert "**tr" in src   # (the train block is handed to fit as it is)
  sco = _sco()
  ds = sco.create_dataset(batch_size=64, drop_remainder=True)
  m = _vae(api, sco)
  m.fit(ds, metadata=sco, epochs=1, optimizer="adamax")
  path = os.path.join(tmp_path, "model")
  m.save_weights(path)
  r = api.load_model(path)
  assert r._engine.get_optimizer()[0] == "adamax"
  r.fit(ds, metadata=sco, epochs=1, optimizer="adamax")
  m.fit(ds, metadata=sco, epochs=1, optimizer="adamax")
  for k, v in m._engine.get_params().items():
    assert np.array_equal(v, r._engine.get_params()[k]), k
