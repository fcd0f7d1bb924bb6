"""Hidden-layer activations other than ReLU (NetConf(activation=...), smx_set_activation) on the device against the float64 oracle,
taught them by tests/activations_ref.py: single steps (loss, every gradient, the Adam moments, BatchNorm state) for every activation
with and without BatchNorm under hidden and input dropout, the BatchNorm launch forms by width, every model family, a mixed model, the
exact keep mask, a trajectory, two draws per cell, data parallelism with and without SyncBatchNorm, eval / forward, the marginal
likelihood and the posterior log-likelihood, and fit -> save -> load.  Tolerances of test_gpu_step.py."""
import dataclasses

import numpy as np
import pytest

from oracle import sisua_oracle as so
from tests import activations_ref as ref
from tests.util import adam_state_errors, grad_errors, make_pair, perturbed_params, synth_counts, synth_labels

pytestmark = pytest.mark.gpu
RTOL = 1e-4
BASE = 1000
GENERAL = ("linear", "leaky_relu", "elu", "selu", "tanh", "sigmoid", "softplus")


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _problem(kw, enc="relu", dec="relu", encl="relu", n=300, seed=0):
  spec, cfg = make_pair(**kw)
  cfg = dataclasses.replace(cfg, enc_activation=enc, dec_activation=dec, encl_activation=encl)
  x = synth_counts(n, spec.n_genes, sparsity=0.85, seed=seed, max_count=2000 if spec.n_genes < 500 else None)
  ys = synth_labels(n, spec.extra_outputs + spec.labels)
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]], dtype=np.float32), (n, 1))
  mask = so.label_mask(n, 0.4, n_omics=1 + len(spec.labels), seed=1)
  return spec, cfg, x, ys, lib, mask


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


def _one_step(Engine, monkeypatch, kw, enc, dec=None, encl="relu", batch=100, params=None, S=1):
  dec = enc if dec is None else dec
  ref.install(monkeypatch, enc=enc, dec=dec, encl=encl)
  spec, cfg, x, ys, lib, mask = _problem(kw, enc, dec, encl)
  params = perturbed_params(spec) if params is None else params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask, max_batch=max(128, batch))
  if S > 1:
    e.set_train_draws(S)
  rows = np.random.default_rng(1).choice(x.shape[0], size=batch, replace=False).astype(np.int32)
  rep = np.tile(rows, S)
  if S > 1:
    from tests.test_train_draws_host import DrawNoise
    noise = DrawNoise(spec.seed, 0, rows + BASE, S)
  else:
    noise = so.PhiloxNoise(spec.seed, 0, rows + BASE)
  res = so.train_step(spec, params, bn, opt, x[rep], noise, y=[y[rep] for y in ys], library=lib[rep], mask=mask[rep])
  m = e.train_step(rows)
  _check_step(e, m, res, spec, bn, opt)
  e.close()


DROP = dict(dropout_enc=0.2, dropout_dec=0.2, input_dropout=0.2)


@pytest.mark.parametrize("bnorm", [True, False])
@pytest.mark.parametrize("act", GENERAL)
def test_one_step_every_activation(Engine, monkeypatch, act, bnorm):
  kw = dict(model="vae", n_genes=150, likelihood="zinb", enc_units=(64,), dec_units=(64,), latent_dim=10, batchnorm=bnorm, **DROP)
  _one_step(Engine, monkeypatch, kw, act)


# the BatchNorm launch forms: 32 units, 128 units (the latent-sample / dense fronts a ReLU layer would take), two encoder layers, batches
# beyond the register-resident forms, and a wide panel (column-major slabs summed by bn_wide_fwd / bwd)
@pytest.mark.parametrize("act", ["elu", "tanh"])
@pytest.mark.parametrize("shape,batch", [
    (dict(enc_units=(32,), dec_units=(32,), latent_dim=8), 64),
    (dict(enc_units=(128,), dec_units=(128,), latent_dim=32), 128),
    (dict(enc_units=(64, 64), dec_units=(64, 64), latent_dim=16), 200),
    (dict(enc_units=(48, 40), dec_units=(40,), latent_dim=10), 256),
])
def test_one_step_launch_forms(Engine, monkeypatch, act, shape, batch):
  kw = dict(model="vae", n_genes=180, likelihood="zinb", **shape, **DROP)
  _one_step(Engine, monkeypatch, kw, act, batch=batch)


@pytest.mark.parametrize("act", ["selu", "softplus"])
def test_one_step_wide_panel(Engine, monkeypatch, act):
  kw = dict(model="vae", n_genes=4600, likelihood="zinb", enc_units=(128,), dec_units=(128,), latent_dim=32, dropout_enc=0.1, dropout_dec=0.1)
  _one_step(Engine, monkeypatch, kw, act, batch=128)


MODELS = {
    "sisua": dict(model="sisua", n_genes=140, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=8,
                  labels=((6, "nb"), (5, "onehot")), alpha=10.0, **DROP),
    "scvi": dict(model="scvi", n_genes=160, likelihood="zinbd", enc_units=(48,), dec_units=(48,), latent_dim=6, encl_units=(16,), **DROP),
    "dca": dict(model="dca", n_genes=120, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=8, **DROP),
    "scale": dict(model="scale", n_genes=130, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=8, n_components=5, **DROP),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_one_step_model_families(Engine, monkeypatch, name):
  # scvi: the library encoder's activation differs from the encoder's
  _one_step(Engine, monkeypatch, MODELS[name], "elu", dec="tanh", encl="sigmoid" if name == "scvi" else "relu")


def test_mixed_model_and_relu_decoder(Engine, monkeypatch):
  kw = dict(model="vae", n_genes=150, likelihood="nb", enc_units=(64, 64), dec_units=(64,), latent_dim=12, **DROP)
  _one_step(Engine, monkeypatch, kw, "elu", dec="tanh")
  _one_step(Engine, monkeypatch, kw, "selu", dec="relu")   # (the ReLU decoder keeps its fused forms beside a general encoder)


@pytest.mark.parametrize("act", ["linear", "tanh"])
def test_keep_mask_is_exact_where_kept_outputs_are_zero(Engine, monkeypatch, act):
  """One encoder column with gamma = beta = 0: its kept outputs are exactly 0 with a non-zero derivative.  A mask read from out != 0
  drops them, and that column's d beta comes out wrong."""
  def params(spec):
    p = perturbed_params(spec)
    p["enc0/gamma"][3] = 0.0
    p["enc0/beta"][3] = 0.0
    return p
  kw = dict(model="vae", n_genes=150, likelihood="zinb", enc_units=(64,), dec_units=(64,), latent_dim=10, **DROP)
  _one_step(Engine, monkeypatch, kw, act, params=params)


def test_two_draws_per_cell(Engine, monkeypatch):
  kw = dict(model="vae", n_genes=150, likelihood="zinb", enc_units=(64,), dec_units=(64,), latent_dim=10, **DROP)
  _one_step(Engine, monkeypatch, kw, "elu", dec="tanh", batch=64, S=2)


@pytest.mark.parametrize("act", ["elu", "tanh"])
def test_trajectory(Engine, monkeypatch, act):
  ref.install(monkeypatch, enc=act, dec=act)
  kw = dict(model="vae", n_genes=150, likelihood="zinb", enc_units=(64,), dec_units=(64,), latent_dim=10, **DROP)
  spec, cfg, x, ys, lib, mask = _problem(kw, act, act)
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  rng = np.random.default_rng(4)
  for s in range(20):
    rows = rng.choice(x.shape[0], size=64, replace=False).astype(np.int32)
    res = so.train_step(spec, params, bn, opt, x[rows], so.PhiloxNoise(spec.seed, s, rows + BASE))
    m = e.train_step(rows)
    assert np.isclose(m["loss"], res["metrics"]["loss"], rtol=1e-3, atol=1e-3), (s, m["loss"], res["metrics"]["loss"])
  worst = grad_errors(e.get_params(0), params)
  assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  e.close()


@pytest.mark.parametrize("sync_bn", [False, True])
def test_data_parallel_loopback(Engine, monkeypatch, sync_bn):
  from tests.test_gpu_dp import run_ranks
  ref.install(monkeypatch, enc="elu", dec="tanh")
  kw = dict(model="vae", n_genes=150, likelihood="zinb", enc_units=(64,), dec_units=(64,), latent_dim=10, **DROP)
  spec, cfg, x, ys, lib, mask = _problem(kw, "elu", "tanh", n=400)
  world, B, steps = 2, 32, 3
  rng = np.random.default_rng(5)
  rows = [rng.permutation(x.shape[0])[: B * world].astype(np.int32).reshape(world, B) for _ in range(steps)]
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  engines = [_engine(Engine, cfg, params, x, ys, lib, mask, max_batch=64) for _ in range(world)]
  Engine.comm_init_local(engines)
  for e in engines:
    e.set_sync_bn(sync_bn)
  refs = [so.dp_train_step(spec, params, bn, opt, x, list(rows[s]), s, cell_base=BASE, sync_bn=sync_bn) for s in range(steps)]
  orders = [np.concatenate([rows[s][r] for s in range(steps)]) for r in range(world)]
  run_ranks([lambda r=r: engines[r].train_steps(orders[r], steps, B, graph=False, metrics=True) for r in range(world)])
  for r in range(world):
    h = engines[r].metrics_history(steps)["loss"]
    for s in range(steps):
      assert np.isclose(h[s], refs[s]["metrics"]["loss"], rtol=RTOL, atol=1e-5), (r, s)
  worst = grad_errors(engines[0].get_params(0), params)
  assert max(worst.values()) < 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  for e in engines:
    e.close()


@pytest.mark.parametrize("bnorm", [True, False])
def test_eval_and_forward(Engine, monkeypatch, bnorm):
  ref.install(monkeypatch, enc="selu", dec="softplus")
  kw = dict(model="vae", n_genes=150, likelihood="zinb", enc_units=(64,), dec_units=(48, 64), latent_dim=10, batchnorm=bnorm, **DROP)
  spec, cfg, x, ys, lib, mask = _problem(kw, "selu", "softplus")
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  rng = np.random.default_rng(2)
  for k in bn:
    bn[k] = (bn[k] + 0.2 * rng.uniform(size=bn[k].shape)).astype(np.float32).astype(np.float64)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  names = [p for p, _ in so.bn_manifest(spec)]
  if names:
    e.set_bn({i: dict(moving_mean=bn[f"{n}/moving_mean"], moving_var=bn[f"{n}/moving_var"]) for i, n in enumerate(names)})
  e.upload(x, ys, lib, mask)
  rows = np.arange(40, 140, dtype=np.int32)
  res = so.forward_backward(spec, params, bn, x[rows], so.PhiloxNoise(spec.seed, 0, rows, sample=0), library=lib[rows],
                            training=False, backward=False)
  m = e.eval_step(rows)
  assert np.isclose(m["loss"], res["loss"], rtol=RTOL)
  out = e.forward(row_ids=rows, sample_index=0)
  assert np.allclose(out["z_mean"], res["z_mean"], rtol=1e-4, atol=1e-5)
  for c in range(spec.k):
    assert np.allclose(out["x_params"][c], res["x_params"][c], rtol=1e-3, atol=1e-4)
  # decode (the stacked eval decoder of predict) on the forward pass's own draw: the same heads
  dec = e.decode(out["z_sample"])
  for c in range(spec.k):
    assert np.allclose(dec["x_params"][c], out["x_params"][c], rtol=1e-4, atol=1e-5)
  e.close()


@pytest.mark.parametrize("dec_units", [(64,), (48, 64)])
@pytest.mark.parametrize("stacked", [True, False])
def test_marginal_and_posterior_llk(Engine, monkeypatch, dec_units, stacked):
  ref.install(monkeypatch, enc="tanh", dec="elu")
  kw = dict(model="vae", n_genes=150, likelihood="zinb", enc_units=(64,), dec_units=dec_units, latent_dim=10, **DROP)
  spec, cfg, x, ys, lib, mask = _problem(kw, "tanh", "elu")
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  e = Engine(cfg, max_batch=64, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=500)
  if not stacked:
    e.set_flag("stacked_scoring", False)
  rows = np.arange(20, 70, dtype=np.int32)
  S = 12
  ref_m, ref_l = so.marginal_log_prob(spec, params, bn, x[rows], rows + 500, S, library=lib[rows])
  got_m, got_l = e.marginal_llk(row_ids=rows, n_samples=S)
  assert np.allclose(got_m, ref_m, rtol=RTOL, atol=1e-3), np.abs(got_m - ref_m).max()
  assert np.allclose(got_l, ref_l, rtol=RTOL, atol=1e-3)
  e.close()


def test_fit_save_load_predict(Engine, tmp_path):
  import sisua_amd.models as M
  from sisua_amd.config import NetConf, RVmeta
  from sisua_amd.data import SingleCellOMIC
  sco = SingleCellOMIC(synth_counts(400, 120, sparsity=0.8, seed=3), name="toy")
  train, test = sco.split(0.8)
  kw = dict(outputs=sco.get_rv("transcriptomic"), latents=RVmeta(6, "diag", True, "Latents"),
            encoder=NetConf([32], batchnorm=True, dropout=0.1, activation="elu"), decoder=NetConf([16, 32], batchnorm=True, activation="Tanh"))
  m1 = M.VAE(**kw)
  m1.fit(train, epochs=2, batch_size=64)
  assert m1._engine.cfg.enc_activation == "elu" and m1._engine.cfg.dec_activation == "tanh"
  x_1, z_1 = m1.predict(test.numpy(), batch_size=64, verbose=False)
  path = str(tmp_path / "model")
  m1.save_weights(path)
  m2 = M.load_model(path)
  assert m2.encoder.activation == "elu" and m2.decoder.activation == "tanh"
  x_2, z_2 = m2.predict(test.numpy(), batch_size=64, verbose=False)
  assert np.array_equal(np.asarray(z_1.mean()), np.asarray(z_2.mean()))
  assert np.array_equal(np.asarray(x_1.mean()), np.asarray(x_2.mean()))
  ll1 = m1.posterior_llk(test.numpy()[:16], sample_shape=4)
  ll2 = m2.posterior_llk(test.numpy()[:16], sample_shape=4)
  assert set(ll1) == set(ll2)
  for k in ll1:
    a, b = np.asarray(ll1[k], dtype=np.float64), np.asarray(ll2[k], dtype=np.float64)
    assert np.isfinite(a).all() and np.array_equal(a, b), k
