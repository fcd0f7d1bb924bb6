"""The 'bernoulli' and 'normal' heads on the device against the float64 oracle, taught the two kinds by tests/head_kinds_ref.py:
one step (loss, metrics, every gradient, the Adam moments, BatchNorm state), the label backward forms, saturated logits,
a trajectory, eval / forward, two draws per cell, and the model API (fit, predict, save / load, the joint marginal likelihood).
Tolerances of test_gpu_step.py."""
import os

import numpy as np
import pytest

from oracle import sisua_oracle as so
from tests import head_kinds_ref as ref
from tests.util import adam_state_errors, grad_errors, make_pair, masked_move_error, perturbed_params, synth_counts

pytestmark = pytest.mark.gpu
RTOL = 1e-4


@pytest.fixture(autouse=True)
def _oracle_knows_the_kinds(monkeypatch):
  ref.install(monkeypatch)


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


CASES = {
    "sisua_bernoulli_onehot": dict(model="sisua", n_genes=150, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=8,
                                   labels=((11, "bernoulli"), (5, "onehot")), alpha=10.0),
    "sisua_bernoulli_wide": dict(model="sisua", n_genes=110, likelihood="nb", enc_units=(40,), dec_units=(40,), latent_dim=6,
                                 labels=((70, "bernoulli"),)),   # (70 markers: every lane takes two columns, padding to 96)
    "sisua_normal": dict(model="sisua", n_genes=120, likelihood="nb", enc_units=(40,), dec_units=(40,), latent_dim=6, labels=((9, "normal"),)),
    "vae_zinb_normal": dict(model="vae", n_genes=140, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=8,
                            extra_outputs=((12, "normal"),)),
    "scalar_bernoulli": dict(model="scale", n_genes=130, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=8, n_components=5,
                             labels=((10, "bernoulli"),)),
    "scvi_bernoulli": dict(model="scvi", n_genes=160, likelihood="zinbd", enc_units=(48,), dec_units=(48,), latent_dim=6, encl_units=(16,),
                           extra_outputs=((12, "bernoulli"),)),
}


def _problem(kw, n=300, seed=0, probabilities=False):
  spec, cfg = make_pair(**kw)
  x = synth_counts(n, spec.n_genes, sparsity=0.85, seed=seed, max_count=2000)
  ys = ref.synth_targets(n, spec.extra_outputs + spec.labels, probabilities=probabilities)
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]], dtype=np.float32), (n, 1))
  mask = so.label_mask(n, 0.4, n_omics=1 + len(spec.labels), seed=1)
  return spec, cfg, x, ys, lib, mask


def _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, step, cell_base=0):
  noise = so.PhiloxNoise(spec.seed, step, rows + cell_base)
  return so.train_step(spec, params, bn, opt, x[rows], noise, y=[y[rows] for y in ys], library=lib[rows], mask=mask[rows])


def _check_step(e, m, res, spec, bn, opt, params, p0):
  assert m["nan_flag"] == 0
  keys = ["loss", "nllk_x", "kl", "nllk_o"] + (["nllk_y"] if spec.labels else []) + (["kl_l"] if spec.model == "scvi" else [])
  for key in keys:
    assert np.isfinite(m[key]) and np.isclose(m[key], res["metrics"][key], rtol=RTOL, atol=1e-5), (key, m[key], res["metrics"][key])
  assert (m["nllk_o"] != 0) == bool(spec.extra_outputs) and (not spec.labels or m["nllk_y"] != 0)
  worst = grad_errors(e.get_params(which=1), res["grads"])
  assert max(worst.values()) < RTOL, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  em, ev, where = adam_state_errors(e, opt)
  assert em < 2e-4 and ev < 4e-4, (em, ev, where)
  got = e.get_params()
  for k in got:
    assert np.abs(got[k] - params[k]).max() <= 1.001 * spec.lr, k
    if k.startswith("lab"):
      err = masked_move_error(got[k], p0[k], params[k], res["grads"][k], spec.lr)
      assert err is None or err < 2e-3, (k, err)
  names = [p for p, _ in so.bn_manifest(spec)]
  for i, st in e.get_bn().items():
    assert np.allclose(st["moving_mean"], bn[f"{names[i]}/moving_mean"], rtol=1e-4, atol=1e-6)
    assert np.allclose(st["moving_var"], bn[f"{names[i]}/moving_var"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("batch", [32, 100, 160])
def test_one_step_matches_oracle(Engine, name, batch):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=max(128, batch), init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=1000)
  rows = np.random.default_rng(1).choice(x.shape[0], size=batch, replace=False).astype(np.int32)
  p0 = {k: v.copy() for k, v in params.items()}
  res = _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, 0, cell_base=1000)
  m = e.train_step(rows)
  assert m["step"] == 1
  _check_step(e, m, res, spec, bn, opt, params, p0)
  e.close()


@pytest.mark.parametrize("flags", [("label_ride",), ("label_ride", "wgrad"), ("wgrad",), ("head_bwd",), ("bwd_front", "wgrad")])
@pytest.mark.parametrize("name", ["sisua_bernoulli_onehot", "sisua_normal", "vae_zinb_normal"])
def test_label_backward_forms_match_oracle(Engine, name, flags):
  """The heads' d d riding on the output head's backward launch, the grouped weight gradients, or the separate launches: same bar."""
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e, e0 = Engine(cfg, max_batch=128, init=False), Engine(cfg, max_batch=128, init=False)
  for eng in (e, e0):
    eng.set_params(params)
    eng.upload(x, ys, lib, mask, cell_id_base=1000)
  for f in flags:
    e.set_flag(f, False)
  rows = np.random.default_rng(1).choice(x.shape[0], size=96, replace=False).astype(np.int32)
  p0 = {k: v.copy() for k, v in params.items()}
  res = _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, 0, cell_base=1000)
  bn0 = {k: v.copy() for k, v in bn.items()}
  for eng in (e, e0):
    _check_step(eng, eng.train_step(rows), res, spec, bn0, opt, params, p0)
  for s in (1, 2):
    r2 = ((rows + 7 * s) % x.shape[0]).astype(np.int32)
    m, m0 = e.train_step(r2), e0.train_step(r2)
  assert np.isclose(m["loss"], m0["loss"], rtol=1e-5)
  e.close(); e0.close()


@pytest.mark.parametrize("bias", [30.0, -30.0, "alternating"])
def test_saturated_bernoulli_logits(Engine, bias):
  """Label biases of +-30: sigmoid and softplus at saturation (one exponential of -|l|), finite and on the oracle."""
  spec, cfg, x, ys, lib, mask = _problem(CASES["sisua_bernoulli_onehot"])
  params = perturbed_params(spec)
  b = params["lab0/b"]
  params["lab0/b"] = np.where(np.arange(b.size) % 2 == 0, 30.0, -30.0) if bias == "alternating" else np.full_like(b, bias)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=1000)
  rows = np.random.default_rng(2).choice(x.shape[0], size=100, replace=False).astype(np.int32)
  p0 = {k: v.copy() for k, v in params.items()}
  res = _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, 0, cell_base=1000)
  m = e.train_step(rows)
  assert m["nllk_y"] > 10.0   # (the wrong side of a saturated logit costs ~30 nats per marker)
  _check_step(e, m, res, spec, bn, opt, params, p0)
  assert all(np.isfinite(g).all() for g in e.get_params(which=1).values())
  e.close()


@pytest.mark.parametrize("name,graph", [("sisua_bernoulli_onehot", True), ("sisua_normal", False), ("vae_zinb_normal", True),
                                        ("scvi_bernoulli", False)])
def test_trajectory_matches_oracle(Engine, name, graph):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name], n=512)
  params = {k: v.copy() for k, v in so.init_params(spec).items()}
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  B, steps = 64, 20
  e = Engine(cfg, max_batch=B, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask)
  order = np.concatenate([so.epoch_order(x.shape[0], ep, shuffle=100, seed=1) for ep in range(3)])[: steps * B].astype(np.int32)
  ref_l, got = [], []
  for s in range(steps):
    rows = order[s * B:(s + 1) * B]
    ref_l.append(_oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, s)["loss"])
    got.append(e.train_step(rows, graph=graph)["loss"])
  ref_l, got = np.array(ref_l), np.array(got)
  assert np.allclose(got, ref_l, rtol=RTOL), np.abs(got / ref_l - 1).max()
  assert np.median(ref_l[-5:]) < np.median(ref_l[:5])   # and it trains (medians: one hard minibatch of scVI's library term is an outlier)
  e.close()


@pytest.mark.parametrize("name", ["sisua_bernoulli_onehot", "sisua_normal", "vae_zinb_normal", "scvi_bernoulli"])
def test_eval_and_forward_match_oracle(Engine, name):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  rng = np.random.default_rng(2)
  for k in bn:
    bn[k] = (bn[k] + 0.2 * rng.uniform(size=bn[k].shape)).astype(np.float32).astype(np.float64)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  names = [p for p, _ in so.bn_manifest(spec)]
  e.set_bn({i: dict(moving_mean=bn[f"{n}/moving_mean"], moving_var=bn[f"{n}/moving_var"]) for i, n in enumerate(names)})
  e.upload(x, ys, lib, mask)
  rows = np.arange(40, 140, dtype=np.int32)
  noise = so.PhiloxNoise(spec.seed, 0, rows, sample=0)
  res = so.forward_backward(spec, params, bn, x[rows], noise, y=[y[rows] for y in ys], library=lib[rows],
                            mask=mask[rows], training=False, backward=False)
  m = e.eval_step(rows)
  assert np.isclose(m["loss"], res["loss"], rtol=RTOL)
  for key in ("nllk_o",) + (("nllk_y",) if spec.labels else ()):
    assert np.isclose(m[key], res["metrics"][key], rtol=RTOL, atol=1e-5), key
  out = e.forward(row_ids=rows, sample_index=0)
  assert len(out["y_params"]) == len(spec.extra_outputs + spec.labels)
  for j in range(len(out["y_params"])):
    assert out["y_params"][j].shape == res["y_params"][j].shape
    assert np.allclose(out["y_params"][j], res["y_params"][j], rtol=1e-3, atol=1e-4)
  e.close()


def test_two_draws_per_cell_match_the_repeated_minibatch(Engine):
  """Two draws per cell (fit(sample_shape=2)): the oracle's unchanged step on the minibatch repeated twice, draw-major."""
  from tests.test_train_draws_host import DrawNoise
  spec, cfg, x, ys, lib, mask = _problem(CASES["sisua_bernoulli_onehot"])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=1000)
  e.set_train_draws(2)
  rows = np.random.default_rng(1).choice(x.shape[0], size=64, replace=False).astype(np.int32)
  rep = np.tile(rows, 2)
  p0 = {k: v.copy() for k, v in params.items()}
  res = so.train_step(spec, params, bn, opt, x[rep], DrawNoise(spec.seed, 0, rows + 1000, 2), y=[y[rep] for y in ys],
                      library=lib[rep], mask=mask[rep])
  m = e.train_step(rows)
  assert m["step"] == 1
  _check_step(e, m, res, spec, bn, opt, params, p0)
  e.close()


# ---- the model API --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


def _markers_sco(probabilities):
  from sisua_amd.data import SingleCellOMIC
  n, P = 600, 8
  x = synth_counts(n, 120, sparsity=0.8, seed=3)
  # markers that follow the cells' expression: a logistic read-out of a few genes' log counts, thresholded (or not)
  rng = np.random.default_rng(4)
  lx = np.log1p(x)
  act = (lx - lx.mean(0)) @ rng.normal(0.0, 0.6, size=(120, P)) + rng.normal(0.0, 0.5, size=(1, P))
  prob = 1.0 / (1.0 + np.exp(-act))
  sco = SingleCellOMIC(x, name="toy")
  sco.add_omic("proteomic", (prob if probabilities else (prob > 0.5)).astype(np.float32))
  return sco, P


@pytest.mark.parametrize("probabilities", [False, True])
def test_sisua_bernoulli_fit_predict_save_load(api, tmp_path, probabilities):
  from sisua_amd import distributions as D
  sco, P = _markers_sco(probabilities)
  train, test = sco.split(0.8)
  kw = dict(outputs=sco.get_rv("transcriptomic"), labels=[api.RVmeta(P, "bernoulli", name="proteomic")],
            latents=api.RVmeta(8, "diag", True, "Latents"), encoder=api.NetConf([32], batchnorm=True, dropout=0.1),
            decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  m = api.SISUA(**kw)
  assert m._make_config().labels == ((P, "bernoulli"),)
  omics = ["transcriptomic", "proteomic"]
  m.fit(train.create_dataset(omics, labels_percent=0.5, batch_size=64, drop_remainder=True), metadata=sco, epochs=12,
        learning_rate=2e-3, verbose=False)
  h = np.asarray(m.train_history["nllk_y"])
  assert len(h) == 12 and np.isfinite(m.train_history["loss"]).all() and np.isfinite(h).all()
  assert h[-3:].mean() < h[:3].mean(), h
  X = test.numpy()[:100]
  (pX, pY), qZ = m.predict(X, verbose=False)
  assert isinstance(pY, D.Independent) and isinstance(pY.distribution, D.Bernoulli) and pY.name == "proteomic"
  assert pY.batch_shape == (100,) and pY.event_shape == (P,)
  mean = pY.mean()
  assert mean.shape == (100, P) and (mean > 0).all() and (mean < 1).all()
  lp = pY.log_prob(test.numpy("proteomic")[:100])
  assert lp.shape == (100,) and np.isfinite(lp).all()
  (sX, sY), _ = m.predict(X, sample_shape=2, verbose=False)
  assert sY.batch_shape == (2, 100) and sY.sample(seed=1).shape == (2, 100, P)
  path = os.path.join(tmp_path, "sisua_bernoulli")
  m.save_weights(path)
  m2 = api.SISUA(**kw).load_weights(path)
  (_, pY2), _ = m2.predict(X, verbose=False)
  assert np.array_equal(pY2.distribution.logits, pY.distribution.logits)
  if not probabilities:   # two draws per cell in training: finite, and the labels are still learnt
    m3 = api.SISUA(**kw)
    m3.fit(train.create_dataset(omics, labels_percent=0.5, batch_size=64, drop_remainder=True), metadata=sco, epochs=6,
           learning_rate=2e-3, sample_shape=2, verbose=False)
    h3 = np.asarray(m3.train_history["nllk_y"])
    assert np.isfinite(m3.train_history["loss"]).all() and h3[-2:].mean() < h3[:2].mean(), h3


@pytest.mark.parametrize("posterior", ["diag", "normal"])
def test_vae_with_a_normal_second_output(api, posterior):
  """VAE(outputs=[zinb, RVmeta(P, 'diag')]): the second output trains, predicts as MultivariateNormalDiag ('diag') or
  Independent(Normal) ('normal'), and the joint marginal log p(x, y) matches the oracle's."""
  from sisua_amd import distributions as D
  from sisua_amd.data import SingleCellOMIC
  x = synth_counts(600, 120, sparsity=0.8, seed=3)
  P = 7
  ys = ref.synth_targets(600, ((P, "normal"),))[0]
  sco = SingleCellOMIC(x, name="toy")
  sco.add_omic("proteomic", ys)
  kw = dict(latents=api.RVmeta(8, "diag", True, "Latents"), encoder=api.NetConf([32], batchnorm=True, dropout=0.1),
            decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  vae = api.VAE(outputs=[api.RVmeta(120, "zinb", name="transcriptomic"), api.RVmeta(P, posterior, name="proteomic")], **kw)
  assert vae._make_config().extra_outputs == ((P, "normal"),)
  vae.fit(sco, epochs=8, batch_size=64, learning_rate=2e-3, verbose=False)
  h = vae.train_history["nllk_o"]
  assert np.isfinite(h).all() and h[-1] < h[0]
  X, Y = sco.numpy()[:128], sco.numpy("proteomic")[:128]
  (pX, pY), qZ = vae.predict(X, sample_shape=2, verbose=False)
  if posterior == "diag":
    assert isinstance(pY, D.MultivariateNormalDiag)
  else:
    assert isinstance(pY, D.Independent) and isinstance(pY.distribution, D.Normal)
  assert pY.batch_shape == (2, 128) and pY.event_shape == (P,) and (pY.stddev() > 0).all()
  mllk, llk = vae.marginal_log_prob(inputs=[X[:40], Y[:40]], sample_shape=6, batch_size=64)
  assert set(llk) == {"transcriptomic", "proteomic"} and mllk.shape == (40,)
  spec = so.Spec(**vae._make_config().to_dict())
  e = vae._engine
  params = {k: v.astype(np.float64) for k, v in e.get_params().items()}
  names = [p for p, _ in so.bn_manifest(spec)]
  bn = {}
  for i, st in e.get_bn().items():
    bn[f"{names[i]}/moving_mean"], bn[f"{names[i]}/moving_var"] = st["moving_mean"].astype(np.float64), st["moving_var"].astype(np.float64)
  ref_m, ref_l = so.marginal_log_prob(spec, params, bn, X[:40], np.arange(40), 6, y=[Y[:40]])
  assert np.allclose(mllk, ref_m, rtol=1e-4, atol=1e-2), np.abs(mllk - ref_m).max()
  assert np.allclose(llk["transcriptomic"], ref_l, rtol=1e-4, atol=1e-2)
