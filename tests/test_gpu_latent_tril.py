"""RVmeta(D, 'mvntril'): the full-covariance latent posterior on the device against the float64 reference (tests/latent_tril_ref.py):
one step (loss, metrics, every gradient, the Adam moments, BatchNorm state) for VAE, SISUA, MISA and SCVI under Philox and injected
noise, the identity with the diagonal model at L = sigma I, a trajectory, several draws per cell, a data-parallel loopback step, encode /
predict / multi-draw samples, the marginal likelihoods, and the model API (fit, save / load, the CSR store).  Tolerances of
test_gpu_step.py."""
import os

import numpy as np
import pytest

from oracle import sisua_oracle as so
from tests import latent_tril_ref as ref
from tests.util import adam_state_errors, grad_errors, perturbed_params, rel_l2, synth_counts, synth_labels

pytestmark = pytest.mark.gpu
RTOL = 1e-4
BASE = 1000


@pytest.fixture(autouse=True)
def _oracle_knows_the_tril_latent(monkeypatch):
  ref.install(monkeypatch)


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


CASES = {
    "vae_zinb_d10": dict(model="vae", n_genes=150, likelihood="zinb", enc_units=(64,), dec_units=(48,), latent_dim=10),
    "vae_nb_d1": dict(model="vae", n_genes=90, likelihood="nb", enc_units=(32,), dec_units=(32,), latent_dim=1),
    "sisua_d7": dict(model="sisua", n_genes=130, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=7,
                     labels=((6, "nb"), (4, "onehot")), alpha=10.0),
    "misa_d10": dict(model="sisua", n_genes=120, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=10, labels=((5, "mixnb2"),)),
    "scvi_nbd_d32": dict(model="scvi", n_genes=140, likelihood="nbd", enc_units=(64,), dec_units=(64,), latent_dim=32, encl_units=(16,)),
    "scvi_zinbd_d7": dict(model="scvi", n_genes=160, likelihood="zinbd", enc_units=(48,), dec_units=(48,), latent_dim=7, encl_units=(16,)),
}


def _problem(kw, n=300, seed=0):
  spec, cfg = ref.make_pair(**kw)
  x = synth_counts(n, spec.n_genes, sparsity=0.85, seed=seed, max_count=2000)
  ys = synth_labels(n, spec.labels, seed=1)
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]], dtype=np.float32), (n, 1))
  mask = so.label_mask(n, 0.4, n_omics=1 + len(spec.labels), seed=1)
  return spec, cfg, x, ys, lib, mask


def _params(spec, seed=3):
  """Perturbed reference parameters with factor entries that matter (off-diagonals, diagonals away from softplus(0))."""
  p = perturbed_params(spec, seed=seed)
  rng = np.random.default_rng(seed + 10)
  p["lat/b"] = (p["lat/b"] + 0.3 * rng.normal(size=p["lat/b"].shape)).astype(np.float32).astype(np.float64)
  return p


def _engine(Engine, cfg, params, x, ys, lib, mask, max_batch=128):
  e = Engine(cfg, max_batch=max_batch, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=BASE)
  return e


def _check_step(e, m, res, spec, bn, opt):
  assert m["nan_flag"] == 0
  keys = ["loss", "nllk_x", "kl"] + (["nllk_y"] if spec.labels else []) + (["kl_l"] if spec.model == "scvi" else [])
  for key in keys:
    assert np.isfinite(m[key]) and np.isclose(m[key], res["metrics"][key], rtol=RTOL, atol=1e-5), (key, m[key], res["metrics"][key])
  worst = grad_errors(e.get_params(which=1), res["grads"])
  assert max(worst.values()) < RTOL, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  em, ev, where = adam_state_errors(e, opt)
  assert em < 2e-4 and ev < 4e-4, (em, ev, where)
  names = [p for p, _ in so.bn_manifest(spec)]
  for i, st in e.get_bn().items():
    assert np.allclose(st["moving_mean"], bn[f"{names[i]}/moving_mean"], rtol=1e-4, atol=1e-6)
    assert np.allclose(st["moving_var"], bn[f"{names[i]}/moving_var"], rtol=1e-4, atol=1e-6)


def _train_ref(spec, params, bn, opt, x, ys, lib, mask, rows, step, noise=None):
  noise = noise or so.PhiloxNoise(spec.seed, step, rows + BASE)
  return so.train_step(spec, params, bn, opt, x[rows], noise, y=[y[rows] for y in ys], library=lib[rows], mask=mask[rows])


@pytest.mark.parametrize("name", list(CASES))
def test_one_step_matches_reference(Engine, name):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = _params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  rows = np.random.default_rng(1).choice(x.shape[0], size=100, replace=False).astype(np.int32)   # (a ragged batch)
  res = _train_ref(spec, params, bn, opt, x, ys, lib, mask, rows, 0)
  m = e.train_step(rows)
  _check_step(e, m, res, spec, bn, opt)
  e.close()


@pytest.mark.parametrize("name", ["vae_zinb_d10", "sisua_d7", "scvi_nbd_d32"])
def test_injected_noise_matches_reference(Engine, name):
  kw = dict(CASES[name], dropout_enc=0.0, dropout_dec=0.0)
  spec, cfg, x, ys, lib, mask = _problem(kw)
  params = _params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  B = 72
  rows = np.arange(5, 5 + B, dtype=np.int32)
  rng = np.random.default_rng(9)
  normal = {so.STREAM_EPS_Z: rng.normal(size=(B, spec.latent_dim)).astype(np.float32)}
  if spec.model == "scvi":
    normal[so.STREAM_EPS_L] = rng.normal(size=(B, 1)).astype(np.float32)
  for s, v in normal.items():
    e.set_noise(s, v)
  res = _train_ref(spec, params, bn, opt, x, ys, lib, mask, rows, 0, noise=so.InjectedNoise({}, normal, {}))
  m = e.train_step(rows)
  _check_step(e, m, res, spec, bn, opt)
  e.close()


def test_identity_factor_is_the_diagonal_model(Engine):
  """Off-diagonal columns of lat/W and lat/b zero, diagonal columns zero with biases giving L_ii = sigma: the tril model's step is the
  diagonal model's at the constant sigma on the same Philox draws (loss, kl, every gradient outside the scale columns)."""
  from sisua_amd.config import ModelConfig
  kw = dict(model="vae", n_genes=120, likelihood="zinb", enc_units=(48,), dec_units=(48,), latent_dim=9)
  D = 9
  spec_d, cfg_d = so.Spec(**kw), ModelConfig(**kw)
  spec_t, cfg_t = ref.make_pair(**kw)
  pd = perturbed_params(spec_d)
  pt = {k: v.copy() for k, v in pd.items() if not k.startswith("lat/")}
  sigma = 0.8
  pd["lat/W"][:, D:] = 0.0
  pd["lat/b"][D:] = float(np.float32(np.log(np.expm1(sigma)) - so.SOFTPLUS_INV_1))
  pt["lat/W"] = np.zeros((pd["lat/W"].shape[0], (1 + D) * D))
  pt["lat/W"][:, :D] = pd["lat/W"][:, :D]
  pt["lat/b"] = np.zeros((1 + D) * D)
  pt["lat/b"][:D] = pd["lat/b"][:D]
  for i in range(D):
    pt["lat/b"][D + i * D + i] = float(np.float32(np.log(np.expm1(sigma - so.TRIL_DIAG_SHIFT))))
  x = synth_counts(200, 120, sparsity=0.85, seed=4)
  rows = np.arange(0, 96, dtype=np.int32)
  ms = []
  grads = []
  for cfg, p in ((cfg_d, pd), (cfg_t, pt)):
    e = Engine(cfg, max_batch=128, init=False)
    e.set_params(p)
    e.upload(x)
    ms.append(e.train_step(rows))
    grads.append(e.get_params(which=1))
    e.close()
  for key in ("loss", "nllk_x", "kl"):
    assert np.isclose(ms[0][key], ms[1][key], rtol=1e-5, atol=1e-5), (key, ms[0][key], ms[1][key])
  for k in grads[0]:
    a, b = grads[0][k], grads[1][k]
    if k.startswith("lat/"):
      a, b = a[..., :D], b[..., :D]
    assert rel_l2(b, a, floor=1e-3 * max(np.linalg.norm(v) for v in grads[0].values())) < RTOL, k


def test_trajectory_draws_and_data_parallel(Engine):
  """60 steps within tolerance of the reference; a step with S = 3 draws per cell; a world-2 loopback step equal to world 1."""
  from tests.test_gpu_dp import run_ranks
  from tests.test_train_draws_host import DrawNoise
  spec, cfg, x, ys, lib, mask = _problem(CASES["sisua_d7"], n=400)
  params = _params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  rng = np.random.default_rng(7)
  ref_l, got = [], []
  for step in range(60):
    rows = rng.choice(x.shape[0], size=64, replace=False).astype(np.int32)
    ref_l.append(_train_ref(spec, params, bn, opt, x, ys, lib, mask, rows, step)["loss"])
    got.append(e.train_step(rows)["loss"])
  ref_l, got = np.array(ref_l), np.array(got)
  assert np.allclose(got, ref_l, rtol=RTOL), np.abs(got / ref_l - 1).max()
  assert np.median(ref_l[-5:]) < np.median(ref_l[:5])
  e.close()
  # three draws per cell
  params = _params(spec, seed=5)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  e.set_train_draws(3)
  rows = rng.choice(x.shape[0], size=48, replace=False).astype(np.int32)
  rep = np.tile(rows, 3)
  res = so.train_step(spec, params, bn, opt, x[rep], DrawNoise(spec.seed, 0, rows + BASE, 3), y=[y[rep] for y in ys], library=lib[rep], mask=mask[rep])
  _check_step(e, e.train_step(rows), res, spec, bn, opt)
  e.close()
  # world 2 (loopback) == world 1 on the concatenated minibatch's reference
  spec, cfg, x, ys, lib, mask = _problem(dict(CASES["vae_zinb_d10"]), n=400)
  params = _params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  world, B, steps = 2, 32, 2
  rows = [rng.permutation(x.shape[0])[: B * world].astype(np.int32).reshape(world, B) for _ in range(steps)]
  engines = [_engine(Engine, cfg, params, x, ys, lib, mask, max_batch=64) for _ in range(world)]
  Engine.comm_init_local(engines)
  refs = [so.dp_train_step(spec, params, bn, opt, x, list(rows[s]), s, cell_base=BASE, y=ys, library=lib, mask=mask) for s in range(steps)]
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


@pytest.mark.parametrize("name", ["vae_zinb_d10", "scvi_zinbd_d7"])
def test_predict_samples_and_scoring(Engine, name):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = _params(spec)
  bn = so.init_bn_state(spec)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  B, S = 40, 4
  xb, lb = x[:B], lib[:B]
  cells = np.arange(B)
  libarg = lb if spec.model == "scvi" else None
  o = e.predict(xb, library=libarg, n_samples=S, batch=B)
  r0 = so.forward_backward(spec, params, bn, xb, so.PhiloxNoise(spec.seed, 0, cells, sample=0), library=lb, training=False, backward=False)
  assert o["scale_tril"].shape == (B, spec.latent_dim, spec.latent_dim)
  assert np.allclose(o["z_mean"], r0["z_mean"], rtol=1e-4, atol=1e-5)
  assert np.allclose(o["scale_tril"], r0["scale_tril"], rtol=1e-4, atol=1e-5)
  assert np.all(np.triu(o["scale_tril"], 1) == 0)
  assert np.allclose(o["z_scale"], np.sqrt((o["scale_tril"].astype(np.float64) ** 2).sum(-1)), rtol=1e-5)
  # every draw is mu + L eps for the device's eps (Philox sample s)
  for s in range(S):
    eps = so.PhiloxNoise(spec.seed, 0, cells, sample=s).normal(so.STREAM_EPS_Z, spec.latent_dim)
    want = o["z_mean"].astype(np.float64) + np.einsum("bij,bj->bi", o["scale_tril"].astype(np.float64), eps)
    assert np.allclose(o["z_sample"][s], want, rtol=1e-4, atol=1e-5), s
  f = e.forward(x=xb, library=libarg)
  assert np.allclose(f["scale_tril"], o["scale_tril"], rtol=1e-6, atol=1e-7) and np.allclose(f["z_mean"], o["z_mean"], rtol=1e-6, atol=1e-7)
  # marginal log-likelihood and posterior llk against the reference's importance-weighted estimates on the same draws
  mllk, llk = e.marginal_llk(x=xb, library=libarg, n_samples=6)
  ref_m, ref_l = so.marginal_log_prob(spec, params, bn, xb, cells, 6, library=lb)
  assert np.allclose(mllk, ref_m, rtol=1e-4, atol=1e-2), np.abs(mllk - ref_m).max()
  assert np.allclose(llk, ref_l, rtol=1e-4, atol=1e-2)
  got = e.score_llk([None], x=xb, library=libarg, n_samples=5)
  want = so.posterior_llk(spec, params, bn, xb, cells, [None], 5, library=lb)
  assert np.allclose(got, want, rtol=1e-4, atol=1e-2), np.abs(got - want).max()
  e.close()


@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


def test_model_api(api, tmp_path):
  """fit -> save_weights -> load_model gives the same encode() bit for bit; a joint marginal log p(x, y) against the reference; fit on a CSR
  store equals fit on the f32 store."""
  from sisua_amd import distributions as D
  from sisua_amd.data import SingleCellOMIC
  n = 400
  sco = SingleCellOMIC(synth_counts(n, 110, sparsity=0.9, seed=11, max_count=500), name="toy")
  P = 6
  sco.add_omic("proteomic", synth_labels(n, ((P, "nb"),))[0])
  train, test = sco.split(0.8)
  X = test.numpy()[:48]
  kw = dict(outputs=sco.get_rv("transcriptomic", "zinb"), latents=api.RVmeta(5, "mvntril", True, "Latents"),
            encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  m1 = api.VAE(**kw)
  m1.fit(train, epochs=3, batch_size=64, verbose=False)
  assert np.isfinite(m1.train_history["loss"]).all()
  q1 = m1.encode(X)
  assert isinstance(q1, D.MultivariateNormalTriL) and q1.batch_shape == (48,) and q1.event_shape == (5,)
  path = os.path.join(tmp_path, "model")
  m1.save_weights(path)
  m2 = api.load_model(path)
  assert type(m2) is api.VAE and m2._make_config().latent_tril
  q2 = m2.encode(X)
  assert np.array_equal(q1.mean(), q2.mean()) and np.array_equal(q1.scale_tril, q2.scale_tril)
  # the joint marginal log p(x, y) of a second output
  vae = api.VAE(outputs=[sco.get_rv("transcriptomic", "zinb"), api.RVmeta(P, "nb", name="proteomic")],
                latents=api.RVmeta(4, "tril"), encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True))
  vae.fit(sco, epochs=2, batch_size=64, verbose=False)
  Y = sco.numpy("proteomic")[:40]
  mllk, llk = vae.marginal_log_prob(inputs=[sco.numpy()[:40], Y], sample_shape=6, batch_size=64)
  spec = ref.Spec(**vae._make_config().to_dict())
  e = vae._engine
  params = {k: v.astype(np.float64) for k, v in e.get_params().items()}
  names = [p for p, _ in so.bn_manifest(spec)]
  bn = {}
  for i, st in e.get_bn().items():
    bn[f"{names[i]}/moving_mean"], bn[f"{names[i]}/moving_var"] = st["moving_mean"].astype(np.float64), st["moving_var"].astype(np.float64)
  ref_m, ref_l = so.marginal_log_prob(spec, params, bn, sco.numpy()[:40], np.arange(40), 6, y=[Y])
  assert np.allclose(mllk, ref_m, rtol=1e-4, atol=1e-2), np.abs(mllk - ref_m).max()
  assert np.allclose(llk["transcriptomic"], ref_l, rtol=1e-4, atol=1e-2)
  # CSR store == f32 store (no input dropout)
  runs = []
  for storage in ("f32", "csr"):
    m = api.SCVI(sco.get_rv("transcriptomic", "zinbd"), latents=api.RVmeta(6, "mvntril"), encoder=api.NetConf([32], batchnorm=True, dropout=0.1),
                 decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
    m.fit(train, epochs=2, batch_size=64, verbose=False, storage=storage)
    q = m.encode(X)
    q = q[0] if isinstance(q, (list, tuple)) else q   # (SCVI: [q(z), q(l)])
    assert isinstance(q, D.MultivariateNormalTriL)
    runs.append((np.asarray(m.train_history["loss"]), m._engine.get_params(), q.scale_tril))
  assert np.array_equal(runs[0][0], runs[1][0])
  for k in runs[0][1]:
    assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
  assert np.array_equal(runs[0][2], runs[1][2])
