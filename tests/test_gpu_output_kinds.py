"""The 'bernoulli' and 'normal' gene outputs on the device against the float64 oracle, taught the two kinds by tests/output_kinds_ref.py:
the element kernels (saturated logits, tiny and huge scales), the one-launch head of wide panels, one step of every model family with
every narrow-panel form, a wide 'normal' panel on the f32 and CSR stores, a trajectory (eager and captured), two draws per cell, a
world-2 loopback step, eval / predict statistics, scoring (both scoring forms bit for bit) and the model API.  Tolerances of
test_gpu_head_kinds.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import sisua_oracle as so
from tests import output_kinds_ref as ref
from tests.util import adam_state_errors, grad_errors, make_pair, perturbed_params

pytestmark = pytest.mark.gpu
RTOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _oracle_knows_the_kinds(monkeypatch):
  ref.install(monkeypatch)


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _cases(kind):
  return {
      f"vae_{kind}": dict(model="vae", n_genes=150, likelihood=kind, enc_units=(48,), dec_units=(48,), latent_dim=8),
      f"dca_{kind}": dict(model="dca", n_genes=130, likelihood=kind, enc_units=(40,), dec_units=(40,), latent_dim=6, latent_activation="relu"),
      f"sisua_{kind}": dict(model="sisua", n_genes=140, likelihood=kind, enc_units=(48,), dec_units=(48,), latent_dim=8,
                            labels=((6, "onehot"),), alpha=10.0),
      f"scale_{kind}": dict(model="scale", n_genes=120, likelihood=kind, enc_units=(48,), dec_units=(48,), latent_dim=8, n_components=5),
      f"fvae_{kind}": dict(model="fvae", n_genes=110, likelihood=kind, enc_units=(40,), dec_units=(40,), latent_dim=6),
  }


CASES = {**_cases("bernoulli"), **_cases("normal")}


def _problem(kw, n=300, seed=0):
  spec, cfg = make_pair(**kw)
  x = ref.synth_x(spec.likelihood, n, spec.n_genes, seed=seed)
  from tests.util import synth_labels
  ys = synth_labels(n, spec.labels, seed=seed + 1) if spec.labels else []
  lib = np.tile(np.array([[1.0, 1.0]], dtype=np.float32), (n, 1))
  mask = so.label_mask(n, 0.4, n_omics=1 + len(spec.labels), seed=1)
  return spec, cfg, x, ys, lib, mask


def _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, step, cell_base=0):
  noise = so.PhiloxNoise(spec.seed, step, rows + cell_base)
  return so.train_step(spec, params, bn, opt, x[rows], noise, y=[y[rows] for y in ys], library=lib[rows], mask=mask[rows])


def _check_step(e, m, res, spec, bn):
  assert m["nan_flag"] == 0
  for key in ["loss", "nllk_x", "kl"] + (["nllk_y"] if spec.labels else []):
    assert np.isfinite(m[key]) and np.isclose(m[key], res["metrics"][key], rtol=RTOL, atol=1e-5), (key, m[key], res["metrics"][key])
  worst = grad_errors(e.get_params(which=1), res["grads"])
  assert max(worst.values()) < RTOL, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  names = [p for p, _ in so.bn_manifest(spec)]
  for i, st in e.get_bn().items():
    assert np.allclose(st["moving_mean"], bn[f"{names[i]}/moving_mean"], rtol=1e-4, atol=1e-6)
    assert np.allclose(st["moving_var"], bn[f"{names[i]}/moving_var"], rtol=1e-4, atol=1e-6)


# ---- element kernels ---------------------------------------------------------------------------------------------------------------
def test_count_llk_kernel_bernoulli_saturated(Engine):
  from sisua_amd.engine import k_count_llk
  rng = np.random.default_rng(0)
  B, G = 16, 333
  x = (rng.uniform(size=(B, G)) < 0.4).astype(np.float32)
  x[0] = rng.uniform(size=G).astype(np.float32)            # probabilities score too
  l = rng.normal(0, 3, size=(1, B, G)).astype(np.float32)
  l[0, 1], l[0, 2], l[0, 3, ::2] = 80.0, -80.0, 80.0      # saturated logits
  llk, grads = k_count_llk("bernoulli", x, l)
  ell, d = ref.count_llk(x, [l[0]], "bernoulli")
  assert np.isfinite(llk).all() and np.isfinite(grads).all()
  assert np.allclose(llk, ell.sum(1), rtol=1e-5, atol=1e-3)
  assert np.allclose(grads[0], d[0], rtol=1e-5, atol=1e-6)


def test_count_llk_kernel_normal_scales(Engine):
  from sisua_amd.engine import k_count_llk
  rng = np.random.default_rng(1)
  B, G = 16, 300
  x = ref.synth_continuous(B, G, seed=2) * 3.0
  m = rng.normal(0, 1, size=(B, G)).astype(np.float32)
  s = rng.normal(0, 1, size=(B, G)).astype(np.float32)
  s[1], s[2] = -12.0, 40.0                                  # tiny (sigma ~ 6e-6) and huge (sigma ~ 40) scales
  x[1] = m[1] + 1e-5 * rng.normal(size=G).astype(np.float32)
  llk, grads = k_count_llk("normal", x, np.stack([m, s]))
  ell, d = ref.count_llk(x, [m, s], "normal")
  assert np.isfinite(llk).all() and np.isfinite(grads).all()
  assert np.allclose(llk, ell.sum(1), rtol=1e-4, atol=1e-2), np.abs(llk - ell.sum(1)).max()
  for c in range(2):
    assert np.allclose(grads[c], d[c], rtol=2e-4, atol=1e-4 * np.abs(d[c]).max()), c


def _hf_problem(G=8192, B=128, seed=3):
  rng = np.random.default_rng(seed)
  x = ref.synth_continuous(B, G, seed=seed)
  d = np.maximum(rng.normal(0, 1, size=(B, 128)), 0).astype(np.float32)
  W = (rng.normal(0, 0.05, size=(128, 2, G))).astype(np.float32)
  bias = np.stack([np.full(G, 0.5), np.full(G, -0.3)]).astype(np.float32)
  return x, d, W, bias


def test_head_fused_normal_against_float64(Engine):
  from sisua_amd.engine import k_head_fused
  x, d, W, bias = _hf_problem()
  r = k_head_fused("normal", x, d, W, bias, grad_scale=-1.0 / 128)
  P = np.einsum("bh,hkg->kbg", d.astype(np.float64), W.astype(np.float64)) + bias[:, None, :]
  ell, dp = ref.count_llk(x, [P[0], P[1]], "normal")
  assert np.isfinite(r["llk"]).all()
  assert np.allclose(r["llk"], ell.sum(1), rtol=1e-3, atol=1.0), np.abs(r["llk"] - ell.sum(1)).max()
  db = np.stack([g.sum(0) for g in dp]) * (-1.0 / 128)
  assert np.allclose(r["db"], db, rtol=5e-3, atol=1e-5 + 5e-3 * np.abs(db).max())
  dW = np.einsum("bh,kbg->hkg", d.astype(np.float64), np.stack(dp)) * (-1.0 / 128)
  assert np.allclose(r["dW"], dW, rtol=5e-3, atol=5e-3 * np.abs(dW).max())


def test_head_fused_normal_stress_is_bitwise_stable(Engine):
  """>= 2 000 launches of the 'normal' head: every one's results equal the first's, bit for bit (one process under its own time limit)."""
  script = ("import numpy as np, sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_output_kinds import _hf_problem\n"
            "from sisua_amd.engine import k_head_fused_stress\n"
            "x, d, W, b = _hf_problem()\n"
            "n, first = k_head_fused_stress('normal', x, d, W, b, launches=2000, grad_scale=-1.0 / 128)\n"
            "print('STRESS', n, first)\n") % ROOT
  p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True)
  assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
  line = [l for l in p.stdout.splitlines() if l.startswith("STRESS")][-1]
  assert line.split()[1:] == ["0", "-1"], line


# ---- one step against the oracle -----------------------------------------------------------------------------------------------------
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
  res = _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, 0, cell_base=1000)
  m = e.train_step(rows)
  _check_step(e, m, res, spec, bn)
  em, ev, where = adam_state_errors(e, opt)
  assert em < 2e-4 and ev < 4e-4, (em, ev, where)
  e.close()


@pytest.mark.parametrize("flag", ["head_loss", "head_bwd", "wgrad"])
@pytest.mark.parametrize("name", ["vae_normal", "sisua_normal", "vae_bernoulli"])
def test_narrow_panel_forms_match_oracle(Engine, name, flag):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=1000)
  e.set_flag(flag, False)
  rows = np.random.default_rng(1).choice(x.shape[0], size=96, replace=False).astype(np.int32)
  res = _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, 0, cell_base=1000)
  _check_step(e, e.train_step(rows), res, spec, bn)
  e.close()


@pytest.mark.parametrize("storage", ["f32", "csr"])
@pytest.mark.parametrize("fused", [True, False])
def test_wide_normal_panel(Engine, storage, fused):
  """A 'normal' output at 128 x 20 000 (the one-launch head when it is on) against the oracle's step."""
  import scipy.sparse as sp
  kw = dict(model="vae", n_genes=20000, likelihood="normal", enc_units=(128,), dec_units=(128,), latent_dim=16)
  spec, cfg = make_pair(**kw)
  n = 160
  x = ref.synth_continuous(n, spec.n_genes, seed=5)
  x[np.random.default_rng(6).uniform(size=x.shape) < 0.7] = 0.0   # mostly zero: the CSR store holds the rest
  lib = np.tile(np.array([[1.0, 1.0]], dtype=np.float32), (n, 1))
  mask = np.zeros((n, 1), np.float32)
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  e.set_flag("head_fused", fused)
  e.upload(sp.csr_matrix(x) if storage == "csr" else x, [], lib, mask, storage=storage)
  assert (e.head_fused_bytes(128) > 0) == fused
  rows = np.arange(10, 138, dtype=np.int32)
  res = _oracle_step(spec, params, bn, opt, x, [], lib, mask, rows, 0)
  m = e.train_step(rows)
  assert m["nan_flag"] == 0
  for key in ("loss", "nllk_x", "kl"):
    assert np.isclose(m[key], res["metrics"][key], rtol=RTOL, atol=1e-4), (key, m[key], res["metrics"][key])
  worst = grad_errors(e.get_params(which=1), res["grads"])
  assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  e.close()


# ---- longer runs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,graph", [("vae_normal", False), ("vae_normal", True), ("sisua_bernoulli", False), ("scale_bernoulli", True)])
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
  assert np.median(ref_l[-5:]) < np.median(ref_l[:5])
  e.close()


@pytest.mark.parametrize("name", ["vae_normal", "vae_bernoulli"])
def test_two_draws_per_cell_match_the_repeated_minibatch(Engine, name):
  """Two draws per cell (fit(sample_shape=2)): the oracle's unchanged step on the minibatch repeated twice, draw-major."""
  from tests.test_train_draws_host import DrawNoise
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=1000)
  e.set_train_draws(2)
  rows = np.random.default_rng(1).choice(x.shape[0], size=64, replace=False).astype(np.int32)
  rep = np.tile(rows, 2)
  res = so.train_step(spec, params, bn, opt, x[rep], DrawNoise(spec.seed, 0, rows + 1000, 2), y=[y[rep] for y in ys],
                      library=lib[rep], mask=mask[rep])
  _check_step(e, e.train_step(rows), res, spec, bn)
  e.close()


def test_world2_loopback_step(Engine):
  """Two replicas over the in-process collective, each drawing its own rows: the oracle's data-parallel step."""
  from tests.test_gpu_dp import run_ranks
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_normal"])
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  engines = []
  for r in range(2):
    e = Engine(cfg, max_batch=64, init=False)
    e.set_params(params)
    e.upload(x, ys, lib, mask, cell_id_base=1000)
    engines.append(e)
  Engine.comm_init_local(engines)
  rows = np.random.default_rng(5).permutation(x.shape[0])[:96].astype(np.int32).reshape(2, 48)
  res = so.dp_train_step(spec, params, bn, opt, x, list(rows), 0, cell_base=1000, y=ys, library=lib, mask=mask, sync_bn=False)
  ms = run_ranks([lambda r=r: engines[r].train_step(rows[r]) for r in range(2)])
  for e, m in zip(engines, ms):
    assert m["nan_flag"] == 0
    for key in ("loss", "nllk_x", "kl"):
      assert np.isclose(m[key], res["metrics"][key], rtol=RTOL, atol=1e-5), (key, m[key], res["metrics"][key])
    worst = grad_errors(e.get_params(which=1), res["grads"])
    assert max(worst.values()) < RTOL, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  finals = [e.get_params() for e in engines]
  for k in finals[0]:
    assert np.array_equal(finals[0][k], finals[1][k]), k
  for e in engines:
    e.close()


# ---- eval, predict, scoring ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae_normal", "vae_bernoulli", "sisua_normal"])
def test_eval_and_forward_match_oracle(Engine, name):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask)
  rows = np.arange(40, 140, dtype=np.int32)
  noise = so.PhiloxNoise(spec.seed, 0, rows, sample=0)
  res = so.forward_backward(spec, params, bn, x[rows], noise, y=[y[rows] for y in ys], library=lib[rows], mask=mask[rows], training=False,
                            backward=False)
  m = e.eval_step(rows)
  assert m["nan_flag"] == 0 and np.isclose(m["loss"], res["loss"], rtol=RTOL)
  out = e.forward(row_ids=rows, sample_index=0)
  for c in range(spec.k):
    assert np.allclose(out["x_params"][c], res["x_params"][c], rtol=1e-3, atol=1e-4), c
  e.close()


@pytest.mark.parametrize("name", ["vae_normal", "vae_bernoulli", "scale_normal"])
def test_marginal_llk_matches_oracle(Engine, name):
  spec, cfg, x, ys, lib, mask = _problem(CASES[name])
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask)
  rows = np.arange(0, 40, dtype=np.int32)
  mllk, llk = e.marginal_llk(row_ids=rows, n_samples=6)
  ref_m, ref_l = so.marginal_log_prob(spec, params, bn, x[rows], rows, 6)
  assert np.isfinite(mllk).all()
  assert np.allclose(mllk, ref_m, rtol=1e-4, atol=1e-2), np.abs(mllk - ref_m).max()
  assert np.allclose(llk, ref_l, rtol=1e-4, atol=1e-2)
  sc = e.score_llk([None], row_ids=rows, n_samples=6)
  ref_s = so.posterior_llk(spec, params, bn, x[rows], rows, [None], 6)
  assert np.allclose(sc, ref_s, rtol=1e-4, atol=1e-2), np.abs(sc - ref_s).max()
  assert np.array_equal(sc[0, 0], sc[0, 1])   # ('imputed' = 'reconstructed': no zero-inflation wrapper)
  e.close()


def test_normal_scoring_forms_bitwise_equal(Engine):
  from sisua_amd import _hip
  spec, cfg, x, ys, lib, mask = _problem(CASES["vae_normal"])
  e = Engine(cfg, max_batch=128)
  e.upload(x, ys, lib, mask)
  rows = np.arange(5, 105, dtype=np.int32)

  def both():
    return e.marginal_llk(row_ids=rows, n_samples=30), e.score_llk([None, x[rows][:, ::-1].copy()], row_ids=rows, n_samples=30)
  walk = both()
  for ranges in (0, 1, 2):
    _hip.set_tuning("score_walk", ranges)
    try:
      got = both()
    finally:
      _hip.clear_tuning("score_walk")
    assert np.array_equal(got[0][0], walk[0][0]) and np.array_equal(got[1], walk[1]), ranges
  assert np.isfinite(walk[0][0]).all()
  e.close()


# ---- the model API -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


@pytest.mark.parametrize("posterior", ["normal", "gaussian", "diag"])
def test_vae_normal_output_fit_predict_save_load(api, tmp_path, posterior):
  from sisua_amd import distributions as D
  from sisua_amd.data import SingleCellOMIC
  G = 90
  x = ref.synth_continuous(500, G, seed=7)
  assert (x < 0).any()
  sco = SingleCellOMIC(x, name="toy")
  kw = dict(outputs=api.RVmeta(G, posterior, name="transcriptomic"), latents=api.RVmeta(8, "diag", True, "Latents"),
            encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  vae = api.VAE(**kw)
  assert vae._make_config().likelihood == "normal" and vae._make_config().k == 2
  vae.fit(sco, epochs=8, batch_size=64, learning_rate=2e-3, verbose=False)
  h = np.asarray(vae.train_history["loss"])
  assert np.isfinite(h).all() and h[-2:].mean() < h[:2].mean(), h
  X = x[:100]
  pX, qZ = vae.predict(X, verbose=False)
  if posterior == "diag":
    assert isinstance(pX, D.MultivariateNormalDiag)
  else:
    assert isinstance(pX, D.Independent) and isinstance(pX.distribution, D.Normal)
  assert pX.batch_shape == (100,) and pX.event_shape == (G,)
  lp = pX.log_prob(X)
  assert lp.shape == (100,) and np.isfinite(lp).all()
  lazy, _ = vae.predict(X, verbose=False, lazy=True)
  assert np.allclose(lazy.mean(), pX.mean(), rtol=1e-5, atol=1e-6)
  assert np.allclose(lazy.variance(), pX.variance(), rtol=1e-4, atol=1e-6)
  assert np.allclose(lazy.log_prob(X), lp, rtol=1e-4, atol=1e-2)
  assert np.array_equal(lazy.materialize().mean(), pX.mean())
  mllk, llk = vae.marginal_log_prob(X[:40], sample_shape=5)
  assert np.isfinite(mllk).all()
  path = os.path.join(tmp_path, "vae_normal")
  vae.save_weights(path)
  m2 = api.load_model(path)
  pX2, _ = m2.predict(X, verbose=False)
  assert type(pX2) is type(pX) and np.array_equal(pX2.mean(), pX.mean()) and np.array_equal(pX2.variance(), pX.variance())


def test_scale_bernoulli_fit_predict_save_load(api, tmp_path):
  from sisua_amd import distributions as D
  from sisua_amd.data import SingleCellOMIC
  G = 100
  x = ref.synth_binary(500, G, seed=8)
  sco = SingleCellOMIC(x, name="atac")
  kw = dict(outputs=api.RVmeta(G, "bernoulli", name="atac"), latents=api.RVmeta(8, "diag", True, "Latents"),
            encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  m = api.SCALE(**kw)
  assert m._make_config().likelihood == "bernoulli" and m._make_config().k == 1
  m.fit(sco, epochs=8, batch_size=64, learning_rate=2e-3, verbose=False)
  h = np.asarray(m.train_history["loss"])
  assert np.isfinite(h).all() and h[-2:].mean() < h[:2].mean(), h
  X = x[:100]
  pX, _ = m.predict(X, verbose=False)
  assert isinstance(pX, D.Independent) and isinstance(pX.distribution, D.Bernoulli)
  mean = pX.mean()
  assert mean.shape == (100, G) and (mean > 0).all() and (mean < 1).all()
  lazy, _ = m.predict(X, verbose=False, lazy=True)
  assert np.allclose(lazy.mean(), mean, rtol=1e-5, atol=1e-6)
  assert np.allclose(lazy.log_prob(X), pX.log_prob(X), rtol=1e-4, atol=1e-2)
  mllk, _ = m.marginal_log_prob(X[:40], sample_shape=5)
  assert np.isfinite(mllk).all() and (mllk < 0).all()
  path = os.path.join(tmp_path, "scale_bernoulli")
  m.save_weights(path)
  m2 = api.load_model(path)
  pX2, _ = m2.predict(X, verbose=False)
  assert np.array_equal(pX2.distribution.logits, pX.distribution.logits)
