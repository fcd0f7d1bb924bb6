"""The 'bernoulli' and 'normal' heads without a GPU: name mapping, plane counts, refusals, the result objects against
scipy.stats, and the float64 reference of tests/head_kinds_ref.py against torch autograd and finite differences."""
import warnings

import numpy as np
import pytest
import torch
from scipy import stats

from oracle import sisua_oracle as so
from tests import head_kinds_ref as ref


def _kw(M):
  return dict(latents=M.RVmeta(6, "diag", True, "Latents"), encoder=M.NetConf([16]), decoder=M.NetConf([16]))


@pytest.fixture(scope="module")
def M():
  import sisua_amd.models as M
  return M


# ---- names, planes, refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("bernoulli", "bernoulli"), ("normal", "normal"), ("gaussian", "normal"), ("diag", "normal"),
                                       ("Bernoulli", "bernoulli"), ("DIAG", "normal")])
def test_head_kind_names(M, name, kind):
  from sisua_amd import _hip
  from sisua_amd.config import ModelConfig, label_planes, manifest
  from sisua_amd.engine import make_smx_config
  assert M._head_kind(M.RVmeta(7, name), "label") == (7, kind)
  assert label_planes(kind) == (1 if kind == "bernoulli" else 2)
  assert _hip.LABEL_LIKELIHOODS[kind] == (9 if kind == "bernoulli" else 10)
  m = M.SISUA(outputs=M.RVmeta(30, "zinb"), labels=[M.RVmeta(7, name), M.RVmeta(4, "onehot")], **_kw(M))
  cfg = m._make_config()
  assert cfg.labels == ((7, kind), (4, "onehot"))
  shapes = dict(manifest(cfg))
  assert shapes["lab0/W"] == (16, label_planes(kind) * 7) and shapes["lab0/b"] == (label_planes(kind) * 7,)
  c = make_smx_config(cfg, 64)
  assert c.n_labels == 2 and list(c.label_llk)[:2] == [_hip.LABEL_LIKELIHOODS[kind], 1] and c.label_components[0] == 1
  assert c.label_observed[0] == 0
  # as an observed second output of the other classes
  for cls, post in ((M.VAE, "zinb"), (M.SCVI, "zinbd")):
    v = cls(outputs=[M.RVmeta(30, post), M.RVmeta(5, name)], **_kw(M))
    assert v._make_config().extra_outputs == ((5, kind),)
  sc = M.SCALAR(outputs=M.RVmeta(30, "zinb"), labels=M.RVmeta(5, name), encoder=M.NetConf([16]), decoder=M.NetConf([16]))
  assert sc._make_config().labels == ((5, kind),)


def test_refusals_and_error_text(M):
  from sisua_amd.config import ModelConfig
  with pytest.raises(ValueError) as ei:
    M.VAE(outputs=[M.RVmeta(30, "zinb"), M.RVmeta(5, "poisson")], **_kw(M))
  msg = str(ei.value)
  assert "'poisson' is not built" in msg and "'bernoulli'" in msg and "'normal' / 'gaussian' / 'diag'" in msg
  with pytest.raises(ValueError):
    M.SemiFVAE(outputs=M.RVmeta(30, "zinb"), labels=M.RVmeta(4, "bernoulli"), **_kw(M))
  with pytest.raises(ValueError):
    M.SemiFVAE(outputs=M.RVmeta(30, "zinb"), labels=M.RVmeta(4, "normal"), **_kw(M))
  with pytest.raises(ValueError, match="unknown head kind"):
    ModelConfig(n_genes=30, labels=((4, "poisson"),))
  with pytest.raises(ValueError, match="unknown head kind"):
    ModelConfig(n_genes=30, extra_outputs=((4, "mixnb7"),))


@pytest.mark.parametrize("name,converted", [("bernoulli", "mixnb2"), ("normal", "mixgauss2"), ("diag", "mixgauss2"), ("gaussian", "mixgauss2")])
def test_misa_still_converts(M, name, converted):
  with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    m = M.MISA(outputs=M.RVmeta(30, "zinb"), labels=M.RVmeta(5, name), **_kw(M))
  assert any("MISA only support labels is a mixture distribution" in str(x.message) for x in w)
  assert m._make_config().labels == ((5, converted),)


@pytest.mark.parametrize("post,kind", [("bernoulli", "bernoulli"), ("diag", "normal"), ("normal", "normal")])
def test_experiment_config_builds_the_new_heads(post, kind):
  """The Experiment driver: `variables.proteomic.posterior: bernoulli` / `diag` builds a SISUA with that label head."""
  from sisua_amd.data import SingleCellOMIC
  from sisua_amd.train import Experiment
  from tests.util import synth_counts
  ex = Experiment({"model": {"name": "sisua"}, "variables": {"proteomic": {"posterior": post, "kwargs": {}}}})
  ex.sco = SingleCellOMIC(synth_counts(50, 30, seed=2), name="toy").add_omic("proteomic", np.zeros((50, 6), np.float32))
  ex.on_create_model()
  assert ex.model._make_config().labels == ((6, kind),) and ex.omics == ["transcriptomic", "proteomic"]


# ---- result objects ------------------------------------------------------------------------------------------------------
def test_bernoulli_result_object():
  from sisua_amd import distributions as D
  rng = np.random.default_rng(0)
  logits = rng.normal(0.0, 2.0, size=(40, 6)).astype(np.float32)
  logits[0, :3] = [30.0, -30.0, 80.0]
  d = D.Bernoulli(logits, name="markers")
  p = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
  assert np.allclose(d.probs, p, rtol=1e-12) and np.allclose(d.mean(), p, rtol=1e-12)
  q = 1.0 / (1.0 + np.exp(logits.astype(np.float64)))   # 1 - p without the subtraction: p (1 - p) in float64 is 1e-3 off at l = 30 and 0 at 80
  assert np.allclose(d.variance(), p * q, rtol=1e-10, atol=1e-300) and np.allclose(d.stddev(), np.sqrt(p * q))
  y = (rng.uniform(size=logits.shape) < 0.5).astype(np.float32)
  lp = d.log_prob(y)
  want = stats.bernoulli.logpmf(y, p)
  ok = np.abs(logits) < 15   # (scipy takes p, whose 1 - p loses its digits at saturation)
  assert np.allclose(lp[ok], want[ok], rtol=1e-9, atol=1e-12)
  sat = -np.abs(logits[0, :3]).astype(np.float64)   # saturated: log p(y) = -|l| on the unlikely side, ~0 on the likely one
  assert np.isfinite(lp).all() and np.allclose(lp[0, :3], np.where((y[0, :3] > 0) == (logits[0, :3] > 0), -np.log1p(np.exp(sat)), sat), rtol=1e-12)
  yf = rng.uniform(size=logits.shape)   # probabilities: TFP's form y log p + (1 - y) log(1 - p)
  l64 = logits.astype(np.float64)
  closed = yf * -np.logaddexp(0.0, -l64) + (1 - yf) * -np.logaddexp(0.0, l64)
  assert np.allclose(d.log_prob(yf), closed, rtol=1e-10, atol=1e-10)
  ind = D.Independent(d, 1, name="markers")
  assert ind.batch_shape == (40,) and ind.event_shape == (6,)
  assert np.allclose(ind.log_prob(y), lp.sum(-1))
  s = d.sample(4000, seed=1)
  assert s.shape == (4000, 40, 6) and s.dtype == np.float32 and set(np.unique(s)) <= {0.0, 1.0}
  assert np.abs(s.mean(0) - p).max() < 0.04 and np.abs(s.var(0) - p * (1 - p)).max() < 0.03
  assert d.sample((2, 3), seed=2).shape == (2, 3, 40, 6) and d.sample(seed=3).shape == (40, 6)
  cat = D.concat_distributions([ind, D.Independent(D.Bernoulli(logits[:5]), 1)], axis=0)
  assert isinstance(cat.distribution, D.Bernoulli) and cat.batch_shape == (45,)


def test_normal_result_objects():
  from sisua_amd import distributions as D
  rng = np.random.default_rng(1)
  loc, scale = rng.normal(size=(30, 5)), np.exp(rng.normal(-0.5, 0.7, size=(30, 5)))
  y = rng.normal(size=(30, 5)) * 2
  want = stats.norm.logpdf(y, loc, scale)
  n = D.Independent(D.Normal(loc, scale), 1)
  mvn = D.MultivariateNormalDiag(loc, scale)
  assert np.allclose(n.log_prob(y), want.sum(-1), rtol=1e-12) and np.allclose(mvn.log_prob(y), want.sum(-1), rtol=1e-12)
  for d in (n, mvn):
    assert d.batch_shape == (30,) and d.event_shape == (5,)
    s = d.sample(6000, seed=4)
    assert s.shape == (6000, 30, 5)
    assert np.abs((s.mean(0) - loc) / scale).max() < 0.08 and np.abs(s.std(0) / scale - 1).max() < 0.08
    assert d.sample((2, 2), seed=5).shape == (2, 2, 30, 5)


# ---- the float64 reference -----------------------------------------------------------------------------------------------
def _torch_llk(kind, y, raw):
  t = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
  yt = torch.tensor(y, dtype=torch.float64)
  zero = torch.zeros((), dtype=torch.float64)   # (torch's softplus turns linear above 20: logaddexp is the exact form)
  if kind == "bernoulli":
    ell = yt * t - torch.logaddexp(t, zero)
  else:
    P = raw.shape[1] // 2
    sg = torch.logaddexp(t[:, P:] + so.SOFTPLUS_INV_1, zero)
    ell = torch.distributions.Normal(t[:, :P], sg).log_prob(yt)
  ell.sum(1).sum().backward()
  return ell.sum(1).detach().numpy(), t.grad.numpy()


def _fd(kind, y, raw, h=1e-6):
  g = np.zeros_like(raw)
  for idx in np.ndindex(raw.shape):
    rp, rm = raw.copy(), raw.copy()
    rp[idx] += h
    rm[idx] -= h
    g[idx] = (ref.label_llk(y, rp, kind)[0].sum() - ref.label_llk(y, rm, kind)[0].sum()) / (2 * h)
  return g


@pytest.mark.parametrize("probabilities", [False, True])
def test_bernoulli_reference_against_autograd(probabilities):
  rng = np.random.default_rng(2)
  B, P = 12, 5
  raw = rng.normal(0.0, 3.0, size=(B, P))
  raw[0] = [30.0, -30.0, 80.0, -80.0, 0.0]   # saturated logits
  y = rng.uniform(size=(B, P)) if probabilities else (rng.uniform(size=(B, P)) < 0.5).astype(np.float64)
  y[0] = [1.0, 1.0, 0.0, 1.0, 0.5] if not probabilities else [0.9, 0.1, 0.3, 0.7, 0.5]
  llk, d = ref.label_llk(y, raw, "bernoulli")
  tl, tg = _torch_llk("bernoulli", y, raw)
  assert np.isfinite(llk).all() and np.isfinite(d).all()
  assert np.allclose(llk, tl, rtol=1e-12, atol=1e-12) and np.allclose(d, tg, rtol=1e-12, atol=1e-14)
  assert np.isclose(ref.bernoulli_llk(1.0, 80.0)[0], 0.0, atol=1e-30) and np.isclose(ref.bernoulli_llk(0.0, 80.0)[0], -80.0)
  fine = np.abs(raw) < 20   # (finite differences of the saturated entries are rounding noise on a zero slope)
  assert np.allclose(d[fine], _fd("bernoulli", y, raw)[fine], rtol=1e-5, atol=1e-6)


def test_normal_reference_against_autograd():
  rng = np.random.default_rng(3)
  B, P = 10, 4
  raw = np.concatenate([rng.normal(size=(B, P)), rng.normal(0.0, 1.5, size=(B, P))], axis=1)
  raw[0, P:] = [-6.0, -10.0, 4.0, 20.0]     # small and large scales
  y = rng.normal(size=(B, P)) * 1.5
  llk, d = ref.label_llk(y, raw, "normal")
  tl, tg = _torch_llk("normal", y, raw)
  assert np.allclose(llk, tl, rtol=1e-12) and np.allclose(d, tg, rtol=1e-10, atol=1e-12)
  assert np.isfinite(llk).all() and np.isfinite(d).all()
  # (finite differences on the moderate scales: at sigma ~ 1e-5 the curvature swamps any step that float64 resolves)
  assert np.allclose(d[1:], _fd("normal", y[1:], raw[1:], h=1e-6), rtol=1e-5, atol=1e-6)


def test_normal_is_one_mixgauss_component():
  """A 'normal' head equals the oracle's own 'mixgauss' formula at one component: a zero logit plane in front, same gradients
  on the location and scale planes, a zero gradient on the logit plane."""
  rng = np.random.default_rng(4)
  B, P = 9, 6
  raw = np.concatenate([rng.normal(size=(B, P)), rng.normal(0.0, 1.0, size=(B, P))], axis=1)
  y = rng.normal(size=(B, P))
  llk, d = ref.label_llk(y, raw, "normal")
  mllk, md = ref._label_llk(y, np.concatenate([np.zeros((B, P)), raw], axis=1), "mixgauss1")
  assert np.allclose(llk, mllk, rtol=1e-12) and np.allclose(md[:, :P], 0.0) and np.allclose(md[:, P:], d, rtol=1e-12, atol=1e-14)


def test_reference_delegates_and_installs(monkeypatch):
  rng = np.random.default_rng(5)
  y, raw = rng.poisson(3.0, size=(4, 3)).astype(np.float64), rng.normal(size=(4, 6))
  a, b = ref.label_llk(y, raw, "nb"), so.label_llk(y, raw, "nb")
  assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
  assert ref.label_planes("mixtril2", 5) == so.label_planes("mixtril2", 5) == 14
  ref.install(monkeypatch)
  assert "bernoulli" in so.LABEL_LIKELIHOODS and so.label_planes("normal") == 2
  spec = so.Spec(model="sisua", n_genes=20, likelihood="zinb", enc_units=(8,), dec_units=(8,), latent_dim=3,
                 labels=((4, "bernoulli"), (3, "normal")))
  shapes = dict(so.manifest(spec))
  assert shapes["lab0/W"] == (8, 4) and shapes["lab1/W"] == (8, 6)
  # one float64 oracle step runs and its head gradients match finite differences of the patched loss
  from tests.util import synth_counts
  x = synth_counts(16, 20, seed=1)
  ys = ref.synth_targets(16, spec.labels)
  params = so.init_params(spec)
  noise = so.PhiloxNoise(spec.seed, 0, np.arange(16))
  mask = np.ones(16)
  r = so.forward_backward(spec, params, so.init_bn_state(spec), x, noise, y=ys, mask=mask)
  assert np.isfinite(r["loss"]) and r["metrics"]["nllk_y"] > 0
  for name in ("lab0/b", "lab1/b"):
    h, i = 1e-6, 1
    pp, pm = dict(params), dict(params)
    pp[name], pm[name] = params[name].copy(), params[name].copy()
    pp[name][i] += h
    pm[name][i] -= h
    f = lambda p: so.forward_backward(spec, p, so.init_bn_state(spec), x, so.PhiloxNoise(spec.seed, 0, np.arange(16)), y=ys, mask=mask,
                                      backward=False)["loss"]
    assert np.isclose(r["grads"][name][i], (f(pp) - f(pm)) / (2 * h), rtol=1e-5, atol=1e-7), name
