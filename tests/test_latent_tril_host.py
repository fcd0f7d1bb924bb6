"""RVmeta(D, 'mvntril'): the full-covariance latent posterior on the host -- the model API's tensor list, parsing and refusals, the float64
reference (tests/latent_tril_ref.py) against torch autograd, finite differences and torch's own KL, and MultivariateNormalTriL against
torch.distributions.MultivariateNormal.  CPU only."""
import warnings

import numpy as np
import pytest
import torch

from sisua_amd import distributions as D
from sisua_amd.config import ModelConfig, RVmeta, manifest
from tests import latent_tril_ref as ref

torch.set_default_dtype(torch.float64)


def _shapes(m):
  return dict(manifest(m._make_config()))


def test_vae_lists_the_tril_head():
  from sisua_amd.models import VAE
  m = VAE(RVmeta(50, "zinb"), latents=RVmeta(10, "mvntril"))
  sh = _shapes(m)
  assert sh["lat/W"] == (64, 110) and sh["lat/b"] == (110,)
  assert m._make_config().latent_tril
  assert _shapes(VAE(RVmeta(50, "zinb"), latents=RVmeta(10, "diag")))["lat/W"] == (64, 20)


def test_tril_alias_models_and_refusals():
  from sisua_amd.models import FVAE, MISA, SCVI, SISUA, VAE
  assert _shapes(VAE(RVmeta(30, "nb"), latents=RVmeta(4, "tril")))["lat/W"] == (64, 20)
  assert _shapes(VAE(RVmeta(30, "nb"), latents=RVmeta(4, "MVNTriL")))["lat/W"] == (64, 20)
  s = SISUA([RVmeta(30, "zinb")], labels=[RVmeta(5, "nb")], latents=RVmeta(3, "mvntril"))
  assert s._make_config().latent_tril and s._make_config().model == "sisua"
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    mi = MISA([RVmeta(30, "zinb")], labels=[RVmeta(5, "nb")], latents=RVmeta(3, "mvntril"))
  assert mi._make_config().latent_tril
  sc = SCVI(RVmeta(30, "zinbd"), latents=RVmeta(6, "mvntril"))
  sh = _shapes(sc)
  assert sh["lat/W"][1] == 42 and sh["latl/W"] == (64, 2)   # (z only: the library latent stays a normal)
  assert _shapes(VAE(RVmeta(30, "nb"), latents=RVmeta(32, "mvntril")))["lat/b"] == (33 * 32,)
  with pytest.raises(ValueError, match="32"):
    VAE(RVmeta(30, "nb"), latents=RVmeta(33, "mvntril"))
  with pytest.raises(ValueError):
    FVAE(RVmeta(30, "nb"), latents=RVmeta(4, "mvntril"))
  with pytest.raises(ValueError):
    ModelConfig(model="fvae", n_genes=10, latent_dim=4, latent_tril=True)
  # other latent names keep the diagonal path
  assert not VAE(RVmeta(30, "nb"), latents=RVmeta(4, "normal"))._make_config().latent_tril


def test_scale_and_dca_warnings_unchanged():
  from sisua_amd.models import SCALE, DeepCountAutoencoder
  with pytest.warns(UserWarning, match="SCALE only allow mixture distribution for latents  posterior, but given: mvntril"):
    s = SCALE(RVmeta(30, "zinb"), latents=RVmeta(4, "mvntril"))
  assert not s._make_config().latent_tril
  with pytest.warns(UserWarning, match="DeepCountAutoencoder only support deterministic latents"):
    d = DeepCountAutoencoder(RVmeta(30, "zinb"), latents=RVmeta(4, "mvntril"))
  assert not d._make_config().latent_tril


def test_to_dict_leaves_latent_tril_out_while_false():
  from oracle import sisua_oracle as so
  cfg = ModelConfig(model="vae", n_genes=10, latent_dim=3)
  assert "latent_tril" not in cfg.to_dict()
  so.Spec(**cfg.to_dict())
  t = ModelConfig(model="vae", n_genes=10, latent_dim=3, latent_tril=True)
  assert ref.Spec(**t.to_dict()).latent_tril


def _torch_latent(lat, eps, D):
  mu, raw = lat[:, :D], lat[:, D:].reshape(-1, D, D)
  L = torch.tril(raw, -1) + torch.diag_embed(torch.nn.functional.softplus(torch.diagonal(raw, dim1=1, dim2=2)) + 1e-5)
  z = mu + (L @ eps[:, :, None])[:, :, 0]
  kl = 0.5 * ((L * L).sum((1, 2)) + (mu * mu).sum(1) - D) - torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)
  return z, kl, mu, L


@pytest.mark.parametrize("D", [1, 3, 7, 10, 32])
def test_reference_layer_matches_autograd_and_torch_kl(D):
  rng = np.random.default_rng(D)
  B = 5
  lat = rng.normal(size=(B, (1 + D) * D)) * 0.7
  eps = rng.normal(size=(B, D))
  wz = rng.normal(size=(B, D))
  k = 0.37
  z, kl, cache = ref.latent_fwd(lat, eps, D)
  t = torch.tensor(lat, requires_grad=True)
  tz, tkl, tmu, tL = _torch_latent(t, torch.tensor(eps), D)
  assert np.allclose(z, tz.detach().numpy(), rtol=1e-12, atol=1e-12)
  assert np.allclose(kl, tkl.detach().numpy(), rtol=1e-12, atol=1e-12)
  q = torch.distributions.MultivariateNormal(tmu, scale_tril=tL)
  p = torch.distributions.MultivariateNormal(torch.zeros(D), scale_tril=torch.eye(D))
  assert np.allclose(kl, torch.distributions.kl_divergence(q, p).detach().numpy(), rtol=1e-10, atol=1e-10)
  ((tz * torch.tensor(wz)).sum() + k * tkl.sum()).backward()
  g = ref.latent_bwd(cache, wz, k)
  assert np.allclose(g, t.grad.numpy(), rtol=1e-10, atol=1e-12)
  # the inert entries above the diagonal: zero gradient
  assert np.all(g[:, D:].reshape(B, D, D)[:, np.triu_indices(D, 1)[0], np.triu_indices(D, 1)[1]] == 0)

  def f(a):
    zz, kk, _ = ref.latent_fwd(a, eps, D)
    return (zz * wz).sum() + k * kk.sum()
  h = 1e-6
  for idx in rng.choice(lat.size, size=min(lat.size, 40), replace=False):
    a1, a2 = lat.copy(), lat.copy()
    a1.flat[idx] += h
    a2.flat[idx] -= h
    assert abs((f(a1) - f(a2)) / (2 * h) - g.flat[idx]) < 1e-6, idx


def test_reference_step_with_identity_factor_is_the_oracle_diagonal_step(monkeypatch):
  """A tril model whose factor is sigma I (off-diagonal columns zero, diagonal biases giving sigma) takes the diagonal model's step."""
  from oracle import sisua_oracle as so
  from tests.util import synth_counts
  ref.install(monkeypatch)
  kw = dict(model="vae", n_genes=40, likelihood="zinb", enc_units=(16,), dec_units=(16,), latent_dim=4, dropout_enc=0.0, dropout_dec=0.0)
  spec_t, spec_d = ref.Spec(**kw), so.Spec(**kw)
  pd = so.init_params(spec_d)
  pt = so.init_params(spec_t)
  Dd = 4
  sigma = 0.8
  pt.update({k: v for k, v in pd.items() if not k.startswith("lat/")})
  pt["lat/W"][:] = 0.0
  pt["lat/W"][:, :Dd] = pd["lat/W"][:, :Dd]
  pt["lat/b"][:] = 0.0
  raw_ii = np.log(np.expm1(sigma - so.TRIL_DIAG_SHIFT))
  for i in range(Dd):
    pt["lat/b"][Dd + i * Dd + i] = raw_ii
  pd["lat/W"][:, Dd:] = 0.0
  pd["lat/b"][Dd:] = np.log(np.expm1(sigma)) - so.SOFTPLUS_INV_1
  x = synth_counts(12, 40, seed=2)
  cells = np.arange(12)
  rt = so.forward_backward(spec_t, pt, so.init_bn_state(spec_t), x, so.PhiloxNoise(8, 0, cells))
  rd = so.forward_backward(spec_d, pd, so.init_bn_state(spec_d), x, so.PhiloxNoise(8, 0, cells))
  for key in ("loss", "nllk_x", "kl"):
    assert np.isclose(rt["metrics"][key], rd["metrics"][key], rtol=1e-10), key
  for k in rd["grads"]:
    if k.startswith("lat/"):
      assert np.allclose(rt["grads"][k][..., :Dd], rd["grads"][k][..., :Dd], rtol=1e-9, atol=1e-12), k
    else:
      assert np.allclose(rt["grads"][k], rd["grads"][k], rtol=1e-9, atol=1e-12), k


def test_mvn_tril_matches_torch():
  rng = np.random.default_rng(4)
  B, Dd = 6, 5
  loc = rng.normal(size=(B, Dd))
  L = np.tril(rng.normal(size=(B, Dd, Dd)) * 0.4, -1) + np.eye(Dd) * rng.uniform(0.5, 1.5, size=(B, 1, Dd))
  d = D.MultivariateNormalTriL(loc, L, name="z")
  t = torch.distributions.MultivariateNormal(torch.tensor(loc), scale_tril=torch.tensor(L))
  x = rng.normal(size=(3, B, Dd))
  assert np.allclose(d.log_prob(x), t.log_prob(torch.tensor(x)).numpy(), rtol=1e-10)
  assert np.allclose(d.entropy(), t.entropy().numpy(), rtol=1e-10)
  assert np.allclose(d.covariance(), t.covariance_matrix.numpy(), rtol=1e-10)
  assert np.allclose(d.variance(), t.variance.numpy(), rtol=1e-10)
  assert np.allclose(d.stddev(), t.stddev.numpy(), rtol=1e-10)
  assert np.allclose(d.mean(), loc)
  assert d.batch_shape == (B,) and d.event_shape == (Dd,)
  s = d.sample(20000, seed=1)
  assert s.shape == (20000, B, Dd)
  assert np.abs(np.cov(s[:, 0].T) - d.covariance()[0]).max() < 0.08
  c = D.concat_distributions([d, D.MultivariateNormalTriL(loc[:2], L[:2])])
  assert isinstance(c, D.MultivariateNormalTriL) and c.batch_shape == (B + 2,)
  assert np.allclose(c.log_prob(np.concatenate([x[0], x[0, :2]])), np.concatenate([d.log_prob(x[0]), d.log_prob(x[0])[:2]]))
