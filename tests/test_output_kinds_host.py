"""The 'bernoulli' and 'normal' gene outputs without a GPU: the float64 forms of tests/output_kinds_ref.py against torch autograd and
central differences, the model configuration and parameter manifest, the C-ABI enum, the refusals, and the host distributions."""
import os
import re

import numpy as np
import pytest
import scipy.stats as st
import torch

from sisua_amd import _hip
from sisua_amd import distributions as D
from sisua_amd.config import SOFTPLUS_INV_1, ModelConfig, RVmeta, manifest
from tests import output_kinds_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_llk(kind, x, planes):
  x = torch.tensor(x, dtype=torch.float64)
  ps = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in planes]
  if kind == "bernoulli":
    ell = torch.distributions.Bernoulli(logits=ps[0]).log_prob(x)
  else:
    ell = torch.distributions.Normal(ps[0], torch.nn.functional.softplus(ps[1] + SOFTPLUS_INV_1)).log_prob(x)
  ell.sum().backward()
  return ell.detach().numpy(), [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("kind", ["bernoulli", "normal"])
def test_forms_against_autograd(kind):
  rng = np.random.default_rng(0)
  x = ref.synth_x(kind, 12, 40, seed=1).astype(np.float64)
  planes = [rng.normal(0, 2, size=x.shape) for _ in range(1 if kind == "bernoulli" else 2)]
  ell, d = ref.count_llk(x, planes, kind)
  tl, tg = _torch_llk(kind, x, planes)
  assert np.allclose(ell, tl, rtol=1e-12, atol=1e-12)
  for a, b in zip(d, tg):
    assert np.allclose(a, b, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("kind", ["bernoulli", "normal"])
def test_forms_against_central_differences(kind):
  rng = np.random.default_rng(2)
  x = ref.synth_x(kind, 4, 9, seed=3).astype(np.float64)
  planes = [rng.normal(0, 1, size=x.shape) for _ in range(1 if kind == "bernoulli" else 2)]
  _, d = ref.count_llk(x, planes, kind)
  h = 1e-6
  for c in range(len(planes)):
    up = [p.copy() for p in planes]; dn = [p.copy() for p in planes]
    up[c] += h; dn[c] -= h
    fd = (ref.count_llk(x, up, kind)[0] - ref.count_llk(x, dn, kind)[0]) / (2 * h)
    assert np.allclose(d[c], fd, rtol=1e-6, atol=1e-7)


def test_bernoulli_form_saturates():
  ell, d = ref.count_llk(np.array([[1.0, 0.0, 1.0, 0.0]]), [np.array([[80.0, 80.0, -80.0, -80.0]])], "bernoulli")
  assert np.isfinite(ell).all() and np.allclose(ell, [[0.0, -80.0, -80.0, 0.0]], atol=1e-12)
  assert np.allclose(d, [[0.0, -1.0, 1.0, 0.0]], atol=1e-12)


@pytest.mark.parametrize("kind,k", [("bernoulli", 1), ("normal", 2)])
def test_config_planes_and_manifest(kind, k):
  cfg = ModelConfig(model="vae", n_genes=50, likelihood=kind, enc_units=(16,), dec_units=(24,), latent_dim=4)
  assert cfg.k == k
  shapes = dict(manifest(cfg))
  assert shapes["out/W"] == (24, k * 50) and shapes["out/b"] == (k * 50,)


def test_likelihood_enum_matches_the_header():
  hdr = open(os.path.join(ROOT, "include", "sisua_hip.h")).read()
  body = re.search(r"typedef enum \{([^}]*)\} smx_likelihood;", hdr).group(1)
  enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"SMX_LLK_(\w+)\s*=\s*(\d+)", body)}
  assert enum == _hip.LIKELIHOODS
  assert enum["bernoulli"] == 5 and enum["normal"] == 6


@pytest.fixture(scope="module")
def M():
  import sisua_amd.models as M
  return M


def _kw(M, posterior, G=30):
  return dict(outputs=RVmeta(G, posterior, name="x"), latents=RVmeta(4, "diag", True, "Latents"),
              encoder=M.NetConf([16], batchnorm=True), decoder=M.NetConf([16], batchnorm=True))


@pytest.mark.parametrize("cls", ["VAE", "DeepCountAutoencoder", "SISUA", "MISA", "SCALE", "SCALAR", "FVAE", "SemiFVAE"])
@pytest.mark.parametrize("posterior,stored", [("bernoulli", "bernoulli"), ("normal", "normal"), ("gaussian", "normal"), ("diag", "normal")])
def test_models_accept_the_new_outputs(M, cls, posterior, stored):
  kw = _kw(M, posterior)
  if cls in ("SISUA", "MISA", "SCALAR"):
    kw["labels"] = [RVmeta(5, "onehot", name="y")]
  if cls == "SemiFVAE":
    kw["labels"] = [RVmeta(4, "onehot", name="y")]
  m = getattr(M, cls)(**kw)
  assert m._make_config().likelihood == stored
  assert m._outputs[0].posterior == posterior   # (the RVmeta keeps its name: predict picks the class by it)


@pytest.mark.parametrize("posterior", ["bernoulli", "normal", "gaussian", "diag"])
def test_scvi_refuses_the_new_outputs(M, posterior):
  with pytest.raises(ValueError):
    M.SCVI(outputs=RVmeta(30, posterior, name="x"))


def test_poisson_stays_refused(M):
  with pytest.raises(ValueError):
    M.VAE(**_kw(M, "poisson"))


def test_normal_log_norm_bound(M):
  m = M.VAE(**_kw(M, "normal"), log_norm=True)
  x = np.zeros((8, 30), np.float32)
  x[3, 4] = -1.0
  with pytest.raises(ValueError, match="log1p"):
    m.predict(x, verbose=False)
  with pytest.raises(ValueError, match="log1p"):
    from sisua_amd.data import SingleCellOMIC
    m.fit(SingleCellOMIC(x, name="toy"), epochs=1, batch_size=4, verbose=False)
  assert m._engine is None   # (refused before any device work)
  M.VAE(**_kw(M, "normal"), log_norm=False)._check_inputs(x)   # log_norm=False: any real value


@pytest.mark.parametrize("name", ["bernoulli", "normal", "gaussian", "diag"])
def test_count_distribution_against_scipy(name):
  rng = np.random.default_rng(4)
  B, G = 5, 7
  if name == "bernoulli":
    l = rng.normal(0, 2, size=(B, G))
    d = D.count_distribution(name, [l], "x", activated=False)
    x = (rng.uniform(size=(B, G)) < 0.5).astype(np.float64)
    assert isinstance(d, D.Independent) and isinstance(d.distribution, D.Bernoulli)
    p = 1 / (1 + np.exp(-l))
    assert np.allclose(d.log_prob(x), st.bernoulli.logpmf(x, p).sum(1))
    assert np.allclose(d.mean(), p) and np.allclose(d.variance(), p * (1 - p))
    return
  m, s = rng.normal(size=(B, G)), rng.normal(size=(B, G))
  d = D.count_distribution(name, [m, s], "x", activated=False)
  sd = np.logaddexp(0.0, s + SOFTPLUS_INV_1)
  if name == "diag":
    assert isinstance(d, D.MultivariateNormalDiag)
  else:
    assert isinstance(d, D.Independent) and isinstance(d.distribution, D.Normal)
  x = ref.synth_continuous(B, G, seed=5)
  assert np.allclose(d.log_prob(x), st.norm.logpdf(x, m, sd).sum(1))
  assert np.allclose(d.mean(), m) and np.allclose(d.variance(), sd ** 2)
