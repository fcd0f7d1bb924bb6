"""Float64 full-covariance latent posterior (RVmeta(D, 'mvntril')) for the oracle, without touching oracle/.

oracle.sisua_oracle's init_params, train_step, dp_train_step, marginal_log_prob and posterior_llk look up `manifest`,
`forward_backward` and `marginal_log_prob` as module globals when they run.  `install(monkeypatch)` puts wrappers in place for one
test: a `Spec` below (the oracle's Spec with latent_tril = True) takes the tril path, every other spec the oracle's own functions.
Only what the tril latent changes is restated; the MLPs, count and label likelihoods and Adam are the oracle's.

  head      lat [B, (1 + D) D]: plane 0 mu; plane 1 + i = row i of the raw factor (columns j > i inert)
  factor    L_ij = raw_ij (j < i),  L_ii = softplus(raw_ii) + 1e-5      ([3P-recall] TFP FillScaleTriL, oracle.TRIL_DIAG_SHIFT)
  draw      z = mu + L eps,  eps the diagonal path's D normals (stream STREAM_EPS_Z)
  KL        1/2 (|L|_F^2 + |mu|^2 - D) - sum_i log L_ii     (analytic, against N(0, I))
  backward  d mu = dz + k mu;  d raw_ij = dz_i eps_j + k L_ij (j < i);  d raw_ii = (dz_i eps_i + k (L_ii - 1 / L_ii)) sigmoid(raw_ii)
  scoring   log N(z; 0, I) - log q(z | x) = -|z|^2 / 2 + |eps|^2 / 2 + sum_i log L_ii
"""
from dataclasses import dataclass

import numpy as np
from scipy.special import expit

from oracle import sisua_oracle as so

MAX_DIM = 32
_manifest = so.manifest
_forward_backward = so.forward_backward
_marginal_log_prob = so.marginal_log_prob


@dataclass(frozen=True)
class Spec(so.Spec):
  latent_tril: bool = True

  def __post_init__(self):
    super().__post_init__()
    assert self.model in ("vae", "sisua", "scvi") and 1 <= self.latent_dim <= MAX_DIM, (self.model, self.latent_dim)


def is_tril(spec):
  return bool(getattr(spec, "latent_tril", False))


def factor(lat, D):
  """mu [B, D], L [B, D, D] (lower-triangular), the raw factor [B, D, D] from the head's output lat [B, (1 + D) D]."""
  lat = np.asarray(lat, np.float64)
  mu, raw = lat[:, :D], lat[:, D:].reshape(-1, D, D)
  L = np.tril(raw, -1)
  idx = np.arange(D)
  L[:, idx, idx] = np.logaddexp(0.0, raw[:, idx, idx]) + so.TRIL_DIAG_SHIFT
  return mu, L, raw


def latent_fwd(lat, eps, D):
  """z [B, D], KL [B] and the backward's cache."""
  mu, L, raw = factor(lat, D)
  eps = np.asarray(eps, np.float64)
  z = mu + np.einsum("bij,bj->bi", L, eps)
  dg = np.einsum("bii->bi", L)
  kl = 0.5 * ((L * L).sum((1, 2)) + (mu * mu).sum(1) - D) - np.log(dg).sum(1)
  return z, kl, dict(mu=mu, L=L, raw=raw, eps=eps, D=D)


def latent_bwd(cache, dz, k):
  """d lat [B, (1 + D) D] from d loss / d z and the KL's weight k (beta / B)."""
  mu, L, raw, eps, D = cache["mu"], cache["L"], cache["raw"], cache["eps"], cache["D"]
  dz = np.asarray(dz, np.float64)
  draw = np.tril(dz[:, :, None] * eps[:, None, :] + k * L, -1)
  idx = np.arange(D)
  dg = L[:, idx, idx]
  draw[:, idx, idx] = (dz * eps + k * (dg - 1.0 / dg)) * expit(raw[:, idx, idx])
  return np.concatenate([dz + k * mu, draw.reshape(-1, D * D)], axis=1)


def manifest(spec):
  out = _manifest(spec)
  if not is_tril(spec):
    return out
  nl = (1 + spec.latent_dim) * spec.latent_dim
  return [(n, (s[0], nl) if n == "lat/W" else (nl,) if n == "lat/b" else s) for n, s in out]


def forward_backward(spec, params, bn_state, x, noise, y=(), library=None, mask=None, training=True, backward=True):
  """oracle.forward_backward for a tril spec (models 'vae', 'sisua', 'scvi'): the same step with the latent above."""
  if not is_tril(spec):
    return _forward_backward(spec, params, bn_state, x, noise, y=y, library=library, mask=mask, training=training, backward=backward)
  x = np.asarray(x, dtype=np.float64)
  B, G = x.shape
  D = spec.latent_dim
  new_bn, out = {}, {}
  h0 = np.log1p(x) if spec.log_norm else x
  in_mask = noise.dropout(so.STREAM_INPUT_DROPOUT, G, spec.input_dropout) if training else 1.0
  h0 = h0 * in_mask
  h, enc_c = so._mlp_fwd(spec, params, bn_state, "enc", spec.enc_units, h0, training, noise, so.STREAM_ENC_DROPOUT, spec.dropout_enc, new_bn)
  lat = h @ params["lat/W"] + params["lat/b"]
  z, kl, lc = latent_fwd(lat, noise.normal(so.STREAM_EPS_Z, D), D)
  out.update(z_mean=lc["mu"], scale_tril=lc["L"], z_scale=np.sqrt((lc["L"] ** 2).sum(-1)), z=z, eps=lc["eps"])
  kl_l = np.zeros(B)
  if spec.model == "scvi":
    hl, encl_c = so._mlp_fwd(spec, params, bn_state, "encl", spec.encl_units, h0, training, noise, so.STREAM_ENCL_DROPOUT, spec.dropout_enc, new_bn)
    latl = hl @ params["latl/W"] + params["latl/b"]
    mu_l, sig_l = latl[:, 0], so.softplus1(latl[:, 1])
    eps_l = noise.normal(so.STREAM_EPS_L, 1)[:, 0]
    l = mu_l + sig_l * eps_l
    library = np.asarray(library, dtype=np.float64)
    mp, sp = library[:, 0], np.sqrt(library[:, 1])
    kl_l = np.log(sp / sig_l) + (sig_l ** 2 + (mu_l - mp) ** 2) / (2 * sp ** 2) - 0.5
    out.update(l_mean=mu_l, l_scale=sig_l, l=l)
  d, dec_c = so._mlp_fwd(spec, params, bn_state, "dec", spec.dec_units, z, training, noise, so.STREAM_DEC_DROPOUT, spec.dropout_dec, new_bn)
  k = spec.k
  if spec.model == "scvi":
    raw = [(d @ params[f"out{c}/W"] if spec.head_plane(c) else 0.0) + np.broadcast_to(params[f"out{c}/b"], (B, G)) for c in range(k)]
    e = np.exp(raw[0] - raw[0].max(1, keepdims=True))
    rho_raw = e / e.sum(1, keepdims=True)
    rho = np.clip(rho_raw, so.SCVI_RHO_MIN, 1.0 - so.SCVI_RHO_MIN)
    lhat = np.clip(l, 0.0, spec.clip_library)
    rate = np.exp(lhat)[:, None] * rho
    theta = np.exp(raw[1])
    planes = [rate, theta] + ([raw[2]] if k == 3 else [])
    llk_e, dplanes = so.count_llk(x, planes, spec.likelihood, direct=True)
  else:
    raw_all = d @ params["out/W"] + params["out/b"]
    planes = [raw_all[:, c * G:(c + 1) * G] for c in range(k)]
    llk_e, dplanes = so.count_llk(x, planes, spec.likelihood)
  llk_x = llk_e.sum(1)
  out["x_params"] = planes
  llk_y, llk_o = np.zeros(B), np.zeros(B)
  lab_raw, lab_d = [], []
  mvec = np.zeros(B) if mask is None else np.asarray(mask, dtype=np.float64).reshape(B)
  for j, (P, kind, observed) in enumerate(spec.heads):
    rawy = d @ params[f"lab{j}/W"] + params[f"lab{j}/b"]
    ly, dly = so.label_llk(np.asarray(y[j], dtype=np.float64), rawy, kind)
    if observed:
      llk_o = llk_o + ly
    else:
      llk_y = llk_y + ly
    lab_raw.append(rawy)
    lab_d.append(dly)
  out["y_params"] = lab_raw
  elbo = llk_x + llk_o + spec.alpha * mvec * llk_y - spec.beta * (kl + kl_l)
  loss = float(-elbo.mean())
  metrics = dict(loss=loss, nllk_x=float(-llk_x.mean()), nllk_y=float(-(mvec * llk_y).mean()), kl=float(kl.mean()),
                 kl_l=float(kl_l.mean()), nllk_o=float(-llk_o.mean()))
  out.update(loss=loss, elbo=elbo, llk_x=llk_x, llk_y=llk_y, llk_o=llk_o, kl=kl, kl_l=kl_l, metrics=metrics, new_bn=new_bn)
  if not backward:
    return out
  grads = {}
  c_x, c_kl = -1.0 / B, spec.beta / B
  dd = np.zeros_like(d)
  for j, (P, kind, observed) in enumerate(spec.heads):
    dr = lab_d[j] * (c_x if observed else (c_x * spec.alpha * mvec)[:, None])
    grads[f"lab{j}/W"] = d.T @ dr
    grads[f"lab{j}/b"] = dr.sum(0)
    dd += dr @ params[f"lab{j}/W"].T
  if spec.model == "scvi":
    drate, dtheta = dplanes[0] * c_x, dplanes[1] * c_x
    inside = (rho_raw > so.SCVI_RHO_MIN) & (rho_raw < 1.0 - so.SCVI_RHO_MIN)
    drho = drate * np.exp(lhat)[:, None] * inside
    draw0 = rho_raw * (drho - (drho * rho_raw).sum(1, keepdims=True))
    dl = (drate * rate).sum(1) * ((l > 0.0) & (l < spec.clip_library))
    draws = [draw0, dtheta * theta] + ([dplanes[2] * c_x] if k == 3 else [])
    for c in range(k):
      grads[f"out{c}/b"] = draws[c].sum(keepdims=True).reshape(1) if spec.plane_single(c) else draws[c].sum(0)
      if spec.head_plane(c):
        grads[f"out{c}/W"] = d.T @ draws[c]
        dd += draws[c] @ params[f"out{c}/W"].T
  else:
    draw_all = np.concatenate(dplanes, axis=1) * c_x
    grads["out/W"] = d.T @ draw_all
    grads["out/b"] = draw_all.sum(0)
    dd += draw_all @ params["out/W"].T
  dz = so._mlp_bwd(spec, params, "dec", spec.dec_units, dec_c, dd, grads, training)
  dlat = latent_bwd(lc, dz, c_kl)
  grads["lat/W"] = h.T @ dlat
  grads["lat/b"] = dlat.sum(0)
  dh0 = so._mlp_bwd(spec, params, "enc", spec.enc_units, enc_c, dlat @ params["lat/W"].T, grads, training)
  if spec.model == "scvi":
    dmu_l = dl + c_kl * (mu_l - mp) / sp ** 2
    dsig_l = dl * eps_l + c_kl * (sig_l / sp ** 2 - 1.0 / sig_l)
    dlatl = np.stack([dmu_l, dsig_l * expit(latl[:, 1] + so.SOFTPLUS_INV_1)], axis=1)
    grads["latl/W"] = hl.T @ dlatl
    grads["latl/b"] = dlatl.sum(0)
    dh0 = dh0 + so._mlp_bwd(spec, params, "encl", spec.encl_units, encl_c, dlatl @ params["latl/W"].T, grads, training)
  out["grads"] = grads
  out["d_h0"] = dh0 * in_mask
  return out


def draw_log_weight(r):
  """log N(z; 0, I) - log q(z | x) of one draw of a tril forward (its z, eps and factor)."""
  z, eps, L = r["z"], r["eps"], r["scale_tril"]
  return (-0.5 * z ** 2 + 0.5 * eps ** 2).sum(1) + np.log(np.einsum("bii->bi", L)).sum(1)


def marginal_log_prob(spec, params, bn_state, x, cell_ids, n_samples, library=None, y=()):
  """oracle.marginal_log_prob for a tril spec: the same importance-weighted estimate with the tril draw's latent term."""
  if not is_tril(spec):
    return _marginal_log_prob(spec, params, bn_state, x, cell_ids, n_samples, library=library, y=y)
  logw, llks = [], []
  for s_ in range(n_samples):
    r = forward_backward(spec, params, bn_state, x, so.PhiloxNoise(spec.seed, 0, cell_ids, sample=s_), y=y, library=library,
                         training=False, backward=False)
    lw = r["llk_x"] + r["llk_o"] + draw_log_weight(r)
    if spec.model == "scvi":
      lib = np.asarray(library, dtype=np.float64)
      mp, sp = lib[:, 0], np.sqrt(lib[:, 1])
      eps_l = (r["l"] - r["l_mean"]) / r["l_scale"]
      lw += -0.5 * ((r["l"] - mp) / sp) ** 2 - np.log(sp) + 0.5 * eps_l ** 2 + np.log(r["l_scale"])
    logw.append(lw)
    llks.append(r["llk_x"])
  logw = np.stack(logw, 0)
  mx = logw.max(0)
  return mx + np.log(np.exp(logw - mx).sum(0)) - np.log(n_samples), np.mean(llks, 0)


def install(monkeypatch):
  """Teach the oracle module the tril latent for the duration of one test."""
  monkeypatch.setattr(so, "manifest", manifest)
  monkeypatch.setattr(so, "forward_backward", forward_backward)
  monkeypatch.setattr(so, "marginal_log_prob", marginal_log_prob)


def make_pair(**kw):
  """(reference Spec, ModelConfig) of one tril configuration."""
  from sisua_amd.config import ModelConfig
  return Spec(**kw), ModelConfig(latent_tril=True, **kw)
