"""Result objects of predict / encode / decode.

The reference returns TensorFlow-Probability distributions and its consumers
(sisua/analysis/posterior.py:187-220, 233-249, 927-937; tests/test_save_load_model.py:32-46)
touch only `.mean() .variance() .stddev() .sample(n) .log_prob(x) .batch_shape
.event_shape .name`, `Independent.distribution / .reinterpreted_batch_ndims` and
`ZeroInflated.count_distribution`.  These classes carry the parameter arrays the
GPU forward produced (NumPy, host side) and implement exactly that surface; they
are result containers, not part of the training hot path.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import scipy.sparse as _sp
from scipy.special import expit, gammaln

SOFTPLUS_INV_1 = float(np.log(np.expm1(1.0)))


def _softplus(x):
  return np.logaddexp(0.0, x)


def _log_sigmoid(x):
  return -_softplus(-x)


class Distribution:
  name: str = "Distribution"
  _event_ndims = 0

  def _params(self) -> List[np.ndarray]:
    raise NotImplementedError

  @property
  def batch_shape(self):
    s = np.broadcast_shapes(*[np.shape(p) for p in self._params()])
    return tuple(s[:len(s) - self._event_ndims])

  @property
  def event_shape(self):
    s = np.broadcast_shapes(*[np.shape(p) for p in self._params()])
    return tuple(s[len(s) - self._event_ndims:])

  def mean(self):
    raise NotImplementedError

  def variance(self):
    raise NotImplementedError

  def stddev(self):
    return np.sqrt(self.variance())

  def log_prob(self, x):
    raise NotImplementedError

  def sample(self, sample_shape=(), seed=None):
    raise NotImplementedError

  def _sshape(self, sample_shape):
    if isinstance(sample_shape, (int, np.integer)):
      return (int(sample_shape),)
    return tuple(int(s) for s in sample_shape)

  def __repr__(self):
    return f"<{type(self).__name__} '{self.name}' batch_shape={self.batch_shape} event_shape={self.event_shape}>"


class Normal(Distribution):

  def __init__(self, loc, scale, name="Normal"):
    self.loc, self.scale, self.name = np.asarray(loc), np.asarray(scale), name

  def _params(self):
    return [self.loc, self.scale]

  def mean(self):
    return np.broadcast_to(self.loc, np.broadcast_shapes(self.loc.shape, self.scale.shape)).copy()

  def variance(self):
    return np.broadcast_to(self.scale ** 2, np.broadcast_shapes(self.loc.shape, self.scale.shape)).copy()

  def log_prob(self, x):
    z = (np.asarray(x) - self.loc) / self.scale
    return -0.5 * z * z - np.log(self.scale) - 0.5 * np.log(2 * np.pi)

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    shp = self._sshape(sample_shape) + np.broadcast_shapes(self.loc.shape, self.scale.shape)
    return self.loc + self.scale * rng.standard_normal(shp)


class MultivariateNormalDiag(Normal):
  """Diagonal Gaussian over the last axis (the 'diag' latent posterior)."""
  _event_ndims = 1

  def __init__(self, loc, scale_diag, name="MultivariateNormalDiag"):
    super().__init__(loc, scale_diag, name)

  def log_prob(self, x):
    return super().log_prob(x).sum(-1)


class MultivariateNormalTriL(Distribution):
  """Full-covariance Gaussian over the last axis, N(loc, L L^T) with L lower-triangular (the RVmeta(D, 'mvntril') latent posterior;
  TFP MultivariateNormalTriL semantics).  Parameters: locations [..., D], scale factors [..., D, D] (entries above the diagonal ignored)."""
  _event_ndims = 1

  def __init__(self, loc, scale_tril, name="MultivariateNormalTriL"):
    self.loc = np.asarray(loc)
    self.scale_tril = np.tril(np.asarray(scale_tril))
    self.name = name

  def _params(self):
    return [self.loc, self.scale_tril[..., 0]]

  def mean(self):
    return np.broadcast_to(self.loc, self.batch_shape + self.event_shape).copy()

  def covariance(self):
    L = self.scale_tril.astype(np.float64)
    return L @ np.swapaxes(L, -1, -2)

  def variance(self):
    return (self.scale_tril.astype(np.float64) ** 2).sum(-1)

  def stddev(self):
    return np.sqrt(self.variance())

  def _whiten(self, x):
    """u = L^-1 (x - loc) by forward substitution (D is 32 at most)."""
    d = np.asarray(x, np.float64) - self.loc
    L = np.broadcast_to(self.scale_tril.astype(np.float64), d.shape[:-1] + self.scale_tril.shape[-2:])
    u = np.zeros(d.shape)
    for p in range(d.shape[-1]):
      u[..., p] = (d[..., p] - (L[..., p, :p] * u[..., :p]).sum(-1)) / L[..., p, p]
    return u

  def _log_det(self):
    return np.log(np.einsum("...pp->...p", self.scale_tril.astype(np.float64))).sum(-1)

  def log_prob(self, x):
    u = self._whiten(x)
    return -0.5 * (u * u).sum(-1) - self._log_det() - 0.5 * u.shape[-1] * np.log(2.0 * np.pi)

  def entropy(self):
    D = self.scale_tril.shape[-1]
    return 0.5 * D * (1.0 + np.log(2.0 * np.pi)) + self._log_det()

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    eps = rng.standard_normal(self._sshape(sample_shape) + self.batch_shape + self.event_shape)
    return self.loc + np.einsum("...pq,...q->...p", self.scale_tril, eps)


class Deterministic(Distribution):
  """Point mass (DCA's deterministic latent, dca.py:13-28)."""
  _event_ndims = 1

  def __init__(self, loc, name="Deterministic"):
    self.loc, self.name = np.asarray(loc), name

  def _params(self):
    return [self.loc]

  def mean(self):
    return self.loc.copy()

  def variance(self):
    return np.zeros_like(self.loc)

  def sample(self, sample_shape=(), seed=None):
    return np.broadcast_to(self.loc, self._sshape(sample_shape) + self.loc.shape).copy()

  def log_prob(self, x):
    return np.where(np.all(np.asarray(x) == self.loc, axis=-1), 0.0, -np.inf)


class VectorDeterministic(Deterministic):
  """The output of RVmeta(dim, 'mse') (the reference's tests/test_singlecell_models.py:82-91): a point mass at `loc` over the
  last axis whose log_prob is MINUS THE MEAN SQUARED ERROR -- the identity the reference's test pins exactly,
  `-dist.log_prob(z) == tf.losses.mse(z, y.mean())` = mean over the last axis of the squared difference, evaluated in the
  arguments' own precision (float32 for float32 inputs, as TensorFlow does)."""

  def __init__(self, loc, name="VectorDeterministic"):
    super().__init__(loc, name)

  def log_prob(self, x):
    x = np.asarray(x)
    d = x - self.loc.astype(np.result_type(x, self.loc), copy=False)
    return -np.mean(d * d, axis=-1)


class NegativeBinomial(Distribution):
  """TFP convention: total_count r, logits l; mean = r exp(l)."""

  def __init__(self, total_count=None, logits=None, name="NegativeBinomial", log_total_count=None):
    # the network emits log total_count: exp() of a whole prediction (75 MB for 940 cells x 10 draws) is only taken when
    # somebody asks for total_count / mean / log_prob, not at construction (8 ms of a 26 ms predict call)
    if (total_count is None) == (log_total_count is None):
      raise ValueError("give total_count or log_total_count")
    self._total_count = None if total_count is None else np.asarray(total_count)
    self._log_total_count = None if log_total_count is None else np.asarray(log_total_count)
    self.logits, self.name = np.asarray(logits), name

  @property
  def total_count(self):
    if self._total_count is None:
      self._total_count = np.exp(self._log_total_count)
    return self._total_count

  def _params(self):
    return [self._total_count if self._total_count is not None else self._log_total_count, self.logits]   # (shapes only)

  def mean(self):
    return self.total_count * np.exp(self.logits)

  def variance(self):
    return self.mean() * (1.0 + np.exp(self.logits))

  def log_prob(self, x):
    x, r, l = np.asarray(x, dtype=np.float64), self.total_count.astype(np.float64), self.logits.astype(np.float64)
    return gammaln(x + r) - gammaln(r) - gammaln(x + 1.0) + x * _log_sigmoid(l) + r * _log_sigmoid(-l)

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    shp = self._sshape(sample_shape) + np.broadcast_shapes(self.total_count.shape, self.logits.shape)
    lam = rng.gamma(np.broadcast_to(self.total_count, shp), np.broadcast_to(np.exp(self.logits), shp))
    return rng.poisson(lam).astype(np.float32)


class NegativeBinomialDisp(Distribution):
  """Mean / dispersion form (scVI): var = mean + mean^2 / disp."""

  def __init__(self, loc, disp, name="NegativeBinomialDisp", eps=1e-8):
    self.loc, self.disp, self.name, self.eps = np.asarray(loc), np.asarray(disp), name, eps

  def _params(self):
    return [self.loc, self.disp]

  def mean(self):
    return np.broadcast_to(self.loc, np.broadcast_shapes(self.loc.shape, self.disp.shape)).copy()

  def variance(self):
    # mu (1 + mu / th): mu^2 underflows in float32 where the variance is still a normal number; mu == 0 has variance 0
    with np.errstate(divide="ignore", invalid="ignore"):
      return np.where(self.loc > 0, self.loc * (1.0 + self.loc / self.disp), self.loc * 0.0)

  def log_prob(self, x):
    x, mu, th, e = np.asarray(x, np.float64), self.loc.astype(np.float64), self.disp.astype(np.float64), self.eps
    lt = np.log(th + mu + e)
    return (th * (np.log(th + e) - lt) + x * (np.log(mu + e) - lt) + gammaln(x + th) - gammaln(th) - gammaln(x + 1.0))

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    shp = self._sshape(sample_shape) + np.broadcast_shapes(self.loc.shape, self.disp.shape)
    lam = rng.gamma(np.broadcast_to(self.disp, shp), np.broadcast_to(self.loc / self.disp, shp))
    return rng.poisson(lam).astype(np.float32)


class ZeroInflated(Distribution):
  """pi = sigmoid(logits) mass at zero mixed with `count_distribution`."""

  def __init__(self, count_distribution: Distribution, logits, name="ZeroInflated"):
    self.count_distribution, self.logits, self.name = count_distribution, np.asarray(logits), name

  def _params(self):
    return self.count_distribution._params() + [self.logits]

  @property
  def probs(self):
    return 1.0 / (1.0 + np.exp(-self.logits))

  @property
  def _complement(self):
    """1 - probs as sigmoid(-logits): the difference cancels from a logit of a few units on (float32: exactly 0 from 17)"""
    return expit(-self.logits)

  def mean(self):
    return self._complement * self.count_distribution.mean()

  def variance(self):
    pi, q, m, v = self.probs, self._complement, self.count_distribution.mean(), self.count_distribution.variance()
    return q * (v + pi * m * m)

  def log_prob(self, x):
    x = np.asarray(x, np.float64)
    g = self.logits.astype(np.float64)
    ell = self.count_distribution.log_prob(x)
    return np.where(x == 0, np.logaddexp(g, ell), ell) - _softplus(g)

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    s = self.count_distribution.sample(sample_shape, seed=rng.integers(1 << 31))
    keep = rng.uniform(size=s.shape) >= np.broadcast_to(self.probs, s.shape)
    return s * keep


class OneHotCategorical(Distribution):
  _event_ndims = 1

  def __init__(self, logits, name="OneHotCategorical"):
    self.logits, self.name = np.asarray(logits), name

  def _params(self):
    return [self.logits]

  def _logp(self):
    m = self.logits.max(-1, keepdims=True)
    return self.logits - (m + np.log(np.exp(self.logits - m).sum(-1, keepdims=True)))

  def mean(self):
    return np.exp(self._logp())

  def variance(self):
    p = self.mean()
    return p * (1 - p)

  def log_prob(self, x):
    return (np.asarray(x) * self._logp()).sum(-1)

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    p = self.mean()
    shp = self._sshape(sample_shape) + p.shape[:-1]
    u = rng.uniform(size=shp + (1,))
    idx = (u > np.cumsum(np.broadcast_to(p, shp + p.shape[-1:]), -1)).sum(-1).clip(0, p.shape[-1] - 1)
    return np.eye(p.shape[-1], dtype=np.float32)[idx]


class Bernoulli(Distribution):
  """Independent binary variables from logits (the 'bernoulli' head: binarised protein markers, several per cell at once).
  TFP Bernoulli semantics: log_prob(y) = y logits - softplus(logits), defined for any y in [0, 1], so a probability matrix
  scores too; sample() draws float 0 / 1."""

  def __init__(self, logits, name="Bernoulli"):
    self.logits, self.name = np.asarray(logits), name

  def _params(self):
    return [self.logits]

  @property
  def probs(self):
    return expit(self.logits.astype(np.float64))

  def mean(self):
    return self.probs

  def variance(self):
    l = self.logits.astype(np.float64)
    return expit(l) * expit(-l)   # (not p (1 - p): 1 - p cancels at saturated logits)

  def log_prob(self, x):
    l = self.logits.astype(np.float64)
    return np.asarray(x, np.float64) * l - _softplus(l)

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    p = self.probs
    return (rng.uniform(size=self._sshape(sample_shape) + p.shape) < p).astype(np.float32)


class MixtureNegativeBinomial(Distribution):
  """Per-dimension mixture of C negative binomials (MISA's label heads, sisua/models/vae.py:47-98; TFP
  MixtureSameFamily(Categorical(logits), NegativeBinomial) semantics).  Parameters [..., C, P]: mixture logits, total
  counts, logits; batch shape [..., P]."""

  def __init__(self, mix_logits, total_count, logits, name="MixtureNegativeBinomial", gate_logits=None):
    self.mix_logits = np.asarray(mix_logits, np.float64)
    self.components = NegativeBinomial(total_count, logits)
    if gate_logits is not None:   # MISA(zero_inflated=True): every component zero-inflated by its own gate
      self.components = ZeroInflated(self.components, np.asarray(gate_logits, np.float64))
    self.name = name

  def _params(self):
    return [self.mix_logits[..., 0, :]]

  def _log_pi(self):
    m = self.mix_logits.max(-2, keepdims=True)
    return self.mix_logits - (m + np.log(np.exp(self.mix_logits - m).sum(-2, keepdims=True)))

  def mean(self):
    return (np.exp(self._log_pi()) * self.components.mean()).sum(-2)

  def variance(self):   # law of total variance over the component index
    pi, mc = np.exp(self._log_pi()), self.components.mean()
    mean = (pi * mc).sum(-2, keepdims=True)
    return (pi * (self.components.variance() + (mc - mean) ** 2)).sum(-2)

  def log_prob(self, x):
    j = self._log_pi() + self.components.log_prob(np.asarray(x, np.float64)[..., None, :])
    m = j.max(-2, keepdims=True)
    return (m + np.log(np.exp(j - m).sum(-2, keepdims=True)))[..., 0, :]

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    comp = self.components.sample(sample_shape, seed=rng.integers(1 << 31))          # [S.., ..., C, P]
    pi = np.broadcast_to(np.exp(self._log_pi()), comp.shape)
    u = rng.uniform(size=comp.shape[:-2] + comp.shape[-1:])[..., None, :]
    pick = (np.cumsum(pi, axis=-2) < u).sum(-2, keepdims=True).clip(0, comp.shape[-2] - 1)
    return np.take_along_axis(comp, pick, axis=-2)[..., 0, :]


class MixtureNormal(MixtureNegativeBinomial):
  """Per-dimension mixture of C normals (MISA's heads for continuous labels, 'mixgaussian', sisua/models/vae.py:86-92; TFP
  MixtureSameFamily(Categorical(logits), Normal) semantics).  Parameters [..., C, P]: mixture logits, locations, scales."""

  def __init__(self, mix_logits, loc, scale, name="MixtureNormal"):
    self.mix_logits = np.asarray(mix_logits, np.float64)
    self.components = Normal(loc, scale)
    self.name = name


class MixtureMultivariateNormalTriL(Distribution):
  """ONE mixture of C full-covariance Gaussians over the last axis (MISA's 'mixtril' heads, the example of
  sisua/models/vae.py:58; TFP MixtureSameFamily(Categorical(logits), MultivariateNormalTriL(loc, scale_tril)) semantics).
  Parameters: mixture logits [..., C], locations [..., C, P], lower-triangular scale factors [..., C, P, P]."""
  _event_ndims = 1

  def __init__(self, mix_logits, loc, scale_tril, name="MixtureMultivariateNormalTriL"):
    self.mix_logits = np.asarray(mix_logits, np.float64)
    self.loc = np.asarray(loc, np.float64)
    self.scale_tril = np.tril(np.asarray(scale_tril, np.float64))
    self.name = name

  def _params(self):
    return [self.loc[..., 0, :]]

  def _log_pi(self):
    a = self.mix_logits
    m = a.max(-1, keepdims=True)
    return a - (m + np.log(np.exp(a - m).sum(-1, keepdims=True)))

  def mean(self):
    return (np.exp(self._log_pi())[..., None] * self.loc).sum(-2)

  def covariance(self):
    """Law of total covariance: sum_c pi_c (L_c L_c^T + mu_c mu_c^T) - mean mean^T."""
    pi = np.exp(self._log_pi())[..., None, None]
    second = self.scale_tril @ np.swapaxes(self.scale_tril, -1, -2) + self.loc[..., :, None] * self.loc[..., None, :]
    mu = self.mean()
    return (pi * second).sum(-3) - mu[..., :, None] * mu[..., None, :]

  def variance(self):
    return np.einsum("...pp->...p", self.covariance())

  def component_log_prob(self, x):
    """log N(x; loc_c, L_c L_c^T) per component: [..., C]."""
    d = np.asarray(x, np.float64)[..., None, :] - self.loc
    L = np.broadcast_to(self.scale_tril, d.shape[:-1] + self.scale_tril.shape[-2:])
    u = np.zeros(d.shape)
    P = d.shape[-1]
    for p in range(P):   # forward substitution (P is tens at most)
      u[..., p] = (d[..., p] - (L[..., p, :p] * u[..., :p]).sum(-1)) / L[..., p, p]
    logdet = np.log(np.einsum("...pp->...p", L)).sum(-1)
    return -0.5 * (u * u).sum(-1) - logdet - 0.5 * P * np.log(2.0 * np.pi)

  def log_prob(self, x):
    j = self._log_pi() + self.component_log_prob(x)
    m = j.max(-1, keepdims=True)
    return (m + np.log(np.exp(j - m).sum(-1, keepdims=True)))[..., 0]

  def sample(self, sample_shape=(), seed=None):
    rng = np.random.default_rng(seed)
    shp = self._sshape(sample_shape)
    pi = np.exp(self._log_pi())
    bshape = pi.shape[:-1]
    u = rng.uniform(size=shp + bshape)[..., None]
    pick = (np.cumsum(np.broadcast_to(pi, shp + pi.shape), axis=-1) < u).sum(-1).clip(0, pi.shape[-1] - 1)        # [S.., ...]
    eps = rng.standard_normal(size=shp + bshape + self.loc.shape[-1:])
    loc = np.take_along_axis(np.broadcast_to(self.loc, shp + self.loc.shape), pick[..., None, None], axis=-2)[..., 0, :]
    L = np.take_along_axis(np.broadcast_to(self.scale_tril, shp + self.scale_tril.shape), pick[..., None, None, None], axis=-3)[..., 0, :, :]
    return loc + np.einsum("...pq,...q->...p", L, eps)


class Independent(Distribution):
  """Reinterprets the last `reinterpreted_batch_ndims` batch axes as event axes."""

  def __init__(self, distribution: Distribution, reinterpreted_batch_ndims: int = 1, name=None):
    self.distribution = distribution
    self.reinterpreted_batch_ndims = int(reinterpreted_batch_ndims)
    self.name = name or distribution.name

  def _params(self):
    return self.distribution._params()

  @property
  def batch_shape(self):
    b = self.distribution.batch_shape
    return tuple(b[:len(b) - self.reinterpreted_batch_ndims])

  @property
  def event_shape(self):
    b = self.distribution.batch_shape
    return tuple(b[len(b) - self.reinterpreted_batch_ndims:]) + tuple(self.distribution.event_shape)

  def mean(self):
    return self.distribution.mean()

  def variance(self):
    return self.distribution.variance()

  def sample(self, sample_shape=(), seed=None):
    return self.distribution.sample(sample_shape, seed)

  def log_prob(self, x):
    lp = self.distribution.log_prob(x)
    return lp.sum(axis=tuple(range(-self.reinterpreted_batch_ndims, 0)))


# ---------------------------------------------------------------------------
def _cat(arrs, axis):
  return np.concatenate([np.asarray(a) for a in arrs], axis=axis)


def concat_distributions(dists: Sequence[Distribution], axis: int = 0, name: Optional[str] = None) -> Distribution:
  """Merge per-minibatch distributions along a batch axis (odin `concat_distributions`,
  used by SingleCellModel.predict, single_cell_model.py:184-210)."""
  d0 = dists[0]
  nm = name or d0.name
  if isinstance(d0, Independent):
    return Independent(concat_distributions([d.distribution for d in dists], axis, d0.distribution.name),
                       d0.reinterpreted_batch_ndims, name=nm)
  if isinstance(d0, ZeroInflated):
    return ZeroInflated(concat_distributions([d.count_distribution for d in dists], axis, d0.count_distribution.name),
                        _cat([d.logits for d in dists], axis), name=nm)
  if isinstance(d0, MultivariateNormalTriL):
    return MultivariateNormalTriL(_cat([d.loc for d in dists], axis), _cat([d.scale_tril for d in dists], axis), name=nm)
  if isinstance(d0, MultivariateNormalDiag):
    return MultivariateNormalDiag(_cat([d.loc for d in dists], axis), _cat([d.scale for d in dists], axis), name=nm)
  if isinstance(d0, Normal):
    return Normal(_cat([d.loc for d in dists], axis), _cat([d.scale for d in dists], axis), name=nm)
  if isinstance(d0, Deterministic):
    return Deterministic(_cat([d.loc for d in dists], axis), name=nm)
  if isinstance(d0, NegativeBinomial):
    return NegativeBinomial(_cat([d.total_count for d in dists], axis), _cat([d.logits for d in dists], axis), name=nm)
  if isinstance(d0, NegativeBinomialDisp):
    return NegativeBinomialDisp(_cat([d.loc for d in dists], axis), _cat([d.disp for d in dists], axis), name=nm)
  if isinstance(d0, OneHotCategorical):
    return OneHotCategorical(_cat([d.logits for d in dists], axis), name=nm)
  if isinstance(d0, Bernoulli):
    return Bernoulli(_cat([d.logits for d in dists], axis), name=nm)
  if isinstance(d0, MixtureNormal):
    return MixtureNormal(_cat([d.mix_logits for d in dists], axis), _cat([d.components.loc for d in dists], axis),
                         _cat([d.components.scale for d in dists], axis), name=nm)
  if isinstance(d0, MixtureNegativeBinomial) and isinstance(d0.components, ZeroInflated):
    return MixtureNegativeBinomial(_cat([d.mix_logits for d in dists], axis), _cat([d.components.count_distribution.total_count for d in dists], axis),
                                   _cat([d.components.count_distribution.logits for d in dists], axis), name=nm,
                                   gate_logits=_cat([d.components.logits for d in dists], axis))
  if isinstance(d0, MixtureNegativeBinomial):   # parameters [..., C, P]: the batch axes are the leading ones
    return MixtureNegativeBinomial(_cat([d.mix_logits for d in dists], axis), _cat([d.components.total_count for d in dists], axis),
                                   _cat([d.components.logits for d in dists], axis), name=nm)
  if isinstance(d0, MixtureMultivariateNormalTriL):
    return MixtureMultivariateNormalTriL(_cat([d.mix_logits for d in dists], axis), _cat([d.loc for d in dists], axis),
                                         _cat([d.scale_tril for d in dists], axis), name=nm)
  raise TypeError(f"cannot concatenate {type(d0)}")


def count_distribution(likelihood: str, planes, name: str, activated: bool) -> Distribution:
  """Build the output distribution from the parameter planes of smx_forward.
  nb/zinb planes: (log total_count, logits[, gate]); nbd/zinbd: pre-activation
  (softplus mean, softplus1 dispersion) unless `activated` (scvi feeds mean/disp);
  bernoulli: logits; normal / gaussian / diag: (loc, softplus1 scale)."""
  if likelihood == "mse":   # one plane: the mean (RVmeta(dim, 'mse'): deterministic output)
    return VectorDeterministic(planes[0], name=name)
  if likelihood == "bernoulli":   # one plane: logits (binarised peak matrices)
    return Independent(Bernoulli(logits=planes[0]), 1, name=name)
  if likelihood in ("normal", "gaussian", "diag"):   # loc | raw scale, scale = softplus(raw + softplus^-1(1)); 'diag': the reference's own test
    loc, scale = planes[0], _softplus(np.asarray(planes[1], np.float64) + SOFTPLUS_INV_1)
    return MultivariateNormalDiag(loc, scale, name=name) if likelihood == "diag" else Independent(Normal(loc, scale), 1, name=name)
  if likelihood in ("nb", "zinb"):
    base = NegativeBinomial(logits=planes[1], name="NegativeBinomial", log_total_count=planes[0])
  else:
    if activated:
      mu, th = planes[0], planes[1]
    else:
      mu, th = _softplus(planes[0]), _softplus(planes[1] + SOFTPLUS_INV_1)
    base = NegativeBinomialDisp(mu, th, name="NegativeBinomialDisp")
  if likelihood in ("zinb", "zinbd"):
    base = ZeroInflated(base, planes[2], name="ZeroInflated")
  return Independent(base, 1, name=name)


def imputation_scores_from_cells(cell_median, cell_changed, global_lohi):
  """The reference's closing reductions (imputation_benchmarks.py:102-127) of what the device selected: np.mean / np.std of the float32
  medians of the changed cells (0 for none), and np.median's mean of the two middle values, 0.5 (lo + hi) in float32."""
  cells = [m for m, c in zip(np.asarray(cell_median, np.float32), np.asarray(cell_changed)) if c]
  lo, hi = np.asarray(global_lohi, np.float32)
  with np.errstate(over="ignore", invalid="ignore"):
    med = np.float32(0.5) * (lo + hi)
  return {"imputation_med": float(med),
          "imputation_mean": float(np.mean(cells)) if len(cells) > 0 else 0.0,
          "imputation_std": float(np.std(cells)) if len(cells) > 0 else 0.0}


def protein_operands(extras):
  """What the device's correlation sums read of the protein matrix `extras` [N, P] (dense or scipy.sparse), prepared once in float64:
  dict(rank2 [P, N] int32: 2 x scipy.stats.rankdata(column) -- integers; unit [P, N] float64: the column centred and scaled to unit norm
  (zeros for a constant column); Sb, Sbb: lists of P Python integers sum b, sum b b; constant [P] bool).  A NaN or an infinity raises."""
  from scipy.stats import rankdata
  ex = np.asarray(extras.toarray() if _sp.issparse(extras) else extras, np.float64)
  if ex.ndim != 2 or ex.shape[1] < 1:
    raise ValueError(f"extras must be [cells, proteins >= 1], got {ex.shape}")
  if not np.isfinite(ex).all():
    raise ValueError("extras holds a NaN or an infinity")
  cols = np.ascontiguousarray(ex.T)
  rank2 = np.stack([np.rint(2.0 * rankdata(c)).astype(np.int32) for c in cols])
  constant = np.array([bool((c == c[0]).all()) for c in cols])
  unit = np.zeros_like(cols)
  for p, c in enumerate(cols):
    if not constant[p]:
      d = c - c.mean()
      unit[p] = d / np.linalg.norm(d)
  r = rank2.astype(np.int64)
  return dict(rank2=rank2, unit=unit, Sb=[int(v) for v in r.sum(axis=1)], Sbb=[int(v) for v in (r * r).sum(axis=1)], constant=constant)


def correlations_from_sums(n_cells, sp_Sa, sp_Saa, sp_Sab, sp_Sb, sp_Sbb, pe_Sxx, pe_Sxy, nonfinite=None, prot_constant=None):
  """The closing arithmetic of the gene x protein correlation matrices -> {'pearson', 'spearman'}, each [G, P] float64.
  Spearman = (N Sab - Sa Sb) / sqrt((N Saa - Sa^2)(N Sbb - Sb^2)) from the integer sums of the doubled average ranks (a of a gene, b of a
  protein): numerator and both factors in Python integers -- exact -- then one float64 division.  Pearson = Sxy / sqrt(Sxx), Sxy against
  the protein column of unit norm, clipped to [-1, 1] as scipy.stats.pearsonr clips.  NaN where the gene column is non-finite or constant
  (N Saa == Sa^2: all its ranks tie) or the protein column is constant: SciPy's answer for a constant input."""
  N = int(n_cells)
  obj = lambda a: np.array([int(v) for v in np.ravel(a)], dtype=object).reshape(np.shape(a))
  Sa, Saa, Sab, Sb, Sbb = obj(sp_Sa), obj(sp_Saa), obj(sp_Sab), obj(sp_Sb), obj(sp_Sbb)
  G, P = Sab.shape
  da, db = N * Saa - Sa * Sa, N * Sbb - Sb * Sb   # N^2 x the variance of the ranks: 0 exactly for a constant column
  num = N * Sab - Sa[:, None] * Sb[None, :]
  bad = np.broadcast_to((da == 0)[:, None] | (db == 0)[None, :], (G, P)).copy()
  if nonfinite is not None:
    bad |= (np.asarray(nonfinite) != 0)[:, None]
  if prot_constant is not None:
    bad |= np.asarray(prot_constant, bool)[None, :]
  den = (da[:, None] * db[None, :]).astype(np.float64)
  with np.errstate(divide="ignore", invalid="ignore"):
    spearman = num.astype(np.float64) / np.sqrt(den)
    pearson = np.clip(np.asarray(pe_Sxy, np.float64) / np.sqrt(np.asarray(pe_Sxx, np.float64))[:, None], -1.0, 1.0)
  spearman[bad] = np.nan
  pearson[bad] = np.nan
  return {"pearson": pearson, "spearman": spearman}


# ---------------------------------------------------------------------------
class LazyCountOutput(Distribution):
  """predict()'s gene output as a handle on the DEVICE side: the parameter planes (4 k G bytes per cell and draw: 24 KB at 1998 genes)
  never reach the host; `mean()`, `variance()`, `log_prob(x)` run the evaluation passes again inside the library (smx_predict_stat: a
  forward pass of 128 cells takes ~40 us) and only the statistic asked for leaves the device.  Same surface as the eager result of
  `count_distribution` -- `.distribution` (the Independent wrapper's inner distribution), `.count_distribution` of a zero-inflated
  output (sisua/analysis/posterior.py:187-255), `batch_shape` / `event_shape` / `name` -- and `materialize()` returns that eager result
  (bit-identical planes); any other attribute of the eager result is looked up there.  The handle is valid while the model's parameters
  stay as they were: after further training or a `load_weights` it raises.  Unlike the eager path of rounds 1-3 the input is taken whole
  (`SingleCellOMIC.numpy()`): the remainder cells of the last minibatch are part of the result."""

  reinterpreted_batch_ndims = 1

  def __init__(self, model, x, library, n_samples, batch, name, count_only=False):
    self._model, self._x, self._lib, self._S, self._B, self.name = model, x, library, int(n_samples), int(batch), name
    self._count_only = bool(count_only)
    # (the optimiser step AND a counter that every restore of weights bumps: load_weights at the same step gives other parameters -- ADVICE r04)
    self._step = (model.step, getattr(model, "_param_version", 0))
    self._eager = None

  # ---- structure -----------------------------------------------------------------
  @property
  def is_zero_inflated(self):
    return self._model._cfg.likelihood in ("zinb", "zinbd") and not self._count_only

  @property
  def batch_shape(self):
    n = self._x.shape[0]
    return (self._S, n) if self._S > 1 else (n,)

  @property
  def event_shape(self):
    return (self._model._cfg.n_genes,)

  @property
  def distribution(self):
    return self

  @property
  def count_distribution(self):
    if not self.is_zero_inflated:
      raise AttributeError("count_distribution: the output is not zero-inflated")
    return LazyCountOutput(self._model, self._x, self._lib, self._S, self._B, self.name, count_only=True)

  def _params(self):
    return []

  # ---- statistics (kernels) ---------------------------------------------------------
  def _engine(self):
    if (self._model.step, getattr(self._model, "_param_version", 0)) != self._step:
      raise RuntimeError("the model's parameters changed (training or load_weights) after this lazy prediction was made: call predict() again")
    return self._model._ensure_engine(max(self._B, 512 if self._x.shape[0] >= 1024 else 1))

  def _stat(self, stat, target=None, out=None):
    squeeze = self._S <= 1 and stat != "mean_over_samples"   # (no draw axis in the caller's view)
    o = out if (out is None or not squeeze) else out.reshape((1,) + tuple(out.shape))
    r = self._engine().predict_stat(self._x, stat, library=self._lib, n_samples=max(self._S, 1), batch=self._B, count_only=self._count_only,
                                    target=target, out=o)
    return (out if out is not None else r[0]) if squeeze else r

  def mean(self, out=None):
    return self._stat("mean", out=out)

  def variance(self, out=None):
    return self._stat("variance", out=out)

  def mean_over_samples(self, genes=None, out=None):
    """E_s[mean] over the Monte-Carlo draws, [n_cells, n_genes] (what `np.mean(imputed.mean(), axis=0)` computes, posterior.py:985-987).
    genes: a list of gene indices (any order, repeats allowed) -- only those columns leave the device, [n_cells, len(genes)], the same
    bits as `mean_over_samples()[:, genes]` (smx_predict_stat_cols: what the marker correlations of sc_metrics.py:287-348 read)."""
    if genes is None:
      return self._stat("mean_over_samples", out=out)
    return self._engine().predict_stat(self._x, "mean_over_samples", library=self._lib, n_samples=max(self._S, 1), batch=self._B,
                                       count_only=self._count_only, out=out, genes=genes)

  def imputation_cells(self, original):
    """What the device reduces for `imputation_scores` (Engine.predict_impute): dict(cell_median [N], cell_changed [N], global_lohi [2]).
    On a zero-inflated output the count distribution is scored, as the reference does (posterior.py:218-225)."""
    if original is None:
      raise ValueError("imputation scores need the original counts")
    n, g = self._x.shape[0], self.event_shape[0]
    if not _sp.issparse(original):
      original = np.asarray(original, np.float32)
    if tuple(original.shape) != (n, g):
      raise ValueError(f"original must have the prediction's shape {(n, g)}, got {tuple(original.shape)}")
    count_only = self._count_only or self.is_zero_inflated
    return self._engine().predict_impute(self._x, original, library=self._lib, n_samples=max(self._S, 1), batch=self._B, count_only=count_only)

  def imputation_scores(self, original):
    """The three scores of `Posterior.cal_imputation_scores` (posterior.py:978-993; imputation_benchmarks.py:102-127) of this prediction,
    the handle's own input being the CORRUPTED matrix: {'imputation_med': median of |original - imputed| over all entries,
    'imputation_mean' / 'imputation_std': mean / standard deviation of the per-cell medians over the cells whose total count the
    corruption changed (0 without any)}, `imputed` = `mean_over_samples()` of the count distribution.  The medians are selected on the
    device (exactly; smx_impute.hip) -- 8 bytes per cell leave it instead of 4 n_genes; the closing lines are the reference's, on the host."""
    r = self.imputation_cells(original)
    return imputation_scores_from_cells(r["cell_median"], r["cell_changed"], r["global_lohi"])

  def correlation_sums(self, operands, genes=None):
    """What the device reduces for `correlation` (Engine.predict_correlate) against `protein_operands(extras)`; on a zero-inflated output
    the count distribution's mean is correlated, as `metrics.CorrelationScores` does."""
    if operands["rank2"].shape[1] != self._x.shape[0]:
      raise ValueError(f"extras must have the prediction's {self._x.shape[0]} cells, got {operands['rank2'].shape[1]}")
    count_only = self._count_only or self.is_zero_inflated
    return self._engine().predict_correlate(self._x, operands["rank2"], operands["unit"], library=self._lib, n_samples=max(self._S, 1),
                                            batch=self._B, count_only=count_only, genes=genes)

  def correlation(self, extras, genes=None):
    """The gene x protein correlation matrices of SingleCellOMIC.get_correlation (_single_cell_analysis.py:1199-1245: pearsonr and
    spearmanr of every pair) between `mean_over_samples()` of this prediction and the protein levels `extras` [n_cells, P] (dense or
    scipy.sparse; a NaN raises ValueError): {'pearson': [G', P], 'spearman': [G', P]} float64, G' = all genes or the list `genes` (any
    order, repeats allowed).  The ranks and every sum over the cells are computed on the device (smx_correlate.hip) -- Spearman exactly,
    from integer sums -- and 16 + 16 P bytes per gene leave it instead of 4 n_cells; the closing division is `correlations_from_sums`.  A
    gene whose column is constant or not finite, and a constant protein, give NaN."""
    ops = protein_operands(extras)
    r = self.correlation_sums(ops, genes)
    return correlations_from_sums(self._x.shape[0], r["sp_Sa"], r["sp_Saa"], r["sp_Sab"], ops["Sb"], ops["Sbb"], r["pe_Sxx"], r["pe_Sxy"],
                                  r["nonfinite"], ops["constant"])

  def mutual_information(self, extras, genes=None, n_neighbors=3):
    """The gene x protein mutual-information matrix [G', P] float64 (`sisua_amd.mutual_information`: scikit-learn's kNN estimators with
    seed 1, on the device) between `mean_over_samples()` of this prediction and the protein levels `extras` [n_cells, P]; G' = all genes
    or the list `genes` (any order, repeats allowed).  On a zero-inflated output the count distribution's mean is used, as `correlation`
    does.  The columns come through `mean_over_samples(genes=...)`: the predict walk is what it was."""
    from sisua_amd.mutual_info import mutual_information
    ex = np.asarray(extras.toarray() if _sp.issparse(extras) else extras, np.float64)
    if ex.ndim != 2 or ex.shape[0] != self._x.shape[0]:
      raise ValueError(f"extras must be [{self._x.shape[0]}, proteins], got {ex.shape}")
    h = self.count_distribution if self.is_zero_inflated else self
    sel = list(range(self.event_shape[0])) if genes is None else [int(g) for g in genes]
    cols = h.mean_over_samples(genes=sel)   # [n_cells, G'] float32
    return mutual_information(cols, ex, n_neighbors=n_neighbors, random_state=1)

  def log_prob(self, x=None):
    """log p(x) summed over the genes, [n_samples, n_cells] ([n_cells] without a draw axis); x = None: of the input counts.  x may be
    scipy.sparse."""
    if x is not None and not _sp.issparse(x):   # (a sparse target goes to the device as CSR)
      x = np.asarray(x, np.float32)
    return self._stat("log_prob", target=x)

  # ---- everything else through the eager result ----------------------------------------
  def materialize(self):
    if self._eager is None:
      pX, _ = self._model.predict(self._x, sample_shape=(self._S,) if self._S > 1 else (), batch_size=self._B, verbose=False, lazy=False)
      pX = pX[0] if isinstance(pX, tuple) else pX
      self._eager = pX.distribution.count_distribution if (self._count_only and hasattr(pX.distribution, "count_distribution")) else pX
      self._engine()   # (raises if the model moved on)
    return self._eager

  def sample(self, sample_shape=(), seed=None, out=None):
    """Posterior-predictive draws on the device (smx_predict_sample): float32 of shape sample_shape + batch_shape + event_shape, as the
    eager distributions return it -- `sample()` of S latent draws is [S, N, G], `sample(3)` [3, S, N, G], `sample((2, 3))` [2, 3, S, N, G];
    on `.count_distribution`: without the zero-inflation gate.  An integer seed gives the same bits every time, at any batch size and
    from a dense or a sparse input; seed=None takes fresh entropy.  `out`: a C-contiguous float32 array of the result's shape."""
    sshape = self._sshape(sample_shape)
    n = int(np.prod(sshape, dtype=np.int64)) if sshape else 1
    shape = sshape + self.batch_shape + self.event_shape
    if n < 1:
      raise ValueError("sample_shape must have at least one element")
    if seed is None:
      seed = int(np.random.SeedSequence().generate_state(1, np.uint64)[0])
    if out is not None and (out.dtype != np.float32 or tuple(out.shape) != shape or not out.flags.c_contiguous):
      raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
    S, N, G = max(self._S, 1), self._x.shape[0], self.event_shape[0]
    r = self._engine().predict_stat(self._x, "sample", library=self._lib, n_samples=S, batch=self._B, count_only=self._count_only,
                                    out=None if out is None else out.reshape(n, S, N, G), seed=seed, n=n)
    return out if out is not None else r.reshape(shape)

  def __getattr__(self, name):
    # anything else a caller of the reference touches on the eager result (`.logits`, `.total_count`, `.inflated_distribution`, ...):
    # through the materialised distribution.  (Only reached for attributes this class does not define.)
    if name.startswith("_"):
      raise AttributeError(name)
    d = self.materialize()
    inner = getattr(d, "distribution", d)
    for obj in (d, inner):
      if hasattr(obj, name):
        return getattr(obj, name)
    raise AttributeError(f"{type(self).__name__} (and the distribution it stands for) has no attribute '{name}'")

  def __repr__(self):
    return f"<LazyCountOutput '{self.name}' batch_shape={self.batch_shape} event_shape={self.event_shape} on device>"
