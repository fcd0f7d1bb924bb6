"""float64 closed forms of the gene output's predictive laws, and the acceptance functions the sampling tests apply to a block of draws.

Count laws are the negative binomial with shape r and mean m (pmf Gamma(x + r) / (Gamma(r) x!) (r / (r + m))^r (m / (r + m))^x), alone or
under a zero-inflation gate: with probability pi the draw is 0.  Both parameterisations of the library map onto (r, m):
  'nb'  planes (log total_count, logits): r = exp(p0), m = r exp(p1);
  'nbd' planes (raw mean, raw dispersion): m = softplus(p0), r = softplus(p1 + softplus^-1(1)); `direct`: m = p0, r = p1.

Acceptance (the bounds are derived, none is tuned):
  (a) moments_check: |mean(x) - m| <= 6 sqrt(v / N) and |var(x) - v| <= 6 sqrt((mu4 - v^2) / N), mu4 the fourth central moment in closed form
      from the factorial moments E[X (X - 1) .. (X - j + 1)] = Gamma(r + j) / Gamma(r) (m / r)^j (times 1 - pi under the gate);
  (b) chi2_check: Pearson's statistic against the float64 law over bins merged to an expected count >= 8, accepted at the 1 - 1e-6 quantile
      of its chi-square law;  ks_check (continuous laws): the Kolmogorov-Smirnov distance at the same level.
"""
import numpy as np
from scipy import special, stats

SOFTPLUS_INV_1 = float(np.log(np.e - 1.0))
N_SIGMA = 6.0
LEVEL = 1e-6          # false-rejection probability of one goodness-of-fit test
MIN_EXPECTED = 8.0

SHAPES = (0.05, 0.5, 1.0, 3.0, 50.0, 1000.0)
MEANS = (0.01, 0.3, 2.0, 15.0, 200.0, 5000.0)
GATES = (None, 0.1, 0.7)
PARAMETERISATIONS = ("nb", "nbd", "nbd_direct")
# (no logit 0: at p = 1 / 2 the sample variance p^ (1 - p^) has no first-order spread, mu4 = v^2, and bound (a) on it is 0 / 0)
BERNOULLI_LOGITS = (-6.0, -3.0, -1.0, -0.25, 0.5, 2.0, 4.0, 6.0)
NORMAL_POINTS = ((0.0, 0.0), (-3.5, -2.0), (12.0, 1.5), (0.25, -6.0), (100.0, 4.0))   # (loc, raw scale)


def softplus(x):
  return np.logaddexp(0.0, np.asarray(x, np.float64))


def softplus_inv(y):
  y = np.asarray(y, np.float64)
  return y + np.log(-np.expm1(-y))


def logit(p):
  return float(np.log(p) - np.log1p(-p))


# ---- planes <-> (r, m, pi) ---------------------------------------------------------------
def count_planes(param, r, m, pi=None):
  """float32 planes (p0, p1[, p2]) of one parameter point in parameterisation `param`."""
  if param == "nb":
    p = [np.log(r), np.log(m / r)]
  elif param == "nbd":
    p = [softplus_inv(m), softplus_inv(r) - SOFTPLUS_INV_1]
  elif param == "nbd_direct":
    p = [m, r]
  else:
    raise ValueError(param)
  if pi is not None:
    p.append(logit(pi))
  return [np.float32(v) for v in p]


def count_params(param, planes):
  """(r, m, pi) in float64 of float32 planes -- what the kernel is asked to sample, exactly."""
  p = [np.asarray(v, np.float32).astype(np.float64) for v in planes]
  if param == "nb":
    r = np.exp(p[0]); m = r * np.exp(p[1])
  elif param == "nbd":
    m = softplus(p[0]); r = softplus(p[1] + SOFTPLUS_INV_1)
  else:
    m, r = p[0], p[1]
  pi = 1.0 / (1.0 + np.exp(-p[2])) if len(p) > 2 else None
  return r, m, pi


# ---- the laws -------------------------------------------------------------------------------
class CountLaw:
  """NB(r, mean m), zero-inflated with probability pi (None: no gate)."""

  def __init__(self, r, m, pi=None):
    self.r, self.m, self.pi = float(r), float(m), (0.0 if pi is None else float(pi))
    self.nb = stats.nbinom(self.r, self.r / (self.r + self.m))

  def pmf(self, x):
    x = np.asarray(x)
    return (1.0 - self.pi) * self.nb.pmf(x) + self.pi * (x == 0)

  def cdf(self, x):
    x = np.asarray(x, np.float64)
    return np.where(x < 0, 0.0, self.pi + (1.0 - self.pi) * self.nb.cdf(x))

  def sf(self, x):
    x = np.asarray(x, np.float64)
    return np.where(x < 0, 1.0, (1.0 - self.pi) * self.nb.sf(x))

  def factorial_moment(self, j):
    return (1.0 - self.pi) * float(np.exp(special.gammaln(self.r + j) - special.gammaln(self.r) + j * (np.log(self.m) - np.log(self.r))))

  def moments(self):
    """mean, variance, fourth central moment"""
    f1, f2, f3, f4 = (self.factorial_moment(j) for j in (1, 2, 3, 4))
    e1, e2, e3, e4 = f1, f2 + f1, f3 + 3 * f2 + f1, f4 + 6 * f3 + 7 * f2 + f1
    return e1, e2 - e1 * e1, e4 - 4 * e3 * e1 + 6 * e2 * e1 * e1 - 3 * e1 ** 4

  def edges(self):
    """candidate bin edges (upper ends, integers): every integer up to 64 and the integer quantiles of the law"""
    q = self.nb.ppf(np.linspace(0.0, 1.0, 513)[1:-1])
    e = np.unique(np.concatenate([np.arange(0, 65, dtype=np.float64), q[np.isfinite(q)]]))
    return e[e >= 0]


class BernoulliLaw:

  def __init__(self, logits):
    self.p = float(1.0 / (1.0 + np.exp(-np.float64(np.float32(logits)))))

  def cdf(self, x):
    x = np.asarray(x, np.float64)
    return np.where(x < 0, 0.0, np.where(x < 1, 1.0 - self.p, 1.0))

  def sf(self, x):
    return 1.0 - self.cdf(x)

  def moments(self):
    p = self.p
    return p, p * (1 - p), p * (1 - p) * (1 - 3 * p * (1 - p))

  def edges(self):
    return np.array([0.0, 1.0])


class NormalLaw:

  def __init__(self, loc, raw_scale):
    self.loc = float(np.float32(loc))
    self.scale = float(softplus(np.float64(np.float32(raw_scale)) + SOFTPLUS_INV_1))

  def cdf(self, x):
    return stats.norm.cdf(x, self.loc, self.scale)

  def moments(self):
    return self.loc, self.scale ** 2, 3.0 * self.scale ** 4


# ---- acceptance -------------------------------------------------------------------------------
def moments_check(x, law, n_sigma=N_SIGMA):
  """(ok, z of the mean, z of the variance): the sample mean and variance within n_sigma standard errors of the law's"""
  x = np.asarray(x, np.float64).ravel()
  n = x.size
  m, v, mu4 = law.moments()
  zm = (x.mean() - m) / np.sqrt(v / n)
  zv = (x.var() - v) / np.sqrt((mu4 - v * v) / n)
  return bool(np.isfinite(zm) and np.isfinite(zv) and abs(zm) <= n_sigma and abs(zv) <= n_sigma), float(zm), float(zv)


def merged_bins(law, n):
  """upper bin ends (the last bin is open) and expected counts, every bin expecting >= MIN_EXPECTED of n draws"""
  e = law.edges()
  cdf = law.cdf(e)
  mass = np.diff(np.concatenate([[0.0], cdf]))          # P(e[i-1] < X <= e[i])
  tail = float(law.sf(e[-1]))                           # P(X > e[-1])
  ends, exp, acc = [], [], 0.0
  for hi, p in zip(e, mass):
    acc += n * p
    if acc >= MIN_EXPECTED:
      ends.append(hi); exp.append(acc); acc = 0.0
  acc += n * tail                                        # what lies above the last closed bin
  if acc >= MIN_EXPECTED or not exp:
    exp.append(acc)                                     # ... is the open bin above ends[-1]
  else:
    ends.pop(); exp[-1] += acc                          # ... or joins the last closed bin, which becomes the open one
  # bins: (ends[i - 1], ends[i]] for i < len(ends), and one open bin above ends[-1]
  return np.asarray(ends, np.float64), np.asarray(exp, np.float64)


def chi2_check(x, law, level=LEVEL):
  """(ok, statistic, critical value, bins): Pearson's chi-square of the draws against the law over merged_bins"""
  x = np.asarray(x, np.float64).ravel()
  if not np.all(np.isfinite(x)):
    return False, np.inf, 0.0, 0
  ends, exp = merged_bins(law, x.size)
  idx = np.searchsorted(ends, x, side="left")          # x <= ends[i] -> bin i; above every end -> the open bin
  obs = np.bincount(idx, minlength=exp.size).astype(np.float64)
  assert obs.size == exp.size and abs(exp.sum() - x.size) < 1e-6 * x.size
  if exp.size < 2:
    return bool(obs[0] == x.size), 0.0, 0.0, int(exp.size)
  stat = float(((obs - exp) ** 2 / exp).sum())
  crit = float(stats.chi2.isf(level, exp.size - 1))
  return stat <= crit, stat, crit, int(exp.size)


def ks_check(x, law, level=LEVEL):
  """(ok, distance, critical value): Kolmogorov-Smirnov against the law's cdf"""
  x = np.sort(np.asarray(x, np.float64).ravel())
  n = x.size
  if not np.all(np.isfinite(x)):
    return False, np.inf, 0.0
  c = law.cdf(x)
  d = float(max(np.max(np.arange(1, n + 1) / n - c), np.max(c - np.arange(0, n) / n)))
  crit = float(stats.kstwo.isf(level, n))
  return d <= crit, d, crit


def integer_valued(x):
  x = np.asarray(x)
  return bool(np.all(np.isfinite(x)) and np.all(x >= 0) and np.all(x == np.floor(x)))
