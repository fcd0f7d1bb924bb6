"""float64 reference of predict()'s gene-output statistics (smx_predict_stat; plane_moments, rv_moments and the plane_logprob kernels of
sisua_amd/csrc/smx_predict.hip), the edge grid they are held to, and the float32 error bounds of the kernels' formulas.

NumPy float64 only, an independent restatement: nothing here comes from sisua_amd/distributions.py.  Every function takes the float32
parameter planes as they were read back from the device, so nothing upstream of the statistic kernels enters a comparison.

Well-conditioned forms only:
  * the gate complement 1 - pi is expit(-g), never 1 - expit(g); the Bernoulli variance is expit(l) expit(-l);
  * softplus is np.logaddexp(0, x); the zero-inflated zero term log(pi + (1 - pi) exp(ell)) is np.logaddexp(g, ell) - softplus(g)
    where it is below log(1/2) and log1p((1 - pi) expm1(ell)) above (there the two logaddexp terms cancel: g = -40 next to an ell of
    -1e-33 left 22 % of error against mpmath);
  * the Bernoulli log-probability x l - softplus(l) is written -x softplus(-l) - (1 - x) softplus(l): two terms of one sign;
  * lgamma(x + r) - lgamma(r) - lgamma(x + 1) of an integer count x is log r + sum_{i=1}^{x-1} log1p((r - 1) / (i + 1)): terms of one
    sign, no difference of two values of size x log x (scipy.special.gammaln serves the non-integer x);
  * log(th + e) - log(th + mu + e) = -log1p(mu / (th + e)) and log(mu + e) - log(th + mu + e) = -log1p(th / (mu + e)).
tests/test_plane_stat_host.py checks all of it against mpmath at 50 digits on the whole grid.

The kinds: 'nb', 'zinb' (planes: log total_count, logits[, gate]), 'nbd', 'zinbd' (planes: mean and dispersion pre-activations[, gate];
`direct`: the mean and the dispersion themselves, as SCVI hands them over), 'mse' (mean), 'bernoulli' (logits), 'normal' (loc, raw
scale; sigma = softplus(raw + softplus^-1(1))).  EPS = float32(1e-8) is part of the nbd / zinbd likelihood's definition.

THE BOUNDS.  u = 2^-24 (the unit roundoff of float32).  Element statistics: |got - ref| <= (K + c (|p0| + |p1| + |p2|)) u |ref|.
One float32 rounding (+, -, *, a correctly rounded /: hipcc's default) counts 1; a function good to 1 ulp counts 2: `expf` of the device
library (HIP math API documentation: 1 ulp), v_exp_f32, v_log_f32 and v_rcp_f32 (1 ulp of the base-2 function / the reciprocal, as
smx_device.h records; docs/LAB_NOTES.md has tools/ulp_probe.hip's measured 1.5e-7 for ln near 1 and 1.9e-6 = 32 u for ln(1 + e), the
rounding of 1 + e itself).  c: fexp(x) = v_exp_f32(x * log2(e)) rounds its argument (the rounded constant and the product: 2 |x| u in
the result); adding softplus^-1(1) to a pre-activation x rounds once (|x| u in the argument, at most |x| u in a softplus).

  building blocks                                                                    K    c
  fexp(x)           v_mul (in c), v_exp_f32 2                                        2    2
  sigmoidf(x)       fexp (halved by e / (1 + e)) 2, 1 + e 1, v_rcp 2, e * s 1        6    2
  softplus(x)       fexp 2, 1 + e 32 (LAB_NOTES), v_log 2, * ln 2 1, + max(x, 0) 1   38   2     (the series under e < 1/32 is smaller)
  softplus(x + c1)  the same, the sum x + c1 rounded                                 39   3
  pi                expf 2, 1 + e 1, / 1                                             4    0

  kind, statistic   formula (after the repair), operations                                         K     c
  nb mean           expf(p0) 2, expf(p1) 2, * 1                                                    5     0
  nb variance       mean 5, 1 + el (el 2, + 1) 3, * 1                                              9     0
  zinb mean         q = sigmoidf(-p2) 6, mc 5, * 1                                                 12    2
  zinb variance     q (vc + pi mc mc): max(vc 9, pi 4 + mc 5 + mc 5 + 2) 16, + 1, q 6, * 1          24    2
  nbd mean          softplus(p0)                                                                   38    2
  nbd variance      mu (1 + mu / th): mu 38, th 39, / 1, 1 + 1, mu 38, * 1                          118   4     (c: 2 + 2 on p0, 3 on p1)
  zinbd mean        q 6, mu 38, * 1                                                                45    2
  zinbd variance    max(vc 118, pi 4 + 2 mu 76 + 2) 118, + 1, q 6, * 1                             126   4
  nbd direct        mean exact; variance mu (1 + mu / th): / 1, + 1, * 1                           0/3   0
  zinbd direct      mean q 6, * 1; variance max(3, pi 4 + 2) 6, + 1, q 6, * 1                      7/14  2
  bernoulli mean    1 / (1 + expf(-l)): expf 2, + 1, / 1                                           4     0
  bernoulli var     sigmoidf(l) 6, sigmoidf(-l) 6, * 1                                             13    4
  normal            mean exact; variance sd sd: 2 x 39, * 1                                        0/79  6
  mse               mean exact, variance 0                                                         0     0
count_only drops the gate: 'zinb' takes the 'nb' rows, 'zinbd' the 'nbd' rows.

log_prob: |got - ref| <= sum_g b_g + gamma sum_g |v_g|, gamma = (ceil(G / 256) + 8) u (a thread's chain of ceil(G / 256) additions, the
six butterfly steps of wave_sum, the two LDS additions), b_g = `logprob_elem_bound`: the first-order float32 error of count_elem /
bernoulli_elem / normal_elem (smx_loss.h) term by term -- every term's operations counted as above and multiplied by the term's size, an
input's error carried through the exact derivative, the additions of a sum at one rounding of the sum of the terms' sizes each -- plus
lgammaf(x + 1) at 6 ulp = 12 u (the project has recorded no figure of its own for lgammaf; 6 ulp is what the CUDA programming guide's
table, which the HIP math reference follows, gives for it away from its negative zeros) with a floor of one u at lgamma's zeros x = 0
and x = 1."""
import numpy as np
from scipy.special import digamma, expit, gammaln

U = 2.0 ** -24
SOFTPLUS_INV_1 = float(np.log(np.expm1(1.0)))
EPS = float(np.float32(1e-8))
F32_MIN, F32_MAX = 2.0 ** -126, 2.0 ** 127
KINDS = ("nb", "zinb", "nbd", "zinbd", "mse", "bernoulli", "normal")
N_PLANES = dict(nb=2, zinb=3, nbd=2, zinbd=3, mse=1, bernoulli=1, normal=2)
G_GRID = 1030        # not a multiple of 4, more than four 256-gene tiles

GATE = (-40.0, -20.0, -8.0, -1.0, 0.0, 1.0, 4.0, 8.0, 12.0, 16.5, 17.0, 20.0, 40.0, 80.0)
AXES = dict(
    nb=((-46.0, -12.0, -2.0, 0.0, 3.0, 9.2), (-30.0, -5.0, 0.0, 0.7, 6.0, 30.0)),
    nbd=((-60.0, -20.0, -3.0, 0.0, 5.0, 40.0), (-60.0, -30.0, -10.0, -1.0, 0.0, 3.0, 10.0, 40.0)),
    bernoulli=((-80.0, -40.0, -17.0, -8.0, 0.0, 8.0, 16.5, 17.0, 40.0, 80.0),),
    normal=((-1e4, 0.0, 3.5, 1e4), (-30.0, -20.0, -1.0, 0.0, 5.0, 60.0)),   # (-30 stands for a listed -60, whose variance 2.4e-52 is no float32: every point of that value failed the grid condition; at -30 sigma^2 = 2.6e-26 and z^2 of the loc 1e4 stays finite)
    mse=((-1e4, -1.0, 0.0, 0.25, 3.5, 1e4),),
)
AXES["zinb"] = AXES["nb"] + (GATE,)
AXES["zinbd"] = AXES["nbd"] + (GATE,)
# SCVI ('zinbd', direct): the extremes sit in the dispersion and the gate planes; theta = exp(bias), so the dispersion axis is the bias
SCVI_AXES = (AXES["nbd"][1], GATE)
MODERATE = dict(nb=((0.5, -0.3), (1.2, 0.4), (-0.7, 0.1)), nbd=((0.3, 0.2), (1.5, -0.4), (-0.8, 0.6)), bernoulli=((0.3,), (-1.1,), (2.0,)),
                normal=((0.4, 0.2), (-1.3, -0.5), (2.2, 0.9)), mse=((0.4,), (-1.3,), (2.2,)))
MODERATE["zinb"] = tuple(p + (g,) for p, g in zip(MODERATE["nb"], (-0.5, 0.3, 1.1)))
MODERATE["zinbd"] = tuple(p + (g,) for p, g in zip(MODERATE["nbd"], (-0.5, 0.3, 1.1)))
CYCLE = (0.0, 1.0, 2.0, 12.0, 181.0, 1000.0, 10738.0)


def _f64(planes, exact=False):
  """the planes as float64: rounded to float32 first (what a kernel reads), or with `exact` as they are -- float64 values that a kernel only
  knows to a stated relative error (tests/scvi_head_ref.py: the rate and the dispersion the scVI head forms in registers)"""
  return [np.asarray(p, np.float64) if exact else np.asarray(p, np.float32).astype(np.float64) for p in planes]


def softplus(x):
  return np.logaddexp(0.0, x)


def is_zi(kind):
  return kind in ("zinb", "zinbd")


def base_kind(kind, count_only=False):
  """the kind whose formulas apply: count_only takes the zero-inflation wrapper off"""
  return {"zinb": "nb", "zinbd": "nbd"}.get(kind, kind) if count_only else kind


# ---- the statistics ----------------------------------------------------------------------------------------------------------------
def parts(kind, planes, direct=False):
  """dict of float64 arrays: mean and variance of the count (or Bernoulli / normal) part, the gate complement q = 1 - pi and pi
  (zero-inflated kinds), the dispersion (count kinds)"""
  p = _f64(planes)
  out = {}
  if kind == "mse":
    out.update(mc=p[0], vc=np.zeros_like(p[0]))
  elif kind == "bernoulli":
    out.update(mc=expit(p[0]), vc=expit(p[0]) * expit(-p[0]))
  elif kind == "normal":
    sd = softplus(p[1] + SOFTPLUS_INV_1)
    out.update(mc=p[0], vc=sd * sd, sd=sd)
  elif kind in ("nb", "zinb"):
    r, el = np.exp(p[0]), np.exp(p[1])
    out.update(mc=np.exp(p[0] + p[1]), vc=np.exp(p[0] + p[1]) * (1.0 + el), disp=r)
  else:
    mu, th = (p[0], p[1]) if direct else (softplus(p[0]), softplus(p[1] + SOFTPLUS_INV_1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
      out.update(mc=mu, vc=mu * (1.0 + mu / th), disp=th)
  if is_zi(kind):
    out.update(q=expit(-p[2]), pi=expit(p[2]))
  return out


def moments(kind, planes, direct=False, count_only=False):
  """(mean, variance), float64"""
  s = parts(kind, planes, direct)
  if is_zi(kind) and not count_only:
    return s["q"] * s["mc"], s["q"] * (s["vc"] + s["pi"] * s["mc"] * s["mc"])
  return s["mc"], s["vc"]


def log_binom(x, r):
  """lgamma(x + r) - lgamma(r) - lgamma(x + 1), x >= 0, r > 0 (see the module docstring)"""
  x, r = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(r, np.float64))
  out = np.zeros(x.shape)
  whole = x == np.floor(x)
  if (~whole).any():
    out[~whole] = gammaln(x[~whole] + r[~whole]) - gammaln(r[~whole]) - gammaln(x[~whole] + 1.0)
  for v in np.unique(x[whole]):
    if v < 1:
      continue
    at = whole & (x == v)
    i = np.arange(1, int(v), dtype=np.float64)
    out[at] = np.log(r[at]) + np.log1p((r[at][:, None] - 1.0) / (i[None, :] + 1.0)).sum(axis=1)
  return out


def log_prob_elem(kind, x, planes, direct=False, count_only=False, exact=False):
  """the per-element log-probability the kernels sum over the genes, float64 (count kinds: including - lgamma(x + 1);
  'mse': -(x - mean)^2 / G, G the last axis)"""
  p = _f64(planes, exact)
  x = np.broadcast_to(np.asarray(x, np.float64), np.broadcast_shapes(np.shape(x), p[0].shape))
  if kind == "mse":
    return -((x - p[0]) ** 2) / float(x.shape[-1])
  if kind == "bernoulli":
    return -x * softplus(-p[0]) - (1.0 - x) * softplus(p[0])
  if kind == "normal":
    sd = softplus(p[1] + SOFTPLUS_INV_1)
    z = (x - p[0]) / sd
    return -0.5 * z * z - np.log(sd) - 0.5 * np.log(2.0 * np.pi)
  if kind in ("nb", "zinb"):
    r = np.exp(p[0])
    ell = log_binom(x, r) - x * softplus(-p[1]) - r * softplus(p[1])
  else:
    mu, th = (p[0], p[1]) if direct else (softplus(p[0]), softplus(p[1] + SOFTPLUS_INV_1))
    ell = log_binom(x, th) - th * np.log1p(mu / (th + EPS)) - x * np.log1p(th / (mu + EPS))
  if is_zi(kind) and not count_only:
    with np.errstate(over="ignore"):
      t = expit(-p[2]) * np.expm1(ell)                      # (1 - pi) (exp(ell) - 1) in (-1, 0]
      zero = np.where(t > -0.5, np.log1p(np.maximum(t, -0.5)), np.logaddexp(p[2], ell) - softplus(p[2]))
    return np.where(x == 0, zero, ell - softplus(p[2]))
  return ell


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
def grid_points(kind, scvi=False):
  """[n, k] float32: the Cartesian product of the kind's axes in plane order (SCVI: dispersion bias x gate, two columns)"""
  axes = SCVI_AXES if scvi else AXES[kind]
  return np.stack([a.ravel() for a in np.meshgrid(*axes, indexing="ij")], axis=1).astype(np.float32)


def in_range(kind, planes, direct=False):
  """the grid condition: the reference mean, variance, gate complement and dispersion are normal float32 numbers in [2^-126, 2^127)
  (a quantity that is exactly 0 by definition -- the 'mse' variance -- or may have either sign -- a loc -- is held to the upper end)"""
  s = parts(kind, planes, direct)
  mean, var = moments(kind, planes, direct)
  ok = np.ones(mean.shape, bool)
  signed = kind in ("mse", "normal")
  for name, v in (("mean", mean), ("var", var), ("mc", s["mc"]), ("vc", s["vc"]), ("q", s.get("q")), ("disp", s.get("disp"))):
    if v is None:
      continue
    a = np.abs(v)
    lo = (a >= F32_MIN) | ((a == 0) & (signed and name in ("mean", "mc") or kind == "mse"))
    ok &= np.isfinite(a) & lo & (a < F32_MAX)
  return ok


def bias_grid(kind, G=G_GRID):
  """(bias [k, G] float32, n_grid, n_dropped): the kept grid points in genes [0, n_grid - n_dropped), moderate points behind them"""
  pts = grid_points(kind)
  keep = in_range(kind, list(pts.T))
  kept = pts[keep]
  pad = np.array(MODERATE[kind], np.float32)
  rows = [kept] + [pad[[i % len(pad)]] * np.float32(1.0 + 0.001 * (i // len(pad))) for i in range(G - len(kept))]
  out = np.concatenate(rows, axis=0).astype(np.float32)
  assert out.shape == (G, N_PLANES[kind]) and len(kept) < G
  return np.ascontiguousarray(out.T), len(pts), int((~keep).sum())


def targets(kind, G=G_GRID, seed=5):
  """[5, G] float32 target rows: all zeros, all ones, CYCLE over the genes, the cycle shifted by three, a Poisson(1) row -- counts for
  the count kinds, {0, 1} for 'bernoulli', reals for 'normal' and 'mse'"""
  cyc = np.array(CYCLE)
  g = np.arange(G)
  t = np.stack([np.zeros(G), np.ones(G), cyc[g % 7], cyc[(g + 3) % 7], np.random.default_rng(seed).poisson(1.0, G).astype(np.float64)])
  if kind == "bernoulli":
    t = np.minimum(t, 1.0)
  elif kind in ("normal", "mse"):
    t[2:] = t[2:] * 0.731 - 2.5
  return t.astype(np.float32)


# ---- the bounds --------------------------------------------------------------------------------------------------------------------
_KC = {   # (kind, direct) -> ((K_mean, c_mean), (K_var, c_var)): the docstring's table
    ("nb", False): ((5, 0), (9, 0)), ("zinb", False): ((12, 2), (24, 2)),
    ("nbd", False): ((38, 2), (118, 4)), ("zinbd", False): ((45, 2), (126, 4)),
    ("nbd", True): ((0, 0), (3, 0)), ("zinbd", True): ((7, 2), (14, 2)),
    ("bernoulli", False): ((4, 0), (13, 4)), ("normal", False): ((0, 0), (79, 6)), ("mse", False): ((0, 0), (0, 0)),
}


def stat_bound(kind, stat, planes, direct=False, count_only=False):
  """the relative bound (K + c (|p0| + |p1| + |p2|)) 2^-24 of `stat` ('mean' | 'variance') per element.  In the direct interpretation the
  count planes are no pre-activations and enter no exponential: only the gate counts in the sum."""
  p = _f64(planes)
  K, c = _KC[(base_kind(kind, count_only), bool(direct) and kind in ("nbd", "zinbd"))][0 if stat == "mean" else 1]
  mag = sum(np.abs(v) for v in (p[2:] if direct else p))
  return (K + c * mag) * U


def _sp_abs(x):
  """softplus(x) as smx_device.h evaluates it: absolute error in u -- the closing sum max(x, 0) + log1p(e) where x > 0, and the log1p
  part at 37 + 2 |x| of its own size"""
  return np.where(x > 0, softplus(x), 0.0) + softplus(-np.abs(x)) * (37.0 + 2.0 * np.abs(x))


def _log1p_abs(ratio, rel):
  """log1p_small(ratio) of a ratio good to `rel` u: absolute error in u (series below 1/32: 3 roundings that count; above: 1 + ratio
  rounded, v_log and the scaling 3)"""
  l = np.log1p(ratio)
  return np.where(ratio < 0.03125, (rel + 3.0) * l, 1.0 + rel * ratio / (1.0 + ratio) + 3.0 * l)


def _lgdiff_abs(x, r, rel_r):
  """lgamma_digamma_diff(x, r).lg of an r good to `rel_r` u: absolute error in u.  r's error goes through the exact derivative
  r (digamma(x + r) - digamma(r)).  x <= 8 (integer, r < 1e4): the product of x factors r + i, two roundings each, and v_log with its
  scaling (3).  Otherwise the shifted Stirling form: A = x log(zr), B = (rs - 1/2) log1p(x / rs), -x, the difference of the two
  corrections and the shift log(num) - log(den), the five added at one rounding of the sum of their sizes each."""
  x, r = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(r, np.float64))
  with np.errstate(invalid="ignore", divide="ignore"):
    lg = np.where(x > 0, gammaln(x + r) - gammaln(r), 0.0)
    carried = rel_r * np.where(x > 0, np.abs(r * (digamma(x + r) - digamma(r))), 0.0)
  small = (x <= 8) & (x == np.floor(x)) & (r < 1e4)
  e_small = 2.0 * x + 3.0 * np.abs(lg)
  nf = np.maximum(np.ceil(4.0 - r), 0.0)
  i = np.arange(4.0).reshape((4,) + (1,) * x.ndim)
  on = i < nf
  lnum = np.where(on, np.log(r + i), 0.0).sum(axis=0)
  lden = np.where(on, np.log(x + r + i), 0.0).sum(axis=0)
  rs = r + nf
  zr = x + rs
  A = x * np.log(zr)
  l1p = np.log1p(x / rs)
  B = (rs - 0.5) * l1p
  corr = lambda z: 1.0 / (12.0 * z)
  Dm = corr(zr) + corr(rs)
  E = np.abs(lnum) + np.abs(lden)
  e_big = (4.0 * np.abs(A) + x                                            # x * flog(zr); zr = x + rs rounded
           + np.abs(rs - 0.5) * _log1p_abs(x / rs, 3.0) + 2.0 * np.abs(B)
           + rs * np.abs(digamma(zr) - digamma(rs))                      # rs = r + nf rounded
           + 7.0 * Dm + 3.0 * E + 4.0 * nf + E
           + 4.0 * (np.abs(A) + np.abs(B) + x + Dm + E))
  return carried + np.where(small, e_small, e_big)


def logprob_elem_bound(kind, x, planes, direct=False, count_only=False, double_const=False, rel_in=None, exact=False):
  """b_g: the absolute float32 error bound of one element of the row sum (the module docstring), float64.  double_const: without the
  lgammaf(x + 1) term -- for the kernels that take the count constant of a row from a double-precision sum.  rel_in = (rel_mu, rel_th), `direct`
  only: the relative errors, in u, of the mean and the dispersion a kernel holds (None: exact inputs, 0)"""
  p = _f64(planes, exact)
  x = np.broadcast_to(np.asarray(x, np.float64), np.broadcast_shapes(np.shape(x), p[0].shape))
  v = np.abs(log_prob_elem(kind, x, planes, direct, count_only, exact))
  if kind == "mse":
    return 4.0 * v * U
  if kind == "bernoulli":
    return (np.abs(x * p[0]) + _sp_abs(p[0]) + v) * U
  if kind == "normal":
    sd = softplus(p[1] + SOFTPLUS_INV_1)
    rel_sd = 39.0 + 3.0 * np.abs(p[1])
    z2 = 0.5 * ((x - p[0]) / sd) ** 2
    t = (2.0 * (rel_sd + 4.0) + 1.0) * z2 + rel_sd + 3.0 * np.abs(np.log(sd)) + 1.0
    return (t + 2.0 * (z2 + np.abs(np.log(sd)) + 1.0)) * U
  if kind in ("nb", "zinb"):
    r, sp, rel_r = np.exp(p[0]), softplus(p[1]), 2.0 + 2.0 * np.abs(p[0])
    lg = np.where(x > 0, np.abs(gammaln(x + r) - gammaln(r)), 0.0)
    t2, t3 = np.abs(x * softplus(-p[1])), r * sp
    e = (_lgdiff_abs(x, r, rel_r) + x * (_sp_abs(p[1]) + softplus(-p[1])) + t2
         + (rel_r + 1.0) * t3 + r * _sp_abs(p[1]) + 2.0 * (lg + t2 + t3))
  else:
    if direct:
      mu, th = p[0], p[1]
      rel_mu, rel_th = (0.0, 0.0) if rel_in is None else rel_in
    else:
      mu, th = softplus(p[0]), softplus(p[1] + SOFTPLUS_INV_1)
      rel_mu, rel_th = 38.0 + 2.0 * np.abs(p[0]), 39.0 + 3.0 * np.abs(p[1])
    ratio = mu / (th + EPS)
    t1 = th * np.log1p(ratio)
    lt, lm = np.abs(np.log(th + mu + EPS)), np.abs(np.log(mu + EPS))
    t2 = np.abs(x * np.log1p(th / (mu + EPS)))
    lg = np.where(x > 0, np.abs(gammaln(x + th) - gammaln(th)), 0.0)
    e = (th * _log1p_abs(ratio, rel_mu + rel_th + 4.0) + (rel_th + 1.0) * t1
         + x * ((np.maximum(rel_mu, rel_th) + 2.0 + 3.0 * lt) + (rel_mu + 1.0 + 3.0 * lm) + np.abs(np.log1p(th / (mu + EPS)))) + t2
         + _lgdiff_abs(x, np.clip(th, 1e-30, 1e30), rel_th) + 2.0 * (t1 + t2 + lg))
  if is_zi(kind) and not count_only:
    g = p[2]
    spg = softplus(g)
    ellv = log_prob_elem(base_kind(kind, True), x, planes[:2], direct, exact=exact) + gammaln(x + 1.0)   # (the kernel's ell has no count constant)
    dlt = np.abs(ellv - g)
    w3 = expit(-dlt)                                                       # e3 / (1 + e3)
    lse = np.abs(np.logaddexp(g, ellv))
    zero = e + (dlt + 2.0 + 2.0 * dlt) * w3 + 35.0 * softplus(-dlt) + lse + _sp_abs(g) + np.abs(lse - spg)
    other = e + _sp_abs(g) + np.abs(ellv - spg)
    e = np.where(x == 0, zero, other)
  lgx = np.abs(gammaln(x + 1.0))
  return (e + (0.0 if double_const else np.maximum(12.0 * lgx, 1.0)) + v) * U


def gamma_sum(G):
  return (np.ceil(G / 256.0) + 8.0) * U


def logprob_bound(kind, x, planes, direct=False, count_only=False):
  """the absolute bound of a row's log_prob: sum_g b_g + gamma sum_g |v_g| over the last axis"""
  b = logprob_elem_bound(kind, x, planes, direct, count_only)
  v = np.abs(log_prob_elem(kind, x, planes, direct, count_only))
  return b.sum(axis=-1) + gamma_sum(b.shape[-1]) * v.sum(axis=-1)
