"""float64 reference of the gradients of the elementwise likelihoods (count_elem / count_elem_vec, bernoulli_elem and normal_elem of
sisua_amd/csrc/smx_loss.h) wrt their parameter planes, and the float32 error bounds of the kernels' formulas.  The values, the edge
grid, the counts and the log-probability bounds are those of tests/plane_stat_ref.py, imported; this module adds the derivatives.

NumPy float64 only, an independent restatement in well-conditioned forms:
  * digamma(x + r) - digamma(r) of an integer count x is sum_{i<x} 1 / (r + i), its r-derivative -sum 1 / (r + i)^2: terms of one sign
    (scipy's digamma / polygamma serve a non-integer x);
  * x - sigmoid(l) of the Bernoulli is x sigmoid(-l) - (1 - x) sigmoid(l); x - (x + r) sigmoid(l) is x sigmoid(-l) - r sigmoid(l);
  * the zero-inflated zero branch: w = sigmoid(ell - g) = expit(ell - g), 1 - w = expit(g - ell), never 1 - expit(...), and
    d2 = (1 - w) - sigmoid(g) = expit(g - ell) expit(-g) (-expm1(ell)): three factors of one sign (sigma(a) - sigma(b) =
    sigma(a) sigma(-b) (1 - e^(b - a)), a = g - ell, b = g);
  * x / (mu + e) - x / (th + mu + e) of the 'nbd' mean gradient is x th / ((mu + e) (th + mu + e)).
What is left as a sum of terms of both signs -- r (dg - sp), the four terms of the 'nbd' dispersion gradient -- is a sum in the
definition; float64 carries it 2^29 times finer than the float32 bound, which is in the same term sizes.
tests/test_likelihood_grad_host.py checks all of it against mpmath on the whole grid.

THE BOUNDS.  u = 2^-24, operation counts as in plane_stat_ref's docstring (a rounding 1, v_exp / v_log / v_rcp 2, fexp's argument
2 |x| u), and its building blocks: r = fexp(p0) good to rel_r = 2 + 2 |p0|; softplus absolute `_sp_abs`; sigmoid of softplus_sigmoid good to
6 + 2 |x| relative (7 + 3 |x| with softplus^-1(1) added first); mu, th good to 38 + 2 |p0|, 39 + 3 |p1| relative (0 where `direct`).
Under `direct` a caller whose kernel formed the mean and the dispersion itself (the scVI head: tests/scvi_head_ref.py) passes their
relative errors as rel_in = (rel_mu, rel_th) and the float64 planes with exact=True; the default is 0 and float32 planes, as before.
Every bound is ABSOLUTE and in term sizes: sum over the terms of (operations of the term) x |term|, plus every input's relative
error times |input x exact partial derivative| (the partials are written out below), plus one rounding of the sum of the sizes per
addition.  Nothing is relative to the result: d1 = x - (x + r) sg and d2 at x = 0 are differences of near-equal numbers.

  quantity                      formula in count_elem, operations                                              bound (in u)
  dg, x <= 8 integer            dP / P by the recurrence: per step t = r + i 1, P t 1, fma 1; rcp 2, * 1       (5 x + 3) dg
  dg, Stirling                  l1p = log1p_small(x rcp(rs)): rs 1, rcp 2, * 1 -> _log1p_abs(x / rs, 4);       E_l1p + 9 (|c(zr)| + |c(rs)|) + 1.1
                                c(z) = digamma_corr: z 2, rcp 2, Horner 4, the difference 1 -> 9; truncation     + 12 shift + 2 (l1p + |c(zr)| + |c(rs)| + shift)
                                1 / (240 z^8) <= 1.1 u at z >= 4; shift = sum x rcp(b) rcp(a): 8 per term + 4
  dg, input r                   rel_r r |dg'|,  dg' = -sum_{i<x} 1 / (r + i)^2
  nb d0 = r (dg - sp)           E_dg, E_sp = _sp_abs(p1), the difference 1, the product 1, r's error through       r (E_dg + E_sp + dg + sp) + (rel_r + 1) |d0|
                                d d0 / d r = (dg - sp) + r dg'  (the second part is inside E_dg)
  nb d1 = x - (x + r) sg        x + r 1, sg 6 + 2 |p1|, * 1, the difference 1 of (x + (x + r) sg); r through sg      (8 + 2 |p1|) (x + r) sg + rel_r r sg + x + (x + r) sg
  nbd S = -th/T + x/(mu+e)      T = th + mu + e 2, rcp 2, * 1 -> 5 on th / T and on x / T; mu + e 1, rcp 2, * 1      5 th/T + 4 x/(mu+e) + 5 x/T + 2 (th/T + x/(mu+e) + x/T)
        - x/T                   -> 4; two additions of the three sizes; inputs through                               + rel_mu mu |dS/dmu| + rel_th th |dS/dth|
                                dS/dmu = th / T^2 - x th (T + mu + e) / ((mu + e)^2 T^2),  dS/dth = (x - mu - e) / T^2
  nbd d0 = S g0                 g0 = sigmoid(p0) 6 + 2 |p0|, * 1                                                     E_S g0 + (7 + 2 |p0|) |d0|
  nbd Q = -l1p + th mu/((th+e)T) l1p = log1p_small(mu rcp(th + e)): + 1, rcp 2, * 1 -> _log1p_abs(ratio, 4);         E_l1p + 10 t2 + 5 x/T + E_dg + 3 (l1p + t2 + x/T + dg)
        - x/T + dg              t2: rcp(th+e) 3, rcp(T) 4, three products 3 -> 10; x / T 5; three additions;         + rel_mu mu |dQ/dmu| + rel_th th (|dQ/dth| + |dg'|)
                                dQ/dmu = (x - mu - e) / T^2,  dQ/dth = mu / ((th+e) T) + mu (e T - th (th+e)) / ((th+e)^2 T^2) + x / T^2 (+ dg')
  nbd d1 = Q g1                 g1 = sigmoid(p1 + c1) 7 + 3 |p1|, * 1                                                E_Q g1 + (8 + 3 |p1|) |d1|
  zi, x = 0: dlt = ell - g      E_ell (the x = 0 row of logprob_elem_bound: nb (rel_r + 1) r sp + r E_sp; nbd            E_dlt = E_ell + |dlt|
                                th _log1p_abs(ratio, rel_mu + rel_th + 4) + (rel_th + 1) th l1p), the difference 1
  w, 1 - w                      e3 = fexp(-|dlt|): 2 + 2 |dlt| and E_dlt in the exponent; 1 + e3 1, rcp 2, e3 inv3 1;      E_w = 4 w + w (1 - w) (2 + 2 |dlt| + E_dlt)
                                the exponent's error through d w / d dlt = w (1 - w); 1 - w is the OTHER branch of    E_omw = 4 (1 - w) + w (1 - w) (2 + 2 |dlt| + E_dlt)
                                the same quotient (e3 inv3 where w = inv3 and the reverse): no subtraction from 1
  zi d0, d1 at x = 0            d w: one product; a w below 2^-126 (the gate 87 or more above ell) comes out of v_exp      E_d w + |d| E_w + |d w| + 2^-126 |d| / u
                                as 0: an absolute error of 2^-126 in w
  every component               the result's own underflow                                                           + 2^-126 / u
  zi d2 at x = 0 = omw - sg     sg = sigmoid(g) 6 + 2 |g|, the difference 1                                          E_omw + (6 + 2 |g|) sg + (omw + sg)
  zi d2 at x > 0 = -sg                                                                                               (6 + 2 |g|) sg
  bernoulli d0 = x - sg         sg 6 + 2 |l|, the difference 1                                                       (6 + 2 |l|) sg + x + sg
  normal d0 = zz inv            inv = rcp(sd): rel_sd + 2; zz = (x - m) inv: 1 + 1 -> rel_zz = rel_sd + 4             (2 rel_sd + 7) |d0|
  normal d1 = (zz^2 - 1) inv sg zz^2: 2 rel_zz + 1; the difference 1 of (z^2 + 1); inv rel_sd + 2, sg 7 + 3 |p1|,      ((2 rel_zz + 2) z^2 + 1) sg / sd + (rel_sd + 11 + 3 |p1|) |d1|
                                two products
The zero branch's row "1 - w is the other branch" is the formula AFTER the repair this module's tests led to: count_elem formed
(1.f - w), which carries w's absolute error 4 u w ~ 4 u into a term of size 1 - w ~ e^(g - ell) (4e-18 at a gate of -40): outside this
bound wherever the gate sits 17 or more below ell.  DESIGN.md 4s has the figures.

THE GRID CONDITION (`grad_in_range`), per element: the intermediates whose RELATIVE error the table uses -- r / mu / th, the
sigmoids, dg, S and Q, 1 / (mu + e) and 1 / T, and at a zero count of a zero-inflated kind 1 - w -- are normal float32 numbers
(2^-126 <= |v| < 2^127) or exactly 0 where the definition makes them 0 (dg at x = 0, S at x = mu + e), and the reference gradients
are below 2^127.  A RESULT below 2^-126 -- a product S g0 or d w, a difference omw - sg, and w itself, which v_exp returns as 0 once
the gate sits 87 above ell -- is no reason to drop the element: every bound carries the absolute term 2^-126 (1 + |d|), the
underflow of the product.  (Dropping them instead would take a fifth of the 'zinb' points' zero counts off the grid.)  No axis value
fails wholesale but one: GRAD_AXES is plane_stat_ref's AXES with the 'normal' raw scale -30 replaced by -22 (the note beside it)."""
import numpy as np
from scipy.special import digamma, expit, gammaln, polygamma

from tests.plane_stat_ref import (AXES, CYCLE, EPS, F32_MAX, F32_MIN, GATE, MODERATE, SOFTPLUS_INV_1, U, _f64, _log1p_abs, _sp_abs,  # noqa: F401
                                  G_GRID, base_kind, bias_grid, grid_points, in_range, is_zi, log_prob_elem, logprob_elem_bound, softplus, targets)

GRAD_KINDS = ("nb", "zinb", "nbd", "zinbd", "bernoulli", "normal")
FLUSH = F32_MIN / U    # 2^-126 in units of u
GRAD_AXES = dict(AXES)
# ('normal', raw scale: -22 stands for plane_stat_ref's -30, at which every point failed the grid condition -- sigma = 1.6e-13 puts the
# intermediate (z^2 - 1) / sigma of normal_elem's d1 past 2^127 for every loc and every x of the grid, 1.5e39 at the least; at -22
# sigma = 4.8e-10 and the same intermediate is 9e35 at the loc 1e4)
GRAD_AXES["normal"] = (AXES["normal"][0], tuple(-22.0 if v == -30.0 else v for v in AXES["normal"][1]))
ALL = [(k, False) for k in GRAD_KINDS] + [("nbd", True), ("zinbd", True)]


def _sum_over_count(x, r, f):
  """sum_{i < x} f(r + i) for integer x, elementwise (x and r broadcast alike), in blocks of 512 terms"""
  out = np.zeros(x.shape)
  for v in np.unique(x):
    if v < 1:
      continue
    at = x == v
    ra = r[at][:, None]
    acc = np.zeros(ra.shape[0])
    for i0 in range(0, int(v), 512):
      i = np.arange(i0, min(i0 + 512, int(v)), dtype=np.float64)[None, :]
      acc += f(ra + i).sum(axis=1)
    out[at] = acc
  return out


def digamma_diff(x, r):
  """(dg, dg'): digamma(x + r) - digamma(r) >= 0 and its r-derivative <= 0, x >= 0, r > 0"""
  x, r = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(r, np.float64))
  whole = x == np.floor(x)
  dg = _sum_over_count(np.where(whole, x, 0.0), r, lambda t: 1.0 / t)
  dp = -_sum_over_count(np.where(whole, x, 0.0), r, lambda t: 1.0 / (t * t))
  if (~whole).any():
    dg[~whole] = digamma(x[~whole] + r[~whole]) - digamma(r[~whole])
    dp[~whole] = polygamma(1, x[~whole] + r[~whole]) - polygamma(1, r[~whole])
  return dg, dp


def _xb(x, p):
  return np.broadcast_to(np.asarray(x, np.float64), np.broadcast_shapes(np.shape(x), p[0].shape))


def _bc(p, shape):
  return [np.broadcast_to(v, shape) for v in p]


def _nbd_inputs(p, direct, rel_in=None):
  """mu, th, g0, g1 and their relative float32 errors in u.  rel_in = (rel_mu, rel_th), `direct` only: the errors of a mean and a dispersion
  that the kernel formed itself (None: exact inputs, 0)"""
  if direct:
    one = np.ones_like(p[0])
    if rel_in is None:
      return p[0], p[1], one, one, 0.0 * one, 0.0 * one, 0.0 * one, 0.0 * one
    return p[0], p[1], one, one, rel_in[0] + 0.0 * one, rel_in[1] + 0.0 * one, 0.0 * one, 0.0 * one
  mu, th = softplus(p[0]), softplus(p[1] + SOFTPLUS_INV_1)
  return (mu, th, expit(p[0]), expit(p[1] + SOFTPLUS_INV_1), 38.0 + 2.0 * np.abs(p[0]), 39.0 + 3.0 * np.abs(p[1]),
          6.0 + 2.0 * np.abs(p[0]), 7.0 + 3.0 * np.abs(p[1]))


def count_terms(kind, x, planes, direct=False, rel_in=None, exact=False):
  """dict of float64 arrays: everything grad_elem, grad_elem_bound and grad_in_range share -- the count part's gradients d0c, d1c (before
  the zero branch scales them), their terms, ell at x = 0, w and 1 - w.  exact: the planes are float64 values, not rounded to float32 first
  (plane_stat_ref._f64); rel_in: _nbd_inputs"""
  p = _f64(planes, exact)
  x = _xb(x, p)
  p = _bc(p, x.shape)
  t = dict(x=x)
  base = base_kind(kind, True)
  if base == "nb":
    r, sp, sg = np.exp(p[0]), softplus(p[1]), expit(p[1])
    dg, dgp = digamma_diff(x, r)
    t.update(r=r, sp=sp, sg=sg, dg=dg, dgp=dgp, d0c=r * (dg - sp), d1c=x * expit(-p[1]) - r * sg, ell0=-r * sp)
  else:
    mu, th, g0, g1, rel_mu, rel_th, rel_g0, rel_g1 = _nbd_inputs(p, direct, rel_in)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
      T = th + mu + EPS
      dg, dgp = digamma_diff(x, np.clip(th, 1e-30, 1e30))
      a, b, c = th / T, x / (mu + EPS), x / T
      S = x * th / ((mu + EPS) * T) - a
      ratio = mu / (th + EPS)
      l1p, t2 = np.log1p(ratio), th * mu / ((th + EPS) * T)
      Q = -l1p + t2 - c + dg
      t.update(mu=mu, th=th, g0=g0, g1=g1, rel_mu=rel_mu, rel_th=rel_th, rel_g0=rel_g0, rel_g1=rel_g1, T=T, dg=dg, dgp=dgp, a=a, b=b, c=c,
               S=S, ratio=ratio, l1p=l1p, t2=t2, Q=Q, d0c=S * g0, d1c=Q * g1, ell0=-th * l1p,
               dS_dmu=th / T ** 2 - x * th * (T + mu + EPS) / ((mu + EPS) ** 2 * T ** 2), dS_dth=(x - mu - EPS) / T ** 2,
               dQ_dth=mu / ((th + EPS) * T) + mu * (EPS * T - th * (th + EPS)) / ((th + EPS) ** 2 * T ** 2) + x / T ** 2)
  if is_zi(kind):
    g = p[2]
    t.update(g=g, sgg=expit(g), w=expit(t["ell0"] - g), omw=expit(g - t["ell0"]))
  return t


def grad_elem(kind, x, planes, direct=False, exact=False):
  """[3, ...] float64: d log p / d p0, p1, p2 per element (0 where the kind has no such plane)"""
  p = _f64(planes, exact)
  x = _xb(x, p)
  p = _bc(p, x.shape)
  zero = np.zeros(x.shape)
  if kind == "bernoulli":
    return np.stack([x * expit(-p[0]) - (1.0 - x) * expit(p[0]), zero, zero])
  if kind == "normal":
    sd = softplus(p[1] + SOFTPLUS_INV_1)
    z = (x - p[0]) / sd
    with np.errstate(over="ignore"):
      return np.stack([z / sd, (z * z - 1.0) / sd * expit(p[1] + SOFTPLUS_INV_1), zero])
  t = count_terms(kind, x, planes, direct, exact=exact)
  if not is_zi(kind):
    return np.stack([t["d0c"], t["d1c"], zero])
  at0 = x == 0
  with np.errstate(over="ignore"):
    d2_zero = t["omw"] * expit(-t["g"]) * -np.expm1(t["ell0"])
  return np.stack([np.where(at0, t["d0c"] * t["w"], t["d0c"]), np.where(at0, t["d1c"] * t["w"], t["d1c"]), np.where(at0, d2_zero, -t["sgg"])])


# ---- the bounds --------------------------------------------------------------------------------------------------------------------
def _dgdiff_abs(x, r, dg):
  """lgamma_digamma_diff(x, r).dg of an exact r: absolute error in u (the docstring's first two rows; r's own error is the third)"""
  small = (x <= 8) & (x == np.floor(x)) & (r < 1e4)
  nf = np.maximum(np.ceil(4.0 - r), 0.0)
  i = np.arange(4.0).reshape((4,) + (1,) * x.ndim)
  on = i < nf
  with np.errstate(divide="ignore", invalid="ignore"):
    shift = np.where(on, x / ((x + r + i) * (r + i)), 0.0).sum(axis=0)
    rs = r + nf
    zr = x + rs
    l1p = np.log1p(x / rs)
    corr = lambda z: 0.5 / z + 1.0 / (12.0 * z * z)
    big = (_log1p_abs(x / rs, 4.0) + 9.0 * (corr(zr) + corr(rs)) + 1.1 + 12.0 * shift + 2.0 * (l1p + corr(zr) + corr(rs) + shift))
  return np.where(small, (5.0 * x + 3.0) * dg, big)


def grad_elem_bound(kind, x, planes, direct=False, rel_in=None, exact=False):
  """[3, ...] float64: the absolute first-order float32 bound of every gradient component (the module docstring's table).  rel_in =
  (rel_mu, rel_th) in u, `direct` only: the table's input-error terms for a mean and a dispersion the kernel formed itself (None: 0, the
  planes are the kernel's inputs)"""
  p = _f64(planes, exact)
  x = _xb(x, p)
  p = _bc(p, x.shape)
  zero = np.zeros(x.shape)
  if kind == "bernoulli":
    sg = expit(p[0])
    return np.stack([(6.0 + 2.0 * np.abs(p[0])) * sg + x + sg + FLUSH, zero, zero]) * U
  if kind == "normal":
    sd, sg = softplus(p[1] + SOFTPLUS_INV_1), expit(p[1] + SOFTPLUS_INV_1)
    rel_sd = 39.0 + 3.0 * np.abs(p[1])
    rel_zz = rel_sd + 4.0
    with np.errstate(over="ignore"):
      z = (x - p[0]) / sd
      d0, d1 = z / sd, (z * z - 1.0) / sd * sg
      return np.stack([(2.0 * rel_sd + 7.0) * np.abs(d0) + FLUSH,
                       ((2.0 * rel_zz + 2.0) * z * z + 1.0) * sg / sd + (rel_sd + 11.0 + 3.0 * np.abs(p[1])) * np.abs(d1) + FLUSH, zero]) * U
  t = count_terms(kind, x, planes, direct, rel_in, exact)
  with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
    if base_kind(kind, True) == "nb":
      r, sp, sg, dg = t["r"], t["sp"], t["sg"], t["dg"]
      rel_r = 2.0 + 2.0 * np.abs(p[0])
      e_dg = _dgdiff_abs(x, np.clip(r, 1e-30, 1e30), dg) + rel_r * r * np.abs(t["dgp"])
      e0 = r * (e_dg + _sp_abs(p[1]) + dg + sp) + (rel_r + 1.0) * np.abs(t["d0c"])
      e1 = (8.0 + 2.0 * np.abs(p[1])) * (x + r) * sg + rel_r * r * sg + x + (x + r) * sg
      e_ell = (rel_r + 1.0) * r * sp + r * _sp_abs(p[1])
    else:
      mu, th, a, b, c, dg = t["mu"], t["th"], t["a"], t["b"], t["c"], t["dg"]
      e_S = (5.0 * a + 4.0 * b + 5.0 * c + 2.0 * (a + b + c) + t["rel_mu"] * mu * np.abs(t["dS_dmu"]) + t["rel_th"] * th * np.abs(t["dS_dth"]))
      e0 = e_S * t["g0"] + (t["rel_g0"] + (0.0 if direct else 1.0)) * np.abs(t["d0c"])
      e_dg = _dgdiff_abs(x, np.clip(th, 1e-30, 1e30), dg)
      e_Q = (_log1p_abs(t["ratio"], 4.0) + 10.0 * t["t2"] + 5.0 * c + e_dg + 3.0 * (t["l1p"] + t["t2"] + c + dg)
             + t["rel_mu"] * mu * np.abs(t["dS_dth"]) + t["rel_th"] * th * (np.abs(t["dQ_dth"]) + np.abs(t["dgp"])))
      e1 = e_Q * t["g1"] + (t["rel_g1"] + (0.0 if direct else 1.0)) * np.abs(t["d1c"])
      e_ell = th * _log1p_abs(t["ratio"], t["rel_mu"] + t["rel_th"] + 4.0) + (t["rel_th"] + 1.0) * th * t["l1p"]
    if not is_zi(kind):
      return np.stack([e0 + FLUSH, e1 + FLUSH, zero]) * U
    g, w, omw, sgg = t["g"], t["w"], t["omw"], t["sgg"]
    dlt = np.abs(t["ell0"] - g)
    expo = w * omw * (2.0 + 2.0 * dlt + e_ell + dlt)
    e_w, e_omw = 4.0 * w + expo, 4.0 * omw + expo
    at0 = x == 0
    z0 = e0 * w + np.abs(t["d0c"]) * e_w + np.abs(t["d0c"] * w) + FLUSH * np.abs(t["d0c"])
    z1 = e1 * w + np.abs(t["d1c"]) * e_w + np.abs(t["d1c"] * w) + FLUSH * np.abs(t["d1c"])
    z2 = e_omw + (6.0 + 2.0 * np.abs(g)) * sgg + omw + sgg
    return (np.stack([np.where(at0, z0, e0), np.where(at0, z1, e1), np.where(at0, z2, (6.0 + 2.0 * np.abs(g)) * sgg)]) + FLUSH) * U


# ---- the grid condition --------------------------------------------------------------------------------------------------------------
def _normal32(v, zero_ok=False):
  a = np.abs(v)
  with np.errstate(invalid="ignore"):
    return np.isfinite(a) & (a < F32_MAX) & ((a >= F32_MIN) | (zero_ok & (a == 0)))


def _below_max(v):
  with np.errstate(invalid="ignore"):
    return np.isfinite(v) & (np.abs(v) < F32_MAX)


def grad_in_range(kind, x, planes, direct=False, exact=False):
  """the grid condition per element (the module docstring)"""
  p = _f64(planes, exact)
  x = _xb(x, p)
  g = grad_elem(kind, x, planes, direct, exact)
  ok = _below_max(g[0]) & _below_max(g[1]) & _below_max(g[2])
  if kind == "bernoulli":
    return ok & _normal32(expit(p[0] + 0.0 * x))
  if kind == "normal":
    sd = softplus(p[1] + SOFTPLUS_INV_1) + 0.0 * x
    with np.errstate(over="ignore"):
      z2 = ((x - p[0]) / sd) ** 2
      ok &= _normal32((z2 - 1.0) / sd)          # ((zz zz - 1) inv, formed before the product by sg)
    return ok & _normal32(sd) & _normal32(1.0 / sd) & _normal32(z2, True) & _normal32(expit(p[1] + SOFTPLUS_INV_1) + 0.0 * x)
  t = count_terms(kind, x, planes, direct, exact=exact)
  pos = x > 0
  ok &= _below_max(t["d0c"]) & _below_max(t["d1c"]) & _normal32(t["dg"], ~pos)
  if base_kind(kind, True) == "nb":
    names = ("r", "sp", "sg")
  else:
    names = ("mu", "th", "g0", "g1", "T", "S", "Q")
    ok &= _normal32(1.0 / (t["mu"] + EPS)) & _normal32(1.0 / t["T"])
  for n in names:
    ok &= _normal32(t[n], n in ("S", "Q"))
  if is_zi(kind):
    ok &= _normal32(t["sgg"]) & np.where(pos, True, _normal32(t["omw"]))
  return ok


def grad_points(kind):
  """[n, k] float32: the Cartesian product of GRAD_AXES[kind] in plane order, the points plane_stat_ref's own grid condition keeps"""
  pts = np.stack([a.ravel() for a in np.meshgrid(*GRAD_AXES[kind], indexing="ij")], axis=1).astype(np.float32)
  return pts[in_range(kind, list(pts.T))]


def grad_bias_grid(kind, G=G_GRID):
  """(bias [k, G] float32, n_points): `grad_points` in genes [0, n_points), plane_stat_ref.bias_grid's moderate filler behind them -- for
  every kind but 'normal' the array bias_grid returns"""
  kept = grad_points(kind)
  pad = np.array(MODERATE[kind], np.float32)
  rows = [kept] + [pad[[i % len(pad)]] * np.float32(1.0 + 0.001 * (i // len(pad))) for i in range(G - len(kept))]
  out = np.concatenate(rows, axis=0).astype(np.float32)
  assert out.shape == (G, len(GRAD_AXES[kind])) and len(kept) < G
  return np.ascontiguousarray(out.T), len(kept)


def grid_elements(kind, direct=False):
  """(x [n, 7], planes k x [n, 1], keep [n, 7]): the whole gradient grid of the kind (`direct`: the activated mean and dispersion of its
  points) x the seven counts, and the grid condition"""
  planes = list(grad_points(kind).T)
  if direct:
    p = _f64(planes)
    planes = [softplus(p[0]).astype(np.float32), softplus(p[1] + SOFTPLUS_INV_1).astype(np.float32)] + planes[2:]
  x = counts_for(kind)[None, :] + np.zeros((len(planes[0]), 1), np.float32)
  planes = [np.ascontiguousarray(pl[:, None]) for pl in planes]
  return x, planes, grad_in_range(kind, x, planes, direct)


def counts_for(kind):
  """the seven values of x every grid point is taken at: CYCLE for the count kinds, {0, 1} for 'bernoulli', reals for 'normal' (the map of
  plane_stat_ref.targets)"""
  c = np.array(CYCLE)
  if kind == "bernoulli":
    c = np.minimum(c, 1.0)
  elif kind == "normal":
    c = c * 0.731 - 2.5
  return c.astype(np.float32)


# ---- sums over the genes (the summation bound of tests/test_gpu_likelihood_grid.py's docstring) -----------------------------------------
def count_const(kind, x):
  """lgamma(x + 1) per element: what count_elem leaves to the caller (0 for 'bernoulli' / 'normal')"""
  return gammaln(np.asarray(x, np.float64) + 1.0) if kind not in ("bernoulli", "normal") else np.zeros(np.shape(x))


def row_sum_bound(kind, x, planes, n_add, direct=False, count_only=False, double_const=True, repeat=1, rel_in=None, exact=False):
  """(ref, bound) of the sum over the last axis, every element taken `repeat` times (rel_in, exact: logprob_elem_bound's)"""
  v = log_prob_elem(kind, x, planes, direct, count_only, exact)
  b = logprob_elem_bound(kind, x, planes, direct, count_only, double_const=double_const, rel_in=rel_in, exact=exact)
  s = np.abs(v + count_const(kind, np.broadcast_to(x, v.shape)))
  ref = repeat * v.sum(axis=-1)
  return ref, repeat * (b.sum(axis=-1) + (n_add + 8.0) * U * s.sum(axis=-1) + v.shape[-1] * F32_MIN) + U * np.abs(ref)


def draw_bound(kind, t, planes, count_only, n_add):
  """(ref, bound) [rows] of one draw's log-likelihood per cell: the summation bound, and 2 u |sum lgamma(x + 1)| for the cell's count constant,
  a float32 (of a double sum) that one float32 subtraction takes off"""
  ref, bound = row_sum_bound(kind, t, planes, n_add, count_only=count_only)
  return ref, bound + 2.0 * U * count_const(kind, t).sum(axis=-1)
