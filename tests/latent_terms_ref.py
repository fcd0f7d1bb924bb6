"""float64 reference of the latent heads' terms of the ELBO and of the importance weight -- the diagonal head (latent_fwd_quad_kernel,
latent_fwd_kernel, the FRONT preload of bn_act_fwd_body; latent_bwd_kernel, gemm_latent_bwd_kernel's epilogue, fold_dz_tile;
iw_accum_kernel, score_draws_kernel, the one-launch decoder), scVI's library latent (lib_latent_fwd / bwd_kernel, the fused copies of
smx_scvi.hip) and the full-covariance head (latent_tril_fwd / bwd_kernel) --, the float32 error bounds of the kernels' formulas, and a
float32 NumPy replay of the kernels' lines.  The pattern is tests/likelihood_grad_ref.py's.

NumPy float64 only, in well-conditioned forms.  x = raw + log(e - 1) (exact in float64 for a float32 raw of the grid);
  sigma = softplus(x) = logaddexp(0, x);   log sigma = x + log1p(-t / 2 + t^2 / 3), t = e^x, below x = -30 (sigma = t (1 - t / 2 + t^2 / 3 - ...):
  no logarithm of a number that float64 could underflow), log(softplus(x)) above;
  dKL / draw = (sigma - 1 / sigma) expit(x): 1 / sigma = 1.6e43 at the grid's lowest raw scale is an ordinary float64.
What is left as a sum of terms of both signs -- sigma^2 + mu^2 - 1 - 2 log sigma near the prior, a cancellation to 4e-7 at raw = 1e-3 -- is a
sum in the definition; float64 carries it 2^29 times finer than the float32 bound, which is in the same term sizes.
tests/test_latent_terms_host.py checks all of it against mpmath on the whole grid.

THE BOUNDS.  u = 2^-24; every bound is ABSOLUTE and in term sizes, by the rule of likelihood_grad_ref: sum over the terms of (operations
of the term) x |term|, plus every input's error times |exact partial derivative|, plus one rounding of the running sum of sizes per
addition, plus 2^-126 for the result's (and sigma's) underflow.  Operation counts: a rounding 1; v_exp / v_log / v_rcp / v_sqrt 2 (the "~1 ulp
of the base-2 function" of smx_device.h, and its scaling), logf / sqrtf / a division 2 and 1; fexp's argument 2 |x| u (inside _sp_abs and the
sigmoid's 7 + 3 |x|, plane_stat_ref's and likelihood_grad_ref's figures).

  quantity                      formula in the kernels, operations                                              bound (in u)
  x = raw + c                   one rounding                                                                    |x|
  sigma                         latent_sigma(x) = max(softplusf(x), 2^-126): _sp_abs(x); x's rounding through       E_s = _sp_abs(x) + |x| expit(x)  (+ 2^-126 / u where sigma < 2^-126)
                                expit(x); where sigma itself is below 2^-126 (v_exp returns 0 there, the clamp
                                2^-126) an absolute 2^-126
  z = mu + sigma eps            the product 1, the sum 1 (or one fma); sigma's error times |eps|                    E_z = E_s |eps| + |sigma eps| + |z|
  log sigma, x >= -20           flog: v_log and its scaling 3 (logf: 2); sigma's error / sigma                      E_l = 3 |log sigma| + E_s / sigma
  log sigma, x < -20            x itself (SMX_SIGMA_TAIL): its rounding; the truncation e^-20 / 2 = 1e-9 = 0.02 u     E_l = |x| + 0.02
  KL element                    0.5 (A + B - 1 - C), A = sigma^2: 2 E_s sigma + A; B = mu^2: B; C = 2 log sigma:    0.5 (2 E_s sigma + A + B + 2 E_l + 3 (A + B + 1 + |C|))
                                2 E_l; three additions of the sizes A + B + 1 + |C|; the halving is exact
  dKL / dmu                     mu (the kernel forms kls mu: in the test's bound)                                    0
  dKL / draw, raw >= -87        (sigma - rcp(sigma)) sgm: E_s; rcp 2 and E_s / sigma on 1 / sigma; the difference   (E_s + (2 + E_s / sigma) / sigma + sigma + 1 / sigma) sgm
    (DRAW_FLOOR)                1 of the sizes; sgm = sigmoidf(x) 7 + 3 |x| relative, the product 1                   + (8 + 3 |x|) |d|
  dKL / draw, raw < -87         the training step's backward forms are left as they were (the floor):  no bound; no NaN
                                sgm comes out of v_exp as 0 and the result is 0 x (2^-126 - 2^126) = -0, not -1
  weight term                   -0.5 z z + 0.5 eps eps + log sigma: z z 1 and 2 E_z |z| halved; eps eps 1; logf      E_z |z| + 0.5 z^2 + 0.5 eps^2 + E_l'
                                (E_l' = E_l with 2 for 3); two additions of the sizes                                + 2 (0.5 z^2 + 0.5 eps^2 + |log sigma|)
  scVI, library latent          sp = sqrtf(vp) 2; log(sp / sigma): the ratio 1 + 2 + E_s / sigma relative, logf 2   2 |log(sp / sigma)| + 3 + E_s / sigma  (tail: 3 |log sp| + 2 + 2 |x| + 0.02)
  KL_l = log(sp / sigma)        Q = (sigma^2 + d^2) / (2 vp), d = mu - mp: d 1, d^2 3 d^2, sigma^2 as A, the sum 1,   + (2 E_s sigma + 2 sigma^2 + 4 d^2) / (2 vp) + Q
    + Q - 0.5                   the division 1; two additions of the sizes                                          + 2 (|log(sp / sigma)| + Q + 0.5)
  dKL_l / dmu = d / vp          d 1, the division 1                                                                  2 |d / vp|
  dKL_l / draw, x < -20         -1 (SMX_SIGMA_TAIL, lib_dsraw): the truncation 0.02; nothing is computed             0.02
  dKL_l / draw, x >= -20        (sigma / vp - 1 / sigma) sgm in divisions (1 each), the difference 1, sgm, product   ((E_s + sigma) / vp + (1 + E_s / sigma) / sigma + sigma / vp + 1 / sigma) sgm + (8 + 3 |x|) |d|
  library weight term           -0.5 d d / vp - 0.5 logf(vp) + 0.5 eps eps + log sigma, d = l - mp: E_d = E_z + |d|;  E_d |d| / vp + 2 T1 + 2 T2 + T3 + E_l' + 3 (T1 + T2 + T3 + |log sigma|)
                                T1 = d^2 / (2 vp), T2 = |log vp| / 2, T3 = eps^2 / 2
  tril: L_ii                    softplusf(raw_ii) + 1e-5: _sp_abs, the sum 1                                       E_L = _sp_abs(raw_ii) + L_ii
  tril: z_i                     mu + acc + L_ii eps_i, acc = sum_{j<i} raw_ij eps_j by i fmas (one rounding of the   i sum |raw_ij eps_j| + E_L |eps_i| + 3 (|mu| + sum |raw_ij eps_j| + |L_ii eps_i|)
                                running sum each); three more roundings of the sizes
  tril: KL row i                0.5 (fro + L_ii^2 + mu^2 - 1) - flog(L_ii), fro = sum_{j<i} raw_ij^2 by i fmas       0.5 ((i + 1) fro + 2 E_L L_ii + L_ii^2 + mu^2 + 3 S) + 3 |log L_ii| + E_L / L_ii + 0.5 S + |log L_ii|,
                                                                                                                     S = fro + L_ii^2 + mu^2 + 1
  tril: dKL / draw_ii           (L_ii - rcp(L_ii)) sg, sg of softplus_sigmoid(raw_ii) 6 + 2 |raw_ii|               (E_L + (2 + E_L / L_ii) / L_ii + L_ii + 1 / L_ii) sg + (7 + 2 |raw_ii|) |d|
                                sg below 2^-126 (raw_ii under -87.3) comes out of v_exp as 0: 2^-126 times the factor  + 2^-126 (L_ii + 1 / L_ii) / u
  tril: dKL / draw_ij, dmu      raw_ij, mu                                                                           0
  every component               the result's own underflow                                                           + 2^-126 / u
A sum over the latent dimensions adds, in the tests, one rounding of the running sum of sizes per addition of the kernel's reduction.

THE REPAIR this module's tests led to.  Below x = -87.3 sigma is a denormal or 0: flog / logf of it is -inf, rcp of it +inf,
and the KL, the scale's gradient ((-inf) x 0) and the importance weight were inf / NaN / -inf where their values are 87, -1 and -87.  The rows
"x < -20" are the formulas after the repair: log sigma = x (and, in the library latent, (sigma / vp - 1 / sigma) sigmoid(x) = -1) far down
sigma's tail, the ordinary branch spelled as before; sigma itself is kept at 2^-126 or above.  The diagonal head's scale gradient inside a
training step keeps its lines and a FLOOR at raw = -87 (DRAW_FLOOR), below which it is only held to "no NaN".  `Replay.diag(...,
repaired=False)` keeps the old lines.

KEPT POINTS: the float64 value of the checked quantity is finite and below 2^127 in magnitude.  On the grid below every point of the
diagonal and the tril head is kept (mu^2 = 1e38 at the location 1e19 is below 2^127 = 1.7e38; sigma^2 = 1e8 at the raw scale 1e4); the library
latent drops its KL and weight term at the locations +-1e19 under the prior (7, 1e-6) (tests/test_latent_terms_host.py counts them)."""
import numpy as np
from scipy.special import expit

from tests.plane_stat_ref import F32_MAX, F32_MIN, SOFTPLUS_INV_1, U, _sp_abs, softplus

FLUSH = F32_MIN / U     # 2^-126 in units of u
TAIL = -20.0            # SMX_SIGMA_TAIL
TRIL_SHIFT = 1e-5
DRAW_FLOOR = -87.0      # the smallest raw scale at which the diagonal head's scale gradient of a training step is inside its bound (the last normal sigma)
C1 = np.float32(SOFTPLUS_INV_1)

RAW_AXIS = (-100.0, -88.0, -87.0, -60.0, -30.0, -15.0, -8.0, -2.0, -1e-3, 0.0, 1e-3, 2.0, 10.0, 20.0, 88.0, 1e4)
LOC_AXIS = (0.0, 1e-20, -1e-20, 1e-3, -1e-3, 1.0, -1.0, 30.0, -30.0, 1e4, -1e4, 1e19, -1e19)
EPS_AXIS = (0.0, 1e-3, -1e-3, 1.0, -1.0, 5.5, -5.5)          # (5.77 is the largest normal4 draws from a 24-bit uniform)
LIB_PRIORS = ((7.0, 0.3), (7.0, 1e-6), (0.0, 1e4))           # (mp, vp); vp = 0 is no grid point
TRIL_LOWER = (0.0, 1e-3, -1e-3, 30.0, -30.0)
TRIL_DIMS = (1, 7, 32)
CENTRE = dict(raw=0.0, loc=1.0, eps=1.0)


def f32(v):
  return np.asarray(v, np.float32)


def kl_grid():
  """(mu, raw) [n] float32 each: RAW_AXIS x LOC_AXIS"""
  r, m = np.meshgrid(f32(RAW_AXIS), f32(LOC_AXIS), indexing="ij")
  return m.ravel(), r.ravel()


def axis_grid():
  """(mu, raw, eps) [n] float32 each: one axis at a time against CENTRE (the sample and the weight term)"""
  pts = []
  for name, axis in (("raw", RAW_AXIS), ("loc", LOC_AXIS), ("eps", EPS_AXIS)):
    for v in axis:
      p = dict(CENTRE)
      p[name] = v
      pts.append((p["loc"], p["raw"], p["eps"]))
  a = f32(pts)
  return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def kept(v):
  with np.errstate(invalid="ignore"):
    return np.isfinite(v) & (np.abs(v) < F32_MAX)


# ---- the diagonal head ----------------------------------------------------------------------------------------------------------------
def x_of(raw):
  """x = raw + log(e - 1) as the kernels form it (the float32 sum of two float32 numbers), in float64"""
  return (f32(raw) + C1).astype(np.float64)


def x_exact(raw):
  return np.asarray(raw, np.float64) + SOFTPLUS_INV_1


def log_sigma(x):
  x = np.asarray(x, np.float64)
  with np.errstate(divide="ignore", under="ignore"):
    t = np.exp(np.minimum(x, 0.0))
    return np.where(x < -30.0, x + np.log1p(-t / 2.0 + t * t / 3.0), np.log(np.maximum(softplus(x), 1e-300)))


def diag_terms(mu, raw, eps=0.0):
  """dict of float64 arrays of the diagonal head at (mu, raw, eps): sigma, z, kl (element), dmu, draw (the KL's partials), w (the weight term)"""
  mu, eps = np.asarray(mu, np.float64), np.asarray(eps, np.float64)
  x = x_exact(raw)
  sg, ls = softplus(x), log_sigma(x)
  z = mu + sg * eps
  with np.errstate(over="ignore"):
    return dict(x=x, sigma=sg, log_sigma=ls, z=z, kl=0.5 * (sg * sg + mu * mu - 1.0) - ls, dmu=mu + 0.0 * x, draw=(sg - 1.0 / sg) * expit(x),
                w=-0.5 * z * z + 0.5 * eps * eps + ls)


def _e_sigma(x):
  return _sp_abs(x) + np.abs(x) * expit(x) + np.where(softplus(x) < F32_MIN * 1.001, FLUSH, 0.0)


def above_floor(raw):
  return np.asarray(raw, np.float64) >= DRAW_FLOOR


def _e_log(x, sg, ls, ops):
  return np.where(x < TAIL, np.abs(x) + 0.02, ops * np.abs(ls) + _e_sigma(x) / sg)


def diag_bounds(mu, raw, eps=0.0):
  """the absolute float32 bounds (already times u) of diag_terms' entries: the module docstring's table"""
  t = diag_terms(mu, raw, eps)
  mu, eps = np.asarray(mu, np.float64), np.asarray(eps, np.float64)
  x, sg, ls, z = t["x"], t["sigma"], t["log_sigma"], t["z"]
  es = _e_sigma(x)
  ez = es * np.abs(eps) + np.abs(sg * eps) + np.abs(z) + FLUSH
  A, B, C = sg * sg, mu * mu, 2.0 * np.abs(ls)
  with np.errstate(over="ignore"):
    kl = 0.5 * (2.0 * es * sg + A + B + 2.0 * _e_log(x, sg, ls, 3.0) + 3.0 * (A + B + 1.0 + C)) + FLUSH
    sgm = expit(x)
    draw = (es + (2.0 + es / sg) / sg + sg + 1.0 / sg) * sgm + (8.0 + 3.0 * np.abs(x)) * np.abs(t["draw"]) + FLUSH      # (meant from DRAW_FLOOR up)
    w = ez * np.abs(z) + 0.5 * z * z + 0.5 * eps * eps + _e_log(x, sg, ls, 2.0) + 2.0 * (0.5 * z * z + 0.5 * eps * eps + np.abs(ls)) + FLUSH
  return dict(sigma=es * U, z=ez * U, kl=kl * U, dmu=0.0 * x + FLUSH * U, draw=draw * U, w=w * U)


# ---- scVI's library latent -------------------------------------------------------------------------------------------------------------
def lib_terms(mu, raw, eps, mp, vp):
  mu, eps, mp, vp = (np.asarray(v, np.float64) for v in (mu, eps, mp, vp))
  x = x_exact(raw)
  sg, ls = softplus(x), log_sigma(x)
  l = mu + sg * eps
  d = mu - mp
  return dict(x=x, sigma=sg, log_sigma=ls, z=l, kl=0.5 * np.log(vp) - ls + (sg * sg + d * d) / (2.0 * vp) - 0.5, dmu=d / vp,
              draw=(sg / vp - 1.0 / sg) * expit(x), w=-0.5 * (l - mp) ** 2 / vp - 0.5 * np.log(vp) + 0.5 * eps * eps + ls)


def lib_bounds(mu, raw, eps, mp, vp):
  t = lib_terms(mu, raw, eps, mp, vp)
  mu, eps, mp, vp = (np.asarray(v, np.float64) for v in (mu, eps, mp, vp))
  x, sg, ls, l = t["x"], t["sigma"], t["log_sigma"], t["z"]
  es = _e_sigma(x)
  el = es * np.abs(eps) + np.abs(sg * eps) + np.abs(l) + FLUSH
  lsp = 0.5 * np.log(vp)
  lr = np.abs(lsp - ls)
  d = mu - mp
  Q = (sg * sg + d * d) / (2.0 * vp)
  e_lr = np.where(x < TAIL, 3.0 * np.abs(lsp) + 2.0 + 2.0 * np.abs(x) + 0.02, 2.0 * lr + 3.0 + es / sg)
  kl = e_lr + (2.0 * es * sg + 2.0 * sg * sg + 4.0 * d * d) / (2.0 * vp) + Q + 2.0 * (lr + Q + 0.5) + FLUSH
  sgm = expit(x)
  draw = np.where(x < TAIL, 0.02, ((es + sg) / vp + (1.0 + es / sg) / sg + sg / vp + 1.0 / sg) * sgm + (8.0 + 3.0 * np.abs(x)) * np.abs(t["draw"])) + FLUSH
  dd = l - mp
  T1, T2, T3 = dd * dd / (2.0 * vp), np.abs(lsp), 0.5 * eps * eps
  w = (el + np.abs(dd)) * np.abs(dd) / vp + 2.0 * T1 + 2.0 * T2 + T3 + _e_log(x, sg, ls, 2.0) + 3.0 * (T1 + T2 + T3 + np.abs(ls)) + FLUSH
  return dict(sigma=es * U, z=el * U, kl=kl * U, dmu=(2.0 * np.abs(t["dmu"]) + FLUSH) * U, draw=draw * U, w=w * U)


# ---- the full-covariance head ----------------------------------------------------------------------------------------------------------
def tril_terms(mu, raw, eps):
  """mu [D], raw [D, D] (row i of the raw factor; columns j > i inert), eps [D]: L, z [D], kl_rows [D] (their sum is the KL), dmu [D],
  draw [D, D] (the KL's partials; 0 above the diagonal)"""
  mu, raw, eps = (np.asarray(v, np.float64) for v in (mu, raw, eps))
  D = mu.size
  idx = np.arange(D)
  L = np.tril(raw, -1)
  lii = softplus(raw[idx, idx]) + TRIL_SHIFT
  L[idx, idx] = lii
  z = mu + L @ eps
  low = np.tril(raw, -1)
  kl_rows = 0.5 * ((low * low).sum(1) + lii * lii + mu * mu - 1.0) - np.log(lii)
  draw = low.copy()
  draw[idx, idx] = (lii - 1.0 / lii) * expit(raw[idx, idx])
  return dict(L=L, diag=lii, z=z, kl_rows=kl_rows, kl=kl_rows.sum(), dmu=mu, draw=draw)


def tril_bounds(mu, raw, eps):
  t = tril_terms(mu, raw, eps)
  mu, raw, eps = (np.asarray(v, np.float64) for v in (mu, raw, eps))
  D = mu.size
  idx = np.arange(D)
  rii, lii = raw[idx, idx], t["diag"]
  eL = _sp_abs(rii) + lii
  low = np.tril(raw, -1)
  sre = np.abs(low * eps[None, :]).sum(1)
  fro = (low * low).sum(1)
  z = idx * sre + eL * np.abs(eps) + 3.0 * (np.abs(mu) + sre + np.abs(lii * eps)) + FLUSH
  S = fro + lii * lii + mu * mu + 1.0
  ll = np.abs(np.log(lii))
  kl_rows = 0.5 * ((idx + 1.0) * fro + 2.0 * eL * lii + lii * lii + mu * mu + 3.0 * S) + 3.0 * ll + eL / lii + 0.5 * S + ll + FLUSH
  sg = expit(rii)
  dii = (eL + (2.0 + eL / lii) / lii + lii + 1.0 / lii) * sg + (7.0 + 2.0 * np.abs(rii)) * np.abs(t["draw"][idx, idx]) + FLUSH * (1.0 + lii + 1.0 / lii)
  draw = np.full((D, D), FLUSH)
  draw[idx, idx] = dii
  # the half-wave sum of the rows: 5 additions of the running sum of sizes
  kl = kl_rows.sum() + 5.0 * (0.5 * S + ll).sum()
  return dict(diag=eL * U, z=z * U, kl_rows=kl_rows * U, kl=kl * U, dmu=np.full(D, FLUSH * U), draw=draw * U)


def tril_case(D, diag_raw, lower, seed=0):
  """(mu [D], raw [D, D], eps [D]) float32: every diagonal raw `diag_raw`, the strict lower triangle cycling through `lower`'s values from a
  seeded start, locations and noise cycling through LOC_AXIS (below 1e19: a row's fro + mu^2 stays a float32) and EPS_AXIS"""
  rng = np.random.default_rng(seed)
  lo = f32(lower)
  raw = lo[(rng.integers(len(lo)) + np.arange(D * D)) % len(lo)].reshape(D, D)
  raw[np.arange(D), np.arange(D)] = np.float32(diag_raw)
  loc = f32(LOC_AXIS[:11])
  return loc[(np.arange(D) + seed) % len(loc)].copy(), raw, f32(EPS_AXIS)[(np.arange(D) + seed) % len(EPS_AXIS)].copy()


# ---- the float32 replay of the kernels' lines -------------------------------------------------------------------------------------------
class Replay:
  """smx_device.h's one-instruction forms in NumPy float32: the function in float64, rounded once (no measurement of the device's last bit).
  flush: denormal operands of v_log / v_rcp / v_exp are taken as 0 and v_exp's denormal results come out as 0 -- what an instruction without
  denormal support does; otherwise denormals are kept throughout."""

  def __init__(self, flush):
    self.flush = bool(flush)

  def _in(self, v):
    v = f32(v)
    return np.where(np.abs(v) < np.float32(F32_MIN), np.float32(0.0) * v, v) if self.flush else v

  def fexp(self, v):
    with np.errstate(over="ignore", under="ignore"):
      r = np.exp(self._in(v).astype(np.float64)).astype(np.float32)
    return np.where(r < np.float32(F32_MIN), np.float32(0.0), r) if self.flush else r

  def flog(self, v):
    with np.errstate(divide="ignore", invalid="ignore"):
      return (np.log2(self._in(v).astype(np.float64)).astype(np.float32) * np.float32(0.6931471805599453)).astype(np.float32)

  def logf(self, v):          # (the library's logf handles denormals in either mode)
    with np.errstate(divide="ignore", invalid="ignore"):
      return np.log(f32(v).astype(np.float64)).astype(np.float32)

  def frcp(self, v):
    with np.errstate(divide="ignore", over="ignore"):
      return (1.0 / self._in(v).astype(np.float64)).astype(np.float32)

  def log1p_small(self, e):
    e = f32(e)
    one, h, t, q, f = (np.float32(v) for v in (1.0, 0.5, 0.33333334, 0.25, 0.2))
    ser = e * (one - e * (h - e * (t - e * (q - e * f))))
    return np.where(e < np.float32(0.03125), ser, self.flog(one + e)).astype(np.float32)

  def softplusf(self, x):
    x = f32(x)
    return (np.maximum(x, np.float32(0.0)) + self.log1p_small(self.fexp(-np.abs(x)))).astype(np.float32)

  def sigmoidf(self, x):
    x = f32(x)
    e = self.fexp(-np.abs(x))
    s = self.frcp(np.float32(1.0) + e)
    return np.where(x >= 0, s, e * s).astype(np.float32)

  def diag(self, mu, raw, eps=0.0, repaired=True):
    """the diagonal head's lines: latent_fwd_quad_kernel (sigma, z, the KL element), latent_bwd_kernel at dz = 0 and kls = 1 (dmu, draw),
    iw_accum_kernel / score_draws_kernel (w)"""
    mu, raw, eps = np.broadcast_arrays(f32(mu), f32(raw), f32(eps))
    half, one, two = np.float32(0.5), np.float32(1.0), np.float32(2.0)
    tail = np.float32(TAIL)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
      xs = (raw + C1).astype(np.float32)
      sg = self.softplusf(xs)
      if repaired:
        sg = np.maximum(sg, np.float32(F32_MIN))
      z = (mu + sg * eps).astype(np.float32)
      lsf = np.where(xs < tail, xs, self.flog(sg)) if repaired else self.flog(sg)
      kl = (half * (sg * sg + mu * mu - one - two * lsf)).astype(np.float32)
      s = self.sigmoidf(xs)
      draw = ((sg - self.frcp(sg)) * s).astype(np.float32)          # (the training step's lines: unchanged)
      lsl = np.where(xs < tail, xs, self.logf(sg)) if repaired else self.logf(sg)
      w = (-half * z * z + half * eps * eps + lsl).astype(np.float32)
    return dict(sigma=sg, z=z, kl=kl, dmu=mu.copy(), draw=draw, w=w)

  def lib(self, mu, raw, eps, mp, vp, repaired=True):
    """lib_latent_fwd / bwd_kernel at dl = 0, kls = 1, and the library term of iw_accum_kernel"""
    mu, raw, eps, mp, vp = np.broadcast_arrays(f32(mu), f32(raw), f32(eps), f32(mp), f32(vp))
    half, one, two = np.float32(0.5), np.float32(1.0), np.float32(2.0)
    tail = np.float32(TAIL)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
      xs = (raw + C1).astype(np.float32)
      sg = self.softplusf(xs)
      l = (mu + sg * eps).astype(np.float32)
      sp = np.sqrt(vp).astype(np.float32)
      old = self.logf((sp / sg).astype(np.float32))
      lr = np.where(xs < tail, self.logf(sp) - xs, old).astype(np.float32) if repaired else old
      kl = (lr + (sg * sg + (mu - mp) * (mu - mp)) / (two * vp) - half).astype(np.float32)
      s = self.sigmoidf(xs)
      old = ((sg / vp - one / sg) * s).astype(np.float32)
      draw = np.where(xs < tail, -one, old).astype(np.float32) if repaired else old
      lsl = np.where(xs < tail, xs, self.logf(sg)) if repaired else self.logf(sg)
      w = (-half * (l - mp) * (l - mp) / vp - half * self.logf(vp) + half * eps * eps + lsl).astype(np.float32)
    return dict(sigma=sg, z=l, kl=kl, dmu=((mu - mp) / vp).astype(np.float32), draw=draw, w=w)

  def tril(self, mu, raw, eps):
    """latent_tril_fwd / bwd_kernel at dz = 0, kls = 1 (no repair: L_ii >= 1e-5 is a normal float)"""
    mu, raw, eps = f32(mu), f32(raw), f32(eps)
    D = mu.size
    half, one = np.float32(0.5), np.float32(1.0)
    z, klr, draw, diag = np.zeros(D, np.float32), np.zeros(D, np.float32), np.zeros((D, D), np.float32), np.zeros(D, np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
      for i in range(D):
        acc, fro = np.float32(0.0), np.float32(0.0)
        for j in range(i):
          acc = np.float32(acc + raw[i, j] * eps[j])
          fro = np.float32(fro + raw[i, j] * raw[i, j])
          draw[i, j] = raw[i, j]
        lii = np.float32(self.softplusf(raw[i, i]) + np.float32(TRIL_SHIFT))
        diag[i] = lii
        z[i] = np.float32(mu[i] + acc + lii * eps[i])
        klr[i] = np.float32(half * (fro + lii * lii + mu[i] * mu[i] - one) - self.flog(lii))
        draw[i, i] = np.float32((lii - self.frcp(lii)) * self.sigmoidf(raw[i, i]))
      kl = klr.astype(np.float32).sum(dtype=np.float32)
    return dict(diag=diag, z=z, kl_rows=klr, kl=kl, dmu=mu.copy(), draw=draw)
