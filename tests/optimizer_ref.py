"""The optimiser stage (smx_adam.h, smx_adam.hip: per-tensor clipnorm, the update rule, the bias-corrected step size) restated in float64, with
an ABSOLUTE float32 bound per component, a float32 replay of the kernels' lines, and the edge grid both test files walk.

THE REFERENCE takes what the C API receives: the hyper-parameters, lr, clipnorm, grad_scale, tied_inv, g and the slots AT THEIR FLOAT32 VALUES,
and evaluates in float64
  s = sum g^2 (or the sum of the sum-of-squares slots the launch is given), s *= tied_inv on a tied tensor, norm = sqrt(s) grad_scale,
  clip = grad_scale (clipnorm / norm  if clipnorm > 0 and norm > clipnorm -- strictly --, else 1), ge = g clip,
  t = step - t0 (1 while step <= t0), and the forms of DESIGN.md 4d's table (FORMS below) with
  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) (adam), lr / (1 - b1^t) (adamax), lr (the others).
(The rule at float64 hyper-parameters -- 0.999 for float32(0.999) -- differs by 1.3e-5 on v: DESIGN.md 4w; that is no test bound.)

THE BOUNDS are first-order error arithmetic over the lines as spelled under `fp contract(off)` (class V: value, bound e, term size s):
  u = 2^-24.  A spelled operation (*, +, fma) adds u |result| to what its operands carry; sqrtf and '/' of the host-like lines (the norm, the
  clip factor, lr_t) count 2 u (correctly rounded as hipcc builds them by default: 1 u would do); frcp = v_rcp_f32 and fsqrt = v_sqrt_f32 count
  2 u (tools/ulp_probe.hip on an MI355X over [1e-30, 1e30]: max rel 9.14e-8 = 1.53 u and 9.29e-8 = 1.56 u).  powf counts POWF_U u = twice the
  maximum tools/ulp_probe.hip measures over b in {0.5, 0.9, 0.999, 0.99999} x t in {1, 2, 3, 10, 1000, 1e5, 2^24 + 1}: 0.697 u measured (at
  0.9^3; exact at every t = 1 and at b = 0.5), 1.394 u bound -- and reaches 1 - b^t multiplied by b^t / (1 - b^t): 500 / t at b = 0.999.
  (float) t is exact up to 2^24; beyond, |t - fl(t)| |ln b| b^t is added.
  The norm: a sum of non-negative terms through ANY tree of depth d is within d u / (1 - d u) of the sum.  Depths (the source's trees):
    partials   grad_sqsum: square 1, the quad's (x^2 + y^2) + (z^2 + w^2) 2, a thread's <= 4 quads of a chunk in order 4, wave_sum 6,
               (0 + 1) + (2 + 3) 2 = 15; adam_tensor_clip over <= 4 chunk partials: 1 + 6 + 2 = 9                       -> 24
    sharded    the same per slice, + world additions of the ranks' partials in rank order                                 -> 24 + world
    slots      a thread's ceil(cnt / 256) slots in order, 6, 2                                                             -> ceil(cnt / 256) + 8
    own sweep  3 for the quad, a thread's <= 16 quads of a tensor of <= 4 chunks in order, 6, 2                            -> 27
  then tied_inv 1, sqrtf 2 (on half the sum's relative error), grad_scale 1.  The clip factor carries the norm's error whichever side of the
  strict comparison the device and the reference fall on (they may differ only where the factor is within that error of 1), + 2 u for the
  division + 1 u for grad_scale; it is exact (grad_scale) where norm + bound <= clipnorm or clipping is off.  The factor's error goes into ge,
  lr_t's into the move.  The move d = p' - p carries u (|p| + |d|) for the weight's own storage (the rounding of the fma / addition that makes p').
  FLOORS (absolute, not subject to the kept-point cap): 2^-149 per operation for results that underflow (squares of 1e-25: the sum of squares
  gets n 2^-149 and the norm sqrt of that); the weight's storage term; and v_sqrt_f32 at a denormal argument returns 0 on the MI355X (sqrt x is
  added: at most 1.1e-19 beside an epsilon of at least 1e-7).
DOMAIN: sum of squares below 2^127.  Beyond it the device gives norm inf and factor 0 as float32 tf.clip_by_norm does: asserted exactly.
KEPT POINTS: the bound is finite and its part without the floors is at most 2^-6 of the component's term size (|b1 m| + |(1 - b1) ge| for m:
what the result would be with every term taken positive).  At most a tenth of any value family may be dropped; both test files assert it.
"""
import math

import numpy as np

U = 2.0 ** -24
DEN = 2.0 ** -149
TINY = 2.0 ** -126
CAP = 2.0 ** -6
# powf: max |powf(b, t) - b^t| / b^t over the ladder, in units of u.  HIP's math table is not among this project's papers, so the figure is
# tools/ulp_probe.hip's ("powf b^t" line, MI355X): see DESIGN.md 4w; the bound is twice it.
POWF_MEASURED_U = 0.697
POWF_U = 2.0 * POWF_MEASURED_U

FORMS = ("adam", "sgd", "sgd_momentum", "sgd_nesterov", "rmsprop", "rmsprop_momentum", "adagrad", "adamax")
USES_M = {"adam", "sgd_momentum", "sgd_nesterov", "rmsprop_momentum", "adamax"}
USES_V = {"adam", "rmsprop", "rmsprop_momentum", "adagrad", "adamax"}
F32 = np.float32


def f32(x):
  """x rounded to float32, as float64: what the C API receives"""
  return np.asarray(x, np.float32).astype(np.float64)


def form_of(rule, hp):
  if rule == "sgd":
    return "sgd" if hp["momentum"] == 0 else ("sgd_nesterov" if hp["nesterov"] else "sgd_momentum")
  if rule == "rmsprop":
    return "rmsprop" if hp["momentum"] == 0 else "rmsprop_momentum"
  return rule


def scalars(rule, hp):
  """(form, b1, b2, eps, mu) as opt_scalars fills AdamArgs, at float32 values"""
  form = form_of(rule, hp)
  g = lambda k, d=0.0: float(f32(hp.get(k, d)))
  if rule == "sgd":
    return form, 0.9, 0.999, 1e-7, g("momentum")
  if rule == "rmsprop":
    return form, g("rho"), 0.999, g("epsilon"), g("momentum")
  if rule == "adagrad":
    return form, 0.9, 0.999, g("epsilon"), 0.0
  return form, g("beta_1"), g("beta_2"), g("epsilon"), 0.0


# ---- error arithmetic ----------------------------------------------------------------------------------------------------------------
class Ctx:
  def __init__(self, floors=True):
    self.floors = floors
    self.den = DEN if floors else 0.0


class V:
  """v: the float64 value; e: bound on |device - v|; s: the term size (the value with every term taken positive)"""
  __slots__ = ("v", "e", "s")

  def __init__(self, v, e=None, s=None):
    self.v = np.asarray(v, np.float64)
    self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)
    self.s = np.abs(self.v) if s is None else np.asarray(s, np.float64)


def _rounded(ctx, val, prop, size, n=1):
  return V(val, prop * (1 + n * U) + n * U * np.abs(val) + ctx.den, size)


def _mulprop(a, b):
  return np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e


def mul(ctx, a, b):
  return _rounded(ctx, a.v * b.v, _mulprop(a, b), a.s * b.s)


def add(ctx, a, b):
  return _rounded(ctx, a.v + b.v, a.e + b.e, a.s + b.s)


def neg(a):
  return V(-a.v, a.e, a.s)


def fma(ctx, a, b, c):
  return _rounded(ctx, a.v * b.v + c.v, _mulprop(a, b) + c.e, a.s * b.s + c.s)


def _sqrt_prop(a):
  r = np.sqrt(a.v)
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.where(a.e > 0, np.minimum(np.where(r > 0, a.e / np.where(r > 0, r, 1.0), np.inf), np.sqrt(a.e)), 0.0)


def sqrt_cr(ctx, a):
  """sqrtf of the norm and of lr_t (2 u allowed)"""
  return _rounded(ctx, np.sqrt(a.v), _sqrt_prop(a), np.sqrt(a.s), 2)


def div_cr(ctx, a, b):
  lo = np.abs(b.v) - b.e
  val = a.v / b.v
  with np.errstate(divide="ignore", invalid="ignore"):
    prop = np.where(lo > 0, (a.e + np.abs(val) * b.e) / np.where(lo > 0, lo, 1.0), np.inf)
  return _rounded(ctx, val, prop, a.s / np.abs(b.v), 2)


def fsqrt(ctx, a):
  """v_sqrt_f32: 2 u; at an argument that may be denormal the instruction may return 0 (floor)"""
  r = _rounded(ctx, np.sqrt(a.v), _sqrt_prop(a), np.sqrt(a.s), 2)
  if ctx.floors:
    r.e = r.e + np.where(a.v - a.e < TINY, np.sqrt(a.v + a.e), 0.0)
  return r


def frcp(ctx, a):
  """v_rcp_f32: 2 u (no denominator of the rules is near the denormals: eps > 0 is added to a non-negative root)"""
  lo = np.abs(a.v) - a.e
  val = 1.0 / a.v
  with np.errstate(divide="ignore", invalid="ignore"):
    prop = np.where(lo > 0, a.e / (np.abs(a.v) * np.where(lo > 0, lo, 1.0)), np.inf)
  return _rounded(ctx, val, prop, np.abs(val), 2)


def vmax(a, b):
  return V(np.maximum(a.v, b.v), np.maximum(a.e, b.e), np.maximum(a.s, b.s))


# ---- the step size -------------------------------------------------------------------------------------------------------------------
def rule_count(step, t0):
  """t of opt_lr_t: `step` = optimiser steps so far, this one included; t0 = the step index at which the rule's state began"""
  return step - t0 if step - 1 >= t0 else 1


def _one_minus_pow(ctx, b, t):
  val = b ** t if b > 0 else 0.0
  tf = float(np.float32(t))
  e = POWF_U * U * val + (abs(t - tf) * abs(math.log(b)) * val if b > 0 else 0.0)
  if ctx.floors and val < TINY:
    e += val + DEN
  return _rounded(ctx, 1.0 - val, e, 1.0 + val)


def step_size(form, b1, b2, lr, t, ctx=None):
  ctx = ctx or Ctx()
  lr = V(float(lr))
  if form == "adam":
    return div_cr(ctx, mul(ctx, lr, sqrt_cr(ctx, _one_minus_pow(ctx, b2, t))), _one_minus_pow(ctx, b1, t))
  if form == "adamax":
    return div_cr(ctx, lr, _one_minus_pow(ctx, b1, t))
  return lr


# ---- clipnorm ------------------------------------------------------------------------------------------------------------------------
def norm_depth(path, cnt=0, world=0):
  return {"partials": 24, "shard": 24 + world, "slots": -(-cnt // 256) + 8, "own": 27}[path]


def tensor_norm(s, depth, n_squares, tied_inv, grad_scale, ctx=None):
  """s: the float64 sum of squares (or of the slots); n_squares: squares formed on the device (0 on the slots' path)"""
  ctx = ctx or Ctx()
  if not s < 2.0 ** 127:
    return V(np.inf, np.inf)
  sv = V(s, depth * U / (1 - depth * U) * s + n_squares * ctx.den)
  if tied_inv != 1.0:
    sv = mul(ctx, sv, V(float(tied_inv)))
  return mul(ctx, sqrt_cr(ctx, sv), V(float(grad_scale)))


def clip_factor(norm, clipnorm, grad_scale, ctx=None):
  n, e = float(norm.v), float(norm.e)
  if not clipnorm > 0 or n + e <= clipnorm:
    return V(float(grad_scale))
  ref = grad_scale * (clipnorm / n if n > clipnorm else 1.0)
  rel = e / (n - e) + 3 * U if n > e else np.inf
  return V(ref, abs(ref) * rel * (1 + 4 * U), abs(ref))


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def update(form, b1, b2, eps, mu, lr_t, clip, g, m, v, p, ctx=None):
  """One tensor: dict(m, v, d) of V (a slot the form does not use is absent); d is the move p' - p.  lr_t, clip: V scalars."""
  ctx = ctx or Ctx()
  g, m, v, p = (V(np.asarray(x, np.float64)) for x in (g, m, v, p))
  B1, B2, EPS, MU = V(b1), V(b2), V(eps), V(mu)
  ge = mul(ctx, g, clip)
  out = {}

  def stored(move):   # p' = round(p + move): the move as the test sees it, p' - p
    if ctx.floors:
      move = V(move.v, move.e + U * (np.abs(p.v) + np.abs(move.v) + move.e) + ctx.den, move.s)
    return move

  def quotient(num, den):   # fma(-num, rcp, p)
    r = frcp(ctx, den)
    return stored(V(-num.v * r.v, _mulprop(num, r), num.s * r.s))

  if form == "adam":
    c1, c2 = add(ctx, V(1.0), neg(B1)), add(ctx, V(1.0), neg(B2))
    out["m"] = fma(ctx, B1, m, mul(ctx, c1, ge))
    out["v"] = fma(ctx, B2, v, mul(ctx, mul(ctx, c2, ge), ge))
    out["d"] = quotient(mul(ctx, lr_t, out["m"]), add(ctx, fsqrt(ctx, out["v"]), EPS))
  elif form == "sgd":
    q = mul(ctx, lr_t, ge)   # fma(-lr_t, ge, p): the product is not rounded
    out["d"] = stored(V(-lr_t.v * ge.v, _mulprop(lr_t, ge), q.s))
  elif form in ("sgd_momentum", "sgd_nesterov"):
    out["m"] = fma(ctx, MU, m, neg(mul(ctx, lr_t, ge)))
    out["d"] = stored(out["m"] if form == "sgd_momentum" else fma(ctx, MU, out["m"], neg(mul(ctx, lr_t, ge))))
  elif form in ("rmsprop", "rmsprop_momentum"):
    c1 = add(ctx, V(1.0), neg(B1))
    out["v"] = fma(ctx, B1, v, mul(ctx, mul(ctx, c1, ge), ge))
    if form == "rmsprop":
      out["d"] = quotient(mul(ctx, lr_t, ge), add(ctx, fsqrt(ctx, out["v"]), EPS))
    else:
      out["m"] = fma(ctx, MU, m, mul(ctx, mul(ctx, lr_t, ge), frcp(ctx, fsqrt(ctx, add(ctx, out["v"], EPS)))))
      out["d"] = stored(neg(out["m"]))
  elif form == "adagrad":
    out["v"] = fma(ctx, ge, ge, v)
    out["d"] = quotient(mul(ctx, lr_t, ge), add(ctx, fsqrt(ctx, out["v"]), EPS))
  elif form == "adamax":
    c1 = add(ctx, V(1.0), neg(B1))
    out["m"] = fma(ctx, B1, m, mul(ctx, c1, ge))
    out["v"] = vmax(mul(ctx, B2, v), V(np.abs(ge.v), ge.e, ge.s))
    out["d"] = quotient(mul(ctx, lr_t, out["m"]), add(ctx, out["v"], EPS))
  else:
    raise ValueError(form)
  return out


def kept(full, rel):
  """the kept-point rule: `full` the bound with its floors, `rel` the same without them"""
  return np.isfinite(full.e) & (rel.e <= CAP * rel.s)


# ---- the float32 replay of the kernels' lines ----------------------------------------------------------------------------------------
def _fma32(a, b, c):
  """one rounding: the product of two float32 is exact in float64"""
  with np.errstate(over="ignore", invalid="ignore"):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


_L = np.arange(64)
_WAVE_STEPS = [_L ^ 1, _L ^ 2, (_L & ~7) | (7 - (_L & 7)), (_L & ~15) | (15 - (_L & 15)), _L ^ 16, _L ^ 32]


def wave_sum32(x):
  """wave_sum (smx_device.h) over the last axis of 64 lanes: two quad_perm steps, row_half_mirror, row_mirror, the two lane swaps"""
  x = np.asarray(x, F32)
  for idx in _WAVE_STEPS:
    x = x + x[..., idx]
  return x[..., 0]


def block_sum32(per_thread):
  """256 threads' values -> wave_sum per wave, then (0 + 1) + (2 + 3)"""
  w = wave_sum32(np.asarray(per_thread, F32).reshape(4, 64))
  return F32(F32(w[0] + w[1]) + F32(w[2] + w[3]))


def _strided32(terms):
  """a thread's terms tid, tid + 256, ... added in order from 0, then block_sum"""
  terms = np.asarray(terms, F32)
  n = -(-len(terms) // 256) * 256
  t = np.zeros(n, F32)
  t[:len(terms)] = terms
  acc = np.zeros(256, F32)
  for row in t.reshape(-1, 256):
    acc = acc + row
  return block_sum32(acc)


def _quad_squares32(g):
  q = np.asarray(g, F32).reshape(-1, 4)
  with np.errstate(over="ignore", under="ignore"):
    sq = q * q
    return (sq[:, 0] + sq[:, 1]) + (sq[:, 2] + sq[:, 3])


def replay_sumsq(path, gpad, lo=0, world=1, slots=None, global_cuts=None):
  """The tensor's float32 sum of squares as adam_tensor_clip sees it.  gpad: the padded gradient of ONE tensor; `shard`: lo = the tensor's
  offset in the flat buffer, global_cuts = the slices' boundaries."""
  if path == "slots":
    return _strided32(slots)
  if path == "own":
    return _strided32(_quad_squares32(gpad))
  chunks = [gpad[c:c + 4096] for c in range(0, len(gpad), 4096)]
  if path == "partials":
    parts = [_strided32(_quad_squares32(c)) for c in chunks]
  else:
    parts = []
    for ci, c in enumerate(chunks):
      off = lo + ci * 4096
      s = F32(0)
      for r in range(world):
        a, b = max(global_cuts[r] - off, 0), min(global_cuts[r + 1] - off, len(c))
        s = F32(s + (_strided32(_quad_squares32(c[a:b])) if b > a else F32(0)))
      parts.append(s)
  return _strided32(np.array(parts, F32))


def replay_norm(s32, tied_inv, grad_scale, clipnorm):
  with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
    s = F32(s32)
    if tied_inv != 1.0:
      s = F32(s * F32(tied_inv))
    norm = F32(np.sqrt(s) * F32(grad_scale))
    clip = F32(grad_scale)
    if clipnorm > 0 and norm > F32(clipnorm):
      clip = F32(clip * F32(F32(clipnorm) / norm))
  return norm, clip


def replay_lr_t(form, b1, b2, lr, t):
  powf = lambda b: F32(float(F32(b)) ** float(F32(t)))
  one = F32(1)
  if form == "adam":
    return F32(F32(F32(lr) * np.sqrt(F32(one - powf(b2)))) / F32(one - powf(b1)))
  if form == "adamax":
    return F32(F32(lr) / F32(one - powf(b1)))
  return F32(lr)


def replay_update(form, b1, b2, eps, mu, lr_t, clip, g, m, v, p, mutate=None):
  """opt_apply4 / adam_apply4 line by line in float32 (fma: one rounding; frcp, fsqrt: correctly rounded, inside their 2 u).  `mutate`: a wrong
  rule the grid must tell from the right one (MUTATIONS)."""
  b1, b2, eps, mu, lr_t, clip = (F32(x) for x in (b1, b2, eps, mu, lr_t, clip))
  g, m, v, p = (np.asarray(x, F32) for x in (g, m, v, p))
  one = F32(1)
  with np.errstate(all="ignore"):
    ge = g * clip
    rcp = lambda x: one / x
    if form == "adam":
      m2 = _fma32(b1, m, (one - b1) * (g if mutate == "m_unclipped" else ge))
      v2 = _fma32(b2, v, ((one - b2) * ge) * ge)
      den = np.sqrt(v2 + eps * eps) if mutate == "eps_inside" else np.sqrt(v2) + eps
      return m2, v2, _fma32(-(lr_t * m2), rcp(den), p)
    if form == "sgd":
      return m, v, _fma32(-lr_t, ge, p)
    if form == "sgd_momentum":
      m2 = _fma32(mu, m, -(lr_t * ge))
      return m2, v, p + m2
    if form == "sgd_nesterov":
      m2 = _fma32(mu, m, -(lr_t * ge))
      return m2, v, p + _fma32(mu, m if mutate == "nesterov_old" else m2, -(lr_t * ge))
    if form == "rmsprop":
      v2 = _fma32(b1, v, ((one - b1) * ge) * ge)
      den = np.sqrt(v2 + eps * eps) if mutate == "eps_inside" else np.sqrt(v2) + eps
      return m, v2, _fma32(-(lr_t * ge), rcp(den), p)
    if form == "rmsprop_momentum":
      v2 = _fma32(b1, v, ((one - b1) * ge) * ge)
      den = np.sqrt(v2) + eps if mutate == "eps_outside" else np.sqrt(v2 + eps)
      m2 = _fma32(mu, m, (lr_t * ge) * rcp(den))
      return m2, v2, p - m2
    if form == "adagrad":
      v2 = _fma32(ge, ge, v)
      den = np.sqrt(v2 + eps * eps) if mutate == "eps_inside" else np.sqrt(v2) + eps
      return m, v2, _fma32(-(lr_t * ge), rcp(den), p)
    if form == "adamax":
      m2 = _fma32(b1, m, (one - b1) * ge)
      v2 = np.maximum(v if mutate == "adamax_no_b2" else b2 * v, np.abs(ge))
      return m2, v2, _fma32(-(lr_t * m2), rcp(v2 + eps), p)
  raise ValueError(form)


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 63, 64, 65, 1020, 1024, 1028, 2044, 2048, 2052, 4095, 4096, 4097, 4096 + 1024 + 4, 8192 + 64, 3 * 4096 + 2048 + 64)
SQ_COUNTS = (1, 255, 256, 257, 1672, 2047, 2048, 2049, 4097, 0)   # 0: the tensor's own sweep
G_FAMILIES = ("n1e-30", "n1e-12", "n1e-4", "n1", "n1e4", "zeros", "outlier", "norm_is_clip", "norm_above_clip", "c1e-25", "ones")
M_FAMILIES = ("0", "+1e-3", "-1e-3", "cancels")
V_FAMILIES = ("0", "1e-40", "1e-30", "eps^2", "1e-6", "1", "1e30", "0.1", "1e8")
P_FAMILIES = ("0", "+1", "-1", "1e-30", "1e6")
B1S, B2S, MUS, EPSS, LRS, CLIPS = (0.0, 0.5, 0.9), (0.9, 0.999, 0.99999), (0.5, 0.9), (1e-7, 1e-3), (0.0, 1e-3, 1.0), (0.0, 5.0)
TS = (1, 2, 3, 10, 1000, 100000, 2 ** 24 + 1)
# (carrier, use_sq, wgs, world): wgs -1 = one workgroup per chunk
CARRIERS = ([("launch", 0, 0, 0), ("launch", 1, 0, 0)] + [("sweep", sq, w, 0) for sq in (0, 1) for w in (1, 2, 3, -1)] +
            [("shard", 0, 2, w) for w in (1, 2, 3, 4)] + [("body512", 0, 0, 0), ("body512", 1, 0, 0)])
CLIP_FOR_FAMILIES = 5.0   # the norm the two clip-edge families are built around, whether or not the launch clips


def hyper(form, k):
  """the k-th case of a form: every value of every axis comes up, the axes out of step with each other"""
  b1, b2, mu, eps = B1S[k % 3], B2S[(k // 3 + k) % 3], MUS[k % 2], EPSS[(k // 2) % 2]
  lr, clipnorm = LRS[(k + k // 3 + 1) % 3], CLIPS[(k + k // 2) % 2]
  t, t0 = TS[k % 7], (0, 3)[(k // 7 + k) % 2]
  step = t + t0
  if k == 5:   # `step < t0` once: the rule counts t = 1
    step, t0 = 2, 3
  rule, hp = {"adam": ("adam", dict(beta_1=b1, beta_2=b2, epsilon=eps)), "sgd": ("sgd", {}), "sgd_momentum": ("sgd", dict(momentum=mu)),
              "sgd_nesterov": ("sgd", dict(momentum=mu, nesterov=True)), "rmsprop": ("rmsprop", dict(rho=b2, epsilon=eps)),
              "rmsprop_momentum": ("rmsprop", dict(rho=b2, momentum=mu, epsilon=eps)), "adagrad": ("adagrad", dict(epsilon=eps)),
              "adamax": ("adamax", dict(beta_1=b1, beta_2=b2, epsilon=eps))}[form]
  grad_scale = (1.0, 0.5)[(k // 4) % 2]
  return dict(rule=rule, hp=hp, lr=lr, clipnorm=clipnorm, step=step, t0=t0, grad_scale=grad_scale)


def _g_family(fam, n, rng, grad_scale):
  c = CLIP_FOR_FAMILIES / grad_scale
  g = np.zeros(n)
  if fam.startswith("n1"):
    g = rng.normal(size=n) * float(fam[1:])
  elif fam == "outlier":
    g[n // 2] = 1e3
  elif fam in ("norm_is_clip", "norm_above_clip"):
    if n == 1:
      g[0] = c * (1.0 if fam == "norm_is_clip" else 1 + 2.0 ** -22)
    else:
      g[0], g[n - 1] = 0.6 * c, 0.8 * c   # (3, 4, 5) scaled: every square and the sum exact in float32
      if fam == "norm_above_clip":
        if n > 2:
          g[1] = 4e-4 * c    # s = c^2 (1 + 1.6e-7): the root is the float above c, or the one after
        else:
          g[0] = 0.6 * c * (1 + 2.0 ** -21)
  elif fam == "c1e-25":
    g[:] = 1e-25
  elif fam == "ones":
    g[:] = 1.0
  return f32(g)


def make_launch(form, k, carrier):
  """The tensors of one launch: dict(hyper..., form, scalars, tensors=[dict(size, g, m, v, p, gf, labels...)], tied, tied_inv, sq)."""
  h = hyper(form, k)
  name, use_sq, wgs, world = carrier
  _, b1, b2, eps, mu = scalars(h["rule"], {**dict(momentum=0.0, nesterov=False, rho=0.9, epsilon=1e-7, beta_1=0.9, beta_2=0.999), **h["hp"]})
  rng = np.random.default_rng(1000 * FORMS.index(form) + k)
  gs = h["grad_scale"]
  fams = [f for f in G_FAMILIES if f != "ones" or form == "adagrad"]
  tensors = []
  for i, n in enumerate(SIZES):
    gf = fams[(i + k) % len(fams)]
    g = _g_family(gf, n, rng, gs)
    j = np.arange(n) + 3 * k + i
    nv = 9 if form == "adagrad" else 7
    mf, vf, pf = j % 4, (j // 4) % nv, (j // (4 * nv)) % 5   # (140 consecutive elements meet every combination; 180 under Adagrad)
    v = f32(np.choose(vf, [0.0, 1e-40, 1e-30, float(f32(eps)) ** 2, 1e-6, 1.0, 1e30, 0.1, 1e8]))
    p = f32(np.choose(pf, [0.0, 1.0, -1.0, 1e-30, 1e6]))
    tensors.append(dict(size=n, g=g, v=v, p=p, gf=gf, mf=mf, vf=vf, pf=pf))
  # the tied pair: two tensors of unit-normal families, C = 4 identical rows -> tied_inv = 1 / 4
  tied = [i for i, t in enumerate(tensors) if t["gf"] in ("n1", "n1e-4") and t["size"] >= 1020][:2] if k % 2 else []
  tied_inv = 0.25 if tied else 1.0
  total = int(sum((t["size"] + 63) // 64 * 64 for t in tensors))
  n_chunks = int(sum(-(-((t["size"] + 63) // 64 * 64) // 4096) for t in tensors))
  slice_ = ((total + world - 1) // world + 63) // 64 * 64 if world else 0
  cuts = [min(r * slice_, total) for r in range(world + 1)] if world else None
  t = rule_count(h["step"], h["t0"])
  lo = 0
  for i, tn in enumerate(tensors):
    n, pad = tn["size"], (tn["size"] + 63) // 64 * 64
    gpad = np.zeros(pad, np.float32)
    gpad[:n] = tn["g"]
    s64 = float((tn["g"] ** 2).sum())
    tn["sq"] = None
    if use_sq:
      cnt = SQ_COUNTS[(i + k) % len(SQ_COUNTS)]
      if cnt:
        if tn["gf"] in ("norm_is_clip", "norm_above_clip"):
          w = np.zeros(cnt)
          w[cnt // 2] = 1.0
          if tn["gf"] == "norm_above_clip":
            s64 = float(f32(s64 * (1 + 2.0 ** -21)))
        else:
          w = rng.uniform(0.5, 1.5, size=cnt)
          w /= w.sum()
        tn["sq"] = np.asarray(s64 * w if s64 < 3e38 else np.zeros(cnt), np.float32)
        s64 = float(tn["sq"].astype(np.float64).sum())
        tn["path"], depth, nsq = "slots", norm_depth("slots", cnt), 0
      else:
        tn["path"], depth, nsq = "own", norm_depth("own"), pad
    elif name == "shard":
      tn["path"], depth, nsq = "shard", norm_depth("shard", world=world), pad
    else:
      tn["path"], depth, nsq = "partials", norm_depth("partials"), pad
    tn.update(s64=s64, depth=depth, nsq=nsq, gpad=gpad, lo=lo, tied_inv=tied_inv if i in tied else 1.0)
    lo += pad
    # the m family needs the reference's own clip factor: the cancelling accumulator is built from ge
    norm = tensor_norm(s64, depth, nsq, tn["tied_inv"], gs)
    clip = float(clip_factor(norm, h["clipnorm"], gs).v) if np.isfinite(norm.v) else 0.0
    ge = tn["g"] * clip
    lr_t = float(step_size(form, b1, b2, float(f32(h["lr"])), t).v)
    with np.errstate(all="ignore"):
      if form in ("adam", "adamax"):
        cancel = -(1 - b1) * ge / b1 if b1 > 0 else np.zeros(n)
      elif form in ("sgd_momentum", "sgd_nesterov"):
        cancel = lr_t * ge / mu
      elif form == "rmsprop_momentum":
        cancel = -lr_t * ge / np.sqrt(b1 * tn["v"] + (1 - b1) * ge * ge + eps) / mu
      else:
        cancel = np.zeros(n)
    tn["m"] = f32(np.choose(tn["mf"], [np.zeros(n), np.full(n, 1e-3), np.full(n, -1e-3), np.nan_to_num(cancel)]))
  return dict(h, form=form, k=k, carrier=name, use_sq=use_sq, wgs=n_chunks if wgs < 0 else wgs, world=world, b1=b1, b2=b2, eps=eps, mu=mu, t=t,
              tensors=tensors, tied=tied, tied_inv=tied_inv, total=total, n_chunks=n_chunks, cuts=cuts)


def reference_launch(L):
  """Per tensor: dict(norm, clip, m, v, d: V with the full bound; keep: {component: bool array}) and L['lr_t'] (V, keep)."""
  full, rel = Ctx(True), Ctx(False)
  lr32 = float(f32(L["lr"]))
  lrt = {c: step_size(L["form"], L["b1"], L["b2"], lr32, L["t"], c) for c in (full, rel)}
  out = dict(lr_t=lrt[full], lr_t_keep=bool(kept(lrt[full], lrt[rel])), tensors=[])
  for tn in L["tensors"]:
    r = {}
    both = {}
    for c in (full, rel):
      norm = tensor_norm(tn["s64"], tn["depth"], tn["nsq"], tn["tied_inv"], L["grad_scale"], c)
      if not np.isfinite(norm.v):
        both[c] = None
        continue
      clip = clip_factor(norm, L["clipnorm"], L["grad_scale"], c)
      both[c] = dict(norm=norm, clip=clip, **update(L["form"], L["b1"], L["b2"], L["eps"], L["mu"], lrt[c], clip, tn["g"], tn["m"], tn["v"], tn["p"], c))
    if both[full] is None:
      out["tensors"].append(None)
      continue
    r.update(both[full])
    r["keep"] = {key: kept(both[full][key], both[rel][key]) for key in both[full]}
    out["tensors"].append(r)
  return out


def replay_launch(L, mutate=None):
  """The float32 replay of the whole launch: per tensor dict(norm, clip, m, v, d), and lr_t."""
  t = L["t"] + {"t_minus_1": -1, "t_plus_1": 1}.get(mutate, 0)
  lr_t = replay_lr_t(L["form"], L["b1"], L["b2"], L["lr"], t)
  if mutate == "lr_for_lr_t":
    lr_t = F32(L["lr"])
  if mutate == "adamax_adam_step" and L["form"] == "adamax":
    lr_t = replay_lr_t("adam", L["b1"], L["b2"], L["lr"], L["t"])
  sums = [replay_sumsq(tn["path"], tn["gpad"], tn["lo"], L["world"], tn["sq"], L["cuts"]) for tn in L["tensors"]]
  if mutate == "global_norm":
    sums = [F32(sum(float(s) for s in sums))] * len(sums)
  out = dict(lr_t=lr_t, tensors=[])
  for tn, s in zip(L["tensors"], sums):
    norm, clip = replay_norm(s, 1.0 if mutate == "no_tied_inv" else tn["tied_inv"], L["grad_scale"], L["clipnorm"])
    if mutate == "grad_scale_twice":
      clip = F32(clip * F32(L["grad_scale"]))
    m, v, p = replay_update(L["form"], L["b1"], L["b2"], L["eps"], L["mu"], lr_t, clip, tn["g"], tn["m"], tn["v"], tn["p"], mutate)
    out["tensors"].append(dict(norm=norm, clip=clip, m=m, v=v, d=p.astype(np.float64) - tn["p"]))
  return out


MUTATIONS = {   # name -> the forms it changes
    "eps_inside": ("adam", "rmsprop", "adagrad"), "eps_outside": ("rmsprop_momentum",), "nesterov_old": ("sgd_nesterov",),
    "adamax_no_b2": ("adamax",), "adamax_adam_step": ("adamax",), "t_minus_1": ("adam", "adamax"), "t_plus_1": ("adam", "adamax"),
    "lr_for_lr_t": ("adam", "adamax"), "m_unclipped": ("adam",), "global_norm": FORMS, "no_tied_inv": FORMS, "grad_scale_twice": FORMS,
}


def ratios(ref, got, L):
  """worst |got - reference| / bound per component over the kept points of a launch; a NaN at a kept point counts as inf.
  Also the kept counts per value family: {(component, axis, family): [kept, all]}."""
  worst, share = {}, {}

  def note(key, err, bound, keep):
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
      r = np.where(keep, np.where(err == 0, 0.0, err / bound), 0.0)
    worst[key] = max(worst.get(key, 0.0), float(np.max(r)) if np.size(r) else 0.0)

  if L["form"] in ("adam", "adamax"):
    note("lr_t", abs(float(got["lr_t"]) - ref["lr_t"].v), ref["lr_t"].e, ref["lr_t_keep"])
  for tn, r, g in zip(L["tensors"], ref["tensors"], got["tensors"]):
    if r is None:
      continue
    note("norm", np.abs(np.float64(g["norm"]) - r["norm"].v), r["norm"].e, r["keep"]["norm"])
    for key in ("m", "v", "d"):
      if key not in r:
        continue
      keep = r["keep"][key]
      note(key, np.abs(np.asarray(g[key], np.float64) - r[key].v), r[key].e, keep)
      for axis, lab in (("g", np.full(tn["size"], G_FAMILIES.index(tn["gf"]))), ("m", tn["mf"]), ("v", tn["vf"]), ("p", tn["pf"])):
        for fam in np.unique(lab):
          c = share.setdefault((key, axis, int(fam)), [0, 0])
          c[0] += int(keep[lab == fam].sum())
          c[1] += int((lab == fam).sum())
  return worst, share
