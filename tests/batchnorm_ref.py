"""float64 reference of the BatchNorm launches of smx_bn.hip -- (split-K slab sum) -> bias | BatchNorm -> activation -> dropout and its
backward, SyncBatchNorm's two-phase form included --, an absolute float32 error bound per element of every output, and a float32 NumPy
replay of the kernels' lines.  Written from the definition; the pattern is tests/latent_terms_ref.py's and tests/likelihood_grad_ref.py's.

FORWARD.   v = sum_s slab_s (+ bias without BatchNorm);  mean = sum_b v / B,  var = sum_b (v - mean)^2 / B  (or the moving statistics in
evaluation mode);  inv = 1 / sqrt(var + eps);  xhat = (v - mean) inv;  y = gamma xhat + beta;  h = act(y);  out = h x multiplier.
BACKWARD, on its actual inputs (d out slabs, out, xhat, inv_std, gamma, beta, the multipliers):  g = sum_s dout_s;
  ReLU forms:   dy = g scale where out > 0, g leak elsewhere (a NaN in `out` is "elsewhere": out > 0 is false);
  other forms:  dy = g x multiplier x act'(y), y = gamma xhat + beta (xhat itself without BatchNorm);
  dbeta = s1 = sum_b dy,  dgamma = s2 = sum_b dy xhat,  dpre = gamma inv (dy - (s1 + xhat s2) / B)   (evaluation mode: gamma inv dy;
  without BatchNorm: dpre = dy, dbias = s1).
float32 inputs (slabs, parameters, eps, the multipliers) enter as the float64 of their float32 values.

THE BOUNDS.  u = 2^-24; every bound is ABSOLUTE, in term sizes, by the rule of likelihood_grad_ref: a rounding costs
u |result|; a sum of n terms through a chain or tree of depth k costs gam(k) sum |terms|, gam(k) = k u / (1 - k u); an input's error is
carried through the exact partial derivative (in its finite form where the input may move far); products of two errors are kept where an
error can be as large as its value, and a factor 1 + 2^-10 on the total covers the other second-order terms; + 2^-126 for an underflow.

  quantity          the kernels' operations                                                         bound
  v                 slabs added in order 0, 1, ... (wide: 16 interleaved chains, then 16 partial      E_v = gam(S) (sum_s |slab_s| + |bias|)
                    sums in order: never more than S roundings on a path for S >= 1), + bias
  column sum        bn_col_reduce: a thread's rows r, r + 64, ... in order, then the balanced tree    depth k(B) = ceil(B / 64) + 5
                    over the 64 threads of a column (3 lane steps, 2 + 1 over the 8 waves)
  mean              the tree over the computed v, one division                                        E_m = (sum E_v + gam(k) sum (|v| + E_v)) / B + u |mean|
  d = v - mean      one rounding; v's and the mean's error                                            E_d = E_v + E_m + u |d|
  var               fma(d, d, .) per row (one rounding of the running sum each), the tree, a          E_var = (sum (2 |d| E_d + E_d^2) + gam(k + 1) sum (|d| + E_d)^2) / B + u var
                    division
  inv               var + eps 1; rsqrtf 2 (one ulp: v_rsq_f32 in the CDNA ISA guide and HIP's math    E_i = 2 u inv + E_ve / (2 (ve - E_ve)^1.5),  ve = var + eps,
                    table; measured 1.56 u over [1e-3, 4e-3] by tools/ulp_probe.hip);   E_ve = E_var + u ve  (no bound where E_ve >= ve / 2)
                    var's error through |d inv / d ve| at the nearest admissible ve
  xhat              one product                                                                       E_x = E_d inv + |d| E_i + E_d E_i + u |xhat|
  y                 one fma (SyncBatchNorm: a product and a sum, + u |gamma xhat|; its d d likewise     E_y = |gamma| E_x + u |y|
                    rounded before the sum: k + 2 for k + 1 under var)
  h                 ReLU: max (1-Lipschitz, exact); leak: a product and a sum; the other activations  E_h = L E_y + K u |h|;  (L, K) = relu (1, 0), leak (1, 2), linear (1, 0),
                    (smx_act.h) are libm calls at <= 2 ulp = 4 u each (HIP's math table: expf,          leaky_relu (1, 2), elu (1, 4), selu (1.7581, 8), tanh (1, 4),
                    expm1f, tanhf, log1pf 1 ulp) and correctly rounded + x /                            sigmoid (1 / 4, 7), softplus (1, 9)
  out               one product with the multiplier (0 or 1 / (1 - p) in float32, an input)           E_o = mult E_h + u |out|
  SyncBatchNorm     per rank: mean_r, q_r = sum (v - mean_r)^2 as above over its B / W rows; then      E_M = (sum E_mr + gam(W) sum |mean_r|) / W + u |mean|;  E_dm = E_mr + E_M + u |dm|;
    statistics      mean = sum_r mean_r / W, m2 = sum_r (q_r + (B / W) dm_r^2), dm_r = mean_r - mean,   E_var = (sum_r (E_qr + (B / W) (2 |dm| E_dm + E_dm^2 + 3 u dm^2))
                    var = m2 / B (Chan's pairwise form: exact for exact operands)                       + gam(2 W) m2) / B + 2 u var
  g                 the slab sum of d out                                                             E_g = gam(S) sum_s |dout_s|
  dy, ReLU forms    one product (scale or leak; the mask is a comparison of an input: exact)          E_dy = |c| E_g + u |dy|
  dy, other forms   y by one fma; act'(h(y)): L2 = max |act''| (elu 1, selu 1.7581, tanh 0.77,        E_a = L2 u |y| + 16 u;  E_dy = |mult a| E_g + |g mult| E_a + 2 u |dy|
                    sigmoid 0.0963, softplus 1 / 4, else 0), its own operations <= 16 u absolute
                    (|act'| <= 1.76); two products
  s1 = dbeta        the tree over dy                                                                  E_1 = sum E_dy + gam(k) sum (|dy| + E_dy)
  s2 = dgamma       product, then the tree                                                            E_2 = sum (E_dy |xhat| + u |dy xhat|) + gam(k) sum (|dy xhat| + E_dy |xhat|)
  dpre              t = fma(xhat, s2, s1); q = fma(-t, 1 / B, dy) (1 / B rounded); (gamma inv) q:     E_t = |xhat| E_2 + E_1 + u |t|;  E_q = (E_t + u |t|) / B + E_dy + u |q|;
                    two roundings                                                                     E = |gamma inv| E_q + 2 u |gamma inv q|
  dpre, evaluation  dy gamma inv: two products                                                        |gamma inv| E_dy + 2 u |dpre|
  dpre, Sync        s1, s2 = per-rank trees, then W additions (depth k(B / W) + W); gamma inv (dpre    E_t += u |xhat s2|;  E_p = E_t / B + 2 u |t| / B;  E_q = E_dy + E_p + u |q|
                    - (1 / B) (s1 + xhat s2)) without the fmas
The moving statistics' update is two products and a sum, not fused: replayed bit for bit (`moving_update`), not bounded.

KEPT POINTS, from the reference alone: a point is asserted where its bound is finite and at most KEEP_REL = 2^-6 of its component's scale
-- for xhat 1 or its largest magnitude in the column, for the others the largest magnitude the component takes in its column or, where that is smaller, the size of the terms it
is made of (y, h, out: |gamma| + |beta|; var and inv: relative to var + eps and inv; dbeta: sum |dy|; dgamma: sum |dy xhat|; dpre:
|gamma inv| (max |dy| + (sum |dy| + max |xhat| sum |dy xhat|) / B)).  A column whose B max v^2 reaches 2^127 is not asserted at all (var
overflows float32 there); a bound of underflow terms only (at most 2^-100: the columns of exact zeros) is kept whatever the scale.
tests/test_batchnorm_host.py counts the dropped points per column family over the GPU test's shapes: none
loses more than a tenth, none is dropped whole (the 1e18 family is asserted at B = 1 and 2 only: 9e36 B reaches 2^127 at B = 19).
One row (B = 1): d = v - v and var are exactly 0, which bounds in term sizes do not know; the tests assert var = 0 and xhat = 0 exactly there.
The kink: the ReLU forms of the backward take their mask from the input `out`, so every point is kept; the composed forward -> backward
check keeps the columns in which every |y| exceeds its bound E_y."""
import numpy as np

from tests import activations_ref as ar

U = 2.0 ** -24
FLUSH = 2.0 ** -126
F32_MAX = 2.0 ** 127
SLACK = 1.0 + 2.0 ** -10
RSQ = 2.0                 # rsqrtf, in u
KEEP_REL = 2.0 ** -6
KEEP_ABS = 2.0 ** -100    # a bound that is only underflow terms (a column of exact zeros) is kept whatever the scale
ACT_FWD = {"relu": (1.0, 0.0), "linear": (1.0, 0.0), "leaky_relu": (1.0, 2.0), "elu": (1.0, 4.0), "selu": (ar.SELU_LAMBDA * ar.SELU_ALPHA, 8.0),
           "tanh": (1.0, 4.0), "sigmoid": (0.25, 7.0), "softplus": (1.0, 9.0)}   # (L, K)
ACT_CURV = {"relu": 0.0, "linear": 0.0, "leaky_relu": 0.0, "elu": 1.0, "selu": ar.SELU_LAMBDA * ar.SELU_ALPHA, "tanh": 0.77, "sigmoid": 0.0963,
            "softplus": 0.25}   # max |act''|
ACT_GRAD_OPS = 16.0

f32 = np.float32


def gam(k):
  return k * U / (1.0 - k * U)


def depth(B):
  return -(-B // 64) + 5


def drop_scale(p):
  """1 / (1 - p) as the kernels form it, in float32"""
  return f32(1.0) / (f32(1.0) - f32(p)) if p > 0 else f32(1.0)


def _tree_bound(absx, E, k, axis=0):
  return E.sum(axis) + gam(k) * (absx + E).sum(axis)


def _col_stats(v, Ev, B, unfused=False):
  """mean, its bound, sum (v - mean)^2, its bound over the rows (axis 0) of one rank (unfused: d d rounded before it is added)"""
  k = depth(B)
  mean = v.sum(0) / B
  Em = _tree_bound(np.abs(v), Ev, k) / B + U * np.abs(mean) + FLUSH
  d = v - mean
  Ed = Ev + Em + U * np.abs(d) + FLUSH
  q = (d * d).sum(0)
  Eq = (2 * np.abs(d) * Ed + Ed * Ed).sum(0) + gam(k + (2 if unfused else 1)) * ((np.abs(d) + Ed) ** 2).sum(0) + FLUSH
  return mean, Em, q, Eq


def forward(slabs, gamma=None, beta=None, bias=None, moving_mean=None, moving_var=None, batchnorm=True, training=True, eps=1e-3, leak=0.0,
            act="relu", mult=None, world=0):
  """slabs [S][B][H] (float32 values).  Returns {name: float64 value, "E_" + name: bound} for v, mean, var, inv, xhat, y, out (mean / var:
  the batch statistics in training mode), and `asserted` [H]: columns whose variance stays inside float32."""
  with np.errstate(all="ignore"):
    t = np.asarray(slabs, np.float64)
    S, B, H = t.shape
    v, A = t.sum(0), np.abs(t).sum(0)
    if bias is not None and not batchnorm:
      b = np.asarray(bias, np.float64)
      v, A = v + b, A + np.abs(b)
    Ev = gam(S) * A + FLUSH
    r = dict(v=v, E_v=Ev, asserted=np.ones(H, bool))
    if not batchnorm:
      y, Ey = v, Ev
      r.update(xhat=v, E_xhat=Ev)
    else:
      g, be, e = np.asarray(gamma, np.float64), np.asarray(beta, np.float64), float(f32(eps))
      if training:
        W = max(world, 1)
        Bs = B // W
        parts = [_col_stats(v[k * Bs:(k + 1) * Bs], Ev[k * Bs:(k + 1) * Bs], Bs, world > 0) for k in range(W)]
        if world == 0:
          mean, Em, q, Eq = parts[0]
          var = q / B
          Evar = Eq / B + U * var + FLUSH
        else:
          mr, Emr = np.array([p[0] for p in parts]), np.array([p[1] for p in parts])
          qr, Eqr = np.array([p[2] for p in parts]), np.array([p[3] for p in parts])
          mean = mr.sum(0) / W
          Em = (Emr.sum(0) + gam(W) * np.abs(mr).sum(0)) / W + U * np.abs(mean) + FLUSH
          dm = mr - mean
          Edm = Emr + Em + U * np.abs(dm) + FLUSH
          m2 = (qr + Bs * dm * dm).sum(0)
          var = m2 / B
          Evar = ((Eqr + Bs * (2 * np.abs(dm) * Edm + Edm * Edm + 3 * U * dm * dm)).sum(0) + gam(2 * W) * m2) / B + 2 * U * var + FLUSH
        r["asserted"] = B * (np.abs(v).max(0) ** 2) < F32_MAX
        r.update(mean=mean, E_mean=Em * SLACK, var=var, E_var=Evar * SLACK)
        ve = var + e
        Eve = Evar + U * ve
      else:
        mean, var = np.asarray(moving_mean, np.float64), np.asarray(moving_var, np.float64)
        Em = np.zeros(H)
        ve = var + e
        Eve = U * ve
      inv = 1.0 / np.sqrt(ve)
      Ei = np.where(Eve < ve / 2, RSQ * U * inv + Eve / (2 * np.maximum(ve - Eve, FLUSH) ** 1.5), np.inf) + FLUSH
      d = v - mean
      Ed = Ev + Em + U * np.abs(d) + FLUSH
      xh = d * inv
      Ex = Ed * inv + np.abs(d) * Ei + Ed * Ei + U * np.abs(xh) + FLUSH
      y = g * xh + be
      Ey = np.abs(g) * Ex + U * np.abs(y) + (U * np.abs(g * xh) if world else 0.0) + FLUSH   # (Sync: gamma v + beta is not spelled as an fma)
      r.update(inv=inv, E_inv=Ei * SLACK, ve=ve, xhat=xh, E_xhat=Ex * SLACK)
    if act == "relu":
      lk = float(f32(leak))
      h = np.maximum(y, 0.0) + lk * np.minimum(y, 0.0)
      L, K = (1.0, 2.0) if lk != 0.0 else ACT_FWD["relu"]
    else:
      h = ar.act_fwd(act, y)
      L, K = ACT_FWD[act]
    Eh = L * Ey + K * U * np.abs(h) + FLUSH
    out, Eo = h, Eh
    if mult is not None:
      m = np.asarray(mult, np.float64)
      out = h * m
      Eo = np.abs(m) * Eh + U * np.abs(out) + FLUSH
    r.update(y=y, E_y=Ey * SLACK, out=out, E_out=Eo * SLACK)
    return r


def backward(dslabs, out, xhat, inv_std=None, gamma=None, beta=None, batchnorm=True, training=True, leak=0.0, act="relu", mult=None, p=0.0,
             world=0):
  """dslabs [S][B][H]; out, xhat [B][H]; inv_std, gamma, beta [H]; mult [B][H] (the multipliers the forward applied; needed by the forms of
  the other activations) or p (the ReLU forms' scale).  Returns {dpre, dgamma, dbeta (dbias without BatchNorm), dy and their E_...}, plus the
  term sizes the kept-point rule uses (S_...)."""
  with np.errstate(all="ignore"):
    t = np.asarray(dslabs, np.float64)
    S, B, H = t.shape
    gsum = t.sum(0)
    Eg = gam(S) * np.abs(t).sum(0) + FLUSH
    o, xh = np.asarray(out, np.float64), np.asarray(xhat, np.float64)
    if act == "relu":
      keep = o > 0      # (false for a NaN)
      c = np.where(keep, float(drop_scale(p) if training else f32(1.0)), float(f32(leak)))
      dy = gsum * c
      Edy = np.abs(c) * Eg + U * np.abs(dy) + FLUSH
    else:
      y = np.asarray(gamma, np.float64) * xh + np.asarray(beta, np.float64) if batchnorm else xh
      a = ar.act_grad(act, ar.act_fwd(act, y))
      m = np.ones_like(y) if mult is None else np.asarray(mult, np.float64)
      Ea = ACT_CURV[act] * U * np.abs(y) + ACT_GRAD_OPS * U
      dy = gsum * m * a
      Edy = np.abs(m * a) * Eg + np.abs(gsum * m) * Ea + 2 * U * np.abs(dy) + FLUSH
    if not batchnorm:
      k = depth(B)
      s1 = dy.sum(0)
      return dict(dy=dy, dpre=dy, E_dpre=Edy * SLACK, dbias=s1, E_dbias=_tree_bound(np.abs(dy), Edy, k) * SLACK + FLUSH, S_dbias=np.abs(dy).sum(0),
                  S_dpre=np.abs(dy).max(0))
    W = max(world, 1)
    k = depth(B // W) + (W if world else 0)
    g, inv = np.asarray(gamma, np.float64), np.asarray(inv_std, np.float64)
    dx = dy * xh
    s1, s2 = dy.sum(0), dx.sum(0)
    E1 = _tree_bound(np.abs(dy), Edy, k) + FLUSH
    E2 = (Edy * np.abs(xh) + U * np.abs(dx)).sum(0) + gam(k) * (np.abs(dx) + Edy * np.abs(xh)).sum(0) + FLUSH
    gi = g * inv
    if training:
      tt = s1 + xh * s2
      Et = np.abs(xh) * E2 + E1 + U * np.abs(tt) + (U * np.abs(xh * s2) if world else 0.0)
      q = dy - tt / B
      Ep = (Et + U * np.abs(tt)) / B + (U * np.abs(tt) / B if world else 0.0)
      Eq = Ep + Edy + U * np.abs(q)
      dpre = gi * q
      Ed = np.abs(gi) * Eq + 2 * U * np.abs(dpre) + FLUSH
    else:
      dpre = dy * gi
      Ed = np.abs(gi) * Edy + 2 * U * np.abs(dpre) + FLUSH
    Sd = np.abs(gi) * (np.abs(dy).max(0) + (np.abs(dy).sum(0) + np.abs(xh).max(0) * np.abs(dx).sum(0)) / B)
    return dict(dy=dy, dpre=dpre, E_dpre=Ed * SLACK, dgamma=s2, E_dgamma=E2 * SLACK, dbeta=s1, E_dbeta=E1 * SLACK, S_dbeta=np.abs(dy).sum(0),
                S_dgamma=np.abs(dx).sum(0), S_dpre=Sd)


def kept(value, bound, scale):
  """the kept-point rule: finite bound, at most KEEP_REL of the component's scale (`scale` broadcasts over the rows)"""
  with np.errstate(all="ignore"):
    return np.isfinite(bound) & np.isfinite(value) & ((bound <= KEEP_REL * np.broadcast_to(scale, np.shape(value))) | (bound <= KEEP_ABS))


def fwd_scales(r, gamma=None, beta=None):
  """the component scales of forward()'s outputs, per column"""
  colmax = lambda a: np.abs(a).max(0)
  s = {}
  gb = (np.abs(np.asarray(gamma, np.float64)) + np.abs(np.asarray(beta, np.float64))) if gamma is not None else 0.0
  if "mean" in r:
    s["mean"] = np.maximum(np.abs(r["mean"]), colmax(r["v"]))
    s["var"] = r["ve"]
  if "inv" in r:
    s["inv"] = r["inv"]
    s["xhat"] = np.maximum(1.0, colmax(r["xhat"]))
  else:
    s["xhat"] = colmax(r["xhat"])
  s["out"] = np.maximum(colmax(r["out"]), gb if gamma is not None else colmax(r["y"]))
  return s


# ---- the float32 replay of the kernels' lines ---------------------------------------------------------------------------------------------
def _fma(a, b, c):
  return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)   # (a b is exact in float64)


def _slab_sum32(slabs, wide=False):
  t = np.asarray(slabs, f32)
  if not wide:
    acc = np.zeros(t.shape[1:], f32)
    for s in range(t.shape[0]):
      acc = acc + t[s]
    return acc
  part = np.zeros((16,) + t.shape[1:], f32)   # thread group sg sums the slabs sg, sg + 16, ...; then the 16 partial sums in order
  for s in range(t.shape[0]):
    part[s % 16] = part[s % 16] + t[s]
  acc = part[0].copy()
  for u in range(1, 16):
    acc = acc + part[u]
  return acc


def _col_tree32(x, fused_square=False):
  """bn_col_reduce over the rows of x [B][H]: a thread's rows r, r + 64, ... in order (fused_square: s = fma(x, x, s)), then the balanced
  tree over the 64 threads"""
  B, H = x.shape
  part = np.zeros((64, H), f32)
  for r0 in range(0, B, 64):
    blk = x[r0:r0 + 64]
    n = blk.shape[0]
    part[:n] = _fma(blk, blk, part[:n]) if fused_square else part[:n] + blk
  while part.shape[0] > 1:
    part = part[0::2] + part[1::2]
  return part[0]


def moving_update(moving, batch, momentum):
  """moving x momentum + batch x (1 - momentum): two products and a sum, not fused"""
  m = f32(momentum)
  return (np.asarray(moving, f32) * m + np.asarray(batch, f32) * (f32(1.0) - m)).astype(f32)


def replay_forward(slabs, gamma=None, beta=None, bias=None, moving_mean=None, moving_var=None, batchnorm=True, training=True, eps=1e-3, leak=0.0,
                   mult=None, wide=False, variance_divisor=None, eval_batch_var=False):
  """bn_act_fwd_body / bn_wide_fwd_body in float32, the ReLU forms.  variance_divisor / eval_batch_var: deliberately wrong formulas for the
  host test (B - 1 under the variance; evaluation mode normalising by the batch variance)."""
  with np.errstate(all="ignore"):
    v = _slab_sum32(slabs, wide)
    B = v.shape[0]
    r = {}
    if not batchnorm:
      if bias is not None:
        v = v + np.asarray(bias, f32)
      y = v
      r["xhat"] = v
    else:
      mean = _col_tree32(v) / f32(B)
      d = v - mean
      var = _col_tree32(d, fused_square=True) / f32(B if variance_divisor is None else variance_divisor)
      r.update(batch_mean=mean, batch_var=var)
      if not training:
        mean = np.asarray(moving_mean, f32)
        var = var if eval_batch_var else np.asarray(moving_var, f32)
      inv = (1.0 / np.sqrt((var + f32(eps)).astype(np.float64))).astype(f32)
      xh = (v - mean) * inv
      y = _fma(np.asarray(gamma, f32), xh, np.asarray(beta, f32))
      r.update(inv_std=inv, xhat=xh)
    h = np.maximum(y, f32(0))
    if leak != 0.0:
      h = h + f32(leak) * np.minimum(y, f32(0))
    r["out"] = h if mult is None else h * np.asarray(mult, f32)
    return r


def replay_backward(dslabs, out, xhat, inv_std=None, gamma=None, batchnorm=True, training=True, leak=0.0, p=0.0, wide=False, drop_s1=False):
  """bn_act_bwd_body / bn_wide_bwd_body in float32, the ReLU forms.  drop_s1: the deliberately wrong formula without its s1 term."""
  with np.errstate(all="ignore"):
    g = _slab_sum32(dslabs, wide)
    B = g.shape[0]
    o, xh = np.asarray(out, f32), np.asarray(xhat, f32)
    keep = o > 0
    dy = np.where(keep, g * (drop_scale(p) if training else f32(1.0)), g * f32(leak) if leak != 0.0 else f32(0)).astype(f32)
    s1 = _col_tree32(dy)
    if not batchnorm:
      return dict(dpre=dy, dbias=s1)
    s2 = _col_tree32((dy * xh).astype(f32))
    gi = np.asarray(gamma, f32) * np.asarray(inv_std, f32)
    if training:
      t = _fma(xh, s2, np.zeros_like(s1) if drop_s1 else s1)
      dpre = gi * _fma(-t, f32(1.0) / f32(B), dy)
    else:
      dpre = dy * np.asarray(gamma, f32) * np.asarray(inv_std, f32)
    return dict(dpre=dpre.astype(f32), dgamma=s2, dbeta=s1)


# ---- the column families of the edge grid -------------------------------------------------------------------------------------------------
#          name           values of the column                                   gamma   beta
FAMILIES = (("normal", 1.0, 0.1), ("const0", 1.0, 0.5), ("const_a", 1.0, -0.25), ("const_b", 1e3, 0.0), ("mean1e3", 1.0, 0.0),
            ("spread1e-3", 1.0, 0.0), ("outlier", 1.0, 0.05), ("tiny", 1.0, 0.0), ("huge18", 1.0, 0.0), ("huge15", 1.0, 0.0),
            ("gamma0", 0.0, 0.3), ("gamma_neg", -1.0, 0.0), ("gamma_small", 1e-3, 0.0), ("gamma_big", 1e3, 0.0), ("beta_pos", 1.0, 2.0),
            ("beta_neg", 1.0, -2.0), ("zero_p0", 1.0, 0.0), ("zero_m0", -1.0, -0.0), ("spread37", 1.0, 0.0), ("normal_b", 0.5, -0.1))
CONSTANT = {"const0": 0.0, "const_a": 0.375, "const_b": -2.0, "zero_p0": 0.0, "zero_m0": 0.0}
DOUT_FAMILIES = ("normal", "cancel", "single_row")


def family_of(col, H, shift=0):
  """the family of column `col` of an H-column launch: every family at H >= 20; at H = 5 every fourth, so that shifts 0 .. 3 cover all"""
  n = len(FAMILIES)
  return FAMILIES[(col + shift) % n] if H >= n else FAMILIES[(4 * col + shift) % n]


def dout_family_of(name):
  return "cancel" if name in ("gamma0", "beta_pos", "mean1e3") else "single_row" if name in ("outlier", "gamma_neg") else "normal"


def make_columns(B, H, S, seed, shift=0):
  """The edge grid as slabs [S][B][H] float32 plus gamma, beta [H] float32 and the family names.  A column's values are split over the
  slabs with positive weights (the constant families: the value in slab 0, zeros behind it, so that every float32 sum is exact); the
  normal families are sums of S independent slabs."""
  rng = np.random.default_rng(seed)
  t = np.zeros((S, B, H), f32)
  gamma, beta, names = np.zeros(H, f32), np.zeros(H, f32), []
  w = rng.dirichlet(np.ones(S) * 4.0, size=(B,)).T.astype(np.float64)   # [S][B]
  for c in range(H):
    name, g, b = family_of(c, H, shift)
    names.append(name)
    gamma[c], beta[c] = g, b
    z = rng.standard_normal(B)
    if name in CONSTANT:
      t[0, :, c] = CONSTANT[name]
      continue
    if name in ("normal", "normal_b", "gamma0", "gamma_neg", "gamma_small", "gamma_big", "beta_pos", "beta_neg"):
      t[:, :, c] = rng.standard_normal((S, B)) / np.sqrt(S)
      continue
    col = {"mean1e3": 1e3 + z, "spread1e-3": 1.0 + 1e-3 * z, "tiny": 1e-30 * z, "huge18": 1e18 * np.clip(z, -3, 3), "huge15": 1e15 * z,
           "spread37": 37.0 * z, "outlier": np.zeros(B)}[name]
    if name == "outlier":
      col[B // 2] = 1e6
    t[:, :, c] = (w * col[None, :]).astype(f32)
  return t, gamma, beta, names


def make_dout(B, names, S, seed):
  """d out slabs [S][B][H] for the columns `names` (make_columns'): unit normals, the cancelling and the single-row families"""
  rng = np.random.default_rng(seed)
  H = len(names)
  t = (rng.standard_normal((S, B, H)) / np.sqrt(S)).astype(f32)
  for c in range(H):
    fam = dout_family_of(names[c])
    if fam == "cancel":      # +-1e4 pairs (slab 0) under unit noise: the column sum of dy cancels where every row is kept
      t[0, :, c] += np.where(np.arange(B) % 2 == 0, 1e4, -1e4).astype(f32) * (np.arange(B) < B - B % 2)
    elif fam == "single_row":
      live = np.zeros(B, f32)
      live[B // 3] = 1.0
      t[:, :, c] *= live[None, :]
  return t


# ---- comparing a result with the reference ------------------------------------------------------------------------------------------------
def fwd_keep(r, gamma=None, beta=None):
  """{output name: mask of asserted points} of forward()'s result: the kept-point rule, within the columns that are asserted at all"""
  s = fwd_scales(r, gamma, beta)
  return {k: kept(r[k], r["E_" + k], s[k]) & r["asserted"] for k in s if k in r}


def bwd_keep(b):
  return {k: kept(b[k], b["E_" + k], b["S_" + k]) for k in ("dpre", "dgamma", "dbeta", "dbias") if k in b}


def worst(got, ref, bound, keep):
  """the largest |got - ref| / bound over the kept points; inf if a kept point of `got` is not finite (a NaN fails every check)"""
  got = np.asarray(got, np.float64)
  with np.errstate(all="ignore"):
    ratio = np.where(keep, np.where(np.isfinite(got), np.abs(got - ref) / np.maximum(bound, 1e-300), np.inf), 0.0)
  return float(ratio.max()) if ratio.size else 0.0


def dropped_by_family(names, keep):
  """{family: (dropped, total)} of a [B][H] or [H] mask"""
  k = np.atleast_2d(keep)
  out = {}
  for c, n in enumerate(names):
    d, t = out.get(n, (0, 0))
    out[n] = (d + int((~k[:, c]).sum()), t + k.shape[0])
  return out


def composed_extra(r, b, gamma):
  """What the forward's own errors (forward()'s r: E_xhat, E_inv) add to the backward's outputs when the backward of the computed forward
  is compared with backward(forward(.)) in float64 (b), on columns where the mask is the same (every |y| above E_y): dy and s1 do not
  move; |delta s2| <= sum |dy| E_x; dpre = gamma inv q, q = dy - (s1 + xhat s2) / B moves by the product rule, error products kept."""
  with np.errstate(all="ignore"):
    B = r["xhat"].shape[0]
    dy, xh, Ex = np.abs(b["dy"]), np.abs(r["xhat"]), r["E_xhat"]
    ds2 = (dy * Ex).sum(0)
    dq = (Ex * np.abs(b["dgamma"]) + xh * ds2 + Ex * ds2) / B
    q = b["dy"] - (b["dbeta"] + r["xhat"] * b["dgamma"]) / B
    g = np.abs(np.asarray(gamma, np.float64))
    return dict(dpre=g * (r["E_inv"] * np.abs(q) + (r["inv"] + r["E_inv"]) * dq) * SLACK, dgamma=ds2 * SLACK, dbeta=np.zeros_like(ds2))
