"""float64 reference of the scVI gene head (sisua_amd/csrc/smx_scvi.hip: scvi_head_train_kernel, scvi_head_fwd / bwd_reg_kernel,
scvi_head_fwd / bwd_vec_kernel), the float32 error bounds of the kernels' formulas, and the inputs tests/test_gpu_scvi_head.py launches.
The pattern is tests/likelihood_grad_ref.py's: NumPy float64 only, an independent restatement FROM THE FLOAT32 INPUTS of a launch.

THE CHAIN, per cell (a row of G genes; raw_0, raw_1, raw_2 the planes of the raw head output, x the counts, l the library latent):
  a_g = raw_0g - max_g raw_0,  e_g = exp(a_g),  S = sum_g e_g,  rho_g = e_g / S                                 (softmax with the row maximum)
  el = exp(clip(l, 0, clip_library)),  rate_g = el clip(rho_g, LO, HI),  theta_g = exp(raw_1g),  gate_g = raw_2g
      (LO = float32(1e-7), HI = float32(1) - float32(1e-7) = 1 - 2^-23: the kernels' float32 constants)
  (d0, d1, d2) = likelihood_grad_ref.grad_elem(kind, x, [rate, theta, gate], direct=True);  dd = d0 grad_scale
  inside_g = LO < rho_g < HI;  s = sum_g dd el inside rho;  dlh = sum_g dd rate
  d raw_0 = rho (dd el inside - s),  d raw_1 = d1 grad_scale theta,  d raw_2 = d2 grad_scale,  dl = dlh if 0 < l < clip_library else 0
  llk_part = sum_g log p(x_g) + lgamma(x_g + 1)                                                                  (without the count constant)
  library latent: latent_terms_ref.lib_terms(mu_l, s_l, eps, prior); d mu_l = dl + kls dKL/dmu, d s_l = dl eps sigmoid(x) + kls dKL/draw
The rate and the dispersion stay float64 through the likelihood (`exact=True` of the two reference modules): the kernel's float32 copies of
them are inputs with an error, carried by `rel_in`.

THE BOUNDS.  u = 2^-24; first order, ABSOLUTE, in term sizes, by likelihood_grad_ref's rule.  A rounding 1 (a correctly rounded division
too: hipcc's default), v_exp / v_rcp and expf 2, fexp's argument 2 |x| u.  Written from the kernels' lines before any output was looked at.

  quantity       formula in the kernels, operations                                                          bound (in u)
  e_g            a = raw - max: 1 rounding, |a| in the exponent; fexp 2 + 2 |a|.  a = 0 (the row's maximum):    rel_e = 2 + 3 |a|  (0 at a = 0)
                 0 x log2(e) and 2^0 are exact
  S              positive terms: relative.  n_add additions on the longest chain of a term, read off the        rel_S = sum_g rel_e e_g / S + min(n_add, G - 1)
                 instance (N_ADD below); an addition of 0 is exact and G live terms have G - 1 additions of
                 two non-zero operands, so no term passes more than min(n_add, G - 1) roundings
  rho            1.f / S 1, the product 1                                                                       rel_rho = rel_e + rel_S + 2;  E_rho = rel_rho rho + 2 x 2^-126 / u
                 (e_g below 2^-126 leaves v_exp as 0; the product's own underflow)
  el             expf 2; the clip of a float32 l against float32 ends is exact.  Where l itself carries an      rel_el = 2 (+ E_l / u inside the clip)
                 error E_l (the row with a random library head) it is the exponent's
  rate           el clip(rho): the product 1; rho's error unless the gene is decided clipped                    rel_rate = rel_el + 1 (+ rel_rho)
  theta          fexp(raw_1)                                                                                    rel_th = 2 + 2 |raw_1|
  d0, d1, d2     likelihood_grad_ref.grad_elem_bound(..., direct=True, rel_in=(rel_rate, rel_th)): E_0, E_1, E_2
  dd             d0 grad_scale 1                                                                                E_dd = |gs| E_0 + |dd|
  d raw_1        (d1 gs) theta: 2 roundings, theta's error                                                      |gs theta| E_1 + (2 + rel_th) |d raw_1|
  d raw_2        d2 gs 1                                                                                        |gs| E_2 + |d raw_2|
  s              term t = dd el inside rho: 2 roundings (inside is 0 or 1), the three factors' errors;          E_s = sum_g (el rho E_dd + (rel_el + rel_rho + 2) |t|)
                 a sum of both signs: n_add + 8 roundings of the sum of sizes; an undecided gene's term           + (min(n_add, G - 1) + 8) sum_g |t| + sum_undecided |rho dd el|
                 may be there or not
  dlh (dl)       term dd rate: 1 rounding                                                                       sum_g (rate E_dd + (rel_rate + 1) |dd rate|) + (min(n_add, G - 1) + 8) sum_g |dd rate|
  d raw_0        rho (T - s), T = dd el inside: E_T = el E_dd + (rel_el + 1) |dd el|; the difference and the    rho (E_T + E_s) + rel_rho |d raw_0| + 2 (|rho dd el| + |rho s|) + 2^-126 (1 + 2 |T - s|) / u
                 product 1 each in the sizes |rho dd el| and |rho s|; rho's relative and absolute error
  llk_part       likelihood_grad_ref.row_sum_bound(..., n_add, direct=True, rel_in=...), and one more rounding of the result
  planes (fwd)   rate, theta as above, gate exact, rho_raw E_rho; columns G .. Gp exactly 0
  bwd entry      its inputs (planes, dplanes, rho_raw, l) are float32 numbers, the float64 reference rounded: inside is decided by the float32
                 comparison, rel_rho = 0, E_dd = 0, rate exact: E_s = sum 2 |t| + (n + 8) sum |t|, dlh: sum |t| + (n + 8) sum |t|,
                 d raw_0: rho ((rel_el + 1) |dd el| + E_s) + 2 (|rho dd el| + |rho s|), d raw_1 = d1 theta: 1, d raw_2 = d2: 0
  library        latent_terms_ref.lib_bounds for sigma, l, KL; d mu_l = dl + kls (mu - mp) / vp: E_dl + |kls| (E_dmu + |dmu|) + |dl| + |kls dmu|;
                 d s_l = (dl eps + kls (sigma / vp - 1 / sigma)) sgm (x >= -20 only here): (E_dl |eps| + (9 + 3 |x|) |dl eps|) sgm + |kls| E_draw
                 + 3 (|dl eps sgm| + |kls draw|).  With a random head mu_l, s_l are dot products of Kl terms by fma: ceil(Kl / 64) on a lane, six
                 butterfly steps, the bias: E_mu = (ceil(Kl / 64) + 7) (sum |h w| + |b|), carried through the exact partial derivatives.

N_ADD, read off the launchers (Gp = G rounded up to 32): 4 NV serial additions of a thread, six butterfly steps of wave_sum, then 3 (four waves),
7 (eight waves) or 15 (block_sum16) additions over the waves.
  train   Gp <= 2048 NV 2: 17;  <= 4096 NV 4: 25;  <= 8192 NV 8: 41;  <= 16384 NV 8, 512 threads: 45;  <= 20480 NV 10, 512 threads: 53
  fwd/bwd Gp <= 2048: 17;  <= 4096: 25;  <= 8192: 41;  above (vec): 4 ceil(Gp / 4096) + 21

TWO CONDITIONS, properties of the reference alone.
  grid      likelihood_grad_ref.grad_in_range at the reference planes, and el, S, theta normal float32 numbers.  (l above 88 overflows expf in
            float32, here as in the original model: outside the condition.)  An element that fails is not held elementwise; its terms stay in the
            row sums with the bound the table gives them.
  undecided |rho - LO| < E_rho or |rho - HI| < E_rho: both values of `inside` are accepted for the gene's own d raw_0, and |rho dd el| of the
            row's undecided genes is in E_s.  (Strictly inside the bound: a single live gene has rho = 1 with E_rho = 2 u = 1 - HI, and every
            kernel gives exactly 1.)  l within E_l of 0 or clip_library would be undecided too; the cases have none (asserted).
In every launch at most a tenth of the live elements may fail the grid condition and at most 1 % may be undecided (tests/test_scvi_head_host.py
asserts both for every launch of the GPU file).
"""
import numpy as np
from scipy.special import expit, gammaln

from tests import latent_terms_ref as T
from tests import likelihood_grad_ref as L
from tests.plane_stat_ref import CYCLE, F32_MAX, F32_MIN, SCVI_AXES, U

FLUSH = F32_MIN / U
LO = float(np.float32(1e-7))
HI = float(np.float32(1.0) - np.float32(1e-7))
KINDS = ("nbd", "zinbd")
WIDTHS = (1, 3, 37, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 20449, 20480, 20481)
TRAIN_MAX_GP = 20480
KLS = float(np.float32(0.37))
S_RAW = float(np.float32(0.3))
LDL = 8
LIB_KL = (1, 63, 65, 257)


def round_up(v, m):
  return (v + m - 1) // m * m


def train_instance(Gp):
  """(NV, threads) of launch_scvi_head_train, None where it refuses"""
  for top, inst in ((2048, (2, 256)), (4096, (4, 256)), (8192, (8, 256)), (16384, (8, 512)), (20480, (10, 512))):
    if Gp <= top:
      return inst
  return None


def sep_instance(Gp):
  """NV of the register form of launch_scvi_head_fwd / _bwd, 0 for the vec form"""
  return 2 if Gp <= 2048 else 4 if Gp <= 4096 else 8 if Gp <= 8192 else 0


def n_add_train(Gp):
  nv, nt = train_instance(Gp)
  return 4 * nv + 6 + (3 if nt == 256 else 7)


def n_add_sep(Gp):
  nv = sep_instance(Gp)
  return 4 * nv + 6 + 3 if nv else 4 * -(-Gp // 4096) + 6 + 15


def _normal32(v):
  a = np.abs(v)
  return np.isfinite(a) & (a >= F32_MIN) & (a < F32_MAX)


# ---- the softmax and the activated planes --------------------------------------------------------------------------------------------
def forward(raw, l, clip, n_add, e_l=0.0):
  """raw [B, k, G] float32 (live columns), l [B] the library latent (float64 value), e_l [B] its absolute error in the kernel (0: pinned).
  dict of float64 arrays: rho, rate, theta, gate, el, S and the relative / absolute bounds in u (rel_*) or absolute (E_*)"""
  raw = np.asarray(raw, np.float32).astype(np.float64)
  B, k, G = raw.shape
  l = np.asarray(l, np.float64).reshape(B)
  clip = float(np.float32(clip))
  e_l = np.broadcast_to(np.asarray(e_l, np.float64), (B,))
  a = raw[:, 0] - raw[:, 0].max(-1, keepdims=True)
  e = np.exp(a)
  S = e.sum(-1, keepdims=True)
  rho = e / S
  n_eff = min(n_add, G - 1)
  rel_e = np.where(a == 0, 0.0, 2.0 + 3.0 * np.abs(a))
  rel_S = (rel_e * e).sum(-1, keepdims=True) / S + n_eff
  rel_rho = rel_e + rel_S + 2.0
  E_rho = (rel_rho * rho + 2.0 * FLUSH) * U
  l_in = (l > 0) & (l < clip)
  l_und = (np.abs(l) <= e_l) | (np.abs(l - clip) <= e_l)
  l_und &= e_l > 0
  el = np.exp(np.clip(l, 0.0, clip))[:, None]
  rel_el = (2.0 + np.where(l_in, e_l / U, 0.0))[:, None]
  inside = (rho > LO) & (rho < HI)
  und = (np.abs(rho - LO) < E_rho) | (np.abs(rho - HI) < E_rho)
  rate = el * np.clip(rho, LO, HI)
  rel_rate = rel_el + 1.0 + np.where(inside | und, rel_rho, 0.0)
  theta = np.exp(raw[:, 1])
  rel_th = 2.0 + 2.0 * np.abs(raw[:, 1])
  gate = raw[:, 2] if k == 3 else np.zeros_like(theta)
  return dict(rho=rho, E_rho=E_rho, rel_rho=rel_rho, S=S, el=el, rel_el=rel_el, inside=inside, und=und, rate=rate, rel_rate=rel_rate,
              E_rate=(rel_rate * rate + FLUSH) * U, theta=theta, rel_th=rel_th, E_theta=(rel_th * theta + FLUSH) * U, gate=gate, l_in=l_in,
              l_und=l_und, n_eff=n_eff)


# ---- the whole head: likelihood, backward pass, row sums ---------------------------------------------------------------------------------
def head(kind, raw, x, l, clip, grad_scale, n_add, e_l=0.0):
  """the training launch's gene outputs and their bounds (absolute).  draw [B, k, G] with draw_alt (an undecided gene's other value of
  `inside`; elsewhere equal) and E_draw; llk, E_llk; dl, E_dl [B]; keep [B, G] the grid condition; und [B, G]; f = forward()'s dict"""
  f = forward(raw, l, clip, n_add, e_l)
  x = np.asarray(x, np.float32).astype(np.float64)
  k = np.asarray(raw).shape[1]
  gs = float(np.float32(grad_scale))
  planes = [f["rate"], f["theta"], f["gate"]][:k]
  rel_in = (f["rel_rate"], f["rel_th"])
  g = L.grad_elem(kind, x, planes, direct=True, exact=True)
  eb = L.grad_elem_bound(kind, x, planes, direct=True, rel_in=rel_in, exact=True)
  keep = L.grad_in_range(kind, x, planes, direct=True, exact=True) & _normal32(f["el"]) & _normal32(f["S"]) & _normal32(f["theta"])
  rho, el, rel_el, rel_rho, rate, theta = f["rho"], f["el"], f["rel_el"], f["rel_rho"], f["rate"], f["theta"]
  ins, und, n8 = f["inside"].astype(np.float64), f["und"], f["n_eff"] + 8.0
  dd = g[0] * gs
  E_dd = abs(gs) * eb[0] + U * np.abs(dd) + F32_MIN
  o1 = g[1] * gs * theta
  E_o1 = np.abs(gs * theta) * eb[1] + (2.0 + f["rel_th"]) * U * np.abs(o1) + F32_MIN
  o2 = g[2] * gs
  E_o2 = abs(gs) * eb[2] + U * np.abs(o2) + F32_MIN
  full = dd * el * rho                       # (the term of s were the gene inside)
  t_s = full * ins
  E_ts = el * rho * ins * E_dd + (rel_el + rel_rho + 2.0) * U * np.abs(t_s)
  s = t_s.sum(-1, keepdims=True)
  E_s = (E_ts.sum(-1, keepdims=True) + n8 * U * np.abs(t_s).sum(-1, keepdims=True) + (np.abs(full) * und).sum(-1, keepdims=True) + F32_MIN)
  t_d = dd * rate
  E_td = rate * E_dd + (f["rel_rate"] + 1.0) * U * np.abs(t_d)
  dlh = t_d.sum(-1)
  E_dlh = E_td.sum(-1) + n8 * U * np.abs(t_d).sum(-1) + F32_MIN
  any_in = np.maximum(ins, und.astype(np.float64))
  E_T = (el * E_dd + (rel_el + 1.0) * U * np.abs(dd * el)) * any_in
  o0 = rho * (dd * el * ins - s)
  o0_alt = np.where(und, rho * (dd * el * (1.0 - ins) - s), o0)
  size = np.abs(full) * any_in + np.abs(rho * s)
  E_o0 = (rho * (E_T + E_s) + rel_rho * U * np.maximum(np.abs(o0), np.abs(o0_alt)) + 2.0 * U * size
          + F32_MIN * (1.0 + 2.0 * (np.abs(dd * el) * any_in + np.abs(s))))
  ref, bound = L.row_sum_bound(kind, x, planes, f["n_eff"], direct=True, double_const=True, rel_in=rel_in, exact=True)
  llk = ref + gammaln(x + 1.0).sum(-1)
  draw = np.stack([o0, o1, o2][:k], axis=1)
  return dict(f=f, draw=draw, draw_alt=np.stack([o0_alt, o1, o2][:k], axis=1), E_draw=np.stack([E_o0, E_o1, E_o2][:k], axis=1), dd=dd, s=s[:, 0],
              E_s=E_s[:, 0], llk=llk, E_llk=bound + U * np.abs(llk), dl=np.where(f["l_in"], dlh, 0.0), E_dl=np.where(f["l_in"], E_dlh, 0.0),
              keep=keep, und=und, dplanes=np.stack([dd, g[1] * gs, o2][:k], axis=1))


def backward_entry(planes, dplanes, rho, l, clip, n_add):
  """the separate backward launch on ITS float32 inputs [B, k, G], [B, k, G], [B, G], [B]: draw, E_draw [B, k, G]; dl, E_dl [B]"""
  pl, dp = (np.asarray(v, np.float32).astype(np.float64) for v in (planes, dplanes))
  rho = np.asarray(rho, np.float32).astype(np.float64)
  l = np.asarray(l, np.float32).astype(np.float64)
  clip = float(np.float32(clip))
  B, k, G = pl.shape
  n8 = min(n_add, G - 1) + 8.0
  el = np.exp(np.clip(l, 0.0, clip))[:, None]
  ins = ((rho > LO) & (rho < HI)).astype(np.float64)
  T_ = dp[:, 0] * el * ins
  t_s = T_ * rho
  s = t_s.sum(-1, keepdims=True)
  E_s = (2.0 + 2.0 + n8) * U * np.abs(t_s).sum(-1, keepdims=True) + F32_MIN            # (el's 2 and the two products; the sum)
  t_d = dp[:, 0] * pl[:, 0]
  l_in = (l > 0) & (l < clip)
  E_dl = (1.0 + n8) * U * np.abs(t_d).sum(-1) + F32_MIN
  o0 = rho * (T_ - s)
  E_o0 = rho * (3.0 * U * np.abs(T_) + E_s) + 2.0 * U * (np.abs(rho * T_) + np.abs(rho * s)) + F32_MIN
  o = [o0, dp[:, 1] * pl[:, 1]] + ([dp[:, 2]] if k == 3 else [])
  E = [E_o0, U * np.abs(o[1]) + F32_MIN] + ([np.zeros_like(o0)] if k == 3 else [])
  return dict(draw=np.stack(o, axis=1), E_draw=np.stack(E, axis=1), dl=np.where(l_in, t_d.sum(-1), 0.0), E_dl=np.where(l_in, E_dl, 0.0))


# ---- the library latent --------------------------------------------------------------------------------------------------------------
def library(mu, sraw, eps, mp, vp, kls, dl, E_dl, e_mu=0.0, e_sraw=0.0):
  """the fused copy of the library latent: sig, l, kl, dlatl0, dlatl1 and their absolute bounds E_*; e_mu, e_sraw: absolute errors of
  (mu_l, s_l) in the kernel (a random head's dot products), carried through the exact partial derivatives"""
  mu, sraw, eps, mp, vp, dl, E_dl = (np.asarray(v, np.float64) for v in (mu, sraw, eps, mp, vp, dl, E_dl))
  t, b = T.lib_terms(mu, sraw, eps, mp, vp), T.lib_bounds(mu, sraw, eps, mp, vp)
  x, sg = t["x"], t["sigma"]
  assert np.all(x >= T.TAIL), "the cases keep the library scale above SMX_SIGMA_TAIL"
  sgm = expit(x)
  o = dict(sig=sg, E_sig=b["sigma"] + e_sraw * sgm, l=t["z"], E_l=b["z"] + e_mu + e_sraw * sgm * np.abs(eps),
           kl=t["kl"], E_kl=b["kl"] + e_mu * np.abs(t["dmu"]) + e_sraw * np.abs(t["draw"]))
  o["dlatl0"] = dl + kls * t["dmu"]
  o["E_dlatl0"] = E_dl + abs(kls) * (b["dmu"] + U * np.abs(t["dmu"]) + e_mu / vp) + U * (np.abs(dl) + np.abs(kls * t["dmu"])) + F32_MIN
  A = dl * eps + kls * (sg / vp - 1.0 / sg)
  dA = kls * (1.0 / vp + 1.0 / (sg * sg)) * sgm
  o["dlatl1"] = dl * eps * sgm + kls * t["draw"]
  o["E_dlatl1"] = ((E_dl * np.abs(eps) + (9.0 + 3.0 * np.abs(x)) * U * np.abs(dl * eps)) * sgm + abs(kls) * b["draw"]
                   + 3.0 * U * (np.abs(dl * eps * sgm) + np.abs(kls * t["draw"])) + e_sraw * np.abs(dA * sgm + A * sgm * (1.0 - sgm)) + F32_MIN)
  return o


def dot_bound(h, w, b, Kl):
  """(value, absolute bound) of the library head's column: sum_k h_k w_k + b by fma on 64 lanes, six butterfly steps, the bias"""
  h, w = np.asarray(h, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
  v = h @ w + float(b)
  return v, (-(-Kl // 64) + 7.0) * U * (np.abs(h) @ np.abs(w) + abs(float(b))) + F32_MIN


# ---- the launches of the GPU file ----------------------------------------------------------------------------------------------------
def _counts(rng, G):
  return np.minimum(rng.poisson(rng.choice([0.3, 3.0, 12.0], size=G)), 60).astype(np.float32)


def _moderate(rng, G):
  return (2.0 * rng.standard_normal(G)).astype(np.float32)


def _spike(rng, G):
  r = (0.5 * rng.standard_normal(G)).astype(np.float32)
  at = G // 3
  r[at] = np.float32(np.delete(r, at).max() + 30.0) if G > 1 else r[at]
  return r


def _straddle(G, k_hi, low_ks):
  """raw_0 = log of a row of targets: gene 0 at HI (1 - 2^-k_hi), genes 1 .. at LO (1 +- 2^-k) for k in low_ks, the rest sharing what is left"""
  tgt = np.zeros(G)
  tgt[0] = HI * (1.0 - 2.0 ** -k_hi)
  low = [LO * (1.0 + sgn * 2.0 ** -k) for k in low_ks for sgn in (1.0, -1.0)]
  tgt[1:1 + len(low)] = low
  rest = 1.0 - tgt.sum()
  n_rest = G - 1 - len(low)
  assert rest > 0 and n_rest > 0
  tgt[1 + len(low):] = rest / n_rest
  return np.log(tgt).astype(np.float32)


def _dispgate(rng, G):
  """(raw_1, raw_2, x): SCVI_AXES x CYCLE, one combination per gene in a stride through the product, a moderate filler behind them"""
  d, g, c = (a.ravel() for a in np.meshgrid(np.array(SCVI_AXES[0]), np.array(SCVI_AXES[1]), np.array(CYCLE), indexing="ij"))
  n = d.size
  at = (np.arange(min(G, n)) * 277) % n          # (277 is prime to 784 = 8 x 14 x 7)
  r1, r2, x = (0.4 * rng.standard_normal(G)).astype(np.float32), (0.8 * rng.standard_normal(G)).astype(np.float32), _counts(rng, G)
  r1[:at.size], r2[:at.size], x[:at.size] = d[at], g[at], c[at]
  return r1, r2, x


def launches(G, kind):
  """the launches of one width: a list of dict(name, clip, raw [B, k, G], x [B, G], l [B], labels [B]) float32.  B = 8 up to G = 4128, 4
  above.  Rows: moderate, spike, flat, straddle (five rows: the HI side needs a row per distance), dispersion-and-gate, the library edges.
  Narrower than 12 genes a row cannot straddle and narrower than 128 a spike alone passes the undecided cap: moderate rows of another seed
  stand there; under 512 genes the straddle rows keep the decided neighbours only (k <= 16)."""
  k = 3 if kind == "zinbd" else 2
  B = 8 if round_up(G, 32) <= 4128 else 4
  rng = np.random.default_rng(1000 + G)
  ks = (4, 8, 12, 16, 20) if G >= 512 else (4, 8, 12, 16)
  rows = []           # (label, raw_0, raw_1, raw_2, x, l, clip)

  def add(label, r0, l, clip=1e3, special=None):
    r1, r2, x = special if special is not None else ((0.4 * rng.standard_normal(G)).astype(np.float32), (0.8 * rng.standard_normal(G)).astype(np.float32), _counts(rng, G))
    rows.append((label, r0, r1, r2, x, np.float32(l), clip))
  add("moderate", _moderate(rng, G), 8.0)
  add("spike", _spike(rng, G) if G >= 128 else _moderate(rng, G), 8.0)
  add("flat", np.full(G, np.float32(0.75)), 8.0)
  for i, kh in enumerate((4, 8, 12, 16, 20)):
    ok = G >= 12 and kh in ks
    add(f"straddle {kh}" if ok else "moderate", _straddle(G, kh, ks if i == 0 else ()) if ok else _moderate(rng, G), 8.0)
  add("dispersion and gate", _moderate(rng, G), 5.0, special=_dispgate(rng, G))
  for lv in (-3.0, 0.0, 11.0):
    add(f"library edge l {lv:g}", _moderate(rng, G), lv)
  for lv in (5.5, 6.0, 7.0, 3.0):
    add(f"library edge l {lv:g} clip 6", _moderate(rng, G), lv, clip=6.0)
  out = []
  for clip in (1e3, 6.0):
    sel = [r for r in rows if r[6] == clip]
    while len(sel) % B:                       # (whole launches: moderate rows fill the last one)
      sel.append(("moderate", _moderate(rng, G), (0.4 * rng.standard_normal(G)).astype(np.float32), (0.8 * rng.standard_normal(G)).astype(np.float32),
                  _counts(rng, G), np.float32(2.0), clip))
    for i in range(0, len(sel), B):
      part = sel[i:i + B]
      raw = np.stack([np.stack([r[1], r[2], r[3]][:k]) for r in part]).astype(np.float32)
      out.append(dict(name=f"G {G} {kind} clip {clip:g} rows {i}..{i + B - 1}", clip=clip, raw=raw, x=np.stack([r[4] for r in part]),
                      l=np.array([r[5] for r in part], np.float32), labels=[r[0] for r in part]))
  return out


def library_rows(B):
  """(library [B, 2], the prior's mean and variance per cell)"""
  return np.stack([7.0 + 0.25 * np.arange(B), 0.3 + 0.05 * np.arange(B)], axis=1).astype(np.float32)


def padded(a, Gp):
  """[..., G] -> [..., Gp] with zeros behind"""
  a = np.asarray(a)
  out = np.zeros(a.shape[:-1] + (Gp,), a.dtype)
  out[..., :a.shape[-1]] = a
  return out


def caps(h):
  """(share of live elements failing the grid condition, share undecided) of a head() result"""
  return float((~h["keep"]).mean()), float(h["und"].mean())
