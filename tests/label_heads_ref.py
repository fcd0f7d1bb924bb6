"""float64 reference of the label heads' launch (label_loss_kernel and label_tril_kernel of sisua_amd/csrc/smx_loss.hip; the entry
smx_k_label_loss), per ELEMENT -- one label dimension of one cell, before the sum over the dimensions --, the float32 error bounds of
the kernels' formulas, and the edge grid both are taken on.  The six kinds that are one count_elem / bernoulli / normal evaluation
('nb', 'nbd', 'zinb', 'zinbd', 'bernoulli', 'normal') and every mixture component are tests/likelihood_grad_ref.py's values and bounds,
imported; this module adds the mixtures over them, 'onehot' and 'mixtril'.  tests/test_label_heads_host.py holds all of it to
oracle.sisua_oracle.label_llk, to mpmath, and to a float32 replay of the kernels' own operations.

WELL-CONDITIONED FORMS (pi = softmax of the mixture logits a, e_c the component log densities):
  * log sum_c pi_c exp(e_c) is logaddexp over (a_c - lse(a)) + e_c;
  * D_c = sum_k pi_k exp(e_k - e_c) (terms of one sign), resp_c = pi_c / D_c;
  * resp_c - pi_c = pi_c (exp(e_c - lse_e) - 1) = -pi_c S_c / D_c, S_c = sum_{k != c} pi_k expm1(e_k - e_c): no difference of the two
    near-equal numbers resp and pi (a logit pattern with all components alike has resp - pi ~ 0 to the last bit of each);
  * 'onehot': d_p = y_p - s_p sum_k y_k = sum_{k != p} (y_p s_k - s_p y_k), s = softmax: at a logit 80 ahead and a one-hot y on it,
    1 - s_p is e^-80, nothing of which survives in 1 - s_p formed directly;
  * 'mixtril': both solves by substitution in float64 (a condition number of 1e4 leaves 12 digits).

THE BOUNDS.  Written as likelihood_grad_ref's table: u = 2^-24, ABSOLUTE, in term sizes -- (operations of a term) x |term|, an input's
error through its exact partial, one rounding of the sum of the sizes per addition -- and composed from logprob_elem_bound /
grad_elem_bound.  The label branches call the device library's expf, logf and lgammaf, not fexp / flog.  Their accuracy: build.py
compiles with -O3 and no fast-math flag, so the calls are the library's full-accuracy functions, not the native_ forms.  No figure for
them ships with the toolchain's files, so each was measured once, by itself, against the host's double functions on the arguments these
kernels produce (tools/dev/libm_probe.hip, an MI355X, ROCm's device library as build.py links it), and enters the table with a margin of
2 x for the arguments between the sampled ones; 1 ulp of a result is at most 2 u of it:
  expf     [-104, 0], 2^22 points and -2^-k                     1.000 ulp measured   ->  2 ulp,   EXPF = 4 u
  logf     [1, 70], 2^22 points                                 2.303 ulp measured   ->  4.6 ulp, LOGF = 10 u
  lgammaf  y + 1 of every integer y = 0 .. 20000                2.781 ulp measured   ->  5.6 ulp: inside the 6 ulp = 12 u (floor 1 u at the
           zeros y = 0, 1) that plane_stat_ref's table already carries, LGAMMAF = 12 u; the worst error is 0.277 of that term (y = 265)
           real y: 2^20 points of [0, 20000], 2^18 of [0, 3]    1.123 of the term at y = 1.17, 112 ulp of a result near the zero at y = 1:
           the term holds for COUNTS only.  Every count of this grid and of likelihood_grad_ref's is an integer; the kinds with real
           targets ('normal', 'mixgauss', 'mixtril', soft 'onehot' rows) have no lgammaf.

  quantity                      formula in the kernel, operations                                              bound (in u unless written out)
  e_c                           count_elem / the normal form: logprob_elem_bound without the count constant,    E_e = b(double_const) + |e_c|
                                and the value's own rounding at the size of e_c (the table's is at e_c - lgamma)
  j_c = a_c + e_c               one addition                                                                   E_j = E_e + |j_c|
  lse over C <= 4 terms         m = max (exact; from -3.0e38: a maximum below it is outside the grid),          ops = [sum_c t_c (|x_c - m| + EXPF) + (C - 1) s] / s
    m + logf(sum expf(x_c - m)) t_c = expf(x_c - m): the difference 1, expf EXPF; C - 1 additions of s = sum t_c; + LOGF |log s| + |lse|
                                logf LOGF; the closing sum 1.  The inputs' errors E_c through the function itself,   in = max(lse(x + E) - lse(x), lse(x) - lse(x - E))
                                which is monotone in every x_c: no linearisation
  resp_c = expf(j_c - lse_j)    softmax is monotone too: the interval of 1 / sum_k exp(j_k - j_c -+ (E_k + E_c))  E_resp = max(hi e^rel - resp, resp - lo e^-rel) + 2^-126
                                (to first order resp (1 - resp) (E_c + E_k): d resp / d joint);                   rel = ops_j + |j_c - lse_j| + EXPF
                                the difference 1, expf and the operations of lse_j, relative; resp <= 1
                                (lse_j >= m + log 1)
  pi_c = expf(a_c - lse_a)      exact inputs                                                                   E_pi = pi (ops_a + |a_c - lse_a| + EXPF) + 2^-126
  d a_c = (resp - pi) gs        the difference 1                                                               E_resp + E_pi + |resp - pi|
  d p_c = resp d_c gs           d_c: grad_elem_bound E_d; one product                                          E_resp (|d| + E_d) + resp E_d + |resp d| + 2^-126 (1 + |d|) / u
  element of the cell's sum     lse_j - lse_a - lgammaf(y + 1): two differences                                E_lse_j + E_lse_a + |lse_j - lse_a| + max(LGAMMAF lgamma, 1) + |v|
  grad_scale                    one product; exact for a power of two                                          |gs| E + |gs d| [gs no power of two]
  onehot lse                    wave_max exact; se: a lane's chain of ceil(P / 64) - 1 additions and              ops as above with n_se = ceil(P / 64) + 5 additions
                                wave_sum's six; logf; mx + 1
  onehot lp = raw - lse         the difference 1                                                               E_lp = E_lse + |lp|
  onehot y lp                   one product                                                                    |y| E_lp + |y lp|
  onehot d = y - expf(lp) ysum  s = expf(lp): EXPF and the exponent's error; ysum: n_se additions of sum |y|;         (s (E_lp + EXPF) + 2^-126 / u) |ysum| + s n_se sum |y|
                                one product, the difference 1 of (|y| + s |ysum|)                              + s |ysum| + |y| + s |ysum|
  mixtril L_pp = softplus + 1e-5 _sp_abs, the sum 1, the constant 1e-5f for 1e-5                                  E_d = _sp_abs(raw) + L_pp + 1e-5
  mixtril u = L^-1 (y - mu)     r = y - mu 1; substitution: per L_pj one product, at most P - 1 further          |du| <= |L^-1| (G |u| + |r|),  G_pj = (P + 4) |L_pj|,
                                differences, rcp 2 and its product 1: the componentwise bound of a triangular    G_pp = E_d + 4 L_pp
                                solve |du| <= gamma_P |L^-1| |L| |u|, with L^-1 in float64 from the inputs
  mixtril w = L^-T u            the same on u's error                                                          |dw| <= |L^-T| (|du| + G^T |w|)
  quad = sum u^2                the square 1, wave_sum 6                                                       sum (2 |u| E_u + E_u^2 + u^2) + 6 sum u^2
  logdet = sum flog(L_pp)       v_log and the scaling 3, the argument's error, wave_sum 6                       sum (3 |log L_pp| + E_d / L_pp) + 6 sum |log L_pp|
  e_c = -quad / 2 - logdet - cP the constant and its product 2, two differences                                E_quad / 2 + E_logdet + 2 cP + 2 (quad / 2 + |logdet| + cP)
  d mu = resp w gs              as d p_c with d = w, E_d = E_w
  d L_pj = resp w_p u_j gs      |w| E_u + E_w |u| + E_w E_u + |w u|, then as d p_c
  d L_pp = resp (w u - inv) sg  inv = rcp(L_pp): E_d / L_pp + 2; the difference 1 of (|w u| + inv); sg 6 + 2 |raw|;  (E_wu + inv (E_d / L_pp + 2) + |w u| + inv) sg + (7 + 2 |raw|) |d|
                                one product
A cell's log-likelihood: `cell_sum_bound`, row_sum_bound's form -- sum of the element bounds + (n_add + 8) u sum |summand| + u |sum| +
P 2^-126, n_add = ceil(Pp / 64) + 6 (+ 1 for the count kinds: the difference with lgammaf closes every summand): a lane's chain over
the passes, wave_sum's six steps.

THE GRID CONDITION.  An element is kept if every component passes likelihood_grad_ref.grad_in_range at the element's y, and -- the
family this module adds -- NOT every joint a_c + e_c lies below -3e38, the start of the kernels' maxima ("all components out of range").
THE KEPT-POINT CAP: per (kind, plane, axis family) at most a tenth of the elements is dropped.  The mixtures meet it by construction:
one component at a time walks the whole element grid of its kind (GRAD_AXES x counts_for) while the others take points that are kept at
all seven counts; 'normal' components at the raw scale -22 are likelihood_grad_ref's note.

THE MIXTURE-LOGIT PATTERNS: all 0; component q ahead by 5, 40, 90 (q walks with the element); all +60; all -60.  'mixnb' and 'mixgauss'
cross the six with every element.  'mixzinb' has 484 kept grid points x 7 counts per walking component: crossed, 'mixzinb4' would be
81 000 elements of four components each, 25 s of reference before a test compares anything, in a suite every later change runs.  There
the pattern is number (i + w) mod 6 of element i = 7 point + count of walker w: the seven counts of one grid point take seven consecutive
numbers, one count over the grid points takes point + count + w, so every (grid point, pattern) pair -- hence every value of every plane
beside every pattern -- and every (count, pattern) pair is on the grid; what is not is the full (point, count, pattern) triple.
tests/test_label_heads_host.py asserts the two pair coverages.

THE 'mixtril' RECIPE.  Component c of a cell: L = d (I + s N), d = softplus(raw_d) + 1e-5 for ONE raw_d of (-12, -3, 0, 5) on the whole
diagonal (-12: d = 1.6e-5, the 1e-5 shift's regime; in every other cell all components share it, in the rest component c takes the c-th
next: densities 1e10 apart) -- the strict lower triangle's raw plane holds float32(d s N_pj) --, N_pj =
cos(1.3 p + 0.7 j + c), s = `tril_scale(P, c, target)`: 0 for the target 1 (the init: zero weights, a diagonal L), else the bisection root
of cond_2(I + s N) = target for the targets 1e2 and 1e4.  A fifth diagonal cycles the four values down the diagonal with s = 0
(cond 3e5, a diagonal solve: the lanes' softplus regimes side by side).  loc_p = 0.5 cos(p + c), y_p = float32(loc_p + d_0 t_p), t_p =
1.7 sin(0.9 p + 0.4 i) (i the cell), so that u stays of order 1 at every d.  P = 1 has no off-diagonal: cond 1 at every target.
`tril_conds` returns the condition numbers reached; the host test prints them (2 <= P: within a factor 1.01 of the target)."""
import functools

import numpy as np
from scipy.special import expit

from tests import likelihood_grad_ref as L
from tests.plane_stat_ref import _sp_abs

U, F32_MIN, FLUSH = L.U, L.F32_MIN, L.FLUSH
SENTINEL = -3.0e38
HALF_LOG_2PI = 0.9189385332046727
EXPF, LOGF, LGAMMAF = 4.0, 10.0, 12.0      # in u, of the result: the docstring's paragraph on the library functions
SIMPLE = L.GRAD_KINDS
MIX_COMPONENT = dict(mixnb="nb", mixzinb="zinb", mixgauss="normal")
ALL_KINDS = SIMPLE + ("onehot",) + tuple(f"{m}{c}" for m in MIX_COMPONENT for c in (1, 2, 3, 4)) + tuple(f"mixtril{c}" for c in (2, 3, 4))
PATTERNS = ("zero", "ahead5", "ahead40", "ahead90", "all+60", "all-60")
TRIL_DIAG = (-12.0, -3.0, 0.0, 5.0)
TRIL_TARGETS = (1.0, 1e2, 1e4)
TRIL_SHIFT = 1e-5


def split_kind(kind):
  """'mixnb3' -> ('mixnb', 3); 'nb' -> ('nb', 1)"""
  for base in tuple(MIX_COMPONENT) + ("mixtril",):
    if kind.startswith(base):
      return base, int(kind[len(base):])
  return kind, 1


def n_planes(kind, P=0):
  base, C = split_kind(kind)
  if base == "mixtril":
    return C * (2 + P)
  if base in MIX_COMPONENT:
    return (4 if base == "mixzinb" else 3) * C
  return {"nb": 2, "nbd": 2, "normal": 2, "zinb": 3, "zinbd": 3, "onehot": 1, "bernoulli": 1}[kind]


def passes(P):
  return -(-((P + 31) // 32 * 32) // 64)


def n_add(kind, P):
  """the longest chain of float32 additions behind a cell's log-likelihood (the docstring's last paragraph)"""
  base = split_kind(kind)[0]
  return passes(P) + 6 + (1 if base in ("nb", "nbd", "zinb", "zinbd", "mixnb", "mixzinb") else 0)


def scale_grad(g, bg, gs):
  """the gradient and its bound after the product by grad_scale (float32 value `gs`)"""
  gs = float(np.float32(gs))
  pow2 = gs == 0.0 or np.frexp(abs(gs))[0] == 0.5
  return g * gs, bg * abs(gs) + (0.0 if pow2 else U * np.abs(g * gs)) + (F32_MIN if gs else 0.0)


# ---- log-sum-exp over a leading axis, with its operations' bound --------------------------------------------------------------------
def _lse(x):
  with np.errstate(invalid="ignore", over="ignore"):
    return np.logaddexp.reduce(x, axis=0)


def _lse_ops(x, n_sum):
  """the operations of m + logf(sum expf(x - m)) on exact inputs x [C, ...]: absolute bound (not yet times u); n_sum additions"""
  m = x.max(axis=0)
  with np.errstate(invalid="ignore", over="ignore"):
    t = np.exp(x - m)
    s = t.sum(axis=0)
    return ((t * (np.abs(x - m) + EXPF)).sum(axis=0) + n_sum * s) / s + LOGF * np.abs(np.log(s)) + np.abs(m + np.log(s))


def _lse_in(x, E):
  """the inputs' errors E through the monotone function: absolute"""
  l = _lse(x)
  return np.maximum(_lse(x + E) - l, l - _lse(x - E))


def _softmax_interval(j, E):
  """(resp, lo, hi) [C, ...] of resp_c = 1 / sum_k exp(j_k - j_c) under |dj_k| <= E_k"""
  C = j.shape[0]
  with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
    out = []
    for sign in (0.0, 1.0, -1.0):
      rows = []
      for c in range(C):
        tot = 0.0
        for k in range(C):
          tot = tot + (1.0 if k == c else np.exp((j[k] - j[c]) + sign * (E[k] + E[c])))
        rows.append(1.0 / tot)
      out.append(np.stack(rows))
  return tuple(out)


def _mixture(a, e, E_e, n_sum=None):
  """the mixture layer over components: a, e, E_e [C, ...] (logits; component log densities and their absolute bounds) ->
  dict(lse_e = log sum pi exp(e), resp, pi, dmix = resp - pi, E_lse (of lse_j - lse_a as the kernel forms it), E_resp, E_pi, E_dmix), the
  E's absolute"""
  C = a.shape[0]
  n_sum = C - 1 if n_sum is None else n_sum
  with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
    lse_a = _lse(a)
    log_pi = a - lse_a
    pi = np.exp(log_pi)
    j = a + e
    lse_j = _lse(j)
    lse_e = _lse(log_pi + e)
    D = np.stack([(pi * np.exp(e - e[c])).sum(axis=0) for c in range(C)])
    S = np.stack([sum(pi[k] * np.expm1(e[k] - e[c]) for k in range(C) if k != c) + 0.0 * pi[c] for c in range(C)])
    resp = pi / D
    dmix = np.where(np.isinf(D), -pi, -pi * S / D)
    E_j = E_e + U * np.abs(j)
    ops_j, ops_a = U * _lse_ops(j, n_sum), U * _lse_ops(a, n_sum)
    E_lse_j = _lse_in(j, E_j) + ops_j
    _, lo, hi = _softmax_interval(j, E_j)
    rel = ops_j + U * np.abs(j - lse_j) + EXPF * U
    up = np.where(hi == 0.0, 0.0, np.minimum(hi * np.exp(np.minimum(rel, 700.0)), 1.0))   # (hi == 0: below float64, whatever rel adds to the exponent)
    E_resp = np.maximum(up - resp, resp - lo * np.exp(-rel)) + F32_MIN
    E_pi = pi * (ops_a + U * np.abs(a - lse_a) + EXPF * U) + F32_MIN
  return dict(lse_e=lse_e, resp=resp, pi=pi, dmix=dmix, E_lse=E_lse_j + ops_a + U * np.abs(lse_e), E_resp=E_resp, E_pi=E_pi,
              E_dmix=E_resp + E_pi + U * np.abs(dmix), all_out=(j < SENTINEL).all(axis=0))


def _times_resp(m, c, d, E_d):
  """resp_c d and its absolute bound (the table's row d p_c)"""
  with np.errstate(invalid="ignore", over="ignore"):
    return m["resp"][c] * d, (m["E_resp"][c] * (np.abs(d) + E_d) + m["resp"][c] * E_d + U * np.abs(m["resp"][c] * d) + F32_MIN * (1.0 + np.abs(d)))


# ---- the elementwise kinds ------------------------------------------------------------------------------------------------------------
def elem(kind, y, planes):
  """One label dimension of one cell, elementwise over arrays of any one shape: y and the kind's planes in the kernel's plane order (a
  mixture: C logits, C first parameters, C second[, C gates]) -> dict(v: the summand of the cell's log-likelihood, bv: its absolute
  bound, g [k, ...]: the gradients wrt the planes at grad_scale 1, bg [k, ...], keep: the grid condition)"""
  base, C = split_kind(kind)
  y = np.asarray(y, np.float32)
  planes = [np.asarray(p, np.float32) for p in planes]
  assert len(planes) == n_planes(kind) and all(p.shape == y.shape for p in planes)
  if base in SIMPLE:
    k = len(planes)
    return dict(v=L.log_prob_elem(kind, y, planes), bv=L.logprob_elem_bound(kind, y, planes), g=L.grad_elem(kind, y, planes)[:k],
                bg=L.grad_elem_bound(kind, y, planes)[:k], keep=L.grad_in_range(kind, y, planes))
  comp = MIX_COMPONENT[base]
  kc = 3 if comp == "zinb" else 2
  const = L.count_const(comp, y)
  a = np.stack([p.astype(np.float64) for p in planes[:C]])
  e, E_e, d, E_d, keep = [], [], [], [], np.ones(y.shape, bool)
  with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
    for c in range(C):
      pl = [planes[(1 + q) * C + c] for q in range(kc)]
      ec = L.log_prob_elem(comp, y, pl) + const
      e.append(ec)
      E_e.append(L.logprob_elem_bound(comp, y, pl, double_const=True) + U * np.abs(ec))
      d.append(L.grad_elem(comp, y, pl)[:kc])
      E_d.append(L.grad_elem_bound(comp, y, pl)[:kc])
      keep &= L.grad_in_range(comp, y, pl)
    m = _mixture(a, np.stack(e), np.stack(E_e))
    v = m["lse_e"] - const
    bv = m["E_lse"] + (np.maximum(LGAMMAF * np.abs(const), 1.0) * U + U * np.abs(v) if comp != "normal" else 0.0)
    g, bg = [m["dmix"][c] for c in range(C)], [m["E_dmix"][c] for c in range(C)]
    for q in range(kc):
      for c in range(C):
        gv, bgv = _times_resp(m, c, d[c][q], E_d[c][q])
        g.append(gv)
        bg.append(bgv)
  return dict(v=v, bv=bv, g=np.stack(g), bg=np.stack(bg), keep=keep & ~m["all_out"], resp=m["resp"], E_resp=m["E_resp"], comp_g=d, comp_bg=E_d)


@functools.lru_cache(maxsize=None)
def grid_eval(kind):
  """`elem` on the whole of `grid(kind)`, computed once"""
  y, planes, _ = grid(kind)
  return elem(kind, y, planes)


def dominance(o, c, q):
  """Of a mixture's `elem` result, for component c's q-th parameter plane: (under, under_bound, dom, dom_bound).  under: the elements whose
  resp_c is below 2^-126 and stays there over its interval; the table's row d p_c then leaves the underflow term 2^-126 (1 + 4 |d| + 3 E_d)
  (E_resp <= 2 x 2^-126 on |d| + E_d, resp E_d, the product, the row's own 2^-126 (1 + |d|)).  dom: resp_c >= 1 - 4 u; the gradient is then
  the single-component kind's d within E_d + (E_resp + 5 u) (|d| + E_d) + 2^-126 (1 + |d|) (the computed resp is within E_resp + 4 u of 1, on
  the computed d; the product 1)"""
  d, E_d, resp, E_resp = np.abs(o["comp_g"][c][q]), o["comp_bg"][c][q], o["resp"][c], o["E_resp"][c]
  under = (resp < F32_MIN) & (E_resp <= 2.0 * F32_MIN)
  dom = resp >= 1.0 - 4.0 * U
  return under, F32_MIN * (1.0 + 4.0 * d + 3.0 * E_d), dom, E_d + (E_resp + 5.0 * U) * (d + E_d) + F32_MIN * (1.0 + d)


def cell_sum_bound(kind, P, v, bv):
  """(ref, bound) of a cell's log-likelihood from its elements' v, bv [..., P] (the docstring's last paragraph)"""
  ref = v.sum(axis=-1)
  return ref, bv.sum(axis=-1) + (n_add(kind, P) + 8.0) * U * np.abs(v).sum(axis=-1) + U * np.abs(ref) + P * F32_MIN


# ---- onehot -----------------------------------------------------------------------------------------------------------------------------
def onehot(raw, y):
  """raw, y [R, P] -> dict(v = y lp, bv, g [1, R, P], bg, keep) per element; the row quantities inside"""
  raw, y = np.asarray(raw, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
  P = raw.shape[1]
  n_se = passes(P) + 5
  x = raw.T                                                        # [P, R]: the components on the leading axis
  lse = _lse(x)
  E_lse = U * _lse_ops(x, n_se)
  lp = (x - lse).T
  s = np.exp(lp)
  E_lp = E_lse[:, None] + U * np.abs(lp)
  ysum, yabs = y.sum(axis=1, keepdims=True), np.abs(y).sum(axis=1, keepdims=True)
  off = 1.0 - np.eye(P)
  d = y * (s @ off) - s * (y @ off)                                # sum_{k != p} (y_p s_k - s_p y_k): neither sum holds its own column
  bd = (s * (E_lp + EXPF * U) + F32_MIN) * np.abs(ysum) + s * n_se * U * yabs + U * (2.0 * s * np.abs(ysum) + np.abs(y)) + F32_MIN
  return dict(v=y * lp, bv=np.abs(y) * E_lp + U * np.abs(y * lp), g=d[None], bg=bd[None], keep=np.ones(raw.shape, bool))


ONEHOT_LOGITS = ("ramp", "equal", "one+80", "one-80")
ONEHOT_TARGETS = ("onehot", "zero", "multihot", "soft1", "soft2.5")


def onehot_grid(P):
  """(raw, y) [R, P] float32: every logit pattern x every target row, the singled-out column at 0, P // 2 and P - 1"""
  raws, ys = [], []
  p = np.arange(P)
  for at in sorted({0, P // 2, P - 1}):
    for lg in ONEHOT_LOGITS:
      r = {"ramp": 0.37 * p - 3.0, "equal": np.full(P, 1.25)}.get(lg)
      if r is None:
        r = 0.1 * np.cos(p + 1.0)
        r[at] = 80.0 if lg == "one+80" else -80.0
      for tg in ONEHOT_TARGETS:
        soft = (1.0 + np.cos(0.7 * p) ** 2)
        t = {"onehot": (p == at) * 1.0, "zero": np.zeros(P), "multihot": ((p % 3 == at % 3) | (p == at)) * 1.0, "soft1": soft / soft.sum(),
             "soft2.5": 2.5 * soft / soft.sum()}[tg]
        raws.append(r)
        ys.append(t)
  return np.array(raws, np.float32), np.array(ys, np.float32)


# ---- the mixtures' element grid -----------------------------------------------------------------------------------------------------------
def mix_logits(pattern, C, q):
  a = np.zeros(C)
  if pattern.startswith("ahead"):
    a[q % C] = float(pattern[5:])
  elif pattern.startswith("all"):
    a[:] = float(pattern[3:])
  return a


@functools.lru_cache(maxsize=None)
def _component_grid(comp):
  """(y [n], planes k x [n], keep [n], safe: indices of the grid points kept at all seven counts) of the component kind's element grid"""
  x, planes, keep = L.grid_elements(comp)
  flat = lambda a: np.ascontiguousarray(np.broadcast_to(a, x.shape).reshape(-1))
  return flat(x), [flat(p) for p in planes], flat(keep), np.flatnonzero(keep.all(axis=1))


@functools.lru_cache(maxsize=None)
def grid(kind):
  """(y [n], planes k x [n], family [n]) float32: the element grid of an elementwise kind.  family: for a mixture the walking component
  (the docstring's cap is per family), 0 otherwise"""
  base, C = split_kind(kind)
  if base in SIMPLE:
    y, planes, _, _ = _component_grid(kind)
    return y, planes, np.zeros(len(y), np.int64)
  comp = MIX_COMPONENT[base]
  y, cpl, _, safe = _component_grid(comp)
  n, kc, n7 = len(y), len(cpl), 7
  pats = PATTERNS if base != "mixzinb" else (None,)                  # 'mixzinb': the patterns cycle with the element (504 grid points x 7 counts)
  ys, fam, cols = [], [], [[] for _ in range((1 + kc) * C)]
  idx = np.arange(n)
  for w in range(C):
    for pi_, pat in enumerate(pats):
      names = [pat] * n if pat is not None else [PATTERNS[(i + w) % len(PATTERNS)] for i in idx]
      a = np.array([mix_logits(nm, C, i // n7 + w) for i, nm in zip(idx, names)])
      ys.append(y)
      fam.append(np.full(n, w))
      for c in range(C):
        cols[c].append(a[:, c])
        # the walker takes element i; every other component a grid point that is kept at every count, at the element's own count
        src = idx if c == w else safe[(idx // n7 * 5 + 11 * c + 3 * pi_) % len(safe)] * n7 + idx % n7
        for q in range(kc):
          cols[(1 + q) * C + c].append(cpl[q][src])
  return (np.concatenate(ys).astype(np.float32), [np.concatenate(c).astype(np.float32) for c in cols], np.concatenate(fam))


# ---- mixtril --------------------------------------------------------------------------------------------------------------------------------
def _tril_N(P, c):
  p, j = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
  return np.tril(np.cos(1.3 * p + 0.7 * j + c), -1)


@functools.lru_cache(maxsize=None)
def tril_scale(P, c, target):
  """s with cond_2(I + s N) = target (0 for target 1 or P = 1), by bisection"""
  if target <= 1.0 or P < 2:
    return 0.0
  N, I = _tril_N(P, c), np.eye(P)
  lo, hi = 0.0, 1.0
  while np.linalg.cond(I + hi * N) < target:
    hi *= 2.0
  for _ in range(60):
    mid = 0.5 * (lo + hi)
    lo, hi = (mid, hi) if np.linalg.cond(I + mid * N) < target else (lo, mid)
  return hi


def tril_grid(C, P):
  """dict(a [R, C], mu [R, C, P], Lraw [R, C, P, P] (row p, column j; the strict upper triangle is NaN: no kernel reads it), y [R, P],
  cond [R, C]) float32 but cond: the recipe of the module docstring, one cell per (diagonal, target, logit pattern)"""
  cells = []
  p = np.arange(P)
  for di in range(len(TRIL_DIAG) + 1):
    for target in (TRIL_TARGETS if di < len(TRIL_DIAG) else (1.0,)):
      for pat in PATTERNS:
        cells.append((di, target, pat))
  R = len(cells)
  o = dict(a=np.zeros((R, C)), mu=np.zeros((R, C, P)), Lraw=np.full((R, C, P, P), np.nan), y=np.zeros((R, P)), cond=np.zeros((R, C)))
  for i, (di, target, pat) in enumerate(cells):
    o["a"][i] = mix_logits(pat, C, i)
    for c in range(C):
      rd = np.full(P, TRIL_DIAG[(di + c * ((i // len(PATTERNS) + i) % 2)) % 4]) if di < len(TRIL_DIAG) else np.array(TRIL_DIAG)[(p + c) % 4]
      d = L.softplus(rd) + TRIL_SHIFT
      Lm = np.diag(d) + d[:, None] * tril_scale(P, c, target) * _tril_N(P, c)
      o["cond"][i, c] = np.linalg.cond(Lm)
      lower = np.tril(np.ones((P, P), bool), -1)
      o["Lraw"][i, c][lower] = Lm[lower]
      o["Lraw"][i, c][p, p] = rd
      o["mu"][i, c] = 0.5 * np.cos(p + c)
      if c == 0:
        o["y"][i] = o["mu"][i, 0] + d[0] * 1.7 * np.sin(0.9 * p + 0.4 * i)
  return {k: (v if k == "cond" else v.astype(np.float32)) for k, v in o.items()}


def tril_pack(g, C, P, Pp, fill=np.nan):
  """the cells of a tril_grid-shaped dict as the kernel's planes: raw [R, C (2 + P) Pp] float32, `fill` in every word the kernel must not
  read (columns P .. Pp; the logit planes beyond column 0; the strict upper triangle stays NaN)"""
  R = g["a"].shape[0]
  raw = np.full((R, C * (2 + P), Pp), fill, np.float32)
  for c in range(C):
    raw[:, c, 0] = g["a"][:, c]
    raw[:, C + c, :P] = g["mu"][:, c]
    for j in range(P):
      raw[:, 2 * C + c * P + j, :P] = g["Lraw"][:, c, :, j]
  return raw.reshape(R, -1)


def tril_unpack(draw, C, P, Pp):
  """the kernel's d raw [R, >= C (2 + P) Pp] -> (dmix [R, C], dmu [R, C, P], dL [R, C, P, P] (row p, column j), the whole planes [R, C (2 + P), Pp])"""
  R = draw.shape[0]
  pl = draw[:, :C * (2 + P) * Pp].reshape(R, C * (2 + P), Pp)
  dL = np.stack([np.stack([pl[:, 2 * C + c * P + j, :P] for j in range(P)], axis=2) for c in range(C)], axis=1)
  return pl[:, :C, 0], pl[:, C:2 * C, :P], dL, pl


def tril(a, mu, Lraw, y):
  """'mixtril' cells: a [R, C], mu [R, C, P], Lraw [R, C, P, P], y [R, P] (float32 values) -> dict(llk, b_llk [R]; dmix, b_dmix [R, C]; dmu,
  b_dmu [R, C, P]; dL, b_dL [R, C, P, P]: the lower triangle with the diagonal, 0 above; resp [R, C]; keep [R]) at grad_scale 1"""
  f = lambda v: np.asarray(v, np.float32).astype(np.float64)
  a, mu, Lraw, y = f(a), f(mu), f(Lraw), f(y)
  R, C, P = mu.shape
  e, E_e = np.zeros((C, R)), np.zeros((C, R))
  keepd = {}
  lower = np.tril(np.ones((P, P), bool), -1)
  for c in range(C):
    for i in range(R):
      rd = np.diagonal(Lraw[i, c]).copy()
      d = L.softplus(rd) + TRIL_SHIFT
      Lm = np.where(lower, Lraw[i, c], 0.0) + np.diag(d)
      E_dd = (_sp_abs(rd) + d + TRIL_SHIFT) * U
      r = y[i] - mu[i, c]
      u, w = np.zeros(P), np.zeros(P)
      for p in range(P):
        u[p] = (r[p] - Lm[p, :p] @ u[:p]) / d[p]
      for p in range(P - 1, -1, -1):
        w[p] = (u[p] - Lm[p + 1:, p] @ w[p + 1:]) / d[p]
      Li = np.abs(np.linalg.inv(Lm))
      G = (P + 4.0) * U * np.abs(np.where(lower, Lm, 0.0)) + np.diag(E_dd + 4.0 * U * d)
      E_u = Li @ (G @ np.abs(u) + U * np.abs(r))
      E_w = Li.T @ (E_u + G.T @ np.abs(w))
      quad, logs = (u * u).sum(), np.log(d)
      E_quad = (2.0 * np.abs(u) * E_u + E_u ** 2 + U * u * u).sum() + 6.0 * U * quad
      E_ld = (3.0 * U * np.abs(logs) + E_dd / d).sum() + 6.0 * U * np.abs(logs).sum()
      cP = HALF_LOG_2PI * P
      e[c, i] = -0.5 * quad - logs.sum() - cP
      E_e[c, i] = 0.5 * E_quad + E_ld + 2.0 * U * cP + 2.0 * U * (0.5 * quad + np.abs(logs.sum()) + cP)
      inv, sg = 1.0 / d, expit(rd)
      wu = w[:, None] * u[None, :]
      E_wu = np.abs(w)[:, None] * E_u[None, :] + E_w[:, None] * np.abs(u)[None, :] + E_w[:, None] * E_u[None, :] + U * np.abs(wu)
      dL = np.where(lower, wu, 0.0)
      E_dL = np.where(lower, E_wu, 0.0)
      dd = (np.diagonal(wu) - inv) * sg
      E_ddiag = (np.diagonal(E_wu) + inv * (E_dd / d + 2.0 * U) + U * (np.abs(np.diagonal(wu)) + inv)) * sg + (7.0 + 2.0 * np.abs(rd)) * U * np.abs(dd)
      dL[np.arange(P), np.arange(P)] = dd
      E_dL[np.arange(P), np.arange(P)] = E_ddiag
      keepd[(i, c)] = (w, E_w, dL, E_dL)
  m = _mixture(a.T, e, E_e)
  o = dict(llk=m["lse_e"], b_llk=m["E_lse"], dmix=m["dmix"].T, b_dmix=m["E_dmix"].T, resp=m["resp"].T, keep=~m["all_out"] & np.isfinite(e).all(axis=0),
           dmu=np.zeros((R, C, P)), b_dmu=np.zeros((R, C, P)), dL=np.zeros((R, C, P, P)), b_dL=np.zeros((R, C, P, P)), e=e.T)
  for c in range(C):
    for i in range(R):
      w, E_w, dL, E_dL = keepd[(i, c)]
      mi = {k: v[:, i] for k, v in m.items() if k in ("resp", "E_resp")}
      o["dmu"][i, c], o["b_dmu"][i, c] = _times_resp(mi, c, w, E_w)
      o["dL"][i, c], o["b_dL"][i, c] = _times_resp(mi, c, dL, E_dL)
  return o


def tril_conds(C, P):
  """{(raw diagonal or 'cycle', target): the range of cond_2(L) over the components}: what the recipe reaches"""
  g = tril_grid(C, P)
  out, i = {}, 0
  for di in range(len(TRIL_DIAG) + 1):
    for target in (TRIL_TARGETS if di < len(TRIL_DIAG) else (1.0,)):
      out[(TRIL_DIAG[di] if di < len(TRIL_DIAG) else "cycle", target)] = (float(g["cond"][i].min()), float(g["cond"][i].max()))
      i += len(PATTERNS)
  return out


# ---- the planes of a cell ---------------------------------------------------------------------------------------------------------------------
def pack(planes, B, P, Pp, fill=np.nan, ld=None):
  """k planes of B x P elements -> raw [B, ld] float32 in the step's layout (plane c of a row at c Pp), `fill` in columns P .. Pp and behind"""
  k = len(planes)
  raw = np.full((B, k * Pp if ld is None else ld), fill, np.float32)
  for c, pl in enumerate(planes):
    raw[:, c * Pp:c * Pp + P] = np.asarray(pl, np.float32).reshape(B, P)
  return raw


def pack_y(y, B, P, Pp, fill=np.nan):
  Y = np.full((B, Pp), fill, np.float32)
  Y[:, :P] = np.asarray(y, np.float32).reshape(B, P)
  return Y


def cells_of(arr, B, P, offset=0):
  """B x P consecutive elements of a flat grid array, cyclically from `offset`"""
  return np.asarray(arr)[(offset + np.arange(B * P)) % len(arr)].reshape(B, P)
