"""tests/likelihood_grad_ref.py held to account on the host: its float64 gradients against mpmath (120 digits) on the whole edge grid x
the seven counts -- closed textbook forms everywhere, and numerical differentiation of the textbook log-probability on a strided
subset, so that the closed forms are themselves checked --, a float32 NumPy replay of count_elem / bernoulli_elem / normal_elem
(smx_loss.h, operation for operation, both branches of lgamma_digamma_diff) inside the derived bounds, two unrepaired formulas
outside them, and the grid condition's dropped share.  The replay checks the derivation of the bounds; it is no measurement of the
device."""
import mpmath as mp
import numpy as np
import pytest

from tests import likelihood_grad_ref as L

RATIO = 1e-3      # |reference - mpmath| <= RATIO x the float32 bound, at every point


@pytest.mark.parametrize("kind,direct", L.ALL)
def test_grid_condition_drops_at_most_a_tenth(kind, direct):
  x, planes, keep = L.grid_elements(kind, direct)
  per_point = (~keep).any(axis=1)
  print(f"{kind} direct={direct}: {int((~keep).sum())} of {keep.size} elements dropped, {int(per_point.sum())} of {len(per_point)} grid points "
        f"lose a count")
  assert per_point.sum() * 10 <= len(per_point), (kind, direct)
  b = L.grad_elem_bound(kind, x, planes, direct)
  g = L.grad_elem(kind, x, planes, direct)
  assert np.isfinite(b[:, keep]).all() and np.isfinite(g[:, keep]).all() and (b[:, keep] >= 0).all()
  for c, axis in enumerate(L.GRAD_AXES[kind]):   # no axis value is lost for a whole kind
    if not direct:
      kept_vals = set(np.broadcast_to(planes[c], keep.shape)[keep])
      assert set(np.float32(axis)) == kept_vals, (kind, c)
  if kind != "normal":   # the gradient grid IS plane_stat_ref's grid
    assert L.GRAD_AXES[kind] == L.AXES[kind]
    assert np.array_equal(L.grad_bias_grid(kind)[0], L.bias_grid(kind)[0])


# ---- mpmath ---------------------------------------------------------------------------------------------------------------------------
def _mp_sp(v):
  return mp.log1p(mp.exp(v))


def _mp_sig(v):
  return 1 / (1 + mp.exp(-v))


def _mp_logp(kind, p, direct, x):
  """the textbook log-probability of one element (up to the count constant), p a list of mpf"""
  c1 = mp.log(mp.expm1(1))
  if kind == "bernoulli":
    return x * p[0] - _mp_sp(p[0])
  if kind == "normal":
    sd = _mp_sp(p[1] + c1)
    return -((x - p[0]) / sd) ** 2 / 2 - mp.log(sd)
  if kind in ("nb", "zinb"):
    r = mp.exp(p[0])
    ell = mp.loggamma(x + r) - mp.loggamma(r) + x * (p[1] - _mp_sp(p[1])) - r * _mp_sp(p[1])
  else:
    mu, th = (p[0], p[1]) if direct else (_mp_sp(p[0]), _mp_sp(p[1] + c1))
    e = mp.mpf(L.EPS)
    lt = mp.log(th + mu + e)
    ell = th * (mp.log(th + e) - lt) + x * (mp.log(mu + e) - lt) + mp.loggamma(x + th) - mp.loggamma(th)
  if not L.is_zi(kind):
    return ell
  pi = _mp_sig(p[2])
  return mp.log(pi + (1 - pi) * mp.exp(ell)) if x == 0 else mp.log(1 - pi) + ell


def _mp_grad(kind, p, direct, x):
  """closed textbook derivatives in mpmath: 1 - pi, digamma differences and all, at 120 digits"""
  c1 = mp.log(mp.expm1(1))
  zero = mp.mpf(0)
  if kind == "bernoulli":
    return [x - _mp_sig(p[0]), zero, zero]
  if kind == "normal":
    sd = _mp_sp(p[1] + c1)
    z = (x - p[0]) / sd
    return [z / sd, (z * z - 1) / sd * _mp_sig(p[1] + c1), zero]
  if kind in ("nb", "zinb"):
    r = mp.exp(p[0])
    ell = mp.loggamma(x + r) - mp.loggamma(r) + x * (p[1] - _mp_sp(p[1])) - r * _mp_sp(p[1])
    d0 = r * (mp.digamma(x + r) - mp.digamma(r) - _mp_sp(p[1]))
    d1 = x - (x + r) * _mp_sig(p[1])
  else:
    mu, th = (p[0], p[1]) if direct else (_mp_sp(p[0]), _mp_sp(p[1] + c1))
    g0, g1 = (1, 1) if direct else (_mp_sig(p[0]), _mp_sig(p[1] + c1))
    e = mp.mpf(L.EPS)
    T = th + mu + e
    ell = th * (mp.log(th + e) - mp.log(T)) + x * (mp.log(mu + e) - mp.log(T)) + mp.loggamma(x + th) - mp.loggamma(th)
    d0 = (-th / T + x / (mu + e) - x / T) * g0
    d1 = (mp.log(th + e) - mp.log(T) + th / (th + e) - th / T - x / T + mp.digamma(x + th) - mp.digamma(th)) * g1
  if not L.is_zi(kind):
    return [d0, d1, zero]
  pi = _mp_sig(p[2])
  if x != 0:
    return [d0, d1, -pi]
  lik = pi + (1 - pi) * mp.exp(ell)
  w = (1 - pi) * mp.exp(ell) / lik
  return [d0 * w, d1 * w, pi * (1 - pi) * (1 - mp.exp(ell)) / lik]


@pytest.mark.parametrize("kind,direct", L.ALL)
def test_reference_agrees_with_mpmath(kind, direct):
  """|grad_elem - mpmath| <= 1e-3 of the float32 bound at every kept element of the grid x the seven counts; the closed mpmath forms agree
  with the numerical derivative of the textbook log-probability at every 11th element"""
  x, planes, keep = L.grid_elements(kind, direct)
  g = L.grad_elem(kind, x, planes, direct)
  b = L.grad_elem_bound(kind, x, planes, direct)
  n, k = x.shape[0], len(planes)
  worst_ratio, worst_rel, at, checked = 0.0, 0.0, None, 0
  with mp.workdps(120):
    for i in range(n):
      pt = [mp.mpf(float(pl[i, 0])) for pl in planes]
      for j in range(x.shape[1]):
        if not keep[i, j]:
          continue
        xv = mp.mpf(float(x[i, j]))
        ref = _mp_grad(kind, pt, direct, xv)
        if (i * x.shape[1] + j) % 11 == 0:
          for c in range(k):
            num = mp.diff(lambda v: _mp_logp(kind, pt[:c] + [v] + pt[c + 1:], direct, xv), pt[c])
            scale = max(abs(ref[c]), abs(num))
            assert scale == 0 or abs(num - ref[c]) <= mp.mpf(10) ** -40 * scale + mp.mpf(10) ** -100, (kind, direct, c, [float(v) for v in pt], float(xv), mp.nstr(num, 15), mp.nstr(ref[c], 15))
          checked += 1
        for c in range(3):
          diff = abs(mp.mpf(float(g[c, i, j])) - ref[c])
          err = float(diff)
          ratio = err / b[c, i, j] if err else 0.0
          rel = float(diff / abs(ref[c])) if abs(ref[c]) >= L.F32_MIN else 0.0     # (of the values float32 can hold)
          if ratio > worst_ratio:
            worst_ratio, at = ratio, (c, [float(v) for v in pt], float(xv), float(g[c, i, j]), mp.nstr(ref[c], 20))
          worst_rel = max(worst_rel, rel)
  print(f"{kind} direct={direct}: {int(keep.sum())} elements ({checked} also differentiated numerically), worst |ref - mpmath| / bound "
        f"{worst_ratio:.2e} at {at}, worst relative difference {worst_rel:.2e}")
  assert worst_ratio <= RATIO, (kind, direct, worst_ratio, at)


# ---- the float32 replay ----------------------------------------------------------------------------------------------------------------
F = np.float32


def _fexp(x):
  return np.exp2(F(x) * F(1.4426950408889634)).astype(F)


def _flog(x):
  return (np.log2(x.astype(F)).astype(F) * F(0.6931471805599453)).astype(F)


def _frcp(x):
  return (F(1) / x.astype(F)).astype(F)


def _log1p_small(e):
  ser = e * (F(1) - e * (F(0.5) - e * (F(0.33333334) - e * (F(0.25) - e * F(0.2)))))
  return np.where(e < F(0.03125), ser, _flog(F(1) + e)).astype(F)


def _softplus_sigmoid(x):
  e = _fexp(-np.abs(x))
  inv = _frcp(F(1) + e)
  return (np.maximum(x, F(0)) + _log1p_small(e)).astype(F), np.where(x >= 0, inv, e * inv).astype(F)


def _fma(a, b, c):
  return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)   # (the product is exact in float64)


def _stirling_corr(z):
  iz = _frcp(z)
  iz2 = iz * iz
  return iz * (F(0.083333333333) + iz2 * (F(-0.0027777777778) + iz2 * F(0.00079365079365)))


def _digamma_corr(z):
  iz = _frcp(z)
  iz2 = iz * iz
  return F(-0.5) * iz - iz2 * (F(0.083333333333) - iz2 * (F(0.0083333333333) - iz2 * F(0.003968253968)))


def _lgamma_digamma_diff(x, r):
  r = np.minimum(np.maximum(r, F(1e-30)), F(1e30))
  P, dP = np.ones_like(r), np.zeros_like(r)
  for i in range(8):
    t = r + F(i)
    on = F(i) < x
    dP = np.where(on, _fma(dP, t, P), dP)
    P = np.where(on, P * t, P).astype(F)
  lg, dg = _flog(P), dP * _frcp(P)
  small = (x <= F(8)) & (x == np.floor(x)) & (r < F(1e4))
  nf = np.maximum(np.ceil(F(4) - r), F(0))
  num, den, dg_shift = np.ones_like(r), np.ones_like(r), np.zeros_like(r)
  for i in range(4):
    a = r + F(i)
    b = x + a
    on = F(i) < nf
    num, den = np.where(on, num * a, num).astype(F), np.where(on, den * b, den).astype(F)
    dg_shift = np.where(on, dg_shift + x * _frcp(b) * _frcp(a), dg_shift).astype(F)
  lg_shift = _flog(num) - _flog(den)
  rs = r + nf
  zr = x + rs
  l1p = _log1p_small(x * _frcp(rs))
  lgr = x * _flog(zr) + (rs - F(0.5)) * l1p - x + (_stirling_corr(zr) - _stirling_corr(rs)) + lg_shift
  dgr = l1p + (_digamma_corr(zr) - _digamma_corr(rs)) + dg_shift
  return np.where(small, lg, lgr).astype(F), np.where(small, dg, dgr).astype(F)


def replay_count_elem(kind, x, planes, direct=False, d2_form="kernel", log_difference=False):
  """count_elem in NumPy float32, operation for operation: (llk without the count constant, [d0, d1, d2]).
  d2_form: 'kernel' -- the other branch of the quotient minus sg; 'one_minus_w' -- (1 - w) - sg, the form before the repair;
  'one_minus_sum' -- 1 - (w + sg).  log_difference: the 'nbd' dispersion gradient's -log1p(mu / (th + e)) as log(th + e) - log(th + mu + e)."""
  p = [np.asarray(v, F) for v in planes]
  x = np.broadcast_to(np.asarray(x, F), np.broadcast_shapes(np.shape(x), p[0].shape))
  p = [np.broadcast_to(v, x.shape) for v in p]
  zero = np.zeros(x.shape, F)
  with np.errstate(all="ignore"):
    if kind == "bernoulli":
      sp, sg = _softplus_sigmoid(p[0])
      return x * p[0] - sp, [x - sg, zero, zero]
    if kind == "normal":
      sp, sg = _softplus_sigmoid(p[1] + F(L.SOFTPLUS_INV_1))
      inv = _frcp(sp)
      zz = (x - p[0]) * inv
      return F(-0.5) * zz * zz - _flog(sp) - F(0.9189385332046727), [zz * inv, (zz * zz - F(1)) * inv * sg, zero]
    if kind in ("nb", "zinb"):
      r = _fexp(p[0])
      sp, sg = _softplus_sigmoid(p[1])
      lg, dg = _lgamma_digamma_diff(x, r)
      ell = lg + x * (p[1] - sp) - r * sp
      d0, d1 = r * (dg - sp), x - (x + r) * sg
    else:
      if direct:
        mu, th, g0, g1 = p[0], p[1], F(1), F(1)
      else:
        (mu, g0), (th, g1) = _softplus_sigmoid(p[0]), _softplus_sigmoid(p[1] + F(L.SOFTPLUS_INV_1))
      e = F(1e-8)
      inv_te, inv = _frcp(th + e), _frcp(th + mu + e)
      l1p = _log1p_small(mu * inv_te)
      lt = _flog(th + mu + e)
      lg, dg = _lgamma_digamma_diff(x, th)
      ell = -th * l1p + x * (_flog(mu + e) - lt) + lg
      d0 = (-th * inv + x * _frcp(mu + e) - x * inv) * g0
      first = (_flog(th + e) - lt) if log_difference else -l1p
      d1 = (first + th * mu * inv_te * inv - x * inv + dg) * g1
    if not L.is_zi(kind):
      return ell.astype(F), [d0.astype(F), d1.astype(F), zero]
    sp, sg = _softplus_sigmoid(p[2])
    dlt = ell - p[2]
    e3 = _fexp(-np.abs(dlt))
    inv3 = _frcp(F(1) + e3)
    lse = np.maximum(p[2], ell) + _log1p_small(e3)
    w = np.where(dlt >= 0, inv3, e3 * inv3).astype(F)
    omw = np.where(dlt >= 0, e3 * inv3, inv3).astype(F)
    at0 = x == 0
    d2z = {"kernel": omw - sg, "one_minus_w": (F(1) - w) - sg, "one_minus_sum": F(1) - (w + sg)}[d2_form]
    llk = np.where(at0, lse, ell) - sp
    return llk.astype(F), [np.where(at0, d0 * w, d0).astype(F), np.where(at0, d1 * w, d1).astype(F), np.where(at0, d2z, -sg).astype(F)]


def _worst(got, ref, bound, keep):
  err = np.where(keep, np.abs(np.asarray(got, np.float64) - ref), 0.0)
  ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
  at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
  return ratio, at


@pytest.mark.parametrize("kind,direct", L.ALL)
def test_float32_replay_stays_inside_the_bound(kind, direct):
  """a correct kernel passes: the replay of count_elem's own operations is inside grad_elem_bound at every kept element, and its
  log-probability inside logprob_elem_bound"""
  x, planes, keep = L.grid_elements(kind, direct)
  llk, d = replay_count_elem(kind, x, planes, direct)
  ref, bound = L.grad_elem(kind, x, planes, direct), L.grad_elem_bound(kind, x, planes, direct)
  for c in range(len(planes)):
    assert d[c].dtype == F
    ratio, at = _worst(d[c], ref[c], bound[c], keep)
    print(f"{kind} direct={direct} d{c}: worst error / bound {ratio.max():.3f} at planes {[float(pl[at[0], 0]) for pl in planes]}, x = {float(x[at])}")
    assert (ratio <= 1.0).all(), (kind, direct, c, float(ratio.max()), [float(pl[at[0], 0]) for pl in planes], float(x[at]), float(d[c][at]), float(ref[c][at]))
  from scipy.special import gammaln
  const = gammaln(x.astype(np.float64) + 1.0) if kind not in ("bernoulli", "normal") else 0.0   # (count_elem's ell leaves the count constant out)
  v = L.log_prob_elem(kind, x, planes, direct)
  ratio, at = _worst(llk.astype(np.float64) - const, v, L.logprob_elem_bound(kind, x, planes, direct), keep)
  print(f"{kind} direct={direct} llk: worst error / bound {ratio.max():.3f}")
  assert (ratio <= 1.0).all(), (kind, direct, float(ratio.max()), [float(pl[at[0], 0]) for pl in planes], float(x[at]))


def _grid_index(planes, point):
  hit = np.ones(len(planes[0]), bool)
  for pl, v in zip(planes, point):
    hit &= pl[:, 0] == F(v)
  assert hit.sum() == 1, point
  return int(np.argmax(hit))


def test_the_gate_gradient_before_the_repair_is_what_the_bound_rejects():
  """(1 - w) - sg with 1 - w formed by subtraction -- count_elem before the repair -- and 1 - (w + sg): both outside the bound at the named
  point 'zinb' (0, -5, gate -40), x = 0 (ell = -0.0067: 1 - w = 4.3e-18, lost whole in 1.f - w), and at every zero count whose gate sits
  17 or more below ell (1 - (w + sg): at the named point and at half of those); the repaired form is inside everywhere (the test above).  The share outside falls as the gate rises: printed
  per gate value."""
  x, planes, keep = L.grid_elements("zinb")
  ref, bound = L.grad_elem("zinb", x, planes)[2], L.grad_elem_bound("zinb", x, planes)[2]
  i = _grid_index(planes, (0.0, -5.0, -40.0))
  ell0 = L.count_terms("zinb", x, planes)["ell0"]
  far = keep[:, 0] & (planes[2][:, 0] - ell0[:, 0] <= -17.0)
  assert far.sum() >= 50
  for form in ("one_minus_w", "one_minus_sum"):
    got = replay_count_elem("zinb", x, planes, d2_form=form)[1][2]
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{form}: at (0, -5, -40), x = 0: got {got[i, 0]:.3e}, reference {ref[i, 0]:.3e}, error / bound {err[i, 0] / bound[i, 0]:.3g}; "
          f"{int((err[far, 0] > bound[far, 0]).sum())} of {int(far.sum())} far points outside")
    assert err[i, 0] > 100.0 * bound[i, 0]
    assert (err[far, 0] > bound[far, 0]).all() if form == "one_minus_w" else (err[far, 0] > bound[far, 0]).sum() * 3 >= far.sum()
    assert (err[:, 1:] <= bound[:, 1:])[keep[:, 1:]].all()          # (x > 0 never takes the branch)
    gate = planes[2][:, 0]
    print("    outside the bound per gate value:", {float(v): f"{int((err[(gate == v) & keep[:, 0], 0] > bound[(gate == v) & keep[:, 0], 0]).sum())}/{int(((gate == v) & keep[:, 0]).sum())}" for v in np.unique(gate)})


def test_the_log_difference_is_what_the_bound_rejects():
  """the 'nbd' dispersion gradient with log(th + e) - log(th + mu + e) formed as a difference of two logarithms (the form smx_loss.h's
  comment warns of): outside the bound at the named point (-20, 40), x = 0 -- the Poisson limit, mu = 2e-9 next to th = 40.5, where
  every term of the gradient is ~5e-11 and the two logarithms are 3.7 -- by more than 1e5 times"""
  x, planes, keep = L.grid_elements("nbd")
  ref, bound = L.grad_elem("nbd", x, planes)[1], L.grad_elem_bound("nbd", x, planes)[1]
  i = _grid_index(planes, (-20.0, 40.0))
  got = replay_count_elem("nbd", x, planes, log_difference=True)[1][1]
  err = np.abs(got.astype(np.float64) - ref)
  print(f"log difference at (-20, 40), x = 0: got {got[i, 0]:.3e}, reference {ref[i, 0]:.3e}, error / bound {err[i, 0] / bound[i, 0]:.3g}")
  assert keep[i, 0] and err[i, 0] > 1e5 * bound[i, 0]
  good = replay_count_elem("nbd", x, planes)[1][1]
  assert np.abs(good.astype(np.float64) - ref)[i, 0] <= bound[i, 0]
