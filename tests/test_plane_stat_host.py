"""tests/plane_stat_ref.py held to account on the host: the float64 reference against mpmath (120 digits: 50 and more) on the whole edge grid, the
grid condition and its dropped share, and a float32 NumPy replay of the statistic kernels' formulas (smx_predict.hip's plane_moments
and rv_moments as repaired: the gate complement as sigmoidf(-g)) inside the derived bounds.  The replay checks the derivation of the
bounds; it is no measurement of the device."""
import mpmath as mp
import numpy as np
import pytest

from tests import plane_stat_ref as R

ALL = [(k, False) for k in R.KINDS] + [("nbd", True), ("zinbd", True)]


def _grid(kind, direct):
  """the planes the comparisons run on: the kept grid points and the moderate points; direct: the activated mean and dispersion of them"""
  bias, n_grid, dropped = R.bias_grid(kind)
  planes = [b[:n_grid - dropped + 3] for b in bias]
  if direct:
    s = R.parts(kind, planes)
    planes = [s["mc"].astype(np.float32), s["disp"].astype(np.float32)] + planes[2:]
    keep = R.in_range(kind, planes, True)
    planes = [p[keep] for p in planes]
  return planes


@pytest.mark.parametrize("kind", R.KINDS)
def test_grid_condition_drops_at_most_a_tenth(kind):
  bias, n_grid, dropped = R.bias_grid(kind)
  print(f"{kind}: {dropped} of {n_grid} grid points outside the float32 range")
  assert dropped * 10 <= n_grid, (kind, dropped, n_grid)
  assert bias.shape == (R.N_PLANES[kind], R.G_GRID) and R.G_GRID % 4 and R.G_GRID > 4 * 256
  assert R.in_range(kind, list(bias)).all()
  pts = R.grid_points(kind)
  for c, axis in enumerate(R.AXES[kind]):   # no axis value is lost for a whole kind
    kept = R.in_range(kind, list(pts.T))
    assert set(np.float32(axis)) == set(pts[kept, c]), (kind, c)


def test_scvi_grid_is_in_range_at_a_unit_rate():
  pts = R.grid_points("zinbd", scvi=True)
  planes = [np.ones(len(pts), np.float32), np.exp(pts[:, 0].astype(np.float64)).astype(np.float32), pts[:, 1]]
  keep = R.in_range("zinbd", planes, True)
  assert (~keep).sum() * 10 <= len(pts)


# ---- mpmath ---------------------------------------------------------------------------------------------------------------------------
def _mp_sp(x):
  return mp.log1p(mp.exp(x))


def _mp_point(kind, p, direct, x):
  """(mean, var, count mean, count var, log_prob, count log_prob) of one point in mpmath, the textbook formulas"""
  p = [mp.mpf(float(v)) for v in p]
  x = mp.mpf(float(x))
  c1 = mp.log(mp.expm1(1))
  if kind == "mse":
    return p[0], mp.mpf(0), p[0], mp.mpf(0), -(x - p[0]) ** 2, -(x - p[0]) ** 2
  if kind == "bernoulli":
    pr = 1 / (1 + mp.exp(-p[0]))
    lp = x * p[0] - _mp_sp(p[0])
    return pr, pr * (1 - pr), pr, pr * (1 - pr), lp, lp
  if kind == "normal":
    sd = _mp_sp(p[1] + c1)
    lp = -((x - p[0]) / sd) ** 2 / 2 - mp.log(sd) - mp.log(2 * mp.pi) / 2
    return p[0], sd * sd, p[0], sd * sd, lp, lp
  if kind in ("nb", "zinb"):
    r, el = mp.exp(p[0]), mp.exp(p[1])
    mc, vc = r * el, r * el * (1 + el)
    ell = mp.loggamma(x + r) - mp.loggamma(r) - mp.loggamma(x + 1) + x * (p[1] - _mp_sp(p[1])) - r * _mp_sp(p[1])
  else:
    mu, th = (p[0], p[1]) if direct else (_mp_sp(p[0]), _mp_sp(p[1] + c1))
    e = mp.mpf(R.EPS)
    mc, vc = mu, mu + mu * mu / th
    lt = mp.log(th + mu + e)
    ell = th * (mp.log(th + e) - lt) + x * (mp.log(mu + e) - lt) + mp.loggamma(x + th) - mp.loggamma(th) - mp.loggamma(x + 1)
  if not R.is_zi(kind):
    return mc, vc, mc, vc, ell, ell
  pi = 1 / (1 + mp.exp(-p[2]))
  lp = (mp.log(pi + (1 - pi) * mp.exp(ell)) if x == 0 else mp.log(1 - pi) + ell)
  return (1 - pi) * mc, (1 - pi) * (vc + pi * mc * mc), mc, vc, lp, ell


@pytest.mark.parametrize("kind,direct", ALL)
def test_reference_agrees_with_mpmath(kind, direct):
  """every statistic of the float64 reference within 1e-13 relative of 120-digit arithmetic on the whole grid: no cancellation is left in
  it.  ('mse': the reference divides by the row width, the mpmath value by the same.)"""
  planes = _grid(kind, direct)
  n = len(planes[0])
  t = R.targets(kind, n)
  got = [*R.moments(kind, planes, direct), *R.moments(kind, planes, direct, True)]
  lp = [(R.log_prob_elem(kind, row, planes, direct), R.log_prob_elem(kind, row, planes, direct, True)) for row in t]
  worst = 0.0
  with mp.workdps(120):   # (the textbook zero term log(pi + (1 - pi) exp(ell)) is 1 - 6.6e-40 at a gate of 80: 50 digits leave it 10)
    for g in range(n):
      pt = [pl[g] for pl in planes]
      for j, row in enumerate(t):
        ref = _mp_point(kind, pt, direct, row[g])
        pairs = list(zip(got, ref[:4])) if j == 0 else []
        scale = n if kind == "mse" else 1
        pairs += [(lp[j][0], ref[4] / scale), (lp[j][1], ref[5] / scale)]
        for a, b in pairs:
          a = a[g]
          err = abs(mp.mpf(float(a)) - b)
          rel = float(err / abs(b)) if b != 0 else float(err)
          worst = max(worst, rel)
          assert rel <= 1e-13, (kind, direct, g, [float(v) for v in pt], float(row[g]), float(a), mp.nstr(b, 20))
  print(f"{kind} direct={direct}: {n} points, worst relative difference from mpmath {worst:.2e}")


# ---- the float32 replay ----------------------------------------------------------------------------------------------------------------
F = np.float32


def _fexp(x):
  return np.exp2(F(x) * F(1.4426950408889634))


def _flog(x):
  return np.log2(F(x)) * F(0.6931471805599453)


def _log1p_small(e):
  ser = e * (F(1) - e * (F(0.5) - e * (F(0.33333334) - e * (F(0.25) - e * F(0.2)))))
  return np.where(e < F(0.03125), ser, _flog(F(1) + e))


def _softplus(x):
  return np.maximum(x, F(0)) + _log1p_small(_fexp(-np.abs(x)))


def _sigmoidf(x):
  e = _fexp(-np.abs(x))
  s = F(1) / (F(1) + e)
  return np.where(x >= 0, s, e * s)


def replay_moments(kind, planes, direct=False, count_only=False):
  """plane_moments / rv_moments in NumPy float32, operation for operation"""
  p = [np.asarray(v, F) for v in planes]
  c1 = F(R.SOFTPLUS_INV_1)
  with np.errstate(over="ignore", under="ignore"):
    if kind == "mse":
      return p[0], np.zeros_like(p[0])
    if kind == "bernoulli":
      return F(1) / (F(1) + np.exp(-p[0])), _sigmoidf(p[0]) * _sigmoidf(-p[0])
    if kind == "normal":
      sd = _softplus(p[1] + c1)
      return p[0], sd * sd
    if kind in ("nb", "zinb"):
      el = np.exp(p[1])
      mc = np.exp(p[0]) * el
      vc = mc * (F(1) + el)
    else:
      mu, th = (p[0], p[1]) if direct else (_softplus(p[0]), _softplus(p[1] + c1))
      mc, vc = mu, mu * (F(1) + mu / th)
    if R.is_zi(kind) and not count_only:
      pi, q = F(1) / (F(1) + np.exp(-p[2])), _sigmoidf(-p[2])
      mc, vc = q * mc, q * (vc + pi * mc * mc)
  assert mc.dtype == F and vc.dtype == F
  return mc, vc


@pytest.mark.parametrize("count_only", [False, True])
@pytest.mark.parametrize("kind,direct", ALL)
def test_float32_replay_stays_inside_the_bound(kind, direct, count_only):
  planes = _grid(kind, direct)
  got = replay_moments(kind, planes, direct, count_only)
  ref = R.moments(kind, planes, direct, count_only)
  for stat, a, b in zip(("mean", "variance"), got, ref):
    bound = R.stat_bound(kind, stat, planes, direct, count_only) * np.abs(b)
    err = np.abs(a.astype(np.float64) - b)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    print(f"{kind} direct={direct} count_only={count_only} {stat}: worst error / bound {ratio.max():.3f}")
    assert (err <= bound).all(), (stat, float(ratio.max()), [float(v[int(ratio.argmax())]) for v in planes])


def test_the_unrepaired_formula_is_what_the_bound_rejects():
  """1 - pi in float32 (the formula before the repair) on the zinb grid: inside the bound up to a gate logit of 1, outside it from 8 on,
  exactly 0 from 17 on -- the table of the issue this file answers"""
  bias, n_grid, dropped = R.bias_grid("zinb")
  planes = [b[:n_grid - dropped] for b in bias]
  mc, _ = replay_moments("zinb", planes, count_only=True)
  with np.errstate(over="ignore"):
    pi = F(1) / (F(1) + np.exp(-planes[2]))
  old = (F(1) - pi) * mc
  ref, _ = R.moments("zinb", planes)
  rel = np.abs(old.astype(np.float64) - ref) / ref
  bound = R.stat_bound("zinb", "mean", planes)
  g = planes[2]
  assert (rel[g <= 1] <= bound[g <= 1]).all()
  assert (rel[g >= 8] > bound[g >= 8]).all()
  assert (old[g >= 17] == 0).all()


def test_logprob_bound_is_finite_and_above_the_summation_term():
  for kind, direct in ALL:
    planes = _grid(kind, direct)
    t = R.targets(kind, len(planes[0]))
    for co in (False, True):
      b = R.logprob_elem_bound(kind, t, planes, direct, co)
      v = R.log_prob_elem(kind, t, planes, direct, co)
      assert b.shape == v.shape == t.shape and np.isfinite(b).all() and np.isfinite(v).all(), (kind, direct, co)
      assert (b >= np.abs(v) * R.U).all()
