"""tests/latent_terms_ref.py held to account on the host: its float64 values against mpmath (120 digits) at every point of the edge grid,
the float32 NumPy replay of the kernels' lines (denormals kept) inside the derived bounds at every kept point, the replay with denormal
operands of v_log / v_rcp / v_exp flushed and the replay of the lines before the repair (where they leave the bounds is printed: what a device
result is read against), and the kept-point count.  The replay checks the derivation of the bounds; it is no measurement of the device."""
import mpmath as mp
import numpy as np
import pytest

from tests import latent_terms_ref as T

RATIO = 1e-3      # |reference - mpmath| <= RATIO x the float32 bound, at every point (tests/test_likelihood_grad_host.py's)


def _mp_sp(v):
  return mp.log1p(mp.exp(v))


def _mp_sig(v):
  return 1 / (1 + mp.exp(-v))


def _mp_diag(mu, raw, eps):
  x = mp.mpf(float(raw)) + mp.log(mp.expm1(1))
  mu, eps = mp.mpf(float(mu)), mp.mpf(float(eps))
  sg = _mp_sp(x)
  z = mu + sg * eps
  return dict(sigma=sg, z=z, kl=(sg * sg + mu * mu - 1 - 2 * mp.log(sg)) / 2, dmu=mu, draw=(sg - 1 / sg) * _mp_sig(x),
              w=-z * z / 2 + eps * eps / 2 + mp.log(sg))


def _mp_lib(mu, raw, eps, mp_, vp):
  x = mp.mpf(float(raw)) + mp.log(mp.expm1(1))
  mu, eps, m0, vp = mp.mpf(float(mu)), mp.mpf(float(eps)), mp.mpf(float(mp_)), mp.mpf(float(vp))
  sg = _mp_sp(x)
  l = mu + sg * eps
  return dict(sigma=sg, z=l, kl=mp.log(mp.sqrt(vp) / sg) + (sg * sg + (mu - m0) ** 2) / (2 * vp) - mp.mpf(1) / 2, dmu=(mu - m0) / vp,
              draw=(sg / vp - 1 / sg) * _mp_sig(x), w=-(l - m0) ** 2 / (2 * vp) - mp.log(vp) / 2 + eps * eps / 2 + mp.log(sg))


def _points(which):
  """(mu, raw, eps, keys): the KL and its partials on the product grid (at eps = 0), the sample and the weight one axis at a time"""
  if which == "product":
    mu, raw = T.kl_grid()
    return mu, raw, np.zeros_like(mu), ("sigma", "kl", "dmu", "draw")
  mu, raw, eps = T.axis_grid()
  return mu, raw, eps, ("sigma", "z", "w", "kl", "draw")


def _dropped_ok(got, ref):
  """a dropped point: no NaN; where the true value overflows float32 the result is +-inf of the right sign or a finite float"""
  got = np.asarray(got, np.float64)
  return ~np.isnan(got) & (np.isfinite(got) | (np.sign(got) == np.sign(ref)))


@pytest.mark.parametrize("which", ["product", "axes"])
def test_diagonal_reference_agrees_with_mpmath(which):
  mu, raw, eps, keys = _points(which)
  ref, bound = T.diag_terms(mu, raw, eps), T.diag_bounds(mu, raw, eps)
  worst = {k: 0.0 for k in keys}
  with mp.workdps(120):
    for i in range(mu.size):
      m = _mp_diag(mu[i], raw[i], eps[i])
      for k in keys:
        assert T.kept(ref[k][i]), (k, i)
        r = float(abs(mp.mpf(float(ref[k][i])) - m[k])) / float(bound[k][i])
        worst[k] = max(worst[k], r)
        assert r <= RATIO, (which, k, float(mu[i]), float(raw[i]), float(eps[i]), float(ref[k][i]), float(m[k]), r)
  print(f"diagonal head, {which} grid ({mu.size} points): worst |ref - mpmath| / bound {worst}")


def test_library_reference_agrees_with_mpmath():
  worst = {}
  with mp.workdps(120):
    for mp_, vp in T.LIB_PRIORS:
      for which in ("product", "axes"):
        mu, raw, eps, keys = _points(which)
        ref, bound = T.lib_terms(mu, raw, eps, mp_, vp), T.lib_bounds(mu, raw, eps, mp_, vp)
        for i in range(mu.size):
          m = _mp_lib(mu[i], raw[i], eps[i], np.float32(mp_), np.float32(vp))
          for k in keys:
            # (the float32 prior is the input: the reference takes the same rounded numbers)
            rf = T.lib_terms(mu[i], raw[i], eps[i], np.float32(mp_), np.float32(vp))[k]
            bd = T.lib_bounds(mu[i], raw[i], eps[i], np.float32(mp_), np.float32(vp))[k]
            r = float(abs(mp.mpf(float(rf)) - m[k])) / float(bd)
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= RATIO, (mp_, vp, which, k, float(mu[i]), float(raw[i]), float(eps[i]), float(rf), float(m[k]), r)
        assert np.isfinite(bound["kl"]).all() and np.isfinite(ref["kl"]).all()
  print(f"library latent: worst |ref - mpmath| / bound {worst}")


def _tril_cases():
  for D in T.TRIL_DIMS:
    for s, dr in enumerate(T.RAW_AXIS):
      yield D, dr, T.tril_case(D, dr, T.TRIL_LOWER, seed=s)


def test_tril_reference_agrees_with_mpmath():
  worst = 0.0
  with mp.workdps(120):
    for D, dr, (mu, raw, eps) in _tril_cases():
      ref, bound = T.tril_terms(mu, raw, eps), T.tril_bounds(mu, raw, eps)
      kl = mp.mpf(0)
      for i in range(D):
        lii = _mp_sp(mp.mpf(float(raw[i, i]))) + mp.mpf(T.TRIL_SHIFT)
        fro = sum((mp.mpf(float(raw[i, j])) ** 2 for j in range(i)), mp.mpf(0))
        z = mp.mpf(float(mu[i])) + sum((mp.mpf(float(raw[i, j])) * mp.mpf(float(eps[j])) for j in range(i)), mp.mpf(0)) + lii * mp.mpf(float(eps[i]))
        row = (fro + lii * lii + mp.mpf(float(mu[i])) ** 2 - 1) / 2 - mp.log(lii)
        kl += row
        dii = (lii - 1 / lii) * _mp_sig(mp.mpf(float(raw[i, i])))
        for name, got, want, bd in (("z", ref["z"][i], z, bound["z"][i]), ("kl_rows", ref["kl_rows"][i], row, bound["kl_rows"][i]),
                                    ("draw_ii", ref["draw"][i, i], dii, bound["draw"][i, i]), ("diag", ref["diag"][i], lii, bound["diag"][i])):
          r = float(abs(mp.mpf(float(got)) - want)) / float(bd)
          worst = max(worst, r)
          assert r <= RATIO, (D, dr, i, name, float(got), float(want), r)
      r = float(abs(mp.mpf(float(ref["kl"])) - kl)) / float(bound["kl"])
      worst = max(worst, r)
      assert r <= RATIO, (D, dr, "kl", r)
      assert np.array_equal(ref["draw"][np.triu_indices(D, 1)], np.zeros(D * (D - 1) // 2))
      assert np.array_equal(np.tril(ref["draw"], -1), np.tril(raw.astype(np.float64), -1))
  print(f"tril head: worst |ref - mpmath| / bound {worst:.3g}")


def test_kept_points():
  """The issue allows the location column 1e19 and the raw-scale row 1e4 to drop.  The diagonal and the tril head drop NOTHING on this grid
  (mu^2 = 1e38 and sigma^2 = 1e8 are below 2^127).  The library latent drops its KL and its weight term at the locations +-1e19 under the prior
  (7, 1e-6) alone -- (mu - mp)^2 / (2 vp) = 5e43 --: 2 x 16 points of the product grid, 2 + 2 of the axes; every gradient stays kept."""
  dropped = {}
  for which in ("product", "axes"):
    mu, raw, eps, keys = _points(which)
    fams = [("diagonal", T.diag_terms(mu, raw, eps))] + [(f"library {a, b}", T.lib_terms(mu, raw, eps, np.float32(a), np.float32(b))) for a, b in T.LIB_PRIORS]
    for fam, terms in fams:
      for k in keys:
        keep = T.kept(terms[k])
        assert (keep | (np.abs(mu) >= 1e19) | (raw >= 1e4)).all(), (which, fam, k)
        if k in ("dmu", "draw", "sigma", "z"):
          assert keep.all(), (which, fam, k)
        dropped[fam] = dropped.get(fam, 0) + int((~keep).sum())
  dropped["tril"] = 0
  for D, dr, (mu, raw, eps) in _tril_cases():
    t = T.tril_terms(mu, raw, eps)
    dropped["tril"] += int((~T.kept(t["z"])).sum() + (~T.kept(t["kl_rows"])).sum() + (~T.kept(t["draw"])).sum())
  print(f"dropped points: {dropped}")
  assert dropped == {"diagonal": 0, "library (7.0, 0.3)": 0, "library (7.0, 1e-06)": 36, "library (0.0, 10000.0)": 0, "tril": 0}


def _replay_check(label, got, ref, bound, keys, must_hold, floor=None):
  """per key: the worst error / bound over the kept points; returns {key: points outside (NaN counts as outside)}.  floor: the points at or above
  DRAW_FLOOR -- below it the diagonal head's scale gradient is held to "no NaN" only"""
  out = {}
  for k in keys:
    keep = T.kept(ref[k])
    if floor is not None and k == "draw":
      if must_hold:
        assert not np.isnan(np.asarray(got[k], np.float64)[~floor]).any(), (label, k)
      keep = keep & floor
    err = np.abs(np.asarray(got[k], np.float64) - ref[k])
    bad = keep & ~(err <= bound[k])
    with np.errstate(invalid="ignore"):
      ratio = np.where(keep & (err > 0), err / bound[k], 0.0)
    worst = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("nan")
    print(f"  {label} {k}: worst replay / bound {worst:.3g}; outside at {int(bad.sum())} of {int(keep.sum())} kept points")
    assert _dropped_ok(np.asarray(got[k])[~keep], ref[k][~keep]).all(), (label, k)
    if must_hold:
      assert not bad.any(), (label, k, np.nonzero(bad)[0][:8].tolist(), np.asarray(got[k])[bad][:4], ref[k][bad][:4])
    out[k] = np.nonzero(bad)[0]
  return out


@pytest.mark.parametrize("which", ["product", "axes"])
def test_replay_with_denormals_kept_is_inside_the_bounds(which):
  mu, raw, eps, keys = _points(which)
  rp = T.Replay(flush=False)
  ref, bound = T.diag_terms(mu, raw, eps), T.diag_bounds(mu, raw, eps)
  _replay_check(f"diagonal {which}", rp.diag(mu, raw, eps), ref, bound, keys, True, floor=T.above_floor(raw))
  for a, b in T.LIB_PRIORS:
    a, b = np.float32(a), np.float32(b)
    _replay_check(f"library ({float(a)}, {float(b):g}) {which}", rp.lib(mu, raw, eps, a, b), T.lib_terms(mu, raw, eps, a, b), T.lib_bounds(mu, raw, eps, a, b), keys, True)


def test_tril_replay_is_inside_the_bounds():
  for flush in (False, True):      # (L_ii >= 1e-5: no denormal reaches v_log / v_rcp; both modes hold)
    rp = T.Replay(flush=flush)
    worst = 0.0
    for D, dr, (mu, raw, eps) in _tril_cases():
      ref, bound, got = T.tril_terms(mu, raw, eps), T.tril_bounds(mu, raw, eps), rp.tril(mu, raw, eps)
      for k in ("diag", "z", "kl_rows", "draw", "kl"):
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        assert (err <= bound[k]).all(), (flush, D, dr, k, float(np.max(err / bound[k])))
        worst = max(worst, float(np.max(err / bound[k])))
    print(f"tril replay (flush {flush}): worst replay / bound {worst:.3g}")


@pytest.mark.parametrize("which", ["product", "axes"])
def test_flushed_replay_and_the_lines_before_the_repair(which):
  """What a flushing instruction does, and what the unrepaired lines did.  The repaired lines hold in BOTH modes (sigma's own flush is the bound's
  2^-126; the scale's gradient, whose lines a training step keeps, from DRAW_FLOOR up and without a NaN below it); the old lines leave the bound from raw = -88 down: flushed, the KL is +inf, the scale's gradient NaN, the weight term -inf; with
  denormals kept the gradient at raw = -100 (1 / sigma = 1.6e43: no float32) is still -inf."""
  mu, raw, eps, keys = _points(which)
  ref, bound = T.diag_terms(mu, raw, eps), T.diag_bounds(mu, raw, eps)
  print(f"repaired lines, flushed ({which}):")
  _replay_check("diagonal", T.Replay(True).diag(mu, raw, eps), ref, bound, keys, True, floor=T.above_floor(raw))
  for a, b in T.LIB_PRIORS:
    a, b = np.float32(a), np.float32(b)
    _replay_check(f"library ({float(a)}, {float(b):g})", T.Replay(True).lib(mu, raw, eps, a, b), T.lib_terms(mu, raw, eps, a, b), T.lib_bounds(mu, raw, eps, a, b), keys, True)
  for flush in (True, False):
    print(f"lines before the repair, flush {flush} ({which}):")
    got = T.Replay(flush).diag(mu, raw, eps, repaired=False)
    out = _replay_check("diagonal", got, ref, bound, keys, False, floor=np.ones(raw.shape, bool))
    for k in [k for k in ("kl", "draw", "w") if k in keys]:
      exits = sorted(set(float(v) for v in raw[out[k]]))
      print(f"    {k} leaves the bound at raw scales {exits}: {[float(v) for v in np.asarray(got[k])[out[k]][:3]]} for {[float(v) for v in ref[k][out[k]][:3]]}")
      # non-finite results: never above the last raw scale with a normal sigma
      wild = sorted(set(float(v) for v in raw[out[k]][~np.isfinite(np.asarray(got[k], np.float64)[out[k]])]))
      assert all(v <= -88.0 for v in wild), (k, wild)
      if k == "draw" or flush:
        assert -100.0 in exits, (k, flush)                         # the old lines DO fail: the repair is needed
