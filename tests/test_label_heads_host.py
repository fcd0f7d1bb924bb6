"""tests/label_heads_ref.py held to account on the host, without a device: its restated values against the oracle's label_llk on an
ordinary batch of every kind; the layers it adds (the mixture over components, 'onehot', the 'mixtril' solves) against mpmath at 60
digits on the whole grid -- from the components' float64 log densities and gradients, which tests/test_likelihood_grad_host.py holds to
mpmath themselves --; a float32 NumPy replay of label_loss_kernel's and label_tril_kernel's branches, operation for operation, inside
the derived bounds (worst error / bound printed per kind and plane: a ratio above 1 here is a mistake in the table, not in a kernel);
three deliberately wrong replays outside them; and the kept-point cap.  The replay is no measurement of the device."""
import mpmath as mp
import numpy as np
import pytest
from scipy.special import gammaln

from tests import head_kinds_ref
from tests import label_heads_ref as R
from tests import likelihood_grad_ref as L
from tests.test_likelihood_grad_host import F, _flog, _frcp, _softplus_sigmoid, replay_count_elem

RATIO = 1e-3      # |reference - mpmath| <= RATIO x the float32 bound
ELEMENTWISE = [k for k in R.ALL_KINDS if k != "onehot" and not k.startswith("mixtril")]
TRIL_SHAPES = [(2, 1), (3, 2), (2, 9), (4, 8), (3, 33)]
ONEHOT_P = (2, 5, 33, 70)


# ---- 1. the oracle on an ordinary batch -----------------------------------------------------------------------------------------------------
def _ordinary(kind, B=6, P=5, seed=3):
  rng = np.random.default_rng(seed)
  base, C = R.split_kind(kind)
  k = R.n_planes(kind, P)
  raw = (0.6 * rng.normal(size=(B, k * P))).astype(np.float32)
  if base in ("normal", "mixgauss", "mixtril"):
    y = rng.normal(size=(B, P))
  elif base == "bernoulli":
    y = rng.integers(0, 2, size=(B, P))
  elif base == "onehot":
    y = np.eye(P)[rng.integers(0, P, size=B)]
  else:
    y = rng.poisson(3.0, size=(B, P))
  return raw, y.astype(np.float32)


def _close(a, b):
  return np.allclose(a, b, rtol=1e-12, atol=1e-12 * max(float(np.abs(b).max()), 1e-300))


@pytest.mark.parametrize("kind", R.ALL_KINDS)
def test_restated_values_are_the_oracles(kind):
  raw, y = _ordinary(kind)
  B, P = y.shape
  base, C = R.split_kind(kind)
  llk, d = head_kinds_ref.label_llk(y.astype(np.float64), raw.astype(np.float64), kind)
  if base == "mixtril":
    a, mu, Lraw, _ = R.tril_unpack(raw, C, P, P)
    o = R.tril(a, mu, Lraw, y)
    da, dmu, dL, _ = R.tril_unpack(d, C, P, P)
    dL = np.tril(dL)                                         # (the oracle's planes hold the lower triangle; what lies above is 0 in both)
    assert _close(o["llk"], llk) and _close(o["dmix"], da) and _close(o["dmu"], dmu) and _close(o["dL"], dL)
    return
  if base == "onehot":
    o = R.onehot(raw, y)
    assert _close(o["v"].sum(axis=1), llk) and _close(o["g"][0], d)
    return
  k = R.n_planes(kind)
  o = R.elem(kind, y, [raw[:, c * P:(c + 1) * P] for c in range(k)])
  assert o["keep"].all()
  assert _close(o["v"].sum(axis=1), llk)
  assert _close(np.concatenate(list(o["g"]), axis=1), d)


# ---- 2. mpmath on the grid --------------------------------------------------------------------------------------------------------------------
def _mp_mixture(a, e):
  """(log sum pi exp(e), resp, pi) of mpf lists"""
  am = max(a)
  lse_a = am + mp.log(sum(mp.exp(v - am) for v in a))
  j = [x + y for x, y in zip(a, e)]
  jm = max(j)
  lse_j = jm + mp.log(sum(mp.exp(v - jm) for v in j))
  return lse_j - lse_a, [mp.exp(v - lse_j) for v in j], [mp.exp(v - lse_a) for v in a]


def _ratio(got, ref_mp, bound):
  err = float(abs(mp.mpf(float(got)) - ref_mp))
  return err / bound if err else 0.0


@pytest.mark.parametrize("kind", [k for k in ELEMENTWISE if k.startswith("mix")])
def test_mixture_layer_agrees_with_mpmath(kind):
  """v, resp - pi and resp d_c of `elem` against 60-digit arithmetic on the components' float64 log densities e_c and gradients d_c, at
  every kept element of the grid"""
  base, C = R.split_kind(kind)
  y, planes, _ = R.grid(kind)
  o = R.elem(kind, y, planes)
  comp = R.MIX_COMPONENT[base]
  kc = 3 if comp == "zinb" else 2
  const = L.count_const(comp, y)
  e = [L.log_prob_elem(comp, y, [planes[(1 + q) * C + c] for q in range(kc)]) + const for c in range(C)]
  worst, at = 0.0, None
  with mp.workdps(60):
    for i in range(len(y)):
      if not o["keep"][i]:
        continue
      lse, resp, pi = _mp_mixture([mp.mpf(float(planes[c][i])) for c in range(C)], [mp.mpf(float(e[c][i])) for c in range(C)])
      rs = [_ratio(o["v"][i], lse - mp.mpf(float(const[i])), o["bv"][i])]
      for c in range(C):
        rs.append(_ratio(o["g"][c, i], resp[c] - pi[c], o["bg"][c, i]))
        for q in range(kc):
          rs.append(_ratio(o["g"][(1 + q) * C + c, i], resp[c] * mp.mpf(float(o["comp_g"][c][q][i])), o["bg"][(1 + q) * C + c, i]))
      if max(rs) > worst:
        worst, at = max(rs), (i, int(np.argmax(rs)))
  print(f"{kind}: {int(o['keep'].sum())} kept elements, worst |ref - mpmath| / bound {worst:.2e} at (element, quantity) {at}")
  assert worst <= RATIO, (kind, worst, at)


@pytest.mark.parametrize("P", ONEHOT_P)
def test_onehot_agrees_with_mpmath(P):
  raw, y = R.onehot_grid(P)
  o = R.onehot(raw, y)
  worst = 0.0
  with mp.workdps(60):
    for i in range(len(raw)):
      r, t = [mp.mpf(float(v)) for v in raw[i]], [mp.mpf(float(v)) for v in y[i]]
      m = max(r)
      lse = m + mp.log(sum(mp.exp(v - m) for v in r))
      ys = sum(t)
      for p in range(P):
        worst = max(worst, _ratio(o["v"][i, p], t[p] * (r[p] - lse), o["bv"][i, p]), _ratio(o["g"][0, i, p], t[p] - mp.exp(r[p] - lse) * ys, o["bg"][0, i, p]))
  print(f"onehot P = {P}: {len(raw)} rows, worst |ref - mpmath| / bound {worst:.2e}")
  assert worst <= RATIO


@pytest.mark.parametrize("C,P", TRIL_SHAPES)
def test_mixtril_agrees_with_mpmath(C, P):
  g = R.tril_grid(C, P)
  o = R.tril(g["a"], g["mu"], g["Lraw"], g["y"])
  assert o["keep"].all()
  worst = 0.0
  with mp.workdps(60):
    for i in range(len(g["a"])):
      e, W, DL = [], [], []
      for c in range(C):
        rd = [mp.mpf(float(g["Lraw"][i, c, p, p])) for p in range(P)]
        d = [mp.log(1 + mp.exp(v)) + mp.mpf(R.TRIL_SHIFT) for v in rd]
        Lm = [[mp.mpf(float(g["Lraw"][i, c, p, j])) if j < p else mp.mpf(0) for j in range(P)] for p in range(P)]
        r = [mp.mpf(float(g["y"][i, p])) - mp.mpf(float(g["mu"][i, c, p])) for p in range(P)]
        u, w = [mp.mpf(0)] * P, [mp.mpf(0)] * P
        for p in range(P):
          u[p] = (r[p] - sum(Lm[p][j] * u[j] for j in range(p))) / d[p]
        for p in range(P - 1, -1, -1):
          w[p] = (u[p] - sum(Lm[q][p] * w[q] for q in range(p + 1, P))) / d[p]
        e.append(-sum(v * v for v in u) / 2 - sum(mp.log(v) for v in d) - mp.mpf(P) / 2 * mp.log(2 * mp.pi))
        W.append(w)
        DL.append([[w[p] * u[j] if j < p else ((w[p] * u[p] - 1 / d[p]) / (1 + mp.exp(-rd[p])) if j == p else mp.mpf(0)) for j in range(P)] for p in range(P)])
      lse, resp, pi = _mp_mixture([mp.mpf(float(v)) for v in g["a"][i]], e)
      worst = max(worst, _ratio(o["llk"][i], lse, o["b_llk"][i]))
      for c in range(C):
        worst = max(worst, _ratio(o["dmix"][i, c], resp[c] - pi[c], o["b_dmix"][i, c]))
        for p in range(P):
          worst = max(worst, _ratio(o["dmu"][i, c, p], resp[c] * W[c][p], o["b_dmu"][i, c, p]))
          for j in range(p + 1):
            worst = max(worst, _ratio(o["dL"][i, c, p, j], resp[c] * DL[c][p][j], o["b_dL"][i, c, p, j]))
  conds = R.tril_conds(C, P)
  print(f"mixtril{C} P = {P}: worst |ref - mpmath| / bound {worst:.2e}; cond_2(L) per (diagonal, target): " + ", ".join(f"{k}: {v[0]:.3g}..{v[1]:.3g}" for k, v in conds.items()))
  assert worst <= RATIO
  for (diag, target), (lo, hi) in conds.items():
    if P >= 2 and diag != "cycle":
      assert target / 1.01 <= lo <= hi <= target * 1.01, (diag, target, lo, hi)


# ---- 3. the float32 replay ------------------------------------------------------------------------------------------------------------------
IDX = np.arange(64)


def _wave_sum(lanes):
  v = np.asarray(lanes, F)
  for s in (32, 16, 8, 4, 2, 1):
    v = (v + v[..., IDX ^ s]).astype(F)
  return v[..., 0]


def _lane_sum(x):
  """sum over the last axis as the kernels do: lane p % 64 adds its columns in order, then wave_sum"""
  x = np.asarray(x, F)
  n = -(-x.shape[-1] // 64) * 64
  x = np.concatenate([x, np.zeros(x.shape[:-1] + (n - x.shape[-1],), F)], axis=-1).reshape(x.shape[:-1] + (n // 64, 64))
  acc = np.zeros(x.shape[:-2] + (64,), F)
  for t in range(x.shape[-2]):
    acc = (acc + x[..., t, :]).astype(F)
  return _wave_sum(acc)


def _lgammaf1(y):
  return gammaln(np.asarray(y, np.float64) + 1.0).astype(F)


def _replay_mix_layer(mx, e, fault=None):
  """the two log-sum-exps, resp and pi of label_loss_kernel / label_tril_kernel over lists of float32 arrays: (lse_j, lse_a, resp, pi)"""
  am = jm = F(R.SENTINEL)
  for a, ec in zip(mx, e):
    am, jm = np.maximum(am, a), np.maximum(jm, (a + ec).astype(F))
  sa = sj = F(0)
  for a, ec in zip(mx, e):
    sa = (sa + np.exp((a - am).astype(F))).astype(F)
    sj = (sj + np.exp(((a + ec).astype(F) - jm).astype(F))).astype(F)
  lse_a, lse_j = (am + np.log(sa)).astype(F), (jm + np.log(sj)).astype(F)
  resp = [np.exp(((a + ec).astype(F) - lse_j).astype(F)) for a, ec in zip(mx, e)]
  pi = [np.exp((a - lse_a).astype(F)) for a in mx]
  return lse_j, lse_a, resp, pi


def replay_elem(kind, y, planes, gs=1.0, fault=None):
  """label_loss_kernel's elementwise branches in NumPy float32: (the summand of the cell's llk, the gradient planes).  fault: 'no_resp' --
  the first parameter plane of component 0 without its resp factor"""
  base, C = R.split_kind(kind)
  y, planes, gs = np.asarray(y, F), [np.asarray(p, F) for p in planes], F(gs)
  with np.errstate(all="ignore"):
    if base in R.SIMPLE:
      llk, d = replay_count_elem(kind, y, planes)
      if base not in ("bernoulli", "normal"):
        llk = (llk - _lgammaf1(y)).astype(F)
      return llk, [(d[c] * gs).astype(F) for c in range(len(planes))]
    comp = R.MIX_COMPONENT[base]
    kc = 3 if comp == "zinb" else 2
    parts = [replay_count_elem(comp, y, [planes[(1 + q) * C + c] for q in range(kc)]) for c in range(C)]
    lse_j, lse_a, resp, pi = _replay_mix_layer(planes[:C], [pt[0] for pt in parts])
    llk = (lse_j - lse_a).astype(F)
    if comp != "normal":
      llk = (llk - _lgammaf1(y)).astype(F)
    out = [((resp[c] - pi[c]).astype(F) * gs).astype(F) for c in range(C)]
    for q in range(kc):
      for c in range(C):
        r = F(1) if (fault == "no_resp" and q == 0 and c == 0) else resp[c]
        out.append(((r * parts[c][1][q]).astype(F) * gs).astype(F))
    return llk, out


def replay_onehot(raw, y, gs=1.0, fault=None):
  """the 'onehot' branch: (llk [R], d [R, P]).  fault: 'no_ysum'"""
  raw, y, gs = np.asarray(raw, F), np.asarray(y, F), F(gs)
  with np.errstate(all="ignore"):
    mx = raw.max(axis=1, keepdims=True)
    ysum = _lane_sum(y)[:, None]
    se = _lane_sum(np.exp((raw - mx).astype(F)))[:, None]
    lse = (mx + np.log(se)).astype(F)
    lp = (raw - lse).astype(F)
    s = np.exp(lp)
    d = (y - (s if fault == "no_ysum" else (s * ysum).astype(F))).astype(F)
    return _lane_sum((y * lp).astype(F)), (d * gs).astype(F)


def replay_tril(a, mu, Lraw, y, gs=1.0, fault=None):
  """label_tril_kernel: (llk [R], dmix [R, C], dmu [R, C, P], dL [R, C, P, P]).  fault: 'no_sg' -- the diagonal gradient without sg"""
  a, mu, Lraw, y, gs = np.asarray(a, F), np.asarray(mu, F), np.asarray(Lraw, F), np.asarray(y, F), F(gs)
  R_, C, P = mu.shape
  lanes = np.arange(P)
  es, keep = [], []
  with np.errstate(all="ignore"):
    for c in range(C):
      sp, sg = _softplus_sigmoid(Lraw[:, c, lanes, lanes])
      lpp = (sp + F(1e-5)).astype(F)
      inv = _frcp(lpp)
      Lm = np.where(lanes[:, None] > lanes[None, :], Lraw[:, c], F(0)).astype(F)
      r, u = (y - mu[:, c]).astype(F), np.zeros((R_, P), F)
      for j in range(P):
        uj = (r[:, j] * inv[:, j]).astype(F)
        u[:, j] = uj
        r = np.where(lanes[None, :] > j, (r - (Lm[:, :, j] * uj[:, None]).astype(F)).astype(F), r)
      sw, w = u.copy(), np.zeros((R_, P), F)
      for i in range(P - 1, -1, -1):
        wi = (sw[:, i] * inv[:, i]).astype(F)
        w[:, i] = wi
        sw = np.where(lanes[None, :] < i, (sw - (Lm[:, i, :] * wi[:, None]).astype(F)).astype(F), sw)
      quad, logdet = _lane_sum((u * u).astype(F)), _lane_sum(_flog(lpp))
      es.append(((F(-0.5) * quad).astype(F) - logdet - (F(R.HALF_LOG_2PI) * F(P)).astype(F)).astype(F))
      wu = (w[:, :, None] * u[:, None, :]).astype(F)
      dL = np.where(lanes[:, None] > lanes[None, :], wu, F(0)).astype(F)
      dd = (wu[:, lanes, lanes] - inv).astype(F)
      dL[:, lanes, lanes] = dd if fault == "no_sg" else (dd * sg).astype(F)
      keep.append((w, dL))
    lse_j, lse_a, resp, pi = _replay_mix_layer([a[:, c] for c in range(C)], es)
    dmix = np.stack([((resp[c] - pi[c]).astype(F) * gs).astype(F) for c in range(C)], axis=1)
    dmu = np.stack([((resp[c][:, None] * keep[c][0]).astype(F) * gs).astype(F) for c in range(C)], axis=1)
    dL = np.stack([((resp[c][:, None, None] * keep[c][1]).astype(F) * gs).astype(F) for c in range(C)], axis=1)
    return (lse_j - lse_a).astype(F), dmix, dmu, dL


def _worst(got, ref, bound, keep):
  got = np.asarray(got, np.float64)
  assert not (np.isnan(got) & keep).any()
  err = np.where(keep, np.abs(got - ref), 0.0)
  ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
  return float(ratio.max()), np.unravel_index(int(np.argmax(ratio)), ratio.shape)


def _elem_ratios(kind, fault=None, gs=1.0):
  y, planes, _ = R.grid(kind)
  o = R.elem(kind, y, planes)
  llk, d = replay_elem(kind, y, planes, gs, fault)
  out = {"llk": _worst(llk, o["v"], o["bv"], o["keep"])}
  for c in range(len(planes)):
    g, bg = R.scale_grad(o["g"][c], o["bg"][c], gs)
    out[f"d{c}"] = _worst(d[c], g, bg, o["keep"])
  return out, y, planes


@pytest.mark.parametrize("kind", ELEMENTWISE)
def test_replay_of_the_elementwise_branches_stays_inside_the_bound(kind):
  for gs in (1.0, -0.7 / 37.0):
    out, y, planes = _elem_ratios(kind, gs=gs)
    print(f"{kind} grad_scale {gs:.4g}: worst error / bound (CPU replay) " + ", ".join(f"{n} {r:.3f}" for n, (r, _) in out.items()))
    for n, (r, at) in out.items():
      assert r <= 1.0, (kind, n, r, float(y[at]), [float(p[at]) for p in planes])


def test_replay_of_a_cell_sum_stays_inside_the_bound():
  """the lane chain and wave_sum over cells of 70 dimensions (two passes): cell_sum_bound"""
  for kind in ("nb", "zinbd", "normal", "mixnb2", "mixgauss3"):
    y, planes, _ = R.grid(kind)
    P = 70
    B = len(y) // P
    o = R.elem(kind, y, planes)
    llk, _ = replay_elem(kind, y, planes)
    cut = lambda v: np.asarray(v)[:B * P].reshape(B, P)
    ref, bound = R.cell_sum_bound(kind, P, cut(o["v"]), cut(o["bv"]))
    r, at = _worst(_lane_sum(cut(llk)), ref, bound, cut(o["keep"]).all(axis=1))
    print(f"{kind}: cell sums over {P} dimensions, worst error / bound (CPU replay) {r:.3f}")
    assert r <= 1.0, (kind, r, at)


@pytest.mark.parametrize("P", ONEHOT_P)
def test_replay_of_onehot_stays_inside_the_bound(P):
  raw, y = R.onehot_grid(P)
  o = R.onehot(raw, y)
  for gs in (1.0, -0.7 / 37.0):
    llk, d = replay_onehot(raw, y, gs)
    g, bg = R.scale_grad(o["g"][0], o["bg"][0], gs)
    rd, at = _worst(d, g, bg, o["keep"])
    ref, bound = R.cell_sum_bound("onehot", P, o["v"], o["bv"])
    rl, _ = _worst(llk, ref, bound, np.ones(len(raw), bool))
    print(f"onehot P = {P} grad_scale {gs:.4g}: worst error / bound (CPU replay) d0 {rd:.3f}, llk {rl:.3f}")
    assert rd <= 1.0 and rl <= 1.0, (P, rd, rl, at)


def _tril_ratios(C, P, fault=None, gs=1.0):
  g = R.tril_grid(C, P)
  o = R.tril(g["a"], g["mu"], g["Lraw"], g["y"])
  llk, dmix, dmu, dL = replay_tril(g["a"], g["mu"], g["Lraw"], g["y"], gs, fault)
  k = o["keep"]
  out = {"llk": _worst(llk, o["llk"], o["b_llk"], k)}
  low = np.tril(np.ones((P, P), bool), -1)
  eye = np.eye(P, dtype=bool)
  for name, got, where in (("d logit", dmix, None), ("d mu", dmu, None), ("d L below", dL, low), ("d L diagonal", dL, eye)):
    key = {"d logit": "dmix", "d mu": "dmu"}.get(name, "dL")
    ref, b = R.scale_grad(o[key], o["b_" + key], gs)
    kk = np.broadcast_to(k.reshape((-1,) + (1,) * (ref.ndim - 1)), ref.shape) & (True if where is None else where)
    out[name] = _worst(got, ref, b, kk)
  assert (dL[:, :, np.triu(np.ones((P, P), bool), 1)] == 0).all()
  return out


@pytest.mark.parametrize("C,P", TRIL_SHAPES + [(4, 64)])
def test_replay_of_mixtril_stays_inside_the_bound(C, P):
  for gs in (1.0, -0.7 / 37.0):
    out = _tril_ratios(C, P, gs=gs)
    print(f"mixtril{C} P = {P} grad_scale {gs:.4g}: worst error / bound (CPU replay) " + ", ".join(f"{n} {r:.3f}" for n, (r, _) in out.items()))
    for n, (r, at) in out.items():
      assert r <= 1.0, (C, P, n, r, at)


# ---- 4. wrong replays lie outside -------------------------------------------------------------------------------------------------------------
def test_a_dropped_resp_factor_lies_outside_the_bound():
  for kind in ("mixnb2", "mixgauss3", "mixzinb2"):
    C = R.split_kind(kind)[1]
    out, _, _ = _elem_ratios(kind, fault="no_resp")
    print(f"{kind} without resp on component 0's first parameter plane: " + ", ".join(f"{n} {r:.3g}" for n, (r, _) in out.items()))
    assert out[f"d{C}"][0] > 1.0 and all(r <= 1.0 for n, (r, _) in out.items() if n != f"d{C}")


def test_an_onehot_gradient_without_ysum_lies_outside_the_bound():
  raw, y = R.onehot_grid(33)
  o = R.onehot(raw, y)
  _, d = replay_onehot(raw, y, fault="no_ysum")
  err = np.abs(d.astype(np.float64) - o["g"][0])
  rows = np.abs(y.sum(axis=1) - 1.0) > 0.25                       # (all-zero, multi-hot and 2.5-sum targets; a row summing to 1 cannot tell)
  print(f"onehot without ysum: worst error / bound {float((err / o['bg'][0]).max()):.3g}; rows outside {int((err > o['bg'][0]).any(axis=1).sum())} of {len(raw)}")
  assert (err > o["bg"][0]).any(axis=1)[rows].all() and not (err > o["bg"][0])[~rows].any()


def test_a_mixtril_diagonal_without_sg_lies_outside_the_bound():
  out = _tril_ratios(3, 9, fault="no_sg")
  print("mixtril3 P = 9 without sg on the diagonal: " + ", ".join(f"{n} {r:.3g}" for n, (r, _) in out.items()))
  assert out["d L diagonal"][0] > 1.0 and all(r <= 1.0 for n, (r, _) in out.items() if n != "d L diagonal")


# ---- 5. the kept-point cap ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ELEMENTWISE)
def test_kept_point_cap(kind):
  """per (kind, plane, axis family): at most a tenth of the elements dropped, every reference value and bound of a kept element finite,
  and no axis value of a plane lost wholesale"""
  y, planes, fam = R.grid(kind)
  o = R.elem(kind, y, planes)
  keep = o["keep"]
  for w in np.unique(fam):
    dropped = int((~keep[fam == w]).sum())
    print(f"{kind} family {int(w)}: {dropped} of {int((fam == w).sum())} elements dropped")
    assert dropped * 10 <= (fam == w).sum(), (kind, w)
  for n in ("v", "bv", "g", "bg"):
    assert np.isfinite(o[n][..., keep]).all(), (kind, n)
  assert (o["bv"][keep] >= 0).all() and (o["bg"][:, keep] >= 0).all()
  for c, pl in enumerate(planes):
    assert set(np.unique(pl)) == set(np.unique(pl[keep])), (kind, c)


def test_all_components_out_of_range_is_a_named_family():
  """the rule this module adds to grad_in_range: every joint below the kernels' starting maximum -3e38"""
  m = R._mixture(np.zeros((1, 2)), np.array([[-3.3e38, -1.0]]), np.zeros((1, 2)))
  assert list(m["all_out"]) == [True, False]


def test_mixzinb_patterns_meet_every_grid_point_and_every_count():
  """'mixzinb' cycles the six logit patterns with the element instead of crossing them (label_heads_ref's docstring): every (grid point,
  pattern) pair and every (count, pattern) pair is on the grid all the same, for every walking component"""
  for C in (2, 3, 4):
    y, planes, fam = R.grid(f"mixzinb{C}")
    n = len(y) // C
    a = np.stack(planes[:C], axis=1)
    pat = [PATTERN_OF[tuple(sorted(row))] for row in a.astype(np.float64)]
    for w in range(C):
      sl = slice(w * n, (w + 1) * n)
      assert (fam[sl] == w).all()
      point, count = np.arange(n) // 7, y[sl]
      assert len({(int(p), q) for p, q in zip(point, pat[sl])}) == (n // 7) * len(R.PATTERNS)
      assert len({(float(c), q) for c, q in zip(count, pat[sl])}) == 7 * len(R.PATTERNS)


PATTERN_OF = {}
for _C in (2, 3, 4):
  for _p in R.PATTERNS:
    PATTERN_OF[tuple(sorted(R.mix_logits(_p, _C, 0)))] = _p
