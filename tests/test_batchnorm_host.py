"""tests/batchnorm_ref.py held to its own claims on the CPU: the float64 reference against mpmath at 120 digits on the whole edge grid, the
composed forward -> backward against torch's float64 autograd, the float32 replay of the kernels' lines inside every bound at every kept
point, the dropped points per column family, and three deliberately wrong formulas outside the bounds."""
import numpy as np
import pytest

from tests import batchnorm_ref as br

B_AXIS = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
S_AXIS = (1, 3, 9, 16, 17, 33)
H_ALL = len(br.FAMILIES)


def _mp_forward(t, gamma, beta, eps):
  import mpmath as mp
  S, B, H = t.shape
  res = {k: np.zeros((B, H)) for k in ("xhat", "out")}
  stats = {k: np.zeros(H) for k in ("mean", "var", "inv")}
  for c in range(H):
    v = [mp.fsum(mp.mpf(float(t[s, b, c])) for s in range(S)) for b in range(B)]
    mean = mp.fsum(v) / B
    var = mp.fsum((x - mean) ** 2 for x in v) / B
    inv = 1 / mp.sqrt(var + mp.mpf(float(np.float32(eps))))
    stats["mean"][c], stats["var"][c], stats["inv"][c] = float(mean), float(var), float(inv)
    for b in range(B):
      xh = (v[b] - mean) * inv
      y = mp.mpf(float(gamma[c])) * xh + mp.mpf(float(beta[c]))
      res["xhat"][b, c], res["out"][b, c] = float(xh), float(max(y, 0))
  res.update(stats)
  return res


def _mp_backward(dt, out, xhat, inv, gamma):
  import mpmath as mp
  S, B, H = dt.shape
  dpre, dg, db = np.zeros((B, H)), np.zeros(H), np.zeros(H)
  for c in range(H):
    dy = [mp.fsum(mp.mpf(float(dt[s, b, c])) for s in range(S)) if out[b, c] > 0 else mp.mpf(0) for b in range(B)]
    xh = [mp.mpf(float(xhat[b, c])) for b in range(B)]
    s1, s2 = mp.fsum(dy), mp.fsum(a * b for a, b in zip(dy, xh))
    gi = mp.mpf(float(gamma[c])) * mp.mpf(float(inv[c]))
    dg[c], db[c] = float(s2), float(s1)
    for b in range(B):
      dpre[b, c] = float(gi * (dy[b] - (s1 + xh[b] * s2) / B))
  return dict(dpre=dpre, dgamma=dg, dbeta=db)


@pytest.mark.parametrize("B,S", [(1, 1), (2, 3), (65, 3)])
def test_reference_against_mpmath(B, S):
  """the float64 reference is 2^-29 finer than the float32 bounds; it is held to 2^-20 of each bound, on every point with a finite bound"""
  import mpmath as mp
  mp.mp.dps = 120
  t, gamma, beta, names = br.make_columns(B, H_ALL, S, seed=11)
  r = br.forward(t, gamma, beta)
  m = _mp_forward(t, gamma, beta, 1e-3)
  for k in ("mean", "var", "inv", "xhat", "out"):
    ok = np.isfinite(r["E_" + k])
    assert ok.any()
    assert br.worst(r[k], m[k], r["E_" + k] * 2.0 ** -20, ok) <= 1.0, k
  rp = br.replay_forward(t, gamma, beta)
  dt = br.make_dout(B, names, S, seed=12)
  b = br.backward(dt, rp["out"], rp["xhat"], rp["inv_std"], gamma, beta)
  mb = _mp_backward(dt, rp["out"], rp["xhat"], rp["inv_std"], gamma)
  for k in ("dpre", "dgamma", "dbeta"):
    ok = np.isfinite(b["E_" + k])
    assert br.worst(b[k], mb[k], b["E_" + k] * 2.0 ** -20, ok) <= 1.0, k


@pytest.mark.parametrize("leak", [0.0, 0.2])
def test_composition_against_torch_autograd(leak):
  """backward(forward(.)) in float64 == torch's float64 autograd of the same composition, on the columns whose every |y| clears its bound"""
  import torch
  B, S = 65, 3
  t, gamma, beta, names = br.make_columns(B, H_ALL, S, seed=21)
  dt = br.make_dout(B, names, S, seed=22)
  r = br.forward(t, gamma, beta, leak=leak)
  b = br.backward(dt, r["out"], r["xhat"], r["inv"], gamma, beta, leak=leak)
  v = torch.tensor(r["v"], dtype=torch.float64, requires_grad=True)
  g = torch.tensor(gamma.astype(np.float64), requires_grad=True)
  be = torch.tensor(beta.astype(np.float64), requires_grad=True)
  mean = v.mean(0)
  var = ((v - mean) ** 2).mean(0)
  y = g * (v - mean) / torch.sqrt(var + float(np.float32(1e-3))) + be
  h = torch.clamp(y, min=0) + float(np.float32(leak)) * torch.clamp(y, max=0)
  (h * torch.tensor(dt.astype(np.float64).sum(0))).sum().backward()
  away = (np.abs(r["y"]) > r["E_y"]).all(0) & r["asserted"]
  assert away.sum() >= H_ALL - 6    # (the constant columns sit on the kink: y = beta = 0 exactly in three of them)
  for got, ref, scale in ((b["dpre"], v.grad.numpy(), b["S_dpre"]), (b["dgamma"], g.grad.numpy(), b["S_dgamma"]), (b["dbeta"], be.grad.numpy(), b["S_dbeta"])):
    err = np.abs(got - ref)[..., away]
    assert np.all(err <= 1e-9 * np.maximum(np.broadcast_to(scale, got.shape)[..., away], 1e-300)), float(err.max())


def _replay_case(B, S, wide=False, training=True, leak=0.0, p=0.0, seed=0):
  t, gamma, beta, names = br.make_columns(B, H_ALL, S, seed=31 + seed, shift=seed)
  rng = np.random.default_rng(41 + seed)
  mm, mv = rng.standard_normal(H_ALL).astype(np.float32), np.abs(rng.standard_normal(H_ALL)).astype(np.float32)
  mult = None if p == 0.0 else np.where(rng.random((B, H_ALL)) >= p, br.drop_scale(p), np.float32(0)).astype(np.float32)
  kw = dict(moving_mean=mm, moving_var=mv, training=training, leak=leak, mult=mult)
  r = br.forward(t, gamma, beta, **kw)
  rp = br.replay_forward(t, gamma, beta, wide=wide, **kw)
  dt = br.make_dout(B, names, S, seed=51 + seed)
  b = br.backward(dt, rp["out"], rp["xhat"], rp["inv_std"], gamma, beta, training=training, leak=leak, p=p)
  bp = br.replay_backward(dt, rp["out"], rp["xhat"], rp["inv_std"], gamma, training=training, leak=leak, p=p, wide=wide)
  return t, gamma, beta, names, r, rp, b, bp


@pytest.mark.parametrize("B", B_AXIS)
def test_replay_inside_bounds_and_dropped_counts(B):
  """the float32 replay of the kernels' lines stays inside every bound at every kept point, over the GPU test's batch sizes and slab counts;
  no column family loses more than a tenth of its points (the 1e18 family: asserted whole below B = 19, not at all above)"""
  total = {}
  for i, S in enumerate(S_AXIS):
    t, gamma, beta, names, r, rp, b, bp = _replay_case(B, S, seed=i)
    fk, bk = br.fwd_keep(r, gamma, beta), br.bwd_keep(b)
    pairs = [("mean", rp["batch_mean"]), ("var", rp["batch_var"]), ("inv", rp["inv_std"]), ("xhat", rp["xhat"]), ("out", rp["out"])]
    for k, got in pairs:
      assert br.worst(got, r[k], r["E_" + k], fk[k]) <= 1.0, (k, B, S)
    for k in ("dpre", "dgamma", "dbeta"):
      assert br.worst(bp[k], b[k], b["E_" + k], bk[k]) <= 1.0, (k, B, S)
    for k, keep in list(fk.items()) + list(bk.items()):
      for fam, (d, n) in br.dropped_by_family(names, keep).items():
        if B == 1 and k in fk and k != "mean":
          continue      # (one row: d = 0 and var = 0 exactly, which a bound in term sizes does not know -- asserted exactly below)
        if fam == "huge18" and k in fk:
          assert d == (0 if B < 19 else n), (k, fam, B, S, d, n)
        else:
          d0, n0 = total.get((k, fam), (0, 0))
          total[(k, fam)] = (d0 + d, n0 + n)
    for c, n in enumerate(names):     # the constant columns: exact
      if n in br.CONSTANT:
        assert np.all(rp["batch_var"][c] == 0) and np.all(rp["xhat"][:, c] == 0) and np.all(rp["out"][:, c] == max(beta[c], 0))
  if B == 1:
    assert np.all(rp["batch_var"] == 0) and np.all(rp["xhat"] == 0)
  for (k, fam), (d, n) in total.items():   # over the slab counts of this batch size
    assert 10 * d <= n, (k, fam, B, d, n)


@pytest.mark.parametrize("kw", [dict(wide=True, B=37, S=15), dict(wide=True, B=128, S=250), dict(training=False, B=129, S=3),
                                dict(leak=0.2, B=257, S=9), dict(p=0.5, B=65, S=3), dict(p=0.1, B=1025, S=1)])
def test_replay_inside_bounds_other_modes(kw):
  t, gamma, beta, names, r, rp, b, bp = _replay_case(**kw)
  fk, bk = br.fwd_keep(r, gamma, beta), br.bwd_keep(b)
  for k, got in (("inv", rp["inv_std"]), ("xhat", rp["xhat"]), ("out", rp["out"])):
    assert br.worst(got, r[k], r["E_" + k], fk[k]) <= 1.0, k
  for k in ("dpre", "dgamma", "dbeta"):
    assert br.worst(bp[k], b[k], b["E_" + k], bk[k]) <= 1.0, k


def test_wide_and_plain_replays_agree_bit_for_bit_up_to_16_slabs():
  """one chain per slab up to 16 slabs: the wide order is the plain order there (the source's claim is for the sums a reduce launch left)"""
  t, gamma, beta, names = br.make_columns(37, H_ALL, 1, seed=3)
  a, w = br.replay_forward(t, gamma, beta), br.replay_forward(t, gamma, beta, wide=True)
  for k in a:
    assert np.array_equal(a[k], w[k], equal_nan=True), k


def test_wrong_formulas_are_rejected():
  """a variance divisor of B - 1, the backward without its s1 term, evaluation mode on the batch variance: each is outside the bounds at
  kept points of the ordinary columns"""
  B, S = 65, 3
  t, gamma, beta, names = br.make_columns(B, H_ALL, S, seed=61)
  normal = np.array([n in ("normal", "normal_b", "beta_pos", "beta_neg", "spread37") for n in names])
  r = br.forward(t, gamma, beta)
  fk = br.fwd_keep(r, gamma, beta)
  good, bad = br.replay_forward(t, gamma, beta), br.replay_forward(t, gamma, beta, variance_divisor=B - 1)
  assert br.worst(good["xhat"], r["xhat"], r["E_xhat"], fk["xhat"]) <= 1.0
  for k, got in (("var", bad["batch_var"]), ("inv", bad["inv_std"]), ("xhat", bad["xhat"])):
    assert br.worst(got[..., normal], r[k][..., normal], r["E_" + k][..., normal], fk[k][..., normal]) > 100.0, k
  dt = br.make_dout(B, names, S, seed=62)
  b = br.backward(dt, good["out"], good["xhat"], good["inv_std"], gamma, beta)
  bk = br.bwd_keep(b)
  ok, wrong = (br.replay_backward(dt, good["out"], good["xhat"], good["inv_std"], gamma, drop_s1=d) for d in (False, True))
  assert br.worst(ok["dpre"], b["dpre"], b["E_dpre"], bk["dpre"]) <= 1.0
  assert br.worst(wrong["dpre"][:, normal], b["dpre"][:, normal], b["E_dpre"][:, normal], bk["dpre"][:, normal]) > 100.0
  mm, mv = np.zeros(H_ALL, np.float32), np.full(H_ALL, 4.0, np.float32)
  re = br.forward(t, gamma, beta, moving_mean=mm, moving_var=mv, training=False)
  ek = br.fwd_keep(re, gamma, beta)
  right = br.replay_forward(t, gamma, beta, moving_mean=mm, moving_var=mv, training=False)
  wrong = br.replay_forward(t, gamma, beta, moving_mean=mm, moving_var=mv, training=False, eval_batch_var=True)
  assert br.worst(right["xhat"], re["xhat"], re["E_xhat"], ek["xhat"]) <= 1.0
  assert br.worst(wrong["xhat"][:, normal], re["xhat"][:, normal], re["E_xhat"][:, normal], ek["xhat"][:, normal]) > 100.0


def test_moving_update_is_not_fused():
  """two products and a sum: a fused form differs in the last bit on some of a few thousand random operands"""
  rng = np.random.default_rng(5)
  mm, bm = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
  got = br.moving_update(mm, bm, 0.99)
  m = np.float32(0.99)
  fused = (mm.astype(np.float64) * np.float64(m) + (bm * (np.float32(1) - m)).astype(np.float64)).astype(np.float32)
  assert got.dtype == np.float32 and np.array_equal(got, mm * m + bm * (np.float32(1) - m)) and not np.array_equal(got, fused)
