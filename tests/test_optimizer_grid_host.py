"""tests/optimizer_ref.py on the host: the float64 reference against mpmath at 120 digits and against torch.optim in float64, the float32
replay of the kernels' lines inside every bound at every kept point of the whole grid (all four norm paths), the share of dropped points per
value family, and the mutations the grid must tell from the shipped rules.  CPU only."""
import mpmath as mp
import numpy as np
import pytest
import torch

from tests import optimizer_ref as R

mp.mp.dps = 120


@pytest.fixture(scope="module")
def grid():
  """every launch of the grid with its reference, made once"""
  out = []
  for form in R.FORMS:
    for k, carrier in enumerate(R.CARRIERS):
      L = R.make_launch(form, k, carrier)
      out.append((L, R.reference_launch(L)))
  return out


def test_grid_covers_every_axis(grid):
  for form in R.FORMS:
    Ls = [L for L, _ in grid if L["form"] == form]
    assert {L["lr"] for L in Ls} == set(R.LRS) and {L["clipnorm"] for L in Ls} == set(R.CLIPS) and {L["t"] for L in Ls} >= set(R.TS)
    assert {L["t0"] for L in Ls} == {0, 3} and any(L["step"] < L["t0"] for L in Ls) and {L["grad_scale"] for L in Ls} == {1.0, 0.5}
    assert {L["eps"] for L in Ls} == {float(R.f32(e)) for e in R.EPSS} or form.startswith("sgd")
    if form in ("adam", "adamax"):
      assert {L["b1"] for L in Ls} == {float(R.f32(b)) for b in R.B1S} and {L["b2"] for L in Ls} == {float(R.f32(b)) for b in R.B2S}
    if form.startswith("rmsprop"):
      assert {L["b1"] for L in Ls} == {float(R.f32(b)) for b in R.B2S}
    if form in ("sgd_momentum", "sgd_nesterov", "rmsprop_momentum"):
      assert {L["mu"] for L in Ls} == {float(R.f32(b)) for b in R.MUS}
    assert {(L["carrier"], L["use_sq"]) for L in Ls} == {(c[0], c[1]) for c in R.CARRIERS} and any(L["tied"] for L in Ls)
    assert {tn["path"] for L in Ls for tn in L["tensors"]} == {"partials", "shard", "slots", "own"}
    assert {len(tn["sq"]) for L in Ls for tn in L["tensors"] if tn["sq"] is not None} == set(R.SQ_COUNTS) - {0}
    fams = {tn["gf"] for L in Ls for tn in L["tensors"]}
    assert fams == set(R.G_FAMILIES) - (set() if form == "adagrad" else {"ones"})
    # a slice boundary inside a chunk, and a rank that owns no part of some tensor
    sh = [L for L in Ls if L["carrier"] == "shard" and L["world"] > 1]
    assert any(c % 4096 for L in sh for c in L["cuts"][1:-1])
    assert any(all(not (L["cuts"][r] < tn["lo"] + len(tn["gpad"]) and L["cuts"][r + 1] > tn["lo"]) for r in [L["world"] - 1]) for L in sh for tn in L["tensors"])


# ---- mpmath --------------------------------------------------------------------------------------------------------------------------
def _mp_update(form, b1, b2, eps, mu, lr_t, ge, m, v, p):
  b1, b2, eps, mu, ge, m, v, p = (mp.mpf(float(x)) for x in (b1, b2, eps, mu, ge, m, v, p))
  if form == "adam":
    m2, v2 = b1 * m + (1 - b1) * ge, b2 * v + (1 - b2) * ge * ge
    return m2, v2, -lr_t * m2 / (mp.sqrt(v2) + eps)
  if form == "sgd":
    return None, None, -lr_t * ge
  if form == "sgd_momentum":
    m2 = mu * m - lr_t * ge
    return m2, None, m2
  if form == "sgd_nesterov":
    m2 = mu * m - lr_t * ge
    return m2, None, mu * m2 - lr_t * ge
  if form == "rmsprop":
    v2 = b1 * v + (1 - b1) * ge * ge
    return None, v2, -lr_t * ge / (mp.sqrt(v2) + eps)
  if form == "rmsprop_momentum":
    v2 = b1 * v + (1 - b1) * ge * ge
    m2 = mu * m + lr_t * ge / mp.sqrt(v2 + eps)
    return m2, v2, -m2
  if form == "adagrad":
    v2 = v + ge * ge
    return None, v2, -lr_t * ge / (mp.sqrt(v2) + eps)
  m2, v2 = b1 * m + (1 - b1) * ge, max(b2 * v, abs(ge))
  return m2, v2, -lr_t * m2 / (v2 + eps)


def _mp_lr_t(form, b1, b2, lr, t):
  lr, b1, b2 = mp.mpf(float(lr)), mp.mpf(float(b1)), mp.mpf(float(b2))
  if form == "adam":
    return lr * mp.sqrt(1 - b2 ** t) / (1 - b1 ** t)
  return lr / (1 - b1 ** t) if form == "adamax" else lr


@pytest.mark.parametrize("form", R.FORMS)
def test_reference_matches_mpmath(grid, form):
  """lr_t, every norm and clip factor, and m, v and the move at a stride of elements: inside 2^-20 of the bound."""
  worst = 0.0
  for L, ref in [x for x in grid if x[0]["form"] == form][::3]:
    lr_t = _mp_lr_t(form, L["b1"], L["b2"], float(R.f32(L["lr"])), L["t"])
    assert abs(lr_t - mp.mpf(float(ref["lr_t"].v))) <= mp.mpf(float(ref["lr_t"].e)) * 2.0 ** -20
    for tn, r in zip(L["tensors"], ref["tensors"]):
      src = tn["sq"] if tn["sq"] is not None else tn["g"]
      s = mp.fsum(mp.mpf(float(x)) ** (1 if tn["sq"] is not None else 2) for x in src[: 4200]) if len(src) <= 4200 else None
      if s is not None:
        norm = mp.sqrt(s * mp.mpf(tn["tied_inv"])) * mp.mpf(L["grad_scale"])
        assert abs(norm - mp.mpf(float(r["norm"].v))) <= mp.mpf(float(r["norm"].e)) * 2.0 ** -20, (tn["size"], tn["gf"])
        clip = mp.mpf(L["grad_scale"]) * (mp.mpf(L["clipnorm"]) / norm if L["clipnorm"] > 0 and norm > L["clipnorm"] else 1)
        # (where the float64 norm and the exact one fall on different sides of clipnorm the factors differ by the norms' difference)
        assert abs(clip - mp.mpf(float(r["clip"].v))) <= mp.mpf(float(r["clip"].e)) * 2.0 ** -20 + abs(norm - mp.mpf(float(r["norm"].v))) * L["grad_scale"] / max(L["clipnorm"], 1.0)
      clip = mp.mpf(float(r["clip"].v))
      for i in range(0, tn["size"], max(1, tn["size"] // 37)):
        ge = mp.mpf(float(tn["g"][i])) * clip
        got = _mp_update(form, L["b1"], L["b2"], L["eps"], L["mu"], lr_t, ge, tn["m"][i], tn["v"][i], tn["p"][i])
        for key, val in zip(("m", "v", "d"), got):
          if val is None:
            continue
          err, bound = abs(val - mp.mpf(float(r[key].v[i]))), float(r[key].e[i])
          assert err <= mp.mpf(bound) * 2.0 ** -20, (key, tn["size"], tn["gf"], i, float(err), bound)
          if bound > 0:
            worst = max(worst, float(err) / bound)
  print(f"{form}: worst |reference - mpmath| / bound {worst:.2e}")


# ---- torch.optim ---------------------------------------------------------------------------------------------------------------------
def _torch_move(form, L, g, m, v, p):
  """one step of torch's float64 optimiser from the given state; the state is mapped as tests/test_optimizers_host.py describes"""
  w = torch.tensor(p.copy(), dtype=torch.float64, requires_grad=True)
  w.grad = torch.tensor(g.copy(), dtype=torch.float64)
  lr, t = float(R.f32(L["lr"])), L["t"]
  T = lambda a: torch.tensor(np.array(a, np.float64))
  if form == "adam":
    o = torch.optim.Adam([w], lr=lr, betas=(L["b1"], L["b2"]), eps=L["eps"] / np.sqrt(1 - L["b2"] ** t))   # (Keras's epsilon-hat form)
    o.state[w] = dict(step=torch.tensor(float(t - 1)), exp_avg=T(m), exp_avg_sq=T(v))
  elif form == "sgd":
    o = torch.optim.SGD([w], lr=lr)
  elif form in ("sgd_momentum", "sgd_nesterov"):
    o = torch.optim.SGD([w], lr=lr, momentum=L["mu"], nesterov=form == "sgd_nesterov")
    o.state[w] = dict(momentum_buffer=T(-m / lr))
  elif form == "rmsprop":
    o = torch.optim.RMSprop([w], lr=lr, alpha=L["b1"], eps=L["eps"])
    o.state[w] = dict(step=torch.tensor(0.0), square_avg=T(v))
  else:
    o = torch.optim.Adagrad([w], lr=lr, eps=L["eps"])
    o.state[w] = dict(step=torch.tensor(0.0), sum=T(v))
  o.step()
  return w.detach().numpy() - p


@pytest.mark.parametrize("form", ["adam", "sgd", "sgd_momentum", "sgd_nesterov", "rmsprop", "adagrad"])
def test_reference_matches_torch(grid, form):
  """The move of every tensor of the grid's launches with lr > 0 against torch.optim in float64 from the same state, fed the reference's
  clipped gradient: to 1e-12 of the move's term size (and of the weight, whose float64 storage torch's move goes through)."""
  n = 0
  for L, ref in [x for x in grid if x[0]["form"] == form and x[0]["lr"] > 0 and x[0]["t"] < 2 ** 24]:
    for tn, r in zip(L["tensors"], ref["tensors"]):
      ge = tn["g"] * float(r["clip"].v)
      move = _torch_move(form, L, ge, tn["m"], tn["v"], tn["p"])
      tol = 1e-12 * (r["d"].s + np.abs(tn["p"])) + 1e-300
      assert np.all(np.abs(move - r["d"].v) <= tol), (L["k"], tn["size"], tn["gf"], float(np.max(np.abs(move - r["d"].v) / tol)))
      n += tn["size"]
  assert n > 100000


# ---- the replay ----------------------------------------------------------------------------------------------------------------------
def test_replay_inside_every_bound_and_dropped_share(grid):
  worst, share = {}, {}
  for L, ref in grid:
    w, s = R.ratios(ref, R.replay_launch(L), L)
    for key, val in w.items():
      k2 = (L["form"], key)
      worst[k2] = max(worst.get(k2, 0.0), val)
      assert val <= 1.0, (L["form"], L["k"], L["carrier"], key, val)
    for key, (a, b) in s.items():
      c = share.setdefault((L["form"],) + key, [0, 0])
      c[0] += a
      c[1] += b
  for form in R.FORMS:
    print(form, {k[1]: round(v, 3) for k, v in worst.items() if k[0] == form})
  for key, (a, b) in share.items():
    assert a >= 0.9 * b, (key, a, b)   # at most a tenth of any family dropped
  assert all(ref["lr_t_keep"] for _, ref in grid)


@pytest.mark.parametrize("mutation", list(R.MUTATIONS))
def test_grid_tells_the_mutation_apart(grid, mutation):
  """each wrong rule is more than 100 bounds out at some kept point of the grid"""
  worst = 0.0
  for L, ref in grid:
    if L["form"] not in R.MUTATIONS[mutation] or (mutation == "no_tied_inv" and not L["tied"]):
      continue
    w, _ = R.ratios(ref, R.replay_launch(L, mutation), L)
    worst = max(worst, max(w.values()))
    if worst > 100:
      break
  assert worst > 100, (mutation, worst)
