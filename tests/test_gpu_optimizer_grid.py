"""The optimiser's carriers by themselves (Engine k_opt_carrier: the optimiser launch, the background sweep, the sharded chain, the 512-thread
body; norms from the chunk partials, from sum-of-squares slots and from a tensor's own sweep) against the float64 reference and the bounds of
tests/optimizer_ref.py, element by element on its edge grid -- and the exact assertions: zero padding, guard bands, untouched slots, lr = 0,
g = m = 0, the same bits whichever carrier runs the element update, the strict clipnorm comparison, the overflowing norm, the refusals
(DESIGN.md 4w).  `pytest -s` prints the worst error / bound per form, component and carrier."""
import numpy as np
import pytest

from tests import optimizer_ref as R

pytestmark = pytest.mark.gpu
LR_PROPORTIONAL = ("adam", "sgd", "rmsprop", "adagrad", "adamax")   # the forms whose move is lr_t times something


@pytest.fixture(scope="module")
def K():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import k_opt_carrier
  return k_opt_carrier


def _run(K, L, **over):
  T = L["tensors"]
  kw = dict(carrier=L["carrier"], wgs=L["wgs"], world=L["world"], use_sq=L["use_sq"], sq=[t["sq"] for t in T], lr=L["lr"], clipnorm=L["clipnorm"],
            grad_scale=L["grad_scale"], t0=L["t0"], tied=L["tied"], tied_inv=L["tied_inv"])
  kw.update(over)
  return K(L["rule"], [t["g"] * 0 + t["p"] for t in T], [t["g"] for t in T], [t["m"] for t in T], [t["v"] for t in T], L["step"], **kw, **L["hp"])


def _view(o, L):
  """the device's result per tensor, as optimizer_ref.ratios reads it"""
  out = dict(lr_t=o["lr_t"], tensors=[])
  for i, t in enumerate(L["tensors"]):
    a, n = int(o["offsets"][i]), t["size"]
    out["tensors"].append(dict(norm=o["norms"][i], m=o["m"][a:a + n], v=o["v"][a:a + n], d=o["params"][a:a + n].astype(np.float64) - t["p"],
                               p=o["params"][a:a + n]))
  return out


def _exact(o, L, where):
  """what holds bit for bit after every launch"""
  assert o["guards_ok"], where
  assert o["unused_ok"], where
  pad = np.ones(L["total"], bool)
  for a, n in zip(o["offsets"], o["sizes"]):
    pad[int(a):int(a + n)] = False
  used = ["params"] + (["m"] if L["form"] in R.USES_M else []) + (["v"] if L["form"] in R.USES_V else [])
  for key in used:
    assert np.all(o[key][pad] == 0), (where, key, "padding", o[key][pad][o[key][pad] != 0][:4])
  view = _view(o, L)
  bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
  for t, d in zip(L["tensors"], view["tensors"]):
    p32 = t["p"].astype(np.float32)
    if L["lr"] == 0:   # (a momentum accumulator keeps moving the weight at lr = 0, as in Keras: there the elements with m = 0 stand still)
      rest = np.ones(t["size"], bool) if L["form"] in LR_PROPORTIONAL else t["m"] == 0
      assert np.array_equal(bits(d["p"][rest]), bits(p32[rest])), (where, "lr = 0 moved a weight", t["size"])
    still = (t["g"] == 0) & ((t["m"] == 0) if L["form"] in R.USES_M else True)
    assert np.array_equal(bits(d["p"][still]), bits(p32[still])), (where, "g = m = 0 moved a weight", t["size"])
  if L["lr"] == 0:   # ... while the slots still move
    for key in used[1:]:
      assert any(not np.array_equal(d[key], t[key].astype(np.float32)) for t, d in zip(L["tensors"], view["tensors"])), (where, key)
  return view


@pytest.mark.parametrize("form", R.FORMS)
def test_every_carrier_inside_the_bounds(K, form):
  """Every launch of the form's grid: every kept point of lr_t, the norms, m, v and the move inside its bound (a NaN at a kept point
  fails), at most a tenth of any value family dropped, and the exact assertions."""
  table, share = {}, {}
  for k, carrier in enumerate(R.CARRIERS):
    L = R.make_launch(form, k, carrier)
    ref = R.reference_launch(L)
    where = (form, k, carrier)
    view = _exact(_run(K, L), L, where)
    worst, s = R.ratios(ref, view, L)
    for key, val in worst.items():
      row = table.setdefault((carrier[0], "sq" if carrier[1] else "partials"), {})
      row[key] = max(row.get(key, 0.0), val)
    for key, (a, b) in s.items():
      c = share.setdefault(key, [0, 0])
      c[0] += a
      c[1] += b
    for key, val in worst.items():
      assert val <= 1.0, (where, key, val)
  for key, row in table.items():
    print(form, key, {c: round(v, 3) for c, v in row.items()})
  for key, (a, b) in share.items():
    assert a >= 0.9 * b, (form, key, a, b)


@pytest.mark.parametrize("form", R.FORMS)
def test_carriers_give_the_same_bits(K, form):
  """The same tensors through every carrier.  Carriers that take the norm from the same tree (launch, sweep at every wgs, 512-thread body;
  partials and use_sq apart) agree bit for bit everywhere; the sharded chain, whose partials are summed slice by slice, on every tensor
  whose factor is exactly grad_scale."""
  k = 1   # (clipnorm 5 in force, lr > 0, a tied pair)
  for use_sq in (0, 1):
    L = R.make_launch(form, k, ("launch", use_sq, 0, 0))
    assert L["clipnorm"] > 0 and L["lr"] > 0 and L["tied"]
    base = _run(K, L)
    others = [("sweep", w, 0) for w in (1, 2, 3, L["n_chunks"])] + [("body512", 0, 0)] + ([] if use_sq else [("shard", 2, w) for w in (1, 2, 3, 4)])
    for name, wgs, world in others:
      o = _run(K, L, carrier=name, wgs=wgs, world=world)
      assert o["guards_ok"] and o["unused_ok"] and o["lr_t"] == base["lr_t"]
      for i, t in enumerate(L["tensors"]):
        a, n = int(o["offsets"][i]), int(o["pads"][i])
        if name == "shard" and not base["norms"][i] * (1 + 1e-5) < L["clipnorm"]:
          continue
        for key in ("params", "m", "v"):
          assert np.array_equal(o[key][a:a + n].view(np.uint32), base[key][a:a + n].view(np.uint32)), (form, use_sq, name, wgs, world, t["size"], t["gf"], key)


@pytest.mark.parametrize("carrier", [("launch", 0, 0, 0), ("launch", 1, 0, 0), ("sweep", 1, 2, 0), ("shard", 0, 2, 3), ("body512", 0, 0, 0)])
def test_norm_exactly_clipnorm_is_not_clipped(K, carrier):
  """The comparison is strict: a tensor whose float32 norm IS clipnorm (squares and sums exact) comes out with the bits of the launch that
  does not clip at all; its neighbour's norm is a float or two above (what clipping does to
  it is held by the bounds of test_every_carrier_inside_the_bounds)."""
  for form, k in (("adam", 1), ("rmsprop_momentum", 9), ("adamax", 10)):
    L = R.make_launch(form, k, carrier)
    assert L["clipnorm"] == R.CLIP_FOR_FAMILIES and L["lr"] > 0
    on, off = _run(K, L), _run(K, L, clipnorm=0.0)
    seen = 0
    for i, t in enumerate(L["tensors"]):
      a, n = int(on["offsets"][i]), int(on["pads"][i])
      if t["gf"] == "norm_is_clip":
        seen += 1
        assert on["norms"][i] == np.float32(L["clipnorm"]), (form, t["size"], on["norms"][i])
        for key in ("params", "m", "v"):
          assert np.array_equal(on[key][a:a + n].view(np.uint32), off[key][a:a + n].view(np.uint32)), (form, carrier, t["size"], key)
      if t["gf"] == "norm_above_clip":
        seen += 1
        assert on["norms"][i] > np.float32(L["clipnorm"]) and on["norms"][i] <= np.float32(L["clipnorm"]) * np.float32(1 + 2.0 ** -20)
    assert seen >= 2


def test_overflowing_sum_of_squares_gives_factor_zero(K):
  """Sum of squares beyond float32: norm inf, factor clipnorm / inf = 0, as float32 tf.clip_by_norm -- m and v decay, nothing else."""
  rng = np.random.default_rng(0)
  n = 4096 + 64
  g, m, v, p = np.full(n, 1e19), R.f32(1e-3 * rng.normal(size=n)), R.f32(rng.uniform(0, 1, size=n)), R.f32(rng.normal(size=n))
  for carrier, use_sq in (("launch", False), ("launch", True), ("sweep", False), ("body512", True)):
    o = K("adam", [p], [g], [m], [v], 7, carrier=carrier, wgs=2, use_sq=use_sq, sq=[None], lr=1e-3, clipnorm=5.0)
    assert o["guards_ok"] and np.isposinf(o["norms"][0])
    assert np.array_equal(o["m"][:n], R._fma32(np.float32(0.9), m, 0.0)) and np.array_equal(o["v"][:n], R._fma32(np.float32(0.999), v, 0.0))
    assert np.all(np.isfinite(o["params"])) and np.all(o["params"][n:] == 0)


REFUSED = [("adam", dict(epsilon=0.0)), ("rmsprop", dict(epsilon=0.0)), ("rmsprop", dict(momentum=0.9, epsilon=0.0)), ("adagrad", dict(epsilon=0.0)),
           ("adagrad", dict(initial_accumulator_value=0.0, epsilon=0.0)), ("adamax", dict(epsilon=0.0)), ("adam", dict(epsilon=1e-39)),
           ("adamax", dict(epsilon=-1e-7))]


@pytest.mark.parametrize("rule,hp", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_epsilon_that_would_poison_the_padding_is_refused(K, rule, hp):
  """epsilon = 0 (or a denormal: its reciprocal is inf) would turn the zero padding into 0 * inf = NaN: refused by optimizers.canonical, and by
  the library itself (SMX_ERR_INVALID from opt_resolve, before any device work) when the vector reaches it another way."""
  from sisua_amd import optimizers
  from sisua_amd._hip import SmxError
  one = [np.ones(5)]
  with pytest.raises(ValueError, match="epsilon"):
    K(rule, one, one, one, one, 1, **hp)
  defaults = dict(optimizers.RULES[rule][1])
  raw = np.array([float({**defaults, **hp}[key]) for key, _ in optimizers.RULES[rule][1]], np.float32)
  with pytest.raises(SmxError, match="epsilon") as e:
    K(rule, one, one, one, one, 1, hp_raw=raw)
  assert e.value.code == -1


@pytest.mark.parametrize("rule,hp", [("adam", {}), ("rmsprop", {}), ("rmsprop", dict(momentum=0.9)), ("adagrad", {}), ("adamax", {})])
def test_padding_stays_zero_at_the_smallest_accepted_epsilon(K, rule, hp):
  """epsilon = 2^-126, the smallest the library takes, zero slots: the padding of the weights and of both slots stays exactly 0 on every
  carrier, and a real element with g = m = v = 0 stays where it was (0 / eps = 0, as Keras has it)."""
  tiny = float(np.finfo(np.float32).tiny)
  sizes = (1, 65, 4097)
  z = [np.zeros(n) for n in sizes]
  g = [np.concatenate([[0.0], np.ones(n - 1)]) for n in sizes]
  p = [np.full(n, 0.5) for n in sizes]
  for carrier, world in (("launch", 0), ("sweep", 0), ("shard", 3), ("body512", 0)):
    o = K(rule, p, g, z, z, 1, carrier=carrier, wgs=2, world=world, lr=1e-3, clipnorm=0.0, epsilon=tiny, **hp)
    assert o["guards_ok"] and o["unused_ok"]
    pad = np.ones(o["params"].size, bool)
    for a, n in zip(o["offsets"], o["sizes"]):
      pad[int(a):int(a + n)] = False
      assert o["params"][int(a)] == np.float32(0.5)
    for key in ("params", "m", "v"):
      x = o[key][pad]
      assert np.all((x == 0) | (x.view(np.uint32) == 0xFFFFFFFF)), (rule, carrier, key)   # (0xFF words: a slot the rule does not use)
    assert np.all(np.isfinite(o["params"]))


def test_sqrt_of_a_denormal_second_moment(K):
  """What v_sqrt_f32 does at a denormal argument, seen through Adam's move at epsilon = 1e-30: v' = b2 1e-40 is denormal; the move is
  -lr_t m' / (sqrt(v') + eps) with sqrt(v') ~ 1e-20, or -lr_t m' / eps if the instruction reads the denormal as zero.  Either is inside
  the grid's bounds (eps >= 1e-7 there: the floor of optimizer_ref.fsqrt).  The MI355X reads it as ZERO (tools/ulp_probe.hip: every argument
  below 2^-126 gives 0, 2^-126 itself 1.0842e-19); that is what DESIGN.md 4w states, and this test keeps the statement true."""
  n = 64
  m, v, p, g = np.full(n, 1e-3), np.full(n, 1e-40), np.zeros(n), np.zeros(n)
  o = K("adam", [p], [g], [m], [v], 1000, lr=1e-3, clipnorm=0.0, epsilon=1e-30)
  b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
  lr_t = 1e-3 * np.sqrt(1 - b2 ** 1000) / (1 - b1 ** 1000)
  v2 = float(o["v"][0])
  assert 0 < v2 < 2.0 ** -126 and np.isclose(v2, b2 * 1e-40, rtol=1e-4)   # (the fma keeps the denormal)
  kept_, flushed = -lr_t * b1 * 1e-3 / (np.sqrt(v2) + 1e-30), -lr_t * b1 * 1e-3 / 1e-30
  got = float(o["params"][0])
  print(f"v_sqrt_f32 at {v2:.3e}: move {got:.6e}; denormal kept {kept_:.6e}, read as zero {flushed:.6e}")
  assert np.isclose(got, flushed, rtol=1e-5) and not np.isclose(got, kept_, rtol=1e-2)
