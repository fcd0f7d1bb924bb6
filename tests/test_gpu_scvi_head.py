"""The scVI gene head's three launch forms (smx_scvi.hip) held to the float64 reference of tests/scvi_head_ref.py, element by element and inside
bounds derived from the kernels' own lines (that module's docstring has the table), at the smallest and the largest width of every template
instance.  No tolerance here was chosen after looking at a kernel's output.  Every test prints the worst error / bound per output and where it
occurred; DESIGN.md 4sa records them as read on an MI355X.

THE PIN.  The rate cannot be set, but it can be pinned from the inputs: rho by raw_0 of the whole row; l exactly by a library head of one
column, Wl = (1, 0), hl[b] = l_b, bl = (0, s) and the injected noise 0: the product by 1 and the sums with 0 are exact, so mu_l = l = l_b in every
row of a launch (a head with Wl = 0 could only give every row of a launch the same l).  One further launch per Kl in {1, 63, 65, 257} has a
random head and non-zero noise, for the dot-product loop's tails; its l carries the product's bound into el.

THE LAUNCHES (scvi_head_ref.launches): B = 8 rows up to 4128 padded genes, 4 above; rows moderate, spike, flat, five straddle rows, dispersion and
gate (SCVI_AXES x CYCLE), the library edges l in {-3, 0, 5, 11} under clip_library = 1e3 and {5.5, 6, 7} under 6.

INSTANCES: the width table below restates the launchers' thresholds on Gp; tests/test_scvi_head_host.py holds it to the source's.
  train   1, 3, 37, 2048 -> NV 2;  2049, 4096 -> NV 4;  4097, 8192 -> NV 8;  8193, 16384 -> NV 8 x 512;  16385, 20449, 20480 -> NV 10 x 512;  20481 refused
  fwd/bwd 1 .. 2048 -> reg 2;  2049, 4096 -> reg 4;  4097, 8192 -> reg 8;  8193 .. 20481 -> vec
"""
import numpy as np
import pytest

from tests import scvi_head_ref as R

pytestmark = pytest.mark.gpu

TRAIN_INSTANCE = {1: (2, 256), 3: (2, 256), 37: (2, 256), 2048: (2, 256), 2049: (4, 256), 4096: (4, 256), 4097: (8, 256), 8192: (8, 256),
                  8193: (8, 512), 16384: (8, 512), 16385: (10, 512), 20449: (10, 512), 20480: (10, 512), 20481: None}
SEP_INSTANCE = {1: 2, 3: 2, 37: 2, 2048: 2, 2049: 4, 4096: 4, 4097: 8, 8192: 8, 8193: 0, 16384: 0, 16385: 0, 20449: 0, 20480: 0, 20481: 0}
CASES = [(G, kind) for G in R.WIDTHS for kind in R.KINDS]
IDS = [f"{G}-{kind}" for G, kind in CASES]
_REF = {}


@pytest.fixture(scope="module")
def eng():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd import engine
  return engine


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def reference(G, kind):
  """the launches of (G, kind) with their float64 reference, computed once and shared by the forms; nothing in it is written to afterwards"""
  key = (G, kind)
  if key not in _REF:
    Gp = R.round_up(G, 32)
    n_add = R.n_add_train(Gp) if R.train_instance(Gp) else R.n_add_sep(Gp)
    out = []
    for c in R.launches(G, kind):
      B = c["raw"].shape[0]
      gs = np.float32(-1.0 / B)
      h = R.head(kind, c["raw"], c["x"], c["l"].astype(np.float64), c["clip"], gs, n_add)
      out.append(dict(c, B=B, gs=gs, h=h, lib=R.library_rows(B)))
    _REF[key] = out
  return _REF[key]


class Tally:
  """worst error / bound per output; an element outside its bound (both candidates, where there are two), or a NaN, is a failure"""

  def __init__(self, name):
    self.name, self.worst, self.failures = name, {}, []

  def held(self, label, got, ref, bound, where="", keep=None, alt=None):
    got, ref, bound = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64))
    keep = np.ones(got.shape, bool) if keep is None else np.broadcast_to(keep, got.shape)
    err = np.abs(got - ref)
    if alt is not None:
      err = np.minimum(err, np.abs(got - np.broadcast_to(np.asarray(alt, np.float64), got.shape)))
    bad = (keep & ~(err <= bound)) | np.isnan(got)
    with np.errstate(invalid="ignore", divide="ignore"):
      ratio = np.where(keep & (err > 0), err / bound, 0.0)
    r = float(np.nanmax(ratio)) if ratio.size else 0.0
    if r >= self.worst.get(label, (-1.0,))[0]:
      at = np.unravel_index(int(np.nanargmax(ratio)), ratio.shape) if ratio.size else ()
      self.worst[label] = (r, where, tuple(int(i) for i in at))
    if bad.any():
      at = np.unravel_index(int(np.argmax(bad)), bad.shape)
      self.failures.append((label, where, int(bad.sum()), tuple(int(i) for i in at), float(got[at]), float(ref[at]), float(bound[at])))

  def done(self):
    for k, (v, where, at) in self.worst.items():
      print(f"{self.name} {k}: worst error / bound {v:.3f} ({where}, at {at})")
    for f in self.failures[:12]:
      print(f"    OUTSIDE THE BOUND (check, where, elements, at, got, reference, bound) {f}")
    assert not self.failures, (self.name, len(self.failures), self.failures[:6])


def _train(eng, c, G, kind, Gp, x=None, sel=None, rows=None, x_identity=False):
  """the training launch of a case (its rows `sel`), the library head pinned.  With `rows` the counts `x` and the library priors are handed
  over whole: the kernel picks row rows[b] of the priors and, unless x_identity, of x"""
  sel = np.arange(c["B"]) if sel is None else np.asarray(sel)
  x = R.padded(c["x"], Gp) if x is None else x
  B = len(sel)
  x, lib = (x[sel], c["lib"][sel]) if rows is None else (x, c["lib"])
  return eng.k_scvi_head_train(R.padded(c["raw"], Gp)[sel], x, c["l"][sel].reshape(B, 1), np.array([[1.0, 0.0]], np.float32),
                               np.array([0.0, R.S_RAW], np.float32), lib, G, likelihood=kind, eps=np.zeros(B, np.float32), clip_library=c["clip"],
                               grad_scale=c["gs"], kl_weight=R.KLS, ldl=R.LDL, rows=rows, x_identity=x_identity)


def _same(a, b, names, where):
  for n in names:
    assert np.array_equal(_bits(a[n]), _bits(b[n])), (where, n)


TRAIN_OUT = ("draw", "llk_part", "l", "sig", "eps", "kl", "dl", "dlatl")


@pytest.mark.parametrize("G,kind", CASES, ids=IDS)
def test_train_launch(eng, G, kind):
  """scvi_head_train_kernel: every output inside its bound with float and with uint16 counts (the same bits), exact zeros in the padding and in
  dlatl beyond its two columns, dl exactly 0 at and beyond the library clip's ends, no word of the kernel's left as the NaN pattern; a row's bits
  do not depend on B or its neighbours; `rows` as a permutation with x_identity 0 and 1 permutes the outputs.  At 20481 the entry refuses."""
  from sisua_amd._hip import SmxError
  Gp, k = R.round_up(G, 32), 3 if kind == "zinbd" else 2
  assert R.train_instance(Gp) == TRAIN_INSTANCE[G]
  ref = reference(G, kind)
  if TRAIN_INSTANCE[G] is None:
    with pytest.raises(SmxError) as ei:
      _train(eng, ref[0], G, kind, Gp)
    assert ei.value.code == -1 and "scvi_head_train" in str(ei.value)
    return
  t = Tally(f"train {G} {kind}")
  for c in ref:
    h, B, w = c["h"], c["B"], c["name"]
    o = _train(eng, c, G, kind, Gp)
    assert o["guards_ok"], w
    for n in TRAIN_OUT:
      assert not np.isnan(o[n]).any(), (w, n)
    assert not np.isnan(o["latl"][:, :2]).any(), w
    draw = o["draw"].reshape(B, k, Gp)
    assert not draw[:, :, G:].any() and not o["dlatl"][:, 2:].any(), w
    for p in range(k):
      t.held(f"d raw_{p}", draw[:, p, :G], h["draw"][:, p], h["E_draw"][:, p], w, keep=h["keep"], alt=h["draw_alt"][:, p])
    t.held("llk_part", o["llk_part"], h["llk"], h["E_llk"], w)
    t.held("dl", o["dl"], h["dl"], h["E_dl"], w)
    assert not o["dl"][~h["f"]["l_in"]].any(), w
    lb = R.library(c["l"].astype(np.float64), R.S_RAW, 0.0, c["lib"][:, 0], c["lib"][:, 1], R.KLS, h["dl"], h["E_dl"])
    assert np.array_equal(_bits(o["l"]), _bits(c["l"])) and not o["eps"].any(), w
    assert np.array_equal(_bits(o["latl"][:, 0]), _bits(c["l"])) and np.array_equal(_bits(o["latl"][:, 1]), _bits(np.full(B, R.S_RAW, np.float32))), w
    for n, key in (("sig", "sig"), ("kl", "kl")):
      t.held(n, o[n], lb[key], lb["E_" + key], w)
    t.held("d mu_l", o["dlatl"][:, 0], lb["dlatl0"], lb["E_dlatl0"], w)
    t.held("d s_l", o["dlatl"][:, 1], lb["dlatl1"], lb["E_dlatl1"], w)
    # the uint16 load path: the same bits
    u = _train(eng, c, G, kind, Gp, x=R.padded(c["x"], Gp).astype(np.uint16))
    assert u["guards_ok"], w
    _same(o, u, TRAIN_OUT, (w, "u16"))
    # a row alone (B = 1): the same bits as inside the launch
    for b in (0, B - 1):
      one = _train(eng, c, G, kind, Gp, sel=[b])
      for n in TRAIN_OUT:
        assert np.array_equal(_bits(one[n][0]), _bits(o[n][b])), (w, "B = 1", b, n)
  # `rows` as a permutation (the first launch): cell b reads the counts and the library prior of row perm[b]
  c = ref[0]
  B = c["B"]
  o = _train(eng, c, G, kind, Gp)
  perm = np.roll(np.arange(B), 3)[::-1].copy().astype(np.int32)
  xp = R.padded(c["x"], Gp)
  for ident, x in ((0, xp), (1, xp[perm])):
    pc = dict(c, raw=c["raw"][perm], l=c["l"][perm])
    q = _train(eng, pc, G, kind, Gp, x=x, rows=perm, x_identity=bool(ident))
    for n in TRAIN_OUT:
      assert np.array_equal(_bits(q[n]), _bits(o[n][perm])), ("rows", ident, n)
  t.done()


@pytest.mark.parametrize("G,kind", CASES, ids=IDS)
def test_forward_launch(eng, G, kind):
  """scvi_head_fwd_reg_kernel / scvi_head_fwd_vec_kernel: the planes and the saved softmax inside their bounds, zeros in the padding"""
  Gp, k = R.round_up(G, 32), 3 if kind == "zinbd" else 2
  assert R.sep_instance(Gp) == SEP_INSTANCE[G]
  t = Tally(f"fwd {G} {kind}")
  for c in reference(G, kind):
    B, w = c["B"], c["name"]
    f = R.forward(c["raw"], c["l"].astype(np.float64), c["clip"], R.n_add_sep(Gp))
    o = eng.k_scvi_head_fwd(R.padded(c["raw"], Gp), c["l"], G, k=k, clip_library=c["clip"])
    assert o["guards_ok"], w
    pl = o["planes"].reshape(B, k, Gp)
    assert not np.isnan(pl).any() and not np.isnan(o["rho_raw"]).any(), w
    assert not pl[:, :, G:].any() and not o["rho_raw"][:, G:].any(), w
    ok = R._normal32(f["el"]) & R._normal32(f["S"])
    t.held("rho_raw", o["rho_raw"][:, :G], f["rho"], f["E_rho"], w, keep=ok)
    t.held("rate", pl[:, 0, :G], f["rate"], f["E_rate"], w, keep=ok)
    t.held("theta", pl[:, 1, :G], f["theta"], f["E_theta"], w, keep=R._normal32(f["theta"]))
    if k == 3:
      assert np.array_equal(_bits(pl[:, 2, :G]), _bits(c["raw"][:, 2])), w
  t.done()


@pytest.mark.parametrize("G,kind", CASES, ids=IDS)
def test_backward_launch(eng, G, kind):
  """scvi_head_bwd_reg_kernel / scvi_head_bwd_vec_kernel on the float64 reference's planes, gradients and softmax rounded to float32"""
  Gp, k = R.round_up(G, 32), 3 if kind == "zinbd" else 2
  t = Tally(f"bwd {G} {kind}")
  for c in reference(G, kind):
    h, B, w = c["h"], c["B"], c["name"]
    f = h["f"]
    with np.errstate(over="ignore"):
      pl = np.stack([f["rate"], f["theta"], f["gate"]][:k], axis=1).astype(np.float32)
      dp = h["dplanes"].astype(np.float32)
      rho = f["rho"].astype(np.float32)
    assert np.isfinite(pl).all() and np.isfinite(dp).all(), w
    r = R.backward_entry(pl, dp, rho, c["l"], c["clip"], R.n_add_sep(Gp))
    o = eng.k_scvi_head_bwd(R.padded(pl, Gp), R.padded(dp, Gp), R.padded(rho, Gp), c["l"], G, k=k, clip_library=c["clip"])
    assert o["guards_ok"], w
    draw = o["draw"].reshape(B, k, Gp)
    assert not np.isnan(draw).any() and not np.isnan(o["dl"]).any() and not draw[:, :, G:].any(), w
    for p in range(k):
      t.held(f"d raw_{p}", draw[:, p, :G], r["draw"][:, p], r["E_draw"][:, p], w)
    t.held("dl", o["dl"], r["dl"], r["E_dl"], w)
    assert not o["dl"][~f["l_in"]].any(), w
  t.done()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("Kl", R.LIB_KL)
def test_random_library_head(eng, kind, Kl):
  """a random library head of Kl columns and non-zero injected noise (the dot-product loop's tails: Kl = 1, 63, 65, 257): mu_l, s_l, sigma, l,
  KL and both gradients inside their bounds, and the gene outputs with l's bound carried into el"""
  G, B = 37, 4
  Gp, k = 64, 3 if kind == "zinbd" else 2
  rng = np.random.default_rng(77 + Kl)
  c = R.launches(G, kind)[0]
  raw, x = c["raw"][:B], c["x"][:B]
  hl = rng.standard_normal((B, Kl)).astype(np.float32)
  Wl = (rng.standard_normal((Kl, 2)) / np.sqrt(Kl)).astype(np.float32)
  bl = np.array([4.0, -0.5], np.float32)
  eps = np.array([0.7, -1.3, 0.0, 2.1], np.float32)
  lib, gs = R.library_rows(B), np.float32(-0.25)
  mu, e_mu = zip(*[R.dot_bound(hl[b], Wl[:, 0], bl[0], Kl) for b in range(B)])
  sr, e_sr = zip(*[R.dot_bound(hl[b], Wl[:, 1], bl[1], Kl) for b in range(B)])
  mu, e_mu, sr, e_sr = (np.array(v) for v in (mu, e_mu, sr, e_sr))
  l0 = R.library(mu, sr, eps.astype(np.float64), lib[:, 0], lib[:, 1], R.KLS, 0.0, 0.0, e_mu, e_sr)
  h = R.head(kind, raw, x, l0["l"], 1e3, gs, R.n_add_train(Gp), e_l=l0["E_l"])
  assert not h["f"]["l_und"].any() and h["f"]["l_in"].all()
  lb = R.library(mu, sr, eps.astype(np.float64), lib[:, 0], lib[:, 1], R.KLS, h["dl"], h["E_dl"], e_mu, e_sr)
  o = eng.k_scvi_head_train(R.padded(raw, Gp), R.padded(x, Gp), hl, Wl, bl, lib, G, likelihood=kind, eps=eps, clip_library=1e3, grad_scale=gs,
                            kl_weight=R.KLS, ldl=R.LDL)
  assert o["guards_ok"] and np.array_equal(_bits(o["eps"]), _bits(eps)) and not o["dlatl"][:, 2:].any()
  t = Tally(f"library head Kl {Kl} {kind}")
  t.held("mu_l", o["latl"][:, 0], mu, e_mu)
  t.held("s_l", o["latl"][:, 1], sr, e_sr)
  for n, key in (("l", "l"), ("sig", "sig"), ("kl", "kl")):
    t.held(n, o[n], lb[key], lb["E_" + key])
  t.held("d mu_l", o["dlatl"][:, 0], lb["dlatl0"], lb["E_dlatl0"])
  t.held("d s_l", o["dlatl"][:, 1], lb["dlatl1"], lb["E_dlatl1"])
  draw = o["draw"].reshape(B, k, Gp)
  for p in range(k):
    t.held(f"d raw_{p}", draw[:, p, :G], h["draw"][:, p], h["E_draw"][:, p], keep=h["keep"], alt=h["draw_alt"][:, p])
  t.held("llk_part", o["llk_part"], h["llk"], h["E_llk"])
  t.held("dl", o["dl"], h["dl"], h["E_dl"])
  t.done()


def test_refusals(eng):
  """what the launchers and the entries refuse: SMX_ERR_INVALID with a message, nothing launched"""
  from sisua_amd._hip import SmxError
  G, B = 37, 2
  one = np.array([[1.0, 0.0]], np.float32)
  lib, l = R.library_rows(B), np.full(B, 2.0, np.float32)

  def refused(call, word):
    with pytest.raises(SmxError) as ei:
      call()
    assert ei.value.code == -1 and word in str(ei.value), str(ei.value)
  for Gp, ps, ld in ((38, 40, 80), (40, 42, 84), (40, 40, 82)):          # Gp, plane_stride, ld: one at a time no multiple of 4
    raw, x = np.zeros((B, ld), np.float32), np.zeros((B, 40), np.float32)
    refused(lambda: eng.k_scvi_head_train(raw, x, l.reshape(B, 1), one, np.zeros(2, np.float32), lib, G, likelihood="nbd", eps=np.zeros(B, np.float32),
                                          Gp=Gp, plane_stride=ps, ld=ld), "scvi_head_train")
    refused(lambda: eng.k_scvi_head_fwd(raw, l, G, k=2, Gp=Gp, plane_stride=ps, ld=ld), "multiples of 4")
    refused(lambda: eng.k_scvi_head_bwd(raw, raw, np.zeros((B, Gp), np.float32), l, G, k=2, Gp=Gp, plane_stride=ps, ld=ld), "multiples of 4")
  raw, x = np.zeros((B, 128), np.float32), np.zeros((B, 64), np.float32)
  for name in ("draw", "llk_part", "l", "sig", "eps", "kl", "latl", "dlatl", "dl"):
    refused(lambda: eng.k_scvi_head_train(raw, x, l.reshape(B, 1), one, np.zeros(2, np.float32), lib, G, likelihood="nbd", eps=np.zeros(B, np.float32),
                                          omit=(name,)), "scvi_head_train")
  for name in ("planes", "rho_raw"):
    refused(lambda: eng.k_scvi_head_fwd(raw, l, G, k=2, omit=(name,)), "k_scvi_head_fwd")
  for name in ("draw", "dl"):
    refused(lambda: eng.k_scvi_head_bwd(raw, raw, np.zeros((B, 64), np.float32), l, G, k=2, omit=(name,)), "k_scvi_head_bwd")
