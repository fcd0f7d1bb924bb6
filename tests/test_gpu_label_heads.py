"""The label heads' launch by itself (smx_k_label_loss: label_loss_kernel, and label_tril_kernel for 'mixtril'; sisua_amd/csrc/smx_loss.hip)
held to the float64 reference of tests/label_heads_ref.py, element by element, on its edge grid, inside the bounds that module derives
from the kernels' formulas; and the launch's layout -- masks, padding, row gathers, accumulation -- by exact assertions.  Every
tolerance here is label_heads_ref's: no figure in this file was chosen after looking at a kernel's output.  Every elementwise test
prints the worst error / bound and where; DESIGN.md 4sb records them as read on an MI355X.

LAUNCHER BRANCHES (launch_label_loss) and what reaches them:
  label_loss_kernel   nb, nbd, zinb, zinbd, bernoulli, normal         test_elementwise_on_the_grid, test_shapes
                      mixnbC, mixzinbC, mixgaussC, C = 1 .. 4         the same, test_dominated_and_dominating_components
                      onehot                                          test_onehot_on_the_grid, test_shapes
                      unlabelled rows (m == 0), every kind's width    test_layout_and_masks
  label_tril_kernel   mixtrilC, C = 2 .. 4, the 8-plane load groups    test_mixtril_on_the_grid (P = 64, C = 4: the 66.6 KB LDS request)
  both                rows, add, backward = 0, grad_scale              test_layout_and_masks (add), test_rows_gather, test_backward_off_and_grad_scale
  the refusals        of the entry and of the launcher                 test_refused_arguments"""
import numpy as np
import pytest

from tests import label_heads_ref as R

pytestmark = pytest.mark.gpu

ELEMENTWISE = [k for k in R.ALL_KINDS if k != "onehot" and not k.startswith("mixtril")]
BS = (1, 3, 4, 5, 9)
PS = (1, 5, 31, 32, 33, 64, 65, 70)
TRIL_SHAPES = [(2, 1), (3, 2), (4, 7), (2, 8), (3, 9), (4, 33), (2, 64), (3, 64), (4, 64)]
LAYOUT_KINDS = list(R.SIMPLE) + ["onehot", "mixnb3", "mixzinb2", "mixgauss4", "mixtril2", "mixtril3"]
FILL = 7.5          # what draw holds before a launch: no kernel computes it on these inputs


@pytest.fixture(scope="module")
def eng():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd import engine
  return engine


def _pp(P):
  return (P + 31) // 32 * 32


def _report(label, got, ref, bound, keep):
  """the worst error / bound over the kept elements, printed; returns the failures' description (empty: inside).  A NaN at a kept element
  is outside"""
  got = np.asarray(got, np.float64)
  err = np.where(keep, np.abs(got - ref), 0.0)
  ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
  at = np.unravel_index(int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio))), ratio.shape)
  print(f"{label}: worst error / bound {float(ratio[at]):.3f} at {tuple(int(i) for i in at)}")
  bad = keep & ~(err <= bound)
  return [(label, int(bad.sum()), float(ratio[at]), tuple(int(i) for i in at), float(got[at]), float(ref[at]))] if bad.any() else []


def _run_elementwise(eng, kind, B, P, offset=0, gs=-1.0, mask=None, **kw):
  """B cells of P grid elements each, from `offset` on (cyclically), NaN in every padded column: (result, index [B, P] into the grid)"""
  y, planes, _ = R.grid(kind)
  idx = (offset + np.arange(B * P)) % len(y)
  Pp = _pp(P)
  raw = R.pack([p[idx] for p in planes], B, P, Pp)
  Y = R.pack_y(y[idx], B, P, Pp)
  out = eng.k_label_loss(kind, raw, Y, P, mask=np.ones(B, np.uint8) if mask is None else mask, grad_scale=gs, fill=FILL, **kw)
  assert out["guards_ok"]
  return out, idx.reshape(B, P)


def _check_elementwise(label, kind, out, idx, P, gs, labelled=None):
  o = R.grid_eval(kind)
  B, Pp, k = idx.shape[0], _pp(P), R.n_planes(kind)
  lab = np.ones(B, bool) if labelled is None else labelled
  keep = o["keep"][idx] & lab[:, None]
  planes = out["draw"][:, :k * Pp].reshape(B, k, Pp)
  failures = []
  for c in range(k):
    g, bg = R.scale_grad(o["g"][c][idx], o["bg"][c][idx], gs)
    failures += _report(f"{label} d{c}", planes[:, c, :P], g, bg, keep)
  ref, bound = R.cell_sum_bound(kind, P, o["v"][idx], o["bv"][idx])
  failures += _report(f"{label} llk", out["llk"], ref, bound, keep.all(axis=1))
  assert (planes[:, :, P:] == 0).all()                              # the padded columns of every plane, labelled or not
  assert (planes[~lab] == 0).all() and (out["llk"][~lab] == 0).all()
  return failures


# ---- elementwise, labelled cells ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ELEMENTWISE)
def test_elementwise_on_the_grid(eng, kind):
  """the whole element grid of the kind, one grid element per (cell, dimension), in cells of 70 dimensions (two 64-lane passes, Pp = 96)
  and again in cells of 33 from another offset: every plane of d raw inside its bound, every cell's llk inside cell_sum_bound"""
  n = len(R.grid(kind)[0])
  failures = []
  for P, offset, gs in ((70, 0, -1.0), (33, 17, -0.7 / 37.0)):
    out, idx = _run_elementwise(eng, kind, -(-n // P), P, offset, gs)
    failures += _check_elementwise(f"{kind} P = {P}", kind, out, idx, P, gs)
  assert not failures, failures


@pytest.mark.parametrize("kind", [k for k in ELEMENTWISE if k.startswith("mix") and not k.endswith("1")])
def test_dominated_and_dominating_components(eng, kind):
  """a component whose resp is below 2^-126: its gradient planes are inside the bound's underflow term, and no NaN; a component with resp
  within 4 u of 1 in the reference: its gradients are the single-component kind's, bound-wise (label_heads_ref.dominance)"""
  base, C = R.split_kind(kind)
  kc = 3 if base == "mixzinb" else 2
  n, P = len(R.grid(kind)[0]), 64
  out, idx = _run_elementwise(eng, kind, -(-n // P), P, gs=1.0)
  o = R.grid_eval(kind)
  planes = out["draw"][:, :R.n_planes(kind) * P].reshape(idx.shape[0], -1, P).astype(np.float64)
  n_under = n_dom = 0
  for c in range(C):
    for q in range(kc):
      under, ub, dom, db = R.dominance(o, c, q)
      got = planes[:, (1 + q) * C + c]
      u, d = (under & o["keep"])[idx], (dom & o["keep"])[idx]
      assert not np.isnan(got[u | d]).any()
      assert (np.abs(got[u]) <= ub[idx][u]).all(), (kind, c, q)
      assert (np.abs(got[d] - o["comp_g"][c][q][idx][d]) <= db[idx][d]).all(), (kind, c, q)
      n_under, n_dom = n_under + int(u.sum()), n_dom + int(d.sum())
  print(f"{kind}: {n_under} gradient elements of a component below 2^-126, {n_dom} of a component within 4 u of 1")
  assert n_under >= 100 and n_dom >= 100


@pytest.mark.parametrize("P", PS)
def test_onehot_on_the_grid(eng, P):
  raw, y = R.onehot_grid(P)
  o = R.onehot(raw, y)
  B, Pp = len(raw), _pp(P)
  failures = []
  for gs in (-1.0, -0.7 / 37.0):
    out = eng.k_label_loss("onehot", R.pack([raw], B, P, Pp), R.pack_y(y, B, P, Pp), P, mask=np.ones(B), grad_scale=gs, fill=FILL)
    assert out["guards_ok"] and (out["draw"][:, P:] == 0).all()
    g, bg = R.scale_grad(o["g"][0], o["bg"][0], gs)
    failures += _report(f"onehot P = {P} grad_scale {gs:.3g} d0", out["draw"][:, :P], g, bg, o["keep"])
    ref, bound = R.cell_sum_bound("onehot", P, o["v"], o["bv"])
    failures += _report(f"onehot P = {P} llk", out["llk"], ref, bound, np.ones(B, bool))
  assert not failures, failures


def _tril_run(eng, C, P, g, gs=-1.0, **kw):
  Pp = _pp(P)
  B = g["a"].shape[0]
  out = eng.k_label_loss(f"mixtril{C}", R.tril_pack(g, C, P, Pp), R.pack_y(g["y"], B, P, Pp), P, grad_scale=gs, fill=FILL,
                         **({"mask": np.ones(B)} | kw))
  assert out["guards_ok"]
  return out


def _tril_check(label, C, P, out, o, gs, keep):
  dmix, dmu, dL, pl = R.tril_unpack(out["draw"], C, P, _pp(P))
  failures = _report(f"{label} llk", out["llk"], o["llk"], o["b_llk"], keep)
  for name, got in (("dmix", dmix), ("dmu", dmu), ("dL", dL)):
    ref, b = R.scale_grad(o[name], o["b_" + name], gs)
    failures += _report(f"{label} {name}", got, ref, b, np.broadcast_to(keep.reshape((-1,) + (1,) * (ref.ndim - 1)), ref.shape))
  assert (pl[:, :, P:] == 0).all() and (pl[:, :C, 1:] == 0).all()   # padded columns; a logit plane beyond its column 0
  assert (dL[:, :, np.triu(np.ones((P, P), bool), 1)] == 0).all()   # above the diagonal
  return failures


@pytest.mark.parametrize("C,P", TRIL_SHAPES)
def test_mixtril_on_the_grid(eng, C, P):
  """label_tril_kernel on label_heads_ref's recipe (diagonals raw -12 .. 5, cond_2(L) 1, 1e2, 1e4 and the cycled diagonal): llk, d logit,
  d mu and d L inside the bounds of the two triangular solves"""
  g = R.tril_grid(C, P)
  o = R.tril(g["a"], g["mu"], g["Lraw"], g["y"])
  failures = []
  for gs in (-1.0, -0.7 / 37.0):
    failures += _tril_check(f"mixtril{C} P = {P} grad_scale {gs:.3g}", C, P, _tril_run(eng, C, P, g, gs), o, gs, o["keep"])
  assert not failures, failures


# ---- the shapes at which the indexing can go wrong ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ELEMENTWISE + ["onehot", "mixtril3"])
def test_shapes(eng, kind):
  """B in {1, 3, 4, 5, 9} (four cells per workgroup, ragged) x P in {1, 5, 31, 32, 33, 64, 65, 70} (Pp = 32, 64, 96; a second pass from
  65), the second cell unlabelled where there is one: every element inside its bound, unlabelled rows and padded columns exactly 0"""
  failures = []
  for B in BS:
    lab = np.arange(B) != 1
    if kind == "mixtril3":
      g = {k: v[5 * B:6 * B] for k, v in R.tril_grid(3, 9).items()}
      o = R.tril(g["a"], g["mu"], g["Lraw"], g["y"])
      out = _tril_run(eng, 3, 9, g, mask=lab)
      failures += _tril_check(f"mixtril3 B = {B}", 3, 9, out, {k: (np.where(lab.reshape((-1,) + (1,) * (v.ndim - 1)), v, 0.0) if k in ("llk", "dmix", "dmu", "dL") else v)
                                                                for k, v in o.items()}, -1.0, np.ones(B, bool))
      assert (out["draw"][~lab][:, :3 * 11 * 32] == 0).all()
      continue
    for P in PS:
      if kind == "onehot":
        raw, y = R.onehot_grid(P)
        raw, y = raw[B:2 * B], y[B:2 * B]
        o = R.onehot(raw, y)
        out = eng.k_label_loss("onehot", R.pack([raw], B, P, _pp(P)), R.pack_y(y, B, P, _pp(P)), P, mask=lab, grad_scale=-1.0, fill=FILL)
        assert out["guards_ok"] and (out["draw"][:, P:] == 0).all() and (out["draw"][~lab] == 0).all() and (out["llk"][~lab] == 0).all()
        g, bg = R.scale_grad(o["g"][0], o["bg"][0], -1.0)
        failures += _report(f"onehot B = {B} P = {P} d0", out["draw"][:, :P], g, bg, o["keep"] & lab[:, None])
        ref, bound = R.cell_sum_bound("onehot", P, o["v"], o["bv"])
        failures += _report(f"onehot B = {B} P = {P} llk", out["llk"], ref, bound, lab)
      else:
        out, idx = _run_elementwise(eng, kind, B, P, offset=13 * B + 101 * P, mask=lab)
        failures += _check_elementwise(f"{kind} B = {B} P = {P}", kind, out, idx, P, -1.0, lab)
  assert not failures, failures


# ---- layout and masks: exact ---------------------------------------------------------------------------------------------------------------------
def _ordinary(kind, B, P, seed=11, n_rows=None):
  """moderate planes and targets: (raw [B, planes Pp] and Y [n_rows, Pp] with NaN in columns P .. Pp)"""
  rng = np.random.default_rng(seed)
  base, C = R.split_kind(kind)
  n_rows = B if n_rows is None else n_rows
  k, Pp = R.n_planes(kind, P), _pp(P)
  if base in ("normal", "mixgauss", "mixtril"):
    y = rng.normal(size=(n_rows, P))
  elif base == "bernoulli":
    y = rng.integers(0, 2, size=(n_rows, P))
  elif base == "onehot":
    y = np.eye(P)[rng.integers(0, P, size=n_rows)]
  else:
    y = rng.poisson(3.0, size=(n_rows, P))
  return R.pack(list(0.6 * rng.normal(size=(k, B, P))), B, P, Pp), R.pack_y(y, n_rows, P, Pp)


def _same_bits(a, b):
  return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("kind", LAYOUT_KINDS)
def test_layout_and_masks(eng, kind):
  """nine cells -- a workgroup of four unlabelled cells, a mixed one, a ragged one --, NaN in columns P .. Pp of raw and Y and in the whole Y
  row of an unlabelled cell, five spare words behind every row of raw / draw"""
  B, P = 9, (9 if kind.startswith("mixtril") else 33)
  Pp, k = _pp(P), R.n_planes(kind, P)
  raw, Y = _ordinary(kind, B, P)
  raw = np.concatenate([raw, np.full((B, 5), np.nan, np.float32)], axis=1)
  mask = np.array([0, 0, 0, 0, 1, 0, 1, 1, 0], np.uint8)
  Y[mask == 0] = np.nan
  lab = mask == 1
  llk_in = np.linspace(-3.0, 5.0, B).astype(np.float32)
  out = eng.k_label_loss(kind, raw, Y, P, mask=mask, grad_scale=-0.25, fill=FILL)
  assert out["guards_ok"]
  w = k * Pp
  assert (out["draw"][~lab, :w] == 0).all()                         # the whole planes x Pp width of an unlabelled row
  assert (out["draw"][:, w:] == np.float32(FILL)).all()             # nothing beyond it
  planes = out["draw"][:, :w].reshape(B, k, Pp)
  assert (planes[:, :, P:] == 0).all() and not np.isnan(planes).any()
  assert (planes[lab][:, :, :P] != 0).any(axis=(1, 2)).all()
  assert (out["llk"][~lab] == 0).all() and np.isfinite(out["llk"]).all() and (out["llk"][lab] != 0).all()
  acc = eng.k_label_loss(kind, raw, Y, P, mask=mask, grad_scale=-0.25, fill=FILL, add=True, llk_in=llk_in)
  assert _same_bits(acc["llk"][~lab], llk_in[~lab])                 # bit for bit the incoming value
  assert _same_bits(acc["llk"], llk_in + out["llk"]) and _same_bits(acc["draw"], out["draw"])
  none = eng.k_label_loss(kind, raw, Y, P, mask=None, grad_scale=-0.25, fill=FILL)
  assert none["guards_ok"] and (none["draw"][:, :w] == 0).all() and (none["draw"][:, w:] == np.float32(FILL)).all() and (none["llk"] == 0).all()
  Yf = np.where(np.isnan(Y), np.float32(1.0), Y)
  Yf[:, P:] = np.nan
  obs = eng.k_label_loss(kind, raw, Yf, P, mask=np.zeros(B, np.uint8), observed=True, grad_scale=-0.25, fill=FILL)
  ones = eng.k_label_loss(kind, raw, Yf, P, mask=np.ones(B, np.uint8), grad_scale=-0.25, fill=FILL)
  assert obs["guards_ok"] and _same_bits(obs["llk"], ones["llk"]) and _same_bits(obs["draw"], ones["draw"]) and (ones["llk"] != 0).all()
  assert _same_bits(ones["draw"][lab], out["draw"][lab]) and _same_bits(ones["llk"][lab], out["llk"][lab])


@pytest.mark.parametrize("kind", LAYOUT_KINDS)
def test_rows_gather(eng, kind):
  """rows with repeats and a permutation: the bits of the same cells passed in order"""
  B, P, n_rows = 7, (9 if kind.startswith("mixtril") else 33), 10
  raw, Y = _ordinary(kind, B, P, n_rows=n_rows)
  rows = np.array([3, 0, 3, 9, 7, 0, 5], np.int32)
  mask = np.array([0, 1, 1, 1, 1, 1, 0, 1, 1, 1], np.uint8)
  got = eng.k_label_loss(kind, raw, Y, P, rows=rows, mask=mask, grad_scale=-0.5, fill=FILL)
  ref = eng.k_label_loss(kind, raw, Y[rows], P, mask=mask[rows], grad_scale=-0.5, fill=FILL)
  assert got["guards_ok"] and ref["guards_ok"]
  assert _same_bits(got["llk"], ref["llk"]) and _same_bits(got["draw"], ref["draw"])
  assert (got["llk"][[1, 5]] == 0).all() and (got["llk"][[0, 2, 3, 4, 6]] != 0).all() and got["llk"][0] != got["llk"][2]   # (row 0 unlabelled; same row, other planes)


@pytest.mark.parametrize("kind", LAYOUT_KINDS)
def test_backward_off_and_grad_scale(eng, kind):
  """backward = 0: the same llk bits, draw untouched.  grad_scale -1 against -0.7 / 37: every element within one rounding of the product
  (label_heads_ref.scale_grad with no other error); grad_scale 0: exact zeros"""
  B, P = 5, (9 if kind.startswith("mixtril") else 33)
  raw, Y = _ordinary(kind, B, P, seed=5)
  one = np.ones(B, np.uint8)
  full = eng.k_label_loss(kind, raw, Y, P, mask=one, grad_scale=-1.0, fill=FILL)
  fwd = eng.k_label_loss(kind, raw, Y, P, mask=one, grad_scale=-1.0, fill=FILL, backward=False)
  assert fwd["guards_ok"] and _same_bits(fwd["llk"], full["llk"]) and (fwd["draw"] == np.float32(FILL)).all()
  gs = -0.7 / 37.0
  scaled = eng.k_label_loss(kind, raw, Y, P, mask=one, grad_scale=gs, fill=FILL)
  ref, bound = R.scale_grad(-full["draw"].astype(np.float64), np.zeros(full["draw"].shape), gs)
  assert _same_bits(scaled["llk"], full["llk"]) and not _report(f"{kind} grad_scale {gs:.3g} against -1", scaled["draw"], ref, bound, np.ones(ref.shape, bool))
  zero = eng.k_label_loss(kind, raw, Y, P, mask=one, grad_scale=0.0, fill=FILL)
  assert (zero["draw"] == 0).all() and _same_bits(zero["llk"], full["llk"])


def test_refused_arguments(eng):
  """every refusal of the entry and of the launcher: SMX_ERR_INVALID with its own message -- the model's for the label dimension, the
  launcher's for 'mixtril', the entry's for what a model computes itself (Pp, ld, the rows) --, and the library stays usable"""
  from sisua_amd._hip import SmxError
  raw, Y = np.zeros((2, 4096), np.float32), np.zeros((2, 128), np.float32)
  tril = "label_loss: 'mixtril' heads take 1..64 label dimensions and 2..4 components"
  comps = "k_label_loss: mixture label heads have 1..4 components"
  pp, ld = "k_label_loss: Pp is the label dimension rounded up to 32", "k_label_loss: ld is below planes x Pp"
  bad = [(dict(kind="nb", P=0, Pp=32), "label_dim must be > 0"), (dict(kind="mixtril2", P=65, Pp=96), tril), (dict(kind="mixtril1", P=4), tril),
         (dict(kind="mixtril5", P=4), tril), (dict(kind="mixnb0", P=4), comps), (dict(kind="mixgauss5", P=4), comps), (dict(kind="mixzinb5", P=4), comps),
         (dict(kind="nb", P=33, Pp=40), pp), (dict(kind="nb", P=33, Pp=96), pp), (dict(kind="zinb", P=33, ld=3 * 64 - 1), ld),
         (dict(kind="mixtril2", P=9, ld=2 * 11 * 32 - 1), ld), (dict(kind="onehot", P=5, rows=[0, 2]), "k_label_loss: a row index lies outside Y")]
  for kw, message in bad:
    with pytest.raises(SmxError) as e:
      eng.k_label_loss(kw.pop("kind"), raw[:, :kw.pop("ld", 4096)], Y, mask=np.ones(2), **kw)
    assert e.value.code == -1 and message in str(e.value), (kw, str(e.value))
  ok = eng.k_label_loss("nb", raw[:, :64], Y, 5, mask=np.ones(2))
  assert ok["guards_ok"] and np.isfinite(ok["llk"]).all()
