"""The BatchNorm launches of smx_bn.hip by themselves (Engine k_bn_fwd / k_bn_bwd: the library's own dispatch picks the form) against the
float64 reference and the derived float32 bounds of tests/batchnorm_ref.py, elementwise, on the edge grid of column families: every
register-resident form and the round-trip form, the slab batches, the wide column-major form, the forms of the other activations, the
modes, dropout from an injected mask and from Philox, SyncBatchNorm on simulated ranks.  Whatever the launch may load outside [B][H] is NaN,
every output buffer sits between guard bands, and a NaN at a kept point fails every check.  Each check prints its worst error / bound."""
import numpy as np
import pytest

from tests import batchnorm_ref as br

pytestmark = pytest.mark.gpu

B_AXIS = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
S_AXIS = (1, 3, 9, 16, 17, 33)
WIDTHS = ((5, 8, 8), (20, 24, 28), (128, 128, 128), (5, 8, 12), (20, 24, 24), (128, 128, 132))   # (H, Hp, ld): ld in {Hp, Hp + 4}
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def E():
  from sisua_amd import engine
  return engine


def _vec(x, Hp):
  """[H] -> [Hp] with NaN behind H (the launches read nothing there)"""
  if x is None:
    return None
  v = np.full(Hp, NAN, np.float32)
  v[:len(x)] = x
  return v


def _slabs(t, Hp, ld, wide, pad_nan):
  """[S][B][H] -> the launch's layout, NaN in the ld padding and in the wide form's rows from B on; the padded columns NaN or 0"""
  S, B, H = t.shape
  fill = NAN if pad_nan else np.float32(0)
  if wide:
    a = np.full((S, Hp, 128), NAN, np.float32)
    a[:, :, :B] = fill
    a[:, :H, :B] = t.transpose(0, 2, 1)
    return a
  a = np.full((S, B, ld), NAN, np.float32)
  a[:, :, :Hp] = fill
  a[:, :, :H] = t
  return a


def _mask(m, Hp, extra=4):
  if m is None:
    return None
  a = np.full((m.shape[0], Hp + extra), NAN, np.float32)
  a[:, :m.shape[1]] = m
  return a


def run_fwd(E, t, gamma, beta, Hp, ld, wide=False, pad_nan=True, mult=None, bias=None, moving_mean=None, moving_var=None, **kw):
  S, B, H = t.shape
  mm = _vec(np.zeros(H, np.float32) if moving_mean is None else moving_mean, Hp)
  mv = _vec(np.ones(H, np.float32) if moving_var is None else moving_var, Hp)
  o = E.k_bn_fwd(_slabs(t, Hp, ld, wide, pad_nan), B, H, Hp, _vec(gamma, Hp), _vec(beta, Hp), _vec(bias, Hp), mm, mv, mask=_mask(mult, Hp), wide=wide, **kw)
  assert o["guards_ok"], "a store outside an output buffer"
  assert np.all(o["out"][:, H:] == 0), "out of a padded column"
  if not pad_nan:   # zeros in, zeros out: every output of a padded column
    keys = ("xhat",) + (("batch_mean", "batch_var") if kw.get("batchnorm", True) and kw.get("training", True) else ())
    for k in keys:
      assert np.all(o[k][..., H:] == 0), k
  return o


def run_bwd(E, dt, o, gamma, beta, Hp, ld, wide=False, pad_nan=True, mult=None, **kw):
  S, B, H = dt.shape
  b = E.k_bn_bwd(_slabs(dt, Hp, ld, wide, pad_nan), o["out"], o["xhat"], B, H, Hp, o["inv_std"], _vec(gamma, Hp), _vec(beta, Hp), mask=_mask(mult, Hp),
                 wide=wide, **kw)
  assert b["guards_ok"], "a store outside an output buffer"
  if kw.get("batchnorm", True):
    assert np.all(b["dgamma"][:, H:] == 0) and np.all(b["dbeta"][:, H:] == 0), "parameter gradients of a padded column"
  if not pad_nan and not np.isnan(o["xhat"][:, H:]).any():
    assert np.all(b["dpre"][:, H:] == 0), "dpre of a padded column"
  return b


def hold(tag, got, ref, bound, keep, limit=1.0):
  w = br.worst(got, ref, bound, keep)
  print(f"bn-grid {tag} worst error / bound {w:.3f} kept {int(np.sum(keep))} of {np.size(keep)}")
  assert w <= limit, (tag, w)
  return w


def count_dropped(total, names, keeps, forward):
  for k, keep in keeps.items():
    for fam, (d, n) in br.dropped_by_family(names, keep).items():
      d0, n0 = total.get((k, fam, forward), (0, 0))
      total[(k, fam, forward)] = (d0 + d, n0 + n)


def assert_dropped(total, B):
  """the kept-point rule's yield, per output and column family over one batch size's launches: at most a tenth dropped; the 1e18 family's
  forward is asserted whole below B = 19 and not at all from there (B max^2 reaches 2^127).  One and two rows are exempt: one row is
  asserted exactly, and a column of two values is as ill-conditioned as its one difference happens to be small."""
  for (k, fam, forward), (d, n) in sorted(total.items()):
    if d:
      print(f"bn-grid dropped B={B} {k} {fam}: {d} of {n}")
    if fam == "huge18" and forward:
      assert d == (0 if B < 19 else n) or B == 1, (k, fam, d, n)
    elif B > 2:
      assert 10 * d <= n, (k, fam, d, n)


def check_fwd(tag, o, r, gamma, beta, H, stats=True):
  keep = br.fwd_keep(r, gamma, beta)
  pairs = [("xhat", o["xhat"][:, :H]), ("out", o["out"][:, :H])]
  if "inv" in r:
    pairs.append(("inv", o["inv_std"][:H]))
  if stats and "mean" in r:
    pairs += [("mean", o["batch_mean"][:H]), ("var", o["batch_var"][:H])]
  for k, got in pairs:
    hold(f"{tag} {k}", got, r[k], r["E_" + k], keep[k])
  return keep


def check_bwd(tag, b, ref, H):
  keep = br.bwd_keep(ref)
  for k in keep:
    got = b[k].astype(np.float64).sum(0)[:H] if k in ("dgamma", "dbeta") else b[k][..., :H]   # (SyncBatchNorm: the ranks' shares)
    hold(f"{tag} {k}", got, ref[k], ref["E_" + k], keep[k])
  return keep


def check_exact_columns(o, names, gamma, beta, H, act=lambda y: np.maximum(y, np.float32(0))):
  """the constant columns: every float32 sum and the division are exact, so batch_var = 0, xhat = 0 and out = act(beta) exactly"""
  for c, n in enumerate(names):
    if n in br.CONSTANT:
      assert o["batch_mean"][c] == np.float32(br.CONSTANT[n]) and o["batch_var"][c] == 0, n
      assert np.all(o["xhat"][:, c] == 0) and np.all(o["out"][:, c] == act(beta[c])), n


@pytest.mark.parametrize("B", B_AXIS)
def test_training_forms_rows_columns_slabs(E, B):
  """every register-resident form (2, 4, 8, 16 rows per thread), the round trip above 1024 rows, at every slab count and column shape:
  statistics, xhat, out, the moving update bit for bit, the backward on the device's own forward, and the composed pass"""
  total = {}
  for i, S in enumerate(S_AXIS):
    H, Hp, ld = WIDTHS[(i + B_AXIS.index(B)) % len(WIDTHS)]
    tag = f"train B={B} S={S} H={H} ld={ld}"
    t, gamma, beta, names = br.make_columns(B, H, S, seed=100 + i, shift=i)
    rng = np.random.default_rng(200 + i)
    mm, mv = rng.standard_normal(H).astype(np.float32), (1 + rng.random(H)).astype(np.float32)
    upd = i % 2 == 0
    o = run_fwd(E, t, gamma, beta, Hp, ld, pad_nan=i % 2 == 1, moving_mean=mm, moving_var=mv, update_moving=upd, momentum=0.99)
    r = br.forward(t, gamma, beta)
    count_dropped(total, names, check_fwd(tag, o, r, gamma, beta, H), True)
    check_exact_columns(o, names, gamma, beta, H)
    if B == 1:
      assert np.all(o["batch_var"][:H] == 0) and np.all(o["xhat"][:, :H] == 0)
    want_mm, want_mv = (br.moving_update(mm, o["batch_mean"][:H], 0.99), br.moving_update(mv, o["batch_var"][:H], 0.99)) if upd else (mm, mv)
    ok = r["asserted"]
    assert np.array_equal(o["moving_mean"][:H][ok], want_mm[ok]) and np.array_equal(o["moving_var"][:H][ok], want_mv[ok]), tag
    assert np.isnan(o["moving_mean"][H:]).all()     # (the padding of the moving statistics is neither read nor written)
    dt = br.make_dout(B, names, S, seed=300 + i)
    b = run_bwd(E, dt, o, gamma, beta, Hp, ld, pad_nan=i % 2 == 1)
    count_dropped(total, names, check_bwd(tag, b, br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], o["inv_std"][:H], gamma, beta), H), False)
    # composed: the float64 backward of the float64 forward, on the columns where no row sits within its bound of the kink
    rb = br.backward(dt, r["out"], r["xhat"], r["inv"], gamma, beta)
    extra = br.composed_extra(r, rb, gamma)
    away = ((np.abs(r["y"]) > r["E_y"]).all(0) & r["asserted"] & np.isfinite(r["E_inv"]))
    keep = br.bwd_keep(rb)
    for k in ("dpre", "dgamma", "dbeta"):
      got = b[k][0, :H] if k != "dpre" else b[k][:, :H]
      bound = rb["E_" + k] + extra[k]
      hold(f"{tag} composed {k}", got, rb[k], bound, keep[k] & away & br.kept(rb[k], bound, rb["S_" + k]))
  assert_dropped(total, B)


@pytest.mark.parametrize("B", (1, 37, 128))
def test_wide_form(E, B):
  """the wide column-major form: its own slab order, rows B .. 127 NaN; and the same bits as the plain form on the same sums"""
  for i, S in enumerate((1, 15, 16, 17, 250)):
    H, Hp, ld = WIDTHS[i % 3]
    tag = f"wide B={B} S={S} H={H}"
    t, gamma, beta, names = br.make_columns(B, H, S, seed=400 + i, shift=i)
    o = run_fwd(E, t, gamma, beta, Hp, ld, wide=True, pad_nan=i % 2 == 0)
    r = br.forward(t, gamma, beta)
    check_fwd(tag, o, r, gamma, beta, H)
    check_exact_columns(o, names, gamma, beta, H)
    dt = br.make_dout(B, names, S, seed=500 + i)
    b = run_bwd(E, dt, o, gamma, beta, Hp, ld, wide=True, pad_nan=i % 2 == 0)
    check_bwd(tag, b, br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], o["inv_std"][:H], gamma, beta), H)
    # the plain form on the sums the wide form made (its order replayed in float32: plain additions)
    v32, g32 = br._slab_sum32(t, wide=True)[None], br._slab_sum32(dt, wide=True)[None]
    p = run_fwd(E, v32, gamma, beta, Hp, Hp + 4, pad_nan=i % 2 == 0)
    ok = r["asserted"]
    for k in ("out", "xhat", "inv_std", "batch_mean", "batch_var"):
      assert np.array_equal(o[k][..., :H][..., ok], p[k][..., :H][..., ok], equal_nan=True), (tag, k)
    pb = run_bwd(E, g32, p, gamma, beta, Hp, Hp + 4, pad_nan=i % 2 == 0)
    for k in ("dpre", "dgamma", "dbeta"):
      assert np.array_equal(b[k][..., :H][..., ok], pb[k][..., :H][..., ok], equal_nan=True), (tag, k)


@pytest.mark.parametrize("B", (65, 1025))
def test_evaluation_mode_edges(E, B):
  """moving_var of 0, 1e-30, 1e30 and 1, moving means of 0 and +-1e4: inv, xhat, out, and the backward's dy gamma inv"""
  H, Hp, ld, S = 20, 24, 28, 3
  t, gamma, beta, names = br.make_columns(B, H, S, seed=600)
  mv = np.array([0.0, 1e-30, 1e30, 1.0], np.float32)[np.arange(H) % 4]
  mm = np.array([0.0, 1e4, -1e4], np.float32)[np.arange(H) % 3]
  o = run_fwd(E, t, gamma, beta, Hp, ld, moving_mean=mm, moving_var=mv, training=False)
  r = br.forward(t, gamma, beta, moving_mean=mm, moving_var=mv, training=False)
  check_fwd(f"eval B={B}", o, r, gamma, beta, H)
  assert np.array_equal(o["moving_mean"][:H], mm) and np.array_equal(o["moving_var"][:H], mv)
  dt = br.make_dout(B, names, S, seed=601)
  b = run_bwd(E, dt, o, gamma, beta, Hp, ld, training=False)
  check_bwd(f"eval B={B}", b, br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], o["inv_std"][:H], gamma, beta, training=False), H)


@pytest.mark.parametrize("B", (2, 129, 1025))
def test_without_batchnorm_bias_and_dbias(E, B):
  H, Hp, ld, S = 20, 24, 24, 9
  t, gamma, beta, names = br.make_columns(B, H, S, seed=700)
  bias = np.random.default_rng(701).standard_normal(H).astype(np.float32)
  o = run_fwd(E, t, None, None, Hp, ld, bias=bias, batchnorm=False)
  r = br.forward(t, bias=bias, batchnorm=False)
  check_fwd(f"nobn B={B}", o, r, None, None, H)
  dt = br.make_dout(B, names, S, seed=702)
  b = run_bwd(E, dt, o, None, None, Hp, ld, batchnorm=False)
  check_bwd(f"nobn B={B}", b, br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], batchnorm=False), H)


@pytest.mark.parametrize("B", (64, 257, 1025))
def test_leaky_relu_slope(E, B):
  """leak = 0.2 (the discriminator's activation): both sides of the kink, gamma <= 0 included, forward and backward"""
  H, Hp, ld, S = 20, 24, 28, 3
  t, gamma, beta, names = br.make_columns(B, H, S, seed=800)
  o = run_fwd(E, t, gamma, beta, Hp, ld, leak=0.2)
  r = br.forward(t, gamma, beta, leak=0.2)
  check_fwd(f"leak B={B}", o, r, gamma, beta, H)
  lk = np.float32(0.2)
  check_exact_columns(o, names, gamma, beta, H, act=lambda y: np.maximum(y, np.float32(0)) + lk * np.minimum(y, np.float32(0)))
  dt = br.make_dout(B, names, S, seed=801)
  b = run_bwd(E, dt, o, gamma, beta, Hp, ld, leak=0.2)
  check_bwd(f"leak B={B}", b, br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], o["inv_std"][:H], gamma, beta, leak=0.2), H)


@pytest.mark.parametrize("act", [a for a in br.ACT_FWD if a != "relu"])
def test_other_activations(E, act):
  """every activation of smx_act.h through the GEN_ACT forms: each register-resident form, the round trip and the wide form"""
  S = 3
  for B, wide in ((2, False), (129, False), (257, False), (513, False), (1025, False), (37, True)):
    H, Hp, ld = 20, 24, 28
    tag = f"{act} B={B} wide={int(wide)}"
    t, gamma, beta, names = br.make_columns(B, H, S, seed=900)
    mult = None
    if B == 129:   # with an injected mask
      mult = np.where(np.random.default_rng(901).random((B, H)) >= 0.5, br.drop_scale(0.5), np.float32(0)).astype(np.float32)
    kw = dict(drop_p=0.5) if mult is not None else {}
    o = run_fwd(E, t, gamma, beta, Hp, ld, wide=wide, act=act, mult=mult, **kw)
    r = br.forward(t, gamma, beta, act=act, mult=mult)
    check_fwd(tag, o, r, gamma, beta, H)
    dt = br.make_dout(B, names, S, seed=902)
    b = run_bwd(E, dt, o, gamma, beta, Hp, ld, wide=wide, act=act, mult=mult, **kw)
    ref = br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], o["inv_std"][:H], gamma, beta, act=act, mult=mult)
    check_bwd(tag, b, ref, H)


@pytest.mark.parametrize("p", (0.1, 0.5))
def test_dropout_injected_mask(E, p):
  for B in (65, 300, 1025):
    H, Hp, ld, S = 20, 24, 28, 3
    t, gamma, beta, names = br.make_columns(B, H, S, seed=1000)
    mult = np.where(np.random.default_rng(1001).random((B, H)) >= p, br.drop_scale(p), np.float32(0)).astype(np.float32)
    o = run_fwd(E, t, gamma, beta, Hp, ld, mult=mult, drop_p=p)
    check_fwd(f"drop p={p} B={B}", o, br.forward(t, gamma, beta, mult=mult), gamma, beta, H)
    dt = br.make_dout(B, names, S, seed=1002)
    b = run_bwd(E, dt, o, gamma, beta, Hp, ld, drop_p=p)
    check_bwd(f"drop p={p} B={B}", b, br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], o["inv_std"][:H], gamma, beta, p=p), H)


@pytest.mark.parametrize("B,wide", [(65, False), (1025, False), (37, True)])
def test_dropout_philox_equals_injected_multipliers(E, B, wide):
  """the launches' own Philox draw == an injected mask of k_noise's multipliers for the same key and cells, bit for bit: forward (ReLU and
  tanh) and the backward of the other activations (bn_keep)"""
  H, Hp, ld, S, p, seed, stream, step = 20, 24, 28, 3, 0.3, 0x1234567890ABCDEF, 7, 41
  t, gamma, beta, names = br.make_columns(B, H, S, seed=1100)
  dt = br.make_dout(B, names, S, seed=1101)
  for rows, base in ((None, 1000), (np.random.default_rng(1102).permutation(5000)[:B].astype(np.int32), 17)):
    cells = base + (np.arange(B) if rows is None else rows.astype(np.int64))
    mult, _ = E.k_noise(seed, stream, step, cells, Hp, p=p)
    assert set(np.unique(mult)) == {np.float32(0), br.drop_scale(p)}
    key = dict(seed=seed, stream=stream, step=step, rows=rows, cell_base=base, drop_p=p)
    for act in ("relu", "tanh"):
      a = run_fwd(E, t, gamma, beta, Hp, ld, wide=wide, act=act, **key)
      m = run_fwd(E, t, gamma, beta, Hp, ld, wide=wide, act=act, mult=mult[:, :H], drop_p=p)
      assert np.array_equal(a["out"][:, :H], m["out"][:, :H]) and np.array_equal(a["xhat"][:, :H], m["xhat"][:, :H]), act
      ba = run_bwd(E, dt, a, gamma, beta, Hp, ld, wide=wide, act=act, **key)
      bm = run_bwd(E, dt, m, gamma, beta, Hp, ld, wide=wide, act=act, mult=mult[:, :H], drop_p=p)
      for k in ("dpre", "dgamma", "dbeta"):
        assert np.array_equal(ba[k][..., :H], bm[k][..., :H]), (act, k)


@pytest.mark.parametrize("B,wide", [(65, False), (1025, False), (37, True)])
def test_nan_in_out_is_a_dropped_unit(E, B, wide):
  """PINNED: the ReLU forms take their mask from out > 0, which is false for a NaN -- a unit whose forward value is NaN gets the gradient of
  a unit at or below the kink (0, or leak x g), and the column's sums stay finite.  The NaN itself is the forward's to report (the loss and
  smx_metrics.nan_flag carry it); a backward that spread it over the column's s1 and s2 would add nothing to that."""
  H, Hp, ld, S = 20, 24, 28, 3
  t, gamma, beta, names = br.make_columns(B, H, S, seed=1200)
  dt = br.make_dout(B, names, S, seed=1201)
  for leak in (0.0, 0.2):
    o = run_fwd(E, t, gamma, beta, Hp, ld, wide=wide, leak=leak)
    hit = np.random.default_rng(1202).random((B, H)) < 0.1
    o["out"][:, :H][hit] = NAN
    b = run_bwd(E, dt, o, gamma, beta, Hp, ld, wide=wide, leak=leak)
    ref = br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], o["inv_std"][:H], gamma, beta, leak=leak)
    assert np.array_equal(ref["dy"][hit], dt.astype(np.float64).sum(0)[hit] * float(np.float32(leak)))
    check_bwd(f"nan-out B={B} leak={leak}", b, ref, H)
    assert np.isfinite(b["dpre"][:, :H]).all() and np.isfinite(b["dgamma"][:, :H]).all() and np.isfinite(b["dbeta"][:, :H]).all()
    nb = run_bwd(E, dt, o, None, None, Hp, ld, wide=wide, leak=leak, batchnorm=False)
    assert np.array_equal(nb["dpre"][:, :H][hit], (br._slab_sum32(dt, wide) * np.float32(leak))[hit] if leak else np.zeros(int(hit.sum()), np.float32))


@pytest.mark.parametrize("world,B", [(1, 64), (1, 130), (2, 128), (2, 260), (4, 128), (4, 2052)])
def test_sync_batchnorm_on_simulated_ranks(E, world, B):
  """SyncBatchNorm's two phases per simulated rank around a host-side sum of the gather buffers: the GLOBAL batch's statistics by Chan's
  combine (the mean-1e3 column in particular), xhat, out, and the backward"""
  H, Hp, ld, S = 20, 24, 28, 3
  tag = f"sync W={world} B={B}"
  t, gamma, beta, names = br.make_columns(B, H, S, seed=1300)
  o = run_fwd(E, t, gamma, beta, Hp, ld, world=world)
  r, bound = br.forward(t, gamma, beta), br.forward(t, gamma, beta, world=world)
  for k in ("mean", "var", "inv", "xhat", "y", "out"):   # the global batch's values under the two-phase form's bounds
    r["E_" + k] = bound["E_" + k]
  keep = check_fwd(tag, o, r, gamma, beta, H)
  c = names.index("mean1e3")
  assert keep["var"][c] and keep["mean"][c] and keep["xhat"][:, c].mean() >= 0.9
  dt = br.make_dout(B, names, S, seed=1301)
  b = run_bwd(E, dt, o, gamma, beta, Hp, ld, world=world)
  check_bwd(tag, b, br.backward(dt, o["out"][:, :H], o["xhat"][:, :H], o["inv_std"][:H], gamma, beta, world=world), H)


def test_sync_batchnorm_has_no_leaky_form(E):
  """the two-phase kernels spell max(y, 0) only: a slope is refused, not dropped"""
  from sisua_amd import _hip
  t, gamma, beta, names = br.make_columns(64, 20, 1, seed=1400)
  with pytest.raises(_hip.SmxError):
    run_fwd(E, t, gamma, beta, 24, 24, world=2, leak=0.2)
  o = run_fwd(E, t, gamma, beta, 24, 24, world=2)
  with pytest.raises(_hip.SmxError):
    run_bwd(E, br.make_dout(64, names, 1, seed=1401), o, gamma, beta, 24, 24, world=2, leak=0.2)
