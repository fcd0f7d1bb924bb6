"""Every kernel that evaluates the latent heads' sample, KL, gradients or importance-weight terms, held to the float64 values of
tests/latent_terms_ref.py on its edge grid, element by element and inside bounds derived from the kernels' own formulas (that module's
docstring has the table).  No tolerance here was chosen after looking at a kernel's output.  Every test prints the worst error / bound and
where it occurred; DESIGN.md 4t records them as read on an MI355X.

THE PIN.  lat/W = 0 and lat/b = a grid row: every cell of a step has the same (mu, raw) per latent dimension; lr = 0, and lat/W, lat/b are
what was set, bit for bit, after the steps.  The noise is injected (Engine.set_noise): cell b, dimension d takes EPS_AXIS[(b + d) % 7], so a
step's cells carry the whole noise axis against every (mu, raw) -- the product, not one axis at a time.  A grid row holds ONE raw-scale value in
every dimension and the locations cycling over the dimensions (two offsets: the moderate eight, the extreme eight); `isolated` rows hold one
point of the RAW x LOC product and (mu, raw) = (0, 0) elsewhere (their KL: 7e-15, inside the bound's sum term), so that metrics['kl'] cannot
hide a point behind mu^2 = 1e38 of its neighbour.

THE REDUCTIONS.  metrics['kl'] = mean_b sum_d KL_d: |got - ref| <= sum_d b_d + N_ADD_KL u sum_d |KL_d| + u |ref| + D 2^-126, N_ADD_KL = 39: a lane adds
its 4 elements (quad form; the scalar form 2 at the widths here), at most 6 shuffle steps, then metrics_body's sweep and mean over the cells,
for which DESIGN 4s derives 29 (an upper bound here: one partial per cell).  lat/b's gradient = sum_b (beta / B) (partial): B equal terms,
|got - beta ref| <= b + (B + 12) u |ref| + (B + 4) 2^-126 (test_gpu_likelihood_grid's count: the scale's rounding and its product 2, at most B
additions of B equal terms, 2 for a bf16 x 3 product by 1.0, 8 of slack).  The sign and size were read off smx_backward.hip: the step's KL weight is
kl_scale_of = beta / B_global, the bias gradient the column sum of d lat over the cells.

LAUNCHER TABLE: the copies of the formula and what reaches them.
  forward sample + KL
    latent_fwd_quad_kernel        front off, Dp / 4 a power of two (D <= 64 here: 1, 8, 32, 33)         test_forward_kl_and_disconnected_gradient[*] form front_off; eval_step / forward() of every form
    latent_fwd_kernel (scalar)    Dp / 4 no power of two: D = 70 (Dp = 96)                                test_forward_kl_and_disconnected_gradient[d70_b37]
    latent_tile_to_lds (FRONT)    a training step with front on, Dp 32 or 64                              ... forms default, bwd_front_off, no_fold_dz (train_step's kl, and the stored sigma the backward reads)
  backward
    gemm_latent_bwd (EPI = 2)     bwd_front off; or fold_dz not applicable (a first decoder layer != 128)  ... forms default (dec 32), bwd_front_off, no_fold_dz
    fold_dz_tile (smx_bn.hip)     front + bwd_front on, Dp = 32, B <= 128, dec0 = 128 units                test_*[d8_dec128_*] form default
    latent_bwd_kernel             launch_latent_bwd has no caller: NOT REACHED from Engine
  the importance weight
    score_decoder1_kernel         stacked scoring, a one-layer decoder (the default here)                 test_scoring_latent_terms[*] form stacked
    score_draws_kernel            knob no_score_dec1                                                      ... form stacked_three_launches
    iw_stack_kernel               both stacked forms (its log-sum-exp)                                    ... forms stacked*
    score_walk (the head's form)  knob score_walk 1, 2: the tile form's bits                             ... form stacked, asserted
    iw_accum_kernel               stacked_scoring off: latent_fwd_quad_kernel per draw + iw_accum          ... form per_draw
  scVI's library latent
    scvi_head_train (fused)       scvi_fused on (default)                                                  test_scvi_library_latent[fused]
    lib_latent_fwd / bwd_kernel   scvi_fused off; eval_step and forward() always                           test_scvi_library_latent[*]
    the library terms of score_draws_kernel / iw_accum_kernel                                              test_scvi_library_latent[*] (marginal_llk, both forms)
  full covariance
    latent_tril_fwd / bwd_kernel  latent_tril = True, D = 1, 7, 32                                         test_tril_head[*]
  NOT REACHED: latent_bwd_kernel; the mixture posterior (mixlat_*); SCALE's mixture priors (scale_prior_*); lat/W's gradient
  elementwise; per-cell variation of (mu, raw).
"""
import numpy as np
import pytest

from tests import latent_terms_ref as T
from tests import likelihood_grad_ref as L

pytestmark = pytest.mark.gpu

U = T.U
N_ADD_KL = 39
G = 40
STREAM_EPS_Z, STREAM_EPS_L = 64, 65          # (oracle.sisua_oracle's stream numbers)
LOC_SETS = (np.array(T.LOC_AXIS[:8], np.float32), np.array(T.LOC_AXIS[5:], np.float32))


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


@pytest.fixture(scope="module")
def counts():
  from tests.util import synth_counts
  return synth_counts(400, G, sparsity=0.8, seed=2)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eps(B, D):
  ax = np.array(T.EPS_AXIS, np.float32)
  return ax[(np.arange(B)[:, None] + np.arange(D)[None, :]) % len(ax)]


class Tally:
  """worst error / bound per label; a NaN where the reference is kept, or an element outside its bound, is a failure"""

  def __init__(self, name):
    self.name, self.worst, self.failures = name, {}, []

  def held(self, label, got, ref, bound, where="", cells=1, floor=None):
    """cells: a batch mean is formed as a float32 sum over the cells divided by their number -- the checked quantity that has to stay below
    2^127 is that sum (it leaves the kept points only in the location column 1e19, which the grid's rule lets drop).  floor: the elements at or
    above a documented floor; below it an element is held to "no NaN" only"""
    got, ref, bound = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64))
    keep = T.kept(ref * cells)
    err = np.abs(got - ref)
    under = np.zeros(got.shape, bool) if floor is None else ~np.broadcast_to(floor, got.shape)
    keep = keep & ~under
    bad = (keep & ~(err <= bound)) | (under & np.isnan(got))
    # a dropped point: no NaN; +-inf of the right sign or a finite float
    bad |= ~keep & (np.isnan(got) | (np.isinf(got) & (np.sign(got) != np.sign(ref))))
    with np.errstate(invalid="ignore", divide="ignore"):
      ratio = np.where(keep & (err > 0), err / bound, 0.0)
    r = float(np.max(ratio)) if ratio.size and not np.isnan(ratio).any() else float("nan")
    self.worst[label] = r if np.isnan(r) else max(self.worst.get(label, 0.0), r)
    if bad.any():
      at = np.unravel_index(int(np.argmax(bad)), bad.shape)
      self.failures.append((label, where, int(bad.sum()), tuple(int(i) for i in at), float(got[at]), float(ref[at]), float(bound[at])))

  def report(self):
    for k, v in self.worst.items():
      print(f"{self.name} {k}: worst error / bound {v:.3f}")
    for f in self.failures[:12]:
      print(f"    OUTSIDE THE BOUND (check, where, elements, at, got, reference, bound) {f}")

  def done(self):
    self.report()
    assert not self.failures, (self.name, len(self.failures), self.failures[:6])


def grid_rows(D, isolated_at=None):
  """[(label, mu [D], raw [D])] float32: per raw-scale value and location set, every dimension that raw scale and the locations cycling; with
  isolated_at = d, the RAW x LOC product one point at a time in dimension d and (0, 0) elsewhere"""
  rows = []
  if isolated_at is not None:
    mus, raws = T.kl_grid()
    for m, r in zip(mus, raws):
      mu, raw = np.zeros(D, np.float32), np.zeros(D, np.float32)
      mu[isolated_at], raw[isolated_at] = m, r
      rows.append((f"isolated mu {float(m):g} raw {float(r):g}", mu, raw))
    return rows
  for r in T.RAW_AXIS:
    for s, locs in enumerate(LOC_SETS):
      rows.append((f"raw {r:g} locations {s}", locs[np.arange(D) % len(locs)].copy(), np.full(D, r, np.float32)))
  return rows


def _cfg(D, dec=32, **kw):
  from sisua_amd.config import ModelConfig
  base = dict(model="vae", n_genes=G, likelihood="nb", enc_units=(32,), dec_units=(dec,), latent_dim=D, lr=0.0, dropout_enc=0.0, dropout_dec=0.0)
  base.update(kw)
  return ModelConfig(**base)


def _kl_bound(kl_d, b_d):
  ref = kl_d.sum()
  return ref, b_d.sum() + N_ADD_KL * U * np.abs(kl_d).sum() + U * abs(ref) + kl_d.size * T.F32_MIN


# ---- the diagonal head: forward, KL, the disconnected gradient ---------------------------------------------------------------------------
# (D, decoder units, cells, isolated dimension or None)
DIAG_CASES = {
    "d1_b37": (1, 32, 37, 0),             # latent_dim = 1: the RAW x LOC product one point per step
    "d8_b4": (8, 32, 4, None),
    "d8_b37": (8, 32, 37, None),
    "d8_b128": (8, 32, 128, None),
    "d32_b37": (32, 64, 37, None),         # the reductions at full width
    "d33_b37": (33, 32, 37, None),         # ... and ragged (Dp = 64)
    "d8_dec128_b37": (8, 128, 37, None),   # fold_dz_tile
    "d8_dec128_b128": (8, 128, 128, 3),    # ... at its largest minibatch, isolated points in dimension 3
    "d70_b37": (70, 32, 37, 64),           # the scalar forward kernel; isolated points in dimension 64 (a lane's second element)
}
# form: (flags, knobs).  Forward copies: FRONT (front on) | quad / scalar (front off).  Backward copies: fold_dz_tile | gemm epilogue.
DIAG_FORMS = {
    "default": ({}, {}),
    "front_off": ({"front": False}, {}),
    "bwd_front_off": ({"bwd_front": False}, {}),
    "no_fold_dz": ({}, {"no_fold_dz": 1}),
}


def _run_diag(Engine, counts, D, dec, B, rows_, flags, knobs, connected=None):
  """the steps of one form: per grid row train_step's kl and lat/b gradient, eval_step's kl, forward()'s z_scale / z_sample"""
  from sisua_amd import _hip
  e, out = None, []
  eps = _eps(B, D)
  ids = np.arange(B, dtype=np.int32)
  try:
    for name, v in knobs.items():
      _hip.set_tuning(name, v)
    e = Engine(_cfg(D, dec), max_batch=max(B, 4))
    for name, v in flags.items():
      e.set_flag(name, v)
    W0 = np.zeros(e.shapes["lat/W"], np.float32)
    if connected is None:
      e.set_params({"dec0/W": np.zeros(e.shapes["dec0/W"], np.float32)})
    else:
      e.set_params(connected)
    e.upload(counts)
    for label, mu, raw in rows_:
      b = np.concatenate([mu, raw]).astype(np.float32)
      e.set_params({"lat/W": W0, "lat/b": b})
      e.set_noise(STREAM_EPS_Z, eps)          # (injected noise serves until the next training step has used it)
      ev = e.eval_step(ids)
      f = e.forward(row_ids=ids, want_x_params=False)
      m = e.train_step(ids)
      g = e.get_params(1)["lat/b"].copy()
      p = e.get_params(0)
      assert np.array_equal(_bits(p["lat/W"]), _bits(W0)) and np.array_equal(_bits(p["lat/b"]), _bits(b)), label
      out.append(dict(kl=np.float32(m["kl"]), kl_eval=np.float32(ev["kl"]), grad=g, z_scale=f["z_scale"].copy(), z_sample=f["z_sample"].copy(),
                      z_mean=f["z_mean"].copy()))
  finally:
    if e is not None:
      e.close()
    for name in knobs:
      _hip.clear_tuning(name)
  return out


@pytest.mark.parametrize("case", list(DIAG_CASES))
def test_forward_kl_and_disconnected_gradient(Engine, counts, case):
  """dec0/W = 0: the decoder returns dz = 0 exactly, and lat/b's gradient is beta (dKL/dmu, dKL/draw) element by element -- the check that sees a
  wrong sigma - 1 / sigma, a wrong sigmoid shift or a lost term.  forward(): z_scale and z_sample elementwise (every cell another noise value).
  metrics['kl'] of train_step and eval_step against sum_d KL_d.  The forms against each other: the forward copies claim the same arithmetic
  ("same arithmetic, same Philox blocks as latent_fwd_quad_kernel", smx_bn.hip) -- train_step's kl, eval_step's and forward()'s outputs: the same
  bits in every form.  lat/b's gradient is the column sum of d lat, which the backward forms add in different orders (7 ulp apart over 128 equal
  terms on the device): no claim of equal bits, every form inside the bound.  THE FLOOR: the scale's gradient is held to its bound from the raw scale
  DRAW_FLOOR = -87 up (the last normal sigma) and to "no NaN" below it -- the backward forms of the training step keep their lines;
  everything else, the KL of every form included, is held at every raw scale."""
  D, dec, B, iso = DIAG_CASES[case]
  rows_ = grid_rows(D, iso)
  eps = _eps(B, D).astype(np.float64)
  t = Tally(case)
  res = {}
  for form, (flags, knobs) in DIAG_FORMS.items():
    if form == "no_fold_dz" and dec != 128:
      continue
    res[form] = _run_diag(Engine, counts, D, dec, B, rows_, flags, knobs)
    for (label, mu, raw), r in zip(rows_, res[form]):
      ref, bd = T.diag_terms(mu[None, :], raw[None, :], eps), T.diag_bounds(mu[None, :], raw[None, :], eps)
      one, bone = T.diag_terms(mu, raw), T.diag_bounds(mu, raw)
      assert np.array_equal(_bits(r["z_mean"]), _bits(np.broadcast_to(mu, (B, D)))), (form, label)
      t.held(f"{form} z_scale", r["z_scale"], one["sigma"][None, :], bone["sigma"][None, :], label)
      t.held(f"{form} z_sample", r["z_sample"], ref["z"], bd["z"], label)
      kl_ref, kl_bound = _kl_bound(one["kl"], bone["kl"])
      t.held(f"{form} train_step kl", r["kl"], kl_ref, kl_bound, label, cells=B)
      t.held(f"{form} eval_step kl", r["kl_eval"], kl_ref, kl_bound, label, cells=B)
      for name, got, k in (("d lat/b mu", r["grad"][:D], "dmu"), ("d lat/b raw", r["grad"][D:], "draw")):
        t.held(f"{form} {name}", got, one[k], bone[k] + (B + 12.0) * U * np.abs(one[k]) + (B + 4.0) * T.F32_MIN, label,
               floor=T.above_floor(raw) if k == "draw" else None)
  t.report()
  base = res["default"]
  for form, rs in res.items():
    for (label, mu, raw), a, b in zip(rows_, base, rs):
      assert np.array_equal(_bits(a["kl"]), _bits(b["kl"])) and np.array_equal(_bits(a["kl_eval"]), _bits(b["kl_eval"])), (case, form, label, "kl")
      assert np.array_equal(_bits(a["z_sample"]), _bits(b["z_sample"])) and np.array_equal(_bits(a["z_scale"]), _bits(b["z_scale"])), (case, form, label)
  assert not t.failures, (case, len(t.failures), t.failures[:6])


# ---- the diagonal head: the connected gradient against the oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("dec", [32, 128])
def test_connected_gradient_matches_oracle(Engine, counts, dec, monkeypatch):
  """(The scale's gradient from DRAW_FLOOR up; below it: no NaN.)  One pass per raw-scale value at ordinary decoder weights, the moderate locations in the latent bias: lat/b's gradient elementwise against
  oracle.forward_backward in float64 under the same injected noise.  Tolerance: the latent-term bound (as above, B terms) plus the project's
  step tolerance RTOL = 1e-4 (tests/test_gpu_step.py) times sum_b |dz| (the location) or sum_b |dz eps sigmoid(x)| (the scale), dz the oracle's
  own d loss / d z per cell.  dec = 128: fold_dz_tile against the gemm epilogue (knob no_fold_dz), both inside the bound."""
  from oracle import sisua_oracle as so
  from tests.util import perturbed_params
  from scipy.special import expit
  RTOL = 1e-4
  D, B = 8, 37
  kw = dict(model="vae", n_genes=G, likelihood="nb", enc_units=(32,), dec_units=(dec,), latent_dim=D, lr=0.0, dropout_enc=0.0, dropout_dec=0.0)
  spec = so.Spec(**kw)
  params = perturbed_params(spec)
  params["lat/W"] = np.zeros_like(params["lat/W"])
  rows_ = [r for r in grid_rows(D) if r[0].endswith("locations 0")]
  eps = _eps(B, D)
  seen = {}
  orig = so._mlp_bwd

  def spy(spec_, params_, prefix, *a, **k):
    r = orig(spec_, params_, prefix, *a, **k)
    if prefix == "dec":
      seen["dz"] = np.asarray(r, np.float64).copy()
    return r
  monkeypatch.setattr(so, "_mlp_bwd", spy)
  refs = []
  for label, mu, raw in rows_:
    p = dict(params)
    p["lat/b"] = np.concatenate([mu, raw]).astype(np.float64)
    r = so.forward_backward(spec, p, so.init_bn_state(spec), counts[:B], so.InjectedNoise({}, {STREAM_EPS_Z: eps}, {}))
    x = T.x_exact(raw)
    refs.append((r["grads"]["lat/b"], np.abs(seen["dz"]).sum(0), np.abs(seen["dz"] * eps * expit(x)[None, :]).sum(0)))
  t = Tally(f"connected dec {dec}")
  dev = {k: v.astype(np.float32) for k, v in params.items()}
  for form, (flags, knobs) in DIAG_FORMS.items():
    if form == "no_fold_dz" and dec != 128:
      continue
    got = _run_diag(Engine, counts, D, dec, B, rows_, flags, knobs, connected=dev)
    for (label, mu, raw), r, (gref, sdz, sdze) in zip(rows_, got, refs):
      bone = T.diag_bounds(mu, raw)
      latent = lambda k, ref: bone[k] + (B + 12.0) * U * np.abs(ref) + (B + 4.0) * T.F32_MIN
      t.held(f"{form} d lat/b mu", r["grad"][:D], gref[:D], latent("dmu", gref[:D]) + RTOL * sdz, label)
      t.held(f"{form} d lat/b raw", r["grad"][D:], gref[D:], latent("draw", gref[D:]) + RTOL * sdze + T.F32_MIN * sdz * 5.5, label, floor=T.above_floor(raw))
  t.done()


# ---- scoring: the importance weight's latent terms ---------------------------------------------------------------------------------------
S_SCORE = 3
SCORE_FORMS = {   # (stacked_scoring, knobs)
    "stacked": (True, {}),
    "stacked_three_launches": (True, {"no_score_dec1": 1}),
    "per_draw": (False, {}),
}
N_ADD_W = 10      # the latent terms of a draw: a lane adds at most 2 (Dp <= 128), wave_sum 6, the likelihood 1, one of slack


def _row_llk(x, planes, n_add):
  return L.draw_bound("nb", x, planes, False, n_add)


def _lme(lw):
  mx = lw.max(0)
  return mx + np.log(np.exp(lw - mx).sum(0)) - np.log(lw.shape[0])


@pytest.mark.parametrize("form", list(SCORE_FORMS))
@pytest.mark.parametrize("D", [8, 33])
def test_scoring_latent_terms(Engine, counts, D, form):
  """marginal_llk with out/W = 0 and out/b at an ordinary plane: the likelihood is the same in every draw, the first output's latent part the only
  thing that varies.  Reference: log-mean-exp over the S = 3 draws of llk + sum_d (-z^2 / 2 + eps^2 / 2 + log sigma) in float64, eps the device's own
  float32 normals of the draw (k_noise: Philox step 0, sample s, the cell's row id).  Bound per draw: the likelihood's (n_add = 13 + 6 +
  S + 1 covers both forms) + sum_d b_d + N_ADD_W u sum_d sizes + u |lw|; the log-mean-exp (test_scoring_on_the_grid's docstring): its derivative
  with respect to a draw's weight is a softmax weight <= 1, so max_s of the draws' bounds, + 2 u |L| + (S + 10) u (1 + log S).  Resident rows and host
  rows; the walk form of the head (knob score_walk) gives the tile form's bits, and the one-launch decoder the three launches' bits (knob
  no_score_dec1; the source's claim, asserted at every grid row, resident and host rows).  This is the check that reproduces DESIGN 4s's NaN: before the
  repair every raw scale from -88 down gave -inf weights in every draw (logf(0)) and exp(-inf - -inf) = NaN."""
  from sisua_amd import _hip
  from sisua_amd import engine as eng
  stacked, knobs = SCORE_FORMS[form]
  B = 5
  ids = np.arange(B, dtype=np.int32)
  x = counts[:B]
  plane = np.array(L.MODERATE["nb"], np.float32)
  bias = plane[np.arange(G) % len(plane)].T.copy()          # [2, G]
  ref_l, bound_l = _row_llk(x, list(bias), 13 + 6 + S_SCORE + 1)
  t = Tally(f"scoring D {D} {form}")
  e = None
  try:
    e = Engine(_cfg(D), max_batch=8)
    e.set_params({"out/W": np.zeros(e.shapes["out/W"], np.float32), "out/b": bias.reshape(-1), "lat/W": np.zeros(e.shapes["lat/W"], np.float32)})
    e.upload(counts)
    e.set_flag("stacked_scoring", stacked)
    eps = np.stack([eng.k_noise(e.cfg.seed, STREAM_EPS_Z, 0, ids, D, sample=s)[1] for s in range(S_SCORE)]).astype(np.float64)   # [S, B, D]
    for label, mu, raw in grid_rows(D):
      e.set_params({"lat/b": np.concatenate([mu, raw]).astype(np.float32)})
      base = (e.marginal_llk(row_ids=ids, n_samples=S_SCORE), e.marginal_llk(x=x, n_samples=S_SCORE))
      for name, v in knobs.items():
        _hip.set_tuning(name, v)
      try:
        res, host = (e.marginal_llk(row_ids=ids, n_samples=S_SCORE), e.marginal_llk(x=x, n_samples=S_SCORE)) if knobs else base
        if stacked and not knobs:
          for ranges in (1, 2):
            _hip.set_tuning("score_walk", ranges)
            try:
              alt = e.marginal_llk(row_ids=ids, n_samples=S_SCORE)
            finally:
              _hip.clear_tuning("score_walk")
            assert np.array_equal(_bits(alt[0]), _bits(res[0])) and np.array_equal(_bits(alt[1]), _bits(res[1])), (label, ranges)
        if "no_score_dec1" in knobs:     # smx_score.hip: "The draws are score_draws_kernel's, bit for bit" -- and with out/W = 0 the likelihood is too
          for a, b in ((base[0], res), (base[1], host)):
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), (label, "one launch against three")
      finally:
        for name in knobs:
          _hip.clear_tuning(name)
      w, bw = T.diag_terms(mu, raw, eps), T.diag_bounds(mu, raw, eps)
      sizes = 0.5 * w["z"] ** 2 + 0.5 * eps ** 2 + np.abs(w["log_sigma"])
      lw = ref_l[None, :] + w["w"].sum(-1)                                  # [S, B]
      b_draw = bound_l[None, :] + bw["w"].sum(-1) + N_ADD_W * U * sizes.sum(-1) + U * np.abs(lw)
      ref = _lme(lw)
      bound = b_draw.max(0) + 2.0 * U * np.abs(ref) + (S_SCORE + 10.0) * U * (1.0 + np.log(S_SCORE))
      for name, r in (("resident rows", res), ("host rows", host)):
        t.held(f"marginal_llk ({name})", r[0], ref, bound, label)
        t.held(f"mean llk ({name})", r[1], ref_l, bound_l, label)
  finally:
    if e is not None:
      e.close()
  t.done()


# ---- scVI's library latent ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_scvi_library_latent(Engine, counts, fused):
  """latl/W = 0, latl/b = the RAW x LOC product one point per step, under each of the three library priors (every cell of a step the same prior).
  clip_library = 1e-30 and, in the training step, the library noise 0: l = mu, and no grid location lies inside (0, 1e-30), so d loss / d l is
  exactly 0 (the rate's gradient reaches l only inside the clip) and latl/b's gradient is beta (dKL_l/dmu, dKL_l/draw).  l_scale, l_sample (forward(), the noise axis over the cells), metrics['kl_l'] of
  train_step (the fused copy, or lib_latent_fwd_kernel) and eval_step, and marginal_llk's library terms in both scoring forms: there the rate
  cannot be pinned, so the likelihood of a draw is the call's own second output -- the same in every draw with out*/W = 0 and the
  clip at 1e-30 -- and the check is on mllk - llk = log-mean-exp of the latent terms, with 4 u |llk| for that difference; all three priors, resident rows
  and host rows.  Under the prior (7, 1e-6) the locations +-1e19 are dropped points (the weight is -5e43 in every draw): held to "-inf or a finite
  float, no NaN" -- the all--inf log-sum-exp."""
  from sisua_amd import engine as eng
  from sisua_amd.config import ModelConfig
  B, D = 7, 4
  ids0 = np.arange(B, dtype=np.int32)
  cfg = ModelConfig(model="scvi", n_genes=G, likelihood="nbd", enc_units=(32,), dec_units=(32,), encl_units=(16,), latent_dim=D, lr=0.0, dropout_enc=0.0,
                    dropout_dec=0.0, clip_library=1e-30)
  lib = np.concatenate([np.tile(np.array([p], np.float32), (B, 1)) for p in T.LIB_PRIORS])
  mus, raws = T.kl_grid()
  eps_l = np.array(T.EPS_AXIS, np.float32)[np.arange(B) % 7]
  t = Tally(f"scvi {'fused' if fused else 'separate'}")
  e = None
  try:
    e = Engine(cfg, max_batch=8)
    e.set_flag("scvi_fused", fused)
    zero = {k: np.zeros(e.shapes[k], np.float32) for k in e.shapes if k in ("latl/W", "lat/W", "lat/b") or (k.startswith("out") and k.endswith("/W"))}
    e.set_params(zero)
    e.upload(counts[:3 * B], library=lib)
    bl = np.zeros(e.shapes["latl/b"], np.float32)
    for m_, r_ in zip(mus, raws):
      bl.reshape(-1)[:2] = (m_, r_)
      e.set_params({"latl/b": bl})
      for k, (mp_, vp_) in enumerate(T.LIB_PRIORS):
        mp_, vp_ = np.float32(mp_), np.float32(vp_)
        label = f"mu {float(m_):g} raw {float(r_):g} prior ({float(mp_):g}, {float(vp_):g})"
        ids = ids0 + k * B
        e.set_noise(STREAM_EPS_Z, np.zeros((B, D), np.float32))
        e.set_noise(STREAM_EPS_L, eps_l.reshape(B, 1))
        ev = e.eval_step(ids)
        f = e.forward(row_ids=ids, want_x_params=False)
        # the training step at the noise 0: l = mu exactly, outside (0, 1e-30) at every grid location (sigma eps of a raw scale of -87 is not)
        e.set_noise(STREAM_EPS_L, np.zeros((B, 1), np.float32))
        m = e.train_step(ids)
        g = e.get_params(1)["latl/b"].reshape(-1)[:2].copy()
        ref, bd = T.lib_terms(m_, r_, eps_l.astype(np.float64), mp_, vp_), T.lib_bounds(m_, r_, eps_l.astype(np.float64), mp_, vp_)
        one, bone = T.lib_terms(m_, r_, 0.0, mp_, vp_), T.lib_bounds(m_, r_, 0.0, mp_, vp_)
        t.held("l_scale", f["l_scale"], one["sigma"], bone["sigma"], label)
        t.held("l_sample", f["l_sample"], ref["z"], bd["z"], label)
        klb = bone["kl"] + (N_ADD_KL + 1.0) * U * abs(one["kl"]) + T.F32_MIN
        t.held("train_step kl_l", m["kl_l"], one["kl"], klb, label, cells=B)
        t.held("eval_step kl_l", ev["kl_l"], one["kl"], klb, label, cells=B)
        for name, got, key in (("d latl/b mu", g[0], "dmu"), ("d latl/b raw", g[1], "draw")):
          t.held(name, got, one[key], bone[key] + (B + 12.0) * U * abs(one[key]) + (B + 4.0) * T.F32_MIN, label)
      assert np.array_equal(_bits(e.get_params(0)["latl/b"]), _bits(bl))
    # the library terms of the importance weight: one axis at a time (the raw-scale axis and the location axis) under every prior, the resident
    # rows and the same cells as host rows with their library prior (their cell ids, and so their draws, are 0 .. B - 1)
    e.clear_noise()
    amu, araw, _ = T.axis_grid()
    made = {}

    def noise(ids):          # the device's own draws of the cells `ids`: [S, B, D] of the latent, [S, B] of the library latent
      key = int(ids[0])
      if key not in made:
        made[key] = (np.stack([eng.k_noise(cfg.seed, STREAM_EPS_Z, 0, ids, D, sample=s)[1] for s in range(S_SCORE)]).astype(np.float64),
                     np.stack([eng.k_noise(cfg.seed, STREAM_EPS_L, 0, ids, 1, sample=s)[1][:, 0] for s in range(S_SCORE)]).astype(np.float64))
      return made[key]
    for m_, r_ in zip(amu, araw):
      bl.reshape(-1)[:2] = (m_, r_)
      e.set_params({"latl/b": bl})
      for k in range(len(T.LIB_PRIORS)):
        mp_, vp_ = (np.float32(v) for v in T.LIB_PRIORS[k])
        label = f"mu {float(m_):g} raw {float(r_):g} prior ({float(mp_):g}, {float(vp_):g})"
        for rows_name, ids in (("resident rows", ids0 + k * B), ("host rows", ids0)):
          ez, el = noise(ids)
          wz, bz = T.diag_terms(0.0, 0.0, ez), T.diag_bounds(0.0, 0.0, ez)
          wl, bwl = T.lib_terms(m_, r_, el, mp_, vp_), T.lib_bounds(m_, r_, el, mp_, vp_)
          sizes = (0.5 * wz["z"] ** 2 + 0.5 * ez ** 2).sum(-1) + np.abs(wl["w"])
          lw = wz["w"].sum(-1) + wl["w"]
          for stacked in (True, False):
            e.set_flag("stacked_scoring", stacked)
            if rows_name == "resident rows":
              mllk, llk = e.marginal_llk(row_ids=ids, n_samples=S_SCORE)
            else:
              mllk, llk = e.marginal_llk(x=counts[k * B:(k + 1) * B], library=lib[k * B:(k + 1) * B], n_samples=S_SCORE)
            with np.errstate(invalid="ignore", over="ignore"):
              b_draw = bz["w"].sum(-1) + bwl["w"] + (N_ADD_W + 4.0) * U * sizes + U * np.abs(lw) + 4.0 * U * np.abs(llk.astype(np.float64))[None, :]
              ref = _lme(lw)
              bound = b_draw.max(0) + 2.0 * U * (np.abs(ref) + np.abs(llk)) + (S_SCORE + 10.0) * U * (1.0 + np.log(S_SCORE))
            t.held(f"marginal_llk - llk ({'stacked' if stacked else 'per draw'}, {rows_name})", mllk.astype(np.float64) - llk.astype(np.float64), ref, bound, label)
  finally:
    if e is not None:
      e.close()
  t.done()


# ---- the full-covariance head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", T.TRIL_DIMS)
def test_tril_head(Engine, counts, D):
  """latent_tril: lat/W = 0, the 1 + D planes' biases = tril_case (every diagonal raw one raw-scale value, the strict lower triangle from
  {0, +-1e-3, +-30}, the locations and the noise cycling); dec0/W = 0.  forward()'s factor and z_sample, metrics['kl'] of both steps, and lat/b's
  gradient elementwise (location, diagonal, strict lower triangle; the inert upper triangle exactly 0)."""
  from sisua_amd.config import ModelConfig
  B = 7
  ids = np.arange(B, dtype=np.int32)
  cfg = ModelConfig(model="vae", n_genes=G, likelihood="nb", enc_units=(32,), dec_units=(32,), latent_dim=D, lr=0.0, dropout_enc=0.0, dropout_dec=0.0,
                    latent_tril=True)
  t = Tally(f"tril D {D}")
  e = None
  try:
    e = Engine(cfg, max_batch=8)
    W0 = np.zeros(e.shapes["lat/W"], np.float32)
    e.set_params({"dec0/W": np.zeros(e.shapes["dec0/W"], np.float32), "lat/W": W0})
    e.upload(counts)
    for s, dr in enumerate(T.RAW_AXIS):
      mu, raw, eps = T.tril_case(D, dr, T.TRIL_LOWER, seed=s)
      label = f"diagonal raw {dr:g}"
      b = np.concatenate([mu, raw.reshape(-1)]).astype(np.float32)
      e.set_params({"lat/b": b})
      e.set_noise(STREAM_EPS_Z, np.tile(eps, (B, 1)))
      ev = e.eval_step(ids)
      f = e.forward(row_ids=ids, want_x_params=False)
      m = e.train_step(ids)
      g = e.get_params(1)["lat/b"].copy()
      ref, bd = T.tril_terms(mu, raw, eps), T.tril_bounds(mu, raw, eps)
      t.held("z_sample", f["z_sample"], ref["z"][None, :], bd["z"][None, :], label)
      assert "scale_tril" in f, label
      t.held("factor diagonal", np.einsum("bii->bi", f["scale_tril"]), ref["diag"][None, :], bd["diag"][None, :], label)
      klb = bd["kl"] + N_ADD_KL * U * np.abs(ref["kl_rows"]).sum() + U * abs(ref["kl"]) + D * T.F32_MIN
      t.held("train_step kl", m["kl"], ref["kl"], klb, label, cells=B)
      t.held("eval_step kl", ev["kl"], ref["kl"], klb, label, cells=B)
      scale = lambda v, bv: bv + (B + 12.0) * U * np.abs(v) + (B + 4.0) * T.F32_MIN
      t.held("d lat/b mu", g[:D], ref["dmu"], scale(ref["dmu"], bd["dmu"]), label)
      gr = g[D:].reshape(D, D)
      t.held("d lat/b factor", np.tril(gr), ref["draw"], scale(ref["draw"], bd["draw"]), label)
      assert np.array_equal(gr[np.triu_indices(D, 1)], np.zeros(D * (D - 1) // 2, np.float32)), label
      p = e.get_params(0)
      assert np.array_equal(_bits(p["lat/W"]), _bits(W0)) and np.array_equal(_bits(p["lat/b"]), _bits(b)), label
  finally:
    if e is not None:
      e.close()
  t.done()
