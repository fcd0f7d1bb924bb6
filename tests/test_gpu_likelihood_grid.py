"""Every kernel family that evaluates count_elem / count_elem_vec (sisua_amd/csrc/smx_loss.h), held to the float64 gradients of
tests/likelihood_grad_ref.py on the saturated edge grid of tests/plane_stat_ref.py, element by element and inside bounds derived from
the kernels' own formulas (the two modules' docstrings have the tables).  No tolerance here was chosen after looking at a kernel's
output.  Every test prints the worst error / bound and where it occurred; DESIGN.md 4s records them as read on an MI355X.

THE SUMMATION BOUND of a sum over genes: |got - ref| <= sum_g b_g + gamma sum_g |s_g| + u |ref| + G 2^-126, b_g = plane_stat_ref's
logprob_elem_bound, without its lgammaf(x + 1) term where the count constant is summed in double precision; s_g the float32 summands
(the element values without the count constant); gamma = (n_add + 8) u, n_add the longest chain of float32 additions in the kernel's
reduction; u |ref| is the rounding of the result to float32, G 2^-126 the underflow of G summands (the 'nbd' element at the
pre-activations (-60, -60) and a zero count is -1.3e-44).
  standalone kernel   count_loss_kernel at one gene per lane (below 400 000 elements: loss_vec): a lane's accumulator takes its one
                      element (0 + v, exact), wave_sum's six butterfly steps, one partial per wave; smx_k_count_llk adds the partials
                      and -lgamma(x + 1) in double.  n_add = 6; two genes per lane (from 400 000 elements): 7.
  fused head          N_ADD_FUSED beside test_fused_head_on_the_grid: 10.
  training step       N_ADD_STEP, derived in test_training_step_on_the_grid's docstring: 29.
  scoring             N_ADD_DRAW and what the draws add, derived in test_scoring_on_the_grid's docstring: 13, 23.

EVERY LAUNCHER BRANCH that evaluates count_elem / count_elem_vec and is reachable with <= 8000 genes and <= 260 cells, and what reaches it:
  smx_loss.hip    count_loss_kernel<LK, DIRECT, BWD = 1, VEC = 1> (launch_loss_t), the per-wave queue form, float counts
                    nb, zinb, nbd, zinbd, bernoulli, normal; DIRECT 0 / 1 for nbd, zinbd     test_standalone_kernel_one_point_per_row, _ragged_rows
                  the same inside a training step (head_loss off; 'bernoulli' always)          test_training_step_on_the_grid[*-b128_head_loss_0], [bernoulli-*]
                  VEC = 2 (from 400 000 elements: 260 cells x 1998 genes are inside the limits)  test_standalone_kernel_two_genes_per_lane
                  VEC = 4 (from 8 M elements: beyond the limits)                                 not reachable: test_count_llk_wide_access_forms, ordinary data
                  BWD = 0 (scoring draw by draw)                                                 test_scoring_on_the_grid[*-per_draw]
                  likelihood -2 (a diagnostic, not a result)                                     NOT REACHED
                  label_loss_kernel's count_elem calls                                           tests/test_gpu_label_heads.py (smx_k_label_loss; tests/label_heads_ref.py)
  smx_headloss.hip  out_head_loss_kernel<LK, U16 = 0, EPI = 1, NW = 8, 128, B3 = 0 / 1>, count_elem_vec through the per-wave queue (QUEUE: EPI == 1, NW >= 4)
                    nb, zinb, nbd, zinbd, normal; B3 by the bf16x3 flag                         test_training_step_on_the_grid[*-b128_bf16x3_0 / _1, b4, b130, ...]
                  U16 = 1 (the uint16 store in a training step)                                 test_training_step_on_the_grid[*-b128_u16]
                  EPI = 2, NW = 2 (scoring over stacked draws, knob score_head_wide; no queue:    test_scoring_on_the_grid[*-stacked_wide_head]
                    the straight-line lgamma_digamma_diff_vec with its wave-uniform `rare` test)
  smx_headfused.hip  head_fused kernel, count_elem_vec<LK, 0, 4> with the queue inside the operand image, u16 on and off
                    nb, zinb, nbd, zinbd at 128, 37 and 1 cells                                 test_fused_head_on_the_grid
                  129 .. 256 cells                                                              NOT REACHED
  smx_score.hip   score_tile_llk (count_elem_vec<LK, 0, 8>) in score_head_kernel (tile) and score_walk_kernel (walk), the queue and -- knob
                  no_score_queue -- the straight-line lgamma_digamma_diff_vec                   test_scoring_on_the_grid[*-stacked, *-stacked_no_queue] (walk: forced)
                  count_loss_kernel BWD = 0 (the draw-by-draw form; 'bernoulli' always)         test_scoring_on_the_grid[*-per_draw, bernoulli-*]
                  the scvi form count_elem_vec<LK, 1, 4>                                        the instance held in tests/test_gpu_scvi_head.py (smx_scvi.hip); this launch: not reached
  smx_scvi.hip    count_elem_vec<LK, 1, 4>                                                      tests/test_gpu_scvi_head.py (the rate pinned from raw_0 and l); forward planes also: test_gpu_plane_stats
  smx_predict.hip plane_logprob (count_elem<LK, DIRECT>)                                        tests/test_gpu_plane_stats.py
"""
import numpy as np
import pytest

from tests import likelihood_grad_ref as L

pytestmark = pytest.mark.gpu

U = L.U


@pytest.fixture(scope="module")
def eng():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd import engine
  return engine


def _report(label, err, bound):
  ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))      # (a NaN stays a NaN: np.argmax finds it, the checks below fail on it)
  at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
  print(f"{label}: worst error / bound {float(ratio.max()):.3f} at {tuple(int(i) for i in at)}")
  return ratio, at


def _outside(err, bound):
  """elements outside their bound; a NaN error -- a NaN from the kernel -- is outside"""
  return ~(err <= bound)


_count_const, row_sum_bound = L.count_const, L.row_sum_bound          # (shared with tests/test_gpu_latent_grid.py: they live in the reference module)


def _check_grads(label, kind, direct, grads, x, planes, keep):
  """every gradient component elementwise inside grad_elem_bound (x, planes and keep broadcast against the gradients); returns the failures
  (all components are looked at first)"""
  ref, bound = L.grad_elem(kind, x, planes, direct), L.grad_elem_bound(kind, x, planes, direct)
  ref, bound = np.broadcast_to(ref, (3,) + grads[0].shape), np.broadcast_to(bound, (3,) + grads[0].shape)
  keep = np.broadcast_to(keep, grads[0].shape)
  failures = []
  for c in range(len(planes)):
    got = grads[c]
    assert got.dtype == np.float32
    assert not (np.isnan(got) & keep).any(), (label, c)
    err = np.where(keep, np.abs(got.astype(np.float64) - ref[c]), 0.0)
    ratio, at = _report(f"{label} d{c}", err, bound[c])
    bad = _outside(err, bound[c])
    if bad.any():
      failures.append((f"d{c}", int(bad.sum()), float(ratio.max()), [float(np.broadcast_to(p, got.shape)[at]) for p in planes],
                       float(np.broadcast_to(x, got.shape)[at]), float(got[at]), float(ref[c][at])))
      print(f"    OUTSIDE THE BOUND (component, elements, worst ratio, planes, x, got, reference) {failures[-1]}")
  return failures


# ---- a. the standalone kernel, unclipped -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,direct", L.ALL)
def test_standalone_kernel_one_point_per_row(eng, kind, direct):
  """smx_k_count_llk on the whole grid x the seven counts, every row ONE element repeated 64 times (the layout of
  test_count_llk_saturated_gate: a row sum is 64 times one element and cannot hide it): the gradients elementwise inside
  grad_elem_bound, the row sums inside the summation bound"""
  x, planes, keep = L.grid_elements(kind, direct)
  n = x.size
  xe = np.ascontiguousarray(np.broadcast_to(x.reshape(n, 1), (n, 64)))
  pe = [np.ascontiguousarray(np.broadcast_to(np.broadcast_to(p, x.shape).reshape(n, 1), (n, 64))) for p in planes]
  assert n * 64 < 400000          # (one gene per lane: the docstring's n_add)
  llk, grads = eng.k_count_llk(kind, xe, np.stack(pe), direct=direct)
  x1, p1 = x.reshape(n, 1), [np.broadcast_to(p, x.shape).reshape(n, 1) for p in planes]
  failures = _check_grads(f"{kind} direct={direct}", kind, direct, grads, x1, p1, keep.reshape(n, 1))
  for c in range(len(planes)):
    assert (grads[c] == grads[c][:, :1]).all()          # (one element, 64 lanes: the same bits)
  ref, bound = row_sum_bound(kind, x1, p1, 6, direct, repeat=64)
  rows = keep.reshape(n)
  err = np.where(rows, np.abs(llk.astype(np.float64) - ref), 0.0)
  ratio, at = _report(f"{kind} direct={direct} row sums", err, bound)
  if _outside(err, bound).any():
    failures.append(("llk", int(_outside(err, bound).sum()), float(ratio.max()), [float(p[at[0], 0]) for p in pe], float(xe[at[0], 0]), float(llk[at]), float(ref[at])))
  assert not failures, (kind, direct, failures)


@pytest.mark.parametrize("order", ["point_major", "count_major"])
@pytest.mark.parametrize("kind,direct", L.ALL)
def test_standalone_kernel_ragged_rows(eng, kind, direct, order):
  """The same elements laid end to end in rows of 201 genes (no multiple of 4; three full waves and a ragged one per row).  Point major:
  the seven counts cycle along a row, every wave holds zero counts, small counts and counts beyond 8 side by side (the per-entry branch
  of the queue's drain, both branches of lgamma_digamma_diff in one wave).  Count major: whole waves of zeros (an empty queue), whole
  waves of one small count, whole waves of 10738.  The last row is filled up with moderate points at a zero count."""
  x, planes, keep = L.grid_elements(kind, direct)
  G = 201
  flat = (lambda a: np.broadcast_to(a, x.shape).reshape(-1)) if order == "point_major" else (lambda a: np.broadcast_to(a, x.shape).T.reshape(-1))
  n = x.size
  pad = (-n) % G
  fill = [np.float32(v) for v in L.MODERATE[kind][0]]
  if direct:
    fill[:2] = [np.float32(L.softplus(fill[0])), np.float32(L.softplus(fill[1] + L.SOFTPLUS_INV_1))]
  xe = np.concatenate([flat(x), np.zeros(pad, np.float32)]).reshape(-1, G)
  pe = [np.concatenate([flat(p), np.full(pad, f, np.float32)]).reshape(-1, G) for p, f in zip(planes, fill)]
  ke = np.concatenate([flat(keep), np.ones(pad, bool)]).reshape(-1, G)
  assert xe.size < 400000 and G % 4
  llk, grads = eng.k_count_llk(kind, xe, np.stack(pe), direct=direct)
  failures = _check_grads(f"{kind} direct={direct} {order}", kind, direct, grads, xe, pe, ke)
  ref, bound = row_sum_bound(kind, xe, pe, 6, direct)
  rows = ke.all(axis=1)
  err = np.where(rows, np.abs(llk.astype(np.float64) - ref), 0.0)
  ratio, at = _report(f"{kind} direct={direct} {order} row sums", err, bound)
  if _outside(err, bound).any():
    failures.append(("llk", int(_outside(err, bound).sum()), float(ratio.max()), int(at[0]), float(llk[at]), float(ref[at])))
  assert not failures, (kind, direct, order, failures)


@pytest.mark.parametrize("kind,direct", L.ALL)
def test_standalone_kernel_two_genes_per_lane(eng, kind, direct):
  """count_loss_kernel's 8-byte access form (VEC = 2: from 400 000 elements, loss_vec): the grid's elements, point major, repeated end to
  end over 260 cells x 1998 genes (519 480 elements; no multiple of 4, the padded row of 2016 leaves a lane pair half in range).  The
  reference is computed once per (point, count) and gathered.  n_add = 7: a lane's accumulator takes its first element exactly, adds
  the second (1), wave_sum's six steps; smx_k_count_llk adds the partials and the count constant in double."""
  x, planes, keep = L.grid_elements(kind, direct)
  B, G = 260, 1998
  assert 400000 <= B * 2016 < 8000000
  idx = (np.arange(B * G) % x.size).reshape(B, G)
  flat = lambda a: np.ascontiguousarray(np.broadcast_to(a, x.shape).reshape(-1)[idx])
  xe, pe = flat(x), [flat(p) for p in planes]
  llk, grads = eng.k_count_llk(kind, xe, np.stack(pe), direct=direct)
  ref, bound = L.grad_elem(kind, x, planes, direct), L.grad_elem_bound(kind, x, planes, direct)
  failures = []
  for c in range(len(planes)):
    err = np.where(flat(keep), np.abs(grads[c].astype(np.float64) - flat(ref[c])), 0.0)
    ratio, at = _report(f"{kind} direct={direct} two genes per lane d{c}", err, flat(bound[c]))
    bad = _outside(err, flat(bound[c]))
    if bad.any():
      failures.append((f"d{c}", int(bad.sum()), float(ratio.max()), [float(p[at]) for p in pe], float(xe[at]), float(grads[c][at]), float(flat(ref[c])[at])))
      print(f"    OUTSIDE THE BOUND {failures[-1]}")
  v = L.log_prob_elem(kind, x, planes, direct)
  b = L.logprob_elem_bound(kind, x, planes, direct, double_const=True)
  ref_l = flat(v).sum(axis=1)
  bound_l = flat(b).sum(axis=1) + (7 + 8.0) * U * flat(np.abs(v + _count_const(kind, x))).sum(axis=1) + U * np.abs(ref_l) + G * L.F32_MIN
  err = np.where(flat(keep).all(axis=1), np.abs(llk.astype(np.float64) - ref_l), 0.0)
  ratio, at = _report(f"{kind} direct={direct} two genes per lane row sums", err, bound_l)
  if _outside(err, bound_l).any():
    failures.append(("llk", int(_outside(err, bound_l).sum()), float(ratio.max()), int(at[0]), float(llk[at]), float(ref_l[at])))
  assert not failures, (kind, direct, failures)


# ---- c. the narrow-panel training step through Engine ------------------------------------------------------------------------------
G_STEP = L.G_GRID
_NET = dict(n_genes=G_STEP, enc_units=(32,), dec_units=(32,), latent_dim=6, lr=0.0)
STEP_KINDS = {"nb": {}, "zinb": {}, "nbd": {}, "zinbd": {}, "bernoulli": {}, "normal": dict(log_norm=False)}
N_ADD_STEP = 29
# (cells, flags, tuning knobs, dW-late expected -- of the four count kinds; None: the form taken is printed): a ragged 4-cell minibatch, the
# path beyond 128 cells, at 128 cells the dW-late form (bf16x3 on) and its knob, and each switch that changes which kernel evaluates the
# likelihood or forms db: head_loss (out_head_loss_kernel | product + count_loss_kernel), head_bwd (the wide
# direct-operand backward | the grouped products), bf16x3 (the head's product form; on: the dW-late carrier).  The other flags of smx_set_flag
# (front, bwd_front, wgrad, act_epilogue, twin, label_ride, head_sweep, scvi_fused, opt_shard) act below the head or on other models; head_fused
# needs 4096 genes: test_fused_head_on_the_grid.
STEP_VARIANTS = {
    "b4": (4, {}, {}, None),
    "b4_bf16x3_1": (4, {"bf16x3": True}, {}, None),
    "b128_no_dw_late": (128, {"bf16x3": True}, {"no_dw_late": 1}, False),
    "b130": (130, {}, {}, None),
    "b128": (128, {}, {}, None),
    "b128_head_loss_0": (128, {"head_loss": False}, {}, None),
    "b128_head_loss_1": (128, {"head_loss": True}, {}, None),
    "b128_head_bwd_0": (128, {"head_bwd": False}, {}, None),
    "b128_head_bwd_1": (128, {"head_bwd": True}, {}, None),
    "b128_bf16x3_0": (128, {"bf16x3": False}, {}, False),
    "b128_bf16x3_1": (128, {"bf16x3": True}, {}, True),
    "b128_u16": (128, {}, {}, None),          # the counts resident as uint16 (not 'normal': its targets are reals)
}
STEP_CASES = [(k, v) for k in STEP_KINDS for v in STEP_VARIANTS if not (k == "normal" and v == "b128_u16")]


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


@pytest.mark.parametrize("kind,variant", STEP_CASES)
def test_training_step_on_the_grid(Engine, kind, variant):
  """out/W = 0, out/b = the grid, lr = 0: gene g of every cell sits at grid point g in every step.  One step per target row of
  plane_stat_ref.targets, every cell of the minibatch that row: the gradient of out/b is then B terms d s, d one element's gradient and
  s = -fl(1 / B) the step's grad_scale (smx_forward.hip: -inv_gb; the gradient buffer is read before clipnorm -- the optimiser's sweep
  forms the clip factor per tensor and applies it on the fly, reading the gradients through a const pointer: adam_sweep_body), held
  ELEMENTWISE to -grad_elem inside  bound_d + (B + 12) u |d| + (B + 4) 2^-126:  the elements' bounds (B s = 1), s's and the product's
  roundings 2, at most B additions of the B equal terms (the issue's B u sum |terms|), 2 for a bf16 x 3 product by 1.0, 8 of slack as in
  gamma.  nllk_x is held to -sum_g log_prob_elem inside the summation bound with n_add = 29 -- out_head_loss_kernel: half_wave_sum's 5
  steps per (cell, 32-gene tile), or count_loss_kernel: wave_sum's 6 per wave; then metrics_body's flat sweep of the B n_chunks partials:
  ceil(B n_chunks / 2048) <= 3 rounds here, at most 8 remainder additions, the 3-level tree of the eight partial sums, the cell's count
  constant (float32 of a double sum: u |lgamma sum| more), wave_sum 6, the four waves 2: 6 + 3 + 8 + 3 + 1 + 6 + 2.  After the steps out/W
  and out/b are what was set, bit for bit."""
  from sisua_amd import _hip
  from sisua_amd.config import ModelConfig
  B, flags, knobs, late = STEP_VARIANTS[variant]
  bias, n_pts = L.grad_bias_grid(kind, G_STEP)
  t = L.targets(kind, G_STEP)
  planes = list(bias)
  k = len(planes)
  e = None
  try:
    for name, v in knobs.items():
      _hip.set_tuning(name, v)
    e = Engine(ModelConfig(model="vae", likelihood=kind, **_NET, **STEP_KINDS[kind]), max_batch=max(B, 4))
    for name, v in flags.items():
      e.set_flag(name, v)
    W0 = np.zeros(e.shapes["out/W"], np.float32)
    e.set_params({"out/W": W0, "out/b": bias.reshape(-1)})
    e.upload(np.repeat(t, B, axis=0), storage="u16" if variant.endswith("u16") else "f32")
    failures = []
    for r in range(len(t)):
      m = e.train_step(np.arange(r * B, (r + 1) * B, dtype=np.int32))
      # ('normal': the grid's d1 reaches 4e33, the sum of squares of the step's gradient is no float32 and the step says so)
      assert m["nan_flag"] == 0 or kind == "normal", (kind, variant, r)
      if r == 0:
        print(f"{kind} {variant}: head_dw_late {e.head_dw_late()}, nan_flag {m['nan_flag']}")
      if late is not None and kind in ("nb", "zinb", "nbd", "zinbd"):
        assert e.head_dw_late() == late, (kind, variant)
      keep = L.grad_in_range(kind, t[r], planes)
      ref, bound_d = L.grad_elem(kind, t[r], planes), L.grad_elem_bound(kind, t[r], planes)
      got = e.get_params(1)["out/b"].reshape(k, G_STEP)
      for c in range(k):
        bound = bound_d[c] + (B + 12.0) * U * np.abs(ref[c]) + (B + 4.0) * L.F32_MIN
        err = np.where(keep, np.abs(got[c].astype(np.float64) + ref[c]), 0.0)
        ratio, at = _report(f"{kind} {variant} target row {r} d out/b plane {c}", err, bound)
        if _outside(err, bound).any():
          failures.append((r, f"d{c}", int(_outside(err, bound).sum()), float(ratio.max()), [float(p[at]) for p in planes], float(t[r][at]), float(got[c][at]), float(-ref[c][at])))
          print(f"    OUTSIDE THE BOUND {failures[-1]}")
      ref_l, bound_l = row_sum_bound(kind, t[r], planes, N_ADD_STEP)
      bound_l += 2.0 * U * _count_const(kind, t[r]).sum()
      err = abs(float(m["nllk_x"]) + ref_l)
      print(f"{kind} {variant} target row {r} nllk_x: error / bound {err / bound_l:.3f} (bound / |ref| {bound_l / abs(ref_l):.2e})")
      if not err <= bound_l:
        failures.append((r, "nllk_x", float(err / bound_l), float(m["nllk_x"]), float(-ref_l)))
    p = e.get_params(0)
    assert (_bits(p["out/W"]) == _bits(W0)).all() and (_bits(p["out/b"]) == _bits(bias.reshape(-1))).all()
  finally:
    if e is not None:
      e.close()
    for name in knobs:
      _hip.set_tuning(name, 0)
  assert not failures, (kind, variant, failures)


# ---- b. the fused head at wide panels ----------------------------------------------------------------------------------------------
G_FUSED = 4100          # the smallest ragged width from 4096 on; it holds every kind's grid (648 points at the most), moderate filler behind
N_ADD_FUSED = 10        # smx_k_head_fused at 4128 padded genes: 258 units of 16 genes, 129 workgroups of 2 units; a lane adds its 4 elements
                        # per unit into lsum (8 additions), two __shfl_xor steps (16, 32) join the lane groups; smx_k_head_fused adds the 129
                        # partials per cell and -lgamma(x + 1) in double


@pytest.fixture(scope="module")
def fused_ref():
  """per kind: the bias, and reference / bounds of every gene at each of the seven counts [7, G] -- computed once, gathered per case"""
  made = {}

  def get(kind):
    if kind not in made:
      bias, n_pts = L.grad_bias_grid(kind, G_FUSED)
      planes = list(bias)
      x7 = np.broadcast_to(L.counts_for(kind)[:, None], (7, G_FUSED))
      v = L.log_prob_elem(kind, x7, planes)
      made[kind] = dict(bias=bias, keep=L.grad_in_range(kind, x7, planes), g=L.grad_elem(kind, x7, planes), gb=L.grad_elem_bound(kind, x7, planes),
                        v=v, vb=L.logprob_elem_bound(kind, x7, planes, double_const=True), s=np.abs(v + _count_const(kind, x7)))
    return made[kind]
  return get


@pytest.mark.parametrize("u16", [False, True])
@pytest.mark.parametrize("B", [128, 37, 1])
@pytest.mark.parametrize("kind", ["nb", "zinb", "nbd", "zinbd"])
def test_fused_head_on_the_grid(eng, fused_ref, kind, B, u16):
  """smx_k_head_fused with W = 0, bias = the grid, d = the first B rows of the 128 x 128 identity, x[b][g] = CYCLE[(b + g) % 7] (every
  gene meets every count; rows 64-127 -- waves 4-7 -- and lanes 48-63 carry every count class): dW[b][k][g] = grad_scale d llk(x[b][g],
  grid[g]), ONE element per cell row and gene, held inside |grad_scale| bound_d + 3 u |value| + 4 2^-126 (the product by grad_scale 1,
  the bf16 x 3 product by 1.0 at the issue's 2 u, the underflow of the three split terms); rows h >= B and d d exactly 0; db against the
  float64 column sums inside the sum of the elements' bounds + B u sum |terms|; llk[b] inside the summation bound, n_add = 10."""
  r = fused_ref(kind)
  k = r["bias"].shape[0]
  scale = -1.0 / 128
  cyc = L.counts_for(kind)
  idx = (np.arange(B)[:, None] + np.arange(G_FUSED)[None, :]) % 7
  x = cyc[idx]
  cols = np.arange(G_FUSED)[None, :]
  got = eng.k_head_fused(kind, x, np.eye(128, dtype=np.float32)[:B], np.zeros((128, k, G_FUSED), np.float32), r["bias"], grad_scale=scale, u16=u16)
  keep = r["keep"][idx, cols]
  failures = []
  assert (got["dd"] == 0).all() and (got["dW"][B:] == 0).all()
  ref_db, bound_db = np.zeros((k, G_FUSED)), np.zeros((k, G_FUSED))
  for c in range(k):
    ref = scale * r["g"][c][idx, cols]
    bound = abs(scale) * r["gb"][c][idx, cols] + 3.0 * U * np.abs(ref) + 4.0 * L.F32_MIN
    err = np.where(keep, np.abs(got["dW"][:B, c].astype(np.float64) - ref), 0.0)
    ratio, at = _report(f"{kind} B={B} u16={u16} dW plane {c}", err, bound)
    if _outside(err, bound).any():
      failures.append((f"dW{c}", int(_outside(err, bound).sum()), float(ratio.max()), [float(p[at[1]]) for p in r["bias"]], float(x[at]), float(got["dW"][at[0], c, at[1]]), float(ref[at])))
      print(f"    OUTSIDE THE BOUND {failures[-1]}")
    ref_db[c], bound_db[c] = ref.sum(axis=0), bound.sum(axis=0) + B * U * np.abs(ref).sum(axis=0)
  col_ok = keep.all(axis=0)
  err = np.where(col_ok[None], np.abs(got["db"].astype(np.float64) - ref_db), 0.0)
  ratio, at = _report(f"{kind} B={B} u16={u16} db", err, bound_db)
  if _outside(err, bound_db).any():
    failures.append(("db", int(_outside(err, bound_db).sum()), float(ratio.max()), at, float(got["db"][at]), float(ref_db[at])))
  ref_l = r["v"][idx, cols].sum(axis=1)
  bound_l = r["vb"][idx, cols].sum(axis=1) + (N_ADD_FUSED + 8.0) * U * r["s"][idx, cols].sum(axis=1) + U * np.abs(ref_l) + G_FUSED * L.F32_MIN
  err = np.abs(got["llk"].astype(np.float64) - ref_l)
  ratio, at = _report(f"{kind} B={B} u16={u16} llk", err, bound_l)
  if _outside(err, bound_l).any():
    failures.append(("llk", int(_outside(err, bound_l).sum()), float(ratio.max()), at, float(got["llk"][at]), float(ref_l[at])))
  assert not failures, (kind, B, u16, failures)


# ---- d. scoring ------------------------------------------------------------------------------------------------------------------------
S_SCORE = 3
N_ADD_DRAW = 13
SCORE_FORMS = {   # (stacked_scoring, tuning knobs)
    "stacked": (True, {}),
    "stacked_no_queue": (True, {"no_score_queue": 1}),
    "stacked_wide_head": (True, {"score_head_wide": 1}),
    "per_draw": (False, {}),
    "per_draw_no_queue": (False, {"no_score_queue": 1}),
}


_draw_bound = L.draw_bound


@pytest.mark.parametrize("form", list(SCORE_FORMS))
@pytest.mark.parametrize("kind", list(STEP_KINDS))
def test_scoring_on_the_grid(Engine, kind, form):
  """The engines of the training-step test (out/W = 0, out/b = the grid): every draw of every cell decodes to the grid, so the scores are
  deterministic.  The five target rows, as the resident input rows and as a separate target matrix over another input:
    eval_step's nllk_x against -mean_b sum_g log_prob_elem (n_add = 29: the training step's forward kernels and metrics_body);
    marginal_llk's second output (the mean over the draws of log p(x | z)) against sum_g log_prob_elem;
    both columns of score_llk (the output distribution; its count part without the gate) against sum_g log_prob_elem(count_only).
  ONE DRAW of one cell, n_add = 13.  Stacked: score_tile_llk's halving exchange over a tile's 32 columns is 5 additions (16, 8, 4, 2, 1) --
  out_head_loss_kernel<EPI = 2>'s half_wave_sum (knob score_head_wide) the same 5 --; iw_stack_kernel: a lane takes ONE of the 33 partials
  (n_chunks <= 64: no addition), wave_sum 6, the count constant 1: 12.  Draw by draw: count_loss_kernel at one gene per lane, wave_sum 6;
  iw_accum_kernel: a lane takes one of the 20 partials (0 + v), wave_sum 6, the constant 1: 13.
  OVER THE DRAWS.  marginal_llk: the S = 3 values are added (iw_stack: one per lane, wave_sum 6; iw_accum: S - 1) and divided by S:
  n_add = 13 + 6 + S + 1 = 23 on the same sizes.  score_llk: run_max + logf(run_sum) - logf(S); the S weights lie within the draw's
  bound of each other, expf of their differences from the maximum is 1 to 2 u each, their sum S to (S + 2) u relative, logf 2 u |log S|
  + (S + 4) u absolute, logf(S) again 2 u |log S|, two additions of sizes |L| + log S: bound_draw + 2 u |L| + (S + 10) u (1 + log S).
  Knob no_score_queue: the straight-line form lgamma_digamma_diff_vec with its wave-uniform `rare` test instead of the per-wave queue --
  the SAME BITS as with the queue, asserted.  The walk form of the scoring head (knob score_walk 1, 2: forced) gives the bits of the tile form
  (0), as tests/test_gpu_step.py asserts on ordinary data."""
  from sisua_amd import _hip
  from sisua_amd.config import ModelConfig
  stacked, knobs = SCORE_FORMS[form]
  bias, n_pts = L.grad_bias_grid(kind, G_STEP)
  planes = list(bias)
  t = L.targets(kind, G_STEP)
  other = np.ascontiguousarray(t[::-1])
  rows = np.arange(len(t), dtype=np.int32)
  zi = L.is_zi(kind)
  e, failures = None, []

  def held(label, got, ref, bound):
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    ratio, at = _report(f"{kind} {form} {label}", err, bound)
    if _outside(err, bound).any():
      failures.append((label, float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("nan"), [float(v) for v in got], [float(v) for v in ref]))
      print(f"    OUTSIDE THE BOUND {failures[-1]}")

  try:
    e = Engine(ModelConfig(model="vae", likelihood=kind, **_NET, **STEP_KINDS[kind]), max_batch=8)
    e.set_params({"out/W": np.zeros(e.shapes["out/W"], np.float32), "out/b": bias.reshape(-1)})
    e.upload(t)
    e.set_flag("stacked_scoring", stacked)

    def run():
      return (e.marginal_llk(row_ids=rows, n_samples=S_SCORE), e.marginal_llk(x=t, n_samples=S_SCORE),
              e.score_llk([None, other], row_ids=rows, n_samples=S_SCORE), e.score_llk([t], x=other, n_samples=S_SCORE))
    base = run()                      # (default knobs: the bits the knobs are held to)
    m = e.eval_step(rows)
    for name, v in knobs.items():
      _hip.set_tuning(name, v)
    (mres, mhost, sres, shost) = got = run() if knobs else base
    if "no_score_queue" in knobs:     # the straight-line form and the queue form: the same bits
      for a, b in zip((base[0][1], base[1][1], base[2], base[3]), (mres[1], mhost[1], sres, shost)):
        assert np.array_equal(_bits(a), _bits(b)), (kind, form)
    if stacked and not knobs:
      for ranges in (0, 1, 2):
        _hip.set_tuning("score_walk", ranges)
        try:
          alt = run()
        finally:
          _hip.clear_tuning("score_walk")
        for a, b in zip((base[0][0], base[0][1], base[2], base[3]), (alt[0][0], alt[0][1], alt[2], alt[3])):
          assert np.array_equal(_bits(a), _bits(b)), (kind, form, ranges)
    ref_e, bound_e = _draw_bound(kind, t, planes, False, N_ADD_STEP)
    held("eval_step nllk_x", [m["nllk_x"]], np.array([-ref_e.mean()]), np.array([bound_e.mean()]))
    ref_m, bound_m = _draw_bound(kind, t, planes, False, N_ADD_DRAW + 6 + S_SCORE + 1)
    for label, r in (("marginal_llk llk (resident rows)", mres), ("marginal_llk llk (host rows)", mhost)):
      if not np.isfinite(r[0]).all():   # (the first output carries the latent posterior's terms: the encoder's business, not the likelihood's)
        print(f"    {kind} {form} {label}: importance-weighted estimate not finite at cells {np.nonzero(~np.isfinite(r[0]))[0].tolist()}")
      held(label, r[1], ref_m, bound_m)
    lme = (S_SCORE + 10.0) * U * (1.0 + np.log(S_SCORE))
    for col, count_only in ((0, False), (1, True)):
      ref_t, bound_t = _draw_bound(kind, t, planes, count_only and zi, N_ADD_DRAW)
      ref_o, bound_o = _draw_bound(kind, other, planes, count_only and zi, N_ADD_DRAW)
      held(f"score_llk column {col} (the input rows)", sres[0, col], ref_t, bound_t + 2.0 * U * np.abs(ref_t) + lme)
      held(f"score_llk column {col} (a target matrix, resident input)", sres[1, col], ref_o, bound_o + 2.0 * U * np.abs(ref_o) + lme)
      held(f"score_llk column {col} (a target matrix, host input)", shost[0, col], ref_t, bound_t + 2.0 * U * np.abs(ref_t) + lme)
    if not zi:
      assert np.array_equal(_bits(sres[:, 0]), _bits(sres[:, 1]))
  finally:
    if e is not None:
      e.close()
    for name in knobs:
      _hip.clear_tuning(name)
  assert not failures, (kind, form, failures)
