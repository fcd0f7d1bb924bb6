"""predict()'s draw axis where the Monte-Carlo draws of a minibatch span SEVERAL decoder passes (predict_batch_stacked,
sisua_amd/csrc/smx_predict.hip).  A pass holds at most 4096 stacked rows: Sc = min(S, max(1, 4096 // B)) draws of the B rows it decodes, and
with super-batches B is batch * (max_batch // batch), not the caller's batch.  The second and later passes run code no first pass runs: the
draw kernel's first draw index, the sampler's counter, every destination offset with an s0 term, the pack jobs' s0 * Cn offsets and the
accumulation of `mean_over_samples` across passes.

Shapes: 40 genes (padded 64), one hidden layer of 32, latent_dim 6, 300 cells, minibatches of 32.
  engine A: max_batch 128 -- super-batches of 128, 128 and a ragged 44 rows: 32 draws per pass for the full ones, 93 for the ragged one;
  engine B: max_batch 32 -- no super-batches, 128 draws per pass (the last minibatch of 12 rows: 341): ONE pass wherever S <= 128.
Both give every cell the noise id row % 32, so all 300 cells are comparable.  Draw counts 32 (exactly one full pass), 33 (a pass of one
draw), 64 (two full passes), 70 (32 + 32 + 6 while the ragged super-batch takes one pass of 70), 100 (the ragged one splits too: 93 + 7).

  1. per-draw outputs of A equal B's bit for bit, and draw s differs from draw s - Sc;
  2. draws {0, Sc - 1, Sc, S - 1} against smx_forward minibatch by minibatch and (VAE 'zinb') against the float64 oracle;
  3. mean_over_samples against the float64 mean of the per-draw means inside a derived bound (`mos_bound`; its host check is
     test_mean_bound_holds_for_the_kernels_order), the column gather, the imputation scores and the correlation sums on that mean;
  4. one draw per pass (2304 rows per pass);
  5. through a fitted model.

The GPU tests carry the `gpu` mark one by one: the host test of the bound runs without a device."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import sisua_oracle as so
from tests import correlation_ref as CR
from tests import imputation_ref as IR
from tests import output_kinds_ref as kinds
from tests.util import make_pair, perturbed_params, synth_counts, synth_labels

gpu = pytest.mark.gpu

N, G, BATCH = 300, 40, 32
PASS_ROWS = 4096                 # the stacked rows of one decoder pass (predict_batch_stacked)
DRAWS = [32, 33, 64, 70, 100]
SEED = 20261019                  # of the predictive samples; written before the first GPU run
TOL = dict(rtol=2e-5, atol=2e-5)   # test_predict_packs_every_label_plane's bound of stacked decode against smx_forward

_NET = dict(n_genes=G, enc_units=(32,), dec_units=(32,), latent_dim=6)
MODELS = {
    "vae_zinb": dict(model="vae", likelihood="zinb", **_NET),
    "vae_nb": dict(model="vae", likelihood="nb", **_NET),                       # two planes
    "sisua_nb_head": dict(model="sisua", likelihood="zinb", labels=((12, "nb"),), **_NET),
    "scale_mixture_prior": dict(model="scale", likelihood="zinb", n_components=7, **_NET),
    "vae_bernoulli": dict(model="vae", likelihood="bernoulli", **_NET),        # plane_stat_rv_kernel / plane_logprob_rv_kernel
    "vae_normal": dict(model="vae", likelihood="normal", **_NET),
}
SCVI = dict(model="scvi", likelihood="zinbd", encl_units=(16,), **_NET)        # outside the stacked form: the control


@pytest.fixture(autouse=True)
def _oracle_knows_the_kinds(monkeypatch):
  kinds.install(monkeypatch)


# ---- the pass plan and the bound of the accumulated mean (host) ----------------------------------------------------------------
def draws_per_pass(n, batch, max_batch, S):
  """[n] int: the draws per decoder pass of every cell's (super-)batch -- predict_core's step and predict_batch_stacked's Sc restated"""
  step = batch * (max_batch // batch) if max_batch >= 2 * batch else batch
  sc = np.empty(n, np.int64)
  for b0 in range(0, n, step):
    rows = min(step, n - b0)
    sc[b0:b0 + rows] = min(S, max(1, PASS_ROWS // rows))
  return sc


def mos_bound(mean_draws, sc):
  """The bound of |mean_over_samples - float64 mean over the draws| per element.  The kernel adds a pass's Sn <= S per-draw means one after
  the other in float32 (at most Sn - 1 roundings of partial sums that never exceed the pass's sum of |mean|), multiplies by a rounded 1 / S
  (two roundings) and adds the share to the running value (one rounding per pass, of a value no larger than the whole sum / S).  With
  u = 2^-24 and P passes that is below (S + 2 P + 2) u mean_s |mean_s|, first order; the terms in u^2 are 2^-24 of it."""
  m = np.abs(np.asarray(mean_draws, np.float64))
  S = m.shape[0]
  P = -(-S // np.asarray(sc, np.float64))                       # passes per cell
  P = P.reshape(P.shape + (1,) * (m.ndim - 1 - P.ndim))
  return (S + 2.0 * P + 2.0) * 2.0 ** -24 * m.mean(axis=0)


def replay_mean_f32(mean_draws, sc):
  """plane_stat_kernel's stat 2 in NumPy float32: per pass the draws added in order, the sum times float32(1 / S), the share added to what
  the earlier passes left"""
  m = np.asarray(mean_draws, np.float32)
  S = m.shape[0]
  inv = np.float32(1.0) / np.float32(S)
  run = None
  for s0 in range(0, S, sc):
    acc = np.zeros(m.shape[1:], np.float32)
    for s in range(s0, min(S, s0 + sc)):
      acc = acc + m[s]
    run = acc * inv if run is None else run + acc * inv
  assert run.dtype == np.float32
  return run


def test_pass_plan_is_the_one_this_file_is_built_on():
  a = draws_per_pass(N, BATCH, 128, 100)
  assert set(a[:256]) == {32} and set(a[256:]) == {93}
  assert set(draws_per_pass(N, BATCH, 128, 70)[256:]) == {70}
  assert set(draws_per_pass(N, BATCH, 32, 100)) == {100} and set(draws_per_pass(N, BATCH, 32, 128)[:288]) == {128}
  assert set(draws_per_pass(2304, 2304, 2304, 2)) == {1}
  assert set(draws_per_pass(N, 8, 64, 70)[:256]) == {64} and set(draws_per_pass(N, 8, 64, 70)[256:]) == {70}   # the fitted model's engine


@pytest.mark.parametrize("S,sc", [(32, 32), (33, 32), (64, 32), (70, 32), (100, 32), (100, 93), (2, 1), (70, 64)])
def test_mean_bound_holds_for_the_kernels_order(S, sc):
  """The float64 reference against a NumPy float32 replay of the kernel's order stays inside `mos_bound` on random non-negative data:
  twelve decades of magnitudes, exact zeros, and draws of one element that differ by decades."""
  rng = np.random.default_rng(S * 1000 + sc)
  m = (rng.lognormal(0.0, 4.0, size=(S, 8192)) * 10.0 ** rng.integers(-3, 4, size=(1, 8192))).astype(np.float32)
  m[rng.uniform(size=m.shape) < 0.1] = 0.0
  m[:, :64] = np.float32(0.1)   # equal terms: every partial sum rounds
  ref = m.astype(np.float64).mean(axis=0)
  err = np.abs(replay_mean_f32(m, sc).astype(np.float64) - ref)
  bound = mos_bound(m, np.full(m.shape[1], sc))
  worst = float((err / np.maximum(bound, 1e-300)).max())
  print(f"host replay S={S} Sc={sc}: worst error / bound {worst:.3f}")
  assert (err <= bound).all(), worst


# ---- engines, parameters and rows: made once per model ---------------------------------------------------------------------------
_SETUP = {}


def _setup(name):
  if name not in _SETUP:
    kw = SCVI if name == "scvi" else MODELS[name]
    spec, cfg = make_pair(**kw)
    if spec.likelihood in ("bernoulli", "normal"):
      x = kinds.synth_x(spec.likelihood, N, G, seed=0)
    else:
      x = synth_counts(N, G, sparsity=0.85, seed=0, max_count=2000)
    params, bn = perturbed_params(spec), so.init_bn_state(spec)
    rng = np.random.default_rng(2)
    for k in bn:   # moving statistics that are not the initial ones
      bn[k] = (bn[k] + 0.2 * rng.uniform(size=bn[k].shape)).astype(np.float32).astype(np.float64)
    lib = None
    if spec.model == "scvi":
      _, lm, lv = so.library_size(x)
      lib = np.tile(np.array([[lm, lv]], dtype=np.float32), (N, 1))
    x.setflags(write=False)
    _SETUP[name] = (spec, cfg, params, bn, x, lib)
  return _SETUP[name]


@pytest.fixture(scope="module")
def engines():
  """engines(name, max_batch): the model's engine with the perturbed parameters and moving statistics; every engine is closed at the end"""
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  made = {}

  def get(name, max_batch):
    if (name, max_batch) not in made:
      spec, cfg, params, bn, _, _ = _setup(name)
      e = Engine(cfg, max_batch=max_batch, init=False)
      e.set_params(params)
      names = [p for p, _ in so.bn_manifest(spec)]
      e.set_bn({i: dict(moving_mean=bn[f"{n}/moving_mean"], moving_var=bn[f"{n}/moving_var"]) for i, n in enumerate(names)})
      made[(name, max_batch)] = e
    return made[(name, max_batch)]
  yield get
  for e in made.values():
    e.close()


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
  """bit for bit, any NaN standing for any NaN"""
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _other_target(spec, x):
  """rows that are not the input: counts + 1, the flipped bits, the shifted levels"""
  if spec.likelihood == "bernoulli":
    return (1.0 - x).astype(np.float32)
  return (x + (0.5 if spec.likelihood == "normal" else 1.0)).astype(np.float32)


def _per_draw(e, spec, x, S, form=np.asarray):
  """every output with a draw axis, of one engine: {name: array}"""
  xin = form(x)
  p = e.predict(xin, n_samples=S, batch=BATCH)
  t = _other_target(spec, x)
  out = dict(z_mean=p["z_mean"], z_sample=p["z_sample"], x_params=p["x_params"])
  for j, y in enumerate(p["y_params"]):
    out[f"y_params{j}"] = y
  for stat in ("mean", "variance"):
    out[stat] = e.predict_stat(xin, stat, n_samples=S, batch=BATCH)
  out["log_prob_input"] = e.predict_stat(xin, "log_prob", n_samples=S, batch=BATCH)
  out["log_prob_dense"] = e.predict_stat(xin, "log_prob", n_samples=S, batch=BATCH, target=t)
  out["log_prob_csr"] = e.predict_stat(xin, "log_prob", n_samples=S, batch=BATCH, target=sp.csr_matrix(t))
  out["sample"] = e.predict_stat(xin, "sample", n_samples=S, batch=BATCH, seed=SEED, n=2)
  return out


# ---- 1. per-draw outputs ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S", DRAWS)
@pytest.mark.parametrize("name", list(MODELS))
def test_per_draw_outputs_do_not_depend_on_the_pass_split(engines, name, S):
  """Engine A (several passes) against engine B (one pass): every draw of every cell, bit for bit.  This rests on the planes of a cell not
  depending on how many rows share its pass (the products of the stacked form take the 128 x 32 tile at every row count that occurs here:
  more than 64 rows per pass; the encoder's, at 128, 44, 32 and 12 rows, gave the same bits too).  On an MI355X no element of any output
  differed at any of the draw counts.  And within A: draw s is not draw s - Sc, the draw a later pass would repeat if it started from 0
  again."""
  spec, _, _, _, x, _ = _setup(name)
  a, b = _per_draw(engines(name, 128), spec, x, S), _per_draw(engines(name, BATCH), spec, x, S)
  assert set(draws_per_pass(N, BATCH, BATCH, S)) == {S}   # B: one pass
  assert a["x_params"].shape == (S, spec.k, N, G) and a["z_sample"].shape == (S, N, 6) and a["sample"].shape == (2, S, N, G)
  assert a["log_prob_input"].shape == (S, N) and a["mean"].shape == (S, N, G)
  if spec.labels:
    assert a["y_params0"].shape == (S, N, 2 * 12)
  for key in a:
    assert np.isfinite(a[key]).all(), key
    differ = int((_bits(a[key]) != _bits(b[key])).sum())
    print(f"{name} S={S} {key}: {differ} of {a[key].size} elements differ between the pass splits")
    assert _same(a[key], b[key]), (key, differ)
  assert _same(a["log_prob_dense"], a["log_prob_csr"])
  sc = draws_per_pass(N, BATCH, 128, S)
  for c in np.unique(sc):
    cells = np.flatnonzero(sc == c)
    if c >= S:
      continue
    for key in ("z_sample", "mean"):   # vectors per cell and draw: a repeated draw repeats every entry
      moved = (a[key][c:][:, cells] != a[key][:S - c][:, cells]).any(axis=-1)
      assert moved.all(), (key, int(c), int((~moved).sum()))
    later, earlier = a["x_params"][c:][:, :, cells], a["x_params"][:S - c][:, :, cells]
    assert (later[:, 0] != earlier[:, 0]).any(axis=-1).all()
    # log_prob is ONE float32 per cell and draw: two different draws may round to the same sum (seen on the device: 1 pair of 17 408 at
    # 100 draws of the SCALE model), a repeated pass repeats them all
    moved = a["log_prob_input"][c:][:, cells] != a["log_prob_input"][:S - c][:, cells]
    assert moved.mean() > 0.99, (int(c), float(moved.mean()))
    # the predictive samples of the two draws: other planes and other counters -- not the same matrix
    assert not np.array_equal(a["sample"][:, c:][:, :, cells], a["sample"][:, :S - c][:, :, cells])


@gpu
def test_scvi_control_is_smx_forward_draw_by_draw(engines):
  """scvi is outside the stacked form (its draws go one decoder pass each): 40 draws equal smx_forward(sample_index=s) bit for bit."""
  spec, _, _, _, x, lib = _setup("scvi")
  e = engines("scvi", 128)
  S = 40
  got = e.predict(x, library=lib, n_samples=S, batch=BATCH)
  for b0 in range(0, N, BATCH):
    sl = slice(b0, b0 + BATCH)
    for s in (0, 31, 32, 39):
      one = e.forward(x=x[sl], library=lib[sl], sample_index=s)
      assert np.array_equal(got["x_params"][s][:, sl], one["x_params"]), (b0, s)
      assert np.array_equal(got["z_sample"][s][sl], one["z_sample"]) and np.array_equal(got["l_sample"][s][sl], one["l_sample"]), (b0, s)
    assert np.array_equal(got["z_mean"][sl], one["z_mean"])
  assert not np.array_equal(got["z_sample"][32], got["z_sample"][0])


# ---- 2. against something that is not predict ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_draws_of_every_pass_match_forward(engines, name):
  """S = 70 on engine A: the first and the last draw of the first pass, the first draw of the second and the last draw of the third (of the
  ragged super-batch's single pass: its draws 0, 31, 32, 69) against smx_forward(sample_index=s) minibatch by minibatch -- the same-cell,
  other-pass errors a defect shared by A and B would hide.  VAE 'zinb': also against the float64 oracle's evaluation forward under the
  draw's noise, at test_eval_and_forward_match_oracle's tolerance.  (On an MI355X the stacked planes equalled smx_forward's at these
  shapes; the bound stays test_predict_packs_every_label_plane's.)"""
  spec, _, params, bn, x, _ = _setup(name)
  e = engines(name, 128)
  S = 70
  got = e.predict(x, n_samples=S, batch=BATCH)
  worst = {}
  for b0 in range(0, N, BATCH):
    sl = slice(b0, min(N, b0 + BATCH))
    for s in (0, 31, 32, S - 1):
      one = e.forward(x=x[sl], sample_index=s)
      pairs = [("x_params", got["x_params"][s][:, sl], one["x_params"]), ("z_sample", got["z_sample"][s][sl], one["z_sample"])]
      pairs += [(f"y_params{j}", a[s][sl], b) for j, (a, b) in enumerate(zip(got["y_params"], one["y_params"]))]
      for key, a, b in pairs:
        worst[key] = max(worst.get(key, 0.0), float(np.abs(a - b).max()))
        assert np.allclose(a, b, **TOL), (key, b0, s, float(np.abs(a - b).max()))
      if name == "vae_zinb":
        nb = sl.stop - sl.start
        res = so.forward_backward(spec, params, bn, x[sl], so.PhiloxNoise(spec.seed, 0, np.arange(nb), sample=s), training=False,
                                  backward=False)
        assert np.allclose(got["z_sample"][s][sl], res["z"], rtol=1e-3, atol=1e-4), (b0, s)
        for c in range(spec.k):
          assert np.allclose(got["x_params"][s][c][sl], res["x_params"][c], rtol=1e-3, atol=1e-4), (b0, s, c)
    assert np.array_equal(got["z_mean"][sl], one["z_mean"])
  assert len(got["y_params"]) == len(spec.labels)
  print(f"{name} S={S}: max |predict - forward| {worst}")


# ---- 3. the accumulated mean ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S", DRAWS)
@pytest.mark.parametrize("name", list(MODELS))
def test_mean_over_samples_accumulates_every_pass(engines, name, S):
  """mean_over_samples of A against the float64 mean over s of A's own per-draw `mean` (both read the same planes through the same
  moment code): every element inside `mos_bound`, about 5e-6 relative at S = 70.  The dense and the CSR input form give the same bits, and
  genes=[...] the bits of those columns."""
  spec, _, _, _, x, _ = _setup(name)
  e = engines(name, 128)
  idx = [17, 3, 39, 3, 0]
  for count_only in ((False, True) if spec.likelihood == "zinb" else (False,)):
    kw = dict(n_samples=S, batch=BATCH, count_only=count_only)
    draws = e.predict_stat(x, "mean", **kw)
    mos = e.predict_stat(x, "mean_over_samples", **kw)
    assert mos.shape == (N, G) and mos.dtype == np.float32 and np.isfinite(mos).all()
    ref = draws.astype(np.float64).mean(axis=0)
    err, bound = np.abs(mos.astype(np.float64) - ref), mos_bound(draws, draws_per_pass(N, BATCH, 128, S))
    scale = np.abs(draws.astype(np.float64)).mean(axis=0)
    print(f"{name} S={S} count_only={count_only}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
          f"worst error / mean |mean| {float((err / np.maximum(scale, 1e-300)).max()):.3e}")
    assert (err <= bound).all(), (int((err > bound).sum()), float((err / np.maximum(bound, 1e-300)).max()))
    assert _same(e.predict_stat(sp.csr_matrix(x), "mean_over_samples", **kw), mos)
    assert _same(e.predict_stat(x, "mean_over_samples", genes=idx, **kw), mos[:, idx])
    assert _same(e.predict_stat(sp.csr_matrix(x), "mean_over_samples", genes=idx, **kw), mos[:, idx])


@gpu
@pytest.mark.parametrize("S", [70, 100])
@pytest.mark.parametrize("name", ["vae_zinb", "vae_bernoulli"])
def test_imputation_scores_are_exact_functions_of_a_multi_pass_mean(engines, name, S):
  """The scores of a call whose draws span several passes are the exact functions (tests/imputation_ref.py, as
  test_scores_are_exact_functions_of_the_device_mean at 3 draws) of that call's mean_over_samples: the imputation kernels read the mean
  when the last pass has added its share."""
  from sisua_amd.data import corrupt
  from sisua_amd.distributions import imputation_scores_from_cells
  spec, _, _, _, x, _ = _setup(name)
  e = engines(name, 128)
  cor = np.array(x)
  cor[40:200] = corrupt(x[40:200], dropout_rate=0.3, retain_rate=0.2, seed=8)
  changed = IR.cell_changed(x, cor)
  assert changed.any() and not changed.all()
  kw = dict(n_samples=S, batch=BATCH, count_only=spec.likelihood == "zinb")
  mean = e.predict_stat(cor, "mean_over_samples", **kw)
  for form_x, form_o in ((np.asarray, np.asarray), (sp.csr_matrix, sp.csr_matrix)):
    cells = e.predict_impute(form_x(cor), form_o(x), **kw)
    assert _same(cells["cell_median"], IR.cell_medians(x, mean))
    assert np.array_equal(cells["cell_changed"].astype(bool), changed)
    lo, hi = IR.middle_two(IR.abs_diff(x, mean).reshape(1, -1))
    assert _same(cells["global_lohi"], [lo[0], hi[0]])
    got, want = imputation_scores_from_cells(cells["cell_median"], cells["cell_changed"], cells["global_lohi"]), IR.scores(x, cor, mean)
    for k in want:
      assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])


@gpu
@pytest.mark.parametrize("S", [70, 100])
@pytest.mark.parametrize("name", ["vae_zinb", "vae_normal"])
def test_correlation_sums_read_a_multi_pass_mean(engines, name, S):
  """The correlation sums of a multi-pass call against tests/correlation_ref.py on that call's mean_over_samples, at
  tests/test_gpu_correlation.py's bounds: the integer sums equal, Pearson and Spearman within 1e-9 of the per-pair SciPy calls."""
  from sisua_amd.distributions import correlations_from_sums, protein_operands
  spec, _, _, _, x, _ = _setup(name)
  e = engines(name, 128)
  extras = synth_labels(N, ((9, "nb"),))[0].astype(np.float64)
  ops = protein_operands(extras)
  kw = dict(n_samples=S, batch=BATCH, count_only=spec.likelihood == "zinb")
  mean = e.predict_stat(x, "mean_over_samples", **kw)
  sums = e.predict_correlate(x, ops["rank2"], ops["unit"], **kw)
  want = CR.numpy_sums(mean.T, extras)
  for k in ("sp_Sa", "sp_Saa", "sp_Sab"):
    assert np.array_equal(sums[k], want[k]), k
  assert not sums["nonfinite"].any()
  csr = e.predict_correlate(sp.csr_matrix(x), ops["rank2"], ops["unit"], **kw)
  for k in sums:
    assert sums[k].tobytes() == csr[k].tobytes(), k
  got = correlations_from_sums(N, sums["sp_Sa"], sums["sp_Saa"], sums["sp_Sab"], ops["Sb"], ops["Sbb"], sums["pe_Sxx"], sums["pe_Sxy"],
                               sums["nonfinite"], ops["constant"])
  pe, spm = CR.pair_matrices(mean.astype(np.float64), extras)
  for key, ref in (("pearson", pe), ("spearman", spm)):
    assert np.array_equal(np.isnan(got[key]), np.isnan(ref)) and np.isfinite(ref).sum() > G
    ok = ~np.isnan(ref)
    delta = float(np.abs(got[key][ok] - ref[ok]).max())
    print(f"{name} S={S} {key}: max |delta| {delta:.3e}")
    assert delta <= 1e-9, (key, delta)


# ---- 4. one draw per pass ---------------------------------------------------------------------------------------------------------
def _zinb_mean64(planes):
  p = np.asarray(planes, np.float64)
  return (1.0 - 1.0 / (1.0 + np.exp(-p[2]))) * np.exp(p[0]) * np.exp(p[1])


@gpu
def test_one_draw_per_pass():
  """max_batch = batch = 2304 rows: 4096 // 2304 = 1 draw per pass, so the second of two draws is a pass of its own.  Both draws against
  smx_forward(sample_index=s) at test 2's bound, mean_over_samples against the per-draw means at test 3's (two passes)."""
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  spec, cfg, params, bn, _, _ = _setup("vae_zinb")
  n, S = 2304, 2
  x = synth_counts(n, G, sparsity=0.85, seed=4)
  sc = draws_per_pass(n, n, n, S)
  e = Engine(cfg, max_batch=n, init=False)
  try:
    e.set_params(params)
    names = [p for p, _ in so.bn_manifest(spec)]
    e.set_bn({i: dict(moving_mean=bn[f"{k}/moving_mean"], moving_var=bn[f"{k}/moving_var"]) for i, k in enumerate(names)})
    got = e.predict(x, n_samples=S, batch=n)
    draws = e.predict_stat(x, "mean", n_samples=S, batch=n)
    mos = e.predict_stat(x, "mean_over_samples", n_samples=S, batch=n)
    ones = [e.forward(x=x, sample_index=s) for s in range(S)]
  finally:
    e.close()
  fwd_mean = np.stack([_zinb_mean64(o["x_params"]) for o in ones])
  for s in range(S):
    assert np.allclose(got["x_params"][s], ones[s]["x_params"], **TOL), s
    assert np.allclose(got["z_sample"][s], ones[s]["z_sample"], **TOL), s
    assert np.allclose(draws[s], fwd_mean[s], **TOL), (s, float(np.abs(draws[s] - fwd_mean[s]).max()))
  assert (got["z_sample"][1] != got["z_sample"][0]).any(axis=-1).all()
  assert np.allclose(mos, fwd_mean.mean(axis=0), **TOL)
  err = np.abs(mos.astype(np.float64) - draws.astype(np.float64).mean(axis=0))
  assert (err <= mos_bound(draws, sc)).all(), float(err.max())


# ---- 5. through the model ----------------------------------------------------------------------------------------------------------
@gpu
def test_draw_passes_through_a_fitted_model():
  """A VAE fitted at batch_size 64 keeps an engine of max_batch 64; predict(batch_size=8) then decodes super-batches of 64 rows, 64 draws
  per pass: sample_shape = 40 would be ONE pass, so 70 draws are asked for -- passes of 64 and 6 (the ragged super-batch of 44 rows: one pass
  of 70).  The lazy handle against the eager result at test_lazy_predict_keeps_the_planes_on_the_device's tolerances;
  materialize().mean() is the eager mean bit for bit.  The eager distributions draw their samples with NumPy, so `sample(2, seed)` is held
  to what can be said of it: the same bits as an engine of max_batch 8 (no super-batches: one pass of 70) gives from the same parameters,
  and per gene the pooled sample mean within 6 standard errors of the eager mean (test_lazy_sample_end_to_end's bound)."""
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as api
  from sisua_amd import distributions as D
  from sisua_amd.data import SingleCellOMIC
  from sisua_amd.engine import Engine
  n, g, S = 300, 120, 70
  x = synth_counts(n, g, sparsity=0.8, seed=3)
  sco = SingleCellOMIC(x, name="toy")
  m = api.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), latents=api.RVmeta(8, "diag", True, "Latents"),
              encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  m.fit(sco, epochs=3, batch_size=64, verbose=False)
  assert m._engine.max_batch == 64
  sc = draws_per_pass(n, 8, m._engine.max_batch, S)
  assert set(sc[:256]) == {64} and S > 64   # two passes
  eX, _ = m.predict(x, sample_shape=S, batch_size=8, verbose=False)
  lX, _ = m.predict(sco, sample_shape=S, batch_size=8, verbose=False)
  assert isinstance(lX, D.LazyCountOutput) and not isinstance(eX, D.LazyCountOutput) and lX.batch_shape == eX.batch_shape == (S, n)
  tol = dict(rtol=2e-5, atol=1e-6)
  lmean, emean = lX.mean(), eX.mean()
  assert lmean.shape == (S, n, g) and np.allclose(lmean, emean, **tol)
  evar = eX.variance()
  assert np.allclose(lX.variance(), evar, rtol=1e-4, atol=1e-5)
  assert np.allclose(lX.log_prob(), eX.log_prob(x), rtol=2e-5, atol=1e-3)
  mos = lX.mean_over_samples()
  assert np.allclose(mos, emean.mean(0), **tol)
  err = np.abs(mos.astype(np.float64) - lmean.astype(np.float64).mean(axis=0))
  assert (err <= mos_bound(lmean, sc)).all()
  assert (lmean[64:, :256] != lmean[:S - 64, :256]).any(axis=-1).all()   # the second pass is not the first again
  assert np.array_equal(lX.materialize().mean(), emean)
  xs = lX.sample(2, seed=SEED)
  assert xs.shape == (2, S, n, g) and xs.dtype == np.float32 and np.array_equal(xs, np.floor(xs)) and (xs >= 0).all()
  one = Engine(m._make_config(), max_batch=8, init=False)
  try:
    one.set_params(m._engine.get_params())
    one.set_bn(m._engine.get_bn())
    assert set(draws_per_pass(n, 8, 8, S)) == {S}
    assert _same(one.predict_stat(x, "mean", n_samples=S, batch=8), lmean)
    assert np.array_equal(one.predict_stat(x, "sample", n_samples=S, batch=8, seed=SEED, n=2), xs)
  finally:
    one.close()
  pooled = xs.astype(np.float64).mean(axis=(0, 1, 2))
  want = np.asarray(emean, np.float64).mean(axis=(0, 1))
  se = np.sqrt(np.asarray(evar, np.float64).sum(axis=(0, 1)) * 2) / (2 * S * n)
  z = (pooled - want) / se
  print(f"fitted model: max |z| of the per-gene pooled sample mean {np.abs(z).max():.2f}")
  assert np.all(np.abs(z) <= 6.0), float(np.abs(z).max())
