"""The training step, evaluation and predict against the float64 oracle across the minibatch-size ladder: the last and first row counts
of every BatchNorm bracket of smx_bn.hip (BN_RL * RPT = 128, 256, 512, 1024 rows, and the form beyond that makes a round trip through
xhat), both sides of the 128- and 256-row bounds of the fused launch forms, and the one-, two- and three-row batches that
fit(drop_remainder=False) can end an epoch with.  DESIGN.md ("Row-count predicates") lists the bounds and the cases on each side.

Rows are drawn WITHOUT replacement from a dataset larger than the batch (noise is keyed by cell id: duplicate rows would share their
draws and hide a row-indexing error), and the engine's capacity is the batch itself (routing reads max_batch).  Tolerances of
test_gpu_step.py (1e-4 relative, BASELINE.json north_star); nothing here is wider."""
import functools

import numpy as np
import pytest

from oracle import sisua_oracle as so
from tests import activations_ref
from tests import test_gpu_activations as tga
from tests import test_gpu_train_draws as tgd
from tests.test_gpu_step import CASES, RTOL, _oracle_step, _problem, check_one_step
from tests.util import adam_state_errors, masked_move_error, perturbed_params, rel_l2

pytestmark = pytest.mark.gpu
BASE = 1000
FLOOR_FRAC = 1e-3   # tests.util.grad_errors: tensors below this fraction of the largest gradient norm are judged on an absolute floor
WIDE = ("wide_panel_64", "wide_panel_128")

LADDER = {
    "vae_zinb": (1, 2, 3, 64, 65, 127, 128, 129, 256, 257, 512, 513, 1024, 1025, 1500),
    "vae_nb_nobn": (1, 2, 129, 257, 1025, 1500),
    "paper_shape": (1, 128, 129, 256, 257, 513, 1100),
    "scvi_default": (1, 2, 256, 257, 1025),
    "sisua": (1, 3, 129, 257, 1025),
    "fvae": (2, 257, 1025),
    "scale_post": (2, 257, 1025),
    "misa_tril": (129, 1025),
    "wide_panel_64": (1, 128, 129, 256, 257, 600),
    "wide_panel_128": (1, 128, 129, 256, 257, 600),
}
AT_THE_DEGENERATE_POINT = ("vae_zinb", "sisua")   # at one row: most of their tensors sit upstream of a BatchNorm layer


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _n_cells(name, batch):
  """1600 cells for the narrow cases, 700 for the wide panels -- more where a batch would not fit without replacement."""
  return max(700 if name in WIDE else 1600, batch + 75)


@functools.lru_cache(maxsize=4)
def _data(name, n):
  """One dataset per (case, size), shared by the tests of the case and left unchanged (the arrays are read-only)."""
  spec, cfg, x, ys, lib, mask = _problem(CASES[name], n=n)
  for a in [x, lib, mask] + list(ys):
    a.setflags(write=False)
  return spec, cfg, x, ys, lib, mask


def _rows(n, batch, seed=1):
  return np.random.default_rng(seed).choice(n, size=batch, replace=False).astype(np.int32)


def _below_floor(grads):
  """The tensors grad_errors judges on its absolute floor: the oracle's gradient norm is below FLOOR_FRAC of the largest."""
  norms = {k: np.linalg.norm(np.asarray(v, np.float64)) for k, v in grads.items()}
  top = max(norms.values())
  return sorted(k for k, v in norms.items() if v < max(FLOOR_FRAC * top, 1e-5))


# Where the oracle itself puts tensors below the floor from two rows up (float64, measured as a fraction of the largest gradient norm):
# misa_tril's full-covariance label head (alpha = 10) has a gradient norm 1e6 times the gene head's at every batch size -- out/W 6e-7,
# out/b 2e-7, lab1/W 2e-7, lab1/b 3e-8 of it at 129 and 1025 rows -- and at two rows fvae's discriminator biases are at 4e-5 .. 7e-4.
# These tensors are NOT left to the floor: each is held to RTOL of its own norm (_check_floor).
SMALL_BY_STRUCTURE = {
    ("misa_tril", 129): ["lab1/W", "lab1/b", "out/W", "out/b"],
    ("misa_tril", 1025): ["lab1/W", "lab1/b", "out/W", "out/b"],
    ("fvae", 2): ["disc0/b", "disc1/b", "disc2/b", "discout/b"],
}


def _check_floor(e, res, spec, name, batch):
  """The floor cannot hide a dead comparison.  From two rows up, and without BatchNorm at any size, NO tensor is judged on it: the oracle
  puts none below it, except the SMALL_BY_STRUCTURE ones, which are held to RTOL of their OWN norm here.  At one row with BatchNorm
  (variance exactly 0: every gradient upstream of a BatchNorm layer is analytically 0) the tensors below the floor are the oracle's own
  set, computed from its gradients -- at least 5 of them in the AT_THE_DEGENERATE_POINT cases -- and the device puts the same tensors,
  no more and no fewer, below the floor, with finite values.  (Not every member of that set is an analytic zero: at wide_panel_64-1 the
  oracle's lat/W has a norm of 6.5e-2 under a floor of 6.9e-2 -- a 6 % margin, hundreds of times the 1e-4 of the floor that the gradient
  bar allows the device's norm to differ by; a change of the case's data or seed that moves that norm across the floor changes the
  oracle's set and the device's alike.)"""
  low = _below_floor(res["grads"])
  got = e.get_params(which=1)
  if batch >= 2 or not spec.batchnorm:
    assert low == SMALL_BY_STRUCTURE.get((name, batch), []), (name, batch, low)
    for k in low:
      err = rel_l2(got[k], res["grads"][k])
      assert err < RTOL, (k, err)
    return
  if name in AT_THE_DEGENERATE_POINT:
    assert len(low) >= 5, (name, low)
  top = max(np.linalg.norm(v) for v in res["grads"].values())
  low_dev = sorted(k for k, v in got.items() if np.linalg.norm(np.asarray(v, np.float64)) < max(FLOOR_FRAC * top, 1e-5))
  assert low_dev == low, (name, low_dev, low)
  for k in low:
    assert np.isfinite(got[k]).all(), k


def _one_step(Engine, name, batch, problem):
  spec, cfg, x, ys, lib, mask = problem
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=batch, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=BASE)
  rows = _rows(x.shape[0], batch)
  p0 = {k: v.copy() for k, v in params.items()}
  res = _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, 0, cell_base=BASE)
  m = e.train_step(rows)
  check_one_step(e, m, res, spec, params, p0, bn, opt)
  _check_floor(e, res, spec, name, batch)
  assert all(np.isfinite(g).all() for g in e.get_params(which=1).values())
  e.close()


@pytest.mark.parametrize("name,batch", [(n, b) for n, sizes in LADDER.items() for b in sizes])
def test_one_step_on_the_ladder(Engine, name, batch):
  """test_gpu_step.py::test_one_step_matches_oracle's assertions (check_one_step, its bars) at the brackets' edges, and the floor-count
  condition of _check_floor."""
  _one_step(Engine, name, batch, _data(name, _n_cells(name, batch)))


@pytest.mark.parametrize("batch", [129, 513, 1025])
def test_one_step_general_activation_on_the_ladder(Engine, monkeypatch, batch):
  """The `_gen` BatchNorm templates (an activation other than ReLU on both nets, as test_gpu_activations.py sets it) in the RPT = 4, 16
  and xhat-round-trip brackets."""
  activations_ref.install(monkeypatch, enc="elu", dec="elu", encl="relu")
  _one_step(Engine, "vae_zinb", batch, tga._problem(CASES["vae_zinb"], "elu", "elu", "relu", n=1600))


TWO_STEP_CASES = [(n, b) for n in ("vae_zinb", "paper_shape", "scvi_default") for b in (257, 1025)]


@pytest.mark.parametrize("name,batch", TWO_STEP_CASES)
def test_second_step_reads_the_first_steps_state(Engine, name, batch):
  """Two steps on different rows against two oracle steps: the Adam moments and moving statistics a large-B launch leaves are what the
  next one reads.  The ELBO of every step within 1e-4 relative (the trajectory bar of test_gpu_step.py); and AFTER the second step, whose
  results are functions of the state the first one left: the Adam moments (m2 = b1 m1 + (1 - b1) g2, v2 likewise: linear / quadratic in
  the gradients) and the moving statistics at check_one_step's bars, and the second step's own move of every weight -- as a bound
  everywhere, and against the oracle's (masked_move_error, 2e-3) where the step's gradient is far above rounding.  The bound: with the
  bias corrections of step 2 the move is lr sqrt(1 + b2) / (1 + b1) * (b1 g1 + g2) / sqrt(b2 g1^2 + g2^2), at most
  lr sqrt(1 + b2) / (1 + b1) * sqrt(b1^2 / b2 + 1) = 1.0013 lr by Cauchy-Schwarz (epsilon and clipping only shrink it); the 1.001 slack of
  check_one_step's bound on top."""
  spec, cfg, x, ys, lib, mask = _data(name, _n_cells(name, batch))
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = Engine(cfg, max_batch=batch, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=BASE)
  ref, got = [], []
  for s in range(2):
    rows = _rows(x.shape[0], batch, seed=11 + s)
    before, before_dev = {k: v.copy() for k, v in params.items()}, e.get_params()
    res = _oracle_step(spec, params, bn, opt, x, ys, lib, mask, rows, s, cell_base=BASE)
    ref.append(res["loss"])
    m = e.train_step(rows)
    assert m["nan_flag"] == 0 and m["step"] == s + 1
    got.append(m["loss"])
  ref, got = np.array(ref), np.array(got)
  assert np.allclose(got, ref, rtol=RTOL), np.abs(got / ref - 1).max()
  em, ev, where = adam_state_errors(e, opt)
  assert em < 2e-4 and ev < 4e-4, (em, ev, where)
  names = [p for p, _ in so.bn_manifest(spec)]
  for i, st in e.get_bn().items():
    assert np.allclose(st["moving_mean"], bn[f"{names[i]}/moving_mean"], rtol=1e-4, atol=1e-6)
    assert np.allclose(st["moving_var"], bn[f"{names[i]}/moving_var"], rtol=1e-4, atol=1e-6)
  b1, b2 = spec.adam_beta1, spec.adam_beta2
  bound = 1.001 * spec.lr * np.sqrt(1 + b2) / (1 + b1) * np.sqrt(b1 * b1 / b2 + 1)
  after_dev = e.get_params()
  for k in after_dev:
    move = np.asarray(after_dev[k], np.float64) - before_dev[k]
    assert np.abs(move).max() <= bound and np.abs(params[k] - before[k]).max() <= bound, k
    err = masked_move_error(before[k] + move, before[k], params[k], res["grads"][k], spec.lr)   # (the device's move from the oracle's start)
    assert err is None or err < 2e-3, (k, err)
  e.close()


@pytest.mark.parametrize("name,batch", TWO_STEP_CASES)
def test_graph_replay_is_the_eager_step_at_large_row_counts(Engine, name, batch):
  spec, cfg, x, ys, lib, mask = _data(name, _n_cells(name, batch))
  params = perturbed_params(spec)
  n = 3
  order = np.concatenate([_rows(x.shape[0], batch, seed=30 + t) for t in range(n)]).astype(np.int32)
  hist, out = [], []
  for graph in (False, True):
    e = Engine(cfg, max_batch=batch, init=False)
    e.set_params(params)
    e.upload(x, ys, lib, mask, cell_id_base=BASE)
    e.train_steps(order, n, batch, graph=graph)
    hist.append(e.metrics_history(n))
    out.append(e.get_params())
    e.close()
  assert all(np.array_equal(hist[0][k], hist[1][k]) for k in hist[0])
  assert np.isfinite(np.asarray(hist[0]["loss"])).all()
  assert all(np.array_equal(out[0][k], out[1][k]) for k in out[0])


@pytest.mark.parametrize("batch,S", [(128, 4), (129, 4), (256, 4), (257, 4), (300, 4)])   # 512, 516, 1024, 1028 and 1200 stacked rows
@pytest.mark.parametrize("name", ["vae_zinb", "sisua"])
def test_stacked_draws_across_the_brackets(Engine, name, batch, S):
  """set_train_draws(S) stacks S x B rows: test_gpu_train_draws.py's oracle and bars where the stacked row count crosses the brackets."""
  spec, cfg, x, ys, lib, mask = _data(name, 1600)
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = tgd._engine(Engine, cfg, params, x, ys, lib, mask, max_batch=batch)
  e.set_train_draws(S)
  rows = _rows(x.shape[0], batch)
  res = tgd._oracle(spec, params, bn, opt, x, ys, lib, mask, rows, 0, S)
  m = e.train_step(rows)
  assert m["step"] == 1
  tgd._check_step(e, m, res, spec, bn, opt)
  assert _below_floor(res["grads"]) == []
  e.close()


@pytest.mark.parametrize("batch", [1, 257, 1025])
@pytest.mark.parametrize("name", ["vae_zinb", "scvi_default", "wide_panel_64"])
def test_eval_and_forward_on_the_ladder(Engine, name, batch):
  """eval_step and forward (the score_bn_* and stacked-decoder kernels) with non-trivial moving statistics: the block around
  e.eval_step(rows) of test_gpu_step.py::test_eval_and_forward_match_oracle and its tolerances.  (wide_panel_64 at 1025 rows: 1100 cells,
  so that the rows are still drawn without replacement.)"""
  spec, cfg, x, ys, lib, mask = _data(name, _n_cells(name, batch))
  params = perturbed_params(spec)
  bn = so.init_bn_state(spec)
  rng = np.random.default_rng(2)
  for k in bn:
    bn[k] = (bn[k] + 0.2 * rng.uniform(size=bn[k].shape)).astype(np.float32).astype(np.float64)
  e = Engine(cfg, max_batch=batch, init=False)
  e.set_params(params)
  names = [p for p, _ in so.bn_manifest(spec)]
  e.set_bn({i: dict(moving_mean=bn[f"{n}/moving_mean"], moving_var=bn[f"{n}/moving_var"]) for i, n in enumerate(names)})
  e.upload(x, ys, lib, mask)
  rows = _rows(x.shape[0], batch, seed=2)
  noise = so.PhiloxNoise(spec.seed, 0, rows, sample=0)
  res = so.forward_backward(spec, params, bn, x[rows], noise, y=[y[rows] for y in ys], library=lib[rows],
                            mask=mask[rows], training=False, backward=False)
  m = e.eval_step(rows)
  assert np.isclose(m["loss"], res["loss"], rtol=RTOL), (m["loss"], res["loss"])
  out = e.forward(row_ids=rows, sample_index=0)
  assert out["z_mean"].shape[0] == batch
  assert np.allclose(out["z_mean"], res["z_mean"], rtol=1e-4, atol=1e-5)
  assert np.allclose(out["z_scale"], res["z_scale"], rtol=1e-4, atol=1e-5)
  assert np.allclose(out["z_sample"], res["z"], rtol=1e-3, atol=1e-4)
  for c in range(spec.k):
    assert np.allclose(out["x_params"][c], res["x_params"][c], rtol=1e-3, atol=1e-4), c
  e.close()


def test_refusals_stay_refusals(Engine):
  """A batch beyond max_batch raises and leaves the engine usable (its next legal step is a fresh engine's, bit for bit); more than
  2^20 stacked rows are refused before anything is allocated."""
  from sisua_amd import SmxError
  spec, cfg, x, ys, lib, mask = _data("vae_zinb", 1600)
  params = perturbed_params(spec)
  B = 129
  e, e0 = (tgd._engine(Engine, cfg, params, x, ys, lib, mask, max_batch=B) for _ in range(2))
  with pytest.raises(SmxError):
    e.train_step(_rows(x.shape[0], B + 1))
  with pytest.raises(SmxError, match="2\\^20"):
    e.set_train_draws((1 << 20) // B + 1)   # (129 x 8129 = 2^20 + 65 rows)
  rows = _rows(x.shape[0], B)
  m, m0 = e.train_step(rows), e0.train_step(rows)
  assert m == m0 and m["step"] == 1 and m["nan_flag"] == 0
  p, p0 = e.get_params(), e0.get_params()
  assert all(np.array_equal(p[k], p0[k]) for k in p)
  e.close(); e0.close()
