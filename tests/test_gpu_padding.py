"""The layout's invariant on the device: what lies outside the logical extent of a tensor stays exactly zero (sisua_amd/csrc/smx_model.h).

Every feature axis is padded to 32 and every tensor to 64 floats; dozens of kernels keep the padding at zero by hand (`live = col < a.H`,
`col < a.G`, the lanes beyond D of the latent kernels).  smx_get_tensor strips the padding, and a padded hidden column that is not zero
meets padded weight rows that still are: the first step is right, the padded weight rows then receive a gradient, and the model drifts
from step 2 on -- under an activation with act(0) != 0 (sigmoid 0.5, softplus log 2) at a width that is not a multiple of 32.

a. smx_pad_audit / smx_pad_poke: the instrument sees a planted violation and nothing else.
b. an oracle-free matrix: every pair of option values of fit() together at least once (a deterministic covering design, CASES), three eager
   steps and three through a captured graph at ragged widths, then the audit of parameters, gradients, both optimiser slots and the work
   buffers; fixed cases: wide panels, the BatchNorm forms by batch size, the separate-launch forms, data-parallel loopback, evaluation.
c. parity with the float64 oracle where the padding matters numerically: one step of every general activation, 20-step trajectories and
   the scores after them under sigmoid / softplus at encoder (48, 40), decoder (40,), latent 10, 203 genes.

Wall time on one MI355X: docs/LAB_NOTES.md ("Padding audit")."""
import functools
import itertools
import random

import numpy as np
import pytest

from oracle import sisua_oracle as so
from sisua_amd import interpolation as I
from tests import activations_ref as ref
from tests.test_gpu_activations import BASE, DROP, GENERAL, RTOL, _check_step, _engine, _problem
from tests.util import grad_errors, make_pair, perturbed_params, synth_counts, synth_labels

pytestmark = pytest.mark.gpu
N_CELLS = 300
WHICH = ("parameters", "gradients", "optimiser slot 2", "optimiser slot 3", "work buffers")


@pytest.fixture(scope="module")
def Engine():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd.engine import Engine
  return Engine


def _assert_clean(e, whichs=range(5), where=""):
  for w in whichs:
    n, name, off = e.pad_audit(w)
    assert n == 0, f"{where}: {n} non-zero padded elements in the {WHICH[w]}, first in '{name}' at offset {off}"


# ---- a. the instrument ---------------------------------------------------------------------------------------------------------------
def test_audit_sees_a_planted_violation_and_nothing_else(Engine):
  from sisua_amd._hip import SmxError
  kw = dict(model="vae", n_genes=203, likelihood="zinb", enc_units=(48, 64), dec_units=(64,), latent_dim=10)
  spec, cfg = make_pair(**kw)
  params = perturbed_params(spec)
  x = synth_counts(N_CELLS, 203, sparsity=0.85, seed=0)
  e = Engine(cfg, max_batch=64, init=False)
  e.set_params(params)
  e.upload(x)
  _assert_clean(e, where="after set_params + upload")
  for name, value in (("enc0/W", 1.0), ("enc0/gamma", np.float32(1e-42)), ("out/b", float("nan"))):   # (a denormal and a NaN count)
    e.pad_poke(0, name, value)
    n, first, off = e.pad_audit(0)
    assert n == 1 and first == name, (name, n, first, off)
    e.pad_poke(0, name, -0.0)   # (-0 is zero)
    assert e.pad_audit(0)[0] == 0
    e.pad_poke(0, name, value)
    e.set_params({name: params[name]})
    assert e.pad_audit(0)[0] == 0, name
  # the first padded element of enc0/W [203 -> 224][48 -> 64] is row 0, column 48
  e.pad_poke(0, "enc0/W", 2.0)
  assert e.pad_audit(0) == (1, "enc0/W", 48)
  e.set_params(params)
  for which in (1, 2, 3):
    e.pad_poke(which, "lat/b", 3.0)
    assert e.pad_audit(which)[:2] == (1, "lat/b") and e.pad_audit(0)[0] == 0
  with pytest.raises(SmxError):
    e.pad_poke(0, "enc1/gamma", 1.0)   # (64 wide: no padding)
  e.close()


def test_poke_refuses_a_tensor_without_padding(Engine):
  from sisua_amd._hip import SmxError
  spec, cfg = make_pair(model="vae", n_genes=64, likelihood="nb", enc_units=(64, 64), dec_units=(64,), latent_dim=32)
  e = Engine(cfg, max_batch=32, init=False)
  e.set_params(perturbed_params(spec))
  for name in ("enc0/W", "enc1/W", "enc1/gamma", "out/W"):   # 64 x 64 weights, a 64-wide vector, [64][2 x 64]: no padding at all
    with pytest.raises(SmxError):
      e.pad_poke(0, name, 1.0)
  with pytest.raises(SmxError):
    e.pad_audit(5)
  _assert_clean(e, range(4))
  e.close()


# ---- b. the crossed matrix -----------------------------------------------------------------------------------------------------------
FACTORS = dict(
    model=("vae", "dca", "sisua", "misa", "scvi_full", "scvi_share", "scale_diag", "scale_tril", "scale_mixture", "fvae", "semifvae"),
    act=("relu", "leaky_relu", "elu", "selu", "tanh", "sigmoid", "softplus", "linear"),
    latent=("diag", "mvntril"),
    out=("zinb", "nb", "zinbd", "nbd", "mse", "bernoulli", "normal"),
    bn=(True, False),
    drop=(0.2, 0.0),
    opt=("adam", "sgd", "rmsprop", "adagrad", "adamax"),
    clip=(True, False),
    draws=(1, 3),
    sched=(True, False),
)
TRIL_MODELS = ("vae", "sisua", "misa", "scvi_full", "scvi_share")
OPTIMIZERS = dict(adam={}, sgd=dict(momentum=0.9), rmsprop=dict(momentum=0.5), adagrad={}, adamax={})


def refusals(c):
  """Everything the library refuses about a configuration, from the configuration alone: a list of (where the refusal is raised, a piece of
  its message), in the order in which the library would raise them."""
  out = []
  if c["latent"] == "mvntril" and c["model"] not in TRIL_MODELS:
    out.append(("config", "mvntril"))
  if c["model"].startswith("scvi") and c["out"] not in ("nbd", "zinbd"):
    out.append(("create", "scvi supports nbd / zinbd only"))
  if c["model"] in ("fvae", "semifvae") and c["draws"] > 1:
    out.append(("draws", "one draw"))
  return out


def refusal(c):
  """The refusal of a case of the design (which holds at most one: covering_cases), or None."""
  r = refusals(c)
  return r[0] if r else None


def _tuples(c, n):
  keys = list(FACTORS)
  return {tuple((k, c[k]) for k in ks) for ks in itertools.combinations(keys, n)}


def _pairs(c):
  return _tuples(c, 2)


def covering_cases():
  """A deterministic covering design over FACTORS, in three parts.
  1. Pairs: greedy over cases the library accepts (the best of 200 candidates, each seeded with an uncovered pair) until no accepted case
     covers a new pair.
  2. Refusals: every pair left can only stand in a refused configuration -- (model without it, mvntril), (scvi, an output that is not
     nbd / zinbd), (fvae / semifvae, 3 draws) -- and gets a case that holds EXACTLY ONE reason for refusal, so that each refusal is the one
     the case asserts (a second reason would hide behind the first).  One model and one first output per case: these cannot be merged.
  3. The issue caps refusals at a tenth of the cases.  Accepted cases are added until that holds, each the candidate that covers the most
     option TRIPLES no earlier case holds: they buy three-way coverage, not repeats."""
  rng = random.Random(20261016)
  keys = list(FACTORS)
  todo = set()
  for a, b in itertools.combinations(keys, 2):
    todo |= {((a, u), (b, v)) for u in FACTORS[a] for v in FACTORS[b]}

  def draw(fixed=()):
    c = {k: rng.choice(FACTORS[k]) for k in keys}
    c.update(dict(fixed))
    return c

  cases = []
  while True:
    best, gain = None, 0
    open_pairs = sorted(todo, key=repr)
    for _ in range(200):
      c = draw(rng.choice(open_pairs)) if open_pairs else draw()
      if refusals(c):
        continue
      g = len(_pairs(c) & todo)
      if g > gain:
        best, gain = c, g
    if best is None:
      break
    cases.append(best)
    todo -= _pairs(best)
  while todo:
    pair = sorted(todo, key=repr)[0]
    best, gain = None, 0
    for _ in range(400):
      c = draw(pair)
      if len(refusals(c)) != 1:
        continue
      g = len(_pairs(c) & todo)
      if g > gain:
        best, gain = c, g
    assert best is not None, pair
    cases.append(best)
    todo -= _pairs(best)
  n_ref = sum(1 for c in cases if refusals(c))
  seen3 = set()
  for c in cases:
    seen3 |= _tuples(c, 3)
  while 10 * n_ref > len(cases):
    best, gain = None, -1
    for _ in range(100):
      c = draw()
      if refusals(c):
        continue
      g = len(_tuples(c, 3) - seen3)
      if g > gain:
        best, gain = c, g
    cases.append(best)
    seen3 |= _tuples(best, 3)
  return cases


CASES = covering_cases()


def _case_id(i, c):
  return f"{i:03d}-{c['model']}-{c['act']}-{c['latent']}-{c['out']}-bn{int(c['bn'])}-dr{c['drop']}-{c['opt']}-cl{int(c['clip'])}-s{c['draws']}-sc{int(c['sched'])}"


def case_kwargs(i, c):
  """The model keywords of case i: ragged widths throughout (genes 203 / 97, units (48, 40) / (33,) / (17,), latent 10 / 7, labels 12 / 7)."""
  big = i % 2 == 0
  kw = dict(n_genes=203 if big else 97, likelihood=c["out"], enc_units=(48, 40) if big else (33,), dec_units=(40,) if big else (17,),
            latent_dim=10 if big else 7, batchnorm=c["bn"], dropout_enc=c["drop"], dropout_dec=c["drop"], input_dropout=c["drop"])
  if c["clip"]:
    kw.update(clipnorm=0.05)
  m = c["model"]
  if m in ("vae", "dca"):
    kw.update(model=m)
  elif m == "sisua":
    kw.update(model="sisua", labels=((12, "nb"), (7, "onehot")))
  elif m == "misa":
    kw.update(model="sisua", labels=((12, "mixnb2"), (7, "mixtril2")))
  elif m.startswith("scvi"):
    kw.update(model="scvi", encl_units=(17,), dispersion="share" if m == "scvi_share" else "full")
  elif m.startswith("scale"):
    kw.update(model="scale", n_components=4, covariance="tril" if m == "scale_tril" else "none", latent_mixture=m == "scale_mixture")
  else:
    kw.update(model="fvae", disc_units=60, disc_layers=2, labels=((7, "onehot"),) if m == "semifvae" else ())
  return kw


def _data(kw, n=N_CELLS):
  x = synth_counts(n, kw["n_genes"], sparsity=0.85, seed=0, max_count=2000 if kw["n_genes"] < 500 else None)
  if kw["likelihood"] == "bernoulli":
    x = (x > 0).astype(np.float32)
  elif kw["likelihood"] == "normal":
    x = np.log1p(x).astype(np.float32)
  ys = synth_labels(n, tuple(kw.get("extra_outputs", ())) + tuple(kw.get("labels", ())))
  _, lm, lv = so.library_size(x)
  lib = np.tile(np.array([[lm, lv]], dtype=np.float32), (n, 1))
  mask = so.label_mask(n, 0.4, n_omics=1 + len(kw.get("labels", ())), seed=1)
  return x, ys, lib, mask


def _pair(kw, act, tril):
  """(ModelConfig, its perturbed parameters): the config's own initial values (sisua_amd.config.init_params -- the oracle's,
  tests/test_abi.py) moved off the symmetric point as tests/util.py::perturbed_params moves the oracle's (same scale and seed, float32-
  representable, SCALE's full-covariance factors with off-diagonals that matter).  The oracle's Spec, which perturbed_params takes, does not
  accept every output kind and latent crossed here."""
  from sisua_amd.config import ModelConfig, init_params
  cfg = ModelConfig(latent_tril=tril, enc_activation=act, dec_activation=act, encl_activation=act, **kw)
  rng = np.random.default_rng(3)
  params = {k: (v + 0.05 * rng.normal(size=v.shape)).astype(np.float32) for k, v in init_params(cfg).items()}
  if cfg.scale_tril:
    params["prior/scale"] = (params["prior/scale"] + 0.3 * rng.normal(size=params["prior/scale"].shape)).astype(np.float32)
  return cfg, params


def _train_and_audit(e, n_cells, batch, where, eval_too=False, clipnorm=None):
  """Three eager steps on different rows (the second a ragged batch below max_batch), three more through train_steps(graph=True); finite
  losses, no NaN flag; then the audit of every buffer.  clipnorm: the case's per-tensor bound, which has to bind -- the largest gradient
  norm of the first step (before clipping) lies above it."""
  rng = np.random.default_rng(7)
  sizes = [batch, max(batch - 37, 5), batch]
  for s, b in enumerate(sizes):
    rows = rng.choice(n_cells, size=b, replace=False).astype(np.int32)
    m = e.train_step(rows)
    assert m["nan_flag"] == 0 and np.isfinite(m["loss"]), (where, "eager step", s, m)
    if s == 0 and clipnorm is not None:
      assert m["grad_norm_max"] > clipnorm, (where, "the clipnorm does not bind", m["grad_norm_max"], clipnorm)
  order = np.concatenate([rng.permutation(n_cells)[:batch] for _ in range(3)]).astype(np.int32)
  m = e.train_steps(order, 3, batch, graph=True, metrics=True)
  assert m["nan_flag"] == 0, (where, "graph steps", m)
  h = e.metrics_history(3)["loss"]
  assert np.isfinite(h).all(), (where, h)
  _assert_clean(e, where=where)
  if eval_too:
    rows = np.arange(11, 11 + min(batch, 50), dtype=np.int32)
    assert np.isfinite(e.eval_step(rows)["loss"]), where
    _assert_clean(e, (4, 0), where + " / eval_step")
    e.forward_samples(3, row_ids=rows)
    _assert_clean(e, (4, 0), where + " / forward_samples")
    mllk, llk = e.marginal_llk(row_ids=rows, n_samples=6)
    assert np.isfinite(mllk).all() and np.isfinite(llk).all(), where
    _assert_clean(e, (4, 0), where + " / marginal_llk")


def test_the_design_covers_every_pair_and_few_cases_are_refusals():
  """(no device work: the case list alone)"""
  seen = set()
  for c in CASES:
    seen |= _pairs(c)
  keys = list(FACTORS)
  for a, b in itertools.combinations(keys, 2):
    for u in FACTORS[a]:
      for v in FACTORS[b]:
        assert ((a, u), (b, v)) in seen, (a, u, b, v)
  # a refused case holds one reason only, and every refusable pair stands in a case refused for THAT reason
  assert all(len(refusals(c)) <= 1 for c in CASES)
  want = {("config", m) for m in FACTORS["model"] if m not in TRIL_MODELS}
  want |= {("create", m, o) for m in ("scvi_full", "scvi_share") for o in FACTORS["out"] if o not in ("nbd", "zinbd")}
  want |= {("draws", m) for m in ("fvae", "semifvae")}
  got = {(refusal(c)[0], c["model"]) + ((c["out"],) if refusal(c)[0] == "create" else ()) for c in CASES if refusal(c)}
  assert got == want, got ^ want
  n_ref = sum(1 for c in CASES if refusal(c))
  assert n_ref == len(want) == 18 and 10 * n_ref <= len(CASES), (n_ref, len(CASES))
  assert CASES == covering_cases()   # deterministic


# three accepted cases go on to eval_step / forward_samples / marginal_llk, where the stacked evaluation decoder of smx_score.hip runs:
# the first under each of these activations with a diagonal latent on a model and output that take the stacked form (smx_predict.hip:
# stacked_scoring_ok -- not the deterministic dca, SCALE's full-covariance or mixture-density forms, nor a one-plane output)
EVAL_TOO = tuple(next(i for i, c in enumerate(CASES) if not refusal(c) and c["act"] == a and c["latent"] == "diag" and
                      c["model"] in ("vae", "sisua", "misa", "scale_diag", "scvi_full", "scvi_share") and c["out"] not in ("mse", "bernoulli"))
                 for a in ("sigmoid", "softplus", "tanh"))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[_case_id(i, c) for i, c in enumerate(CASES)])
def test_crossed_options_keep_the_padding_zero(Engine, i):
  from sisua_amd._hip import SmxError
  c = CASES[i]
  kw = case_kwargs(i, c)
  why = refusal(c)
  if why and why[0] == "config":
    with pytest.raises(ValueError, match=why[1]):
      _pair(kw, c["act"], True)
    return
  cfg, params = _pair(kw, c["act"], c["latent"] == "mvntril")
  if why and why[0] == "create":
    with pytest.raises(SmxError, match=why[1]):
      Engine(cfg, max_batch=100, init=False)
    return
  x, ys, lib, mask = _data(kw)
  e = Engine(cfg, max_batch=100, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=BASE)
  if why:
    with pytest.raises(SmxError, match=why[1]):
      e.set_train_draws(c["draws"])
    e.close()
    return
  e.set_optimizer(c["opt"], **OPTIMIZERS[c["opt"]])
  if c["draws"] > 1:
    e.set_train_draws(c["draws"])
  if c["sched"]:
    e.set_schedule("beta", I.linear(vmin=0.2, vmax=1.5, norm=3))
    e.set_schedule("lr", {"class_name": "ExponentialDecay", "config": dict(initial_learning_rate=2e-3, decay_steps=2, decay_rate=0.5)})
  _train_and_audit(e, N_CELLS, 100, _case_id(i, c), eval_too=i in EVAL_TOO, clipnorm=kw.get("clipnorm"))
  e.close()


# wide panels: the one-launch head on and off, the background head sweep, the compact stores -- every pair of (panel, batch, activation)
# with a flag setting and with a store, and of a flag setting with a store (a 4 x 3 Latin arrangement: 12 of the 36 combinations)
WIDE_SHAPES = [(4100, 100, "sigmoid"), (4500, 128, "relu"), (4500, 100, "sigmoid"), (4100, 128, "relu")]
WIDE_FLAGS = [(), ("head_fused",), ("head_sweep",)]
WIDE_STORES = ["f32", "u16", "csr"]
WIDE = [WIDE_SHAPES[g] + (WIDE_FLAGS[j], WIDE_STORES[(j + g) % 3]) for g in range(4) for j in range(3)]


@functools.lru_cache(maxsize=None)
def _wide_counts(G):
  return synth_counts(N_CELLS, G, sparsity=0.9, seed=0)


@pytest.mark.parametrize("G,batch,act,flags,storage", WIDE)
def test_wide_panels_keep_the_padding_zero(Engine, G, batch, act, flags, storage):
  kw = dict(model="vae", n_genes=G, likelihood="zinb" if G == 4100 else "nb", enc_units=(128,), dec_units=(128,), latent_dim=10,
            dropout_enc=0.0, dropout_dec=0.1)
  cfg, params = _pair(kw, act, False)
  x = _wide_counts(G)
  e = Engine(cfg, max_batch=128, init=False)
  e.set_params(params)
  e.upload(x, cell_id_base=BASE, storage=storage)
  for f in flags:
    e.set_flag(f, False)
  if not flags:
    assert e.head_fused_bytes(batch) > 0   # (the one-launch head is what runs)
  _train_and_audit(e, N_CELLS, batch, f"wide {G} batch {batch} {act} {flags} {storage}")
  e.close()


# the BatchNorm launch forms by batch size: 8 and 16 rows per lane, and the generic form
@pytest.mark.parametrize("batch", [300, 1100])
def test_large_batches_keep_the_padding_zero(Engine, batch):
  kw = dict(model="vae", n_genes=203, likelihood="zinb", enc_units=(48, 40), dec_units=(40,), latent_dim=10, **DROP)
  cfg, params = _pair(kw, "softplus", False)
  n = 1400
  x, ys, lib, mask = _data(kw, n)
  e = Engine(cfg, max_batch=batch, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=BASE)
  _train_and_audit(e, n, batch, f"batch {batch}")
  e.close()


# every flag of tests/test_gpu_step.py::test_separate_launch_forms_match_oracle switched off, one at a time
@pytest.mark.parametrize("flag", ["head_loss", "front", "bwd_front", "head_bwd", "wgrad"])
@pytest.mark.parametrize("bnorm", [True, False])
def test_separate_launch_forms_keep_the_padding_zero(Engine, flag, bnorm):
  kw = dict(model="vae", n_genes=203, likelihood="zinb", enc_units=(48, 40), dec_units=(40,), latent_dim=10, batchnorm=bnorm, **DROP)
  cfg, params = _pair(kw, "sigmoid", False)
  x, ys, lib, mask = _data(kw)
  e = Engine(cfg, max_batch=100, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=BASE)
  e.set_flag(flag, False)
  _train_and_audit(e, N_CELLS, 100, f"flag {flag} off, batchnorm {bnorm}", eval_too=True)
  e.close()


# the stacked scoring decoder's three forms of its last layer: the bf16 split (up to 128 decoder columns), the k-major f32 form the wider
# heads read (a last layer beyond 128 columns), and scvi's row-major one
@pytest.mark.parametrize("model,dec_units", [("vae", (150,)), ("vae", (40, 150)), ("vae", (40,)), ("scvi", (40,))])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
def test_scoring_forms_keep_the_padding_zero(Engine, model, dec_units, act):
  kw = dict(model=model, n_genes=203, likelihood="zinbd" if model == "scvi" else "zinb", enc_units=(48, 40), dec_units=dec_units, latent_dim=10, **DROP)
  if model == "scvi":
    kw.update(encl_units=(17,))
  cfg, params = _pair(kw, act, False)
  x, ys, lib, mask = _data(kw)
  e = Engine(cfg, max_batch=100, init=False)
  e.set_params(params)
  e.upload(x, ys, lib, mask, cell_id_base=BASE)
  _train_and_audit(e, N_CELLS, 100, f"scoring forms {model} {dec_units} {act}", eval_too=True)
  rows = np.arange(5, 55, dtype=np.int32)
  assert np.isfinite(e.score_llk([None, x[rows]], row_ids=rows, n_samples=4)).all()
  _assert_clean(e, (4, 0), where=f"score_llk {model} {dec_units} {act}")
  e.close()


@pytest.mark.parametrize("opt_shard", [False, True])
@pytest.mark.parametrize("sync_bn", [False, True])
def test_data_parallel_loopback_keeps_the_padding_zero(Engine, sync_bn, opt_shard):
  from tests.test_gpu_dp import run_ranks
  kw = dict(model="vae", n_genes=203, likelihood="zinb", enc_units=(48, 40), dec_units=(40,), latent_dim=10, **DROP)
  cfg, params = _pair(kw, "sigmoid", True)
  x, ys, lib, mask = _data(kw, 400)
  world, B, steps = 2, 50, 3
  engines = [_engine(Engine, cfg, params, x, ys, lib, mask, max_batch=64) for _ in range(world)]
  Engine.comm_init_local(engines)
  for e in engines:
    e.set_sync_bn(sync_bn)
    if opt_shard:
      e.set_flag("opt_shard", True)
      assert e.comm_form == 2   # (the flag takes the chained form)
  rng = np.random.default_rng(5)
  orders = [rng.permutation(x.shape[0])[: B * steps].astype(np.int32) for _ in range(world)]
  outs = run_ranks([lambda r=r: engines[r].train_steps(orders[r], steps, B, graph=False, metrics=True) for r in range(world)])
  for r in range(world):
    assert outs[r]["nan_flag"] == 0 and np.isfinite(engines[r].metrics_history(steps)["loss"]).all(), r
  if opt_shard:
    from sisua_amd._hip import SmxError
    with pytest.raises(SmxError):   # (the heads' moments are stale until gathered: smx_get_tensor's rule)
      engines[0].pad_audit(2)
    run_ranks([lambda r=r: engines[r].opt_gather() for r in range(world)])
  for r in range(world):
    _assert_clean(engines[r], where=f"rank {r}, sync_bn {sync_bn}, opt_shard {opt_shard}")
  for e in engines:
    e.close()


# ---- c. parity with the float64 oracle where the padding matters numerically -----------------------------------------------------------
RAGGED = dict(model="vae", n_genes=203, likelihood="zinb", enc_units=(48, 40), dec_units=(40,), latent_dim=10, **DROP)


@pytest.mark.parametrize("bnorm", [True, False])
@pytest.mark.parametrize("act", GENERAL)
def test_one_step_ragged_widths(Engine, monkeypatch, act, bnorm):
  ref.install(monkeypatch, enc=act, dec=act)
  spec, cfg, x, ys, lib, mask = _problem(dict(RAGGED, batchnorm=bnorm), act, act)
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  rows = np.random.default_rng(1).choice(x.shape[0], size=100, replace=False).astype(np.int32)
  res = so.train_step(spec, params, bn, opt, x[rows], so.PhiloxNoise(spec.seed, 0, rows + BASE), y=[y[rows] for y in ys], library=lib[rows],
                      mask=mask[rows])
  m = e.train_step(rows)
  _check_step(e, m, res, spec, bn, opt)
  _assert_clean(e, where=f"one step {act} batchnorm {bnorm}")
  e.close()


def _trajectory(Engine, monkeypatch, act, bnorm, dec_units=(40,), oracle=True):
  """20 steps at the ragged shape; with the oracle stepped beside the engine, loss and parameters are held to test_trajectory's bounds."""
  ref.install(monkeypatch, enc=act, dec=act)
  spec, cfg, x, ys, lib, mask = _problem(dict(RAGGED, batchnorm=bnorm, dec_units=dec_units), act, act)
  params = perturbed_params(spec)
  bn, opt = so.init_bn_state(spec), so.init_opt_state(params)
  e = _engine(Engine, cfg, params, x, ys, lib, mask)
  rng = np.random.default_rng(4)
  for s in range(20):
    rows = rng.choice(x.shape[0], size=64, replace=False).astype(np.int32)
    m = e.train_step(rows)
    assert m["nan_flag"] == 0
    if oracle:
      res = so.train_step(spec, params, bn, opt, x[rows], so.PhiloxNoise(spec.seed, s, rows + BASE))
      assert np.isclose(m["loss"], res["metrics"]["loss"], rtol=1e-3, atol=1e-3), (s, m["loss"], res["metrics"]["loss"])
  if oracle:
    worst = grad_errors(e.get_params(0), params)
    assert max(worst.values()) < 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
  _assert_clean(e, where=f"trajectory {act} batchnorm {bnorm}")
  return e, spec, x, lib


@pytest.mark.parametrize("bnorm", [True, False])
@pytest.mark.parametrize("act", ["sigmoid", "softplus"])
def test_trajectory_ragged_widths(Engine, monkeypatch, act, bnorm):
  e, _, _, _ = _trajectory(Engine, monkeypatch, act, bnorm)
  e.close()


@pytest.mark.parametrize("dec_units", [(40,), (33, 17)])
@pytest.mark.parametrize("stacked", [True, False])
def test_scores_after_a_trajectory(Engine, monkeypatch, dec_units, stacked):
  """marginal_llk and the posterior log-likelihood of the model the 20 steps left (its parameters and moving statistics read back),
  against the oracle's; tolerances of tests/test_gpu_activations.py::test_marginal_and_posterior_llk."""
  e, spec, x, lib = _trajectory(Engine, monkeypatch, "sigmoid", True, dec_units, oracle=False)
  params = {k: v.astype(np.float64) for k, v in e.get_params(0).items()}
  names = [p for p, _ in so.bn_manifest(spec)]
  bn = {}
  for i, st in e.get_bn().items():
    bn[f"{names[i]}/moving_mean"] = st["moving_mean"].astype(np.float64)
    bn[f"{names[i]}/moving_var"] = st["moving_var"].astype(np.float64)
  if not stacked:
    e.set_flag("stacked_scoring", False)
  rows = np.arange(20, 70, dtype=np.int32)
  S = 12
  ref_m, ref_l = so.marginal_log_prob(spec, params, bn, x[rows], rows + BASE, S, library=lib[rows])
  got_m, got_l = e.marginal_llk(row_ids=rows, n_samples=S)
  assert np.allclose(got_m, ref_m, rtol=RTOL, atol=1e-3), np.abs(got_m - ref_m).max()
  assert np.allclose(got_l, ref_l, rtol=RTOL, atol=1e-3)
  _assert_clean(e, (4, 0), where=f"marginal_llk decoder {dec_units} stacked {stacked}")
  sc = e.score_llk([None], row_ids=rows, n_samples=S)
  assert np.isfinite(sc).all()
  _assert_clean(e, (4, 0), where=f"score_llk decoder {dec_units} stacked {stacked}")
  e.close()
