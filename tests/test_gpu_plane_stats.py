"""predict()'s gene-output statistics (smx_predict_stat: plane_moments, rv_moments, plane_stat_kernel, plane_stat_rv_kernel and the two
plane_logprob kernels of sisua_amd/csrc/smx_predict.hip) against the float64 reference of tests/plane_stat_ref.py at saturated planes.

The planes of the gene output are d @ out/W + out/b.  With out/W = 0 and out/b = the edge grid, gene g of every cell sits at grid point g
whatever the cell; everything else keeps its initial value.  The planes are read back (Engine.predict's x_params) and the read-back
float32 values feed the reference, so nothing upstream of the statistic kernels enters a comparison.  Tiny models (one hidden layer of
32, latent_dim 6, max_batch 4), 5 cells (a full minibatch and a ragged one), 2 draws, 1030 genes: the grid's kept points first, moderate
points behind them -- no multiple of 4, more than four 256-gene tiles.  SCVI 'zinbd' takes the `direct` path: its rate comes out of the
row softmax and the library, the extremes sit in its shared dispersion and gate vectors.

Bounds: plane_stat_ref's derived ones (its docstring has the table), `mos_bound` of test_gpu_predict_draw_passes for the average over
the draws.  Every test prints the worst error / bound per statistic; DESIGN.md 4r records them as read on an MI355X.

Before the repair of plane_moments / rv_moments (1 - pi and p (1 - p) taken in float32) the mean and variance tests failed at every
gate logit >= 8 and every Bernoulli logit >= 8: see DESIGN.md 4r for the figures."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import plane_stat_ref as R
from tests.test_gpu_predict_draw_passes import draws_per_pass, mos_bound

pytestmark = pytest.mark.gpu

G, N, BATCH, S = R.G_GRID, 5, 4, 2
_NET = dict(n_genes=G, enc_units=(32,), dec_units=(32,), latent_dim=6)
CASES = {   # name -> (kind, configuration)
    "nb": ("nb", dict(model="vae", likelihood="nb", **_NET)),
    "zinb": ("zinb", dict(model="vae", likelihood="zinb", **_NET)),
    "nbd": ("nbd", dict(model="vae", likelihood="nbd", **_NET)),
    "zinbd": ("zinbd", dict(model="vae", likelihood="zinbd", **_NET)),
    "bernoulli": ("bernoulli", dict(model="vae", likelihood="bernoulli", **_NET)),
    "normal": ("normal", dict(model="vae", likelihood="normal", log_norm=False, **_NET)),
    "mse": ("mse", dict(model="vae", likelihood="mse", log_norm=False, **_NET)),
    "scvi_zinbd": ("zinbd", dict(model="scvi", likelihood="zinbd", encl_units=(16,), dispersion="share", inflation="share", **_NET)),
}
LIB = np.tile(np.array([[6.0, 0.5]], np.float32), (N, 1))


def _scvi_bias():
  """{tensor: value}: the head of the rate silenced (its bias a smooth moderate profile), dispersion bias x gate on the shared vectors"""
  pts = R.grid_points("zinbd", scvi=True)
  pad = np.array([(0.2, -0.5), (-0.4, 0.3), (0.6, 1.1)], np.float32)
  full = np.concatenate([pts] + [pad[[i % 3]] for i in range(G - len(pts))]).astype(np.float32)
  return {"out0/b": (1.5 * np.sin(np.arange(G) * 0.37)).astype(np.float32), "out1/b": full[:, 0].copy(), "out2/b": full[:, 1].copy()}


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


class Case:
  def __init__(self, name):
    from sisua_amd.config import ModelConfig
    from sisua_amd.engine import Engine
    self.name, (self.kind, kw) = name, CASES[name]
    self.scvi = kw["model"] == "scvi"
    self.lib = LIB if self.scvi else None
    self.e = Engine(ModelConfig(**kw), max_batch=BATCH)
    if self.scvi:
      self.bias = None
      self.e.set_params({"out0/W": np.zeros(self.e.shapes["out0/W"], np.float32), **_scvi_bias()})
    else:
      self.bias, _, _ = R.bias_grid(self.kind)
      self.e.set_params({"out/W": np.zeros(self.e.shapes["out/W"], np.float32), "out/b": self.bias.reshape(-1)})
    self.t = R.targets(self.kind)                  # the five target rows; also the input rows
    self.other = np.ascontiguousarray(self.t[::-1])   # another input, for the calls whose targets are given apart from it
    self._planes = {}
    self.sc = np.ones(N, np.int64) if self.scvi else draws_per_pass(N, BATCH, BATCH, S)   # scvi: one draw per decoder pass

  def planes(self, which="t"):
    """the read-back planes of the input `which` as a list of k arrays [S, N, G]"""
    if which not in self._planes:
      x = self.t if which == "t" else self.other
      p = self.e.predict(x, library=self.lib, n_samples=S, batch=BATCH)["x_params"]
      assert p.shape == (S, R.N_PLANES[self.kind], N, G) and p.dtype == np.float32
      self._planes[which] = [np.ascontiguousarray(p[:, c]) for c in range(p.shape[1])]
    return self._planes[which]

  def stat(self, stat, x=None, **kw):
    return self.e.predict_stat(self.t if x is None else x, stat, library=self.lib, n_samples=S, batch=BATCH, **kw)


@pytest.fixture(scope="module")
def cases():
  from sisua_amd import build
  build.build(verbose=False)
  made = {}

  def get(name):
    if name not in made:
      made[name] = Case(name)
    return made[name]
  yield get
  for c in made.values():
    c.e.close()


def _report(label, err, bound):
  ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
  at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
  print(f"{label}: worst error / bound {float(ratio.max()):.3f} at {tuple(int(i) for i in at)}")
  return ratio, at


def _by_last_plane(planes, bad, rel):
  """{value of the last plane (the gate, the Bernoulli logit): (elements outside the bound, their worst relative error)}"""
  last = planes[-1]
  return {float(v): (int((bad & (last == v)).sum()), float(f"{rel[bad & (last == v)].max():.3g}")) for v in np.unique(last[bad])}


@pytest.mark.parametrize("name", [n for n in CASES if n != "scvi_zinbd"])
def test_planes_are_the_bias_bit_for_bit(cases, name):
  """d @ 0 + b = b exactly: every plane of every cell and draw is the bias vector"""
  c = cases(name)
  for which in ("t", "other"):
    for k, p in enumerate(c.planes(which)):
      assert np.isfinite(p).all()
      assert _same(p, np.broadcast_to(c.bias[k], p.shape)), (name, which, k, int((_bits(p) != _bits(np.broadcast_to(c.bias[k], p.shape))).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_mean_and_variance_on_the_grid(cases, name):
  """mean, variance and mean_over_samples, each also count_only, against float64 inside the derived relative bound at every point that
  satisfies the grid condition (all of them outside SCVI, whose rate is not ours to set: at most a tenth may fall out there); the
  genes= gather returns the bits of its columns"""
  c = cases(name)
  planes, direct = c.planes(), c.scvi
  ok = R.in_range(c.kind, planes, direct)
  print(f"{name}: {int((~ok).sum())} of {ok.size} elements outside the grid condition")
  assert ok.all() if not c.scvi else (~ok).sum() * 10 <= ok.size
  idx, failures = [0, 7, 300, 7, G - 1, 511, 512], []
  for count_only in ((False, True) if R.is_zi(c.kind) else (False,)):
    ref = dict(zip(("mean", "variance"), R.moments(c.kind, planes, direct, count_only)))
    got = {}
    for stat in ("mean", "variance"):
      got[stat] = c.stat(stat, count_only=count_only)
      assert got[stat].shape == (S, N, G) and got[stat].dtype == np.float32
      assert not (np.isnan(got[stat]) & np.isfinite(ref[stat])).any(), (name, stat)
      bound = R.stat_bound(c.kind, stat, planes, direct, count_only) * np.abs(ref[stat])
      err = np.where(ok, np.abs(got[stat].astype(np.float64) - ref[stat]), 0.0)
      ratio, at = _report(f"{name} count_only={count_only} {stat}", err, bound)
      bad = err > bound
      if bad.any():   # (every statistic is looked at before the test fails: the message names them all)
        failures.append((stat, count_only, int(bad.sum()), float(ratio.max()), [float(p[at]) for p in planes], float(got[stat][at]),
                         float(ref[stat][at]), _by_last_plane(planes, bad, err / np.abs(ref[stat]))))
        print(f"    OUTSIDE THE BOUND {failures[-1]}")
    mos = c.stat("mean_over_samples", count_only=count_only)
    assert mos.shape == (N, G) and mos.dtype == np.float32
    elem = (R.stat_bound(c.kind, "mean", planes, direct, count_only) * np.abs(ref["mean"])).mean(axis=0)
    bound = elem + mos_bound(got["mean"], c.sc)
    err = np.where(ok.all(axis=0), np.abs(mos.astype(np.float64) - ref["mean"].mean(axis=0)), 0.0)
    ratio, at = _report(f"{name} count_only={count_only} mean_over_samples", err, bound)
    if (err > bound).any():
      failures.append(("mean_over_samples", count_only, int((err > bound).sum()), float(ratio.max()), at))
      print(f"    OUTSIDE THE BOUND {failures[-1]}")
    assert _same(c.stat("mean_over_samples", count_only=count_only, genes=idx), mos[:, idx])
    assert _same(c.stat("mean_over_samples", x=sp.csr_matrix(c.t), count_only=count_only), mos)
  assert not failures, (name, failures)


@pytest.mark.parametrize("name", list(CASES))
def test_log_prob_on_the_grid(cases, name):
  """log_prob of the five target rows -- given as the input rows themselves, as a dense target and as a CSR target of another input --
  inside sum_g b_g + gamma sum_g |v_g|; the dense and the CSR target give the same bits"""
  c = cases(name)
  direct = c.scvi
  for count_only in ((False, True) if R.is_zi(c.kind) else (False,)):
    runs = {"input": (c.stat("log_prob", count_only=count_only), c.planes("t")),
            "dense": (c.stat("log_prob", x=c.other, target=c.t, count_only=count_only), c.planes("other")),
            "csr": (c.stat("log_prob", x=c.other, target=sp.csr_matrix(c.t), count_only=count_only), c.planes("other"))}
    assert _same(runs["dense"][0], runs["csr"][0])
    for way, (got, planes) in runs.items():
      assert got.shape == (S, N) and got.dtype == np.float32 and np.isfinite(got).all(), (name, way)
      ref = R.log_prob_elem(c.kind, c.t[None], planes, direct, count_only).sum(axis=-1)
      assert np.isfinite(ref).all() and (np.abs(ref) < R.F32_MAX).all()
      bound = R.logprob_bound(c.kind, c.t[None], planes, direct, count_only)
      err = np.abs(got.astype(np.float64) - ref)
      ratio, at = _report(f"{name} count_only={count_only} log_prob ({way})", err, bound)
      print(f"    per target row: worst error / bound {[round(float(v), 4) for v in ratio.max(axis=0)]}, bound / |ref| "
            f"{[float(f'{v:.2e}') for v in (bound / np.abs(ref)).max(axis=0)]}")
      assert (err <= bound).all(), (name, way, count_only, float(ratio.max()), at, float(got[at]), float(ref[at]))


def test_out_of_range_planes_give_no_nan(cases):
  """Outside the float32 range of the grid condition no relative bound holds, but a statistic whose reference is finite is not NaN: 'nbd'
  at the pre-activations (-110, -110) -- mean and dispersion both underflow, the reference variance is 2.7e-48 -- and (45, -50)."""
  c = cases("nbd")
  pts = np.array([(-110.0, -110.0), (45.0, -50.0)], np.float32)
  bias = c.bias.copy()
  bias[:, :2] = pts.T
  try:
    c.e.set_params({"out/b": bias.reshape(-1)})
    p = c.e.predict(c.t, n_samples=S, batch=BATCH)["x_params"]
    assert _same(p[:, :, :, :2], np.broadcast_to(pts.T[None, :, None, :], (S, 2, N, 2)))
    for stat in ("mean", "variance", "mean_over_samples"):
      got = c.stat(stat)[..., :2]
      m, v = R.moments("nbd", [pts[:, 0], pts[:, 1]])
      assert np.isfinite(m).all() and np.isfinite(v).all()
      print(f"nbd {stat} at (-110, -110), (45, -50): {got.reshape(-1, 2)[0]}, reference mean {m}, variance {v}")
      assert not np.isnan(got).any(), (stat, got)
  finally:
    c.e.set_params({"out/b": c.bias.reshape(-1)})


def test_model_route_gives_the_repaired_values(cases):
  """The route users take: SingleCellModel.predict on an array (the host distributions, float32) and on a SingleCellOMIC (LazyCountOutput,
  the kernels), one 'zinb' model whose output head is the grid: mean, variance and mean_over_samples, with and without the gate"""
  import sisua_amd.models as api
  from sisua_amd import distributions as D
  from sisua_amd.data import SingleCellOMIC
  c = cases("zinb")
  x = c.t.copy()
  x[0] = 2.0                                            # (no empty cell in a dataset)
  sco = SingleCellOMIC(x, name="toy")
  m = api.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), latents=api.RVmeta(6, "diag", True, "Latents"),
              encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  e = m._ensure_engine(64)
  try:
    e.set_params({"out/W": np.zeros(e.shapes["out/W"], np.float32), "out/b": c.bias.reshape(-1)})
    m._param_version = getattr(m, "_param_version", 0) + 1
    p = e.predict(x, n_samples=S, batch=BATCH)["x_params"]
    planes = [np.ascontiguousarray(p[:, k]) for k in range(3)]
    assert all(_same(pl, np.broadcast_to(c.bias[k], pl.shape)) for k, pl in enumerate(planes))
    eX, _ = m.predict(x, sample_shape=S, batch_size=BATCH, verbose=False)
    lX, _ = m.predict(sco, sample_shape=S, batch_size=BATCH, verbose=False)
    assert isinstance(lX, D.LazyCountOutput) and not isinstance(eX, D.LazyCountOutput)
    sc = draws_per_pass(N, BATCH, e.max_batch, S)
    for count_only, lazy, eager in ((False, lX, eX.distribution), (True, lX.count_distribution, eX.distribution.count_distribution)):
      ref = dict(zip(("mean", "variance"), R.moments("zinb", planes, False, count_only)))
      for stat in ("mean", "variance"):
        bound = R.stat_bound("zinb", stat, planes, False, count_only) * np.abs(ref[stat])
        for route, got in (("lazy", getattr(lazy, stat)()), ("eager", getattr(eager, stat)())):
          assert got.shape == (S, N, G) and got.dtype == np.float32, (route, stat, got.dtype)
          err = np.abs(got.astype(np.float64) - ref[stat])
          ratio, at = _report(f"model route {route} count_only={count_only} {stat}", err, bound)
          assert (err <= bound).all(), (route, stat, count_only, float(ratio.max()), [float(pl[at]) for pl in planes])
      mos, draws = lazy.mean_over_samples(), lazy.mean()
      bound = (R.stat_bound("zinb", "mean", planes, False, count_only) * np.abs(ref["mean"])).mean(axis=0) + mos_bound(draws, sc)
      err = np.abs(mos.astype(np.float64) - ref["mean"].mean(axis=0))
      ratio, at = _report(f"model route lazy count_only={count_only} mean_over_samples", err, bound)
      assert (err <= bound).all(), (count_only, float(ratio.max()))
      assert _same(lazy.mean_over_samples(genes=[300, 7, 7]), mos[:, [300, 7, 7]])
  finally:
    e.close()
    m._engine = None
