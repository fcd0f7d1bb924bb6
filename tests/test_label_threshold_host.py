"""Host side of ProbabilisticEmbedding (sisua_amd/label_threshold.py, SingleCellOMIC.probabilistic_embedding) without a GPU: the float64
restatement (tests/gmm_ref.py) against what the reference's own code and scikit-learn computed (tests/golden/gmm_fixture.npz, made by
tests/golden/make_gmm_fixtures.py), the guards that make the equalities of tests/test_gpu_label_threshold.py legitimate, the argument
checks, and the host logic of the data layer.

Normalisation.  The reference sums a column in float32 (NumPy's pairwise sum), the restatement and the device in float64 in cell order.
Where both give the same float32 denominator fl32(s + eps) the float32 argument of the log1p is bit-equal; where they differ (by one
float32 ulp of the sum) the argument agrees to 1 float32 ulp.  The test prints which case every fixture column is.

Quality of the optimum.  The restatement's best lower bound of 8 random-cell starts is >= scikit-learn's lower_bound_ (k-means starts) - tol,
tol = 1e-3 being the stop rule's own resolution: both loops stop inside it."""
import os
import pickle

import numpy as np
import pytest

from tests import gmm_ref as G

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmm_fixture.npz")
SETS = list(G.FIXTURE_SETS)
TOL = 1e-3


@pytest.fixture(scope="module")
def fx():
  with np.load(FIXTURE) as f:
    return {k: f[k] for k in f.files}


_OURS = {}


def _ours(fx, s, K):
  """the restatement's fit of a fixture set with the host's seeding: made once"""
  if (s, K) not in _OURS:
    X = fx[f"{s}_X"]
    _OURS[s, K] = G.fit(X, G.draw_init_raw(X, K, 8, 8))
  return _OURS[s, K]


@pytest.mark.parametrize("s", SETS)
def test_normalisation_is_the_reference(fx, s):
  X = fx[f"{s}_X"]
  assert np.array_equal(X, G.fixture_matrix(s))
  for c in range(X.shape[1]):
    tv = G.training_vector(X[:, c])
    s64 = G.column_sum(X[:, c])
    arg, ref = G.log_norm_argument(tv, s64), fx[f"{s}_c{c}_arg"]
    assert arg.dtype == np.float32 and ref.dtype == np.float32 and arg.shape == ref.shape
    same_den = np.float32(s64 + float(G.EPS32)) == np.float32(fx[f"{s}_c{c}_sum32"] + G.EPS32)
    ulps = np.abs(arg.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max()
    print(f"{s} column {c}: float64 sum {s64!r}, float32 sum {float(fx[f'{s}_c{c}_sum32'])!r}: "
          f"{'the same denominator' if same_den else 'denominators one float32 ulp apart'}, argument off by at most {ulps} ulp")
    assert ulps == 0 if same_den else ulps <= 1
    # and the normalised vector itself, which the reference holds in float32
    t = G.normalize(X[:, c])
    assert np.max(np.abs(t - fx[f"{s}_c{c}_train"])) <= 2.0 ** -23 * max(1.0, float(t.max())) * 2


@pytest.mark.parametrize("K", G.FIXTURE_K)
@pytest.mark.parametrize("s", SETS)
def test_best_lower_bound_against_scikit_learn(fx, s, K):
  ours = _ours(fx, s, K)
  for c in range(2):
    best, theirs = float(ours["lower_bound"][c, ours["best"][c]]), float(fx[f"{s}_K{K}_lower_bound"][c])
    print(f"{s} K = {K} column {c}: best of 8 random-cell starts {best!r}, scikit-learn {theirs!r}, ours - theirs {best - theirs:+.3e}")
    assert best >= theirs - TOL, (s, K, c, best, theirs)


def test_distance_to_scikit_learn_at_two_components(fx):
  """What DESIGN.md 4n quotes: at K = 2 the sorted means against scikit-learn's and the share of cells with the same y_bin.  Both runs stop
  inside tol of their optimum, so the means may differ by what a change of tol in the lower bound allows: asserted at 5e-3, measured far
  inside."""
  worst, same, cells = 0.0, 0, 0
  for s in SETS:
    ours, X = _ours(fx, s, 2), fx[f"{s}_X"]
    d = np.abs(np.sort(ours["means"], axis=1).T - fx[f"{s}_K2_means"]).max()
    bins = G.predict(X, ours["weights"], ours["means"], ours["variances"])[1]
    same, cells, worst = same + int((bins == fx[f"{s}_K2_y_bin"]).sum()), cells + bins.size, max(worst, float(d))
  print(f"K = 2: largest distance of sorted means to scikit-learn {worst:.3e}; y_bin equal on {same} of {cells} cells ({same / cells:.4%})")
  assert worst <= 5e-3 and same / cells >= 0.99


@pytest.mark.parametrize("name", list(G.DATASETS))
def test_guards_of_the_device_equalities(name):
  """n_iter, converged, best and y_bin have one answer only where nothing sits on a decision boundary: asserted on the restatement, at
  1e-9, four decades above the summation noise the device tests allow"""
  X, _, kw = G.dataset(name)
  f = G.fitted(name)
  for c, runs in enumerate(f["traces"]):
    for tr in runs:
      steps = np.abs(np.diff(np.concatenate([[-np.inf], tr])))
      assert np.min(np.abs(steps - TOL)) > 1e-9, (name, c)
    lb = np.sort(f["lower_bound"][c])[::-1]
    gaps = lb[:-1] - lb[1:]
    assert np.all((gaps > 1e-9) | (gaps == 0.0)), (name, c, gaps)
  _, _, _, T, thr = G.predict(X, f["weights"], f["means"], f["variances"], log_norm=kw["log_norm"])
  assert np.min(np.abs(T - thr[None, :])) > 1e-9, name


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
  from sisua_amd import _hip

  def no_device(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", no_device)


def test_fit_argument_checks_come_before_the_device(monkeypatch):
  from sisua_amd.engine import k_gmm1d_fit
  _no_device(monkeypatch)
  X, seeds, _ = G.dataset("n1000")   # [1000, 3], seeds [3, 8, 3]
  neg, nan, zero = X.copy(), X.copy(), X.copy()
  neg[5, 1], nan[7, 2], zero[:, 1] = -1.0, np.nan, 0.0
  bad = [dict(X=X[:, 0], init_raw=seeds), dict(X=np.ones((4, 4097), np.float32), init_raw=np.ones((4097, 1, 2), np.float32)),
         dict(X=X, init_raw=seeds[:2]), dict(X=X, init_raw=seeds[:, :, :1]), dict(X=X, init_raw=np.ones((3, 8, 9), np.float32)),
         dict(X=X, init_raw=seeds[:, :0]), dict(X=X, init_raw=np.ones((3, 65, 3), np.float32)), dict(X=X, init_raw=seeds[0]),
         dict(X=X, init_raw=seeds, max_iter=0), dict(X=X, init_raw=seeds, tol=0.0), dict(X=X, init_raw=seeds, tol=np.nan),
         dict(X=X, init_raw=seeds, reg_covar=-1e-6), dict(X=neg, init_raw=seeds), dict(X=nan, init_raw=seeds), dict(X=X, init_raw=-seeds),
         dict(X=X[:2], init_raw=seeds), dict(X=np.zeros((0, 3), np.float32), init_raw=seeds)]
  for kw in bad:
    with pytest.raises(ValueError):
      k_gmm1d_fit(**kw)
  with pytest.raises(ValueError, match="column 1 has 1 training"):   # an all-zero column: one synthetic sample
    k_gmm1d_fit(zero, seeds)


def test_predict_argument_checks_come_before_the_device(monkeypatch):
  from sisua_amd.engine import k_gmm1d_predict
  _no_device(monkeypatch)
  X = G.dataset("n1000")[0]
  w, m, v = np.full((3, 2), 0.5), np.tile([1.0, 3.0], (3, 1)), np.ones((3, 2))
  order, thr = np.tile([0, 1], (3, 1)), np.ones(3)
  ok = dict(X=X, weights=w, means=m, variances=v, order=order, positive_component=1, threshold=thr)
  bad = [dict(X=X[:, :2]), dict(positive_component=0), dict(positive_component=2), dict(order=np.zeros((3, 2), int)), dict(order=order[:2]),
         dict(threshold=np.array([1.0, np.nan, 1.0])), dict(threshold=thr[:2]), dict(variances=np.zeros((3, 2))), dict(weights=-w),
         dict(means=np.full((3, 2), np.inf)), dict(X=-X), dict(variances=v[:, :1]),
         dict(weights=np.ones((3, 9)), means=np.ones((3, 9)), variances=np.ones((3, 9)), order=np.tile(np.arange(9), (3, 1)))]
  for kw in bad:
    with pytest.raises(ValueError):
      k_gmm1d_predict(**{**ok, **kw})


def test_embedding_argument_checks_come_before_the_device(monkeypatch):
  from sisua_amd import ProbabilisticEmbedding
  from sisua_amd.data import SingleCellOMIC
  _no_device(monkeypatch)
  X = G.dataset("n1000")[0]
  for kw in (dict(clip_quartile=1.5), dict(n_components_per_class=1), dict(n_components_per_class=9), dict(positive_component=0),
             dict(positive_component=2), dict(ci_threshold=1.5), dict(n_init=0), dict(n_init=65), dict(max_iter=0), dict(tol=0.0),
             dict(reg_covar=-1.0)):
    with pytest.raises(ValueError):
      ProbabilisticEmbedding(**kw)
  pbe = ProbabilisticEmbedding()
  zero, neg = X.copy(), X.copy()
  zero[:, 2], neg[0, 0] = 0.0, -2.0
  with pytest.raises(ValueError, match="column 2"):
    pbe.fit(zero)
  for x in (neg, X[:, 0], X[:1]):
    with pytest.raises(ValueError):
      pbe.fit(x)
  with pytest.raises(ValueError, match="not fitted"):
    pbe.predict(X)
  fitted = ProbabilisticEmbedding.from_parameters(np.full((3, 2), 0.5), np.tile([1.0, 3.0], (3, 1)), np.ones((3, 2)))
  with pytest.raises(ValueError, match="mis-match"):
    fitted.predict_proba(X[:, :2])
  sco = SingleCellOMIC(np.ones((1000, 5), np.float32)).add_omic("proteomic", X)
  with pytest.raises(TypeError):
    sco.probabilistic_embedding("proteomic", pbe="a mixture")
  with pytest.raises(ValueError, match="not built"):
    sco.probabilistic_embedding("proteomic", clip_quartile=1.5)
  sco.add_omic("bad", neg)
  with pytest.raises(ValueError):
    sco.probabilistic_embedding("bad")


# ---- host logic ----------------------------------------------------------------------------------------------------------------------
def _fitted_embedding(name="n1000"):
  from sisua_amd import ProbabilisticEmbedding
  f = G.fitted(name)
  return ProbabilisticEmbedding.from_parameters(f["weights"], f["means"], f["variances"], n_init=8), f


def test_seeding_is_the_restatements():
  from sisua_amd import label_threshold as L
  for name in ("n1000", "keep", "raw"):
    X, seeds, kw = G.dataset(name)
    got = L.draw_init_raw(X, kw["K"], kw["R"], 8, kw["remove_zeros"])
    assert got.dtype == np.float32 and np.array_equal(got, seeds)
  assert not np.array_equal(L.draw_init_raw(X, 3, 8, 9), L.draw_init_raw(X, 3, 8, 8))
  assert np.array_equal(L.training_vector(np.array([0, 3, 0, 2], np.float32)), [0, 3, 2])
  assert np.array_equal(L.training_vector(np.array([1, 3], np.float32)), [1, 3])
  assert np.array_equal(L.training_vector(np.array([0, 3, 0, 2], np.float32), remove_zeros=False), [0, 3, 0, 2])


def test_properties_and_threshold_of_a_fitted_object():
  from scipy import stats
  pbe, f = _fitted_embedding()
  order = np.argsort(f["means"], axis=1)
  assert pbe.n_classes == 3 and pbe.means.shape == (3, 3)
  assert np.array_equal(pbe.means, np.sort(f["means"], axis=1).T)
  assert np.array_equal(pbe.precisions, (1.0 / np.take_along_axis(f["variances"], order, 1)).T)
  for c in range(3):   # the reference's stats.norm.interval
    k = order[c, 1]
    lo, hi = stats.norm.interval(0.68, loc=f["means"][c, k], scale=np.sqrt(f["variances"][c, k]))
    assert abs(pbe.thresholds[c] - lo) <= 1e-12 * abs(lo)
    pbe.ci_threshold = 0.68
    assert abs(pbe.thresholds[c] - hi) <= 1e-12 * abs(hi)
    pbe.ci_threshold = -0.68
  assert np.allclose(pbe.thresholds, G.thresholds(f["means"], f["variances"], order), rtol=1e-15)


def test_pickle_round_trip_holds_numpy_only():
  pbe, _ = _fitted_embedding()
  back = pickle.loads(pickle.dumps(pbe))
  assert set(back._fit) == set(pbe._fit) and all(type(v) is np.ndarray for v in back._fit.values())
  assert all(np.array_equal(back._fit[k], pbe._fit[k]) for k in pbe._fit)
  assert np.array_equal(back.means, pbe.means) and np.array_equal(back.thresholds, pbe.thresholds)
  plain = (int, float, bool, type(None), dict)
  assert all(isinstance(v, plain) for v in vars(back).values())


class _Stub:
  """a fitted embedding whose device calls are replaced by given results"""

  def __new__(cls, prob, bins):
    from sisua_amd import ProbabilisticEmbedding

    class Canned(ProbabilisticEmbedding):
      fits = 0

      def fit(self, X):
        Canned.fits += 1
        return self

      def predict_proba(self, X):
        return prob

      def predict(self, X):
        return bins
    return Canned


def test_data_layer_binary_shortcut_clip_and_cache(monkeypatch):
  import scipy.sparse as sp
  from sisua_amd import label_threshold
  from sisua_amd.data import SingleCellOMIC
  _no_device(monkeypatch)
  rs = np.random.RandomState(0)
  genes = rs.poisson(1.0, size=(50, 7)).astype(np.float32)
  onehot = np.eye(4, dtype=np.float32)[rs.randint(0, 4, 50)]
  sco = SingleCellOMIC(genes).add_omic("celltype", onehot)
  pbe, prob, bins = sco.probabilistic_embedding("celltype")   # 0 / 1 only: its own embedding, no mixture, no device
  assert pbe is None and np.array_equal(prob, onehot) and np.array_equal(bins, onehot)
  assert np.array_equal(sco.get_x_probs("celltype"), onehot) and np.array_equal(sco.get_x_bins("celltype"), onehot)
  # the clip and the cache, with the device calls canned
  levels = rs.gamma(2.0, 2.0, size=(50, 3)).astype(np.float32)
  raw_prob = np.linspace(0.0, 1.0, 150).reshape(50, 3)
  raw_bin = (raw_prob > 0.5).astype(np.float32)
  Canned = _Stub(raw_prob, raw_bin)
  monkeypatch.setattr(label_threshold, "ProbabilisticEmbedding", Canned)
  sco.add_omic("proteomic", sp.csr_matrix(levels))   # (sparse storage: densified for the call)
  pbe, prob, bins = sco.probabilistic_embedding("proteomic", seed=3)
  assert isinstance(pbe, Canned) and pbe.random_state == 3 and Canned.fits == 1
  assert prob.min() == 1e-8 and prob.max() == 1 - 1e-8 and np.array_equal(prob[1:-1], raw_prob[1:-1]) and np.array_equal(bins, raw_bin)
  again = sco.probabilistic_embedding("proteomic")
  assert again[0] is pbe and again[1] is prob and again[2] is bins and Canned.fits == 1   # cached
  assert sco.get_x_probs("proteomic") is prob and sco.get_x_bins("proteomic") is bins
  assert sco.probabilistic_embedding()[0] is not pbe   # omic=None: the first omic, fitted on its own
  assert Canned.fits == 2
  # a subset and a copy start without; a given pbe is used without fitting; replacing the omic drops its entry
  for other in (sco[np.arange(10)], sco.copy()):
    assert other._embeddings == {}
  sub = sco.copy()
  given = Canned()
  got = sub.probabilistic_embedding("proteomic", pbe=given)
  assert got[0] is given and Canned.fits == 2
  sco.add_omic("proteomic", levels)
  assert "proteomic" not in sco._embeddings
  with pytest.warns(UserWarning, match="100 GMM"):
    SingleCellOMIC(np.full((5, 100), 2.0, np.float32)).probabilistic_embedding(pbe=given)


def test_abi_and_sources():
  from sisua_amd import _hip, build
  assert _hip.SMX_ABI_VERSION >= 9 and "smx_gmm.hip" in build.SOURCES
  assert {"smx_gmm1d_fit", "smx_gmm1d_predict"} <= set(_hip.SIGNATURES)
  import sisua_amd
  assert sisua_amd.ProbabilisticEmbedding is __import__("sisua_amd.label_threshold", fromlist=["x"]).ProbabilisticEmbedding
