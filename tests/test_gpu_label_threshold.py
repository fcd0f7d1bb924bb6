"""ProbabilisticEmbedding on the device (smx_gmm.hip) against the float64 restatement tests/gmm_ref.py, at the smallest shapes that reach
every path: n_cells 257, 1000, 4096 | 4097 (one slice of the cells | two: the slice count is ceil(n_cells / 4096)) and 4099; 1, 3 and 13
columns; 2, 3 and 5 components; 1 and 8 restarts; columns without zeros, with 60 % zeros, constant, with fewer distinct values than
components; with and without log_norm and remove_zeros (tests.gmm_ref.DATASETS).

Equalities.  n_iter, converged, best, n_train and y_bin are EQUAL to the restatement's: tests/test_label_threshold_host.py asserts on the
restatement that no lower-bound step lies within 1e-9 of tol, no two restarts' lower bounds within 1e-9 of each other unless they are the
same number, and no cell within 1e-9 of its threshold.

Tolerance.  Weights, means, variances, lower bounds, y_prob and the per-sample scores are sums of N terms in another order than NumPy's: each
carries about N 2^-53 (1e-13 at N = 1000), through at most 120 iterations.  Measured on an MI355X over the sets of MAIN, the largest relative
deviation was MEASURED_RTOL = 7.2e-10 (DESIGN.md 4n has every figure); RTOL is 100 x that, and no looser than 1e-8: 1e-8.

`const_log`: a constant column under log_norm.  The variance of its one live component is reg_covar plus the rounding residue of
sum t^2 / n - mean^2, whose true value is 0: the condition number is t^2 / reg_covar (1e7 here), so the residue of ANY order of summation is
of the order of n 2^-53 t^2 -- 1e-8 of reg_covar -- and a relative tolerance of 1e-8 has no meaning for it.  It is held to that absolute
bound instead, and to every equality.  The same kinds of column are held to the restatement at RTOL where their arithmetic is exact
(`raw`: small whole numbers without log_norm)."""
import numpy as np
import pytest

from tests import gmm_ref as G

pytestmark = pytest.mark.gpu

MEASURED_RTOL = 7.2e-10   # score_samples of n4099; the variances reach 4.6e-10 (a component of n1000 that sits on one value: var = reg_covar)
RTOL = min(100 * MEASURED_RTOL, 1e-8)


@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.engine as E
  return E


_DEV = {}


def _device(api, name):
  """the device's fit of a data set: made once"""
  if name not in _DEV:
    X, seeds, kw = G.dataset(name)
    _DEV[name] = api.k_gmm1d_fit(X, seeds, remove_zeros=kw["remove_zeros"], log_norm=kw["log_norm"], all_params=True)
  return _DEV[name]


def _rel(got, want):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape
  assert np.all(got[want == 0] == 0)
  return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0, where=want != 0))


def _close(got, want, what):
  err = _rel(got, want)
  print(f"{what}: max relative error {err:.3e}")
  assert err <= RTOL, (what, err)


def _bits(a):
  return np.ascontiguousarray(a).tobytes()


def _same_bits(a, b, keys=("lower_bound", "n_iter", "converged", "best", "weights", "means", "variances", "n_train", "col_sum", "params_all")):
  return all(_bits(a[k]) == _bits(b[k]) for k in keys)


def _predict_both(api, name, fit_dev, fit_ref):
  X, _, kw = G.dataset(name)
  order = np.argsort(fit_dev["means"], axis=1, kind="stable").astype(np.int32)
  assert np.array_equal(order, np.argsort(fit_ref["means"], axis=1, kind="stable"))
  thr = G.thresholds(fit_dev["means"], fit_dev["variances"], order)
  dev = api.k_gmm1d_predict(X, fit_dev["weights"], fit_dev["means"], fit_dev["variances"], order, 1, thr, log_norm=kw["log_norm"], score=True)
  ref = G.predict(X, fit_ref["weights"], fit_ref["means"], fit_ref["variances"], log_norm=kw["log_norm"])
  return dev, ref


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.MAIN)
def test_fit_is_the_restatement(api, name):
  dev, ref = _device(api, name), G.fitted(name)
  for k in ("n_iter", "converged", "best", "n_train"):
    assert np.array_equal(dev[k], ref[k]), (k, dev[k], ref[k])
  assert dev["lower_bound"].dtype == np.float64 and dev["n_iter"].dtype == np.int32 and dev["n_train"].dtype == np.int64
  assert np.array_equal(dev["col_sum"], ref["col_sum"])   # (the same sum in the same order)
  for k in ("lower_bound", "weights", "means", "variances", "params_all"):
    _close(dev[k], ref[k], f"{name} {k}")


@pytest.mark.parametrize("name", G.MAIN)
def test_predict_is_the_restatement(api, name):
  (prob, bins, score), (rprob, rbins, rscore, _, _) = _predict_both(api, name, _device(api, name), G.fitted(name))
  assert prob.dtype == np.float64 and bins.dtype == np.float32 and score.dtype == np.float64
  assert np.array_equal(bins, rbins)   # every cell
  assert set(np.unique(bins)) <= {0.0, 1.0}
  # y_prob against 1: a responsibility that is 1e-30 of another is not a number either side resolves
  floor = rprob >= 1e-12
  _close(np.where(floor, prob, 0.0), np.where(floor, rprob, 0.0), f"{name} y_prob")
  assert np.max(np.abs(prob - rprob)) <= RTOL
  _close(score, rscore, f"{name} score_samples")


def test_constant_column_under_log_norm(api):
  """see the module docstring: equalities, and the variance to the rounding residue's own size"""
  X, _, _ = G.dataset("const_log")
  dev, ref = _device(api, "const_log"), G.fitted("const_log")
  for k in ("n_iter", "converged", "best", "n_train"):
    assert np.array_equal(dev[k], ref[k])
  t = float(G.normalize(X[:, 0])[0])
  bound = 8 * X.shape[0] * 2.0 ** -53 * t * t
  print(f"const_log: |var - var_ref| = {np.abs(dev['variances'] - ref['variances']).max():.3e}, bound {bound:.3e}")
  assert np.abs(dev["variances"] - ref["variances"]).max() <= bound
  _close(dev["means"], ref["means"], "const_log means")
  _close(dev["weights"], ref["weights"], "const_log weights")


# ---- 2. the same bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n1000", "n4099"])
def test_two_calls_give_the_same_bits(api, name):
  X, seeds, kw = G.dataset(name)
  first = _device(api, name)
  again = api.k_gmm1d_fit(X, seeds, remove_zeros=kw["remove_zeros"], log_norm=kw["log_norm"], all_params=True)
  assert _same_bits(first, again)
  order = np.argsort(first["means"], axis=1, kind="stable").astype(np.int32)
  thr = G.thresholds(first["means"], first["variances"], order)
  a = api.k_gmm1d_predict(X, first["weights"], first["means"], first["variances"], order, 1, thr, score=True)
  b = api.k_gmm1d_predict(X, first["weights"], first["means"], first["variances"], order, 1, thr, score=True)
  assert all(_bits(p) == _bits(q) for p, q in zip(a, b))


def test_a_job_alone_is_the_job_in_the_batch(api):
  X, seeds, kw = G.dataset("n4099")   # 13 columns, 8 restarts
  batch = _device(api, "n4099")
  for c, r in ((0, 0), (5, 3), (12, 7)):
    one = api.k_gmm1d_fit(X[:, c:c + 1], seeds[c:c + 1, r:r + 1], all_params=True)
    assert one["n_iter"][0, 0] == batch["n_iter"][c, r] and one["converged"][0, 0] == batch["converged"][c, r]
    assert _bits(one["lower_bound"][0, 0]) == _bits(batch["lower_bound"][c, r])
    assert _bits(one["params_all"][0, 0]) == _bits(batch["params_all"][c, r])
  for c in (0, 6, 12):   # a column alone, every restart
    col = api.k_gmm1d_fit(X[:, c:c + 1], seeds[c:c + 1], all_params=True)
    assert _same_bits(col, {k: v[c:c + 1] for k, v in batch.items() if k != "stats"})
  # and the embeddings of a column alone
  order = np.argsort(batch["means"], axis=1, kind="stable").astype(np.int32)
  thr = G.thresholds(batch["means"], batch["variances"], order)
  every = api.k_gmm1d_predict(X, batch["weights"], batch["means"], batch["variances"], order, 1, thr, score=True)
  alone = api.k_gmm1d_predict(X[:, 4:5], batch["weights"][4:5], batch["means"][4:5], batch["variances"][4:5], order[4:5], 1, thr[4:5], score=True)
  assert all(_bits(p[:, 4:5]) == _bits(q) for p, q in zip(every, alone))


# ---- 3. max_iter ---------------------------------------------------------------------------------------------------------------------
def test_max_iter_one_and_max_iter_n_iter(api):
  X, seeds, kw = G.dataset("n1000")
  ref1 = G.fit(X, seeds, max_iter=1)
  dev1 = api.k_gmm1d_fit(X, seeds, max_iter=1, all_params=True)
  assert np.all(dev1["n_iter"] == 1) and np.all(dev1["converged"] == 0) and np.array_equal(dev1["best"], ref1["best"])
  for k in ("lower_bound", "params_all"):
    _close(dev1[k], ref1[k], f"max_iter = 1 {k}")
  full = _device(api, "n1000")
  c, r = 1, int(np.argmax(G.fitted("n1000")["n_iter"][1]))
  n = int(G.fitted("n1000")["n_iter"][c, r])
  assert n > 2
  cut = api.k_gmm1d_fit(X[:, c:c + 1], seeds[c:c + 1, r:r + 1], max_iter=n, all_params=True)
  assert cut["n_iter"][0, 0] == n and cut["converged"][0, 0] == 1
  assert _bits(cut["params_all"][0, 0]) == _bits(full["params_all"][c, r]) and _bits(cut["lower_bound"][0, 0]) == _bits(full["lower_bound"][c, r])
  short = api.k_gmm1d_fit(X[:, c:c + 1], seeds[c:c + 1, r:r + 1], max_iter=n - 1, all_params=True)
  assert short["n_iter"][0, 0] == n - 1 and short["converged"][0, 0] == 0


# ---- 4. the C entries refuse and recover -----------------------------------------------------------------------------------------------
def test_invalid_arguments_through_the_c_entry(api):
  import ctypes as C
  from sisua_amd import _hip
  lib = _hip.require_gpu()
  X, seeds, kw = G.dataset("n257")
  x, sd = np.ascontiguousarray(X), np.ascontiguousarray(seeds)
  N, Cn = x.shape
  R, K = sd.shape[1:]

  def call(x=x, N=N, Cn=Cn, K=K, sd=sd, R=R, max_iter=120, tol=1e-3, reg=1e-6):
    o = dict(lb=np.empty((Cn, R)), it=np.empty((Cn, R), np.int32), cv=np.empty((Cn, R), np.int32), best=np.empty((Cn,), np.int32),
             w=np.empty((Cn, K)), m=np.empty((Cn, K)), v=np.empty((Cn, K)), nt=np.empty((Cn,), np.int64), cs=np.empty((Cn,)))
    dp, ip = api._dp, api._ip
    return lib.smx_gmm1d_fit(api._fp(x), N, Cn, K, api._fp(sd), R, max_iter, tol, reg, 1, 1, dp(o["lb"]), ip(o["it"]), ip(o["cv"]), ip(o["best"]),
                             dp(o["w"]), dp(o["m"]), dp(o["v"]), o["nt"].ctypes.data_as(C.POINTER(C.c_int64)), dp(o["cs"]), None, None), o

  neg, zero = x.copy(), np.zeros_like(x)
  neg[3, 0] = -1.0
  big = np.ones((N, Cn, 9), np.float32)
  for kw in (dict(Cn=0), dict(Cn=4097), dict(K=1), dict(K=9, sd=big), dict(R=0), dict(R=65), dict(N=0), dict(N=2 ** 31), dict(max_iter=0),
             dict(tol=0.0), dict(reg=-1.0), dict(x=neg), dict(x=zero), dict(sd=-sd)):
    rc, _ = call(**kw)
    assert rc == -1, kw   # SMX_ERR_INVALID
  rc, _ = call(x=zero)
  assert rc == -1 and b"column 0 has 1 training" in lib.smx_last_error()
  rc, o = call()
  assert rc == 0
  ref = G.fitted("n257")
  assert np.array_equal(o["it"], ref["n_iter"])
  _close(o["m"], ref["means"], "after the refusals: means")
  with pytest.raises(_hip.SmxError) as e:   # the same through check()
    _hip.check(call(K=1)[0])
  assert e.value.code == -1


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
def test_data_layer_is_fit_and_predict_and_trains(api):
  from sisua_amd import ProbabilisticEmbedding
  from sisua_amd.config import RVmeta
  from sisua_amd.data import SingleCellOMIC, synthetic_8kly
  import sisua_amd.models as M
  x, y = synthetic_8kly(n=300, g=64)
  sco = SingleCellOMIC(x).add_omic("proteomic", y)
  pbe, prob, bins = sco.probabilistic_embedding("proteomic")
  own = ProbabilisticEmbedding(random_state=1).fit(y)
  assert np.array_equal(pbe.means, own.means) and np.array_equal(pbe.precisions, own.precisions)
  assert np.array_equal(prob, np.clip(own.predict_proba(y), 1e-8, 1 - 1e-8)) and np.array_equal(bins, own.predict(y))
  assert prob.shape == (300, 12) and prob.min() >= 1e-8 and prob.max() <= 1 - 1e-8 and set(np.unique(bins)) <= {0.0, 1.0}
  assert np.array_equal(own.fit_transform(y), own.predict_proba(y))
  assert np.isfinite(own.score(y)) and own.score_samples(y).shape == (300,)
  # the restatement on the same matrix
  ref = G.fit(y, G.draw_init_raw(y, 2, 8, 1))
  _close(pbe.means, np.sort(ref["means"], axis=1).T, "end to end: means")
  rprob, rbins = G.predict(y, ref["weights"], ref["means"], ref["variances"])[:2]
  assert np.max(np.abs(own.predict_proba(y) - rprob)) <= RTOL
  # the probabilities as Bernoulli labels of SISUA
  sco.add_omic("y_prob", sco.get_x_probs("proteomic"))
  model = M.SISUA(outputs=sco.get_rv("transcriptomic"), labels=[RVmeta(12, "bernoulli", name="y_prob")],
                  latents=RVmeta(8, "diag", True, "Latents"), encoder=M.NetConf([32], batchnorm=True), decoder=M.NetConf([32], batchnorm=True))
  model.fit(sco.create_dataset(["transcriptomic", "y_prob"], labels_percent=1.0, batch_size=64, drop_remainder=True), metadata=sco, epochs=1,
            max_iter=2, verbose=False)
  assert len(model.train_history["loss"]) >= 1 and np.isfinite(model.train_history["loss"]).all()
  assert np.isfinite(model.train_history["nllk_y"]).all()
