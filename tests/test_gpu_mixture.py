"""The full-covariance Gaussian mixture on the device (smx_gmm_full.hip) against the float64 restatement tests/gmm_full_ref.py: parity from
the best k-means start on eight sets, determinism and independence of the batch, replay at the iteration limit, predict, a failing
restart as a value, the refused arguments, and the route to the reference's default clustering scores.

Equalities.  n_iter, converged, best, status and labels are EQUAL: tests/test_mixture_host.py asserts on the restatement that no
lower-bound step lies within 1e-9 of tol and that every cell's best l_nk leads the second-best by more than 1e-6, five decades and more
above the deviations below.

Tolerances.  The device sums in another order than NumPy (slices of cells in index order, one chain per triangle entry), over a few
thousand terms, with covariance condition numbers up to 1.7e3 and at most 22 iterations.  The rule: per quantity 100 x the largest
deviation measured on an MI355X against the restatement, capped at 1e-8.  Covariances and chol_inv are taken relative to the largest entry
of the matrix, the others absolute.  Measured -- the largest over the eight sets, from the best k-means start, from each of the 8 starts
(lower bound, weights, means, covariances) and after one iteration on m3 -- and asserted:
  lower_bound  7.1e-15 from the best start and after one iteration (m33, d32)                           7.1e-13
  lower_bound  6.3e-12 over each of the 8 starts (d32, one start: 83 cells per component at D = 32;
               2.8e-14 on the other sets), asserted in the 8-start test alone                          6.3e-10
  weights      6.2e-16                                                                                 6.2e-14
  means        2.8e-14 (m16)                                                                           2.8e-12
  covariances  3.1e-14 (m16)                                                                           3.1e-12
  chol_inv     4.2e-14 (m16; m3 2.0e-14)                                                               4.2e-12
  score        3.0e-13 (m16: the per-cell log-likelihood of predict against the restatement's)         3.0e-11
"""
import warnings

import numpy as np
import pytest

from tests import clustering_ref as CR
from tests import gmm_full_ref as G
from tests.util import synth_counts, synth_labels

pytestmark = pytest.mark.gpu

# quantity: (largest deviation measured on an MI355X, asserted = min(100 x measured, 1e-8))
MEASURED = dict(lower_bound=7.105e-15, lower_bound_8_starts=6.274e-12, weights=6.176e-16, means=2.798e-14, covariances=3.119e-14, chol_inv=4.182e-14, score=2.984e-13)
TOL = {k: min(100.0 * v, 1e-8) for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def eng():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd import engine
  return engine


def _bits(a):
  return np.ascontiguousarray(a).tobytes()


def _best_start(name):
  st = G.starts(name)
  return st["labels_all"][st["best"]], G.fitted(name)["runs"][st["best"]]


def _dev(got, want, relative_to_matrix=False):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  d = np.abs(got - want)
  if relative_to_matrix:
    d = d / np.abs(want).max(axis=(-2, -1), keepdims=True)
  return float(d.max())


_FIT = {}


def _fit(eng, name):
  """the device's fit of a set from its best k-means start with the default settings: made once"""
  if name not in _FIT:
    Z, _, K = G.dataset(name)
    _FIT[name] = eng.k_gmm_full_fit(Z, _best_start(name)[0], n_components=K)
  return _FIT[name]


FIELDS = ("lower_bound", "n_iter", "converged", "status", "weights", "means", "covariances", "chol_inv", "labels")


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.NAMES)
def test_fit_is_the_restatement(eng, name):
  got, ref = _fit(eng, name), _best_start(name)[1]
  dev = dict(lower_bound=_dev(got["lower_bound"][0], ref["lower_bound"]), weights=_dev(got["weights"], ref["weights"]),
             means=_dev(got["means"], ref["means"]), covariances=_dev(got["covariances"], ref["covariances"], True),
             chol_inv=_dev(got["chol_inv"], ref["chol_inv"], True))
  print(f"{name}: n_iter {int(got['n_iter'][0])} (restatement {ref['n_iter']}); deviations " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
  assert got["n_iter"][0] == ref["n_iter"] and got["converged"][0] == ref["converged"] == 1 and got["best"] == 0 and got["status"][0] == 0
  assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], ref["labels"])
  for k, v in dev.items():
    assert v <= TOL[k], (name, k, v)
  for k in range(got["weights"].size):   # zeros above the diagonal, exactly
    assert np.array_equal(got["chol_inv"][k], np.tril(got["chol_inv"][k])) and np.array_equal(got["covariances"][k], got["covariances"][k].T)


# ---- 2. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.NAMES)
def test_two_calls_and_a_restart_alone_give_the_same_bits(eng, name):
  Z, _, K = G.dataset(name)
  starts = G.starts(name)["labels_all"]
  batch = eng.k_gmm_full_fit(Z, starts, n_components=K, all_params=True)
  again = eng.k_gmm_full_fit(Z, starts, n_components=K, all_params=True)
  keys = FIELDS + ("weights_all", "means_all", "covariances_all")
  assert all(_bits(batch[k]) == _bits(again[k]) for k in keys) and batch["best"] == again["best"]
  # the best restart is the highest lower bound, ties to the lowest index, and the single-restart outputs are its
  b = batch["best"]
  assert (batch["status"] == 0).all() and b == int(np.argmax(batch["lower_bound"]))
  assert _bits(batch["weights"]) == _bits(batch["weights_all"][b]) and _bits(batch["means"]) == _bits(batch["means_all"][b])
  assert _bits(batch["covariances"]) == _bits(batch["covariances_all"][b])
  ref = G.fitted(name)["runs"]
  assert np.array_equal(batch["n_iter"], [r["n_iter"] for r in ref]) and np.array_equal(batch["converged"], [r["converged"] for r in ref])
  dev = dict(lower_bound_8_starts=_dev(batch["lower_bound"], [r["lower_bound"] for r in ref]), weights=_dev(batch["weights_all"], [r["weights"] for r in ref]),
             means=_dev(batch["means_all"], [r["means"] for r in ref]),
             covariances=_dev(batch["covariances_all"], [r["covariances"] for r in ref], True))
  print(f"{name}: all 8 starts, deviations " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
  for k, v in dev.items():
    assert v <= TOL[k], (name, k, v)
  for r in range(len(starts)):   # every restart, those that leave the list of running restarts in mid-call included
    alone = eng.k_gmm_full_fit(Z, starts[r], n_components=K, all_params=True)
    assert alone["best"] == 0
    for k in ("lower_bound", "n_iter", "converged", "status"):
      assert _bits(alone[k][0]) == _bits(batch[k][r]), (r, k)
    for k in ("weights", "means", "covariances"):
      assert _bits(alone[k]) == _bits(batch[k + "_all"][r]), (r, k)
    if r == b:
      assert _bits(alone["labels"]) == _bits(batch["labels"]) and _bits(alone["chol_inv"]) == _bits(batch["chol_inv"])
  if name == "d5":   # the fit of the parity test is the single-restart call of the best k-means start
    r = G.starts(name)["best"]
    assert _bits(_fit(eng, name)["means"]) == _bits(batch["means_all"][r])


# ---- 3. replay ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m2", "m3", "m33", "d1"])
def test_iteration_limit_at_n_iter_reproduces_the_run(eng, name):
  Z, _, K = G.dataset(name)
  full = _fit(eng, name)
  exact = eng.k_gmm_full_fit(Z, _best_start(name)[0], n_components=K, max_iter=int(full["n_iter"][0]))
  assert all(_bits(exact[k]) == _bits(full[k]) for k in FIELDS)


def test_one_iteration_returns_the_first_m_step_of_the_loop(eng):
  Z, _, K = G.dataset("m3")
  start = _best_start("m3")[0]
  got = eng.k_gmm_full_fit(Z, start, n_components=K, max_iter=1)
  ref = G.fit_one(Z, start, K, max_iter=1)
  assert got["converged"][0] == 0 == ref["converged"] and got["n_iter"][0] == 1 and got["status"][0] == 0
  assert np.array_equal(got["labels"], ref["labels"])
  dev = dict(lower_bound=_dev(got["lower_bound"][0], ref["lower_bound"]), weights=_dev(got["weights"], ref["weights"]),
             means=_dev(got["means"], ref["means"]), covariances=_dev(got["covariances"], ref["covariances"], True),
             chol_inv=_dev(got["chol_inv"], ref["chol_inv"], True))
  print("m3 after one iteration: deviations " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
  for k, v in dev.items():
    assert v <= TOL[k], (k, v)
  # and they are not the parameters of the start
  assert _dev(got["means"], ref["first"][1]) > 1e-6


# ---- 4. predict --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.NAMES)
def test_predict_from_the_fitted_parameters(eng, name):
  Z, _, K = G.dataset(name)
  fit, ref = _fit(eng, name), _best_start(name)[1]
  got = eng.k_gmm_full_predict(Z, fit["weights"], fit["means"], fit["chol_inv"], resp=True, score=True)
  assert np.array_equal(got["labels"], fit["labels"])
  assert got["resp"].shape == (Z.shape[0], K) and np.abs(got["resp"].sum(axis=1) - 1.0).max() <= 1e-14
  assert np.array_equal(got["resp"].argmax(axis=1), fit["labels"])
  dev = _dev(got["score"], ref["lse"])
  print(f"{name}: score against the restatement's lse {dev:.3e}")
  assert dev <= TOL["score"]
  plain = eng.k_gmm_full_predict(Z, fit["weights"], fit["means"], fit["chol_inv"])
  assert set(plain) == {"labels"} and np.array_equal(plain["labels"], fit["labels"])


def test_the_class_is_the_kernels(eng):
  from sisua_amd import GaussianMixture
  from sisua_amd.clustering import draw_init_idx
  from sisua_amd.mixture import ConvergenceWarning, starts_from_kmeans
  Z, _, K = G.dataset("d5")
  gm = GaussianMixture(K, kmeans_n_init=8)
  labels = gm.fit_predict(Z)
  km = eng.k_cluster_kmeans(Z, draw_init_idx(Z.shape[0], K, 8), all_labels=True)
  want = eng.k_gmm_full_fit(Z, starts_from_kmeans(km, 1), n_components=K)
  assert labels.dtype == np.int64 and np.array_equal(labels, want["labels"]) and np.array_equal(gm.predict(Z), labels)
  assert _bits(gm.means_) == _bits(want["means"]) and _bits(gm.covariances_) == _bits(want["covariances"]) and _bits(gm.weights_) == _bits(want["weights"])
  assert np.array_equal(gm.precisions_cholesky_, np.swapaxes(want["chol_inv"], 1, 2))
  assert gm.lower_bound_ == want["lower_bound"][0] and gm.n_iter_ == want["n_iter"][0] and gm.converged_ is True
  assert all(isinstance(v, (np.ndarray, int, float, bool, str)) for v in vars(gm).values())
  # draw_init_idx(.., 8) is what tests.gmm_full_ref.starts draws: the restatement's fit is this one
  assert np.array_equal(labels, _best_start("d5")[1]["labels"])
  lse = gm.score_samples(Z)
  assert gm.score(Z) == float(np.mean(lse)) and gm.score(Z) >= gm.lower_bound_ - 1e-9   # (one M-step later: EM does not go down)
  n, p = Z.shape[0], gm._n_parameters()
  assert gm.aic(Z) == -2.0 * gm.score(Z) * n + 2.0 * p and gm.bic(Z) == -2.0 * gm.score(Z) * n + p * np.log(n)
  assert np.abs(gm.predict_proba(Z).sum(axis=1) - 1.0).max() <= 1e-14
  # n_init restarts: the best of them is not worse
  gm3 = GaussianMixture(K, n_init=3, kmeans_n_init=8).fit(Z)
  assert gm3.lower_bound_ >= gm.lower_bound_
  with pytest.warns(ConvergenceWarning):
    GaussianMixture(K, max_iter=1, kmeans_n_init=8).fit(Z)


# ---- 5. failure is a value ---------------------------------------------------------------------------------------------------------
def test_a_restart_with_an_ill_defined_covariance(eng):
  """m3 with two cells moved to the origin and a start that gives component 2 those two alone, reg_covar = 0.  (At the origin because nk =
  2 + 10 eps: the mean of two identical cells elsewhere differs from them by rounding, and the sign of the pivots that follow is noise.
  Here the mean, the differences and the covariance are exactly zero, and the first pivot is 0.)"""
  from sisua_amd import GaussianMixture
  Z, _, K = G.dataset("m3")
  Z = Z.copy()
  Z[5] = Z[9] = 0.0
  good = _best_start("m3")[0]
  bad = np.where(good == 2, 0, good).astype(np.int32)
  bad[5] = bad[9] = 2
  got = eng.k_gmm_full_fit(Z, np.stack([bad, good]), n_components=K, reg_covar=0.0)
  assert got["status"].tolist() == [1, 0] and np.isnan(got["lower_bound"][0]) and got["converged"][0] == 0 and got["n_iter"][0] == 0
  assert got["best"] == 1 and np.isfinite(got["lower_bound"][1]) and got["converged"][1] == 1
  alone = eng.k_gmm_full_fit(Z, good, n_components=K, reg_covar=0.0)
  assert all(_bits(alone[k]) == _bits(got[k]) for k in ("weights", "means", "covariances", "chol_inv", "labels"))
  with pytest.raises(ValueError, match="ill-defined empirical covariance"):
    eng.k_gmm_full_fit(Z, bad, n_components=K, reg_covar=0.0)
  gm = GaussianMixture(K, reg_covar=0.0)
  with pytest.raises(ValueError, match="increase reg_covar"):
    gm._fit_from_labels(Z, bad[None])
  # the library stays usable
  after = eng.k_gmm_full_fit(G.dataset("m3")[0], good, n_components=K)
  assert all(_bits(after[k]) == _bits(_fit(eng, "m3")[k]) for k in FIELDS)


# ---- 6. limits ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(eng):
  from sisua_amd import _hip
  Z, _, K = G.dataset("d5")
  good = _best_start("d5")[0]
  N = Z.shape[0]
  fit = _fit(eng, "d5")
  nan = Z.copy()
  nan[7, 2] = np.nan
  inf = Z.copy()
  inf[0, 0] = np.inf
  high, low = good.copy(), good.copy()
  high[11], low[11] = K, -1
  w, m, li = fit["weights"], fit["means"], fit["chol_inv"]
  neg_diag, nan_li, zero_w, inf_m = li.copy(), li.copy(), w.copy(), m.copy()
  neg_diag[1, 2, 2], nan_li[0, 3, 1], zero_w[0], inf_m[2, 4] = -1.0, np.nan, 0.0, np.inf
  calls = [lambda: eng.k_gmm_full_fit(np.zeros((N, 65), np.float32), good, n_components=K),
           lambda: eng.k_gmm_full_fit(np.zeros((N, 0), np.float32), good, n_components=K),
           lambda: eng.k_gmm_full_fit(Z, np.zeros(N, np.int32), n_components=1),
           lambda: eng.k_gmm_full_fit(Z, np.zeros(N, np.int32), n_components=257),
           lambda: eng.k_gmm_full_fit(Z[:2], good[:2] % 2, n_components=K),
           lambda: eng.k_gmm_full_fit(Z, np.zeros((0, N), np.int32), n_components=K),
           lambda: eng.k_gmm_full_fit(Z, np.tile(good, (9, 1)), n_components=K),
           lambda: eng.k_gmm_full_fit(Z, high, n_components=K), lambda: eng.k_gmm_full_fit(Z, low, n_components=K),
           lambda: eng.k_gmm_full_fit(nan, good, n_components=K), lambda: eng.k_gmm_full_fit(inf, good, n_components=K),
           lambda: eng.k_gmm_full_fit(Z, good, n_components=K, max_iter=0), lambda: eng.k_gmm_full_fit(Z, good, n_components=K, tol=0.0),
           lambda: eng.k_gmm_full_fit(Z, good, n_components=K, reg_covar=-1.0),
           lambda: eng.k_gmm_full_predict(nan, w, m, li), lambda: eng.k_gmm_full_predict(Z[:2], w, m, li),
           lambda: eng.k_gmm_full_predict(Z, zero_w, m, li), lambda: eng.k_gmm_full_predict(Z, w, inf_m, li),
           lambda: eng.k_gmm_full_predict(Z, w, m, neg_diag), lambda: eng.k_gmm_full_predict(Z, w, m, nan_li)]
  for i, call in enumerate(calls):
    with pytest.raises(_hip.SmxError) as err:
      call()
    assert err.value.code == -1, i   # SMX_ERR_INVALID


# ---- 7. the scores -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5", "d32"])
def test_latent_scores(eng, name):
  from sisua_amd import clustering as C
  from sisua_amd import metrics
  Z, y, _ = CR.dataset(name)
  K = CR.DATASETS[name][2]
  kw = dict(n_init=8, max_iter=300)   # the 8 starts of tests.gmm_full_ref.starts
  knn = metrics.clustering_scores(Z, y, K, **kw)
  ref_labels = _best_start(name)[1]["labels"]
  gmm = metrics.latent_scores(Z, y, K, prediction_algorithm="gmm", **kw)
  want = dict(ASW=knn["ASW"], ARI=C.adjusted_rand(y, ref_labels), NMI=C.normalized_mutual_info(y, ref_labels),
              UCA=C.unsupervised_clustering_accuracy(y, ref_labels))
  assert gmm == want
  both = metrics.latent_scores(Z, y, K, **kw)   # the reference's default
  assert both == {k: (knn[k] + gmm[k]) / 2 for k in knn}
  again = metrics.latent_scores(Z, y, K, prediction_algorithm="knn", **kw)
  assert {k: _bits(np.float64(v)) for k, v in again.items()} == {k: _bits(np.float64(v)) for k, v in knn.items()}
  ml = C.mixture_labels(Z, K, **kw)
  assert np.array_equal(ml["labels"], ref_labels) and np.array_equal(ml["kmeans_labels"], G.starts(name)["labels_all"][G.starts(name)["best"]])
  assert ml["mixture"].converged_ and np.array_equal(ml["mixture"].predict(Z), ml["labels"])


def test_model_method_and_metric_class(eng):
  import sisua_amd.models as M
  from sisua_amd import metrics
  from sisua_amd.data import SingleCellOMIC
  n, g = 257, 60
  x = synth_counts(n, g, sparsity=0.8, seed=3)
  extras = synth_labels(n, ((5, "nb"),))[0].astype(np.float64)
  m = M.VAE(outputs=M.RVmeta(g, "zinb", True, "transcriptomic"), latents=M.RVmeta(6, "diag", True, "Latents"),
            encoder=M.NetConf([32], batchnorm=True, dropout=0.1), decoder=M.NetConf([32], batchnorm=True, dropout=0.1))
  m.fit(SingleCellOMIC(x, name="toy"), epochs=2, batch_size=64)
  kw = dict(n_init=10, max_iter=100)
  z = m._latent_means(x, None, 64)[0]
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")   # (a latent space after two epochs may need more than 100 EM iterations)
    both = metrics.latent_scores(z, extras, 5, "both", **kw)
    assert m.clustering_scores(x, extras, batch_size=64, prediction_algorithm="both", **kw) == both
    assert set(both) == {"ASW", "ARI", "NMI", "UCA"} and all(np.isfinite(v) for v in both.values())
    gmm = metrics.latent_scores(z, np.argmax(extras, 1), 5, "gmm", **kw)
    got = metrics.ClusteringScores(x, extras, batch_size=64, prediction_algorithm="gmm", **kw)(m)
  assert set(got) == {"ASW", "ARI", "NMI", "UCA", "ASW_0", "ARI_0", "NMI_0", "UCA_0"}
  for k, v in gmm.items():
    assert got[k] == got[k + "_0"] == -v, k
  # the default is still k-means, bit for bit
  assert m.clustering_scores(x, extras, batch_size=64, **kw) == metrics.clustering_scores(z, extras, 5, **kw)
  knn = metrics.clustering_scores(z, np.argmax(extras, 1), 5, **kw)
  default = metrics.ClusteringScores(x, extras, batch_size=64, **kw)(m)
  assert all(default[k + "_0"] == -v for k, v in knn.items())
