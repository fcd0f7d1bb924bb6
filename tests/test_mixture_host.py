"""Host side of the full-covariance Gaussian mixture (sisua_amd/mixture.py, smx_gmm_full.hip) without a GPU: the float64 restatement
(tests/gmm_full_ref.py) against scikit-learn's results (tests/golden/mixture_fixture.npz, made by tests/golden/make_mixture_fixtures.py), the
separations that make EQUAL the right demand of tests/test_gpu_mixture.py, the quality of the optimum a k-means start reaches, and the
argument checks.

Tolerances.  Started from the same first M-step the restatement and scikit-learn run the same loop in float64: measured, n_iter and labels
equal on all eight sets, |lb - lb_sklearn| <= 7.2e-15, means and covariances within 2.7e-15; 1e-12 leaves two decades and more for another
BLAS."""
import os
import re

import numpy as np
import pytest

from tests import clustering_ref as CR
from tests import gmm_full_ref as G

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixture_fixture.npz")
TOL = 1e-3


@pytest.fixture(scope="module")
def fx():
  with np.load(FIXTURE) as f:
    return {k: f[k] for k in f.files}


def _best(name):
  ref = G.fitted(name)
  return ref["runs"][G.starts(name)["best"]]


@pytest.mark.parametrize("name", G.NAMES)
def test_restatement_is_scikit_learn(fx, name):
  run = _best(name)
  assert run["status"] == 0
  assert run["n_iter"] == int(fx[f"{name}_a_n_iter"]) and run["converged"] == int(fx[f"{name}_a_converged"]) == 1
  assert np.array_equal(run["labels"], fx[f"{name}_a_labels"])
  err = dict(lb=abs(run["lower_bound"] - float(fx[f"{name}_a_lower_bound"])), means=np.abs(run["means"] - fx[f"{name}_a_means"]).max(),
             cov=np.abs(run["covariances"] - fx[f"{name}_a_covariances"]).max())
  print(f"{name}: n_iter {run['n_iter']}, restatement - scikit-learn: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
  assert all(v <= 1e-12 for v in err.values()), err
  # chol_inv is the inverse factor of the covariance it is returned with
  for k in range(run["weights"].size):
    L = run["chol_inv"][k]
    assert np.array_equal(L, np.tril(L))
    assert np.abs(L @ run["covariances"][k] @ L.T - np.eye(L.shape[0])).max() <= 1e-9


@pytest.mark.parametrize("name", G.NAMES)
def test_separations_the_device_test_relies_on(name):
  ref = G.fitted(name)
  runs = ref["runs"]
  assert not ref["all_failed"] and all(r["status"] == 0 for r in runs)
  near_tol = min(abs(d - TOL) for r in runs for d in r["lb_steps"])
  gap = min(r["gap"] for r in runs)
  print(f"{name}: iterations {[r['n_iter'] for r in runs]}, closest lower-bound step to tol {near_tol:.2e}, smallest top-two gap {gap:.2e}")
  assert near_tol > 1e-9    # the stop rule has one answer
  assert gap > 1e-6         # ... and so has every label
  for i in range(len(runs)):
    for j in range(i + 1, len(runs)):
      if abs(runs[i]["lower_bound"] - runs[j]["lower_bound"]) <= 1e-9:
        # ... and the best restart, unless two restarts end in the same partition (under other component names: k-means numbers its
        # clusters by its starting cells), where either is as good an answer
        assert CR.adjusted_rand(runs[i]["labels"], runs[j]["labels"]) == 1.0, (i, j)


@pytest.mark.parametrize("name", G.NAMES)
def test_quality_of_the_optimum(fx, name):
  """From the best k-means partition of 8 random-cell starts against scikit-learn's own GaussianMixture(K, random_state=5218) (k-means++
  start).  On m2, m3, m16 and m33 the two routes end in the same partition and our lower bound is not below theirs by more than tol.  On
  the others the figures are printed only: with one start each the routes can end in different optima either way (measured: d32 -43.78
  against scikit-learn's -42.18, m64 -89.42 against -92.37, m2 .. m33, d1 and d5 within 1.9e-4)."""
  run = _best(name)
  theirs = float(fx[f"{name}_b_lower_bound"])
  ari = CR.adjusted_rand(fx[f"{name}_b_labels"], run["labels"])
  print(f"{name}: lower bound {run['lower_bound']!r} against scikit-learn's {theirs!r}; ARI of the two labelings {ari!r}")
  if name in ("m2", "m3", "m16", "m33"):
    assert ari == 1.0 and run["lower_bound"] >= theirs - TOL


def test_failure_is_a_value():
  """two identical cells alone in a component with reg_covar = 0: that restart has status 1 and ranks last"""
  Z, _, K = G.dataset("m3")
  Z = Z.copy()
  Z[5] = Z[9] = 0.0
  good = G.starts("m3")["labels_all"][G.starts("m3")["best"]]
  bad = np.where(good == 2, 0, good)
  bad[5] = bad[9] = 2
  ref = G.fit(Z, np.stack([bad, good]), K, reg_covar=0.0)
  assert ref["runs"][0]["status"] == 1 and np.isnan(ref["runs"][0]["lower_bound"]) and ref["runs"][1]["status"] == 0 and ref["best"] == 1
  assert G.fit(Z, bad[None], K, reg_covar=0.0)["all_failed"]


def test_argument_checks_come_before_the_device(monkeypatch):
  from sisua_amd import GaussianMixture, _hip, clustering, metrics, mixture

  def no_device(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", no_device)
  assert GaussianMixture is mixture.GaussianMixture and metrics.latent_scores is clustering.latent_scores
  Z, y, _ = CR.dataset("d5")
  wide = np.zeros((257, 65), np.float32)
  nan = Z.copy()
  nan[3, 1] = np.nan
  # the class: its settings ...
  for kw in (dict(n_components=1), dict(n_components=257), dict(n_components=3, covariance_type="diag"), dict(n_components=3, covariance_type="tied"),
             dict(n_components=3, max_iter=0), dict(n_components=3, tol=0.0), dict(n_components=3, tol=np.nan), dict(n_components=3, reg_covar=-1e-6),
             dict(n_components=3, n_init=0), dict(n_components=3, n_init=9), dict(n_components=3, kmeans_n_init=0), dict(n_components=3, kmeans_n_init=4097),
             dict(n_components=3, n_init=4, kmeans_n_init=3), dict(n_components=3, means_init=np.zeros((3, 5))),
             dict(n_components=3, weights_init=np.ones(3) / 3), dict(n_components=3, precisions_init=np.zeros((3, 5, 5))),
             dict(n_components=3, warm_start=True), dict(n_components=3, init_params="random")):
    with pytest.raises(ValueError):
      mixture.GaussianMixture(**kw)
  with pytest.raises(ValueError, match="full"):
    mixture.GaussianMixture(3, covariance_type="spherical")
  with pytest.raises(TypeError):
    mixture.GaussianMixture(3, colour="red")
  # ... and its data
  gm = mixture.GaussianMixture(3)
  for X in (wide, Z[:, 0], Z[:2], nan, np.zeros((257, 0), np.float32)):
    with pytest.raises(ValueError):
      gm.fit(X)
    with pytest.raises(ValueError):
      gm.fit_predict(X)
  with pytest.raises(RuntimeError):
    gm.predict(Z)
  # mixture_labels
  for kw in (dict(latent=wide, n_labels=3), dict(latent=Z[:, 0], n_labels=3), dict(latent=Z, n_labels=1), dict(latent=Z, n_labels=257),
             dict(latent=Z[:2], n_labels=3), dict(latent=nan, n_labels=3), dict(latent=Z, n_labels=3, n_init=0),
             dict(latent=Z, n_labels=3, n_init=4097), dict(latent=Z, n_labels=3, max_iter=0)):
    with pytest.raises(ValueError):
      clustering.mixture_labels(**kw)
  # latent_scores: what clustering_scores refuses, and the width and the non-finite entries the mixture refuses
  bad = [dict(latent=Z[:, 0], labels=y, n_labels=3), dict(latent=wide, labels=y, n_labels=3), dict(latent=Z, labels=y[:-1], n_labels=3),
         dict(latent=Z, labels=y, n_labels=1), dict(latent=Z, labels=y, n_labels=257), dict(latent=Z, labels=y, n_labels=2),
         dict(latent=Z, labels=y - 1, n_labels=3), dict(latent=Z, labels=np.zeros(257, int), n_labels=3),
         dict(latent=Z[:2], labels=y[:2], n_labels=3), dict(latent=Z, labels=y, n_labels=3, n_init=0),
         dict(latent=Z, labels=y, n_labels=3, n_init=4097), dict(latent=Z, labels=y, n_labels=3, max_iter=0),
         dict(latent=nan, labels=y, n_labels=3)]
  for alg in ("gmm", "both"):
    for kw in bad:
      with pytest.raises(ValueError):
        metrics.latent_scores(prediction_algorithm=alg, **kw)
  with pytest.raises(ValueError):
    metrics.latent_scores(np.zeros((257, 65), np.float32), y, 3)   # the default is 'both'
  with pytest.raises(ValueError, match="spectral"):
    metrics.latent_scores(Z, y, 3, prediction_algorithm="spectral")
  with pytest.raises(ValueError):
    metrics.ClusteringScores(np.zeros((5, 3), np.float32), np.zeros((4, 3)), prediction_algorithm="both")


def test_knn_routes_to_clustering_scores(monkeypatch):
  from sisua_amd import clustering
  seen = []

  def fake(latent, labels, n_labels, prediction_algorithm="knn", **kw):
    seen.append((prediction_algorithm, kw))
    return dict(ASW=0.25, ARI=0.5, NMI=0.75, UCA=1.0)
  monkeypatch.setattr(clustering, "clustering_scores", fake)
  Z, y, _ = CR.dataset("d5")
  got = clustering.latent_scores(Z, y, 3, prediction_algorithm="knn", n_init=7, seed=1, max_iter=9)
  assert got == dict(ASW=0.25, ARI=0.5, NMI=0.75, UCA=1.0) and seen == [("knn", dict(n_init=7, seed=1, max_iter=9))]


def test_starts_are_the_lowest_inertias_in_order():
  from sisua_amd.mixture import starts_from_kmeans
  lab = np.arange(5 * 4).reshape(5, 4)
  km = dict(inertia=np.array([3.0, 1.0, np.nan, 1.0, 2.0]), labels_all=lab)
  got = starts_from_kmeans(km, 4)
  assert got.dtype == np.int32 and np.array_equal(got, lab[[1, 3, 4, 0]])   # ties to the lower index, NaN last


def test_precisions_cholesky_layout_and_information_criteria(monkeypatch):
  """a fitted instance from the restatement's parameters: scikit-learn's upper-triangular layout, and aic / bic from score"""
  from sisua_amd import mixture
  run = _best("d5")
  Z, _, K = G.dataset("d5")
  gm = mixture.GaussianMixture(K)
  gm.weights_, gm.means_, gm.covariances_ = run["weights"], run["means"], run["covariances"]
  gm.precisions_cholesky_ = np.ascontiguousarray(np.swapaxes(run["chol_inv"], 1, 2))
  gm.n_features_in_ = 5
  P = gm.precisions_cholesky_
  assert np.array_equal(P[0], np.triu(P[0])) and np.abs(P[0] @ P[0].T - np.linalg.inv(run["covariances"][0])).max() <= 1e-9
  monkeypatch.setattr(gm, "score_samples", lambda X: run["lse"])
  n, p = 257, K * 15 + K * 5 + K - 1
  assert gm._n_parameters() == p
  assert gm.aic(Z) == -2.0 * float(np.mean(run["lse"])) * n + 2.0 * p
  assert gm.bic(Z) == -2.0 * float(np.mean(run["lse"])) * n + p * np.log(n)


def test_abi_and_sources():
  from sisua_amd import _hip, build
  assert _hip.SMX_ABI_VERSION >= 10 and "smx_gmm_full.hip" in build.SOURCES
  assert {"smx_gmm_full_fit", "smx_gmm_full_predict"} <= set(_hip.SIGNATURES)
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sisua_hip.h")).read()
  assert "int smx_gmm_full_fit(" in header and "int smx_gmm_full_predict(" in header
  assert int(re.search(r"#define SMX_ABI_VERSION (\d+)", header).group(1)) == _hip.SMX_ABI_VERSION
