"""Makes tests/golden/mixture_fixture.npz: scikit-learn's own GaussianMixture on the sets of tests.gmm_full_ref (scikit-learn 1.7.2 when
this file was last run).  The fixture holds recorded results only, so that no test needs scikit-learn at run time.  Per set `s`:
  (a) scikit-learn STARTED FROM THE RESTATEMENT'S OWN FIRST M-STEP -- GaussianMixture(K, weights_init=w0, means_init=mu0,
      precisions_init=inv(S0)), w0, mu0, S0 the first M-step of the best k-means start (tests.gmm_full_ref.starts): this pins the
      restatement to scikit-learn's loop
        {s}_a_lower_bound, {s}_a_n_iter, {s}_a_converged, {s}_a_labels [N], {s}_a_means [K, D], {s}_a_covariances [K, D, D]
  (b) scikit-learn's own GaussianMixture(K, random_state=5218) (its k-means++ start): for the test of the optimum's quality
        {s}_b_lower_bound, {s}_b_labels [N]
Run from the repository root:  python -m tests.golden.make_mixture_fixtures"""
import os
import warnings

import numpy as np


def main():
  import sklearn
  from sklearn.mixture import GaussianMixture
  from tests import gmm_full_ref as G
  out = {"sklearn_version": np.array(sklearn.__version__)}
  for s in G.NAMES:
    Z, _, K = G.dataset(s)
    st = G.starts(s)
    z = Z.astype(np.float64)
    mine = G.fit_one(Z, st["labels_all"][st["best"]], K)
    w0, mu0, S0 = mine["first"]
    with warnings.catch_warnings():
      warnings.simplefilter("error")   # (a run that does not converge is not a fixture)
      a = GaussianMixture(K, weights_init=w0, means_init=mu0, precisions_init=np.linalg.inv(S0)).fit(z)
      b = GaussianMixture(K, random_state=5218).fit(z)
    out[f"{s}_a_lower_bound"], out[f"{s}_a_n_iter"], out[f"{s}_a_converged"] = np.float64(a.lower_bound_), np.int32(a.n_iter_), np.int32(a.converged_)
    out[f"{s}_a_labels"], out[f"{s}_a_means"], out[f"{s}_a_covariances"] = a.predict(z).astype(np.int32), a.means_, a.covariances_
    out[f"{s}_b_lower_bound"], out[f"{s}_b_labels"] = np.float64(b.lower_bound_), b.predict(z).astype(np.int32)
    print(f"{s}: (a) n_iter {a.n_iter_} / restatement {mine['n_iter']}, lb {a.lower_bound_!r} / {mine['lower_bound']!r}, labels equal "
          f"{np.array_equal(out[f'{s}_a_labels'], mine['labels'])}, |means| {np.abs(a.means_ - mine['means']).max():.2e}, |cov| "
          f"{np.abs(a.covariances_ - mine['covariances']).max():.2e}; (b) lb {b.lower_bound_!r}; steps vs tol "
          f"{min(abs(d - 1e-3) for d in mine['lb_steps']):.2e}, gap {mine['gap']:.2e}")
  np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mixture_fixture.npz"), **out)


if __name__ == "__main__":
  main()
