"""Makes tests/golden/clustering_fixture.npz: scikit-learn's results on the four data sets of tests/clustering_ref.py, called the way the
reference calls it (sisua/analysis/latent_benchmarks.py:69-117) -- silhouette_score(Z, y), KMeans(K, n_init=200, random_state=5218) and
adjusted_rand_score / normalized_mutual_info_score of its labels -- so that no test needs scikit-learn at run time.  Per data set `name`:
  {name}_asw, {name}_ari, {name}_nmi   scikit-learn's scores (float64)
  {name}_uca                           the reference's UCA formula on scikit-learn's labels, solved with scipy.optimize.linear_sum_assignment
  {name}_km_labels                     KMeans.labels_ (int32)
  {name}_km_inertia                    KMeans.inertia_ as scikit-learn reports it (it works in the float32 of Z)
  {name}_km_inertia64                  the inertia of those labels in float64: squared distances to the float64 means of its clusters
  {name}_s{seed}_km_inertia(64)        the same two for the data seed of tests.clustering_ref.QUALITY_SEEDS where that is not 3
Run from the repository root with scikit-learn 1.7 installed:  python -m tests.golden.make_clustering_fixtures"""
import os

import numpy as np


def main():
  import sklearn
  from scipy.optimize import linear_sum_assignment
  from sklearn.cluster import KMeans
  from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score, silhouette_score
  from tests import clustering_ref as R
  out = {"sklearn_version": np.array(sklearn.__version__)}
  for name, (N, D, K, _, _) in R.DATASETS.items():
    Z, y, _ = R.dataset(name)
    km = KMeans(K, n_init=200, random_state=5218).fit(Z)
    p = km.labels_
    u = np.unique(np.concatenate((y, p)))
    reward = np.zeros((u.size, u.size), np.int64)
    for p_, y_ in zip(np.searchsorted(u, p), np.searchsorted(u, y)):
      reward[p_, y_] += 1
    ind = linear_sum_assignment(reward.max() - reward)
    z64 = Z.astype(np.float64)
    inertia64 = sum(float(((z64[p == k] - z64[p == k].mean(axis=0)) ** 2).sum()) for k in range(K) if (p == k).any())
    out.update({f"{name}_asw": np.float64(silhouette_score(Z, y)), f"{name}_ari": np.float64(adjusted_rand_score(y, p)),
                f"{name}_nmi": np.float64(normalized_mutual_info_score(y, p)), f"{name}_uca": np.float64(reward[ind].sum() / p.size),
                f"{name}_km_labels": p.astype(np.int32), f"{name}_km_inertia": np.float64(km.inertia_), f"{name}_km_inertia64": np.float64(inertia64)})
    if R.QUALITY_SEEDS[name] != 3:   # the set of the quality test where it is another one: its inertia alone
      q = R.QUALITY_SEEDS[name]
      Zq = R.dataset(name, q)[0]
      pq, zq = KMeans(K, n_init=200, random_state=5218).fit(Zq), Zq.astype(np.float64)
      out[f"{name}_s{q}_km_inertia"] = np.float64(pq.inertia_)
      out[f"{name}_s{q}_km_inertia64"] = np.float64(sum(float(((zq[pq.labels_ == k] - zq[pq.labels_ == k].mean(axis=0)) ** 2).sum()) for k in range(K)))
    print(name, {k: (v if v.ndim == 0 else v.shape) for k, v in out.items() if k.startswith(name)})
  np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "clustering_fixture.npz"), **out)


if __name__ == "__main__":
  main()
