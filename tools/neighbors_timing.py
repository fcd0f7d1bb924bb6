"""Wall times of SingleCellOMIC.dimension_reduce(100) and neighbors() on the device, their entries timed alone, scikit-learn's
PCA(svd_solver='full') + NearestNeighbors(algorithm='brute') on 16 host threads beside them, and the scaling of the exact kNN with n
(profiles/neighbors_e2e.txt).  usage: python tools/neighbors_timing.py [small] [large] [host] [knn]
(default: all; `small large` alone is what one `rocprofv3 --kernel-trace --stats -- python tools/neighbors_timing.py small large` traces)."""
import os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sisua_amd import engine, neighbors
from sisua_amd.data import SingleCellOMIC, synthetic_8kly, _counts

def timed(f, reps=3):
  ts = []
  for _ in range(reps):
    t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)
  return min(ts), r

def device(name, x):
  om = SingleCellOMIC(x).normalize(total=True, log1p=True)
  for label, o in (("dense", om), ("csr", SingleCellOMIC(sp.csr_matrix(om.numpy())))):
    def pca():
      o._pca.clear(); return o.dimension_reduce(n_components=100)
    def nbr():
      o._neighbors.clear(); return o.neighbors()
    t_pca, s = timed(pca)
    t_cov, _ = timed(lambda: engine.k_pca_cov(o.numpy()))
    m = o.get_pca()
    t_proj, _ = timed(lambda: m.transform(o.numpy()))
    t_nb, _ = timed(nbr)     # (PCA cached: kNN + UMAP rows + assembly)
    t_knn, (idx, dist) = timed(lambda: engine.k_knn(s, 11))
    t_umap, _ = timed(lambda: engine.k_knn_umap(*neighbors.self_table(idx, dist)))
    print(f"{name} {label}: dimension_reduce(100) {t_pca*1e3:.1f} ms (smx_pca_cov {t_cov*1e3:.1f}, smx_pca_project {t_proj*1e3:.1f}, "
          f"host eigh + rest {max(0.0, t_pca - t_cov - t_proj)*1e3:.1f}); neighbors() after PCA {t_nb*1e3:.1f} ms "
          f"(smx_knn {t_knn*1e3:.1f}, smx_knn_umap {t_umap*1e3:.1f}, host assembly {max(0.0, t_nb - t_knn - t_umap)*1e3:.1f})", flush=True)
  return om.numpy()

def host(name, L):
  from sklearn.decomposition import PCA
  from sklearn.neighbors import NearestNeighbors
  t_pca, s = timed(lambda: PCA(n_components=100, svd_solver="full").fit_transform(L), reps=1)
  t_nn, _ = timed(lambda: NearestNeighbors(n_neighbors=12, algorithm="brute", n_jobs=16).fit(s).kneighbors(s), reps=1)
  print(f"{name} scikit-learn, 16 host threads: PCA(svd_solver='full') {t_pca*1e3:.1f} ms, NearestNeighbors(brute) {t_nn*1e3:.1f} ms", flush=True)

def knn_scaling():
  for n in (4096, 16384, 65536, 131072):
    z = np.random.default_rng(n).standard_normal((n, 100)).astype(np.float32)
    t, _ = timed(lambda: engine.k_knn(z, 11), reps=2 if n < 100000 else 1)
    print(f"smx_knn n = {n}, D = 100, k = 11: {t*1e3:.1f} ms = {n * n * 100 * 3 / t / 1e12:.2f} T float64 op/s (3 n^2 D operations)", flush=True)

if __name__ == "__main__":
  what = sys.argv[1:] or ["small", "large", "host", "knn"]
  mats = {}
  if "small" in what:
    mats["4697 x 1998 (synthetic_8kly)"] = synthetic_8kly()[0]
  if "large" in what:
    mats["32768 x 2000"] = _counts(32768, 2000, np.random.default_rng(9), 2.9, 0.28, 0.93)
  for name, x in mats.items():
    L = device(name, x)
    if "host" in what:
      host(name, L)
  if "knn" in what:
    knn_scaling()
