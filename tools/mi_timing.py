"""Wall times of the gene x protein mutual-information matrix at the 8kly shape (4697 cells x 1998 genes x 12 proteins), continuous x
continuous and discrete x continuous: `sisua_amd.mutual_information` end to end (host preparation, copies and the device), with
scikit-learn's mutual_info_regression on 16 host threads on the same columns beside it -- on a slice of the genes, scaled to all of them
(profiles/mi_e2e.txt).
usage: python tools/mi_timing.py [device] [host] [slice=200]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sisua_amd import engine, mutual_information
from sisua_amd.data import synthetic_8kly

K = 3

def timed(f, reps=2):
  ts = []
  for _ in range(reps):
    t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)
  return min(ts), r

def problems():
  x, y = synthetic_8kly()
  lib = x.sum(1, keepdims=True)
  cont = np.log1p(x / lib * 1e4).astype(np.float64)   # normalised expression: continuous (the zeros are ties that the noise breaks)
  return {"continuous x continuous": (cont, False), "discrete x continuous": (x.astype(np.float64), True)}, y.astype(np.float64)

def device(name, X, disc, Y):
  t, mi = timed(lambda: mutual_information(X, Y, discrete_features=disc, discrete_targets=False, n_neighbors=K))
  # the device alone, on columns already prepared: what the host preparation and its noise stream cost is the difference
  cols, ycols = np.ascontiguousarray(X.T), np.ascontiguousarray(Y.T)
  t_dev, _ = timed(lambda: engine.mutual_info(cols, np.full(X.shape[1], disc), ycols, np.zeros(Y.shape[1], bool), K))
  n, g, p = X.shape[0], X.shape[1], Y.shape[1]
  print(f"{name}: {n} x {g} x {p}, n_neighbors {K}: mutual_information end to end {t:.2f} s; smx_mutual_info on prepared columns "
        f"{t_dev:.2f} s ({g * p / t_dev:.0f} pairs / s); mean MI {mi.mean():.4f}, max {mi.max():.4f}", flush=True)
  return mi

def host(name, X, disc, Y, n_slice):
  from sklearn.feature_selection import mutual_info_regression
  Xs = X[:, :n_slice]
  def run():
    return np.stack([mutual_info_regression(Xs, Y[:, p], discrete_features=disc, n_neighbors=K, random_state=1, n_jobs=16)
                     for p in range(Y.shape[1])], axis=1)
  t, ref = timed(run, reps=1)
  # (the noise of a slice is another part of the stream than the noise of the whole matrix: the device takes the slice again)
  ours = mutual_information(Xs, Y, discrete_features=disc, discrete_targets=False, n_neighbors=K)
  diff = f"; |device - scikit-learn| on the slice: max {np.abs(ours - ref).max():.2e}, pairs above 1e-12: {(np.abs(ours - ref) > 1e-12).sum()}"
  print(f"{name}: scikit-learn mutual_info_regression, n_jobs=16, {n_slice} genes x {Y.shape[1]} proteins: {t:.1f} s -> scaled to "
        f"{X.shape[1]} genes {t * X.shape[1] / n_slice:.0f} s{diff}", flush=True)

if __name__ == "__main__":
  what = [a for a in sys.argv[1:] if "=" not in a] or ["device", "host"]
  n_slice = int(dict(a.split("=") for a in sys.argv[1:] if "=" in a).get("slice", 200))
  probs, Y = problems()
  mutual_information(probs["continuous x continuous"][0][:512, :8], Y[:512], discrete_features=False)   # (a first call: code objects)
  for name, (X, disc) in probs.items():
    if "device" in what:
      device(name, X, disc, Y)
    if "host" in what:
      host(name, X, disc, Y, n_slice)
