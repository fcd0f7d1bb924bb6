"""Wall times of `SingleCellOMIC.get_importance_matrix` on the 4697 x 1998 benchmark counts with 12 protein levels (each cut into 10
quantile classes; 3522 training cells, of which every fit holds 10 % out), dense and CSR, end to end: 12 fits of 100 stages of 10 depth-3
trees, the training and test accuracies.  The time inside the library's entries (`engine.k_gbt_fit`, `engine.k_gbt_decision`: the host's
checks, the copy of the matrix, all launches, the trees back) is split out from the Python around them; one `engine.k_gbt_bin` gives the
share of the column sorts.  scikit-learn on the same host fits ONE protein for 10 stages, one run, and the full run is extrapolated from
it (x 10 stages x 12 proteins) -- written down as an extrapolation (profiles/gbt_e2e.txt).
usage: python tools/gbt_timing.py [reps=3] [sk_stages=10]"""
import os, sys, time, warnings
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sisua_amd
from sisua_amd import boosting, engine
from sisua_amd.data import SingleCellOMIC, synthetic_8kly

INSIDE = {"t": 0.0, "calls": 0, "stages": 0}


def wrap(name):
  real = getattr(engine, name)
  def timed_entry(*a, **kw):
    t = time.perf_counter(); r = real(*a, **kw); INSIDE["t"] += time.perf_counter() - t
    INSIDE["calls"] += 1
    if name == "k_gbt_fit":
      INSIDE["stages"] += r["n_estimators_"]
    return r
  setattr(engine, name, timed_entry)


def show(ts):
  return f"min {min(ts):.3f} s, median {np.median(ts):.3f} s, max {max(ts):.3f} s of {len(ts)}"


if __name__ == "__main__":
  args = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
  reps, sk_stages = int(args.get("reps", 3)), int(args.get("sk_stages", 10))
  print(f"host threads {os.environ.get('OMP_NUM_THREADS', '?')} (of {os.cpu_count()} CPUs)", flush=True)
  x, prot = synthetic_8kly()
  print(f"matrix {x.shape}, proteins {prot.shape}, {100.0 * (x != 0).mean():.1f} % non-zero, {len(np.unique(x))} distinct counts", flush=True)
  sisua_amd.GradientBoostingClassifier(n_estimators=2).fit(x[:512], np.arange(512) % 3)   # (a first call: code objects)
  t = time.perf_counter(); engine.k_gbt_bin(x); t_bin = time.perf_counter() - t
  print(f"k_gbt_bin of the whole matrix (checks, copy, {x.shape[1]} column sorts, bins back): {t_bin:.3f} s", flush=True)
  wrap("k_gbt_fit"); wrap("k_gbt_decision")
  out = {}
  for name, M in (("dense", x), ("CSR", sp.csr_matrix(x))):
    total, inside = [], []
    for _ in range(reps):
      sco = SingleCellOMIC(M, omic="transcriptomic")
      sco.add_omic("proteomic", prot)
      INSIDE.update(t=0.0, calls=0, stages=0)
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = time.perf_counter(); out[name] = sco.get_importance_matrix(); total.append(time.perf_counter() - t)
      inside.append(INSIDE["t"])
    print(f"{name}: get_importance_matrix end to end: {show(total)}", flush=True)
    print(f"{name}: of it inside the library's entries ({INSIDE['calls']} calls, {INSIDE['stages']} stages): {show(inside)}", flush=True)
  print(f"dense and CSR give the same bits: {out['dense'].tobytes() == out['CSR'].tobytes()}; matrix {out['dense'].shape}, column sums "
        f"{np.round(out['dense'].sum(0), 6).tolist()}", flush=True)
  # scikit-learn on the same host: one protein, sk_stages stages, one run
  import sklearn
  from sklearn.ensemble import GradientBoostingClassifier as Sk
  y = np.stack([boosting.quantile_codes(prot[:, j], 10) for j in range(prot.shape[1])], axis=1)
  rand = np.random.RandomState(1)
  ids = rand.permutation(x.shape[0])
  train = ids[:int(0.75 * x.shape[0])]
  t = time.perf_counter()
  sk = Sk(n_estimators=sk_stages, random_state=rand.randint(1e8), n_iter_no_change=100).fit(x[train], y[train, 0])
  t_sk = time.perf_counter() - t
  print(f"scikit-learn {sklearn.__version__} GradientBoostingClassifier(n_estimators={sk_stages}, n_iter_no_change=100) on protein 0 of the same "
        f"training cells, this host, one run: {t_sk:.1f} s for {sk.n_estimators_} stages", flush=True)
  print(f"EXTRAPOLATED (not run): x {100 // sk_stages} for 100 stages x {prot.shape[1]} proteins = {t_sk * (100 / sk_stages) * prot.shape[1] / 60.0:.0f} min "
        "for the reference's whole call", flush=True)
