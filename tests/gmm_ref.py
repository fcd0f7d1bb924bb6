"""Float64 NumPy restatement of the 1-D Gaussian mixtures of smx_gmm.hip (include/sisua_hip.h: smx_gmm1d_fit, smx_gmm1d_predict): the
normalisation with its float32 roundings, the host's seeding, scikit-learn's diagonal-covariance EM loop from random-cell starts, and
predict / predict_proba / score_samples.  What the device tests compare against, and what the host tests hold to scikit-learn's own results
(tests/golden/gmm_fixture.npz).  Sums are NumPy's (pairwise); the device's are in another fixed order, which is what the tolerances of
tests/test_gpu_label_threshold.py are for.  `dataset(name)`: small two-population count columns from np.random.RandomState."""
import numpy as np

EPS32 = np.finfo(np.float32).eps
EPS64 = np.finfo(np.float64).eps
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


# ---- normalisation -------------------------------------------------------------------------------------------------------------------
def column_sum(x) -> float:
  """the float64 sum of a column in cell order"""
  x = np.asarray(x, np.float64).ravel()
  return float(np.cumsum(x)[-1]) if x.size else 0.0


def log_norm_argument(x, s) -> np.ndarray:
  """float32: fl32(fl32(x / fl32(s + eps)) * 1e4), the argument of the log1p"""
  den = np.float32(s + float(EPS32))
  return (np.asarray(x, np.float32) / den) * np.float32(1e4)


def training_vector(x, remove_zeros=True) -> np.ndarray:
  x = np.asarray(x, np.float32).ravel()
  if not remove_zeros:
    return x
  pos = x[x > 0]
  return pos if pos.size == x.size else np.concatenate([np.zeros((1,), np.float32), pos])


def normalize(x, remove_zeros=True, log_norm=True, test_mode=False) -> np.ndarray:
  """float64: the reference's normalize() of one column"""
  x = np.asarray(x, np.float32).ravel()
  assert np.all(x >= 0), "Only support non-negative values"
  if not test_mode:
    x = training_vector(x, remove_zeros)
  if not log_norm:
    return x.astype(np.float64)
  return np.log1p(log_norm_argument(x, column_sum(x)).astype(np.float64))


def normalize_value(v, s, log_norm=True) -> np.ndarray:
  """raw values (seeds) on the scale of a column whose sum is s"""
  v = np.asarray(v, np.float32)
  return np.log1p(log_norm_argument(v, s).astype(np.float64)) if log_norm else v.astype(np.float64)


# ---- seeding -------------------------------------------------------------------------------------------------------------------------
def draw_init_raw(X, K, R, random_state=8, remove_zeros=True) -> np.ndarray:
  """ONE RandomState, column after column, restart after restart: K distinct cells of the column's training vector; float32 [C, R, K]"""
  rs = np.random.RandomState(random_state)
  out = np.empty((X.shape[1], R, K), np.float32)
  for c in range(X.shape[1]):
    tv = training_vector(X[:, c], remove_zeros)
    for r in range(R):
      out[c, r] = tv[rs.choice(tv.size, K, replace=False)]
  return out


# ---- EM ------------------------------------------------------------------------------------------------------------------------------
def m_step(t, resp, reg_covar):
  nk = resp.sum(axis=0) + 10.0 * EPS64
  mean = (resp * t[:, None]).sum(axis=0) / nk
  var = (resp * (t * t)[:, None]).sum(axis=0) / nk - mean * mean + reg_covar
  return nk / t.size, mean, var


def log_prob(t, w, mean, var):
  """[n, K]: log w_k + log N(t; mean_k, var_k)"""
  with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
    A = np.log(w) - HALF_LOG_2PI - 0.5 * np.log(var)
    d = t[:, None] - mean[None, :]
    return A[None, :] - (0.5 / var)[None, :] * (d * d)


def e_step(t, w, mean, var):
  """(the log-likelihood of every sample [n], the responsibilities [n, K])"""
  lp = log_prob(t, w, mean, var)
  with np.errstate(invalid="ignore", over="ignore"):
    mx = np.fmax.reduce(lp, axis=1, initial=-np.inf)
    e = np.exp(lp - mx[:, None])
    se = e.sum(axis=1)
    return mx + np.log(se), e / se[:, None]


def em(t, seeds, max_iter=120, tol=1e-3, reg_covar=1e-6):
  """One restart on the normalised training vector t from the normalised seeds [K]: hard assignment to the nearest seed (ties to the lowest
  index), an M-step, then scikit-learn's loop.  `trace`: the lower bound of every iteration."""
  K = seeds.size
  resp = np.eye(K)[np.argmin(np.abs(t[:, None] - seeds[None, :]), axis=1)]
  w, mean, var = m_step(t, resp, reg_covar)
  lb, trace, converged, n_iter = -np.inf, [], False, 0
  for it in range(1, max_iter + 1):
    prev = lb
    ll, resp = e_step(t, w, mean, var)
    lb = float(ll.sum() / t.size)
    w, mean, var = m_step(t, resp, reg_covar)
    trace.append(lb)
    n_iter = it
    with np.errstate(invalid="ignore"):
      if abs(lb - prev) < tol:
        converged = True
        break
  return dict(weights=w, means=mean, variances=var, lower_bound=lb, n_iter=n_iter, converged=converged, trace=np.array(trace))


def pick_best(lb) -> int:
  """the highest lower bound, ties to the lowest restart, NaN last"""
  bi = 0
  for r in range(1, len(lb)):
    if lb[r] > lb[bi] or (lb[bi] != lb[bi] and lb[r] == lb[r]):
      bi = r
  return bi


def fit(X, init_raw, max_iter=120, tol=1e-3, reg_covar=1e-6, remove_zeros=True, log_norm=True):
  """Every restart of every column; the outputs of engine.k_gmm1d_fit(all_params=True) plus `traces` [C][R]"""
  X = np.asarray(X, np.float32)
  C, R, K = init_raw.shape
  out = dict(lower_bound=np.empty((C, R)), n_iter=np.empty((C, R), np.int32), converged=np.empty((C, R), np.int32), best=np.empty((C,), np.int32),
             weights=np.empty((C, K)), means=np.empty((C, K)), variances=np.empty((C, K)), n_train=np.empty((C,), np.int64),
             col_sum=np.empty((C,)), params_all=np.empty((C, R, 3, K)), traces=[])
  for c in range(C):
    tv = training_vector(X[:, c], remove_zeros)
    s = column_sum(X[:, c])
    t = normalize_value(tv, s, log_norm)
    out["n_train"][c], out["col_sum"][c] = tv.size, s
    runs = [em(t, normalize_value(init_raw[c, r], s, log_norm), max_iter, tol, reg_covar) for r in range(R)]
    for r, run in enumerate(runs):
      out["lower_bound"][c, r], out["n_iter"][c, r], out["converged"][c, r] = run["lower_bound"], run["n_iter"], run["converged"]
      out["params_all"][c, r] = np.stack([run["weights"], run["means"], run["variances"]])
    b = pick_best(out["lower_bound"][c])
    out["best"][c] = b
    out["weights"][c], out["means"][c], out["variances"][c] = out["params_all"][c, b]
    out["traces"].append([run["trace"] for run in runs])
  return out


# ---- prediction ----------------------------------------------------------------------------------------------------------------------
def ci_bound(loc, scale, ci_threshold):
  from scipy.stats import norm
  z = float(norm.ppf(0.5 + abs(ci_threshold) / 2.0))
  return loc - z * scale if ci_threshold < 0 else loc + z * scale


def thresholds(means, variances, order, positive_component=1, ci_threshold=-0.68):
  rows = np.arange(means.shape[0])
  pos = order[:, positive_component]
  return ci_bound(means[rows, pos], np.sqrt(variances[rows, pos]), ci_threshold)


def predict(X, weights, means, variances, positive_component=1, ci_threshold=-0.68, log_norm=True):
  """(prob [N, C], bin [N, C] float32, score [N, C], t [N, C], threshold [C]) of a matrix under fitted mixtures [C, K]"""
  X = np.asarray(X, np.float32)
  N, C = X.shape
  K = means.shape[1]
  order = np.argsort(means, axis=1, kind="stable")
  thr = thresholds(means, variances, order, positive_component, ci_threshold)
  prob, bins, score, T = np.empty((N, C)), np.empty((N, C), np.float32), np.empty((N, C)), np.empty((N, C))
  for c in range(C):
    t = normalize(X[:, c], log_norm=log_norm, test_mode=True)
    ll, resp = e_step(t, weights[c], means[c], variances[c])
    prob[:, c] = resp[:, order[c, positive_component:]].sum(axis=1) / (K - positive_component)
    bins[:, c] = t >= thr[c]
    score[:, c], T[:, c] = ll, t
  return prob, bins, score, T, thr


# ---- data ----------------------------------------------------------------------------------------------------------------------------
# name -> (n_cells, the kinds of its columns, K, R, remove_zeros, log_norm, data seed)
#   pos     two populations of counts, every cell positive
#   zeros   the same with about 60 % of the cells set to zero
#   const   one positive value in every cell
#   few     two distinct positive values (fewer than K where K >= 3: a component is empty at the start)
# The degenerate kinds sit in sets without log_norm, on small whole numbers: there every sum of a collapsed component is exact.  Under
# log_norm the variance of a component that sits on one repeated value is reg_covar plus a rounding residue of t^2 (condition number t^2 /
# reg_covar, about 1e7), which no two orders of summation reproduce to 1e-8; see `const_log` and DESIGN.md 4n.
DATASETS = {
    "n257": (257, ["pos"], 2, 1, True, True, 11),
    "n1000": (1000, ["pos", "zeros", "pos"], 3, 8, True, True, 12),
    "n4096": (4096, ["zeros", "pos", "zeros"], 5, 8, True, True, 13),
    "n4097": (4097, ["zeros"], 2, 8, True, True, 14),
    "n4099": (4099, ["pos", "zeros"] * 6 + ["pos"], 2, 8, True, True, 15),
    "raw": (1000, ["pos", "const", "few"], 3, 8, True, False, 16),
    "keep": (1000, ["zeros", "pos", "zeros"], 2, 1, False, True, 17),
    "const_log": (257, ["const"], 2, 1, True, True, 18),
}
MAIN = [n for n in DATASETS if n != "const_log"]


def column(kind, N, rs) -> np.ndarray:
  if kind == "const":
    return np.full((N,), 4.0, np.float32)
  if kind == "few":
    return np.where(rs.uniform(size=N) < 0.4, 2.0, 16.0).astype(np.float32)
  high = rs.uniform(size=N) < 0.35
  lam = np.where(high, 180.0, 14.0) * rs.gamma(6.0, 1.0 / 6.0, size=N)
  x = (rs.poisson(lam) + 1).astype(np.float32)
  if kind == "zeros":
    x[rs.uniform(size=N) < 0.6] = 0.0
  return x


def dataset(name):
  """-> (X [N, C] float32, init_raw [C, R, K] float32, dict(K, R, remove_zeros, log_norm))"""
  N, kinds, K, R, remove_zeros, log_norm, seed = DATASETS[name]
  rs = np.random.RandomState(seed)
  X = np.stack([column(k, N, rs) for k in kinds], axis=1)
  return X, draw_init_raw(X, K, R, 8, remove_zeros), dict(K=K, R=R, remove_zeros=remove_zeros, log_norm=log_norm)


# the sets of tests/golden/gmm_fixture.npz (scikit-learn's results through the reference's own code): name -> (n_cells, data seed); columns
# pos, zeros
FIXTURE_SETS = {"s300a": (300, 21), "s300b": (300, 22), "s300c": (300, 23), "s2000a": (2000, 24), "s2000b": (2000, 25), "s2000c": (2000, 26)}
FIXTURE_K = (2, 3)


def fixture_matrix(name) -> np.ndarray:
  N, seed = FIXTURE_SETS[name]
  rs = np.random.RandomState(seed)
  return np.stack([column(k, N, rs) for k in ("pos", "zeros")], axis=1)


_FITS = {}


def fitted(name):
  """the restatement's fit of a data set: made once, not to be changed"""
  if name not in _FITS:
    X, seeds, kw = dataset(name)
    _FITS[name] = fit(X, seeds, remove_zeros=kw["remove_zeros"], log_norm=kw["log_norm"])
  return _FITS[name]
