"""Float64 NumPy restatement of the full-covariance Gaussian mixture of smx_gmm_full.hip (include/sisua_hip.h: smx_gmm_full_fit,
smx_gmm_full_predict): scikit-learn's GaussianMixture(covariance_type='full') loop from a starting labelling.  What the device tests compare
against, and what the host tests hold to scikit-learn's own results (tests/golden/mixture_fixture.npz).  Written for clarity: Python loops
over the components, SciPy's Cholesky factor and triangular solve.  Sums are NumPy's; the device's are in another fixed order, which is what
the tolerance of tests/test_gpu_mixture.py is for."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

from tests import clustering_ref

EPS64 = np.finfo(np.float64).eps
LOG_2PI = np.log(2.0 * np.pi)
N_STARTS = 8

SETS = {   # name: (N, D, K, sep, seed, aniso)
    "m2": (2051, 2, 2, 1.0, 3, 1.5),     # more than one slice of the cells, a ragged tail
    "m3": (515, 3, 3, 1.5, 3, 1.0),      # a long loop: 22 iterations
    "m16": (1030, 16, 6, 0.9, 3, 0.8),   # mid width, several components
    "m33": (700, 33, 3, 0.6, 3, 0.5),    # a width that is no multiple of 4
    "m64": (1300, 64, 3, 0.5, 3, 0.5),   # the D limit
}
CLUSTER_SETS = ("d1", "d5", "d32")      # clustering_ref.dataset's sets (d64 is left out: its covariances are reg_covar-deep singular)
NAMES = list(SETS) + list(CLUSTER_SETS)
_MADE, _STARTS, _FITS = {}, {}, {}


def make(N, D, K, sep, seed, aniso):
  rs = np.random.RandomState(seed)
  c = rs.randn(K, D) * sep
  y = rs.randint(0, K, N)
  A = [np.eye(D) + aniso * rs.randn(D, D) / np.sqrt(D) for _ in range(K)]
  e = rs.randn(N, D)
  Z = (c[y] + np.einsum('nd,nde->ne', e, np.stack(A)[y])).astype(np.float32)
  return Z, y.astype(np.int64)


def dataset(name):
  """(Z [N, D] float32, y [N] int64, K): made once, read-only"""
  if name not in _MADE:
    if name in SETS:
      Z, y = make(*SETS[name])
      K = SETS[name][2]
    else:
      Z, y, _ = clustering_ref.dataset(name)
      K = clustering_ref.DATASETS[name][2]
      Z, y = Z.copy(), y.copy()
    Z.setflags(write=False); y.setflags(write=False)
    _MADE[name] = (Z, y, K)
  return _MADE[name]


def starts(name):
  """dict(labels_all [8, N] int32, inertia [8], best): clustering_ref.kmeans on 8 starts from RandomState(5218).choice(N, K, replace=False)"""
  if name not in _STARTS:
    Z, _, K = dataset(name)
    rs = np.random.RandomState(5218)
    idx = np.stack([rs.choice(Z.shape[0], K, replace=False) for _ in range(N_STARTS)]).astype(np.int32)
    km = clustering_ref.kmeans(Z, idx)
    lab = km["labels_all"].astype(np.int32)
    lab.setflags(write=False)
    _STARTS[name] = dict(labels_all=lab, inertia=km["inertia"], best=km["best"])
  return _STARTS[name]


def m_step(z, resp, reg_covar):
  """(weights [K], means [K, D], covariances [K, D, D]) of responsibilities resp [N, K]: the two-pass form"""
  N, D = z.shape
  nk = resp.sum(axis=0) + 10.0 * EPS64
  means = (resp.T @ z) / nk[:, None]
  cov = np.empty((resp.shape[1], D, D))
  for k in range(resp.shape[1]):
    diff = z - means[k]
    cov[k] = (resp[:, k] * diff.T) @ diff / nk[k]
    cov[k].flat[::D + 1] += reg_covar
  return nk / N, means, cov


def close(cov):
  """(chol_inv [K, D, D] lower triangular, logdet [K]) or None when a factor does not exist"""
  K, D, _ = cov.shape
  linv, logdet = np.zeros_like(cov), np.empty(K)
  for k in range(K):
    try:
      L = cholesky(cov[k], lower=True)
    except np.linalg.LinAlgError:
      return None
    if not np.all(np.isfinite(L)):
      return None
    linv[k] = solve_triangular(L, np.eye(D), lower=True)
    logdet[k] = -np.sum(np.log(np.diag(L)))
  return np.tril(linv), logdet


def log_prob(z, weights, means, chol_inv, logdet=None):
  """l_nk [N, K] = log w_k + logdet_k - (D log(2 pi) + |Linv_k (z_n - mu_k)|^2) / 2"""
  N, D = z.shape
  K = weights.shape[0]
  if logdet is None:
    logdet = np.array([np.sum(np.log(np.diag(chol_inv[k]))) for k in range(K)])
  l = np.empty((N, K))
  for k in range(K):
    y = (z - means[k]) @ chol_inv[k].T
    l[:, k] = np.log(weights[k]) + logdet[k] - (D * LOG_2PI + np.sum(y * y, axis=1)) / 2.0
  return l


def e_step(l):
  """(lse [N], resp [N, K]) with the row maximum taken out"""
  mx = l.max(axis=1, keepdims=True)
  lse = mx[:, 0] + np.log(np.exp(l - mx).sum(axis=1))
  return lse, np.exp(l - lse[:, None])


def fit_one(Z, init_labels, K, max_iter=100, tol=1e-3, reg_covar=1e-6):
  """One restart.  dict(status, lower_bound, n_iter, converged, weights, means, covariances, chol_inv, labels, lb_steps -- every |lb -
  lb_prev| of the loop --, gap -- the smallest difference between the best and the second-best l_nk over the cells of the final E-step --,
  lse -- the per-cell log-likelihood of the final E-step --, first -- the parameters of the first M-step)"""
  z = np.asarray(Z, np.float64)
  resp = np.zeros((z.shape[0], K))
  resp[np.arange(z.shape[0]), np.asarray(init_labels)] = 1.0
  w, mu, cov = m_step(z, resp, reg_covar)
  first = (w, mu, cov)
  out = dict(status=0, lower_bound=-np.inf, n_iter=0, converged=0, lb_steps=[], first=first)
  fac = close(cov)
  lb = -np.inf
  for it in range(1, max_iter + 1):
    if fac is None:
      break
    lse, resp = e_step(log_prob(z, w, mu, fac[0], fac[1]))
    prev, lb = lb, float(lse.mean())
    w, mu, cov = m_step(z, resp, reg_covar)
    fac = close(cov)
    out["n_iter"] = it
    if fac is None:
      break
    out["lb_steps"].append(abs(lb - prev))
    if abs(lb - prev) < tol:
      out["converged"] = 1
      break
  if fac is None:
    out.update(status=1, lower_bound=np.nan, converged=0)
    return out
  l = log_prob(z, w, mu, fac[0], fac[1])
  two = np.sort(l, axis=1)[:, -2:]
  out.update(lower_bound=lb, weights=w, means=mu, covariances=cov, chol_inv=fac[0], labels=l.argmax(axis=1).astype(np.int32),
             gap=float((two[:, 1] - two[:, 0]).min()), lse=e_step(l)[0])
  return out


def fit(Z, init_labels, K, **kw):
  """Every restart of init_labels [R, N]: dict(runs, best): the highest lower bound, ties to the lowest restart, failed restarts last"""
  runs = [fit_one(Z, row, K, **kw) for row in np.atleast_2d(init_labels)]
  best = -1
  for r, run in enumerate(runs):
    if run["status"] == 0 and (best < 0 or run["lower_bound"] > runs[best]["lower_bound"]):
      best = r
  return dict(runs=runs, best=max(best, 0), all_failed=best < 0)


def fitted(name):
  """the restatement's run of all 8 starts of a set with the default settings: made once"""
  if name not in _FITS:
    Z, _, K = dataset(name)
    _FITS[name] = fit(Z, starts(name)["labels_all"], K)
  return _FITS[name]
