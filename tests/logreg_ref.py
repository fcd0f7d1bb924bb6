"""A NumPy restatement of smx_logreg.hip (include/sisua_hip.h): the L2-penalised logistic objective in scikit-learn's
mean form, its gradient, the L-BFGS solve and the logits.  No scikit-learn here: tests/test_logreg_host.py holds this file to it.

  F(W, b) = (1/N) sum_i loss_i + ||W||^2 / (2 C N), the intercept unpenalised
  multinomial (K >= 3): K logit rows, loss_i = logsumexp(z_i) - z_{i, y_i}
  binary (K = 2):       ONE logit row (class 1) beside an implicit zero logit, loss_i = softplus(z_i) - y_i z_i

`objective` is the float64 form the solver uses.  `evaluate` is the yardstick of the device's two matrix launches: the same quantities from
the float32 matrix in np.longdouble, each with a first-order bound on |device - exact| derived from the additions the kernels make (see
`evaluate`).  `fit` restates the solver step for step: L-BFGS with memory 10 as the two-loop recursion on coefficients over the basis
{s_j, y_j, g} from the basis' Gram matrix (the device keeps that matrix on the host and the vectors on the device), Armijo backtracking
with c1 = 1e-4 from t = 1 (1 / max|g| on the first iteration), halved per failure, at most 30 trials, a pair with s.y <= 0 skipped, stop at
max|g| <= tol or max_iter.  Close to the optimum a step changes F by less than F's own rounding (the bound of `evaluate` is about 2^-44 F
per evaluation), and the Armijo test would then decide on noise: a trial with |F_new - F| <= 2^-43 |F| is accepted if it lowers max|g|, the
quantity the stopping rule reads -- a strictly decreasing sequence, so no cycle.  `k_logreg_eval`, `k_logreg_fit` and `k_logreg_decision` have the signatures and return values of the engine's,
so the host tests put them in its place."""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -53
LD = np.longdouble
REF = float(np.finfo(LD).eps) / 2.0 / EPS   # one rounding of the yardstick's arithmetic in units of 2^-53 (2^-11 where long double has 64 bits)
ULP_EXP = ULP_LOG = 2.0                     # the device's float64 exp and log, taken as within 2 ulp (the ROCm device library documents 1)
MEMORY, TRIALS, ARMIJO = 10, 30, 1e-4
FLAT = 2.0 ** -43   # two evaluations of F differ by their rounding alone below this share of |F| (see `fit`)


def dense32(x):
  return np.ascontiguousarray(x.toarray() if sp.issparse(x) else x, dtype=np.float32)


def _softmax_terms(Z, y, binary):
  """full logits [N, Kf] (the implicit zero logit as a last column in the binary form), the target column, shift, exp, sum"""
  if binary:
    Z = np.concatenate([Z, np.zeros((Z.shape[0], 1), Z.dtype)], axis=1)
    idx = np.where(np.asarray(y) == 1, 0, 1)
  else:
    idx = np.asarray(y)
  m = Z.max(axis=1)
  D = Z - m[:, None]
  E = np.exp(D)
  s = E.sum(axis=1)
  return Z, idx, m, D, E, s


def objective(X, y, K, W, b, C=1.0, fit_intercept=True):
  """F, gW [Kz, G], gb [Kz] in the dtype of X (float64 for the solver)"""
  N, binary = X.shape[0], K == 2
  Kz = 1 if binary else K
  W, b = np.asarray(W, X.dtype).reshape(Kz, -1), (np.asarray(b, X.dtype).reshape(Kz) if fit_intercept else np.zeros(Kz, X.dtype))
  Z, idx, m, D, E, s = _softmax_terms(X @ W.T + b, y, binary)
  rows = np.arange(N)
  loss = m + np.log(s) - Z[rows, idx]
  R = E / s[:, None]
  R[rows, idx] -= 1.0
  R = R[:, :Kz]
  F = loss.sum() / N + (W * W).sum() / (2.0 * C * N)
  gW = R.T @ X / N + W / (C * N)
  gb = R.sum(axis=0) / N if fit_intercept else np.zeros(Kz, X.dtype)
  return F, gW, gb


def evaluate(x, y, K, W, b, C=1.0, fit_intercept=True):
  """dict(F, gW, gb: the exact values from the float32 matrix, as float64; bF, bgW, bgb: bounds on |device - exact|).

  With u = 2^-53 and a sum bounded by (the roundings of its longest chain) x u x (the sum of its absolute terms), to first order:
    logit      a lane makes 4 ceil(ld / 256) fmas, the halving tree 6 additions, the intercept 1: n_z roundings on sum_j |x_ij w_kj| + |b_k|
               -> Ez_ik (0 for the implicit zero logit).
    softmax    any shift cancels, so the device's own max counts as exact.  A term exp(z_k - m) carries Ez_k + u |z_k - m| in its
               argument and ULP_EXP u of the function; their sum n_s = ceil(Kf / 64) + 7 roundings; the log ULP_LOG u |log s|; m + log s
               and the subtraction of z_y one rounding each.
    residual   r_k = p_k - [y = k]: p_k's relative error is the numerator's, the denominator's and the division's; the subtraction u |r_k|.
    F          the losses: 3 additions in a wave, 2 across the waves, ceil(workgroups / 256) + 8 in the closing sum.  ||W||^2: the square,
               8 in a workgroup, ceil(partials / 256) + 8 in the closing sum.  Scalings and the last addition: 6 u F.
    gradient   a slice adds 64 rows by fma, then the slices in order: 64 + slices roundings on sum_i |r_ik x_ij|, plus sum_i Er_ik
               |x_ij|; the scalings and the last addition 4 u (|data term| + |penalty term|).  The intercept's: ceil(N / 256) + 8.
  The yardstick's own roundings (np.longdouble) are added to every chain, and 1 % to the whole for the second order."""
  X = dense32(x).astype(LD)
  N, G = X.shape
  binary = K == 2
  Kz, Kf = (1, 2) if binary else (K, K)
  ld = (G + 3) // 4 * 4
  W = np.asarray(W, np.float64).reshape(Kz, G).astype(LD)
  b = (np.asarray(b, np.float64).reshape(Kz) if fit_intercept else np.zeros(Kz)).astype(LD)
  u, invN, lam = LD(EPS), LD(1.0) / N, LD(1.0) / (LD(C) * N)
  rows = np.arange(N)

  n_z = 4 * -(-ld // 256) + 6 + 1 + G * REF
  Z0 = X @ W.T + b
  Ez = n_z * u * (np.abs(X) @ np.abs(W).T + np.abs(b))
  Z, idx, m, D, E, s = _softmax_terms(Z0, y, binary)
  if binary:
    Ez = np.concatenate([Ez, np.zeros((N, 1), LD)], axis=1)
  P = E / s[:, None]
  n_s = -(-Kf // 64) + 7 + Kf * REF
  arg = Ez + u * np.abs(D)                                        # the error of a term's argument
  den = (P * arg).sum(axis=1) + (ULP_EXP + n_s) * u               # the relative error of s
  lse = m + np.log(s)
  loss = lse - Z[rows, idx]
  E_loss = den + ULP_LOG * u * np.abs(np.log(s)) + u * np.abs(lse) + Ez[rows, idx] + u * np.abs(loss)
  R = P.copy()
  R[rows, idx] -= 1.0
  E_r = P * (arg + ULP_EXP * u + den[:, None] + u) + u * np.abs(R)
  R, E_r = R[:, :Kz], E_r[:, :Kz]

  n_loss, n_part = -(-N // 16), (Kz + 1) * -(-ld // 256)
  n_F = 3 + 2 + -(-n_loss // 256) + 8 + N * REF
  n_w = 1 + 8 + -(-n_part // 256) + 8 + Kz * G * REF
  wsq = (W * W).sum()
  F = loss.sum() * invN + 0.5 * lam * wsq
  bF = invN * (E_loss.sum() + n_F * u * np.abs(loss).sum()) + 0.5 * lam * n_w * u * wsq + 6 * u * np.abs(F)

  n_g = 64 + -(-N // 64) + N * REF
  data, pen = R.T @ X * invN, W * lam
  gW = data + pen
  bgW = invN * (E_r.T @ np.abs(X) + n_g * u * (np.abs(R).T @ np.abs(X))) + 4 * u * (np.abs(data) + np.abs(pen))
  if fit_intercept:
    n_b = -(-N // 256) + 8 + N * REF
    gb = R.sum(axis=0) * invN
    bgb = invN * (E_r.sum(axis=0) + n_b * u * np.abs(R).sum(axis=0)) + 2 * u * np.abs(gb)
  else:
    gb, bgb = np.zeros(Kz, LD), np.zeros(Kz, LD)
  f64 = lambda a: np.asarray(a, np.float64)
  tiny = 1e-300   # (a term that underflows has no relative error to speak of)
  return dict(F=float(F), gW=f64(gW), gb=f64(gb), bF=float(bF) * 1.01 + tiny, bgW=f64(bgW) * 1.01 + tiny, bgb=f64(bgb) * 1.01 + tiny)


def fit(x, y, K, C=1.0, fit_intercept=True, tol=1e-4, max_iter=100, W0=None, b0=None):
  """the solver of smx_logreg_fit in float64 -> dict(W [Kz, G], b [Kz], F, gmax, n_iter, n_eval, converged)"""
  X = dense32(x).astype(np.float64)
  G = X.shape[1]
  Kz = 1 if K == 2 else K
  nw = Kz * G

  def ev(th):
    F, gW, gb = objective(X, y, K, th[:nw].reshape(Kz, G), th[nw:], C, fit_intercept)
    g = np.concatenate([gW.ravel(), gb])
    return float(F), g, float(np.abs(g).max())

  theta = np.zeros(nw + Kz)
  if W0 is not None:
    theta[:nw] = np.asarray(W0, np.float64).ravel()
    if fit_intercept:
      theta[nw:] = np.asarray(b0, np.float64).ravel()
  F, g, gm = ev(theta)
  n_eval, it = 1, 0
  if not (np.isfinite(F) and np.isfinite(gm)):
    raise FloatingPointError("the objective is not finite at the start point")
  pairs = []   # (s, y), oldest first
  while gm > tol and it < max_iter:
    # the two-loop recursion on coefficients over the basis V = [s_0 .., y_0 .., g] with its Gram matrix B
    n = len(pairs)
    V = np.stack([p[0] for p in pairs] + [p[1] for p in pairs] + [g])
    B = V @ V.T
    coef, alpha = np.zeros(2 * n + 1), np.zeros(n)
    coef[2 * n] = 1.0
    for i in range(n - 1, -1, -1):
      alpha[i] = coef @ B[i] / B[i, n + i]
      coef[n + i] -= alpha[i]
    if n:
      coef *= B[n - 1, 2 * n - 1] / B[2 * n - 1, 2 * n - 1]
    for i in range(n):
      coef[i] += alpha[i] - coef @ B[n + i] / B[i, n + i]
    gd = -(coef @ B[2 * n])
    if not gd < 0.0:   # (not a descent direction: steepest descent, the history dropped)
      pairs, coef, V = [], np.ones(1), g[None, :]
      gd = -float(g @ g)
      if not gd < 0.0:
        break
    d = -(coef @ V)
    t, ok = (1.0 / gm if it == 0 else 1.0), False
    for _ in range(TRIALS):
      th_new = theta + t * d
      F_new, g_new, gm_new = ev(th_new)
      n_eval += 1
      if np.isfinite(F_new) and np.isfinite(gm_new) and (F_new <= F + ARMIJO * t * gd or
                                                         (abs(F_new - F) <= FLAT * abs(F) and gm_new < gm)):
        ok = True
        break
      t *= 0.5
    if not ok:
      break
    s_vec, y_vec = th_new - theta, g_new - g
    theta, F, g, gm = th_new, F_new, g_new, gm_new
    if s_vec @ y_vec > 0.0:
      pairs = (pairs + [(s_vec, y_vec)])[-MEMORY:]
    it += 1
  return dict(W=theta[:nw].reshape(Kz, G).copy(), b=theta[nw:].copy(), F=F, gmax=gm, n_iter=it, n_eval=n_eval, converged=bool(gm <= tol))


# ---- the engine's entries ---------------------------------------------------------------------------------------------------------------
def k_logreg_eval(x, labels, n_classes, W, b, C_=1.0, fit_intercept=True):
  r = evaluate(x, np.asarray(labels), int(n_classes), W, b, C_, fit_intercept)
  return dict(F=r["F"], gW=r["gW"], gb=r["gb"])


def k_logreg_fit(x, labels, n_classes, C_=1.0, fit_intercept=True, tol=1e-4, max_iter=100, W0=None, b0=None):
  return fit(x, np.asarray(labels), int(n_classes), C_, fit_intercept, tol, max_iter, W0, b0)


def k_logreg_decision(x, W, b, n_classes, block_rows=0):
  Kz = 1 if int(n_classes) == 2 else int(n_classes)
  X = dense32(x).astype(np.float64)
  z = X @ np.asarray(W, np.float64).reshape(Kz, -1).T + np.asarray(b, np.float64).reshape(Kz)
  return z[:, 0] if Kz == 1 and int(n_classes) == 2 else z


# ---- fixtures shared by the host and the GPU tests ------------------------------------------------------------------------------------
CASES = {"k3": (257, 13, 3), "k4": (300, 40, 4), "binary": (130, 70, 2), "k5": (515, 130, 5)}   # name -> (cells, genes, classes)


def make_case(N, G, K, seed=0):
  """log1p of Poisson counts whose rates depend on the class -> (X float32 [N, G], y int32 [N], every class present).  The class effect
  (a factor exp(N(0, 0.15)) on a rate of 2) leaves the classes overlapping, as cell groups do: the optimum's F stays above
  P tol^2 C N / (2 x 1e-12) at tol = 1e-9 for every case (P parameters; the curvature is at least 1 / (C N)), the size at which stopping at
  max|g| <= tol guarantees F to 1e-12 relative -- what tests/test_logreg_host.py asks of F."""
  rng = np.random.RandomState(500 + seed)
  y = np.concatenate([np.arange(K), rng.randint(0, K, N - K)]).astype(np.int32)
  rng.shuffle(y)
  rate = 2.0 * np.exp(rng.normal(0.0, 0.15, (K, G)))
  return np.log1p(rng.poisson(rate[y])).astype(np.float32), y


def case(name):
  N, G, K = CASES[name]
  return make_case(N, G, K, seed=sorted(CASES).index(name)) + (K,)
