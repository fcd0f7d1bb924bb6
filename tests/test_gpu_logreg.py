"""smx_logreg.hip on the device against the restatement (tests/logreg_ref.py), through engine.k_logreg_*, then `sisua_amd.LogisticRegression`
and `SingleCellOMIC.rank_vars_groups(method='logreg')`.

The two matrix launches (`k_logreg_eval`): F and every gradient element within the first-order rounding bound that `logreg_ref.evaluate`
derives from the additions the kernels make, at a random (W, b) and at zero.  Shapes, the smallest at which the launches can go wrong:
rows 1 (a wave with one row), 63 / 64 / 65 (a ragged slice, a whole one, one row into the second) and 257 (five slices, two workgroups'
worth of loss partials and a ragged last wave); genes 1 and 3 (an ld that pads), 13, 257 (one column trip of 256 and a bit: ld 260) and
261 (ld 264); classes 2 (the binary form), 3 (a partial group of 4), 5 (two groups) and 9 (three).  Every matrix has an all-zero row (an
empty CSR row) where it has three rows, and its last class has a single row.  Saturation: weights scaled until the logits reach about
+-800, which exercises the max shift and both tails of the binary softplus.

The solver (`k_logreg_fit`): converged with max|g| <= tol as this file recomputes it in float64, and coefficients within 4 DIS of the
restatement's, DIS being scikit-learn's own lbfgs / newton-cg disagreement on the case (tests/test_logreg_host.py).  Iteration counts are
not compared: a last-bit difference may change a line-search decision.  The same bits: two calls, dense and CSR input, any block_rows."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from tests import logreg_ref as R

pytestmark = pytest.mark.gpu

# name -> (rows, genes, classes, fit_intercept)
SHAPES = {
    "n1_g1_bin": (1, 1, 2, True),
    "n1_g13_k3": (1, 13, 3, True),
    "n63_g3_k5": (63, 3, 5, True),
    "n64_g257_bin": (64, 257, 2, True),
    "n65_g261_k9": (65, 261, 9, True),
    "n65_g1_k9": (65, 1, 9, True),
    "n257_g13_k3": (257, 13, 3, True),
    "n257_g261_k5_nob": (257, 261, 5, False),
    "n257_g3_bin_nob": (257, 3, 2, False),
    "n63_g257_k3": (63, 257, 3, True),
    "n64_g13_k9": (64, 13, 9, True),
}
TOL = 1e-9
FIT_CASES = ("k3", "binary", "k4")


@functools.lru_cache(maxsize=None)
def shape_case(name):
  """the matrix, the labels, a random (W, b) and the restatement's values with their bounds at it and at zero: computed once, shared"""
  N, G, K, icpt = SHAPES[name]
  rng = np.random.RandomState(sorted(SHAPES).index(name))
  x = np.log1p(rng.poisson(2.0, (N, G))).astype(np.float32)
  y = rng.randint(0, max(K - 1, 1), N).astype(np.int32)
  if N >= 3:
    x[2] = 0.0                      # an all-zero row: an empty CSR row
    y[N // 2] = K - 1               # the last class has a single row
  Kz = 1 if K == 2 else K
  W, b = rng.normal(0.0, 0.5, (Kz, G)), rng.normal(0.0, 0.5, Kz)
  zero = (np.zeros((Kz, G)), np.zeros(Kz))
  ref = {"random": R.evaluate(x, y, K, W, b, 0.7, icpt), "zero": R.evaluate(x, y, K, *zero, 0.7, icpt)}
  for a in (x, y, W, b):
    a.setflags(write=False)
  return dict(x=x, y=y, K=K, icpt=icpt, at={"random": (W, b), "zero": zero}, ref=ref)


def hold(got, ref, what):
  eF, eW, eb = abs(got["F"] - ref["F"]), np.abs(got["gW"] - ref["gW"]), np.abs(got["gb"] - ref["gb"])
  print(f"{what}: |dF| {eF:.2e} of {ref['bF']:.2e}   max |dgW| / bound {(eW / ref['bgW']).max():.3f}   max |dgb| / bound {(eb / ref['bgb']).max():.3f}")
  assert np.isfinite(got["F"]) and np.isfinite(got["gW"]).all() and np.isfinite(got["gb"]).all()
  assert eF <= ref["bF"], what
  assert (eW <= ref["bgW"]).all(), what
  assert (eb <= ref["bgb"]).all(), what


@pytest.mark.parametrize("name", list(SHAPES))
def test_eval_is_inside_the_derived_bound(name):
  from sisua_amd import engine
  c = shape_case(name)
  for at, (W, b) in c["at"].items():
    got = engine.k_logreg_eval(c["x"], c["y"], c["K"], W, b, 0.7, c["icpt"])
    hold(got, c["ref"][at], f"{name} {at}")
    again = engine.k_logreg_eval(sp.csr_matrix(c["x"]), c["y"], c["K"], W, b, 0.7, c["icpt"])   # CSR: the same bits
    assert again["F"] == got["F"] and again["gW"].tobytes() == got["gW"].tobytes() and again["gb"].tobytes() == got["gb"].tobytes()
    if not c["icpt"]:
      assert not got["gb"].any()


@pytest.mark.parametrize("name", ["n64_g257_bin", "n257_g13_k3", "n257_g261_k5_nob", "n257_g3_bin_nob"])
def test_saturated_logits_stay_finite_and_inside_the_bound(name):
  from sisua_amd import engine
  c = shape_case(name)
  x, y, K = c["x"], c["y"], c["K"]
  W, b = c["at"]["random"]
  z = x.astype(np.float64) @ W.T
  W = W * (800.0 / min(z.max(), -z.min()))   # the nearer tail at 800, the other beyond it
  z = x.astype(np.float64) @ W.T
  assert z.max() >= 799 and z.min() <= -799
  got = engine.k_logreg_eval(x, y, K, W, b, 1.0, c["icpt"])
  hold(got, R.evaluate(x, y, K, W, b, 1.0, c["icpt"]), f"{name} saturated")


@functools.lru_cache(maxsize=None)
def fit_case(name):
  from sklearn.linear_model import LogisticRegression as Sk
  X, y, K = R.case(name)
  X64 = X.astype(np.float64)
  sk = [Sk(C=1.0, tol=1e-10, max_iter=20000, solver=s).fit(X64, y).coef_ for s in ("lbfgs", "newton-cg")]
  return X, y, K, float(np.abs(sk[0] - sk[1]).max()), R.fit(X, y, K, tol=TOL, max_iter=20000)


@pytest.mark.parametrize("name", FIT_CASES)
def test_fit_reaches_the_restatements_optimum(name):
  from sisua_amd import engine
  X, y, K, dis, ref = fit_case(name)
  got = engine.k_logreg_fit(X, y, K, tol=TOL, max_iter=20000)
  F, gW, gb = R.objective(X.astype(np.float64), y, K, got["W"], got["b"])
  gmax = max(np.abs(gW).max(), np.abs(gb).max())
  d = float(np.abs(got["W"] - ref["W"]).max())
  print(f"{name}: iterations {got['n_iter']} (restatement {ref['n_iter']})  evaluations {got['n_eval']}  max|g| {got['gmax']:.3e} "
        f"(recomputed {gmax:.3e})  distance {d:.3e} = {d / dis:.3f} DIS")
  assert got["converged"] and got["gmax"] <= TOL and gmax <= TOL
  assert got["n_iter"] >= 1 and got["n_eval"] > got["n_iter"]
  assert d <= 4.0 * dis
  e = R.evaluate(X, y, K, got["W"], got["b"])
  assert abs(got["F"] - e["F"]) <= e["bF"]
  # the same bits: a second call, and CSR input
  for x2 in (X, sp.csr_matrix(X)):
    again = engine.k_logreg_fit(x2, y, K, tol=TOL, max_iter=20000)
    assert again["W"].tobytes() == got["W"].tobytes() and again["b"].tobytes() == got["b"].tobytes()
    assert (again["n_iter"], again["n_eval"], again["F"], again["gmax"]) == (got["n_iter"], got["n_eval"], got["F"], got["gmax"])
  # a warm start at the solution has nothing left to do
  warm = engine.k_logreg_fit(X, y, K, tol=TOL, max_iter=20000, W0=got["W"], b0=got["b"])
  assert warm["converged"] and warm["n_iter"] == 0 and warm["n_eval"] == 1 and warm["W"].tobytes() == got["W"].tobytes()


def test_separable_data_converges_to_finite_coefficients():
  from sisua_amd import engine
  rng = np.random.RandomState(3)
  y = (np.arange(90) % 3).astype(np.int32)
  X = (rng.uniform(0.0, 1.0, (90, 7)) + 5.0 * np.eye(3)[y] @ np.eye(3, 7)).astype(np.float32)   # class k alone is large in column k
  for K, yy in ((3, y), (2, (y > 0).astype(np.int32))):
    got = engine.k_logreg_fit(X, yy, K, tol=1e-8, max_iter=5000)
    ref = R.fit(X, yy, K, tol=1e-8, max_iter=5000)
    z = X.astype(np.float64) @ got["W"].T + got["b"]
    pred = (z[:, 0] > 0).astype(int) if K == 2 else z.argmax(1)
    assert np.array_equal(pred, yy)   # separable: every row on its side
    assert got["converged"] and ref["converged"] and np.isfinite(got["W"]).all() and np.isfinite(got["b"]).all()
    # both stand within ||g|| / mu <= sqrt(P) tol C N of the optimum (P parameters, the curvature in W at least mu = 1 / (C N))
    assert np.abs(got["W"] - ref["W"]).max() <= 2.0 * np.sqrt(got["W"].size + got["b"].size) * 1e-8 * len(yy)


def test_three_iterations_return_unconverged_and_the_class_warns():
  import sisua_amd
  from sisua_amd import engine
  X, y, K = R.case("k4")
  got = engine.k_logreg_fit(X, y, K, tol=1e-8, max_iter=3)
  assert not got["converged"] and got["n_iter"] == 3 and got["n_eval"] >= 4 and got["gmax"] > 1e-8 and np.isfinite(got["F"])
  m = sisua_amd.LogisticRegression(tol=1e-8, max_iter=3)
  with pytest.warns(RuntimeWarning, match=r"max\|g\| = "):
    m.fit(X, y)
  assert m.n_iter_[0] == 3 and m.coef_.tobytes() == got["W"].tobytes()
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    full = sisua_amd.LogisticRegression(tol=1e-6, max_iter=5000).fit(sp.csr_matrix(X), np.array(list("abcd"))[y])
  assert list(full.classes_) == list("abcd") and full.score(X, np.array(list("abcd"))[y]) > 0.5
  p = full.predict_proba(X)
  assert p.shape == (len(y), 4) and np.allclose(p.sum(1), 1.0)


@pytest.mark.parametrize("name", ["n257_g261_k5_nob", "n257_g3_bin_nob", "n65_g261_k9"])
def test_decision_is_the_logits_at_any_block_rows(name):
  from sisua_amd import engine
  c = shape_case(name)
  W, b = c["at"]["random"]
  z = engine.k_logreg_decision(c["x"], W, b, c["K"])
  want = R.k_logreg_decision(c["x"], W, b, c["K"])
  assert z.shape == want.shape and z.dtype == np.float64
  n_z = 4 * -(-((c["x"].shape[1] + 3) // 4 * 4) // 256) + 7 + c["x"].shape[1]   # the device's chain and NumPy's
  bound = n_z * R.EPS * (np.abs(c["x"].astype(np.float64)) @ np.abs(W).T + np.abs(b))
  assert (np.abs(z - want) <= (bound[:, 0] if z.ndim == 1 else bound)).all()
  for block_rows, x in ((64, c["x"]), (128, c["x"]), (64, sp.csr_matrix(c["x"])), (0, sp.csr_matrix(c["x"]))):
    assert engine.k_logreg_decision(x, W, b, c["K"], block_rows=block_rows).tobytes() == z.tobytes()


def test_neighbors_louvain_logreg_end_to_end():
  from sisua_amd.data import SingleCellOMIC
  from tests import louvain_ref
  x, planted = louvain_ref.blob_cells("clean")
  x = x - x.min()
  sco = SingleCellOMIC(x, var_names=[f"g{i}" for i in range(x.shape[1])])
  sco.neighbors()
  sco.louvain()
  key = sco.rank_vars_groups(n_vars=4, group_by="transcriptomic_louvain", method="logreg")
  res = sco.get_rank_vars_groups(key)
  assert key == "transcriptomic_transcriptomic_louvain_rank" and set(res) == {"params", "names", "scores"}
  assert sorted(res["names"].dtype.names) == [str(c) for c in range(6)] and res["names"].shape == (4,)
  assert res["params"]["max_grad"] <= 1e-4 and all((np.diff(res["scores"][f]) <= 0).all() for f in res["scores"].dtype.names)
  import sisua_amd
  want = sisua_amd.rank_genes_groups_logreg(sp.csr_matrix(x), sco._obs["transcriptomic_louvain"][2], n_genes=4,
                                            var_names=np.asarray(sco.get_var_names("transcriptomic")))
  for f in res["names"].dtype.names:   # the container hands the omic, the kept ids and the names through: the same bits, CSR or dense
    assert list(res["names"][f]) == list(want["names"][f]) and res["scores"][f].tobytes() == want["scores"][f].tobytes()
