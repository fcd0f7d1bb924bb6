"""Logistic regression without a device: the restatement (tests/logreg_ref.py) is held to scikit-learn's converged solvers, and
`LogisticRegression`, `rank_genes_groups_logreg` and `SingleCellOMIC.rank_vars_groups(method='logreg')` run with the three engine entries
replaced by the restatement -- the layout of the result, group subsets, a reference group, two classes, the cache and every refusal.

The yardstick of the coefficients is scikit-learn's own disagreement: `lbfgs` and `newton-cg`, both at tol=1e-10 and max_iter=20000 on the
float64 copy, differ by DIS (max-abs over coef_, measured per case: 4e-7 .. 2e-6 on these shapes, coefficients of size about 1); the
restatement at tol=1e-9 may stand at most 4 DIS from each (the factor allows for both erring on the same side of the optimum)."""
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.linear_model import LogisticRegression as SkLogisticRegression

import sisua_amd
from sisua_amd import _hip, build, engine
from sisua_amd.data import SingleCellOMIC
from tests import logreg_ref as R

ROOT = build.os.path.dirname(build.HERE)
TOL = 1e-9


def sk_pair(X, y, C=1.0):
  X64 = np.asarray(X, np.float64)
  return {s: SkLogisticRegression(C=C, tol=1e-10, max_iter=20000, solver=s).fit(X64, y) for s in ("lbfgs", "newton-cg")}


def disagreement(sk):
  return float(np.abs(sk["lbfgs"].coef_ - sk["newton-cg"].coef_).max())


@pytest.fixture(scope="module")
def solved():
  """name -> (X, y, K, scikit-learn's two fits, the restatement's fit); computed once"""
  out = {}
  for name in R.CASES:
    X, y, K = R.case(name)
    out[name] = (X, y, K, sk_pair(X, y), R.fit(X, y, K, tol=TOL, max_iter=20000))
  return out


@pytest.fixture
def no_device(monkeypatch):
  """a refusal must never reach the library"""
  def boom(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", boom)


@pytest.fixture
def ref_driver(monkeypatch, no_device):
  """engine.k_logreg_* replaced by the restatement; keeps the arguments of every fit"""
  fits = []

  def fit(x, labels, n_classes, C_=1.0, fit_intercept=True, tol=1e-4, max_iter=100, W0=None, b0=None):
    fits.append(dict(shape=x.shape, sparse=sp.issparse(x), K=int(n_classes), C=C_, tol=tol, max_iter=max_iter, warm=W0 is not None))
    return R.k_logreg_fit(x, labels, n_classes, C_, fit_intercept, tol, max_iter, W0, b0)

  monkeypatch.setattr(engine, "k_logreg_fit", fit)
  monkeypatch.setattr(engine, "k_logreg_eval", R.k_logreg_eval)
  monkeypatch.setattr(engine, "k_logreg_decision", R.k_logreg_decision)
  return fits


# ---- the restatement is scikit-learn's optimum ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_is_scikit_learn(solved, name):
  X, y, K, sk, r = solved[name]
  Kz = 1 if K == 2 else K
  assert r["converged"] and r["W"].shape == sk["lbfgs"].coef_.shape == (Kz, X.shape[1])   # (two classes: scikit-learn's ONE row)
  dis = disagreement(sk)
  X64 = X.astype(np.float64)
  F, gW, gb = R.objective(X64, y, K, r["W"], r["b"])
  gmax = max(np.abs(gW).max(), np.abs(gb).max())
  print(f"{name}: DIS {dis:.3e}  gmax {gmax:.3e}  F {F:.15f}  iterations {r['n_iter']}  evaluations {r['n_eval']}")
  assert gmax <= TOL
  n_par = r["W"].size + r["b"].size
  assert n_par * TOL ** 2 * len(y) / 2.0 <= 1e-12 * F, "the input is too separable for the stopping rule to settle F to 1e-12"
  for s, m in sk.items():
    d = float(np.abs(r["W"] - m.coef_).max())
    F_sk = R.objective(X64, y, K, m.coef_, m.intercept_)[0]
    print(f"  {s}: distance {d:.3e} ({d / dis:.2f} DIS)  F_sk - F {F_sk - F:.3e}")
    assert d <= 4.0 * dis, (name, s, d, dis)
    assert np.abs(r["b"] - m.intercept_).max() <= 4.0 * max(dis, float(np.abs(sk["lbfgs"].intercept_ - sk["newton-cg"].intercept_).max()))
    assert F <= F_sk + 1e-12 * abs(F_sk), (name, s)


def test_two_classes_are_the_binary_fit_not_the_softmax(solved):
  X, y, K, sk, r = solved["binary"]
  X64 = X.astype(np.float64)
  # the two-class softmax with rows (-w / 2, w / 2) has the same loss and half the penalty: its optimum is another one
  F_bin = R.objective(X64, y, 2, r["W"], r["b"])[0]
  Wsm, bsm = np.concatenate([-r["W"], r["W"]]) / 2.0, np.concatenate([-r["b"], r["b"]]) / 2.0
  Z = X64 @ Wsm.T + bsm
  loss = (np.log(np.exp(Z - Z.max(1, keepdims=True)).sum(1)) + Z.max(1) - Z[np.arange(len(y)), y]).mean()
  pen_bin = (r["W"] ** 2).sum() / (2 * len(y))
  assert abs(loss + pen_bin - F_bin) < 1e-12 and abs((Wsm ** 2).sum() / (2 * len(y)) - pen_bin / 2) < 1e-15
  assert pen_bin > 1e-4 * F_bin   # (the penalty is not negligible, so half of it moves the optimum)
  assert np.abs(r["W"] - sk["lbfgs"].coef_).max() <= 4.0 * disagreement(sk)


def test_evaluate_is_the_float64_objective_and_its_bounds_are_small(solved):
  for name, (X, y, K, sk, r) in solved.items():
    rng = np.random.RandomState(3)
    W, b = rng.normal(0, 0.3, r["W"].shape), rng.normal(0, 0.3, r["b"].shape)
    e = R.evaluate(X, y, K, W, b, 0.7)
    F, gW, gb = R.objective(X.astype(np.float64), y, K, W, b, 0.7)
    assert abs(F - e["F"]) <= e["bF"] and (np.abs(gW - e["gW"]) <= e["bgW"]).all() and (np.abs(gb - e["gb"]) <= e["bgb"]).all()
    assert e["bF"] < 1e-12 and e["bgW"].max() < 1e-12 and e["bgb"].max() < 1e-12
    # the gradient is the objective's: central differences along a random direction
    dW, db = rng.normal(size=W.shape), rng.normal(size=b.shape)
    h = 1e-6
    num = (R.objective(X.astype(np.float64), y, K, W + h * dW, b + h * db, 0.7)[0] -
           R.objective(X.astype(np.float64), y, K, W - h * dW, b - h * db, 0.7)[0]) / (2 * h)
    assert abs(num - ((gW * dW).sum() + (gb * db).sum())) < 1e-7


# ---- the class ------------------------------------------------------------------------------------------------------------------------
def test_class_surface(ref_driver, solved):
  X, y, K, sk, r = solved["k4"]
  names = np.array(["b", "a", "d", "c"])[y]   # string labels: classes_ are sorted
  m = sisua_amd.LogisticRegression(tol=TOL, max_iter=20000).fit(X, names)
  assert list(m.classes_) == ["a", "b", "c", "d"] and m.coef_.shape == (4, X.shape[1]) and m.intercept_.shape == (4,)
  assert m.n_iter_.shape == (1,) and m.n_iter_[0] >= 1
  perm = [1, 0, 3, 2]   # class 'a' is code 1, ...
  assert np.abs(m.coef_ - r["W"][perm]).max() <= 4.0 * disagreement(sk)
  skm = sk["lbfgs"]
  z = m.decision_function(X)
  assert z.shape == (len(y), 4) and np.abs(z - skm.decision_function(X.astype(np.float64))[:, perm]).max() < 1e-4
  p = m.predict_proba(X)
  assert np.allclose(p.sum(1), 1.0) and np.allclose(np.log(p), m.predict_log_proba(X))
  assert np.array_equal(m.predict(X), np.array(["b", "a", "d", "c"])[skm.predict(X.astype(np.float64))])
  assert m.score(X, names) == skm.score(X.astype(np.float64), y)
  # CSR input is the dense input; two classes: one row, a 1-D decision
  Xb, yb, _, skb, rb = solved["binary"]
  mb = sisua_amd.LogisticRegression(tol=TOL, max_iter=20000).fit(sp.csr_matrix(Xb), yb)
  assert ref_driver[-1]["sparse"] and mb.coef_.shape == (1, Xb.shape[1]) and np.array_equal(mb.coef_, rb["W"])
  zb = mb.decision_function(sp.csr_matrix(Xb))
  assert zb.shape == (len(yb),) and np.array_equal(mb.predict(Xb), skb["lbfgs"].predict(Xb.astype(np.float64)))
  assert mb.predict_proba(Xb).shape == (len(yb), 2) and np.allclose(mb.predict_proba(Xb)[:, 1], 1 / (1 + np.exp(-zb)))


def test_unconverged_warns_and_warm_start_continues(ref_driver, solved):
  X, y, K, _, r = solved["k3"]
  m = sisua_amd.LogisticRegression(max_iter=3, tol=1e-8, warm_start=True)
  with pytest.warns(RuntimeWarning, match=r"max\|g\| = "):
    m.fit(X, y)
  assert m.n_iter_[0] == 3 and not ref_driver[-1]["warm"] and m.max_grad_ > 1e-8
  first = m.objective_
  with pytest.warns(RuntimeWarning):
    m.fit(X, y)
  assert ref_driver[-1]["warm"] and m.objective_ < first
  m.max_iter = 20000
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    m.fit(X, y)
  assert m.max_grad_ <= 1e-8 and np.abs(m.coef_ - r["W"]).max() < 1e-5


# ---- the ranking ----------------------------------------------------------------------------------------------------------------------
def hold_ranking(out, X, y, classes, shown, n_genes, var_names=None, rankby_abs=False):
  """names and scores against scikit-learn on the cells of `classes`; the inputs must separate the compared scores"""
  rows = np.flatnonzero(np.isin(y, classes))
  sk = sk_pair(X[rows], y[rows])
  tol = 4.0 * disagreement(sk)
  assert list(out["names"].dtype.names) == [str(c) for c in shown] == list(out["scores"].dtype.names)
  assert set(out) == {"params", "names", "scores"} and out["scores"].dtype[0] == np.float64
  for i, c in enumerate(shown):
    orders = []
    for m in sk.values():
      assert list(m.classes_) == sorted(classes)
      s = np.abs(m.coef_[i]) if rankby_abs else m.coef_[i]
      order = np.argsort(-s, kind="stable")
      assert (-np.diff(s[order][:n_genes + 1]) > 2.0 * tol).all(), "the input does not separate the compared scores"
      orders.append(order[:n_genes])
    assert np.array_equal(orders[0], orders[1])
    want = orders[0].astype(str) if var_names is None else np.asarray(var_names)[orders[0]]
    assert list(out["names"][str(c)]) == list(want)
    assert np.abs(out["scores"][str(c)] - sk["lbfgs"].coef_[i][orders[0]]).max() <= tol


def ranking_input():
  X, y = R.make_case(320, 24, 4, seed=11)
  return X, y


def test_ranking_is_scikit_learns_coefficient_order(ref_driver):
  X, y = ranking_input()
  kw = dict(tol=TOL, max_iter=20000, n_genes=8)
  out = sisua_amd.rank_genes_groups_logreg(X, y, **kw)
  hold_ranking(out, X, y, [0, 1, 2, 3], [0, 1, 2, 3], 8)
  assert out["params"]["method"] == "logreg" and out["params"]["reference"] == "rest" and out["names"].shape == (8,)
  # CSR input is the dense input, bit for bit
  out_s = sisua_amd.rank_genes_groups_logreg(sp.csr_matrix(X), y, **kw)
  assert ref_driver[-1]["sparse"] and np.array_equal(out_s["names"], out["names"]) and np.array_equal(out_s["scores"], out["scores"])
  # a subset of the groups: only their cells are fitted
  out = sisua_amd.rank_genes_groups_logreg(X, y, groups=[3, 0, 1], **kw)
  assert ref_driver[-1]["shape"][0] == int(np.isin(y, [0, 1, 3]).sum()) and ref_driver[-1]["K"] == 3
  hold_ranking(out, X, y, [0, 1, 3], [0, 1, 3], 8)
  # a reference group joins the classes and gets a column like any other
  out = sisua_amd.rank_genes_groups_logreg(X, y, groups=[1, 3], reference=2, **kw)
  hold_ranking(out, X, y, [1, 2, 3], [1, 2, 3], 8)
  assert out["params"]["reference"] == 2
  # two classes: scikit-learn's single coefficient vector, once, under the first class
  out = sisua_amd.rank_genes_groups_logreg(X, y, groups=[2], reference=0, **kw)
  assert ref_driver[-1]["K"] == 2
  hold_ranking(out, X, y, [0, 2], [0], 8)
  out = sisua_amd.rank_genes_groups_logreg(X, y, groups=[2], reference=0, rankby_abs=True, **kw)
  hold_ranking(out, X, y, [0, 2], [0], 8, rankby_abs=True)
  # string labels and variable names
  lab = np.array(["t", "b", "nk", "mono"])[y]
  var = np.array([f"g{i}" for i in range(X.shape[1])])
  out = sisua_amd.rank_genes_groups_logreg(X, lab, var_names=var, **kw)
  rows_of = {"b": 1, "mono": 3, "nk": 2, "t": 0}
  full = sisua_amd.rank_genes_groups_logreg(X, y, **kw)
  assert out["names"].dtype.names == ("b", "mono", "nk", "t")
  for name, code in rows_of.items():
    assert list(out["names"][name]) == [f"g{i}" for i in full["names"][str(code)]]
  # equal scores go to the lowest gene index
  Xd = np.concatenate([X[:, :5], X[:, :5]], axis=1)
  out = sisua_amd.rank_genes_groups_logreg(Xd, y, n_genes=10, tol=TOL, max_iter=20000)
  for f in out["names"].dtype.names:
    pos = {int(n): i for i, n in enumerate(out["names"][f])}
    sc = dict(zip(out["names"][f].astype(int), out["scores"][f]))
    for j in range(5):
      if abs(sc[j] - sc[j + 5]) == 0.0:
        assert pos[j] < pos[j + 5]


def same(a, b):
  return a["names"].dtype.names == b["names"].dtype.names and all(
      list(a["names"][f]) == list(b["names"][f]) and np.array_equal(a["scores"][f], b["scores"][f]) for f in a["names"].dtype.names)


# ---- the container ------------------------------------------------------------------------------------------------------------------------
def test_rank_vars_groups_logreg_keeps_and_drops(ref_driver, monkeypatch):
  from tests import minibatch_kmeans_ref as MR
  X, y = ranking_input()
  var = [f"g{i}" for i in range(X.shape[1])]
  onehot = np.eye(4, dtype=np.float32)[y]   # (a 0 / 1 omic is its own probability embedding: no mixture is fitted)
  sco = SingleCellOMIC(X, var_names=var)
  sco.add_omic("proteomic", onehot, var_names=["CD3", "CD4", "CD8", "CD19"])
  with pytest.raises(NotImplementedError, match="wilcoxon"):
    sco.rank_vars_groups()                        # the reference's defaults: the clustering='kmeans' refusal, before any fit
  assert not ref_driver
  # a label array; max_iter reaches the solver
  with pytest.warns(RuntimeWarning):
    key = sco.rank_vars_groups(n_vars=5, group_by=y, method="logreg", max_iter=3)
  assert key == "transcriptomic_labels_rank" and ref_driver[-1]["max_iter"] == 3 and len(ref_driver) == 1
  res = sco.get_rank_vars_groups(key)
  assert set(res) == {"params", "names", "scores"} and res["names"].dtype.names == ("0", "1", "2", "3") and res["names"].shape == (5,)
  assert sco.rank_vars_groups(group_by=y, method="logreg") == key and len(ref_driver) == 1   # kept
  # an omic's name with clustering=None: the labels are the variable names at the argmax
  key2 = sco.rank_vars_groups(n_vars=6, group_by="proteomic", clustering=None, method="logreg", corr_method="whatever")
  assert key2 == "transcriptomic_proteomic_rank" and ref_driver[-1]["max_iter"] == 1000
  res2 = sco.get_rank_vars_groups(key2)
  want = sisua_amd.rank_genes_groups_logreg(X, np.array(["CD3", "CD4", "CD8", "CD19"])[y], n_genes=6, var_names=np.array(var))
  assert res2["names"].dtype.names == ("CD19", "CD3", "CD4", "CD8")
  assert same(res2, want)
  # a clustering key
  monkeypatch.setattr(engine, "k_mbkmeans_seed", MR.k_seed)
  monkeypatch.setattr(engine, "k_mbkmeans_step", MR.k_step)
  monkeypatch.setattr(engine, "k_mbkmeans_predict", MR.k_predict)
  ckey = sco.clustering(n_clusters=3, return_key=True)
  key3 = sco.rank_vars_groups(n_vars=4, group_by=ckey, method="logreg")
  assert key3 == f"transcriptomic_{ckey}_rank" and ref_driver[-1]["K"] == 3
  want = sisua_amd.rank_genes_groups_logreg(X, sco.clustering(n_clusters=3), n_genes=4, var_names=np.array(var))
  assert same(sco.get_rank_vars_groups(key3), want)
  # dropped with the omic they were made from
  sco._replace("proteomic", onehot[:, ::-1].copy())
  assert key2 not in sco._uns and key in sco._uns
  sco._replace("transcriptomic", X * 2)
  assert key not in sco._uns and key3 not in sco._uns


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_never_ask_for_the_device(no_device):
  X, y = R.make_case(60, 5, 3, seed=5)
  L = sisua_amd.LogisticRegression
  for kw in (dict(penalty="l1"), dict(penalty="elasticnet"), dict(penalty=None), dict(class_weight="balanced"), dict(class_weight={0: 2.0}),
             dict(solver="saga"), dict(solver="liblinear"), dict(solver="newton-cg"), dict(l1_ratio=0.5), dict(dual=True),
             dict(multi_class="ovr"), dict(C=0.0), dict(C=-1.0), dict(C=np.inf), dict(tol=0.0), dict(tol=np.nan), dict(max_iter=0)):
    with pytest.raises(ValueError):
      L(**kw)
  with pytest.raises(ValueError, match="penalty='l2'"):
    L(penalty="l1")
  L(solver="lbfgs"), L(solver=None)
  with pytest.raises(ValueError, match="sample_weight"):
    L().fit(X, y, sample_weight=np.ones(len(y)))
  with pytest.raises(ValueError, match="2 classes"):
    L().fit(X, np.zeros(len(y), int))                       # one class
  with pytest.raises(ValueError):
    L().fit(X, y[:-1])
  with pytest.raises(ValueError, match="not fitted"):
    L().predict(X)
  bad = X.copy()
  bad[7, 2] = np.inf
  for x in (bad, sp.csr_matrix(bad)):
    with pytest.raises(ValueError, match="not finite"):
      L().fit(x, y)
    with pytest.raises(ValueError, match="not finite"):
      sisua_amd.rank_genes_groups_logreg(x, y)
  # the engine's own checks: an empty class, labels out of range, C, tol, max_iter, the parameters' shape, the limits
  W, b = np.zeros((3, 5)), np.zeros(3)
  with pytest.raises(ValueError, match="no row"):
    engine.k_logreg_fit(X, np.where(y == 1, 0, y), 3)
  for kw in (dict(C_=0.0), dict(C_=-2.0), dict(C_=np.nan), dict(tol=0.0), dict(tol=np.nan), dict(max_iter=0), dict(W0=W), dict(W0=W[:2], b0=b)):
    with pytest.raises(ValueError):
      engine.k_logreg_fit(X, y, 3, **kw)
  for args in ((X, y + 1, 3, W, b), (X, y, 3, W[:2], b), (X, y, 3, W, b[:2]), (X, y.astype(np.float64), 3, W, b), (X, y[:-1], 3, W, b),
               (X, y, 1, W, b), (X, y, 257, W, b), (X, y, 3, W * np.nan, b)):
    with pytest.raises(ValueError):
      engine.k_logreg_eval(*args)
  with pytest.raises(ValueError):
    engine.k_logreg_decision(X, W[:2], b, 3)
  wide = sp.csr_matrix((4, engine.LR_MAX_GENES + 1), dtype=np.float32)
  with pytest.raises(ValueError, match="columns"):
    engine.k_logreg_fit(wide, np.array([0, 1, 0, 1]), 2)
  tall = sp.csr_matrix((2 ** 17, 2 ** 14 + 4), dtype=np.float32)   # (2^31 + 2^19 entries in the tile)
  with pytest.raises(ValueError, match="held on the device"):
    engine.k_logreg_fit(tall, np.arange(2 ** 17) % 2, 2)
  # the ranking's own: unknown groups, one class, names
  for kw in (dict(groups=[7]), dict(reference=9), dict(n_genes=0), dict(var_names=["a"]), dict(groups=[1], reference=1)):
    with pytest.raises(ValueError):
      sisua_amd.rank_genes_groups_logreg(X, y, **kw)
  with pytest.raises(ValueError, match="at least 2 classes"):
    sisua_amd.rank_genes_groups_logreg(X, np.zeros(len(y), int))
  with pytest.raises(ValueError, match="at least 2 classes"):
    sisua_amd.rank_genes_groups_logreg(X, y, groups=[2])
  # the module-level method='logreg' stays refused, with a pointer to the new function
  with pytest.raises(NotImplementedError, match="t-test.*t-test_overestim_var.*wilcoxon.*rank_genes_groups_logreg"):
    sisua_amd.rank_genes_groups(X, y, method="logreg")


def test_header_binding_and_version_agree():
  hdr = open(build.os.path.join(ROOT, "include", "sisua_hip.h")).read()
  assert int(re.search(r"#define SMX_ABI_VERSION (\d+)", hdr).group(1)) == _hip.SMX_ABI_VERSION >= 18
  assert "smx_logreg.hip" in build.SOURCES
  for name, n_args in (("smx_logreg_eval", 16), ("smx_logreg_fit", 22), ("smx_logreg_decision", 12)):
    proto = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
    assert len(proto.split(",")) == n_args == len(_hip.SIGNATURES[name][1])
  for name in ("LogisticRegression", "rank_genes_groups_logreg"):
    assert name in dir(sisua_amd)
  driver = open(build.os.path.join(ROOT, "tools", "asan", "host_driver.cpp")).read()
  assert all(f"smx_logreg_{e}(" in driver for e in ("eval", "fit", "decision"))
