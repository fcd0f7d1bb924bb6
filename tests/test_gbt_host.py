"""Gradient-boosted trees without a device: the restatement (tests/gbt_ref.py) is held to scikit-learn's GradientBoostingClassifier, and the
binning rule, the stopping and holdout rules, `dci_scores`, the quantile discretiser, `marker_scores('importance')`, every refusal and the
header / binding / build agreement are pinned.  `GradientBoostingClassifier`, `importance_matrix` and
`SingleCellOMIC.get_importance_matrix` run here with the two engine entries replaced by the restatement.

Tie-free data.  On continuous float32 columns with at most 256 distinct values the restatement's candidate partitions are scikit-learn's,
so every node of every tree must have scikit-learn's feature and n, and scikit-learn's float32 threshold must be the midpoint of the two
values of the NODE's own cells that the restatement's cut separates (scikit-learn takes the neighbours among the node's cells; the
restatement's own threshold is the midpoint of the neighbours in the whole column, which cuts the node's cells identically -- asserted
too).  A cut that isolates a single cell ties exactly with its mirror image in every other feature (the same two sums change sides), and
scikit-learn breaks such ties by its seeded feature order: with single-cell leaves allowed, ten stages of K = 3 trees agree node for node
at none of 6 000 scanned data seeds (each of the 30 trees has to win its tied draws), ten stages of K = 2 at 3 of 400.  So K = 2 runs at the
default min_samples_leaf = 1 and K = 3 at min_samples_leaf = 2, which the issue leaves open and which takes exactly those ties away; the
data seeds are recorded below, found by a scan; both sides run on the host.  What remains is the 2^-40 quantum accumulated over the
stages.  Measured here (K = 2 / K = 3): leaf values 5.8e-12 / 3.1e-11 relative, decision_function 5.5e-13 / 4.7e-13 absolute,
feature_importances_ 4.4e-14 / 2.6e-14, train_score_ 6.2e-14 / 1.5e-14; the tolerances below are ten times the larger figure.

Count data with ties.  scikit-learn's own answer moves with its random_state (its tie-breaking is seeded); the restatement must stand
within twice scikit-learn's spread over ten seeds of the seed-mean."""
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.ensemble import GradientBoostingClassifier as SkGradientBoosting

import sisua_amd
from sisua_amd import _hip, boosting, build, engine, metrics
from sisua_amd.data import SingleCellOMIC
from tests import gbt_ref as R

ROOT = build.os.path.dirname(build.HERE)
# (K, min_samples_leaf, data seed): seeds at which every tree agrees with scikit-learn (random_state=0), found by a scan
TIE_FREE_CASES = [(2, 1, 163), (3, 2, 165)]
VALUE_RTOL, DECISION_ATOL, IMPORTANCE_ATOL, SCORE_ATOL = 3.1e-10, 5.5e-12, 4.4e-13, 6.2e-13


@pytest.fixture
def no_device(monkeypatch):
  """a refusal must never reach the library"""
  def boom(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", boom)


@pytest.fixture
def ref_driver(monkeypatch, no_device):
  """engine.k_gbt_fit / k_gbt_decision replaced by the restatement; keeps the arguments of every fit"""
  fits = []

  def fit(x, labels, n_classes, n_estimators=100, learning_rate=0.1, max_depth=3, min_samples_split=2, min_samples_leaf=1, x_val=None,
          labels_val=None, n_iter_no_change=None, tol=1e-4, pass_pairs=0):
    fits.append(dict(shape=x.shape, sparse=sp.issparse(x), K=int(n_classes), n_estimators=n_estimators, patience=n_iter_no_change,
                     n_val=None if x_val is None else x_val.shape[0]))
    r = R.fit(x, labels, int(n_classes), n_estimators, learning_rate, max_depth, min_samples_split, min_samples_leaf, x_val, labels_val,
              n_iter_no_change, tol)
    r["max_depth"] = max_depth
    return r

  def decision(x, trees, init, learning_rate, block_rows=0, n_stages=None):
    return R.decision(trees, init, learning_rate, x, n_stages)

  monkeypatch.setattr(engine, "k_gbt_fit", fit)
  monkeypatch.setattr(engine, "k_gbt_decision", decision)
  return fits


# ---- 1. the restatement against scikit-learn on tie-free data ------------------------------------------------------------------------------
@pytest.mark.parametrize("K, msl, seed", TIE_FREE_CASES)
def test_restatement_has_scikit_learns_trees_on_tie_free_data(K, msl, seed):
  N, G, S = 200, 6, 10
  rng = np.random.RandomState(seed)
  X = rng.normal(size=(N, G)).astype(np.float32)
  y = rng.randint(0, K, size=N)
  assert all(len(np.unique(X[:, j])) <= 256 for j in range(G))
  sk = SkGradientBoosting(n_estimators=S, max_depth=3, min_samples_leaf=msl, random_state=0).fit(X, y)
  T = R.fit(X, y, K, n_estimators=S, min_samples_leaf=msl)
  Kz = 1 if K == 2 else K
  worst = 0.0
  for s in range(S):
    for k in range(Kz):          # every tree, none left out
      t = sk.estimators_[s, k].tree_
      stack, seen = [(0, 0, np.arange(N))], 0
      while stack:
        a, b, rows = stack.pop()
        seen += 1
        where = (s, k, a, b)
        assert t.n_node_samples[a] == T["n"][s, k, b] == len(rows), where
        if t.children_left[a] < 0:
          assert T["feature"][s, k, b] == -1, where
          worst = max(worst, abs(t.value[a, 0, 0] - T["value"][s, k, b]) / abs(t.value[a, 0, 0]))
          continue
        f, thr = T["feature"][s, k, b], T["threshold"][s, k, b]
        assert f == t.feature[a], where
        x = X[rows, f]
        lo, hi = x[x <= thr].max(), x[x > thr].min()                      # the node's own neighbours of the restatement's cut
        assert np.float32(t.threshold[a]) == np.float32(np.float64(lo) / 2.0 + np.float64(hi) / 2.0), where
        assert lo <= thr < hi, where
        stack.append((t.children_left[a], 2 * b + 1, rows[x <= thr]))
        stack.append((t.children_right[a], 2 * b + 2, rows[x > thr]))
      assert seen == t.node_count == (T["n"][s, k] > 0).sum()
  mine = R.decision(T, T["init"], 0.1, X)
  d_dec = np.abs(sk.decision_function(X).reshape(N, Kz) - mine).max()
  d_imp = np.abs(sk.feature_importances_ - R.feature_importances(T, G)).max()
  d_score = np.abs(sk.train_score_ - T["train_score_"]).max()
  print(f"K={K}: leaf values {worst:.2e} relative, decision {d_dec:.2e}, importances {d_imp:.2e}, train_score {d_score:.2e}")
  assert worst < VALUE_RTOL and d_dec < DECISION_ATOL and d_imp < IMPORTANCE_ATOL and d_score < SCORE_ATOL
  assert np.array_equal(mine, T["raw"])   # (the walk by thresholds lands where the bins did)


# ---- 2. the restatement against scikit-learn on count data with ties -----------------------------------------------------------------------
def test_restatement_within_scikit_learns_own_spread_on_counts():
  rng = np.random.RandomState(0)
  X = rng.poisson(3.0, size=(600, 40)).astype(np.float32)
  y = R.make_labels(X, 4, seed=0)
  fits = [SkGradientBoosting(n_estimators=20, max_depth=3, random_state=s).fit(X, y) for s in range(10)]
  imp = np.array([m.feature_importances_ for m in fits])
  spread = max(np.abs(imp[i] - imp[j]).max() for i in range(10) for j in range(i))
  acc = np.mean([m.score(X, y) for m in fits])
  T = R.fit(X, y, 4, n_estimators=20)
  dist = np.abs(R.feature_importances(T, 40) - imp.mean(axis=0)).max()
  mine = np.mean(np.argmax(R.decision(T, T["init"], 0.1, X), axis=1) == y)
  print(f"scikit-learn's spread over ten seeds {spread:.2e}, the restatement's distance to the seed-mean {dist:.2e}; accuracy {mine:.4f} vs {acc:.4f}")
  assert spread > 0                       # (measured here: 3.5e-3; the ties are real)
  assert dist <= 2 * spread               # (measured here: 2.3e-3)
  assert abs(mine - acc) <= 0.01          # one cell per 100 (measured here: 0.7833 vs 0.7800)


# ---- 3. pins -------------------------------------------------------------------------------------------------------------------------------
def test_binning_rule_on_hand_cases():
  for d, want in ((255, 254), (256, 255)):
    v = np.resize(np.arange(d, dtype=np.float32), 3 * d)
    thr, bins = R.bin_column(v)
    assert len(thr) == want and np.array_equal(thr, np.arange(d - 1) + np.float32(0.5)) and np.array_equal(bins, v.astype(np.uint8))
  # 257 distinct values, each twice (N = 514): cuts only at floor(j 514 / 256) where the two neighbours differ
  v = np.repeat(np.arange(257, dtype=np.float32), 2)
  thr, bins = R.bin_column(v)
  ps = (np.arange(1, 256) * 514) // 256
  want = [p for p in ps if v[p - 1] != v[p]]
  assert len(thr) == len(want) < 255 and np.array_equal(thr, [v[p - 1] / 2 + v[p] / 2 for p in want])
  assert np.array_equal(bins, np.searchsorted(thr, v, side="left"))        # bin(x) <= b exactly where x <= thr[b]
  inside = [p for p in ps if v[p - 1] == v[p]]
  assert inside and all(bins[p - 1] == bins[p] for p in inside)           # duplicates that straddle a quantile position stay together
  thr, bins = R.bin_column(np.full(50, 2.5, np.float32))
  assert len(thr) == 0 and not bins.any()                                  # a constant column: one bin, no candidate
  thr, bins = R.bin_column(np.array([0.0, -0.0, 1.0], np.float32))
  assert len(thr) == 1 and list(bins) == [0, 0, 1]                         # -0 is +0
  big = np.float32(3.0e38)
  thr, _ = R.bin_column(np.array([big, np.nextafter(big, np.float32(np.inf))], np.float32))
  assert np.isfinite(thr).all() and thr[0] == big                          # halves first: no overflow; a midpoint that rounds up takes a
  B = R.bin_matrix(sp.csr_matrix(np.array([[0, 1.5], [0, 0], [0, 1.5]], np.float32)))
  assert list(B["n_thr"]) == [0, 1] and B["thr"][1, 0] == np.float32(0.75) and B["thr"].shape == (2, 255)


def test_stopping_rule_is_scikit_learns():
  hist = np.full(3, np.inf)
  losses = [1.0, 0.9, 0.95, 0.93, 0.91, 0.9001, 0.94]
  stops = [R.should_stop(hist, i, v, 1e-4) for i, v in enumerate(losses)]
  # a stage goes on while it beats ANY loss of the ring by tol (0.95 after 0.9 does: its slot still holds +inf); after stage 5 the ring
  # holds 0.93, 0.91, 0.9001, and 0.94 beats none of them
  assert stops == [False, False, False, False, False, False, True]
  hist = np.full(2, np.inf)
  assert [R.should_stop(hist, i, v, 0.0) for i, v in enumerate([1.0, 1.0, 1.0])] == [False, False, True]


def test_holdout_rule():
  y = np.array([0] * 10 + [1] * 3 + [2] * 1 + [3] * 2)
  tr, va = R.holdout(y, 4, 0.25, 7)
  assert np.array_equal(np.sort(np.concatenate([tr, va])), np.arange(16)) and not set(tr) & set(va)
  assert [int((y[va] == c).sum()) for c in range(4)] == [3, 1, 0, 1]   # ceil(0.25 n_c), but one row of every class stays
  rs = np.random.RandomState(7)
  assert set(va[y[va] == 0]) == set(rs.permutation(np.arange(10))[-3:])  # class 0 draws first from the one stream
  tr2, va2 = boosting.holdout_rows(y, 4, 0.25, 7)
  assert np.array_equal(tr, tr2) and np.array_equal(va, va2)
  assert not np.array_equal(va, R.holdout(y, 4, 0.25, 8)[1])


def test_dci_scores_on_hand_matrices():
  d = metrics.dci_scores(np.eye(4), [1.0, 0.5, 0.5, 1.0])
  assert d["disentanglement"] == pytest.approx(1.0, abs=1e-8) and d["completeness"] == pytest.approx(1.0, abs=1e-8)
  assert d["informativeness"] == 0.75 and set(d) == {"disentanglement", "completeness", "informativeness"}
  d = metrics.dci_scores(np.ones((3, 4)))
  assert d["disentanglement"] == pytest.approx(0.0, abs=1e-12) and d["completeness"] == pytest.approx(0.0, abs=1e-12)
  assert np.isnan(d["informativeness"])
  with_zero_row = np.vstack([np.eye(3), np.zeros((1, 3))])      # the zero row is uniform (score 0) and has weight 0
  assert metrics.dci_scores(with_zero_row)["disentanglement"] == pytest.approx(1.0, abs=1e-8)
  m = np.array([[0.9, 0.1], [0.2, 0.8], [0.0, 0.0]])
  from scipy.stats import entropy
  rows = np.array([1 - entropy(r + 1e-11, base=2) for r in m])
  assert metrics.dci_scores(m)["disentanglement"] == pytest.approx(float(rows @ (m.sum(1) / m.sum())), rel=1e-12)
  assert metrics.dci_scores(m)["completeness"] == pytest.approx(np.mean([1 - entropy(c + 1e-11, base=3) for c in m.T]), rel=1e-12)
  for edge in (np.ones((3, 1)), np.zeros((3, 4)), np.zeros((1, 1)), np.ones((1, 3))):
    assert all(np.isfinite(v) for k, v in metrics.dci_scores(edge, np.full(edge.shape[1], 0.5)).items()), edge.shape
  assert metrics.dci_scores(np.zeros((3, 4)))["disentanglement"] == 0.0
  assert metrics.dci_scores(np.ones((3, 1)))["disentanglement"] == 1.0
  assert np.isnan(metrics.dci_scores(np.eye(2), [np.nan, np.nan])["informativeness"])
  assert metrics.dci_scores(np.eye(2), [np.nan, 0.5])["informativeness"] == 0.5
  for bad in (np.ones(3), np.ones((0, 2)), np.array([[np.nan, 1.0]])):
    with pytest.raises(ValueError):
      metrics.dci_scores(bad)
  with pytest.raises(ValueError):
    metrics.dci_scores(np.eye(2), [1.0])
  assert sisua_amd.dci_scores is metrics.dci_scores


def test_quantile_codes_are_kbins_discretizers():
  from sklearn.preprocessing import KBinsDiscretizer
  rng = np.random.RandomState(3)
  cols = [rng.normal(size=301), rng.poisson(1.0, 301).astype(float), np.log1p(rng.poisson(30.0, 301)), np.r_[np.zeros(200), rng.uniform(size=101)]]
  for n_bins in (5, 10):
    for c in cols:
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = KBinsDiscretizer(n_bins=n_bins, encode="ordinal", strategy="quantile", subsample=None).fit_transform(c[:, None])[:, 0]
      assert np.array_equal(boosting.quantile_codes(c, n_bins), want.astype(np.int64))
      assert np.array_equal(R.quantile_codes(c, n_bins), want.astype(np.int64))


def test_marker_scores_importance_is_the_fourth_kind():
  m = np.arange(6.0).reshape(3, 2)
  genes, prots, markers = ["g0", "g1", "g2"], ["p0", "p1"], {"p0": "g2", "p1": "g0", "p9": "g1"}
  assert metrics.marker_scores(m, "importance", genes, prots, markers) == {"importance_g2_p0": 4.0, "importance_g0_p1": 1.0}
  assert metrics.marker_scores(m, "mi", genes, prots, markers) == {"mi_g2_p0": 4.0, "mi_g0_p1": 1.0}
  with pytest.raises(NotImplementedError):
    metrics.marker_scores(m, "lasso", genes, prots, markers)


def test_every_refusal_is_raised_without_a_device(no_device):
  X = R.make_matrix(60, 5, seed=1)
  y = R.make_labels(X, 3, seed=1)
  G = sisua_amd.GradientBoostingClassifier
  for kw in (dict(subsample=0.5), dict(max_features="sqrt"), dict(loss="exponential"), dict(warm_start=True), dict(ccp_alpha=0.1),
             dict(max_leaf_nodes=8), dict(criterion="squared_error"), dict(init="zero"), dict(presort=True)):
    with pytest.raises(ValueError, match="is built for loss='log_loss'"):
      G(**kw)
  for kw in (dict(n_estimators=0), dict(learning_rate=0.0), dict(learning_rate=-1.0), dict(learning_rate=np.inf), dict(learning_rate=np.nan),
             dict(max_depth=0), dict(max_depth=7), dict(min_samples_split=1), dict(min_samples_leaf=0), dict(n_iter_no_change=0),
             dict(validation_fraction=0.0), dict(validation_fraction=1.0), dict(tol=np.nan)):
    with pytest.raises(ValueError):
      G(**kw)
  with pytest.raises(ValueError, match="max_depth must be 1 .. 6"):
    G(max_depth=7)
  with pytest.raises(ValueError, match="learning_rate must be finite and > 0"):
    G(learning_rate=0.0)
  with pytest.raises(ValueError, match="sample_weight"):
    G().fit(X, y, sample_weight=np.ones(len(y)))
  with pytest.raises(ValueError, match="2 classes"):
    G().fit(X, np.zeros(len(y), int))
  with pytest.raises(ValueError):
    G().fit(X, y[:-1])
  with pytest.raises(ValueError, match="not fitted"):
    G().predict(X)
  bad = X.copy()
  bad[7, 2] = np.inf
  for x in (bad, sp.csr_matrix(bad)):
    with pytest.raises(ValueError, match="not finite"):
      G().fit(x, y)
    with pytest.raises(ValueError, match="not finite"):
      engine.k_gbt_bin(x)
  # the engine's own checks: the limits, each named
  with pytest.raises(ValueError, match="N <= 2\\^20"):
    engine.k_gbt_fit(sp.csr_matrix((2 ** 20 + 1, 2), dtype=np.float32), np.arange(2 ** 20 + 1) % 2, 2)
  with pytest.raises(ValueError, match="G <= 32768"):
    engine.k_gbt_fit(sp.csr_matrix((4, 32769), dtype=np.float32), np.array([0, 1, 0, 1]), 2)
  with pytest.raises(ValueError, match="held on the device"):
    engine.k_gbt_fit(sp.csr_matrix((2 ** 17, 2 ** 14 + 4), dtype=np.float32), np.arange(2 ** 17) % 2, 2)
  for K in (1, 33):
    with pytest.raises(ValueError, match="2 .. 32 classes"):
      engine.k_gbt_fit(X, np.zeros(60, int), K)
  with pytest.raises(ValueError, match="2 .. 32 classes"):
    G().fit(np.zeros((40, 2), np.float32), np.arange(40))                 # 40 classes
  with pytest.raises(ValueError, match="has no row"):
    engine.k_gbt_fit(X, np.where(y == 1, 0, y), 3)
  for kw in (dict(max_depth=0), dict(max_depth=7), dict(learning_rate=0.0), dict(learning_rate=np.nan), dict(n_estimators=0),
             dict(min_samples_split=1), dict(min_samples_leaf=0), dict(pass_pairs=17), dict(pass_pairs=-1), dict(n_iter_no_change=3),
             dict(n_iter_no_change=0, x_val=X, labels_val=y), dict(n_iter_no_change=3, x_val=X[:, :4], labels_val=y),
             dict(n_iter_no_change=3, x_val=X, labels_val=y + 1), dict(n_iter_no_change=3, x_val=X, labels_val=y, tol=np.nan)):
    with pytest.raises(ValueError):
      engine.k_gbt_fit(X, y, 3, **kw)
  for labels in (y + 1, y.astype(np.float64), y[:-1]):
    with pytest.raises(ValueError):
      engine.k_gbt_fit(X, labels, 3)
  # grow: the bins, the statistics, the shapes
  B = R.bin_matrix(X)
  q = np.ones((2, 60), np.int64)
  for args, kw in (((B, q[:, :-1], q[:, :-1]), {}), ((B, q, q[:1]), {}), ((B, np.ones((33, 60), np.int64), np.ones((33, 60), np.int64)), {}),
                   ((B, q * 2 ** 42, q), {}), ((B, q, -q), {}), ((B, q, q), dict(max_depth=7)), ((B, q, q), dict(pass_pairs=17)),
                   ((B, q, q), dict(scale=np.nan)), ((dict(B, n_thr=B["n_thr"] - 1), q, q), {}), ((dict(B, thr=B["thr"][:, :-1]), q, q), {})):
    with pytest.raises(ValueError):
      engine.k_gbt_grow(*args, **kw)
  # decision: trees that would leave the matrix or the tree
  T = R.fit(X, y, 3, n_estimators=2)
  trees = {a: T[a] for a in ("feature", "threshold", "left", "right", "value")}
  wide = dict(trees, feature=np.where(trees["feature"] >= 0, 5, -1).astype(np.int32))
  loop = dict(trees, left=np.zeros_like(trees["left"]))
  for t, kw in ((wide, {}), (loop, {}), (trees, dict(n_stages=3)), (dict(trees, value=trees["value"][:1]), {}),
                ({a: v[:, :, :6] for a, v in trees.items()}, {})):
    with pytest.raises(ValueError):
      engine.k_gbt_decision(X, t, T["init"], 0.1, **kw)
  with pytest.raises(ValueError):
    engine.k_gbt_decision(X, trees, T["init"][:2], 0.1)
  with pytest.raises(ValueError):
    engine.k_gbt_decision(X[:, :4], trees, T["init"], 0.1) if (trees["feature"] >= 4).any() else engine.k_gbt_decision(bad, trees, T["init"], 0.1)
  # importance_matrix and dci's shapes
  with pytest.raises(ValueError):
    sisua_amd.importance_matrix(X, y[:, None], X[:10], y[:9, None])
  with pytest.raises(ValueError):
    sisua_amd.importance_matrix(X, y, X, y)


def test_init_raw_is_the_restatements_and_scikit_learns():
  for K, y in ((2, np.array([0, 1, 1, 1, 0, 1])), (4, np.array([0, 1, 2, 3, 3, 3, 1, 0, 0]))):
    assert np.array_equal(engine.gbt_init_raw(y, K), R.init_raw(y, K))
    sk = SkGradientBoosting(n_estimators=1).fit(np.zeros((len(y), 1)), y)
    assert np.allclose(sk.decision_function(np.zeros((1, 1))).reshape(-1) - 0.1 * np.array([e.tree_.value[0, 0, 0] for e in sk.estimators_[0]]),
                       R.init_raw(y, K), rtol=1e-12, atol=1e-14)


def test_class_surface_on_the_restatement(ref_driver):
  X = R.make_matrix(150, 7, seed=2)
  for K, names in ((2, np.array(["a", "b"])), (3, np.array([5, 7, 11]))):
    y = names[R.make_labels(X, K, seed=2)]
    m = sisua_amd.GradientBoostingClassifier(n_estimators=6).fit(sp.csr_matrix(X) if K == 3 else X, y)
    assert list(m.classes_) == list(names) and m.n_classes_ == K and m.n_estimators_ == 6 and m.train_score_.shape == (6,)
    assert m.estimators_.shape == (6, 1 if K == 2 else K) and m.feature_importances_.shape == (7,)
    assert m.feature_importances_.sum() == pytest.approx(1.0) and (m.feature_importances_ >= 0).all()
    t = m.estimators_[0, 0]
    assert t.node_count == (t.n_node_samples > 0).sum() >= 3 and t.n_node_samples[0] == 150
    with pytest.raises((AttributeError, ValueError)):
      t.value[0] = 1.0
    with pytest.raises(AttributeError):
      t.value = None
    z = m.decision_function(X)
    assert z.shape == ((150,) if K == 2 else (150, K))
    p = m.predict_proba(X)
    assert p.shape == (150, K) and np.allclose(p.sum(axis=1), 1.0) and np.array_equal(m.predict(X), names[np.argmax(p, axis=1)])
    assert m.score(X, y) == np.mean(m.predict(X) == y) > 1.0 / K
    staged = list(m.staged_decision_function(X))
    assert len(staged) == 6 and np.array_equal(staged[-1], z) and not np.array_equal(staged[0], z)
    sk = SkGradientBoosting(n_estimators=6, random_state=0).fit(X, y)
    assert np.mean(sk.predict(X) == m.predict(X)) > 0.97 and np.abs(sk.feature_importances_ - m.feature_importances_).max() < 0.05
  assert [f["sparse"] for f in ref_driver] == [False, True] and all(f["patience"] is None for f in ref_driver)
  # early stopping: the holdout rows leave the fit
  y = R.make_labels(X, 3, seed=2)
  m = sisua_amd.GradientBoostingClassifier(n_estimators=30, n_iter_no_change=2, validation_fraction=0.2, random_state=4).fit(X, y)
  tr, va = R.holdout(y, 3, 0.2, 4)
  assert ref_driver[-1]["shape"] == (len(tr), 7) and ref_driver[-1]["n_val"] == len(va) and ref_driver[-1]["patience"] == 2
  assert m.n_estimators_ == len(m.train_score_) == len(m.validation_score_) == m.estimators_.shape[0] <= 30


def test_importance_matrix_on_the_restatement(ref_driver):
  rng = np.random.RandomState(0)
  Z = rng.normal(size=(240, 4)).astype(np.float32)
  F = np.stack([(Z[:, 0] > 0).astype(int), np.digitize(Z[:, 2], [-0.5, 0.5]), np.zeros(240, int)], axis=1)
  with pytest.warns(RuntimeWarning, match="single class"):
    M, tr, te = sisua_amd.importance_matrix(Z[:180], F[:180], Z[180:], F[180:], n_estimators=8)
  assert M.shape == (4, 3) and np.argmax(M[:, 0]) == 0 and np.argmax(M[:, 1]) == 2 and not M[:, 2].any()
  assert np.isnan(tr[2]) and np.isnan(te[2]) and (te[:2] > 0.9).all() and (tr[:2] >= te[:2] - 0.05).all()
  assert np.allclose(M[:, :2].sum(axis=0), 1.0)
  # the recalled default: n_iter_no_change=100 -> a 10 % holdout per fit, and no early stop at 8 stages
  assert all(f["patience"] == 100 and f["n_val"] == 180 - f["shape"][0] and f["shape"][0] < 180 for f in ref_driver)
  assert "[3P-recall]" in sisua_amd.importance_matrix.__doc__
  d = sisua_amd.dci_scores(M[:, :2], te[:2])
  assert d["disentanglement"] > 0.8 and d["completeness"] > 0.8 and d["informativeness"] > 0.9


def test_get_importance_matrix_on_the_restatement(ref_driver, monkeypatch):
  rng = np.random.RandomState(1)
  X = rng.poisson(2.0, size=(200, 6)).astype(np.float32)
  prot = np.stack([X[:, 1] * 3 + rng.normal(size=200), rng.normal(size=200) + 5, np.full(200, 2.0)], axis=1).astype(np.float32)
  calls = []
  real = boosting.importance_matrix

  def spy(*a, **kw):
    calls.append((a[0].shape, a[2].shape, sp.issparse(a[0]), a[1].copy(), kw))
    return real(*a, n_estimators=5, **kw)

  monkeypatch.setattr(boosting, "importance_matrix", spy)
  out = {}
  for name, x in (("dense", X), ("csr", sp.csr_matrix(X))):
    sco = SingleCellOMIC(x, omic="transcriptomic")
    sco.add_omic("proteomic", prot, ["p0", "p1", "p2"])
    with pytest.warns(RuntimeWarning, match="single class"):
      out[name] = sco.get_importance_matrix(random_state=99)
    assert sco.get_importance_matrix() is out[name] and len(calls) == (1 if name == "dense" else 2)      # kept under the uns key
    assert "importance_transcriptomic_proteomic" in sco._uns
    with pytest.raises(AssertionError):
      sco.get_importance_matrix("proteomic", "proteomic")
  assert out["dense"].shape == (6, 3) and np.array_equal(out["dense"], out["csr"]) and np.argmax(out["dense"][:, 0]) == 1
  assert not out["dense"][:, 2].any()
  shape_tr, shape_te, sparse, factors, kw = calls[1]
  assert shape_tr == (150, 6) and shape_te == (50, 6) and sparse and not calls[0][2]                    # 75 / 25; a sparse omic stays sparse
  rand = np.random.RandomState(1)                                                                       # the seed is 1 whatever random_state
  ids = rand.permutation(200)
  assert kw == dict(random_state=rand.randint(1e8))
  want = np.stack([R.quantile_codes(prot[:, j], 10) for j in range(3)], axis=1)[ids[:150]]
  assert np.array_equal(factors, want) and factors[:, 0].max() == 9
  # a discrete target is taken as it is
  sco = SingleCellOMIC(X, omic="transcriptomic")
  sco.add_omic("proteomic", np.stack([(X[:, 0] > 1).astype(np.float32), (X[:, 3] > 2).astype(np.float32) * 4], axis=1), ["a", "b"])
  sco.get_importance_matrix()
  assert set(np.unique(calls[-1][3][:, 1])) == {0.0, 4.0}


def test_header_binding_and_build_agree():
  hdr = open(build.os.path.join(ROOT, "include", "sisua_hip.h")).read()
  assert int(re.search(r"#define SMX_ABI_VERSION (\d+)", hdr).group(1)) == _hip.SMX_ABI_VERSION >= 21
  assert "smx_gbt.hip" in build.SOURCES
  for name, n_args in (("smx_gbt_bin", 9), ("smx_gbt_grow", 21), ("smx_gbt_fit", 33), ("smx_gbt_decision", 18)):
    proto = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
    assert len(proto.split(",")) == n_args == len(_hip.SIGNATURES[name][1]), name
  src = open(build.os.path.join(build.CSRC, "smx_gbt.hip")).read()
  for name in ("smx_gbt_bin", "smx_gbt_grow", "smx_gbt_fit", "smx_gbt_decision"):
    assert re.search(r"^int %s\(" % name, src, re.M), name
  for name in ("GradientBoostingClassifier", "importance_matrix", "dci_scores"):
    assert name in dir(sisua_amd)
  for name in ("k_gbt_bin", "k_gbt_grow", "k_gbt_fit", "k_gbt_decision", "GBT_MAX_CELLS", "GBT_MAX_GENES", "GBT_MAX_CLASSES", "GBT_MAX_DEPTH"):
    assert hasattr(engine, name)
  assert (engine.GBT_MAX_CELLS, engine.GBT_MAX_GENES, engine.GBT_MAX_CLASSES, engine.GBT_MAX_DEPTH) == \
      (R.MAX_CELLS, R.MAX_FEATURES, R.MAX_CLASSES, R.MAX_DEPTH) == (2 ** 20, 32768, 32, 6)
