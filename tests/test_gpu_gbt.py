"""smx_gbt.hip on the device against the restatement (tests/gbt_ref.py), through engine.k_gbt_*, then `sisua_amd.GradientBoostingClassifier`,
`importance_matrix`, `SingleCellOMIC.get_importance_matrix` and `model.dci_scores`.

The bins and one stage's trees are integer work: they equal the restatement exactly -- every threshold, every bin, every node record, every
cell's leaf.  Shapes, the smallest at which the launches can go wrong: rows 193 (a ragged tile of the sort, one workgroup of node sums) and
700 (three tiles, columns with more than 256 distinct values: the quantile cuts); features 1, 5 and 67 (the closing reduction over features
with idle lanes, with one wave, with a second trip); 1, 3 and 11 trees at depths 1, 3 and 6 (1 .. 352 (class, node) pairs: one pass of the
sweep up to 22); min_samples_leaf 1 and 20.  The matrices (gbt_ref.make_matrix) hold a constant column, an all-zero column (an empty CSR
column), two identical columns and negative values.

The stage loop goes through the device's exp, which may differ from NumPy's in the last place and move a quantised value by one unit of
2^-40; the fit tests therefore first assert, on the restatement alone, that at every split node the best and the second-best improvement
differ by more than a relative 1e-9 (candidates with the same left sums cut the same cells apart and count once), and then require identical structure and
values to 1e-9 relative."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import gbt_ref as R

pytestmark = pytest.mark.gpu

TREE_ARRAYS = ("feature", "threshold", "left", "right", "value", "n", "improvement")


@functools.lru_cache(maxsize=None)
def binned(N, G):
  """the matrix and the restatement's bins: computed once, shared, never written to"""
  X = R.make_matrix(N, G, seed=N + G)
  if G == 1 and N == 193:
    X[:, 0] = R.make_matrix(N, 2, seed=7)[:, 1]   # (counts: few distinct values)
  B = R.bin_matrix(X)
  for a in B.values():
    a.setflags(write=False)
  X.setflags(write=False)
  return X, B


# ---- smx_gbt_bin ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [193, 700])
@pytest.mark.parametrize("G", [1, 5, 67])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_bins_equal_the_restatement(N, G, sparse):
  from sisua_amd import engine
  X, B = binned(N, G)
  if N == 700 and G >= 5:
    # more than 256 distinct values with duplicates that straddle quantile cuts; an all-zero and a constant column
    assert len(np.unique(X[:, 0])) > 256 and 0 < B["n_thr"][0] < 255 and B["n_thr"][2] == 0 and B["n_thr"][3] == 0
  if N == 700 and G == 67:
    assert B["n_thr"][5] == 255   # (a continuous column: every quantile cut exists)
  got = engine.k_gbt_bin(sp.csr_matrix(X) if sparse else X)
  assert np.array_equal(got["n_thr"], B["n_thr"])
  assert np.array_equal(got["thr"], B["thr"])
  assert np.array_equal(got["bins"], B["bins"])


def test_bins_255_256_257_distinct_values():
  from sisua_amd import engine
  cols = []
  for d in (255, 256, 257):
    cols.append(np.resize(np.arange(d, dtype=np.float32) * 0.37 - 11.0, 600))
  X = np.stack(cols, axis=1)[np.random.RandomState(0).permutation(600)]
  B, got = R.bin_matrix(X), engine.k_gbt_bin(X)
  assert list(B["n_thr"][:2]) == [254, 255] and B["n_thr"][2] < 256
  for a in ("n_thr", "thr", "bins"):
    assert np.array_equal(got[a], B[a]), a


# ---- smx_gbt_grow ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def statistics(N, G, K):
  """integer statistics of a real stage: labels that depend on the matrix, raw scores a little off the prior"""
  X, _ = binned(N, G)
  classes = max(K, 2)
  y = R.make_labels(X, classes, seed=K)
  rng = np.random.RandomState(K)
  raw = np.tile(R.init_raw(y, classes), (N, 1)) + 0.3 * rng.normal(size=(N, 1 if classes == 2 else classes))
  q_r, q_h, _ = R.stats(raw, y, classes)
  return q_r[:K].copy(), q_h[:K].copy()


def assert_same_trees(got, ref):
  for a in TREE_ARRAYS + ("leaf",):
    assert got[a].dtype == ref[a].dtype and np.array_equal(got[a], ref[a]), a


@pytest.mark.parametrize("msl", [1, 20])
@pytest.mark.parametrize("N", [193, 700])
@pytest.mark.parametrize("G", [1, 5, 67])
@pytest.mark.parametrize("depth", [1, 3, 6])
@pytest.mark.parametrize("K", [1, 3, 11])
def test_grow_equals_the_restatement(K, depth, G, N, msl):
  from sisua_amd import engine
  _, B = binned(N, G)
  q_r, q_h = statistics(N, G, K)
  scale = 1.0 if K == 1 else (K - 1.0) / K
  ref = R.grow(B, q_r, q_h, depth, 2, msl, scale)
  got = engine.k_gbt_grow(B, q_r, q_h, depth, 2, msl, scale)
  assert_same_trees(got, ref)
  assert (ref["feature"][:, 0] >= 0).any() or G == 1   # (the case grows something)


def test_grow_a_node_that_turns_pure_at_depth_one():
  from sisua_amd import engine
  X, B = binned(193, 5)
  hit = X[:, 1] > np.median(X[:, 1])
  q_r = np.where(hit, 2 ** 39, -2 ** 39).astype(np.int64)[None, :]   # (r = +-1/2: every product below is exact)
  q_h = np.full((1, 193), 2 ** 38, np.int64)
  ref = R.grow(B, q_r, q_h, 3, 2, 1, 1.0)
  assert ref["feature"][0, 0] == 1 and list(ref["feature"][0, 1:3]) == [-1, -1] and ref["n"][0, 3:].sum() == 0
  assert list(ref["value"][0, 1:3]) == [-2.0, 2.0]
  assert_same_trees(engine.k_gbt_grow(B, q_r, q_h, 3, 2, 1, 1.0), ref)


def test_grow_identical_columns_tie_to_the_lower_index():
  from sisua_amd import engine
  X, B = binned(700, 5)
  assert np.array_equal(B["bins"][1], B["bins"][4])
  y = (X[:, 1] > 3).astype(np.int64)
  q_r, q_h, _ = R.stats(np.zeros((700, 1)), y, 2)
  ref = R.grow(B, q_r, q_h, 2, 2, 1, 1.0)
  got = engine.k_gbt_grow(B, q_r, q_h, 2, 2, 1, 1.0)
  assert ref["feature"][0, 0] == 1 and got["feature"][0, 0] == 1
  assert_same_trees(got, ref)


@pytest.mark.parametrize("pass_pairs", [1, 3, 7])
def test_grow_pass_size_changes_no_bit(pass_pairs):
  from sisua_amd import engine
  _, B = binned(193, 5)
  q_r, q_h = statistics(193, 5, 11)
  want = engine.k_gbt_grow(B, q_r, q_h, 6, 2, 1, 10.0 / 11.0)
  got = engine.k_gbt_grow(B, q_r, q_h, 6, 2, 1, 10.0 / 11.0, pass_pairs=pass_pairs)
  for a in TREE_ARRAYS + ("leaf",):
    assert got[a].tobytes() == want[a].tobytes(), a


# ---- smx_gbt_fit ----------------------------------------------------------------------------------------------------------------------------
FIT_SEED = {2: 0, 4: 0}   # seeds at which the restatement's splits are clear of ties (asserted below, on the CPU)


@functools.lru_cache(maxsize=None)
def fit_case(K):
  X = R.make_matrix(400, 12, seed=100 + FIT_SEED[K])
  y = R.make_labels(X, K, seed=FIT_SEED[K])
  margins = []
  ref = R.fit(X, y, K, n_estimators=15, margins=margins)
  return X, y, ref, np.array(margins)


@pytest.mark.parametrize("K", [2, 4])
def test_fit_equals_the_restatement(K):
  from sisua_amd import engine
  X, y, ref, margins = fit_case(K)
  assert margins.size and margins.min() > 1e-9, margins.min()
  got = engine.k_gbt_fit(X, y, K, n_estimators=15)
  assert got["n_estimators_"] == 15
  for a in ("feature", "threshold", "left", "right", "n"):
    assert np.array_equal(got[a], ref[a]), a
  leaves = (ref["feature"] < 0) & (ref["n"] > 0)
  assert np.allclose(got["value"][leaves], ref["value"][leaves], rtol=1e-9, atol=0)
  assert np.allclose(got["train_score_"], ref["train_score_"], rtol=1e-9, atol=0)
  raw = engine.k_gbt_decision(X, got, got["init"], 0.1)
  assert np.allclose(raw, ref["raw"], rtol=1e-9, atol=0)
  from sisua_amd.boosting import feature_importances
  assert np.allclose(feature_importances(got, 12), R.feature_importances(ref, 12), rtol=1e-9, atol=0)


@pytest.mark.parametrize("K", [2, 4])
def test_fit_same_bits_dense_csr_twice_and_block_rows(K):
  from sisua_amd import engine
  X, y, _, _ = fit_case(K)
  a, b, c = engine.k_gbt_fit(X, y, K, n_estimators=15), engine.k_gbt_fit(X, y, K, n_estimators=15), \
      engine.k_gbt_fit(sp.csr_matrix(X), y, K, n_estimators=15)
  for name in TREE_ARRAYS + ("train_score_",):
    assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes(), name
  r0 = engine.k_gbt_decision(X, a, a["init"], 0.1)
  for x, br in ((X, 64), (sp.csr_matrix(X), 0), (sp.csr_matrix(X), 128)):
    assert engine.k_gbt_decision(x, a, a["init"], 0.1, block_rows=br).tobytes() == r0.tobytes()
  assert r0.shape == (400, 1 if K == 2 else K)


def test_fit_early_stopping_stops_at_the_restatements_stage():
  from sisua_amd import engine
  X = R.make_matrix(400, 12, seed=5)
  y = R.make_labels(X, 3, seed=5, noise=4.0)   # (mostly noise: the validation loss turns early)
  tr, va = R.holdout(y, 3, 0.25, 7)
  ref = R.fit(X[tr], y[tr], 3, n_estimators=40, X_val=X[va], y_val=y[va], n_iter_no_change=3, tol=1e-4)
  assert 3 < ref["n_estimators_"] < 40
  gaps = np.abs(np.diff(ref["val_score"]))
  got = engine.k_gbt_fit(X[tr], y[tr], 3, n_estimators=40, x_val=X[va], labels_val=y[va], n_iter_no_change=3, tol=1e-4)
  assert got["n_estimators_"] == ref["n_estimators_"], (got["val_score"], ref["val_score"], gaps)
  assert np.allclose(got["val_score"], ref["val_score"], rtol=1e-9, atol=0)
  assert np.array_equal(got["feature"], ref["feature"])


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------
def test_classifier_predict_proba_and_score():
  import sisua_amd
  for K in (2, 4):
    X, y, ref, _ = fit_case(K)
    names = np.array(["t%d" % k for k in range(K)])
    m = sisua_amd.GradientBoostingClassifier(n_estimators=15).fit(sp.csr_matrix(X), names[y])
    raw = ref["raw"]
    if K == 2:
      p1 = 1.0 / (1.0 + np.exp(-raw[:, 0]))
      want = np.stack([1.0 - p1, p1], axis=1)
    else:
      e = np.exp(raw - raw.max(axis=1, keepdims=True))
      want = e / e.sum(axis=1, keepdims=True)
    p = m.predict_proba(X)
    assert p.shape == (400, K) and np.allclose(p, want, rtol=1e-8, atol=1e-12)
    assert m.score(X, names[y]) == np.mean(names[np.argmax(want, axis=1)] == names[y]) > 1.5 / K
    assert m.n_estimators_ == 15 and m.estimators_.shape == (15, 1 if K == 2 else K) and list(m.classes_) == list(names)
    assert np.allclose(m.feature_importances_, R.feature_importances(ref, 12), rtol=1e-9, atol=0)
    staged = list(m.staged_decision_function(X))
    assert len(staged) == 15 and staged[-1].tobytes() == m.decision_function(X).tobytes()
    assert np.allclose(staged[4].reshape(400, -1), R.decision(ref, ref["init"], 0.1, X, n_stages=5), rtol=1e-9, atol=0)


@functools.lru_cache(maxsize=None)
def factor_case():
  rng = np.random.RandomState(0)
  Z = rng.normal(size=(320, 5)).astype(np.float32)
  F = np.stack([(Z[:, 0] > 0).astype(int), np.digitize(Z[:, 2], [-0.5, 0.5]), np.digitize(Z[:, 4] + 0.5 * Z[:, 0], [-1.0, 0.0, 1.0])], axis=1)
  return Z, F


def test_importance_matrix_on_three_factors():
  import sisua_amd
  Z, F = factor_case()
  M, tr, te = sisua_amd.importance_matrix(Z[:240], F[:240], Z[240:], F[240:], random_state=11, n_estimators=12)
  assert M.shape == (5, 3) and np.allclose(M.sum(axis=0), 1.0) and list(np.argmax(M, axis=0)) == [0, 2, 4]
  # the restatement on the same rows: the holdout of the recalled default (n_iter_no_change=100: 10 % per class), then 12 stages
  for f in range(3):
    a, b = R.holdout(F[:240, f], len(np.unique(F[:240, f])), 0.1, 11)
    K = len(np.unique(F[:240, f]))
    ref = R.fit(Z[a], F[a, f], K, n_estimators=12, X_val=Z[:240][b], y_val=F[b, f], n_iter_no_change=100)
    assert ref["n_estimators_"] == 12
    assert np.allclose(M[:, f], R.feature_importances(ref, 5), rtol=1e-9, atol=1e-15)
    raw = R.decision(ref, ref["init"], 0.1, Z[240:])
    pred = (raw[:, 0] > 0).astype(int) if K == 2 else np.argmax(raw, axis=1)
    assert abs(te[f] - np.mean(pred == F[240:, f])) <= 1.0 / 80 + 1e-12 and te[f] > 0.8 and tr[f] >= te[f] - 0.05
  d = sisua_amd.dci_scores(M, te)
  assert d["disentanglement"] > 0.5 and d["completeness"] > 0.5 and d["informativeness"] == pytest.approx(te.mean())


def test_get_importance_matrix_caches_and_dense_equals_csr():
  import warnings
  from sisua_amd.data import SingleCellOMIC
  rng = np.random.RandomState(1)
  X = rng.poisson(2.0, size=(200, 9)).astype(np.float32)
  prot = np.stack([X[:, 1] * 3 + rng.normal(size=200), X[:, 4] - X[:, 7] + 0.3 * rng.normal(size=200)], axis=1).astype(np.float32)
  out = {}
  for name, x in (("dense", X), ("csr", sp.csr_matrix(X))):
    sco = SingleCellOMIC(x, omic="transcriptomic")
    sco.add_omic("proteomic", prot, ["p0", "p1"])
    with warnings.catch_warnings():
      warnings.simplefilter("error")
      out[name] = sco.get_importance_matrix()
    assert sco.get_importance_matrix(random_state=5) is out[name] and "importance_transcriptomic_proteomic" in sco._uns
  assert out["dense"].shape == (9, 2) and out["dense"].tobytes() == out["csr"].tobytes()
  assert np.argmax(out["dense"][:, 0]) == 1 and set(np.argsort(out["dense"][:, 1])[-2:]) == {4, 7}
  assert np.allclose(out["dense"].sum(axis=0), 1.0)


def test_model_dci_scores_on_a_tiny_fitted_sisua():
  """Three planted cell types drive the genes and the protein counts SISUA is supervised with; the one-hot type matrix collapses to one
  categorical factor.  The restatement on the same latent means (same split, same holdout, 20 stages) gives the factor's test accuracy;
  the device must report it to within one test cell, and it must exceed chance (1/3) by at least half the restatement's own excess."""
  import sisua_amd.models as M
  from sisua_amd.data import SingleCellOMIC
  rng = np.random.RandomState(4)
  N, G = 240, 60
  kind = np.arange(N) % 3
  rate = np.where(np.arange(G)[None, :] % 3 == kind[:, None], 6.0, 0.5)
  x = rng.poisson(rate).astype(np.float32)
  prot = rng.poisson(np.where(np.arange(3)[None, :] == kind[:, None], 20.0, 1.0)).astype(np.float32)
  sco = SingleCellOMIC(x, name="planted")
  sco.add_omic("proteomic", prot)
  net = dict(encoder=M.NetConf([32], batchnorm=True, dropout=0.1), decoder=M.NetConf([32], batchnorm=True, dropout=0.1))
  m = M.SISUA(outputs=M.RVmeta(G, "zinb", True, "transcriptomic"), labels=[M.RVmeta(3, "nb", True, "proteomic")],
              latents=M.RVmeta(6, "diag", True, "Latents"), **net)
  m.fit(sco, epochs=4, batch_size=64, verbose=False)
  onehot = np.eye(3)[kind]
  got = m.dci_scores(x, onehot, n_estimators=20)
  assert set(got) == {"dci_disentanglement", "dci_completeness", "dci_informativeness"} and all(np.isfinite(v) for v in got.values())
  assert m.dci_scores(sp.csr_matrix(x), onehot, n_estimators=20, batch_size=32) == got
  # the restatement on the same latents
  z = np.ascontiguousarray(np.asarray(m.encode(x).mean()), dtype=np.float32)
  rand = np.random.RandomState(1)
  ids = rand.permutation(N)
  train, test = ids[:180], ids[180:]
  a, b = R.holdout(kind[train], 3, 0.1, rand.randint(1e8))
  ref = R.fit(z[train][a], kind[train][a], 3, n_estimators=20, X_val=z[train][b], y_val=kind[train][b], n_iter_no_change=100)
  want = float(np.mean(np.argmax(R.decision(ref, ref["init"], 0.1, z[test]), axis=1) == kind[test]))
  chance = 1.0 / 3.0
  print(f"dci on the planted factor: device {got}, the restatement's test accuracy {want:.4f}")
  assert want - chance > 0.2
  assert abs(got["dci_informativeness"] - want) <= 1.0 / 60 + 1e-12
  assert got["dci_informativeness"] > chance + 0.5 * (want - chance)
  assert 0.0 <= got["dci_disentanglement"] <= 1.0 and got["dci_completeness"] > 0.0
