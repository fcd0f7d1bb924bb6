"""Ranking genes between groups, without a device: the restatement (tests/rank_groups_ref.py) is held to scipy.stats one gene and group at
a time on float64 casts, and `rank_genes_groups` / `SingleCellOMIC.rank_vars_groups` run with the two engine entries replaced by the
restatement -- the layout of the result, the order of ties, group subsets, a reference group, the cache and every refusal."""
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy import stats

import sisua_amd
from sisua_amd import _hip, build, engine, rank_groups
from sisua_amd.data import SingleCellOMIC
from tests import rank_groups_ref as R

ROOT = build.os.path.dirname(build.HERE)


def counts(N=300, G=40, K=4, seed=0):
  """Poisson counts (many ties, many zeros) with a group effect on some genes, log1p'd to float32; labels of K groups"""
  rng = np.random.RandomState(seed)
  lab = rng.randint(0, K, size=N)
  lam = np.exp(rng.normal(0.0, 1.0, size=G))[None, :] * (1.0 + 0.8 * (np.arange(G)[None, :] % K == lab[:, None]))
  return np.log1p(rng.poisson(lam)).astype(np.float32), lab


@pytest.fixture(scope="module")
def data():
  X, lab = counts()
  return X, lab, {m: R.rank_genes_groups(X, lab, method=m, n_genes=40) for m in rank_groups.METHODS}


@pytest.fixture
def no_device(monkeypatch):
  """a refusal must never reach the library"""
  def boom(*a, **k):
    raise AssertionError("the device was asked for")
  monkeypatch.setattr(_hip, "require_gpu", boom)


@pytest.fixture
def ref_driver(monkeypatch, no_device):
  """engine.k_group_* replaced by the restatement; counts the calls"""
  calls = dict(moments=0, ranksums=0)

  def moments(x, labels, n_groups, block_rows=0):
    calls["moments"] += 1
    return R.group_moments(x, labels, n_groups)

  def ranksums(cols, labels, n_groups, reference=-1):
    calls["ranksums"] += 1
    return R.group_ranksums(cols, labels, n_groups, reference)

  monkeypatch.setattr(engine, "k_group_moments", moments)
  monkeypatch.setattr(engine, "k_group_ranksums", ranksums)
  return calls


def rel(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny)))


# ---- the restatement against scipy.stats ------------------------------------------------------------------------------------------------
def test_wilcoxon_is_scipy_ranksums(data):
  X, lab, ref = data
  X64 = X.astype(np.float64)
  for k in range(4):
    want = np.array([stats.ranksums(X64[lab == k, g], X64[lab != k, g]).statistic for g in range(X.shape[1])])
    assert np.array_equal(ref["wilcoxon"][k]["all_scores"], want)


def test_wilcoxon_tie_corrected_is_scipy_mannwhitneyu(data):
  X, lab, _ = data
  X64 = X.astype(np.float64)
  got = R.rank_genes_groups(X, lab, method="wilcoxon", tie_correct=True, n_genes=40)
  for k in range(4):
    want = np.array([stats.mannwhitneyu(X64[lab == k, g], X64[lab != k, g], use_continuity=False, method="asymptotic").pvalue
                     for g in range(X.shape[1])])
    assert rel(got[k]["all_pvals"], want) < 1e-13   # (measured: 3e-15)


def test_wilcoxon_with_a_reference_is_scipy_on_the_two_groups(data):
  X, lab, _ = data
  X64 = X.astype(np.float64)
  got = R.rank_genes_groups(X, lab, method="wilcoxon", reference=2, n_genes=40)
  assert sorted(got) == [0, 1, 3]
  for k in got:
    want = np.array([stats.ranksums(X64[lab == k, g], X64[lab == 2, g]).statistic for g in range(X.shape[1])])
    assert np.array_equal(got[k]["all_scores"], want)


def test_t_test_is_scipy_ttest_ind(data):
  X, lab, ref = data
  X64 = X.astype(np.float64)
  for k in range(4):
    want = stats.ttest_ind(X64[lab == k], X64[lab != k], equal_var=False)
    assert rel(ref["t-test"][k]["all_scores"], want.statistic) < 1e-13   # (measured: 3e-16; the rest's moments come from the groups')
    assert rel(ref["t-test"][k]["all_pvals"], want.pvalue) < 1e-11
  over = ref["t-test_overestim_var"][1]
  n = int((lab == 1).sum())
  want = stats.ttest_ind_from_stats(X64[lab == 1].mean(0), X64[lab == 1].std(0, ddof=1), n, X64[lab != 1].mean(0), X64[lab != 1].std(0, ddof=1), n,
                                    equal_var=False)
  assert rel(over["all_scores"], want.statistic) < 1e-12


def test_bh_is_scipy_false_discovery_control():
  rng = np.random.RandomState(3)
  p = np.concatenate([rng.uniform(size=60), [0.0, 1.0, 0.5, 0.5, 1e-300]])
  want = stats.false_discovery_control(p, method="bh")
  assert rel(R.bh(p)[want > 0], want[want > 0]) < 1e-15 and np.array_equal(R.bh(p) == 0, want == 0)
  assert rel(rank_groups.benjamini_hochberg(p)[want > 0], want[want > 0]) < 1e-15


def test_constant_columns_score_zero_with_p_one():
  X, lab = counts(N=120, G=6, K=3, seed=2)
  X[:, 1], X[:, 4] = 0.0, 2.5
  for m in rank_groups.METHODS:
    for tc in (False, True):
      got = R.rank_genes_groups(X, lab, method=m, tie_correct=tc, n_genes=6)
      for k in got:
        assert np.array_equal(got[k]["all_scores"][[1, 4]], [0.0, 0.0]) and np.array_equal(got[k]["all_pvals"][[1, 4]], [1.0, 1.0])


# ---- the package on the restatement's entries -------------------------------------------------------------------------------------------
FIELDS = ("names", "scores", "pvals", "pvals_adj", "logfoldchanges")


@pytest.mark.parametrize("method", rank_groups.METHODS)
@pytest.mark.parametrize("sparse", [False, True])
def test_layout_and_values(ref_driver, data, method, sparse):
  X, lab, ref = data
  names = np.array([f"g{i}" for i in range(X.shape[1])])
  out = sisua_amd.rank_genes_groups(sp.csr_matrix(X) if sparse else X, lab, method=method, n_genes=7, var_names=names, pts=True, gene_chunk=9)
  assert set(out) == set(FIELDS) | {"params", "pts", "pts_rest"}
  assert out["params"]["method"] == method and out["params"]["reference"] == "rest" and out["params"]["corr_method"] == "benjamini-hochberg"
  assert ref_driver["moments"] == 1 and ref_driver["ranksums"] == (5 if method == "wilcoxon" else 0)   # (40 genes, 9 at a time)
  for f in FIELDS:
    assert out[f].shape == (7,) and out[f].dtype.names == ("0", "1", "2", "3")
  want = R.rank_genes_groups(X, lab, method=method, n_genes=7, var_names=names)
  for k in range(4):
    assert list(out["names"][str(k)]) == list(want[k]["names"])
    for f in FIELDS[1:]:
      assert rel(out[f][str(k)], want[k][f]) < 1e-9, (f, k)
  X64 = X.astype(np.float64)
  assert np.array_equal(out["pts"], np.stack([(X64[lab == k] != 0).mean(0) for k in range(4)], axis=1))
  assert np.allclose(out["pts_rest"], np.stack([(X64[lab != k] != 0).mean(0) for k in range(4)], axis=1), rtol=1e-15)


def test_equal_scores_go_to_the_lowest_gene_index(ref_driver):
  X, lab = counts(N=80, G=9, K=2, seed=4)
  X[:, 5] = X[:, 2]
  X[:, 7] = X[:, 2]
  X[:, 0] = 1.0   # (score 0: among the last)
  for method in rank_groups.METHODS:
    out = sisua_amd.rank_genes_groups(X, lab, method=method, n_genes=9)
    for k in ("0", "1"):
      order = [int(n) for n in out["names"][k]]
      at = order.index(2)
      assert order[at:at + 3] == [2, 5, 7]
      assert np.all(np.diff(out["scores"][k]) <= 0)
    both = sisua_amd.rank_genes_groups(X, lab, method=method, n_genes=9, rankby_abs=True)
    assert np.all(np.diff(np.abs(both["scores"]["0"])) <= 0) and int(both["names"]["0"][-1]) == 0


def test_groups_subset_reference_and_corrections(ref_driver, data):
  X, lab, _ = data
  words = np.array(["b", "a", "d", "c"])[lab]   # (sorted order differs from the order of appearance)
  out = sisua_amd.rank_genes_groups(X, words, groups=["d", "a"], method="wilcoxon", n_genes=5, corr_method="bonferroni", tie_correct=True)
  assert out["scores"].dtype.names == ("d", "a")
  want = R.rank_genes_groups(X, words, groups=["d", "a"], method="wilcoxon", n_genes=5, corr_method="bonferroni", tie_correct=True)
  for g in ("d", "a"):
    assert list(out["names"][g]) == list(want[g]["names"]) and rel(out["pvals_adj"][g], want[g]["pvals_adj"]) < 1e-9
    assert np.array_equal(out["pvals_adj"][g], np.minimum(out["pvals"][g] * 40, 1.0))
  for method in rank_groups.METHODS:
    out = sisua_amd.rank_genes_groups(X, words, reference="c", method=method, n_genes=5, pts=True)
    assert out["scores"].dtype.names == ("a", "b", "d") and out["params"]["reference"] == "c" and "pts_rest" not in out
    want = R.rank_genes_groups(X, words, reference="c", method=method, n_genes=5)
    for g in ("a", "b", "d"):
      assert list(out["names"][g]) == list(want[g]["names"])
      for f in FIELDS[1:]:
        assert rel(out[f][g], want[g][f]) < 1e-9, (method, f, g)


def test_refusals_never_ask_for_the_device(no_device):
  X, lab = counts(N=60, G=5, K=3, seed=5)
  with pytest.raises(NotImplementedError, match="t-test.*t-test_overestim_var.*wilcoxon"):
    sisua_amd.rank_genes_groups(X, lab, method="logreg")
  for kw in (dict(method="anova"), dict(corr_method="holm"), dict(groups=[7]), dict(reference=9), dict(n_genes=0), dict(gene_chunk=-1),
             dict(var_names=["a"])):
    with pytest.raises(ValueError):
      sisua_amd.rank_genes_groups(X, lab, **kw)
  with pytest.raises(ValueError, match="labels"):
    sisua_amd.rank_genes_groups(X, lab[:-1])
  single = lab.copy()
  single[single == 2] = 0
  single[0] = 2
  with pytest.raises(ValueError, match="at least 2"):
    sisua_amd.rank_genes_groups(X, single)
  with pytest.raises(ValueError, match="at least 2"):
    sisua_amd.rank_genes_groups(X, single, groups=[0], reference=2)
  with pytest.raises(ValueError):
    engine.k_group_moments(X, lab, 2)             # a label outside 0 .. K - 1
  with pytest.raises(ValueError):
    engine.k_group_moments(X, lab.astype(np.float64), 3)
  with pytest.raises(ValueError):
    engine.k_group_moments(X, lab, 3, block_rows=-1)
  with pytest.raises(ValueError):
    engine.k_group_ranksums(X.T, lab, 3, reference=3)
  with pytest.raises(ValueError):
    engine.k_group_ranksums(X.T, lab, 257)
  bad = X.T.copy()
  bad[1, 3] = np.inf
  with pytest.raises(ValueError, match="column 1"):
    engine.k_group_ranksums(bad, lab, 3)


def test_a_singleton_outside_the_comparison_and_non_finite_values(ref_driver):
  X, lab = counts(N=60, G=5, K=3, seed=5)
  single = lab.copy()
  single[single == 2] = 0
  single[0] = 2
  out = sisua_amd.rank_genes_groups(X, single, groups=[0, 1], method="wilcoxon", n_genes=3)
  assert out["scores"].dtype.names == ("0", "1")
  for v in (np.nan, np.inf, -np.inf):
    bad = X.copy()
    bad[7, 2] = v
    for m in ("t-test", "wilcoxon"):
      with pytest.raises(ValueError, match="gene column 2"):
        sisua_amd.rank_genes_groups(bad, lab, method=m)
      with pytest.raises(ValueError, match="gene column 2"):
        sisua_amd.rank_genes_groups(sp.csr_matrix(bad), lab, method=m)


def test_rank_vars_groups_keeps_and_drops(ref_driver, data):
  X, lab, _ = data
  onehot = np.eye(4, dtype=np.float32)[lab]   # (a 0 / 1 omic is its own probability embedding: no mixture is fitted)
  sco = SingleCellOMIC(X, var_names=[f"g{i}" for i in range(40)])
  sco.add_omic("proteomic", onehot, var_names=["CD3", "CD4", "CD8", "CD19"])
  with pytest.raises(NotImplementedError, match="wilcoxon"):
    sco.rank_vars_groups()                                        # the reference's defaults: logreg on k-means clusters
  with pytest.raises(NotImplementedError, match="clustering=None"):
    sco.rank_vars_groups(method="t-test")                         # clustering='kmeans'
  with pytest.raises(ValueError):
    sco.rank_vars_groups(method="t-test", group_by="epigenomic", clustering=None)
  with pytest.raises(ValueError):
    sco.rank_vars_groups(method="t-test", group_by=lab[:-1])
  with pytest.raises(KeyError):
    sco.get_rank_vars_groups("transcriptomic_proteomic_rank")
  assert ref_driver["moments"] == 0

  key = sco.rank_vars_groups(n_vars=6, group_by="proteomic", clustering=None, method="wilcoxon")
  assert key == "transcriptomic_proteomic_rank"
  res = sco.get_rank_vars_groups(key)
  assert res["names"].dtype.names == ("CD19", "CD3", "CD4", "CD8") and res["names"].shape == (6,)
  want = R.rank_genes_groups(X, np.array(["CD3", "CD4", "CD8", "CD19"])[lab], method="wilcoxon", n_genes=6, var_names=sco.get_var_names("transcriptomic"))
  for g in want:
    assert list(res["names"][g]) == list(want[g]["names"])
  n = ref_driver["moments"]
  assert sco.rank_vars_groups(n_vars=3, group_by="proteomic", clustering=None, method="t-test") == key and ref_driver["moments"] == n   # kept

  key2 = sco.rank_vars_groups(n_vars=4, group_by=lab, method="t-test", reference=3)
  assert key2 == "transcriptomic_labels_rank" and sco.get_rank_vars_groups(key2)["scores"].dtype.names == ("0", "1", "2")
  sco._replace("proteomic", onehot[:, ::-1].copy())
  assert key not in sco._uns and key2 in sco._uns                  # only what was made from the replaced omic goes
  sco._replace("transcriptomic", X * 2)
  assert key2 not in sco._uns
  key3 = sco.rank_vars_groups(group_by=lab, method="t-test")
  assert key3 not in sco[np.arange(100)]._uns                      # a subset starts without


def test_header_binding_and_version_agree():
  hdr = open(build.os.path.join(ROOT, "include", "sisua_hip.h")).read()
  assert int(re.search(r"#define SMX_ABI_VERSION (\d+)", hdr).group(1)) == _hip.SMX_ABI_VERSION >= 15
  assert "smx_rankgroups.hip" in build.SOURCES
  for name, n_args in (("smx_group_moments", 13), ("smx_group_ranksums", 8)):
    proto = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
    assert len(proto.split(",")) == n_args == len(_hip.SIGNATURES[name][1])
  assert "rank_genes_groups" in dir(sisua_amd)
