"""A plain NumPy / SciPy restatement of ranking genes between groups of cells, written from the definitions of the issue (scanpy's
documented behaviour, scipy.stats as the yardstick), not from the kernels: exact sums are math.fsum, ranks are scipy.stats.rankdata, and
every closing formula is evaluated one (group, gene) at a time.  tests/test_rank_groups_host.py holds it to SciPy; the GPU tests hold the
device and the package to it."""
import math

import numpy as np
from scipy import stats


def _dense64(X):
  X = X.toarray() if hasattr(X, "toarray") else np.asarray(X)
  return np.asarray(X, np.float32).astype(np.float64)   # (the matrix is float32; -0.0 == +0.0 in every comparison below)


def group_moments(X, labels, n_groups, block_rows=0):
  """-> dict(count [K], sum, css [K, G] float64, nnz [K, G] int64): the exactly rounded sum of a group's values, the exactly rounded sum
  of the float64 squares of (x - sum / count), and the values != 0"""
  X, lab, K = _dense64(X), np.asarray(labels), int(n_groups)
  G = X.shape[1]
  out = dict(count=np.bincount(lab, minlength=K).astype(np.int64), sum=np.zeros((K, G)), css=np.zeros((K, G)), nnz=np.zeros((K, G), np.int64))
  for k in range(K):
    rows = X[lab == k]
    if not len(rows):
      continue
    for g in range(G):
      v = rows[:, g]
      s = math.fsum(v)
      with np.errstate(invalid="ignore"):   # (a non-finite sum stays one)
        d = v - s / len(v)
      out["sum"][k, g], out["css"][k, g], out["nnz"][k, g] = s, math.fsum(d * d), int((v != 0).sum())
  return out


def _rank2_and_ties(v):
  """the doubled average ranks of v (integers) and sum (t^3 - t) over its runs of equal values"""
  r2 = np.rint(2.0 * stats.rankdata(v, method="average")).astype(np.int64)
  t = np.unique(v, return_counts=True)[1].astype(object)   # (Python integers: t^3 is exact whatever t)
  return r2, int((t ** 3 - t).sum())


def group_ranksums(cols, labels, n_groups, reference=-1):
  """cols [G', N] gene-major -> (rank2_sum [K, G'] int64, tie_term [G'] against the rest or [K, G'] against group `reference`)"""
  cols, lab, K = np.asarray(cols, np.float32).astype(np.float64) + 0.0, np.asarray(labels), int(n_groups)
  n = cols.shape[0]
  rank2, tie = np.zeros((K, n), np.int64), np.zeros((n,) if reference < 0 else (K, n), np.int64)
  for j in range(n):
    if reference < 0:
      r2, tie[j] = _rank2_and_ties(cols[j])
      for k in range(K):
        rank2[k, j] = r2[lab == k].sum()
    else:
      for k in range(K):
        if k == reference or not (lab == k).any():
          continue
        sel = np.concatenate([np.flatnonzero(lab == k), np.flatnonzero(lab == reference)])
        r2, tie[k, j] = _rank2_and_ties(cols[j][sel])
        rank2[k, j] = r2[: int((lab == k).sum())].sum()
  return rank2, tie


def ranksums_vectorised(X, labels, n_groups):
  """The fast SciPy route of the rank sums against the rest, for the measurement: one rankdata over the columns, one product"""
  r = stats.rankdata(_dense64(X), method="average", axis=0)
  onehot = np.zeros((int(n_groups), len(labels)))
  onehot[np.asarray(labels), np.arange(len(labels))] = 1.0
  return onehot @ r


def bh(p):
  """Benjamini-Hochberg's step-up adjusted p-values, from the definition: adj_(i) = min over j >= i of p_(j) G / j, at most 1"""
  p = np.asarray(p, np.float64)
  G, order = len(p), np.argsort(p, kind="stable")
  adj, running = np.empty(G), 1.0
  for i in range(G - 1, -1, -1):
    running = min(running, p[order[i]] * G / (i + 1))
    adj[order[i]] = running
  return adj


def _fix(score, p):
  return (0.0 if math.isnan(score) else float(score)), (1.0 if math.isnan(p) else float(p))


def welch(n1, mean1, var1, n2, mean2, var2):
  """Welch's t and two-sided p of one gene from the moments (scipy.stats.ttest_ind_from_stats); NaN -> (0, 1)"""
  with np.errstate(all="ignore"):
    t, p = stats.ttest_ind_from_stats(mean1, math.sqrt(var1), n1, mean2, math.sqrt(var2), n2, equal_var=False)
  return _fix(t, p)


def wilcoxon(R, tie, n_g, m, tie_correct):
  """z and p of a rank sum R of n_g cells among n_g + m; NaN -> (0, 1)"""
  n = n_g + m
  T = 1.0 - tie / (float(n) ** 3 - n) if tie_correct else 1.0
  sd = math.sqrt(T * n_g * m * (n + 1) / 12.0)
  z = (R - n_g * (n + 1) / 2.0) / sd if sd > 0 else float("nan")
  return _fix(z, 2.0 * stats.norm.sf(abs(z)))


def rank_genes_groups(X, labels, groups="all", reference="rest", method="t-test", corr_method="benjamini-hochberg", n_genes=100,
                      tie_correct=False, rankby_abs=False, var_names=None):
  """-> {group: dict(names, scores, pvals, pvals_adj, logfoldchanges, order, all_scores, all_pvals)}: the first n_genes genes of every
  reported group, and the unselected scores / p-values of all genes"""
  Xd, lab = _dense64(X), np.asarray(labels)
  N, G = Xd.shape
  cats, codes = np.unique(lab, return_inverse=True)
  codes = codes.reshape(-1)
  K = len(cats)
  names = np.arange(G).astype(str) if var_names is None else np.asarray(var_names)
  ref = -1 if reference == "rest" else list(cats).index(reference)
  report = [k for k in (range(K) if groups == "all" else [list(cats).index(g) for g in groups]) if k != ref]
  mom = group_moments(Xd, codes, K)
  if method == "wilcoxon":
    rank2, tie = group_ranksums(np.ascontiguousarray(Xd.T), codes, K, ref)
  out = {}
  for k in report:
    n_g = int(mom["count"][k])
    score, p, lfc = np.empty(G), np.empty(G), np.empty(G)
    for g in range(G):
      mean_g, var_g = mom["sum"][k, g] / n_g, mom["css"][k, g] / (n_g - 1)
      if ref < 0:
        m = N - n_g
        mean_c = (math.fsum(mom["sum"][:, g]) - mom["sum"][k, g]) / m
        css_c = math.fsum(mom["css"][h, g] + mom["count"][h] * (mom["sum"][h, g] / mom["count"][h] - mean_c) ** 2 for h in range(K) if h != k)
      else:
        m = int(mom["count"][ref])
        mean_c, css_c = mom["sum"][ref, g] / m, mom["css"][ref, g]
      if method == "wilcoxon":
        score[g], p[g] = wilcoxon(rank2[k, g] / 2.0, tie[g] if ref < 0 else tie[k, g], n_g, m, tie_correct)
      else:
        score[g], p[g] = welch(n_g, mean_g, var_g, n_g if method == "t-test_overestim_var" else m, mean_c, css_c / (m - 1))
      with np.errstate(all="ignore"):   # (a negative mean can make the ratio negative: NaN, as NumPy gives)
        lfc[g] = np.log2(np.float64(math.expm1(mean_g) + 1e-9) / np.float64(math.expm1(mean_c) + 1e-9))
    adj = bh(p) if corr_method == "benjamini-hochberg" else np.minimum(p * G, 1.0)
    key = np.abs(score) if rankby_abs else score
    order = np.array(sorted(range(G), key=lambda g: (-key[g], g))[: min(n_genes, G)])
    out[cats[k].item() if hasattr(cats[k], "item") else cats[k]] = dict(
        names=names[order], scores=score[order], pvals=p[order], pvals_adj=adj[order], logfoldchanges=lfc[order], order=order,
        all_scores=score, all_pvals=p)
  return out
