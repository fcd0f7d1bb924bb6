"""Ranking genes between groups of cells: "which genes mark this group?" (the reference's `SingleCellOMIC.rank_vars_groups`,
data/_single_cell_analysis.py:862-918, a proxy to `scanpy.tl.rank_genes_groups`; scanpy is not a dependency).  What is of size
cells x genes runs on the device (smx_rankgroups.hip: the groups' moments in one streamed two-pass entry, the Wilcoxon rank sums in one
sort per gene); the closing formulas below are NumPy / SciPy on [groups, genes] arrays.  Definitions: include/sisua_hip.h, restated in
tests/rank_groups_ref.py, DESIGN.md section 4z.

Deviations from scanpy, all stated: there is no `use_raw` or `layer` (the matrix is ranked as it stands), `method='logreg'` of
`rank_genes_groups` stays refused (a test pins that; `rank_genes_groups_logreg` below is the logistic ranking),
every numeric field is float64 (scanpy stores scores and log fold changes as float32), and equal scores are ordered by the lowest gene
index (scanpy leaves the order of ties open)."""
from __future__ import annotations

import numpy as np

METHODS = ("t-test", "t-test_overestim_var", "wilcoxon")
CORR_METHODS = ("benjamini-hochberg", "bonferroni")
_HOST_CHUNK_BYTES = 64 << 20   # gene columns on the host at a time (float32, gene-major)


def _engine():
  from sisua_amd import engine
  return engine


def _dense(a):
  return np.asarray(a.toarray() if hasattr(a, "toarray") else a)


def benjamini_hochberg(p):
  """The step-up adjusted p-values of p [G] (scipy.stats.false_discovery_control(method='bh'))"""
  from scipy.stats import false_discovery_control
  return false_discovery_control(np.asarray(p, np.float64), method="bh")


def _nan_to(score, p):
  score, p = np.array(score, np.float64), np.array(p, np.float64)
  score[np.isnan(score)] = 0.0
  p[np.isnan(p)] = 1.0
  return score, p


def welch_t(mean1, var1, n1, mean2, var2, n2):
  """Welch's t and its two-sided p per gene: scipy.stats.ttest_ind_from_stats(equal_var=False); NaN -> (0, 1)"""
  from scipy.stats import ttest_ind_from_stats
  with np.errstate(all="ignore"):
    t, p = ttest_ind_from_stats(mean1, np.sqrt(var1), n1, mean2, np.sqrt(var2), n2, equal_var=False)
  return _nan_to(t, p)


def ranksum_z(rank2_sum, tie_term, n_g, m, tie_correct):
  """z and p = 2 norm.sf(|z|) of the doubled rank sums [G] of a group of n_g cells against m others; NaN -> (0, 1)"""
  from scipy.special import ndtr
  n = n_g + m
  R = np.asarray(rank2_sum, np.float64) / 2.0   # (exact: 2 R < 2^53)
  T = 1.0 - np.asarray(tie_term, np.float64) / (float(n) ** 3 - n) if tie_correct else 1.0
  with np.errstate(all="ignore"):
    z = (R - n_g * (n + 1) / 2.0) / np.sqrt(T * n_g * m * (n + 1) / 12.0)
    p = 2.0 * ndtr(-np.abs(z))   # (norm.sf(x) = ndtr(-x))
  return _nan_to(z, p)


def _moments_of_rest(mom, g):
  """(n, mean [G], css [G]) of the cells outside group g from the groups' moments, float64 on the host"""
  count, S, css = mom["count"].astype(np.float64), mom["sum"], mom["css"]
  n_r = count.sum() - count[g]
  mean_r = (S.sum(axis=0) - S[g]) / n_r
  out = np.zeros_like(mean_r)
  for h in range(len(count)):
    if h != g and count[h] > 0:
      out += css[h] + count[h] * np.square(S[h] / count[h] - mean_r)
  return n_r, mean_r, out


def _comparison(X, labels, groups, reference, n_genes, var_names, gene_chunk=0):
  """The checks every method shares -> (N, G, cats, codes int32 [N], K, ref (-1: the rest), report, names [G])"""
  if getattr(X, "ndim", 0) != 2 or X.shape[0] < 1 or X.shape[1] < 1:
    raise ValueError(f"X must be [cells, genes], got {getattr(X, 'shape', None)}")
  N, G = X.shape
  lab = np.asarray(labels)
  if lab.shape != (N,):
    raise ValueError(f"labels must be [{N}], got {lab.shape}")
  if int(gene_chunk) < 0 or int(n_genes) < 1:
    raise ValueError("gene_chunk must be >= 0 and n_genes >= 1")
  cats, codes = np.unique(lab, return_inverse=True)
  codes = codes.reshape(-1).astype(np.int32)
  K = len(cats)
  index = {c.item() if hasattr(c, "item") else c: i for i, c in enumerate(cats)}

  def find(name):
    if name not in index:
      raise ValueError(f"unknown group {name!r}: the groups are {list(index)}")
    return index[name]

  ref = -1 if isinstance(reference, str) and reference == "rest" and "rest" not in index else find(reference)
  want = list(range(K)) if isinstance(groups, str) and groups == "all" else [find(g) for g in groups]
  report = [g for g in dict.fromkeys(want) if g != ref]
  if not report:
    raise ValueError("no group to report")
  names = np.arange(G).astype(str) if var_names is None else np.asarray(var_names)
  if names.shape != (G,):
    raise ValueError(f"var_names must be [{G}], got {names.shape}")
  return N, G, cats, codes, K, ref, report, names


def _plain(v):
  return v.item() if hasattr(v, "item") else v


def _records(fields, columns, dtype, top):
  rec = np.empty((top,), dtype=[(f, dtype) for f in fields])
  for f, col in zip(fields, columns):
    rec[f] = col
  return rec


def rank_genes_groups(X, labels, groups="all", reference="rest", method="t-test", corr_method="benjamini-hochberg", n_genes=100,
                      tie_correct=False, rankby_abs=False, pts=False, var_names=None, gene_chunk=0):
  """scanpy.tl.rank_genes_groups on a matrix X [cells, genes] (dense, or scipy.sparse: never densified whole) and labels [cells] (any
  sortable values; the distinct values in sorted order are the groups).  groups: 'all' or the groups to report.  reference: 'rest' (each
  group against all other cells) or a group (which is then not reported itself).  method: 't-test' (Welch), 't-test_overestim_var' (the
  comparison's size replaced by the group's), 'wilcoxon' (rank sums over the cells of the comparison, normal approximation, tie_correct
  as in scanpy).  corr_method: 'benjamini-hochberg' or 'bonferroni', over all genes of a group.  The first n_genes by decreasing score
  (|score| with rankby_abs; equal scores: the lowest gene index first) are reported.

  Returns scanpy's dict: 'params', and 'names', 'scores', 'pvals', 'pvals_adj', 'logfoldchanges' as structured arrays of n_genes rows with
  one field per reported group; with pts=True also 'pts' (and 'pts_rest' against the rest) [genes, reported groups]: the share of cells
  with a value != 0.  A group in a comparison with fewer than 2 cells, a non-finite entry of X, an unknown group or method raise
  ValueError; method='logreg' raises NotImplementedError.  gene_chunk: the genes of a Wilcoxon call on the device at a time (0: the
  library's choice); no bit depends on it."""
  eng = _engine()
  if method == "logreg":
    raise NotImplementedError(f"method='logreg' is not built: only {', '.join(repr(m) for m in METHODS)} are; logistic ranking is "
                              "rank_genes_groups_logreg (or SingleCellOMIC.rank_vars_groups(method='logreg'))")
  if method not in METHODS:
    raise ValueError(f"method must be one of {METHODS}, got {method!r}")
  if corr_method not in CORR_METHODS:
    raise ValueError(f"corr_method must be one of {CORR_METHODS}, got {corr_method!r}")
  N, G, cats, codes, K, ref, report, names = _comparison(X, labels, groups, reference, n_genes, var_names, gene_chunk)
  count = np.bincount(codes, minlength=K)
  for g in report + ([ref] if ref >= 0 else []):
    if count[g] < 2:
      raise ValueError(f"group {cats[g]!r} has {count[g]} cell(s): a comparison needs at least 2")
    if ref < 0 and N - count[g] < 2:
      raise ValueError(f"the rest of group {cats[g]!r} has {N - count[g]} cell(s): a comparison needs at least 2")

  mom = eng.k_group_moments(X, codes, K)
  bad = np.flatnonzero(~np.isfinite(mom["sum"]).all(axis=0))
  if bad.size:
    raise ValueError(f"gene column {int(bad[0])} holds a value that is not finite")
  cnt = mom["count"].astype(np.float64)
  mean = mom["sum"] / np.maximum(cnt, 1.0)[:, None]

  ranks = None
  if method == "wilcoxon":
    if N > eng.RANK_MAX_CELLS or K > eng.RANK_MAX_GROUPS:
      raise ValueError(f"method='wilcoxon' takes at most {eng.RANK_MAX_CELLS} cells and {eng.RANK_MAX_GROUPS} groups, got {N} and {K}")
    sparse = hasattr(X, "tocsc")
    Xc = X.tocsc() if sparse else X
    step = int(gene_chunk) if int(gene_chunk) > 0 else max(1, _HOST_CHUNK_BYTES // (4 * N))
    r2, tie = np.empty((K, G), np.int64), np.empty((G,) if ref < 0 else (K, G), np.int64)
    for g0 in range(0, G, step):
      g1 = min(G, g0 + step)
      cols = np.ascontiguousarray(_dense(Xc[:, g0:g1]).T, dtype=np.float32)   # gene-major: a gene's cells are contiguous
      r2[:, g0:g1], tie[..., g0:g1] = eng.k_group_ranksums(cols, codes, K, ref)
    ranks = (r2, tie)

  res = {k: [] for k in ("names", "scores", "pvals", "pvals_adj", "logfoldchanges")}
  pts_g, pts_r = [], []
  top = min(int(n_genes), G)
  for g in report:
    n_g = cnt[g]
    if ref < 0:
      n_c, mean_c, css_c = _moments_of_rest(mom, g)
    else:
      n_c, mean_c, css_c = cnt[ref], mean[ref], mom["css"][ref]
    if method == "wilcoxon":
      score, p = ranksum_z(ranks[0][g], ranks[1] if ref < 0 else ranks[1][g], n_g, n_c, tie_correct)
    else:
      score, p = welch_t(mean[g], mom["css"][g] / (n_g - 1.0), n_g, mean_c, css_c / (n_c - 1.0),
                         n_g if method == "t-test_overestim_var" else n_c)
    adj = benjamini_hochberg(p) if corr_method == "benjamini-hochberg" else np.minimum(p * G, 1.0)
    with np.errstate(all="ignore"):
      lfc = np.log2((np.expm1(mean[g]) + 1e-9) / (np.expm1(mean_c) + 1e-9))
    order = np.argsort(-(np.abs(score) if rankby_abs else score), kind="stable")[:top]   # (stable: ties to the lowest gene index)
    for k, v in zip(res, (names, score, p, adj, lfc)):
      res[k].append(v[order])
    if pts:
      pts_g.append(mom["nnz"][g] / n_g)
      if ref < 0:
        pts_r.append((mom["nnz"].sum(axis=0) - mom["nnz"][g]) / n_c)

  fields = [str(cats[g]) for g in report]
  out = {"params": dict(groupby="labels", reference="rest" if ref < 0 else _plain(cats[ref]),
                        method=method, use_raw=False, layer=None, corr_method=corr_method, tie_correct=bool(tie_correct),
                        rankby_abs=bool(rankby_abs))}
  for k, v in res.items():
    out[k] = _records(fields, v, v[0].dtype if k == "names" else np.float64, top)
  if pts:
    out["pts"] = np.stack(pts_g, axis=1)
    if ref < 0:
      out["pts_rest"] = np.stack(pts_r, axis=1)
  return out


def rank_genes_groups_logreg(X, labels, groups="all", reference="rest", n_genes=100, rankby_abs=False, var_names=None, C=1.0, tol=1e-4,
                             max_iter=1000):
  """scanpy.tl.rank_genes_groups(method='logreg') on a matrix X [cells, genes] (dense, or scipy.sparse: never densified on the host) and
  labels [cells]: the scores are the coefficients of one L2-penalised logistic regression (`sisua_amd.LogisticRegression(C, tol=tol,
  max_iter=max_iter)`, solved on the device, smx_logreg.hip).  The cells are those of the selected groups, plus the reference group if
  reference is not 'rest'; the classes are those groups in sorted order, at least two.  With three and more classes a group's scores are
  its row of coef_ and the reference group is reported like any other; with two classes the single coefficient vector is reported once,
  under the first class.  The first n_genes by decreasing score (|score| with rankby_abs; equal scores: the lowest gene index first).

  Returns a dict of 'params', 'names' and 'scores' (float64) as structured arrays of n_genes rows with one field per reported group: a
  logistic fit has no p-values and no fold changes.  One class, a class without a cell, a non-finite entry of X, an unknown group raise
  ValueError; a fit that ends above tol raises a RuntimeWarning."""
  from sisua_amd.logistic import LogisticRegression
  N, G, cats, codes, K, ref, report, names = _comparison(X, labels, groups, reference, n_genes, var_names)
  classes = sorted(set(report) | ({ref} if ref >= 0 else set()))
  if isinstance(groups, str) and groups == "all":
    classes = list(range(K))
  if len(classes) < 2:
    raise ValueError(f"a logistic regression needs at least 2 classes, got {[_plain(cats[g]) for g in classes]}")
  if len(classes) < K:
    rows = np.flatnonzero(np.isin(codes, classes))
    X, codes = X[rows], codes[rows]   # (a row selection of a dense or scipy.sparse matrix; the rows keep their order)
  model = LogisticRegression(C=C, tol=tol, max_iter=int(max_iter)).fit(X, codes)
  coef = model.coef_
  shown = classes[:1] if len(classes) == 2 else classes
  top = min(int(n_genes), G)
  cols_n, cols_s = [], []
  for i in range(len(shown)):
    order = np.argsort(-(np.abs(coef[i]) if rankby_abs else coef[i]), kind="stable")[:top]   # (stable: ties to the lowest gene index)
    cols_n.append(names[order])
    cols_s.append(coef[i][order])
  fields = [str(cats[g]) for g in shown]
  return {"params": dict(groupby="labels", reference="rest" if ref < 0 else _plain(cats[ref]), method="logreg", use_raw=False, layer=None,
                         corr_method=None, rankby_abs=bool(rankby_abs), C=float(C), tol=float(tol), max_iter=int(max_iter),
                         n_iter=int(model.n_iter_[0]), max_grad=model.max_grad_),
          "names": _records(fields, cols_n, names.dtype, top), "scores": _records(fields, cols_s, np.float64, top)}
