"""The reference's gene x protein correlations restated (sisua/data/_single_cell_analysis.py:1199-1245): one scipy.stats.pearsonr and one
scipy.stats.spearmanr per (gene, protein) pair, called as lines 1226-1228 call them; and the NumPy forms of the sums the device reduces."""
import warnings

import numpy as np
from scipy.stats import pearsonr, rankdata, spearmanr


def pair_matrices(x1, x2):
  """x1 [N, G], x2 [N, P] -> (pearson [G, P], spearman [G, P]) float64.  A pair SciPy refuses (fewer than two cells) is NaN."""
  x1, x2 = np.asarray(x1), np.asarray(x2)
  pe, sp = np.full((x1.shape[1], x2.shape[1]), np.nan), np.full((x1.shape[1], x2.shape[1]), np.nan)
  for i1 in range(x1.shape[1]):
    for i2 in range(x2.shape[1]):
      y1, y2 = x1[:, i1], x2[:, i2]
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
          pe[i1, i2] = pearsonr(y1, y2)[0]
          sp[i1, i2] = spearmanr(y1, y2, nan_policy="omit").correlation
        except ValueError:
          pass
  return pe, sp


def rank2(col):
  """2 x the average ranks of a column (taken in float64): int32"""
  return np.rint(2.0 * rankdata(np.asarray(col, np.float64))).astype(np.int32)


def numpy_sums(cols, prot):
  """The sums of smx_predict_correlate in NumPy: cols [G, N] float32 (gene-major), prot [N, P] float64 -> dict with the device's keys plus
  the protein side (sp_Sb, sp_Sbb as Python integers, prot_constant).  int64 from 2 x rankdata; float64 two-pass."""
  cols = np.asarray(cols, np.float32)
  prot = np.asarray(prot, np.float64)
  a = np.stack([rank2(c) for c in cols]).astype(np.int64)
  b = np.stack([rank2(c) for c in prot.T]).astype(np.int64)
  x = cols.astype(np.float64)
  mean = x.mean(axis=1)
  dx = x - mean[:, None]
  const = np.array([bool((c == c[0]).all()) for c in prot.T])
  unit = np.zeros_like(prot.T)
  for p, c in enumerate(prot.T):
    if not const[p]:
      d = c - c.mean()
      unit[p] = d / np.linalg.norm(d)
  return dict(sp_Sa=a.sum(1), sp_Saa=(a * a).sum(1), sp_Sab=a @ b.T, pe_mean=mean, pe_Sxx=(dx * dx).sum(1), pe_Sxy=dx @ unit.T,
              nonfinite=(~np.isfinite(cols).all(axis=1)).astype(np.int32),
              sp_Sb=[int(v) for v in b.sum(1)], sp_Sbb=[int(v) for v in (b * b).sum(1)], prot_constant=const)
