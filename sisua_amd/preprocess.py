"""Count-matrix preprocessing: what the reference's loaders call on a SingleCellOMIC before they train
(sisua/data/_single_cell_analysis.py: filter_cells, filter_genes, normalize, expm1, filter_highly_variable_genes -- proxies to
scanpy there; scanpy is not a dependency here, DESIGN.md section 4q states the behaviour this file restates).

The two things of size cells x genes run on the device (smx_prep.hip through engine.k_prep_stats / k_prep_apply): the statistics of
a VIEW f(x / c_r) of the matrix, and the view written out.  Everything of size cells or genes is NumPy here: bounds, size factors,
moments, bins, cut-offs.  The host functions take statistics, not matrices, and never load the library; the drivers at the end of
the file check every argument first and only then ask for the device.  No pandas: the bins of pandas.cut are restated.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

MAX_CELLS = 2 ** 31 - 1   # the limits of smx_prep_stats / smx_prep_apply (include/sisua_hip.h)
MAX_GENES = 2 ** 20
MAD_SCALE = 0.6745        # median(|d - median|) / 0.6745: the robust standard deviation of the 'cell_ranger' flavour
FLAVORS = ("seurat", "cell_ranger")


# ---------------------------------------------------------------------------
# argument checks (no device, no library)
# ---------------------------------------------------------------------------
def check_shape(n_cells: int, n_genes: int):
  if not 1 <= int(n_cells) <= MAX_CELLS:
    raise ValueError(f"n_cells = {n_cells} is outside the limit 1 .. 2^31 - 1 (MAX_CELLS)")
  if not 1 <= int(n_genes) <= MAX_GENES:
    raise ValueError(f"n_genes = {n_genes} is outside the limit 1 .. 2^20 (MAX_GENES)")


def single_bound(names, values) -> Tuple[str, float]:
  """scanpy's rule for filter_cells / filter_genes: exactly one of the four bounds -> (its name, its value)"""
  given = [(n, v) for n, v in zip(names, values) if v is not None]
  if len(given) != 1:
    raise ValueError("Only provide one of the optional parameters " + ", ".join(f"`{n}`" for n in names) + " per call.")
  return given[0][0], float(given[0][1])


def keep_by_bound(number, name: str, value: float) -> np.ndarray:
  """number >= min or number <= max"""
  number = np.asarray(number)
  return number >= value if name.startswith("min_") else number <= value


def check_normalize(target_sum, max_fraction, max_value):
  if target_sum is not None and not (np.isfinite(target_sum) and target_sum > 0):
    raise ValueError(f"target_sum must be a positive finite number (limit: > 0), got {target_sum}")
  if not 0 < float(max_fraction) < 1:
    raise ValueError(f"max_fraction must lie in the open interval (0, 1) (limits 0 and 1), got {max_fraction}")
  if max_value is not None and np.isnan(max_value):
    raise ValueError("max_value is NaN")


def check_variable_genes(n_genes: int, n_cells: int, n_top_genes, n_bins, flavor) -> Tuple[Optional[int], int, str]:
  """-> (n_top_genes as a count or None, n_bins, flavor); a share in (0, 1) becomes int(share * n_genes) as in the reference"""
  flavor = str(flavor).lower()
  if flavor not in FLAVORS:
    raise ValueError('`flavor` needs to be "seurat" or "cell_ranger"')
  if int(n_bins) < 1:
    raise ValueError(f"n_bins must be at least 1 (limit: >= 1), got {n_bins}")
  if n_cells < 2:
    raise ValueError(f"a variance needs at least 2 cells (limit: n_cells >= 2), got {n_cells}")
  if n_top_genes is not None:
    if 0. < n_top_genes < 1.:
      n_top_genes = int(n_top_genes * n_genes)
    if int(n_top_genes) != n_top_genes or n_top_genes < 1:
      raise ValueError(f"n_top_genes must be a count of at least 1 or a share in (0, 1) (limit: >= 1), got {n_top_genes}")
    n_top_genes = int(n_top_genes)
  return n_top_genes, int(n_bins), flavor


# ---------------------------------------------------------------------------
# host arithmetic on statistics
# ---------------------------------------------------------------------------
def size_factors(total, target_sum=None) -> np.ndarray:
  """scanpy.pp.normalize_total's divisor per cell from the cells' totals: counts float32; after = target_sum or the median of the positive
  counts; counts += (counts == 0); c = counts / after in float32"""
  counts = np.asarray(total).astype(np.float32)
  if target_sum is None:
    if not (counts > 0).any():
      raise ValueError("normalize(total=True) without target_sum needs a cell with a positive total")
    after = np.median(counts[counts > 0])
  else:
    after = np.float32(target_sum)
  counts = counts + (counts == 0).astype(np.float32)
  return (counts / np.float32(after)).astype(np.float32)


def moments(gene_sum, gene_sumsq, n: int) -> Tuple[np.ndarray, np.ndarray]:
  """mean = sum / n, var = (sumsq / n - mean^2) n / (n - 1), float64"""
  s, q = np.asarray(gene_sum, np.float64), np.asarray(gene_sumsq, np.float64)
  mean = s / n
  return mean, (q / n - mean ** 2) * (n / (n - 1))


def scale_params(gene_sum, gene_sumsq, n: int) -> Tuple[np.ndarray, np.ndarray]:
  """The float32 (mean, std) of scanpy.pp.scale: std = sqrt(var), a zero std becomes 1"""
  mean, var = moments(gene_sum, gene_sumsq, n)
  with np.errstate(invalid="ignore"):
    std = np.sqrt(var)
  std[std == 0] = 1
  return mean.astype(np.float32), std.astype(np.float32)


def equal_width_bins(x, n_bins: int) -> Tuple[np.ndarray, np.ndarray]:
  """(codes, edges) of pandas.cut(x, bins=n_bins): n_bins equal-width right-closed bins over [min, max], the lowest edge lowered by 0.1 % of
  the range (a constant x: the range widened by 0.1 % of |x|, or by 0.001 at 0); -1 for a NaN"""
  x = np.asarray(x, np.float64)
  lo, hi = np.nanmin(x), np.nanmax(x)
  if lo == hi:
    lo -= 0.001 * abs(lo) if lo != 0 else 0.001
    hi += 0.001 * abs(hi) if hi != 0 else 0.001
    edges = np.linspace(lo, hi, n_bins + 1)
  else:
    edges = np.linspace(lo, hi, n_bins + 1)
    edges[0] -= (hi - lo) * 0.001
  return right_closed_codes(x, edges), edges


def percentile_bins(x) -> Tuple[np.ndarray, np.ndarray]:
  """(codes, edges) of the 'cell_ranger' bins: edges -inf, the 10, 15, ..., 100th percentiles of x, +inf; right-closed"""
  x = np.asarray(x, np.float64)
  edges = np.r_[-np.inf, np.percentile(x, np.arange(10, 105, 5)), np.inf]
  return right_closed_codes(x, edges), edges


def right_closed_codes(x, edges) -> np.ndarray:
  """bin b holds edges[b] < x <= edges[b + 1]; -1 outside every bin and for a NaN"""
  ids = np.searchsorted(edges, x, side="left")
  bad = np.isnan(x) | (ids == 0) | (ids == len(edges))
  return np.where(bad, -1, ids - 1).astype(np.int64)


def _bin_centre_spread(d, codes, n_bins: int, flavor: str):
  """Per bin, over its non-NaN dispersions: 'seurat' the mean and the ddof = 1 standard deviation, a bin with fewer than two of them taking
  (0, its mean) instead so that a lone gene normalises to exactly 1; 'cell_ranger' the median and median(|d - median|) / MAD_SCALE"""
  centre, spread = np.full(n_bins, np.nan), np.full(n_bins, np.nan)
  order = np.argsort(codes, kind="stable")
  sc = codes[order]
  starts = np.searchsorted(sc, np.arange(n_bins), side="left")
  ends = np.searchsorted(sc, np.arange(n_bins), side="right")
  for b in range(n_bins):
    v = d[order[starts[b]:ends[b]]]
    v = v[~np.isnan(v)]
    if v.size == 0:
      continue
    if flavor == "seurat":
      m = v.sum() / v.size
      if v.size > 1:
        centre[b], spread[b] = m, np.sqrt(((v - m) ** 2).sum() / (v.size - 1))
      else:
        centre[b], spread[b] = 0.0, m
    else:
      m = np.median(v)
      centre[b], spread[b] = m, np.median(np.abs(v - m)) / MAD_SCALE
  return centre, spread


def normalized_dispersion(mean, var, flavor: str = "seurat", n_bins: int = 20) -> dict:
  """scanpy.pp.highly_variable_genes' statistics from the genes' mean and variance (float64, of the expm1 view): means, dispersions,
  dispersions_norm [G] float64 and the genes' bin (mean_bin, -1: none)"""
  mean, var = np.array(mean, np.float64), np.asarray(var, np.float64)
  mean[mean == 0] = 1e-12
  with np.errstate(divide="ignore", invalid="ignore"):
    disp = var / mean
    if flavor == "seurat":
      disp[disp == 0] = np.nan
      disp = np.log(disp)
      mean = np.log1p(mean)
      codes, _ = equal_width_bins(mean, n_bins)
      nb = n_bins
    else:
      codes, edges = percentile_bins(mean)
      nb = len(edges) - 1
    centre, spread = _bin_centre_spread(disp, codes, nb, flavor)
    inside = codes >= 0
    norm = np.full(mean.shape, np.nan)
    norm[inside] = (disp[inside] - centre[codes[inside]]) / spread[codes[inside]]
  return dict(means=mean, dispersions=disp, dispersions_norm=norm, mean_bin=codes)


def select_variable(means, dispersions_norm, n_top_genes: Optional[int] = None, min_disp=1.0, max_disp=np.inf, min_mean=0.01,
                    max_mean=8.0) -> np.ndarray:
  """With n_top_genes: nan_to_num(dispersions_norm) >= the n_top_genes-th largest non-NaN one (ties may keep more; fewer non-NaN genes than
  asked: all of them).  Otherwise the four open intervals on the mean and the normalised dispersion (a NaN counting as 0)."""
  norm = np.asarray(dispersions_norm, np.float64)
  if n_top_genes is not None:
    ok = np.sort(norm[~np.isnan(norm)])[::-1]
    if ok.size == 0:
      raise ValueError("no gene has a normalised dispersion: nothing to rank")
    cut = ok[min(int(n_top_genes), ok.size) - 1]
    return np.nan_to_num(norm) >= cut
  z = np.where(np.isnan(norm), 0.0, norm)
  m = np.asarray(means, np.float64)
  return (m > min_mean) & (m < max_mean) & (z > min_disp) & (z < max_disp)


def highly_variable(gene_sum, gene_sumsq, n_cells: int, flavor="seurat", n_bins=20, n_top_genes=None, min_disp=1.0, max_disp=np.inf,
                    min_mean=0.01, max_mean=8.0) -> dict:
  """From the per-gene sums of the expm1 view -> dict(highly_variable bool [G], means, dispersions, dispersions_norm float64 [G])"""
  mean, var = moments(gene_sum, gene_sumsq, n_cells)
  out = normalized_dispersion(mean, var, flavor, n_bins)
  out["highly_variable"] = select_variable(out["means"], out["dispersions_norm"], n_top_genes, min_disp, max_disp, min_mean, max_mean)
  return out


# ---------------------------------------------------------------------------
# drivers: arguments checked, then the device
# ---------------------------------------------------------------------------
def _stats(x, **kw):
  from sisua_amd import engine
  check_shape(*x.shape)
  return engine.k_prep_stats(x, **kw)


def filter_cells(x, min_counts=None, max_counts=None, min_genes=None, max_genes=None):
  """-> (cells_subset bool [N], number_per_cell): the cell's total for a *_counts bound, its entries > 0 for a *_genes bound"""
  name, value = single_bound(("min_counts", "min_genes", "max_counts", "max_genes"), (min_counts, min_genes, max_counts, max_genes))
  st = _stats(x)
  number = st["total"] if name.endswith("counts") else st["n_genes"]
  return keep_by_bound(number, name, value), number


def filter_genes(x, min_counts=None, max_counts=None, min_cells=None, max_cells=None):
  """-> (gene_subset bool [G], number_per_gene): the gene's sum for a *_counts bound, its entries > 0 for a *_cells bound"""
  name, value = single_bound(("min_counts", "min_cells", "max_counts", "max_cells"), (min_counts, min_cells, max_counts, max_cells))
  st = _stats(x)
  number = st["sum"] if name.endswith("counts") else st["n_cells"]
  return keep_by_bound(number, name, value), number


def total_size_factors(x, target_sum=None, exclude_highly_expressed=False, max_fraction=0.05) -> np.ndarray:
  """The per-cell divisor of normalize(total=True), float32 [N].  exclude_highly_expressed: a gene that holds more than max_fraction of
  the total of some cell is left out of the totals (a second pass with the column mask)."""
  check_normalize(target_sum, max_fraction, None)
  st = _stats(x)
  if exclude_highly_expressed:
    counts = st["total"].astype(np.float32)
    above = _stats(x, row_thresh=counts * np.float32(max_fraction))["n_above"]
    st = _stats(x, col_mask=(above == 0).astype(np.uint8))
  return size_factors(st["total"], target_sum)


def apply_view(x, func=None, row_div=None, scale=False, max_value=None):
  """The matrix under f(x / row_div); scale: then (v - mean) / std per gene, the moments those of the view, and the clip from above at
  max_value.  Sparse in, sparse out unless scaled."""
  from sisua_amd import engine
  check_shape(*x.shape)
  if not scale:
    return engine.k_prep_apply(x, func=func, row_div=row_div)
  if x.shape[0] < 2:
    raise ValueError(f"a variance needs at least 2 cells (limit: n_cells >= 2), got {x.shape[0]}")
  st = engine.k_prep_stats(x, func=func, row_div=row_div)
  mean, std = scale_params(st["sum"], st["sumsq"], x.shape[0])
  return engine.k_prep_apply(x, func=func, row_div=row_div, mean=mean, std=std, max_value=max_value)


def highly_variable_genes(x, min_disp=1.0, max_disp=np.inf, min_mean=0.01, max_mean=8.0, n_top_genes=None, n_bins=20,
                          flavor="seurat") -> dict:
  n_top_genes, n_bins, flavor = check_variable_genes(x.shape[1], x.shape[0], n_top_genes, n_bins, flavor)
  st = _stats(x, func="expm1")
  return highly_variable(st["sum"], st["sumsq"], x.shape[0], flavor, n_bins, n_top_genes, min_disp, max_disp, min_mean, max_mean)
