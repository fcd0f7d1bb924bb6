"""NumPy restatement of the count-matrix preprocessing (the behaviour of scanpy's filter_cells, filter_genes,
normalize_total, log1p, scale and highly_variable_genes at the time of the reference, which is not installed here).  Written from the
text of the specification, one loop per bin, and kept apart from sisua_amd/preprocess.py: the tests hold one against the other.
Sums are float64; what the specification calls float32 (the view, the size factors, the scaled values) is float32 here too.
"""
import numpy as np

MAD_SCALE = 0.6745


def counts(n, g, seed, zero_cell=True, zero_gene=True):
  """Negative-binomial counts [n, g] float32: gene rates exp(N(-1, 1.3)), cell factors exp(N(0, 0.4)), Gamma(shape 2) mixing -- about
  65-70 % zeros.  Optionally one all-zero cell and one all-zero gene (never the first of either)."""
  rng = np.random.default_rng(seed)
  rate = np.exp(rng.normal(-1.0, 1.3, size=g))[None, :] * np.exp(rng.normal(0.0, 0.4, size=n))[:, None]
  x = rng.poisson(rate * rng.gamma(2.0, 0.5, size=(n, g))).astype(np.float32)
  if zero_cell and n > 2:
    x[n // 2] = 0
  if zero_gene and g > 2:
    x[:, g // 3] = 0
  return x


def exact(func):
  """f as the float64 function rounded to float32: what a correctly rounded float32 f would return"""
  f64 = {None: lambda a: a, "identity": lambda a: a, "log1p": np.log1p, "expm1": np.expm1}[func]
  return lambda a: f64(a.astype(np.float64)).astype(np.float32)


def view_argument(x, row_div=None):
  """x / c_r in float32 (IEEE division: these are the device's bits)"""
  x = np.asarray(x, np.float32)
  return x if row_div is None else x / np.asarray(row_div, np.float32)[:, None]


def view(x, func=None, row_div=None):
  return exact(func)(view_argument(x, row_div))


def stats(v, col_mask=None, row_thresh=None):
  """The statistics of a float32 matrix of view values, sums in float64"""
  v = np.asarray(v, np.float32)
  d = v.astype(np.float64)
  out = dict(total=(d if col_mask is None else d[:, np.asarray(col_mask, bool)]).sum(axis=1),
             n_genes=(v > 0).sum(axis=1).astype(np.int32), sum=d.sum(axis=0), sumsq=(d * d).sum(axis=0),
             n_cells=(v > 0).sum(axis=0).astype(np.int64))
  if row_thresh is not None:
    out["n_above"] = (v > np.asarray(row_thresh, np.float32)[:, None]).sum(axis=0).astype(np.int64)
  return out


def filter_mask(number, **bound):
  (name, value), = [(k, v) for k, v in bound.items() if v is not None]
  return number >= value if name.startswith("min") else number <= value


def filter_cells(x, min_counts=None, max_counts=None, min_genes=None, max_genes=None):
  s = stats(x)
  if min_counts is not None or max_counts is not None:
    return filter_mask(s["total"], min_counts=min_counts, max_counts=max_counts)
  return filter_mask(s["n_genes"], min_genes=min_genes, max_genes=max_genes)


def filter_genes(x, min_counts=None, max_counts=None, min_cells=None, max_cells=None):
  s = stats(x)
  if min_counts is not None or max_counts is not None:
    return filter_mask(s["sum"], min_counts=min_counts, max_counts=max_counts)
  return filter_mask(s["n_cells"], min_cells=min_cells, max_cells=max_cells)


def size_factors(x, target_sum=None, exclude_highly_expressed=False, max_fraction=0.05):
  x = np.asarray(x, np.float32)
  cnt = stats(x)["total"].astype(np.float32)
  if exclude_highly_expressed:
    above = stats(x, row_thresh=cnt * np.float32(max_fraction))["n_above"]
    cnt = stats(x, col_mask=above == 0)["total"].astype(np.float32)
  after = np.float32(target_sum) if target_sum is not None else np.median(cnt[cnt > 0])
  cnt = cnt + (cnt == 0)
  return (cnt / after).astype(np.float32)


def mean_var(v):
  n = v.shape[0]
  s = stats(v)
  mean = s["sum"] / n
  return mean, (s["sumsq"] / n - mean ** 2) * n / (n - 1)


def scale(v, max_value=None):
  """(v - mean) / std per gene in float32, mean and std from float64 moments (a zero std is 1), then the clip from above"""
  v = np.asarray(v, np.float32)
  mean, var = mean_var(v)
  with np.errstate(invalid="ignore"):
    std = np.sqrt(var)
  std[std == 0] = 1
  out = (v - mean.astype(np.float32)[None, :]) / std.astype(np.float32)[None, :]
  if max_value is not None:
    out[out > max_value] = np.float32(max_value)
  return out, mean, std


def normalize(x, total=False, log1p=False, do_scale=False, target_sum=None, exclude_highly_expressed=False, max_fraction=0.05,
              max_value=None):
  c = size_factors(x, target_sum, exclude_highly_expressed, max_fraction) if total else None
  v = view(x, "log1p" if log1p else None, c)
  return scale(v, max_value)[0] if do_scale else v


def cut_edges(means, n_bins):
  lo, hi = float(np.min(means)), float(np.max(means))
  if lo == hi:
    lo -= 0.001 * abs(lo) if lo != 0 else 0.001
    hi += 0.001 * abs(hi) if hi != 0 else 0.001
    return np.linspace(lo, hi, n_bins + 1)
  edges = np.linspace(lo, hi, n_bins + 1)
  edges[0] -= (hi - lo) * 0.001
  return edges


def codes_of(means, edges):
  """right-closed bins, one gene at a time: the first b with edges[b] < m <= edges[b + 1], else -1"""
  out = np.full(len(means), -1, np.int64)
  for i, m in enumerate(means):
    for b in range(len(edges) - 1):
      if edges[b] < m <= edges[b + 1]:
        out[i] = b
        break
  return out


def highly_variable(e, flavor="seurat", n_bins=20, n_top_genes=None, min_disp=1.0, max_disp=np.inf, min_mean=0.01, max_mean=8.0):
  """From the matrix under the expm1 view (float32) -> dict(highly_variable, means, dispersions, dispersions_norm, mean_bin, edges)"""
  mean, var = mean_var(e)
  mean[mean == 0] = 1e-12
  with np.errstate(divide="ignore", invalid="ignore"):
    disp = var / mean
    if flavor == "seurat":
      disp[disp == 0] = np.nan
      disp = np.log(disp)
      mean = np.log1p(mean)
      edges = cut_edges(mean, n_bins)
    else:
      edges = np.concatenate([[-np.inf], np.percentile(mean, np.arange(10, 105, 5)), [np.inf]])
    codes = codes_of(mean, edges)
    norm = np.full(len(mean), np.nan)
    for b in range(len(edges) - 1):
      idx = np.flatnonzero(codes == b)
      d = disp[idx]
      d = d[~np.isnan(d)]
      if d.size == 0:
        continue
      if flavor == "seurat":
        if d.size == 1:
          centre, spread = 0.0, d[0]
        else:
          centre, spread = np.mean(d), np.std(d, ddof=1)
      else:
        centre = np.median(d)
        spread = np.median(np.abs(d - centre)) / MAD_SCALE
      norm[idx] = (disp[idx] - centre) / spread
  if n_top_genes is not None:
    if 0 < n_top_genes < 1:
      n_top_genes = int(n_top_genes * len(mean))
    ranked = np.sort(norm[~np.isnan(norm)])[::-1]
    cut = ranked[min(n_top_genes, len(ranked)) - 1]
    keep = np.nan_to_num(norm) >= cut
  else:
    z = np.nan_to_num(norm)
    keep = (mean > min_mean) & (mean < max_mean) & (z > min_disp) & (z < max_disp)
  return dict(highly_variable=keep, means=mean, dispersions=disp, dispersions_norm=norm, mean_bin=codes, edges=edges)


def top_gap(norm, n_top):
  """The relative gap between the n_top-th and the next normalised dispersion: a selection is only comparable when it is not a near tie"""
  r = np.sort(norm[~np.isnan(norm)])[::-1]
  return abs(r[n_top - 1] - r[n_top]) / max(abs(r[n_top - 1]), abs(r[n_top]))


def chain(x, n_top_genes=50, n_bins=20, flavor="seurat"):
  """filter_cells(min_counts=1) . filter_genes(min_cells=3) . normalize(total, log1p) . filter_highly_variable_genes(n_top_genes), on a
  dense float32 matrix -> dict(cells, genes: the ids kept of the input; hv: the last stage's result; x: the final matrix)"""
  x = np.asarray(x, np.float32)
  cells = np.flatnonzero(filter_cells(x, min_counts=1))
  x = x[cells]
  genes = np.flatnonzero(filter_genes(x, min_cells=3))
  x = x[:, genes]
  x = normalize(x, total=True, log1p=True)
  hv = highly_variable(view(x, "expm1"), flavor, n_bins, n_top_genes)
  return dict(cells=cells, genes=genes[hv["highly_variable"]], hv=hv, x=x[:, hv["highly_variable"]])


def ulp_distance(a, b):
  """Units in the last place between two float32 arrays (finite values; +0 and -0 are 0 apart)"""
  def key(v):
    i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)
  return np.abs(key(a) - key(b))
