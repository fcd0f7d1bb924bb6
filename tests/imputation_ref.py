"""NumPy restatement of the reference's imputation scores (sisua/analysis/imputation_benchmarks.py:102-127), written from their
definition: tests/golden/imputation_fixture.npz holds what the reference's own functions return, and tests/test_imputation_host.py checks
that these reproduce it bit for bit.  The GPU tests compare the device's selections with these."""
import numpy as np


def abs_diff(original, imputed):
  original, imputed = np.asarray(original), np.asarray(imputed)
  assert original.shape == imputed.shape
  return np.abs(original - imputed)


def imputation_score(original, imputed):
  """median of |original - imputed| over ALL entries"""
  return float(np.median(abs_diff(original, imputed)))


def cell_changed(original, corrupted):
  """[N] bool: the cell's total differs between the two matrices (np.sum of the row, in the row's dtype)"""
  return np.array([np.sum(o) != np.sum(c) for o, c in zip(np.asarray(original), np.asarray(corrupted))], dtype=bool)


def cell_medians(original, imputed):
  """[N]: np.median of every cell's |original - imputed| (the row's dtype)"""
  d = abs_diff(original, imputed)
  return np.array([np.median(r) for r in d], dtype=d.dtype)


def _changed_medians(original, corrupted, imputed):
  assert np.shape(original) == np.shape(corrupted) == np.shape(imputed)
  return [m for m, c in zip(cell_medians(original, imputed), cell_changed(original, corrupted)) if c]


def imputation_mean_score(original, corrupted, imputed):
  cells = _changed_medians(original, corrupted, imputed)
  return np.mean(cells) if len(cells) > 0 else 0


def imputation_std_score(original, corrupted, imputed):
  cells = _changed_medians(original, corrupted, imputed)
  return np.std(cells) if len(cells) > 0 else 0


def scores(original, corrupted, imputed):
  """the three keys of Posterior.cal_imputation_scores as Python floats"""
  return {"imputation_med": imputation_score(original, imputed),
          "imputation_mean": float(imputation_mean_score(original, corrupted, imputed)),
          "imputation_std": float(imputation_std_score(original, corrupted, imputed))}


def middle_two(rows, n=None):
  """the order statistics (n - 1) // 2 and n // 2 of the first n entries of every row, by np.partition (NaN last): (lo, hi)"""
  rows = np.asarray(rows)
  n = rows.shape[1] if n is None else n
  p = np.partition(rows[:, :n], sorted({(n - 1) // 2, n // 2}), axis=1)
  return p[:, (n - 1) // 2].copy(), p[:, n // 2].copy()
