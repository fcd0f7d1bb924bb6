"""The host side of the gene x protein correlation matrices: `distributions.correlations_from_sums` fed NumPy-computed sums against the
reference's per-pair SciPy calls (tests/correlation_ref.py), the protein operands, and the two views `metrics.correlation_list` /
`metrics.marker_correlations`.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import correlation_ref as R


def _columns(n, rng):
  """gene columns [G, n] float32: continuous, heavily tied (counts 0..2), constant, +0 / -0, negative values"""
  cols = [rng.normal(size=n) * 10.0 ** rng.integers(-3, 3), rng.gamma(2.0, 3.0, size=n), rng.integers(0, 3, size=n), rng.integers(0, 3, size=n),
          np.full(n, 7.25), np.zeros(n), np.where(rng.uniform(size=n) < 0.5, 0.0, -0.0), -rng.gamma(2.0, 1.0, size=n),
          rng.integers(-2, 3, size=n) * 0.5]
  return np.stack(cols).astype(np.float32)


def _proteins(n, rng):
  return np.stack([rng.poisson(3.0, size=n), rng.poisson(40.0, size=n), np.full(n, 5.0), rng.normal(size=n)], axis=1).astype(np.float64)


@pytest.mark.parametrize("n", [2, 3, 257, 1537])
def test_closing_arithmetic_is_scipy(n):
  from sisua_amd.distributions import correlations_from_sums
  rng = np.random.default_rng(n)
  cols, prot = _columns(n, rng), _proteins(n, rng)
  s = R.numpy_sums(cols, prot)
  got = correlations_from_sums(n, s["sp_Sa"], s["sp_Saa"], s["sp_Sab"], s["sp_Sb"], s["sp_Sbb"], s["pe_Sxx"], s["pe_Sxy"], s["nonfinite"],
                               s["prot_constant"])
  pe, spm = R.pair_matrices(cols.T.astype(np.float64), prot)
  for key, want in (("pearson", pe), ("spearman", spm)):
    assert got[key].shape == want.shape and got[key].dtype == np.float64
    assert np.array_equal(np.isnan(got[key]), np.isnan(want)), (key, n)
    ok = ~np.isnan(want)
    delta = float(np.abs(got[key][ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"N={n} {key}: max |delta| {delta:.3e}")
    assert delta <= 1e-12, (key, n, delta)
  assert np.isnan(got["pearson"][4:7]).all() and np.isnan(got["spearman"][:, 2]).all()   # constant genes (+0 / -0 among them), constant protein
  assert np.isfinite(got["pearson"][[0, 1, 7]][:, [0, 1, 3]]).all()


def test_nonfinite_gene_gives_nan_row():
  from sisua_amd.distributions import correlations_from_sums
  rng = np.random.default_rng(5)
  cols, prot = _columns(64, rng), _proteins(64, rng)
  s = R.numpy_sums(cols, prot)
  flag = np.zeros(len(cols), np.int32)
  flag[1] = 1
  got = correlations_from_sums(64, s["sp_Sa"], s["sp_Saa"], s["sp_Sab"], s["sp_Sb"], s["sp_Sbb"], s["pe_Sxx"], s["pe_Sxy"], flag, s["prot_constant"])
  assert np.isnan(got["pearson"][1]).all() and np.isnan(got["spearman"][1]).all() and np.isfinite(got["spearman"][0, 0])


def test_protein_operands():
  from sisua_amd.distributions import protein_operands
  rng = np.random.default_rng(2)
  prot = _proteins(301, rng)
  ops = protein_operands(prot)
  s = R.numpy_sums(np.zeros((1, 301), np.float32), prot)
  assert ops["rank2"].dtype == np.int32 and ops["rank2"].shape == (4, 301) and ops["unit"].dtype == np.float64
  assert np.array_equal(ops["rank2"], np.stack([R.rank2(c) for c in prot.T]))
  assert ops["Sb"] == s["sp_Sb"] and ops["Sbb"] == s["sp_Sbb"] and all(isinstance(v, int) for v in ops["Sb"] + ops["Sbb"])
  assert list(ops["constant"]) == [False, False, True, False] and not ops["unit"][2].any()
  assert np.allclose(np.linalg.norm(ops["unit"][[0, 1, 3]], axis=1), 1.0, atol=1e-14) and np.abs(ops["unit"].sum(axis=1)).max() < 1e-12
  dense = protein_operands(prot[:, :2])
  sparse = protein_operands(sp.csr_matrix(prot[:, :2]))
  assert all(np.array_equal(dense[k], sparse[k]) for k in ("rank2", "unit", "constant")) and dense["Sb"] == sparse["Sb"]
  for bad in (np.nan, np.inf):
    p2 = prot.copy()
    p2[7, 1] = bad
    with pytest.raises(ValueError):
      protein_operands(p2)


def test_correlation_list_ordering():
  from sisua_amd.metrics import correlation_list
  pe = np.array([[0.5, np.nan, -0.2], [0.9, 0.1, np.nan]])
  spm = np.array([[0.3, 0.4, -0.4], [0.7, 0.1, np.nan]])
  got = correlation_list(pe, spm)
  assert [(g, p) for g, p, _, _ in got] == [(1, 0), (0, 0), (1, 1), (0, 2), (0, 1), (1, 2)]
  assert got[0] == (1, 0, 0.9, 0.7) and np.isnan(got[4][2]) and got[4][3] == 0.4 and np.isnan(got[5][2]) and np.isnan(got[5][3])
  # the reference's own sort on the pairs without NaN (_single_cell_analysis.py:1240-1243)
  rng = np.random.default_rng(0)
  pe, spm = rng.uniform(-1, 1, size=(5, 3)), rng.uniform(-1, 1, size=(5, 3))
  pe[2], spm[2] = pe[4], spm[4]   # equal averages
  results = [(i1, i2, pe[i1, i2], spm[i1, i2]) for i1 in range(5) for i2 in range(3)]
  want = sorted(results, key=lambda scores: (scores[-2] + scores[-1]) / 2)[::-1]
  assert correlation_list(pe, spm) == [(a, b, float(c), float(d)) for a, b, c, d in want]
  with pytest.raises(ValueError):
    correlation_list(pe, spm[:, :2])


def test_marker_correlations_keys():
  from sisua_amd.metrics import marker_correlations
  m = np.arange(12, dtype=np.float64).reshape(4, 3)
  genes, prots = ["CD3E", "CD4", "CD8A", "MS4A1"], ["CD3", "CD8", "CD45RA"]
  markers = {"CD3": "CD3E", "CD8": "CD8A", "CD19": "CD19", "CD45RA": "PTPRC"}
  assert marker_correlations(m, "pearson", genes, prots, markers) == {"pearson_CD3E_CD3": 0.0, "pearson_CD8A_CD8": 7.0}
  assert set(marker_correlations(m, "spearman", genes, prots, markers)) == {"spearman_CD3E_CD3", "spearman_CD8A_CD8"}
  with pytest.raises(NotImplementedError):
    marker_correlations(m, "mi", genes, prots, markers)
  with pytest.raises(ValueError):
    marker_correlations(m[:3], "pearson", genes, prots, markers)


def test_entry_points_are_declared():
  from sisua_amd import _hip, build
  for name in ("smx_predict_correlate", "smx_k_col_rank2", "smx_k_col_correlate"):
    assert name in _hip.SIGNATURES
  assert "smx_correlate.hip" in build.SOURCES
