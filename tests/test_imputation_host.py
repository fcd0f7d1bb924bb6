"""Host side of the imputation scores: tests/imputation_ref.py reproduces what the reference's own functions returned
(tests/golden/imputation_fixture.npz, made by tests/golden/make_imputation_fixtures.py) bit for bit; the closing reductions of the
device's selections; argument checks; the metric classes against a stand-in model; the C-ABI's new symbols."""
import os
import warnings

import numpy as np
import pytest

from tests import imputation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "imputation_fixture.npz"))
CASES = sorted({k.split("/")[0] for k in FIX.files})


def _identical(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.dtype == b.dtype and a.shape == b.shape and (a.tobytes() == b.tobytes() or bool(np.all(np.isnan(a) & np.isnan(b))))


def test_fixture_covers_the_cases():
  assert {"odd", "even", "ties", "nan", "unchanged", "one_gene"} <= set(CASES)
  assert FIX["odd/original"].shape[1] % 2 == 1 and FIX["even/original"].shape[1] % 2 == 0
  assert np.isnan(FIX["nan/med"]) and FIX["unchanged/mean"] == 0 and FIX["unchanged/std"] == 0
  ch = R.cell_changed(FIX["even/original"], FIX["even/corrupted"])
  assert ch.any() and not ch.all()


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
  org, crt, imp = (FIX[f"{case}/{k}"] for k in ("original", "corrupted", "imputed"))
  assert org.dtype == np.float32 and imp.dtype == np.float32
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    assert _identical(R.imputation_score(org, imp), FIX[f"{case}/med"])
    assert _identical(R.imputation_mean_score(org, crt, imp), FIX[f"{case}/mean"])
    assert _identical(R.imputation_std_score(org, crt, imp), FIX[f"{case}/std"])


@pytest.mark.parametrize("case", CASES)
def test_closing_reductions_of_the_selections(case):
  """what LazyCountOutput.imputation_scores does with the device's selections == the reference, given exact selections"""
  from sisua_amd.distributions import imputation_scores_from_cells
  org, crt, imp = (FIX[f"{case}/{k}"] for k in ("original", "corrupted", "imputed"))
  d = R.abs_diff(org, imp)
  lo, hi = R.middle_two(d.reshape(1, -1))
  rlo, rhi = R.middle_two(d)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    med = np.where(np.isnan(d).any(axis=1), np.float32(np.nan), np.float32(0.5) * (rlo + rhi))
    assert _identical(med, R.cell_medians(org, imp))   # np.median of a float32 row IS 0.5f * (lo + hi)
    lohi = [np.nan, np.nan] if np.isnan(d).any() else [lo[0], hi[0]]
    got = imputation_scores_from_cells(med, R.cell_changed(org, crt), lohi)
    want = R.scores(org, crt, imp)
  for k in want:
    assert _identical(np.float64(got[k]), np.float64(want[k])), (k, got[k], want[k])
    assert isinstance(got[k], float)
  for k in ("med", "mean", "std"):
    assert _identical(np.float64(got[f"imputation_{k}"]), np.float64(FIX[f"{case}/{k}"])), k


def test_gene_indices():
  from sisua_amd.engine import gene_indices
  assert gene_indices([3, 0, 3], 4).tolist() == [3, 0, 3] and gene_indices(np.array([1]), 2).dtype == np.int32
  for bad in ([0, 4], [-1], []):
    with pytest.raises((IndexError, ValueError)):
      gene_indices(bad, 4)
  with pytest.raises(ValueError):
    gene_indices([0.5], 4)
  with pytest.raises(ValueError):
    gene_indices([[0, 1]], 4)


# ---- the metric classes against a stand-in model -----------------------------------------------------------------------------------
class _Handle:
  is_zero_inflated = False

  def __init__(self, x, mean):
    self.x, self.mean = x, mean

  def imputation_scores(self, original):
    return R.scores(np.asarray(original, np.float32), self.x, self.mean)

  def mean_over_samples(self, genes=None):
    return self.mean if genes is None else self.mean[:, list(genes)]


class _Model:
  def __init__(self, mean):
    self.mean, self.calls = mean, []

  def _imputation_handle(self, corrupted, library, sample_shape, batch_size):
    self.calls.append((sample_shape, batch_size))
    return _Handle(np.asarray(corrupted, np.float32), self.mean)


def test_imputation_error_metric():
  from sisua_amd.data import corrupt
  from sisua_amd.metrics import ImputationError
  org, crt, imp = (FIX[f"even/{k}"] for k in ("original", "corrupted", "imputed"))
  model = _Model(imp)
  got = ImputationError(org, corrupted=crt, sample_shape=2, batch_size=16)(model)
  want = R.scores(org, crt, imp)
  assert got == {"imp_med": want["imputation_med"], "imp_mean": want["imputation_mean"]} and model.calls == [(2, 16)]
  auto = ImputationError(org)   # corrupted=None: data.corrupt's defaults
  assert np.array_equal(auto.corrupted, corrupt(org, inplace=False)) and np.array_equal(auto.original, org)
  with pytest.raises(ValueError):
    ImputationError(org, corrupted=crt[:-1])


def test_correlation_scores_metric():
  from scipy.stats import pearsonr, spearmanr
  from sisua_amd.metrics import CorrelationScores, marker_pairs
  org, imp = FIX["wide/original"], FIX["wide/imputed"]
  rng = np.random.default_rng(2)
  prot = rng.gamma(2.0, 1.0, size=(org.shape[0], 3))
  genes = [f"g{i}" for i in range(org.shape[1])]
  pairs = marker_pairs(genes, ["CD3", "CD4", "CD99"], {"CD3": "g17", "CD4": "g2", "CD8": "g5", "CD99": "not there"})
  assert pairs == [(17, 0), (2, 1)]
  got = CorrelationScores(org, prot, pairs)(_Model(imp))
  pe = [-pearsonr(imp[:, g], prot[:, p])[0] for g, p in pairs]
  spm = [-spearmanr(imp[:, g], prot[:, p]).correlation for g, p in pairs]
  assert got == {"pearson_mean": float(np.mean(pe)), "spearman_mean": float(np.mean(spm)), "pearson_med": float(np.median(pe)),
                 "spearman_med": float(np.median(spm))}
  assert CorrelationScores(org, prot, [])(_Model(imp)) == {}
  with pytest.raises(IndexError):
    CorrelationScores(org, prot, [(org.shape[1], 0)])
  with pytest.raises(ValueError):
    CorrelationScores(org, prot[:-1], pairs)


def test_abi_declares_and_binds_the_new_symbols():
  from sisua_amd import _hip
  hdr = open(os.path.join(ROOT, "include", "sisua_hip.h")).read()
  for name in ("smx_predict_impute", "smx_predict_stat_cols", "smx_k_row_select",
               "smx_pad_audit", "smx_pad_poke"):
    assert name + "(" in hdr and name in _hip.SIGNATURES
  assert _hip.SMX_ABI_VERSION >= 6 and "smx_impute.hip" in __import__("sisua_amd.build", fromlist=["SOURCES"]).SOURCES


def test_lazy_handle_checks_before_any_device_work():
  """shape and index errors come from the host, with no engine"""
  from sisua_amd.distributions import LazyCountOutput

  class M:
    step, _param_version = 0, 0

    class _cfg:
      likelihood, n_genes = "nb", 5

    def _ensure_engine(self, b):
      raise AssertionError("no device work expected")
  lz = LazyCountOutput(M(), np.zeros((4, 5), np.float32), None, 0, 2, "x")
  for bad in (np.zeros((4, 4)), np.zeros((3, 5)), None):
    with pytest.raises(ValueError):
      lz.imputation_scores(bad)
