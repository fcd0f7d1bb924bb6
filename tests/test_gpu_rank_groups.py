"""Ranking genes between groups on the device (smx_rankgroups.hip) against the restatement (tests/rank_groups_ref.py): every integer of
the rank sums equal, the moments within a bound derived from the lengths of the sums, the same bits for every way of cutting the work,
and the package's result on a planted data set."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy import stats

import sisua_amd
from sisua_amd import engine, rank_groups
from sisua_amd.data import SingleCellOMIC
from tests import rank_groups_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53

# ---- rank sums --------------------------------------------------------------------------------------------------------------------------
# (N, K, G', layout): every N of {2 K, 63, 64, 65, 255, 256, 257, 1000} (the tile and wave edges of the sort and of the tie-run scan), every K
# of {2, 3, 7, 64}, every G' of {1, 5, 33}.  'pairs': groups of exactly 2 cells beside one dominant group (N = 2 K: every group has 2).
RANK_CASES = [(4, 2, 5, "pairs"), (6, 3, 33, "pairs"), (14, 7, 1, "pairs"), (128, 64, 5, "pairs"), (63, 3, 5, "random"), (63, 64, 5, "random"),
              (64, 7, 33, "random"), (65, 2, 5, "random"), (255, 64, 5, "pairs"), (256, 3, 33, "random"), (257, 7, 5, "pairs"),
              (1000, 64, 33, "random"), (1000, 2, 1, "random"), (1000, 7, 5, "pairs")]
KINDS = 6


def make_labels(N, K, layout, rng):
  if layout == "pairs":
    lab = np.zeros(N, np.int64)
    lab[: 2 * (K - 1)] = np.repeat(np.arange(1, K), 2)
    return rng.permutation(lab)
  return rng.randint(0, K, size=N)


def make_column(kind, N, lab, rng):
  if kind == 0:   # smooth, with negatives
    return rng.normal(size=N)
  if kind == 1:   # Poisson counts: long tie runs
    return rng.poisson(1.5, size=N).astype(np.float64)
  if kind == 2:   # a grid with -0.0 among 0.0
    return rng.choice(np.array([-1.0, -0.0, 0.0, 0.5, 2.0]), size=N)
  if kind == 3:   # all equal
    return np.full(N, 3.25)
  if kind == 4:   # one group holds exactly the tied block; every other value is distinct, below and above it
    v = rng.permutation(N).astype(np.float64) - N // 2 + 0.25
    v[lab == lab[0]] = 1.0
    return v
  return np.round(np.exp(rng.normal(size=N)), 1)   # moderate ties


def rank_case(i):
  N, K, G, layout = RANK_CASES[i]
  rng = np.random.RandomState(100 + i)
  lab = make_labels(N, K, layout, rng)
  cols = np.stack([make_column((j + i) % KINDS, N, lab, rng) for j in range(G)]).astype(np.float32)
  return cols, lab, K


@pytest.mark.parametrize("i", range(len(RANK_CASES)), ids=["N%d-K%d-G%d-%s" % c for c in RANK_CASES])
def test_rank_sums_are_the_restatements_integers(i):
  cols, lab, K = rank_case(i)
  r2, tie = engine.k_group_ranksums(cols, lab, K)
  want_r2, want_tie = R.group_ranksums(cols, lab, K)
  assert r2.dtype == tie.dtype == np.int64 and np.array_equal(r2, want_r2) and np.array_equal(tie, want_tie)
  N = cols.shape[1]
  assert np.array_equal(r2.sum(axis=0), np.full(cols.shape[0], N * (N + 1)))   # (the doubled ranks of a column add up to N (N + 1))
  ref = int(lab[1])   # (a group that has cells)
  r2, tie = engine.k_group_ranksums(cols, lab, K, reference=ref)
  want_r2, want_tie = R.group_ranksums(cols, lab, K, reference=ref)
  assert np.array_equal(r2, want_r2) and np.array_equal(tie, want_tie)
  assert not r2[ref].any() and not tie[ref].any()


def test_rank_sums_do_not_depend_on_the_call_the_selection_or_the_order_of_cells():
  cols, lab, K = rank_case(11)
  a = engine.k_group_ranksums(cols, lab, K)
  b = engine.k_group_ranksums(cols, lab, K)
  assert all(np.array_equal(x, y) for x, y in zip(a, b))
  sel = np.array([31, 0, 7, 7, 20])
  part = engine.k_group_ranksums(cols[sel], lab, K)
  assert np.array_equal(part[0], a[0][:, sel]) and np.array_equal(part[1], a[1][sel])
  perm = np.random.RandomState(5).permutation(cols.shape[1])
  moved = engine.k_group_ranksums(np.ascontiguousarray(cols[:, perm]), lab[perm], K)
  assert all(np.array_equal(x, y) for x, y in zip(a, moved))
  ref = int(lab[0])
  a = engine.k_group_ranksums(cols, lab, K, reference=ref)
  moved = engine.k_group_ranksums(np.ascontiguousarray(cols[:, perm]), lab[perm], K, reference=ref)
  assert all(np.array_equal(x, y) for x, y in zip(a, moved))


# ---- moments ----------------------------------------------------------------------------------------------------------------------------
def moment_bounds(X, lab, K):
  """|device - restatement| for sum and css [K, G].  A group's sum has n terms added one after the other in float64: at most
  (n - 1) 2^-53 sum |x| from the exact sum, and the restatement's correctly rounded sum lies within 2^-53 |s| <= 2^-53 sum |x| of it.  The
  device's mean = sum / n is then off by dm <= bound / n + 2^-53 |mean|.  With d = x - mean (one rounding each, squared: 3 x 2^-53 d^2 per
  term on either side), n fused terms added one after the other, and the mean moved by dm:
  (n + 8) 2^-53 sum d^2 + 2 dm sum |d| + n dm^2."""
  X = np.asarray(X, np.float64)
  G = X.shape[1]
  bs, bc = np.zeros((K, G)), np.zeros((K, G))
  for k in range(K):
    v = X[lab == k]
    n = len(v)
    if not n:
      continue
    bs[k] = (n + 1) * U * np.abs(v).sum(axis=0)
    mean = v.sum(axis=0) / n
    dm = bs[k] / n + U * np.abs(mean)
    d = v - mean
    bc[k] = (n + 8) * U * np.square(d).sum(axis=0) + 2 * dm * np.abs(d).sum(axis=0) + n * dm * dm
  return bs, bc


MOMENT_CASES = [(4, 1, 2), (63, 65, 3), (64, 63, 7), (65, 64, 2), (129, 300, 3), (1000, 65, 7), (1000, 1, 64)]   # (N, G, K)


def moment_case(i):
  N, G, K = MOMENT_CASES[i]
  rng = np.random.RandomState(200 + i)
  lab = make_labels(N, K, "pairs" if i % 2 == 0 and N >= 2 * K else "random", rng)
  X = np.log1p(rng.poisson(np.exp(rng.normal(0.0, 1.0, size=G))[None, :] * (1.0 + (np.arange(G)[None, :] % K == lab[:, None])))).astype(np.float32)
  X[rng.uniform(size=N) < 0.1] = 0.0        # empty rows
  X[:, rng.uniform(size=G) < 0.1] = 0.0     # empty columns
  if G > 2:
    X[:, 2] = 0.7                           # a constant column
    X[::3, 1] *= -1.0                       # negatives
  return X, lab, K


@pytest.mark.parametrize("i", range(len(MOMENT_CASES)), ids=["N%d-G%d-K%d" % c for c in MOMENT_CASES])
def test_moments_are_the_restatements_and_the_same_bits_for_every_block_and_form(i):
  X, lab, K = moment_case(i)
  want = R.group_moments(X, lab, K)
  bs, bc = moment_bounds(X, lab, K)
  first = None
  for block_rows in (0, 64, 128):
    for form in (X, sp.csr_matrix(X)):
      got = engine.k_group_moments(form, lab, K, block_rows=block_rows)
      if first is None:
        first = got
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["nnz"], want["nnz"])
        es, ec = np.abs(got["sum"] - want["sum"]), np.abs(got["css"] - want["css"])
        print("sum: worst error / bound %.3g; css: %.3g" % (np.max(es / np.maximum(bs, 1e-300)), np.max(ec / np.maximum(bc, 1e-300))))
        assert np.all(es <= bs) and np.all(ec <= bc)
      else:
        for f in ("count", "sum", "css", "nnz"):
          assert got[f].tobytes() == first[f].tobytes(), (f, block_rows, sp.issparse(form))


def test_moments_do_not_depend_on_the_call_or_the_selection_and_move_within_the_bound_under_a_permutation():
  X, lab, K = moment_case(4)
  a, b = engine.k_group_moments(X, lab, K), engine.k_group_moments(X, lab, K)
  sel = np.array([299, 3, 3, 64, 0])
  part = engine.k_group_moments(np.ascontiguousarray(X[:, sel]), lab, K, block_rows=64)
  perm = np.random.RandomState(6).permutation(len(X))
  moved = engine.k_group_moments(X[perm], lab[perm], K)
  bs, bc = moment_bounds(X, lab, K)
  for f in ("count", "sum", "css", "nnz"):
    assert a[f].tobytes() == b[f].tobytes()
    if f != "count":
      assert part[f].tobytes() == np.ascontiguousarray(a[f][:, sel]).tobytes()
  assert np.array_equal(moved["count"], a["count"]) and np.array_equal(moved["nnz"], a["nnz"])
  assert np.all(np.abs(moved["sum"] - a["sum"]) <= 2 * bs) and np.all(np.abs(moved["css"] - a["css"]) <= 2 * bc)   # (each within the bound of the exact value)


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
SHIFT = 1.5   # with it the restatement ranks exactly the planted genes first, for all three methods (checked on the host: test below)


def planted():
  """300 x 40, 4 groups; genes 5 k .. 5 k + 4 are shifted up in group k"""
  rng = np.random.RandomState(7)
  lab = rng.permutation(np.arange(300) % 4)
  X = np.log1p(rng.poisson(2.0, size=(300, 40))).astype(np.float64)
  for k in range(4):
    X[np.ix_(lab == k, np.arange(5 * k, 5 * k + 5))] += SHIFT
  return X.astype(np.float32), lab


@pytest.fixture(scope="module")
def truth():
  X, lab = planted()
  return X, lab, {m: R.rank_genes_groups(X, lab, method=m, n_genes=5) for m in rank_groups.METHODS}


def t_bounds(X, lab, k, overestim):
  """(dt [G], p_lo, p_hi [G]) of group k against the rest: the moments' bounds carried through Welch's t.  With a = m1 - m2 and s2 = v1 / n1
  + v2 / n2: dt = da / sqrt(s2) + |t| (ds2 / (2 s2) + 3 x 2^-53); the rest's moments are formed from the groups' (every term's bound added,
  the K additions at 2^-53 each); the degrees of freedom move by at most 2 (dA + dB) / (A + B) + 2 max(dA / A, dB / B) + 8 x 2^-53 in
  relative terms, and p is monotone in |t| and in the degrees of freedom, so it lies between its values at the corners."""
  X = np.asarray(X, np.float64)
  N, K = len(X), int(lab.max()) + 1
  mom = R.group_moments(X, lab, K)
  bs, bc = moment_bounds(X, lab, K)
  cnt = mom["count"].astype(np.float64)
  mean = mom["sum"] / cnt[:, None]
  dmean = bs / cnt[:, None] + U * np.abs(mean)
  n1, n2 = cnt[k], N - cnt[k]
  v1, dv1 = mom["css"][k] / (n1 - 1), bc[k] / (n1 - 1) + U * mom["css"][k] / (n1 - 1)
  m2 = (mom["sum"].sum(axis=0) - mom["sum"][k]) / n2
  dm2 = (bs.sum(axis=0) + (K + 1) * U * np.abs(mom["sum"]).sum(axis=0)) / n2 + U * np.abs(m2)
  css2, dcss2 = np.zeros_like(m2), np.zeros_like(m2)
  for h in range(K):
    if h != k:
      gap, dgap = np.abs(mean[h] - m2), dmean[h] + dm2
      css2 += mom["css"][h] + cnt[h] * gap * gap
      dcss2 += bc[h] + cnt[h] * (2 * gap * dgap + dgap * dgap)
  dcss2 += (K + 4) * U * css2
  v2, dv2 = css2 / (n2 - 1), dcss2 / (n2 - 1) + U * css2 / (n2 - 1)
  nobs2 = n1 if overestim else n2
  a, da = mean[k] - m2, dmean[k] + dm2 + U * np.abs(mean[k] - m2)
  A, B, dA, dB = v1 / n1, v2 / nobs2, dv1 / n1, dv2 / nobs2
  s2, ds2 = A + B, dA + dB + 2 * U * (A + B)
  t = a / np.sqrt(s2)
  dt = da / np.sqrt(s2) + np.abs(t) * (ds2 / (2 * s2) + 3 * U)
  df = s2 * s2 / (A * A / (n1 - 1) + B * B / (nobs2 - 1))
  edf = 2 * (dA + dB) / s2 + 2 * np.maximum(dA / A, dB / B) + 8 * U
  corners = [2 * stats.t.sf(np.maximum(np.abs(t) + st * dt, 0.0), df * (1 + sd * edf)) for st in (-1, 1) for sd in (-1, 1)]
  return dt, np.min(corners, axis=0), np.max(corners, axis=0)


def test_the_planted_genes_are_what_the_restatement_ranks_first(truth):
  _, _, want = truth
  for m in rank_groups.METHODS:
    for k in range(4):
      assert sorted(int(n) for n in want[m][k]["names"]) == list(range(5 * k, 5 * k + 5)), (m, k)


@pytest.mark.parametrize("method", rank_groups.METHODS)
@pytest.mark.parametrize("sparse", [False, True])
def test_rank_genes_groups_on_the_planted_data(truth, method, sparse):
  X, lab, want = truth
  got = sisua_amd.rank_genes_groups(sp.csr_matrix(X) if sparse else X, lab, method=method, n_genes=5)
  again = sisua_amd.rank_genes_groups(X, lab, method=method, n_genes=5, gene_chunk=7)
  for k in range(4):
    w, f = want[method][k], str(k)
    assert list(got["names"][f]) == list(w["names"])
    for key in ("names", "scores", "pvals", "pvals_adj", "logfoldchanges"):
      assert got[key][f].tobytes() == again[key][f].tobytes()   # no bit depends on the gene chunk or on the form of the matrix
    if method == "wilcoxon":   # the integers are equal: only the closing formula's roundings differ; d ln p / dz = -z for large z
      z = np.abs(w["scores"])
      dz, p_lo, p_hi = 8 * U * z, w["pvals"] * (1 - 16 * U * (z * z + 1)), w["pvals"] * (1 + 16 * U * (z * z + 1))
    else:
      dz, p_lo, p_hi = (b[w["order"]] for b in t_bounds(X, lab, k, method == "t-test_overestim_var"))
    es = np.abs(got["scores"][f] - w["scores"])
    slack = 1e-13 * w["pvals"]   # (the relative accuracy taken for SciPy's incomplete beta function, evaluated at two nearby points)
    print(method, k, "score error / bound", np.max(es / dz), "p in [%s]" % ((got["pvals"][f] - p_lo) / np.maximum(p_hi - p_lo, 1e-300)))
    assert np.all(es <= dz)
    assert np.all(got["pvals"][f] >= p_lo - slack) and np.all(got["pvals"][f] <= p_hi + slack)


def test_rank_vars_groups_on_the_planted_data(truth):
  X, lab, want = truth
  sco = SingleCellOMIC(X, var_names=[f"g{i}" for i in range(40)])
  key = sco.rank_vars_groups(n_vars=5, group_by=lab, method="wilcoxon")
  res = sco.get_rank_vars_groups(key)
  for k in range(4):
    assert list(res["names"][str(k)]) == [f"g{i}" for i in want["wilcoxon"][k]["order"]]
