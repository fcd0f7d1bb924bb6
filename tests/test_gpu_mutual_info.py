"""The device's mutual-information estimators (smx_mi.hip) held to their restatement (tests/mutual_info_ref.py, itself held to
scikit-learn in tests/test_mutual_info_host.py): per cell through the kernel-level entry -- every integer equal, every radius the same
bits -- and as a matrix within a bound derived from the closing sums; the bits across calls, gene chunks, gene selections and input
forms; the invariance under a permutation of the cells; and the public surface."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.special import digamma

from tests import mutual_info_ref as R
from tests.util import synth_counts, synth_labels

pytestmark = pytest.mark.gpu

SIZES = [2, 5, 63, 64, 65, 255, 256, 257, 1000]   # tile and wave edges of the sort, the sweep (tiles of 128 and 256) and the reductions
CAP = 8


@pytest.fixture(scope="module")
def eng():
  from sisua_amd import build
  build.build(verbose=False)
  from sisua_amd import engine
  assert engine.MI_MAX_NEIGHBORS == CAP
  return engine


def bound(N):
  """Four fixed-order sums of N table entries of magnitude at most psi(N), each entry exact: 4 N 2^-53 psi(N) absolute"""
  return 4 * N * 2.0 ** -53 * max(float(digamma(N)), 1.0)


def ks(N):
  return [k for k in (1, 3, CAP) if k < N]


def continuous(N, seed):
  """name -> (x, y): smooth with negative values; exact ties on a grid without noise, -0.0 among them; an all-equal column;
  duplicated cells"""
  rng = np.random.RandomState(seed)
  x = rng.standard_normal(N)
  y = 0.6 * x + rng.standard_normal(N)
  gx, gy = np.floor(x * 2) / 2, np.floor(y * 2) / 2
  gx[gx == 0.0] = -0.0
  dup = rng.randint(0, max(1, N // 3), N)
  return {"smooth": (x, y), "ties": (gx, gy), "equal": (np.full(N, -1.25), y), "both_equal": (np.zeros(N), np.full(N, 3.0)),
          "duplicates": (x[dup], y[dup])}


def labels(N, k, seed):
  """name -> d: one dominant label plus singletons, a group of exactly k + 1 and a group of 2 (where N allows), -0.0 and 0.0 as one
  label, negative labels; all unique; a single label"""
  rng = np.random.RandomState(seed)
  d = np.zeros(N)
  d[rng.uniform(size=N) < 0.5] = -0.0
  at = 0
  for size, lab in ((k + 1, -3.0), (2, 5.0), (1, 7.0), (1, 8.0), (1, -9.5)):
    if at + size < N:
      d[at:at + size] = lab
      at += size
  d = d[rng.permutation(N)]
  return {"dominant": d, "unique": np.arange(N, dtype=np.float64) - 3.0, "single": np.full(N, 2.0),
          "few": rng.randint(-1, 3, N).astype(np.float64)}


def same_bits(a, b):
  a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
  return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


# ---- 1. per cell ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_cc_cells(eng, N):
  for k in ks(N):
    for name, (x, y) in continuous(N, 10 + N).items():
      got = eng.k_mi_cells(x, False, y, False, k)
      r, nx, ny = R.mi_cc_cells(x, y, k)
      assert same_bits(got["r"], r), (N, k, name)
      assert np.array_equal(got["nx"], nx) and np.array_equal(got["ny"], ny), (N, k, name)
      assert abs(got["mi"] - R.mi_cc_from_cells(nx, ny, k)) <= bound(N), (N, k, name)


@pytest.mark.parametrize("N", SIZES)
def test_cd_cells(eng, N):
  for k in ks(N):
    cols, lab = continuous(N, 20 + N), labels(N, k, 30 + N)
    for cname, dname in (("smooth", "dominant"), ("ties", "dominant"), ("duplicates", "few"), ("smooth", "unique"), ("ties", "single"),
                         ("both_equal", "few")):
      c, d = cols[cname][0], lab[dname]
      kept, ki, count, m, r = R.mi_cd_cells(c, d, k)
      for flip in (False, True):   # (the discrete column as the protein, and as the gene)
        got = eng.k_mi_cells(d, True, c, False, k) if flip else eng.k_mi_cells(c, False, d, True, k)
        where = (N, k, cname, dname, flip)
        assert np.array_equal(got["kept"], kept) and np.array_equal(got["k"], ki) and np.array_equal(got["count"], count), where
        assert np.array_equal(got["m"], m) and same_bits(got["r"], r), where
        assert abs(got["mi"] - R.mi_cd_from_cells(kept, ki, count, m)) <= bound(N), where


@pytest.mark.parametrize("N", SIZES)
def test_dd_triples(eng, N):
  lab = labels(N, 3, 40 + N)
  for an, bn in (("dominant", "few"), ("few", "few"), ("unique", "few"), ("single", "dominant"), ("unique", "unique"), ("few", "single")):
    a, b = lab[an], lab[bn][::-1].copy()
    got = eng.k_mi_cells(a, True, b, True, 1)
    va, vb, n = R.mi_dd_triples(a, b)
    assert np.array_equal(got["a"], va) and np.array_equal(got["b"], vb) and np.array_equal(got["n_ab"], n), (N, an, bn)
    # R runs: every term is formed from the same table entries in the same way; only the order of the sum differs: R 2^-52 log N
    assert abs(got["mi"] - R.mi_dd(a, b)) <= len(n) * 2.0 ** -52 * np.log(N), (N, an, bn)


# ---- 2. the matrix -------------------------------------------------------------------------------------------------------------------
def mixed_columns(N, seed=3):
  """G = 7 genes and P = 4 proteins of mixed kind, prepared columns (gene-major): all four branches in one call"""
  rng = np.random.RandomState(seed)
  x = rng.standard_normal((7, N))
  x[1] = rng.poisson(1.5, N)
  x[3] = np.floor(x[0] * 2) / 2
  x[4] = rng.randint(0, 4, N)
  x[6] = x[1] + rng.randint(0, 2, N)
  xd = np.array([0, 1, 0, 0, 1, 0, 1], bool)
  y = np.stack([0.5 * x[0] + rng.standard_normal(N), x[4] + (rng.uniform(size=N) < 0.2), np.exp(x[2]), rng.randint(0, 2, N) - 1.0])
  return x, xd, y, np.array([0, 1, 0, 1], bool)


@pytest.mark.parametrize("N", [64, 257, 1000])
def test_matrix_within_the_bound(eng, N):
  x, xd, y, yd = mixed_columns(N)
  for k in (1, 3):
    got = eng.mutual_info(x, xd, y, yd, k)
    assert got.shape == (7, 4) and (got >= 0).all()
    for g in range(7):
      for p in range(4):
        want = R.mi_pair(x[g], y[p], xd[g], yd[p], k)
        tol = len(R.mi_dd_triples(x[g], y[p])[2]) * 2.0 ** -52 * np.log(N) if xd[g] and yd[p] else bound(N)
        assert abs(got[g, p] - want) <= tol, (N, k, g, p, got[g, p], want)
    assert (got[:, [0, 2]] > 0).any() and (got[[1, 4, 6]][:, [1, 3]] > 0).any()   # (not a matrix of clipped zeros)


def test_same_bits_across_calls_chunks_selections_and_forms(eng):
  from sisua_amd import mutual_information
  N = 257
  x, xd, y, yd = mixed_columns(N)
  first = eng.mutual_info(x, xd, y, yd, 3)
  assert same_bits(first, eng.mutual_info(x, xd, y, yd, 3))
  for chunk in (1, 3, 7):
    assert same_bits(first, eng.mutual_info(x, xd, y, yd, 3, gene_chunk=chunk)), chunk
  X, Y = x.T.copy(), y.T.copy()
  full = mutual_information(X, Y, discrete_features=xd, discrete_targets=yd)
  assert same_bits(full, mutual_information(sp.csr_matrix(X), Y, discrete_features=xd, discrete_targets=yd))
  assert same_bits(full, mutual_information(X, Y, discrete_features=xd, discrete_targets=yd, gene_chunk=2))
  sel = [5, 0, 0, 6, 1]
  picked = mutual_information(X, Y, discrete_features=xd, discrete_targets=yd, genes=sel)
  assert same_bits(picked, mutual_information(X[:, sel], Y, discrete_features=xd[sel], discrete_targets=yd))
  assert same_bits(picked, mutual_information(sp.csc_matrix(X), Y, discrete_features=xd, discrete_targets=yd, genes=sel, gene_chunk=1))
  # without the noise the matrix is a pure function of the data: the rows of a selection are the rows of the whole
  pure = mutual_information(X, Y, discrete_features=xd, discrete_targets=yd, noise=False)
  assert same_bits(pure[sel], mutual_information(X, Y, discrete_features=xd, discrete_targets=yd, noise=False, genes=sel))
  assert same_bits(pure[sel][1], pure[sel][2])


def test_permutation_of_the_cells(eng):
  N, k = 257, 3
  x, xd, y, yd = mixed_columns(N)
  perm = np.random.RandomState(9).permutation(N)
  a, b = eng.mutual_info(x, xd, y, yd, k), eng.mutual_info(x[:, perm], xd, y[:, perm], yd, k)
  for g in range(7):
    for p in range(4):
      tol = len(R.mi_dd_triples(x[g], y[p])[2]) * 2.0 ** -52 * np.log(N) if xd[g] and yd[p] else bound(N)
      assert abs(a[g, p] - b[g, p]) <= tol, (g, p)
  for g, p in ((0, 0), (3, 2), (0, 1), (4, 0), (1, 3)):
    u = eng.k_mi_cells(x[g], xd[g], y[p], yd[p], k)
    v = eng.k_mi_cells(x[g][perm], xd[g], y[p][perm], yd[p], k)
    for key in u:
      if key == "mi":
        continue
      if key in ("a", "b", "n_ab"):   # (the sorted triples do not move at all)
        assert np.array_equal(u[key], v[key]), (g, p, key)
      else:   # the cells' values move with the cells
        assert np.array_equal(np.asarray(u[key])[perm], v[key]), (g, p, key)


# ---- 3. the public surface -------------------------------------------------------------------------------------------------------------
def test_mutual_information_is_sklearn(eng):
  from sklearn.feature_selection import mutual_info_classif, mutual_info_regression
  from sisua_amd import mutual_information
  X, mask, y, yd = R.mixed_problem()   # 300 x 6, small label groups folded: scikit-learn's distances differ there
  Y = np.stack([y, yd, np.exp(0.3 * y)], axis=1)
  got = mutual_information(X, Y, n_neighbors=3)   # 'auto' finds the two discrete genes and the discrete protein
  assert got.shape == (6, 3)
  for p, disc in enumerate((False, True, False)):
    fn = mutual_info_classif if disc else mutual_info_regression
    want = fn(X, Y[:, p], discrete_features=mask, n_neighbors=3, random_state=1)
    assert np.abs(got[:, p] - want).max() <= 1e-12, p
  assert same_bits(got, mutual_information(X, Y, discrete_features=mask, discrete_targets=np.array([False, True, False])))
  with pytest.raises(ValueError, match="below the number of cells"):
    eng.mutual_info(np.zeros((1, 4)), [False], np.zeros((1, 4)), [False], 4)
  with pytest.raises(ValueError, match="gene column 1"):
    eng.mutual_info(np.array([[0.0, 1, 2, 3], [0, np.nan, 2, 3]]), [False, True], np.zeros((1, 4)), [False], 1)


def test_single_cell_omic_and_marker_scores(eng):
  from sisua_amd import marker_scores, mutual_information
  from sisua_amd.data import SingleCellOMIC
  n = 200
  x = synth_counts(n, 12, sparsity=0.6, seed=3)
  prot = synth_labels(n, ((3, "nb"),))[0]
  sco = SingleCellOMIC(sp.csr_matrix(x), name="toy")
  sco.add_omic("proteomic", np.log1p(prot) + 0.25)
  mi = sco.get_mutual_information()
  assert mi.shape == (12, 3) and mi.dtype == np.float64
  assert same_bits(mi, mutual_information(sco.numpy("transcriptomic"), sco.numpy("proteomic"), n_neighbors=3, random_state=1))
  assert sco.get_mutual_information(random_state=5) is mi   # the reference's cache, and its fixed seed
  assert sco.get_mutual_information("proteomic", "transcriptomic").shape == (3, 12)   # (its own key)
  with pytest.raises(AssertionError):
    sco.get_mutual_information("proteomic", "proteomic")
  sco.add_omic("proteomic", prot)   # replacing an omic drops the matrices made of it
  assert sco.get_mutual_information() is not mi
  genes, prots = [f"g{i}" for i in range(12)], ["a", "b", "c"]
  assert marker_scores(mi, "mi", genes, prots, {"a": "g3", "c": "g0", "z": "g1"}) == {"mi_g3_a": float(mi[3, 0]), "mi_g0_c": float(mi[0, 2])}


def test_model_mutual_information(eng):
  import sisua_amd.models as M
  from sisua_amd import metrics, mutual_information
  from sisua_amd.data import SingleCellOMIC
  n, g = 200, 40
  x = synth_counts(n, g, sparsity=0.8, seed=3)
  extras = synth_labels(n, ((3, "nb"),))[0].astype(np.float64)
  sco = SingleCellOMIC(x, name="toy")
  m = M.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), latents=M.RVmeta(8, "diag", True, "Latents"),
            encoder=M.NetConf([32], batchnorm=True, dropout=0.1), decoder=M.NetConf([32], batchnorm=True, dropout=0.1))
  m.fit(sco.create_dataset(["transcriptomic"], batch_size=64, drop_remainder=True), metadata=sco, epochs=2, learning_rate=2e-3)
  got = m.mutual_information(x, extras, sample_shape=2, batch_size=64)
  h = m._imputation_handle(x, None, 2, 64)
  assert h.is_zero_inflated
  cols = h.count_distribution.mean_over_samples()   # on a zero-inflated output: the count distribution's mean, as `correlation` takes it
  assert got.shape == (g, 3) and same_bits(got, mutual_information(cols, extras, n_neighbors=3, random_state=1))
  sel = [7, 0, 7, 39]
  lazy = h.mutual_information(extras, genes=sel)
  assert same_bits(lazy, mutual_information(cols[:, sel], extras)) and same_bits(lazy, m.mutual_information(x, extras, sample_shape=2, batch_size=64, genes=sel))
  pairs = [(7, 0), (39, 2)]
  score = metrics.MutualInformation(x, extras, pairs, sample_shape=2, batch_size=64)(m)
  mat = m.mutual_information(x, extras, sample_shape=2, batch_size=64, genes=[7, 39])
  vals = [-mat[0, 0], -mat[1, 2]]
  assert score == {"mi_mean": float(np.mean(vals)), "mi_med": float(np.median(vals))}
