"""The UMAP layout on the device (smx_umap.hip through engine.k_umap_layout, sisua_amd/neighbors.py and SingleCellOMIC.umap) against the
float64 restatement tests/umap_ref.py.

Shapes are the smallest at which the kernel can still go wrong: cells around the sixteen cells of a workgroup and the four of a wave,
more than one workgroup, rows shorter and longer than one chunk of 16 entries, hubs of 64 and 65 entries (the edge between sixteen lanes and a
workgroup per row), of 300 and of 600 (more than two chunks of 256), an empty row, cells on top of each other.

Bounds.
  one epoch    next_sample and next_negative EQUAL (bits): the schedule is decided on rounded float64 operations that both sides spell
               alike.  Y per cell j and component c:
                   |dY_jc| <= (2 T_j + 12 + POW_ALLOWED) 2^-53 alpha A_jc  +  2 x 2^-53 |Y_jc|
               A_jc = the sum of the cell's |term|, T_j the number of its terms.  Device and restatement differ in pow and in the order
               of the sum alone.  A term is c / (..) with pow entering once above or below the line with |d ln g / d ln pb| <= 1: its
               relative difference is at most pow's, plus the six roundings behind the pow on either side (12).  Either side's sum
               is within (T - 1) 2^-53 A of the exact sum of its own terms (2 T - 2), alpha x sum rounds once on either side (2).
               The last term is the rounding of y + alpha x sum itself, at the magnitude of y, on either side: it is what the
               number format leaves of ANY difference in the sum, and without it a cell at |y| = 50 whose terms are 1e-6 could not
               pass however exact the sum.
               POW_SEEN: the largest relative difference between the device's pow (engine.k_umap_pow) and numpy.power on the
               arguments of exactly these cases, in units of 2^-53; POW_ALLOWED is twice that.  test_device_pow holds the device to it.
  trajectory   the dynamics amplify rounding, so the tolerance is a measurement: the restatement run with each cell's terms added in three
               orders (attraction first then negatives, the reverse, a random permutation) on exactly these inputs differs, relative
               to max |Y|, by SPREAD:   n = 60: 0 after 1 epoch, 7.7e-10 after 10        n = 300: 0 after 1, 8.9e-9 after 10.
               Nothing is active in epoch 0 (next_sample starts at e >= 1), so after one epoch Y is the start, exactly, on both sides;
               after ten a pair of cells that a negative sample found 0.03 apart has had its last bits multiplied by
               2 b / 0.001 ~ 2700 per epoch.  The tolerance is 100 x SPREAD.  The schedule state is EQUAL.
  whole run    judged by what it is for: finite, every cell's nearest neighbour in the embedding in its own group, and a trustworthiness
               (12 neighbours) no more than 0.02 below that of the restatement's per-epoch run from the same start."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from sisua_amd import _hip, engine, neighbors
from sisua_amd.data import SingleCellOMIC
from tests import neighbors_ref as NR
from tests import umap_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
A_B = (0.5830300203414425, 1.3341669924314914)   # find_ab_params(1, 0.5)
ONE_N = [2, 15, 16, 17, 255, 256, 257, 600]
ONE_GRAPHS = [("blob", n, 5) for n in ONE_N] + [("blob", n, 12) for n in ONE_N if n >= 15] + [("star", 320, 300), ("star", 320, 64), ("star", 320, 65), ("star", 700, 600), ("empty", 257, 5), ("dup", 257, 12)]
ONE_EPOCHS = [10, 200]
ONE_SCALE = [1e-4, 1.0, 50.0]
POW_SEEN = 2.0                 # measured on the device, units of 2^-53
POW_ALLOWED = 2.0 * POW_SEEN
SPREAD = {(60, 1): 0.0, (60, 10): 7.7e-10, (300, 1): 0.0, (300, 10): 8.9e-9}   # the restatement's order-to-order spread (CPU)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _knn_graph(X, K):
  """the fuzzy graph of the cells X with K neighbours (the cell itself among them), on the host"""
  idx, dist, _ = NR.knn(X, K - 1)
  tab = neighbors.self_table(idx, dist)
  return neighbors.assemble_graph(tab[0], tab[1], NR.umap_rows(*tab)[2])[0]


@functools.lru_cache(maxsize=None)
def _graph(kind, n, K):
  """a symmetric weighted graph over n cells (scipy CSR), never written to"""
  if kind == "star":   # the hub 0 holds K entries, the other cells a ring.  A row of more than 64 entries is a workgroup's: 64 and 65 are the edge
    rng = np.random.default_rng(5)
    leaves = np.arange(1, K + 1)
    rest = np.arange(K + 1, n)
    r = np.concatenate([np.zeros(K, np.int64), rest])
    c = np.concatenate([leaves, np.roll(rest, 1)])
    low = 0.004 if K == 300 else 0.2   # (K = 300: some of the hub's entries fall to the cut, at 200 epochs too; the others keep every entry)
    w = np.concatenate([rng.uniform(low, 1.0, K), rng.uniform(0.2, 1.0, rest.size)])
    G = sp.coo_matrix((w, (r, c)), shape=(n, n)).tocsr()
    return (G + G.T).tocsr()
  X = R.blobs((n + 2) // 3, sep=4.25, seed=n)[:n].copy()
  if kind == "dup":
    X[1:21] = X[0]
  G = _knn_graph(X, min(K, n)).astype(np.float64).tolil()
  if kind == "empty":   # every weight of cell 3 below max / 200 (and max / 10): the cut leaves its row empty
    for k in G.rows[3]:
      G[3, k] = G[k, 3] = 1e-4
  return G.tocsr()


@functools.lru_cache(maxsize=None)
def _prepared(kind, n, K, n_epochs):
  return R.prepare(_graph(kind, n, K), n_epochs)


@functools.lru_cache(maxsize=None)
def _state(kind, n, K, n_epochs, at):
  """the restatement's schedule state at the start of epoch `at`"""
  return R.state_at(_prepared(kind, n, K, n_epochs).data, 5, n_epochs, at)


def _start(kind, n, C, scale, seed):
  Y = np.random.default_rng(seed).standard_normal((n, C)) * scale
  if kind == "dup":
    Y[1:21] = Y[0]   # cells on top of each other: d2 == 0 in the attraction and in the negatives that hit them
  return Y


# ---- one epoch, elementwise ------------------------------------------------------------------------------------------------------------
POW_ARGS = []   # the arguments of every pow the one-epoch cases took, for test_device_pow


@pytest.mark.parametrize("n_epochs", ONE_EPOCHS)
@pytest.mark.parametrize("kind,n,K", ONE_GRAPHS)
def test_one_epoch_against_restatement(kind, n, K, n_epochs):
  E = _prepared(kind, n, K, n_epochs)
  a, b = A_B
  if kind == "empty":
    assert E.indptr[4] == E.indptr[3]
  if kind == "star":
    assert E.indptr[1] - E.indptr[0] >= 250 if K == 300 else E.indptr[1] - E.indptr[0] == K
  worst, most_m = 0.0, 0
  for at in (0, 1, 7, n_epochs - 1):
    nxt0, neg0 = _state(kind, n, K, n_epochs, at)
    for C in (1, 2, 3):
      for scale in ONE_SCALE:
        Y = _start(kind, n, C, scale, 1000 * at + 10 * C + n)
        nxt, neg = nxt0.copy(), neg0.copy()
        want, A, T, m, args = R.epoch(E, Y, at, n_epochs, a, b, 1.0, 1.0, 5, 9, nxt, neg, detail=True)
        got = engine.k_umap_layout(E, Y, n_epochs, a, b, 1.0, 1.0, 5, 9, epoch_begin=at, epoch_end=at + 1, next_sample=nxt0, next_negative=neg0)
        assert got["Y"].shape == (n, C) and got["Y"].dtype == np.float64
        assert _same_bits(got["next_sample"], nxt) and _same_bits(got["next_negative"], neg), (at, C, scale)
        alpha = 1.0 * (1.0 - at / n_epochs)
        bound = (2.0 * T[:, None] + 12.0 + POW_ALLOWED) * U * alpha * A + 2.0 * U * np.abs(want)
        err = np.abs(got["Y"] - want)
        with np.errstate(invalid="ignore", divide="ignore"):
          frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        worst, most_m = max(worst, float(frac.max())), max(most_m, int(m.max(initial=0)))
        assert frac.max() <= 1.0, (at, C, scale, float(frac.max()))
        if kind == "empty":
          assert _same_bits(got["Y"][3], Y[3])   # an empty row never moves
        if C == 2 and len(POW_ARGS) < 400:
          POW_ARGS.append(args)
  if n <= 17 or kind != "blob":   # a stale next_negative: the entries active in the last epoch draw hundreds of negatives each (the star's: the clamp S x n_epochs)
    at = n_epochs - 1
    nxt0, _ = _state(kind, n, K, n_epochs, at)
    neg0 = np.full(E.nnz, -1e30) if kind == "star" else R.start_state(E.data, 5)[1]
    Y = _start(kind, n, 2, 1.0, n)
    nxt, neg = nxt0.copy(), neg0.copy()
    want, A, T, m, args = R.epoch(E, Y, at, n_epochs, a, b, 1.0, 1.0, 5, 9, nxt, neg, detail=True)
    got = engine.k_umap_layout(E, Y, n_epochs, a, b, 1.0, 1.0, 5, 9, epoch_begin=at, epoch_end=at + 1, next_sample=nxt0, next_negative=neg0)
    assert _same_bits(got["next_sample"], nxt) and _same_bits(got["next_negative"], neg)
    bound = (2.0 * T[:, None] + 12.0 + POW_ALLOWED) * U * (1.0 - at / n_epochs) * A + 2.0 * U * np.abs(want)
    frac = np.abs(got["Y"] - want) / bound
    worst, most_m = max(worst, float(frac.max())), max(most_m, int(m.max(initial=0)))
    assert frac.max() <= 1.0, ("stale", float(frac.max()))
    assert m.max() == 5 * n_epochs if kind == "star" else m.max() >= 4 * (n_epochs - 1)
  print(kind, n, K, n_epochs, "entries", E.nnz, "largest m", most_m, "largest err / bound", worst)


def test_device_pow():
  """the device's pow against numpy's on the arguments the one-epoch cases produce (run after them; alone it takes a case of its own)"""
  if not POW_ARGS:
    E = _prepared("blob", 257, 12, 200)
    for scale in ONE_SCALE:
      nxt, neg = _state("blob", 257, 12, 200, 7)
      POW_ARGS.append(R.epoch(E, _start("blob", 257, 2, scale, 1), 7, 200, *A_B, 1.0, 1.0, 5, 9, nxt.copy(), neg.copy(), detail=True)[4])
  x = np.unique(np.concatenate(POW_ARGS))
  want = np.power(x, A_B[1])
  ok = np.isfinite(want) & (want > 0)   # (a d2 whose power underflows has no relative error to speak of)
  got = engine.k_umap_pow(x, A_B[1])
  rel = np.abs(got[ok] - want[ok]) / want[ok] / U
  print("pow: arguments", x.size, "from", float(x.min()), "to", float(x.max()), "largest relative difference in 2^-53:", float(rel.max()))
  assert rel.max() <= POW_ALLOWED


def test_c_abi_refuses_before_device_work():
  lib = _hip.require_gpu()
  E = _prepared("blob", 16, 5, 10)
  indptr, cols, eps, y = engine._umap_problem(E, np.zeros((16, 2)))
  nxt, neg = R.start_state(eps, 5)
  out = np.empty_like(y)

  def call(n_cells=16, C=2, n_epochs=10, begin=0, end=10, a=1.0, S=5, cols_=cols, eps_=eps):
    return lib.smx_umap_layout(engine._ptr(indptr), engine._ip(cols_), engine._dp(eps_), n_cells, C, engine._dp(y), n_epochs, begin, end, a, 1.0, 1.0,
                               1.0, S, 0, engine._dp(nxt), engine._dp(neg), engine._dp(out))

  assert call() == 0
  bad_col, bad_eps = cols.copy(), eps.copy()
  bad_col[0], bad_eps[1] = 0, np.nan   # (row 0: an entry on the diagonal)
  for kw in (dict(C=4), dict(C=0), dict(n_epochs=0), dict(n_epochs=10001, end=10), dict(begin=3, end=2), dict(end=11), dict(a=-1.0), dict(a=np.nan),
             dict(S=65), dict(S=-1), dict(cols_=bad_col), dict(eps_=bad_eps), dict(n_cells=1)):
    assert call(**kw) == -1, kw


# ---- a short trajectory ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epochs", [1, 10])
@pytest.mark.parametrize("n", [60, 300])
def test_short_trajectory(n, epochs):
  E = _prepared("blob", n, 12, 200)
  Y0 = R.normalise(np.random.RandomState(1).uniform(-10, 10, (n, 2)))
  want = R.layout(E, Y0, 200, *A_B, seed=3, end=epochs)
  got = engine.k_umap_layout(E, Y0, 200, *A_B, seed=3, epoch_end=epochs)
  tol = 100.0 * SPREAD[(n, epochs)]
  err = np.abs(got["Y"] - want["Y"]).max() / np.abs(want["Y"]).max()
  print(n, epochs, "err", float(err), "tolerance", tol)
  assert err <= tol
  assert _same_bits(got["next_sample"], want["next_sample"]) and _same_bits(got["next_negative"], want["next_negative"])


# ---- pieces equal the whole --------------------------------------------------------------------------------------------------------------------
def test_pieces_equal_the_whole_and_two_calls_agree():
  E = _prepared("blob", 300, 12, 200)
  Y0 = R.normalise(np.random.RandomState(2).uniform(-10, 10, (300, 3)))
  whole = engine.k_umap_layout(E, Y0, 200, *A_B, seed=5)
  again = engine.k_umap_layout(E, Y0, 200, *A_B, seed=5)
  assert np.isfinite(whole["Y"]).all()
  for q in ("Y", "next_sample", "next_negative"):
    assert _same_bits(whole[q], again[q]), q
  for s in (1, 77, 199):
    first = engine.k_umap_layout(E, Y0, 200, *A_B, seed=5, epoch_end=s)
    rest = engine.k_umap_layout(E, first["Y"], 200, *A_B, seed=5, epoch_begin=s, next_sample=first["next_sample"],
                                next_negative=first["next_negative"])
    for q in ("Y", "next_sample", "next_negative"):
      assert _same_bits(whole[q], rest[q]), (s, q)
  other = engine.k_umap_layout(E, Y0, 200, *A_B, seed=6)
  assert not _same_bits(other["Y"], whole["Y"]) and _same_bits(other["next_sample"], whole["next_sample"])   # the seed moves the draws alone


# ---- a whole run -----------------------------------------------------------------------------------------------------------------------------------
def test_whole_run_embeds_the_groups():
  skm = pytest.importorskip("sklearn.manifold")
  X = R.blobs(100, sep=4.25)
  group = np.arange(300) % 3
  model = neighbors.UMAP(n_neighbors=12, n_epochs=200, init="pca", random_state=1)
  Y = model.fit_transform(X)
  assert Y is model.embedding_ and Y.shape == (300, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
  assert model.n_epochs_ == 200 and abs(model.a_ - A_B[0]) < 1e-3 and abs(model.b_ - A_B[1]) < 1e-3
  assert sp.issparse(model.graph_) and model.graph_.shape == (300, 300)
  assert R.nearest_in_group(Y, group)
  Y0 = R.normalise(neighbors.pca(X, 2)[1])
  ref = R.layout(R.prepare(model.graph_, 200), Y0, 200, model.a_, model.b_, seed=1)["Y"]
  mine, theirs = skm.trustworthiness(X, Y, n_neighbors=12), skm.trustworthiness(X, ref, n_neighbors=12)
  print("trustworthiness: device", mine, "restatement", theirs)
  assert mine >= theirs - 0.02
  assert _same_bits(neighbors.umap(X, n_neighbors=12, n_epochs=200), Y)
  Y3 = neighbors.umap(X, n_neighbors=12, n_components=3, n_epochs=30, init="random", random_state=4)
  assert Y3.shape == (300, 3) and np.isfinite(Y3).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
def test_singlecell_umap_end_to_end():
  rng = np.random.default_rng(11)
  counts = rng.poisson(rng.gamma(0.6, 2.0, size=(1, 300)) * (1.0 + (np.arange(500) % 3)[:, None] * rng.uniform(0, 2, (1, 300)))).astype(np.float32)
  dense = SingleCellOMIC(counts).normalize(total=True, log1p=True)
  sparse = SingleCellOMIC(sp.csr_matrix(counts)).normalize(total=True, log1p=True)
  assert sparse.is_sparse() and not dense.is_sparse()
  Y = dense.umap()
  assert Y.shape == (500, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
  assert dense.umap() is Y
  assert _same_bits(sparse.umap(), Y)
  fresh = SingleCellOMIC(counts).normalize(total=True, log1p=True)
  for mine, theirs in zip(dense.neighbors()[:2], fresh.neighbors()[:2]):   # neighbors() is left as neighbors() leaves it
    assert np.array_equal(mine.indptr, theirs.indptr) and np.array_equal(mine.indices, theirs.indices) and _same_bits(mine.data, theirs.data)
  assert dense.neighbors()[2] == fresh.neighbors()[2]
  Y1 = dense.umap(n_components=1, n_epochs=20)
  assert Y1.shape == (500, 1) and dense.umap() is Y
