"""smx_louvain.hip on the device against the NumPy restatement (tests/louvain_ref.py), through engine.k_louvain / k_modularity,
`sisua_amd.louvain` and `SingleCellOMIC.louvain`.

What is compared, per graph: labels, the number of levels, every level's size, sweep count and colour count EQUAL; the Q trace within
1e-12 (its only float sum is mirrored, so it is in fact the same bits).  Equality is honest for unit and weighted graphs alike: every
degree, total and internal weight is an int64 sum of quantised weights, a gain is float64 from those integers with every operation rounded
once on both sides, and ties go to the lowest id -- nothing depends on a summation order.

Graphs: the blob kNN graphs of the host test (300 to 2000 vertices; "wide" spans several workgroups per colour and 13 colours), weighted
"touch" at three resolutions, a ring of cliques, two cliques with isolated vertices, a graph without entries, a single vertex, and a hub
joined to 40 cliques of 128: its row is far beyond the wave form's table (the bound is read from the library), and the cliques' rows
of 128 entries fill that table to its limit."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import louvain_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def graphs():
  out = {name: (A, uw, g) for name, A, uw, g in R.blob_cases()}
  out["ring"] = (R.ring_of_cliques(), False, 1.0)
  out["two"] = (R.two_cliques_and_isolated(), False, 1.0)
  out["empty"] = (R.empty_graph(), False, 1.0)
  out["single"] = (sp.csr_matrix((1, 1), dtype=np.float64), False, 1.0)
  out["hub"] = (R.hub_graph(), False, 1.0)
  return out


NAMES = ["clean", "touch", "cloud", "ragged", "wide", "touch_w_g0.5", "touch_w_g1.0", "touch_w_g2.0", "touch_g0.5", "touch_g2.0", "ring", "two",
         "empty", "single", "hub"]


@functools.lru_cache(maxsize=None)
def reference(name):
  A, uw, g = graphs()[name]
  return R.louvain(A, g, uw)


def csr_args(A, use_weights):
  A = sp.csr_matrix(A)
  return A.indptr.astype(np.int64), A.indices.astype(np.int32), (A.data.astype(np.float64) if use_weights else None), A.shape[0]


def same_result(got, want):
  assert np.array_equal(got["labels"], want["labels"])
  assert got["n_levels"] == want["n_levels"] and got["n_communities"] == want["n_communities"]
  for k in ("level_size", "sweeps", "colours"):
    assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
  if want["n_levels"]:
    assert np.abs(got["modularity"] - want["modularity"]).max() <= 1e-12, (got["modularity"], want["modularity"])


def test_names_cover_the_graphs():
  assert sorted(NAMES) == sorted(graphs())


@pytest.mark.parametrize("name", NAMES)
def test_device_is_the_restatement(name):
  from sisua_amd import engine
  A, uw, g = graphs()[name]
  want = reference(name)
  got = engine.k_louvain(*csr_args(A, uw), resolution=g)
  print(name, "levels", got["n_levels"], "sizes", got["level_size"], "sweeps", got["sweeps"], "colours", got["colours"], "Q", got["modularity"])
  same_result(got, want)
  # the scoring entry, on the result and on a random labelling
  ip, cj, w, n = csr_args(A, uw)
  for labels in (want["labels"], np.random.RandomState(5).randint(0, min(n, 9), n)):
    q = engine.k_modularity(ip, cj, w, n, labels, resolution=g)
    assert abs(q - R.modularity(A, labels, g, uw)) <= 1e-12
  if want["n_levels"]:
    assert abs(engine.k_modularity(ip, cj, w, n, want["labels"], resolution=g) - want["modularity"][-1]) <= 1e-12


def test_hub_row_is_beyond_the_wave_form():
  from sisua_amd import engine
  A = graphs()["hub"][0]
  degree = np.diff(A.indptr)
  bound = engine.louvain_table_degree()
  assert degree.max() > 8 * bound and (degree == bound).sum() >= 40 * 128 - 1 and bound >= 64


@pytest.mark.parametrize("name", ["wide", "touch_w_g1.0", "hub"])
def test_same_bits_across_calls_and_column_orders(name):
  from sisua_amd import engine
  A, uw, g = graphs()[name]
  want = reference(name)
  A = sp.csr_matrix(A)
  ip, n = A.indptr.astype(np.int64), A.shape[0]
  rng = np.random.RandomState(7)
  orders = {"again": np.arange(A.nnz), "reversed": np.arange(A.nnz), "permuted": np.arange(A.nnz)}
  for i in range(n):
    s, e = ip[i], ip[i + 1]
    orders["reversed"][s:e] = orders["reversed"][s:e][::-1]
    orders["permuted"][s:e] = rng.permutation(orders["permuted"][s:e])
  for how, p in orders.items():
    got = engine.k_louvain(ip, A.indices[p].astype(np.int32), A.data[p].astype(np.float64) if uw else None, n, resolution=g)
    assert got["labels"].tobytes() == want["labels"].tobytes(), how
    assert got["modularity"].tobytes() == want["modularity"].tobytes(), how


@pytest.mark.parametrize("name", ["wide", "touch_w_g1.0", "ring", "cloud"])
def test_workgroup_form_gives_the_wave_forms_labels(name):
  """every row of more than 4 entries through the workgroup form (the sort and the tie runs): the same result"""
  from sisua_amd import _hip, engine
  A, uw, g = graphs()[name]
  _hip.set_tuning("louvain_table_degree", 4)
  assert engine.louvain_table_degree() == 4
  got = engine.k_louvain(*csr_args(A, uw), resolution=g)
  _hip.clear_tuning("louvain_table_degree")
  assert engine.louvain_table_degree() > 4
  same_result(got, reference(name))


def test_settings_reach_the_device():
  from sisua_amd import engine
  A, uw, g = graphs()["touch"]
  for kw in (dict(max_sweeps=2), dict(max_levels=1), dict(max_levels=2, tol=1e-2)):
    want = R.louvain(A, g, uw, **kw)
    same_result(engine.k_louvain(*csr_args(A, uw), resolution=g, **kw), want)


def test_library_refuses_before_any_device_work():
  from sisua_amd import _hip, engine
  A = sp.csr_matrix(graphs()["ragged"][0])
  ip, cj, _, n = csr_args(A, False)
  U = sp.triu(A).tocsr()
  with pytest.raises(_hip.SmxError, match="symmetric"):
    engine.k_louvain(*csr_args(U, False))
  w = np.ones(A.nnz)
  w[0] = 3.0
  with pytest.raises(_hip.SmxError, match="symmetric"):
    engine.k_louvain(ip, cj, w, n)
  twice = cj.copy()
  twice[1] = twice[0]
  with pytest.raises(_hip.SmxError, match="twice|symmetric"):
    engine.k_louvain(ip, twice, None, n)
  with pytest.raises(_hip.SmxError, match="symmetric"):
    engine.k_modularity(*csr_args(U, False), np.zeros(n, np.int32))


def cells_container(sparse):
  from sisua_amd.data import SingleCellOMIC
  x, planted = R.blob_cells("clean")
  x = x - x.min()
  sco = SingleCellOMIC(sp.csr_matrix(x) if sparse else x, var_names=[f"g{i}" for i in range(x.shape[1])])
  sco.add_omic("proteomic", np.eye(6, dtype=np.float32)[planted], var_names=["CD3", "CD4", "CD8", "CD19", "CD14", "CD56"])
  return sco, planted


def test_dense_and_csr_containers_give_the_same_labels():
  import sisua_amd
  a, planted = cells_container(False)
  b, _ = cells_container(True)
  ga, gb = a.neighbors()[0], b.neighbors()[0]
  la, lb = sisua_amd.louvain(ga), sisua_amd.louvain(gb)
  assert la.tobytes() == lb.tobytes()
  assert np.array_equal(la, R.louvain(ga)["labels"])
  wa, wb = sisua_amd.louvain(ga, use_weights=True), sisua_amd.louvain(gb, use_weights=True)
  assert wa.tobytes() == wb.tobytes() and np.array_equal(wa, R.louvain(ga, use_weights=True)["labels"])
  assert len({(p, c) for p, c in zip(planted, la)}) == 6   # the planted blobs


def test_neighbors_louvain_rank_end_to_end():
  sco, planted = cells_container(False)
  sco.neighbors()
  y, y_labels = sco.louvain()
  assert y.dtype == np.float32 and y.shape == y_labels.shape == (300,)
  assert len({(p, c) for p, c in zip(planted, y)}) == 6
  assert len(set(zip(y.tolist(), y_labels.tolist()))) == len(np.unique(y)) == 6   # one name per community
  var = set(sco.get_var_names("transcriptomic"))
  assert all(set(name.split("_")) <= var for name in set(y_labels) if name)
  key = sco.rank_vars_groups(n_vars=4, group_by="transcriptomic_louvain", method="wilcoxon")
  res = sco.get_rank_vars_groups(key)
  assert sorted(res["names"].dtype.names) == [str(c) for c in range(6)] and len(res["names"]) == 4
  y2, names2 = sco.louvain(resolution=3.0)
  assert np.array_equal(y2, y) and names2 is y_labels   # kept
  # the protein omic: a 0 / 1 matrix is its own embedding, six variables go through the mixtures
  yp, names_p = sco.louvain("proteomic")
  assert len(set(zip(yp.tolist(), names_p.tolist()))) == len(np.unique(yp))
  assert {"proteomic_louvain", "proteomic_louvain_labels", "transcriptomic_louvain", "transcriptomic_louvain_labels"} <= set(sco._obs)
