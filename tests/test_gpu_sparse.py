"""Sparse count matrices end to end on the GPU: every inference and scoring entry point given CSR rows (the rows convention of
include/sisua_hip.h: smx_predict and its statistics, smx_marginal_llk) returns the bits it returns for the dense rows of the same
counts, a fit on a sparse SingleCellOMIC is the fit on its dense twin, and every such entry refuses rows given in both forms or in
neither."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.util import synth_counts, synth_labels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
  from sisua_amd import build
  build.build(verbose=False)
  import sisua_amd.models as M
  return M


def _counts(n=300, g=120, seed=3):
  """Counts with empty rows and a fully dense block of rows (chunks cut by non-zeros there)."""
  x = synth_counts(n, g, sparsity=0.85, seed=seed)
  x[5] = 0.0
  x[n - 3] = 0.0
  x[40:104] = np.maximum(x[40:104], 1.0)
  return x


def _sco(x, sparse, labels=None):
  from sisua_amd.data import SingleCellOMIC
  s = SingleCellOMIC(sp.csr_matrix(x) if sparse else x, name="toy")
  if labels is not None:
    s.add_omic("proteomic", labels)
  return s


KINDS = ["vae_zinb", "vae_nb", "dca", "mse", "scvi_nbd", "scvi_zinbd", "sisua", "scale", "scale_post", "fvae"]


def _model(api, kind, g, n_lab=9):
  rna = api.RVmeta(g, {"vae_nb": "nb", "mse": "mse", "scvi_nbd": "nbd", "scvi_zinbd": "zinbd"}.get(kind, "zinb"), True, "transcriptomic")
  net = dict(encoder=api.NetConf([32], batchnorm=True, dropout=0.1), decoder=api.NetConf([32], batchnorm=True, dropout=0.1))
  lat = api.RVmeta(6, "diag", True, "Latents")
  if kind in ("vae_zinb", "vae_nb"):
    return api.VAE(outputs=rna, latents=lat, **net)
  if kind in ("dca", "mse"):
    return api.DeepCountAutoencoder(outputs=rna, **net)
  if kind.startswith("scvi"):
    return api.SCVI(outputs=rna, latents=lat, **net)
  if kind == "sisua":
    return api.SISUA(outputs=rna, labels=[api.RVmeta(n_lab, "nb", True, "proteomic")], latents=lat, **net)
  if kind == "scale":
    return api.SCALE(outputs=rna, latents=api.RVmeta(6, "mixgaus", True, "Latents"), n_components=3, **net)
  if kind == "scale_post":
    return api.SCALE(outputs=rna, latents=api.RVmeta(6, "mixgaus", True, "Latents"), n_components=3, mixture="posterior", **net)
  return api.FVAE(outputs=rna, latents=lat, **net)


def _trained(api, kind, x, y):
  m = _model(api, kind, x.shape[1])
  m.fit(_sco(x, False, y if kind == "sisua" else None), epochs=2, batch_size=64, verbose=False)
  return m


def _first(d):
  return d[0] if isinstance(d, (tuple, list)) else d


def _same_dists(a, b):
  a = a if isinstance(a, (tuple, list)) else [a]
  b = b if isinstance(b, (tuple, list)) else [b]
  assert len(a) == len(b)
  for u, v in zip(a, b):
    assert np.array_equal(u.mean(), v.mean())


@pytest.mark.parametrize("kind", KINDS)
def test_inference_sparse_equals_dense(api, kind):
  x = _counts()
  y = synth_labels(x.shape[0], ((9, "nb"),))[0]
  xs = sp.csr_matrix(x)
  m = _trained(api, kind, x, y)
  # eager predict, one draw and several
  for shape in ((), (3,)):
    Xd, Zd = m.predict(x, sample_shape=shape, batch_size=32, verbose=False)
    Xs, Zs = m.predict(xs, sample_shape=shape, batch_size=32, verbose=False)
    _same_dists(Xd, Xs)
    _same_dists(Zd, Zs)
  # a sparse BatchDataset and a sparse container (lazy where the output has a count distribution)
  ds_d, ds_s = _sco(x, False).create_dataset(batch_size=32, shuffle=0), _sco(x, True).create_dataset(batch_size=32, shuffle=0)
  assert sp.issparse(ds_s.arrays[0])
  _same_dists(m.predict(ds_d, verbose=False)[0], m.predict(ds_s, verbose=False)[0])
  for shape in ((), (2,)):
    Ld, _ = m.predict(_sco(x, False), sample_shape=shape, batch_size=32, verbose=False)
    Ls, _ = m.predict(_sco(x, True), sample_shape=shape, batch_size=32, verbose=False)
    Ld, Ls = _first(Ld), _first(Ls)
    assert np.array_equal(Ld.mean(), Ls.mean()) and np.array_equal(Ld.variance(), Ls.variance())
    if kind != "mse":
      assert np.array_equal(Ld.log_prob(), Ls.log_prob())
      assert np.array_equal(Ld.log_prob(x + 1.0), Ls.log_prob(sp.csr_matrix(x + 1.0)))
      assert np.array_equal(Ld.log_prob(x + 1.0), Ld.log_prob(sp.csr_matrix(x + 1.0)))
  # __call__ and encode on one batch of rows
  for shape in ((), (2,)):
    _same_dists(m(x[:48], sample_shape=shape)[0], m(xs[:48], sample_shape=shape)[0])
  q_d, q_s = m.encode(x[:48]), m.encode(xs[:48])
  for u, v in zip(q_d if isinstance(q_d, list) else [q_d], q_s if isinstance(q_s, list) else [q_s]):
    assert np.array_equal(u.mean(), v.mean())
  # the engine's statistics: all four, dense and CSR targets
  e = m._engine
  lib = None
  if kind.startswith("scvi"):
    from sisua_amd.data import library_matrix
    lib = library_matrix(x)
    assert np.array_equal(library_matrix(xs), lib)
  for stat in ("mean", "variance", "mean_over_samples", "log_prob"):
    if stat == "log_prob" and kind == "mse":
      continue
    a = e.predict_stat(x, stat, library=lib, n_samples=2, batch=32)
    b = e.predict_stat(xs, stat, library=lib, n_samples=2, batch=32)
    assert np.array_equal(a, b), stat
  if kind != "mse":
    t = x[::-1].copy()
    a = e.predict_stat(x, "log_prob", library=lib, n_samples=2, batch=32, target=t)
    assert np.array_equal(a, e.predict_stat(xs, "log_prob", library=lib, n_samples=2, batch=32, target=sp.csr_matrix(t)))
    assert np.array_equal(a, e.predict_stat(x, "log_prob", library=lib, n_samples=2, batch=32, target=sp.csr_matrix(t)))
    # marginal_log_prob (SISUA: given its label array too) and posterior_llk
    if kind == "sisua":
      md, ld = m.marginal_log_prob([x, y], sample_shape=4)
      ms, ls = m.marginal_log_prob([xs, y], sample_shape=4)
    else:
      md, ld = m.marginal_log_prob(x, sample_shape=4)
      ms, ls = m.marginal_log_prob(xs, sample_shape=4)
    assert np.array_equal(md, ms) and all(np.array_equal(ld[k], ls[k]) for k in ld)
    assert m.posterior_llk(x[:64], original=x[:64] + 1.0, sample_shape=3) == \
        m.posterior_llk(xs[:64], original=sp.csr_matrix(x[:64] + 1.0), sample_shape=3)
  # scVI with a given library
  if kind.startswith("scvi"):
    lib2 = np.tile(np.array([[1.5, 0.25]], np.float32), (x.shape[0], 1))
    e = m._engine   # (the scoring calls above may have made the model a new engine)
    a = e.predict(x, library=lib2, n_samples=2, batch=32)
    b = e.predict(xs, library=lib2, n_samples=2, batch=32)
    assert all(np.array_equal(a[k], b[k]) for k in a if k != "y_params" and a[k] is not None)
    assert np.array_equal(m.marginal_log_prob(x, library=lib2, sample_shape=3)[0], m.marginal_log_prob(xs, library=lib2, sample_shape=3)[0])


def test_predict_chunks_cut_by_nonzeros(api):
  """Staging forced small: the dense block of rows makes the CSR chunks shorter than the dense ones; same bits, ragged last chunk."""
  from sisua_amd import _hip
  x = _counts(n=301)
  xs = sp.csr_matrix(x)
  m = _trained(api, "vae_zinb", x, None)
  e = m._engine
  ref = e.predict(x, n_samples=2, batch=16)
  refs = e.predict_stat(x, "log_prob", n_samples=2, batch=16)
  _hip.set_tuning("predict_stage_floats", 8000)   # (log_prob: 48-cell chunks, 4000 non-zeros; predict: one batch per chunk)
  try:
    got = e.predict(xs, n_samples=2, batch=16)
    gots = e.predict_stat(xs, "log_prob", n_samples=2, batch=16)
  finally:
    _hip.clear_tuning("predict_stage_floats")
  assert all(np.array_equal(ref[k], got[k]) for k in ref if k != "y_params" and ref[k] is not None)
  assert np.array_equal(refs, gots)


def test_wide_panel(api):
  """20 000 genes (several LDS segments per row), batch 256."""
  x = synth_counts(520, 20000, sparsity=0.86, seed=5)
  x[7] = 0.0
  xs = sp.csr_matrix(x)
  m = _model(api, "vae_zinb", 20000)
  m._ensure_engine(256)
  e = m._engine
  a, b = e.predict(x, n_samples=1, batch=256), e.predict(xs, n_samples=1, batch=256)
  assert all(np.array_equal(a[k], b[k]) for k in a if k != "y_params" and a[k] is not None)
  assert np.array_equal(e.predict_stat(x, "log_prob", n_samples=2, batch=256), e.predict_stat(xs, "log_prob", n_samples=2, batch=256))
  ma, mb = e.marginal_llk(x=x[:256], n_samples=4), e.marginal_llk(x=xs[:256], n_samples=4)
  assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])


def _fit_state(m):
  return m._engine.get_params(), {k: list(v) for k, v in m.train_history.items()}, {k: list(v) for k, v in m.valid_history.items()}


def _same_fit(a, b):
  pa, ta, va = a
  pb, tb, vb = b
  assert ta == tb and va == vb
  assert all(np.array_equal(pa[k], pb[k]) for k in pa)


@pytest.mark.parametrize("kind", ["vae_zinb", "sisua"])
def test_fit_sparse_equals_dense_csr_store(api, kind):
  x = _counts(n=400)
  y = synth_labels(x.shape[0], ((9, "nb"),))[0] if kind == "sisua" else None
  runs = []
  for sparse in (False, True):
    tr, va = _sco(x, sparse, y).split(0.8)
    m = _model(api, kind, x.shape[1])
    kw = dict(storage="csr") if not sparse else {}
    m.fit(tr, valid=va, epochs=3, batch_size=32, valid_freq=5, verbose=False, **kw)
    runs.append(_fit_state(m))
  _same_fit(*runs)


def test_fit_sparse_u16_store(api):
  x = _counts(n=300)
  runs = []
  for sparse in (False, True):
    m = _model(api, "vae_nb", x.shape[1])
    m.fit(_sco(x, sparse), epochs=2, batch_size=32, storage="u16", verbose=False)
    runs.append(_fit_state(m))
  _same_fit(*runs)


def test_experiment_on_sparse_cortex(api, monkeypatch):
  import sisua_amd.train as T
  from sisua_amd import data
  x, y = data.synthetic_cortex()
  runs = []
  for sparse in (False, True):
    monkeypatch.setattr(T, "get_dataset", lambda name, s=sparse: data.SingleCellOMIC(sp.csr_matrix(x) if s else x, name="cortex")
                        .add_omic("celltype", y))
    exp = T.Experiment(dict(model=dict(name="vae"), dataset=dict(name="cortex", batch_size=64), train=dict(epochs=2)))
    m = exp.run()
    assert exp.sco.is_sparse() == sparse and exp.train.is_sparse() == sparse
    runs.append(_fit_state(m))
  _same_fit(*runs)


def test_rows_in_both_forms_or_in_neither_are_refused(api):
  """The rows convention at the raw binding: each of the seven entries that take (host_x, indptr, cols, vals) answers SMX_ERR_INVALID
  with the one shared wording when given both forms of the rows and when given neither -- as do smx_predict_stat for both forms of its
  target, smx_predict_impute for neither form of the original, and smx_marginal_llk for row_ids beside CSR rows (its own wording).  All
  are host refusals in front of any device work: no result array is touched.  33 genes (ragged against the 32-column padding), 70 cells
  in batches of 32 (ragged last batch), 2 draws."""
  from sisua_amd import _hip
  from sisua_amd.engine._args import _csr3, _dp, _fp, _ip, _matrix_ptrs, _ptr
  G, N, B, S, P, D = 33, 70, 32, 2, 2, 6
  x = np.ascontiguousarray(synth_counts(N, G, sparsity=0.8, seed=11), dtype=np.float32)
  csr = _csr3(sp.csr_matrix(x), G)
  csr_b = (np.ascontiguousarray(csr[0][:B + 1]), csr[1], csr[2])   # the first batch's rows: what smx_marginal_llk takes
  m = _model(api, "vae_zinb", G)
  m._ensure_engine(B)
  h, lib = m._engine._h, _hip.load()
  f32 = lambda *shape: np.full(shape, np.nan, np.float32)
  out = dict(z_mean=f32(N, D), stat=f32(N, G), logp=f32(S, N), sample=f32(1, S, N, G), cols=f32(N, 3), med=f32(N), lohi=f32(2), mllk=f32(B), llk=f32(B),
             pe=np.full((3, G + G + G * P), np.nan, np.float64), chg=np.full(N, -7, np.int32), nonfinite=np.full(G, -7, np.int32),
             sp=np.full((2 * G + G * P,), -7, np.int64))
  genes = np.array([0, 32, 7], np.int32)
  pr, pu, ids = np.zeros((P, N), np.int32), np.zeros((P, N), np.float64), np.zeros(B, np.int32)
  none4, good, good_b = (None,) * 4, _matrix_ptrs(None, csr), _matrix_ptrs(None, csr_b)
  lp = lambda a: _ptr(a, np.int64)
  cor_out = (lp(out["sp"][:G]), lp(out["sp"][G:2 * G]), lp(out["sp"][2 * G:]), _dp(out["pe"][0]), _dp(out["pe"][1]), _dp(out["pe"][2]), _ip(out["nonfinite"]))
  head = (None, N, B, S)   # host_library, n_cells, batch, n_samples
  entries = {   # name -> the call, given the four rows pointers
      "smx_predict": lambda r: lib.smx_predict(h, *r, *head, _fp(out["z_mean"]), None, None, None, None, None, None, None),
      "smx_predict_stat": lambda r: lib.smx_predict_stat(h, *r, *head, 2, 0, *none4, _fp(out["stat"])),
      "smx_predict_sample": lambda r: lib.smx_predict_sample(h, *r, *head, 0, 5, 1, _fp(out["sample"])),
      "smx_predict_stat_cols": lambda r: lib.smx_predict_stat_cols(h, *r, *head, 0, _ip(genes), genes.size, _fp(out["cols"])),
      "smx_predict_impute": lambda r: lib.smx_predict_impute(h, *r, *head, 0, *_matrix_ptrs(x, None), _fp(out["med"]), _ip(out["chg"]), _fp(out["lohi"])),
      "smx_predict_correlate": lambda r: lib.smx_predict_correlate(h, *r, *head, 0, None, 0, _ip(pr), _dp(pu), P, *cor_out),
      "smx_marginal_llk": lambda r: lib.smx_marginal_llk(h, None, *r, None, B, S, _fp(out["mllk"]), _fp(out["llk"])),
  }
  shared = b"exactly one of the dense matrix and the CSR arrays"

  def refused(status, wording):
    assert status == -1, (status, lib.smx_last_error())   # SMX_ERR_INVALID
    assert wording in lib.smx_last_error(), lib.smx_last_error()

  for name, call in entries.items():
    both = (_fp(x), *(good_b if name == "smx_marginal_llk" else good)[1:])
    refused(call(both), shared)
    refused(call(none4), shared)
  # a second matrix is held to the same rule: both forms of the target, neither form of the original
  refused(lib.smx_predict_stat(h, *good, *head, 3, 0, _fp(x), *good[1:], _fp(out["logp"])), shared)
  refused(lib.smx_predict_impute(h, *good, *head, 0, *none4, _fp(out["med"]), _ip(out["chg"]), _fp(out["lohi"])), shared)
  # resident cells by id, or host rows: not both
  refused(lib.smx_marginal_llk(h, _ip(ids), *good_b, None, B, S, _fp(out["mllk"]), _fp(out["llk"])), b"row_ids or host rows")
  for k, a in out.items():
    assert (np.isnan(a) if a.dtype.kind == "f" else a == -7).all(), k
