"""Engine: the Python owner of one `smx_model` (one GPU, one stream).

Thin, mechanical wrapper over the C-ABI (include/sisua_hip.h): it converts numpy
arrays to pointers, keeps the tensor manifest, and raises `SmxError` on any
non-zero status.  All arithmetic happens in libsisua_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from sisua_amd import _hip, interpolation, optimizers
from sisua_amd._hip import SmxError, check, smx_config, smx_metrics
from sisua_amd.config import ModelConfig, init_params, label_planes, manifest

STREAM_INPUT_DROPOUT = 0
STREAM_ENC_DROPOUT = 16
STREAM_ENCL_DROPOUT = 32
STREAM_DEC_DROPOUT = 48
STREAM_EPS_Z = 64
STREAM_EPS_L = 65


def _fp(a: Optional[np.ndarray]):
  return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, shape=None):
  a = np.ascontiguousarray(a, dtype=np.float32)
  if shape is not None and tuple(a.shape) != tuple(shape):
    raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
  return a


def _csr3(x, n_genes: int, n_rows: Optional[int] = None):
  """scipy.sparse rows -> (indptr int64, cols int32, vals float32) of their canonical float32 CSR (data.as_csr), shape-checked."""
  from sisua_amd.data import as_csr
  if x.ndim != 2 or x.shape[1] != n_genes or (n_rows is not None and x.shape[0] != n_rows):
    raise ValueError(f"expected sparse rows [{'n_cells' if n_rows is None else n_rows}, {n_genes}], got {x.shape}")
  c = as_csr(x, copy=False)
  return (np.ascontiguousarray(c.indptr, dtype=np.int64), np.ascontiguousarray(c.indices, dtype=np.int32),
          np.ascontiguousarray(c.data, dtype=np.float32))


def _csr_ptrs(t):
  return (t[0].ctypes.data_as(C.POINTER(C.c_int64)), t[1].ctypes.data_as(C.POINTER(C.c_int32)), _fp(t[2]))


def _fps(arrays):
  """A C array of float pointers to `arrays` (label heads), None without any; the caller keeps `arrays` alive through the call."""
  return (C.POINTER(C.c_float) * max(1, len(arrays)))(*[_fp(a) for a in arrays]) if arrays else None


def _check_u16(a):
  if a.size and (a.min() < 0 or a.max() > 65535 or not np.array_equal(a, np.floor(a))):
    raise ValueError("storage='u16' needs integer counts in [0, 65535]")


def _sparse(x) -> bool:
  from sisua_amd.data import is_sparse
  return is_sparse(x)


def _tril_scale(out):
  """A full-covariance posterior's results: z_scale = the marginal standard deviations sqrt(diag(L L^T)) of the factor the device returned."""
  L = out.get("scale_tril")
  if L is not None:
    out["z_scale"][...] = np.sqrt(np.square(L, dtype=np.float64).sum(-1))
  return out


def gene_indices(genes, n_genes: int) -> np.ndarray:
  """A list of gene indices as int32 [n_sel] (any order, repeats allowed); an index outside 0 .. n_genes - 1 or an empty list raises."""
  g = np.asarray(genes)
  if g.ndim != 1 or g.size == 0 or not np.issubdtype(g.dtype, np.integer):
    raise ValueError("genes must be a non-empty 1-D list of integer gene indices")
  if g.min() < 0 or g.max() >= n_genes:
    raise IndexError(f"gene index out of range 0 .. {n_genes - 1}")
  return np.ascontiguousarray(g, dtype=np.int32)


def make_smx_config(cfg: ModelConfig, max_batch: int) -> smx_config:
  c = smx_config()
  c.abi_version = _hip.SMX_ABI_VERSION
  c.model = _hip.MODEL_KINDS["scale_post" if cfg.latent_mixture else "scale_tril" if cfg.scale_tril else cfg.model]   # (SCALE's covariance='tril' changes a tensor's shape: a model kind of its own, no new field)
  c.likelihood = _hip.LIKELIHOODS[cfg.likelihood]
  c.n_genes, c.latent_dim = int(cfg.n_genes), int(cfg.latent_dim)
  for name, units in (("enc", cfg.enc_units), ("dec", cfg.dec_units), ("encl", cfg.encl_units if cfg.model == "scvi" else ())):
    if len(units) > _hip.SMX_MAX_LAYERS:
      raise ValueError(f"at most {_hip.SMX_MAX_LAYERS} layers per network")
    setattr(c, f"n_{name}", len(units))
    arr = getattr(c, f"{name}_units")
    for i, u in enumerate(units):
      arr[i] = int(u)
  if len(cfg.targets) > _hip.SMX_MAX_LABELS:
    raise ValueError(f"at most {_hip.SMX_MAX_LABELS} heads (extra outputs + label variables)")
  c.n_labels = len(cfg.targets)
  for j, (P, llk) in enumerate(cfg.targets):
    c.label_dim[j] = int(P)
    c.label_llk[j] = _hip.LABEL_LIKELIHOODS[llk[:-1] if llk.startswith("mix") else llk]
    c.label_components[j] = int(llk[-1]) if llk.startswith("mix") else 1
    c.label_observed[j] = 1 if j < len(cfg.extra_outputs) else 0
  c.scvi_dispersion = _hip.SCVI_PLANE_OPTIONS[cfg.dispersion]
  c.scvi_inflation = _hip.SCVI_PLANE_OPTIONS[cfg.inflation]
  c.batchnorm, c.log_norm = int(cfg.batchnorm), int(cfg.log_norm)
  c.latent_activation = _hip.ACTIVATIONS[cfg.latent_activation]
  c.dropout_enc, c.dropout_dec, c.input_dropout = cfg.dropout_enc, cfg.dropout_dec, cfg.input_dropout
  c.beta, c.alpha, c.clip_library = cfg.beta, cfg.alpha, cfg.clip_library
  c.bn_momentum, c.bn_eps = cfg.bn_momentum, cfg.bn_eps
  c.lr, c.adam_beta1, c.adam_beta2, c.adam_eps, c.clipnorm = cfg.lr, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, cfg.clipnorm
  c.n_components = int(cfg.n_components)
  c.latent_tril = int(bool(cfg.latent_tril))
  c.disc_units, c.disc_layers = int(cfg.disc_units), int(cfg.disc_layers)
  c.gamma, c.disc_leak = float(cfg.gamma), float(cfg.disc_leak)
  c.max_batch = int(max_batch)
  c.seed = int(cfg.seed) & 0xFFFFFFFFFFFFFFFF
  return c


_SCHED_TARGETS = {"beta": 0, "lr": 1}   # smx_schedule_target


class Engine:

  def __init__(self, cfg: ModelConfig, max_batch: int = 256, device: int = 0, init: bool = True):
    self.lib = _hip.require_gpu(device)
    self.cfg = cfg
    self.max_batch = int(max_batch)
    self._h = C.c_void_p()
    self.last_comm_error = 0   # the hand-written exchange's error word as the last failed step left it (_step_check)
    c = make_smx_config(cfg, max_batch)
    check(self.lib.smx_model_create(C.byref(c), C.byref(self._h)))
    # manifest handshake: the library's tensor list must equal the host's
    self.names, self.shapes = [], {}
    buf = C.create_string_buffer(64)
    rows, cols = C.c_int32(), C.c_int32()
    for i in range(self.lib.smx_num_tensors(self._h)):
      check(self.lib.smx_tensor_info(self._h, i, buf, 64, C.byref(rows), C.byref(cols)))
      name = buf.value.decode()
      self.names.append(name)
      self.shapes[name] = (rows.value, cols.value) if (name.endswith("/W") or rows.value > 1) else (cols.value,)
    expect = manifest(cfg)
    if [(n, tuple(self.shapes[n])) for n in self.names] != [(n, tuple(s)) for n, s in expect]:
      raise SmxError("tensor manifest of libsisua_hip.so differs from sisua_amd.config.manifest")
    self.index = {n: i for i, n in enumerate(self.names)}
    self.n_cells = 0
    if cfg.model == "scale":   # scale.py:29-33: tied mixture parameters (model semantics carried as flags: no layout change of smx_config)
      for name in ("tie_mixtures", "tie_loc", "tie_scale"):
        if getattr(cfg, name, False):
          check(self.lib.smx_set_flag(self._h, name.encode(), 1))
    # hidden-layer activations (NetConf.activation): set before any step; ReLU is the library's default
    nets = [("enc_activation", _hip.SMX_NET_ENCODER), ("dec_activation", _hip.SMX_NET_DECODER)]
    if cfg.model == "scvi":
      nets.append(("encl_activation", _hip.SMX_NET_LIBRARY_ENCODER))
    for field, net in nets:
      act = getattr(cfg, field)
      if act != "relu":
        check(self.lib.smx_set_activation(self._h, net, _hip.HIDDEN_ACTIVATIONS[act]))
    if init:
      self.set_params(init_params(cfg))

  # ---- lifetime ---------------------------------------------------------------
  def close(self):
    if getattr(self, "_h", None) is not None and self._h:
      self.lib.smx_model_destroy(self._h)
      self._h = C.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  # ---- parameters / state -------------------------------------------------------
  def get_params(self, which: int = 0) -> Dict[str, np.ndarray]:
    """which: 0 params, 1 gradients of the last step, 2 Adam m, 3 Adam v."""
    out = {}
    for i, n in enumerate(self.names):
      a = np.empty(self.shapes[n], dtype=np.float32)
      check(self.lib.smx_get_tensor(self._h, which, i, _fp(a)))
      out[n] = a
    return out

  def set_params(self, params: Dict[str, np.ndarray], which: int = 0):
    for n, v in params.items():
      a = _f32(v, self.shapes[n])
      check(self.lib.smx_set_tensor(self._h, which, self.index[n], _fp(a)))

  def get_bn(self) -> Dict[int, Dict[str, np.ndarray]]:
    out = {}
    w = C.c_int32()
    for i in range(self.lib.smx_num_bn_layers(self._h)):
      check(self.lib.smx_get_bn(self._h, i, 0, None, C.byref(w)))
      mean, var = np.empty(w.value, np.float32), np.empty(w.value, np.float32)
      check(self.lib.smx_get_bn(self._h, i, 0, _fp(mean), None))
      check(self.lib.smx_get_bn(self._h, i, 1, _fp(var), None))
      out[i] = dict(moving_mean=mean, moving_var=var)
    return out

  def set_bn(self, state: Dict[int, Dict[str, np.ndarray]]):
    for i, st in state.items():
      check(self.lib.smx_set_bn(self._h, int(i), 0, _fp(_f32(st["moving_mean"]))))
      check(self.lib.smx_set_bn(self._h, int(i), 1, _fp(_f32(st["moving_var"]))))

  def snapshot(self) -> dict:
    """Everything a training step changes -- parameters, both optimiser slots, the BatchNorm moving statistics, the step counter -- and
    the optimiser rule as host values (what models.py keeps in a checkpoint; parallel.calibrate_forms restores it after its trial steps)."""
    return dict(params=self.get_params(0), m=self.get_params(2), v=self.get_params(3), bn=self.get_bn(), step=self.step,
                opt=self.get_optimizer())

  def restore(self, st: dict):
    if st.get("opt") is not None:
      self.restore_optimizer(*st["opt"])
    self.set_params(st["params"], 0)
    self.set_params(st["m"], 2)
    self.set_params(st["v"], 3)
    self.set_bn(st["bn"])
    self.step = int(st["step"])

  # ---- optimiser rule -------------------------------------------------------------
  def get_optimizer(self):
    """(rule name, {hyper-parameter: value}, t0): the rule of the training steps and the step at which its state began."""
    rule, t0 = C.c_int32(), C.c_int32()
    hp = np.zeros(4, np.float32)
    check(self.lib.smx_get_optimizer(self._h, C.byref(rule), _fp(hp), C.byref(t0)))
    name = optimizers.NAMES[rule.value]
    return name, optimizers.hp_dict(name, hp.astype(np.float64)), int(t0.value)

  def set_optimizer(self, name: str = "adam", **hp) -> bool:
    """The optimiser rule of the later training steps: 'adam', 'sgd' (momentum, nesterov), 'rmsprop' (rho, momentum, epsilon), 'adagrad'
    (initial_accumulator_value, epsilon), 'adamax' (beta_1, beta_2, epsilon); tf.keras 2.x defaults (Adam's: the config's).  The same
    rule with the same hyper-parameters again: nothing changes, the state continues.  Anything else starts the rule fresh, as a new
    Keras optimiser object does -- slots initialised, t0 = the current step (smx_set_optimizer).  True when the rule started fresh."""
    name, full = optimizers.canonical(name, **hp)
    if name == "adam" and not hp:   # (Adam's defaults are the config's)
      full = dict(beta_1=self.cfg.adam_beta1, beta_2=self.cfg.adam_beta2, epsilon=self.cfg.adam_eps)
    cur = self.get_optimizer()
    if optimizers.same_rule((name, full), cur[:2]):
      return False
    self._set_optimizer(name, full)
    return True

  def _set_optimizer(self, name, full):
    v = optimizers.hp_vector(name, full)
    check(self.lib.smx_set_optimizer(self._h, optimizers.RULES[name][0], _fp(v), len(v)))

  def restore_optimizer(self, name: str, hp: Optional[dict], t0: int):
    """Set the rule with its state beginning at step t0 (a checkpoint's entries; the slots are restored by the caller).  hp None: the
    rule's defaults (a checkpoint from before the rules: Adam with the config's betas)."""
    if name == "adam" and hp is None:
      hp = dict(beta_1=self.cfg.adam_beta1, beta_2=self.cfg.adam_beta2, epsilon=self.cfg.adam_eps)
    name, full = optimizers.canonical(name, **(hp or {}))
    cur = self.get_optimizer()
    if optimizers.same_rule((name, full), cur[:2]) and cur[2] == int(t0):
      return
    step = self.step
    self.step = int(t0)   # (smx_set_optimizer records t0 = the step count at the call)
    try:
      self._set_optimizer(name, full)
    finally:
      self.step = step

  # ---- schedules -------------------------------------------------------------------
  def set_schedule(self, target: str, value):
    """The KL weight (target 'beta') or the learning rate ('lr') of the later training steps as a function of the step: a number or any
    schedule sisua_amd.interpolation accepts (smx_set_schedule).  'beta' is keyed by the model's step, 'lr' by step - t0.  ValueError
    for what is not built."""
    rec = interpolation.as_schedule(value, target)
    p = np.ascontiguousarray(rec.params, np.float64)
    check(self.lib.smx_set_schedule(self._h, _SCHED_TARGETS[target], rec.kind, p.ctypes.data_as(C.POINTER(C.c_double)), len(p)))
    return rec

  def get_schedule(self, target: str):
    """The schedule in force for 'beta' or 'lr' as an interpolation.Schedule record (const at the config's value by default)."""
    kind, n = C.c_int32(), C.c_int32()
    check(self.lib.smx_get_schedule(self._h, _SCHED_TARGETS[target], C.byref(kind), None, 0, C.byref(n)))
    p = np.zeros(max(n.value, 1), np.float64)
    check(self.lib.smx_get_schedule(self._h, _SCHED_TARGETS[target], C.byref(kind), p.ctypes.data_as(C.POINTER(C.c_double)), len(p),
                                    C.byref(n)))
    return interpolation.Schedule(kind.value, p[:n.value])

  @property
  def step(self) -> int:
    s = C.c_int32()
    check(self.lib.smx_get_step(self._h, C.byref(s)))
    return s.value

  @step.setter
  def step(self, value: int):
    check(self.lib.smx_set_step(self._h, int(value)))

  # ---- data ----------------------------------------------------------------------
  def upload(self, X, labels: Sequence[np.ndarray] = (), library=None, label_mask=None, cell_id_base: int = 0,
             storage: str = "f32"):
    """Make the cells x genes matrix resident in HBM.  storage='u16' keeps the counts as uint16 (half the bytes;
    integer counts <= 65535 only), storage='f32' is the reference's dense float32 layout, storage='csr' keeps the
    non-zeros only (8 bytes each; X may also be a (indptr, indices, data) triple or a scipy.sparse CSR matrix)."""
    if storage not in ("f32", "u16", "csr"):
      raise ValueError("storage must be 'f32', 'u16' or 'csr'")
    if storage == "csr":
      return self._upload_csr(X, labels, library, label_mask, cell_id_base)
    if _sparse(X):   # a dense store from sparse rows: expanded block by block on the device, never whole on the host
      return self._upload_csr(X, labels, library, label_mask, cell_id_base, dense_store=storage)
    if storage == "u16":
      Xf = np.asarray(X)
      _check_u16(Xf)
      X = np.ascontiguousarray(Xf, dtype=np.uint16)
    else:
      X = _f32(X)
    if X.ndim != 2 or X.shape[1] != self.cfg.n_genes:
      raise ValueError(f"X must be [n_cells, {self.cfg.n_genes}]")
    n = X.shape[0]
    keep, side = self._upload_side(n, labels, library, label_mask)
    if storage == "u16":
      check(self.lib.smx_dataset_upload_u16(self._h, X.ctypes.data_as(C.POINTER(C.c_uint16)), n, *side, int(cell_id_base)))
    else:
      check(self.lib.smx_dataset_upload(self._h, _fp(X), n, *side, int(cell_id_base)))
    self.n_cells = n

  def _upload_side(self, n, labels, library, label_mask):
    """The per-cell side arrays of an upload of n cells: (the arrays, their pointers (labels, library, label mask)); the caller keeps
    the arrays alive through the call."""
    labs = [_f32(y, (n, P)) for y, (P, _) in zip(labels, self.cfg.targets)]
    if len(labs) != len(self.cfg.targets):
      raise ValueError("one label matrix per label head is required")
    lib_arr = None if library is None else _f32(library, (n, 2))
    mask_arr = None if label_mask is None else np.ascontiguousarray(label_mask, dtype=np.uint8).reshape(n)
    mask_ptr = None if mask_arr is None else mask_arr.ctypes.data_as(C.POINTER(C.c_uint8))
    return (labs, lib_arr, mask_arr), (_fps(labs), _fp(lib_arr), mask_ptr)

  def _upload_csr(self, X, labels, library, label_mask, cell_id_base, dense_store=None):
    G = self.cfg.n_genes
    if isinstance(X, tuple) and len(X) == 3:
      indptr, indices, data = X
    elif hasattr(X, "tocsr"):   # scipy.sparse
      if X.shape[1] != G:
        raise ValueError(f"X must be [n_cells, {G}]")
      indptr, indices, data = _csr3(X, G)
    else:
      Xd = _f32(X)
      if Xd.ndim != 2 or Xd.shape[1] != G:
        raise ValueError(f"X must be [n_cells, {G}]")
      nz = Xd != 0
      indptr = np.concatenate([[0], np.cumsum(nz.sum(1))])
      indices = np.nonzero(nz)[1]
      data = Xd[nz]
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.float32)
    n = indptr.size - 1
    if n < 1 or indptr[0] != 0 or indptr[-1] != indices.size or indices.size != data.size:
      raise ValueError("inconsistent CSR arrays")
    keep, side = self._upload_side(n, labels, library, label_mask)
    if dense_store is not None:
      if dense_store == "u16":
        _check_u16(data)
      check(self.lib.smx_dataset_upload_csr_dense(self._h, *_csr_ptrs((indptr, indices, data)), n, *side, int(cell_id_base),
                                                  1 if dense_store == "u16" else 0))
    else:
      check(self.lib.smx_dataset_upload_csr(self._h, *_csr_ptrs((indptr, indices, data)), n, *side, int(cell_id_base)))
    self.n_cells = n

  # ---- steps -----------------------------------------------------------------------
  @staticmethod
  def _ids(row_ids):
    return np.ascontiguousarray(row_ids, dtype=np.int32).reshape(-1)

  def train_step(self, row_ids, graph: bool = False, metrics: bool = True):
    ids = self._ids(row_ids)
    m = smx_metrics()
    fn = self.lib.smx_train_step_graph if graph else self.lib.smx_train_step
    self._step_check(fn(self._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size, C.byref(m) if metrics else None))
    return m.as_dict() if metrics else None

  def train_steps(self, order, n_steps: int, batch: int, graph: bool = False, metrics: bool = False):
    """order = None: the row ids made resident by stage_steps(order, n_steps, batch) (no host-to-device copy in this call)."""
    if order is None:
      ptr = None
    else:
      ids = self._ids(order)
      if ids.size != n_steps * batch:
        raise ValueError("order must hold n_steps * batch row ids")
      ptr = ids.ctypes.data_as(C.POINTER(C.c_int32))
    m = smx_metrics()
    self._step_check(self.lib.smx_train_steps(self._h, ptr, int(n_steps), int(batch), int(graph), C.byref(m) if metrics else None))
    return m.as_dict() if metrics else None

  def _step_check(self, rc: int):
    """check() of a step's status; a failed collective of the hand-written exchange (SMX_ERR_COMM: a wait on a peer timed out, every rank's
    step is void) is reported ONCE -- the sticky error word is read and cleared here, so a caller that has dealt with the cause (ADVICE r04:
    it used to fail every later call until someone called comm_p2p_error) can go on: restore a checkpoint, re-attach the ranks."""
    try:
      check(rc)
    except SmxError as err:
      if getattr(err, "code", 0) == -4:
        try:
          self.last_comm_error = self.comm_p2p_error()   # (1: this rank's wait timed out, 2: a peer reported that its wait did)
        except SmxError:
          pass
      raise

  def stage_steps(self, order, n_steps: int, batch: int):
    """The next train_steps call's row ids, uploaded ahead of it (an input pipeline's prefetch)."""
    ids = self._ids(order)
    if ids.size != n_steps * batch:
      raise ValueError("order must hold n_steps * batch row ids")
    check(self.lib.smx_train_stage(self._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), int(n_steps), int(batch)))

  def metrics_history(self, n_steps: int) -> Dict[str, np.ndarray]:
    """Per-step ELBO scalars of the last train_steps call: dict of arrays [n_steps]."""
    h = np.empty((int(n_steps), 8), np.float32)
    check(self.lib.smx_metrics_history(self._h, int(n_steps), _fp(h)))
    return {k: h[:, i].copy() for i, k in enumerate(("loss", "nllk_x", "nllk_y", "kl", "kl_l", "tc", "dtc_loss", "nllk_o"))}

  def set_train_draws(self, n_draws: int):
    """Monte-Carlo draws per cell of the later train / eval steps (fit(sample_shape)): a step of B cells runs on n_draws x B
    stacked rows, draw s of every cell keyed by Philox sample index s on the draw side (latent draws, decoder dropout); the ELBO
    scalars are means over cells and draws (smx_set_train_draws)."""
    check(self.lib.smx_set_train_draws(self._h, int(n_draws)))

  def eval_step(self, row_ids):
    ids = self._ids(row_ids)
    m = smx_metrics()
    self._step_check(self.lib.smx_eval_step(self._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size, C.byref(m)))
    return m.as_dict()

  def _cells(self, row_ids, x, library):
    """The cells of a call: resident row ids, or host rows x [B, G] with their library prior [B, 2] (optional): (B, the arrays, their
    pointers (row ids, rows, library)); the caller keeps the arrays alive through the call."""
    if row_ids is not None:
      ids = self._ids(row_ids)
      return ids.size, (ids,), (ids.ctypes.data_as(C.POINTER(C.c_int32)), None, None)
    xa = _f32(x)
    la = None if library is None else _f32(library, (xa.shape[0], 2))
    return xa.shape[0], (xa, la), (None, _fp(xa), _fp(la))

  def _outputs(self, B: int, S: Optional[int] = None, want_x_params: bool = True, want=None):
    """The result arrays of a forward pass over B cells -- S: with a leading draw axis on z_sample / l_sample / x_params / y_params --
    and their pointers in the order of smx_forward's output arguments: (dict of arrays, pointers).  want: the names to allocate and ask
    for (of z_mean, z_scale, z_sample, l_mean, l_scale, l_sample, x_params, y_params); the others are None (NULL to the library, which
    then does not fetch them).  Default: all."""
    cfg = self.cfg
    D, G, k = cfg.latent_dim, cfg.n_genes, cfg.k
    lead = () if S is None else (S,)
    w = (lambda name: True) if want is None else (lambda name: name in want)
    new = lambda name, shape: np.empty(shape, np.float32) if w(name) else None
    out = dict(z_mean=new("z_mean", (B, D)), z_sample=new("z_sample", lead + (B, D)))
    out["z_scale"] = new("z_scale", (B, D)) if cfg.stochastic else None
    zs = out["z_scale"]
    if cfg.latent_tril and zs is not None:   # the full-covariance posterior: the device hands back the factor L [B, D, D]; z_scale = its marginal stddevs (_tril_scale)
      out["scale_tril"] = zs = np.empty((B, D, D), np.float32)
    if cfg.model == "scvi":
      out.update(l_mean=new("l_mean", (B,)), l_scale=new("l_scale", (B,)), l_sample=new("l_sample", lead + (B,)))
    out["x_params"] = new("x_params", lead + (k, B, G)) if want_x_params else None
    out["y_params"] = [np.empty(lead + (B, label_planes(llk, P) * P), np.float32) for P, llk in cfg.head_labels] if w("y_params") else []
    return out, (_fp(out["z_mean"]), _fp(zs), _fp(out["z_sample"]), _fp(out.get("l_mean")), _fp(out.get("l_scale")),
                 _fp(out.get("l_sample")), _fp(out["x_params"]), _fps(out["y_params"]))

  def forward(self, row_ids=None, x=None, library=None, sample_index: int = 0, training: bool = False,
              want_x_params: bool = True):
    """Eval-mode forward; returns dict of logical-shape arrays."""
    B, keep, cells = self._cells(row_ids, x, library)
    out, res = self._outputs(B, want_x_params=want_x_params)
    check(self.lib.smx_forward(self._h, *cells, B, int(sample_index), int(training), *res))
    return _tril_scale(out)

  def forward_samples(self, n_samples: int, row_ids=None, x=None, library=None):
    """n_samples Monte-Carlo draws of one batch in one call (the encoders run once): arrays with a leading draw axis
    for z_sample / l_sample / x_params / y_params, one copy of the posterior means and scales."""
    S = int(n_samples)
    B, keep, cells = self._cells(row_ids, x, library)
    out, res = self._outputs(B, S)
    check(self.lib.smx_forward_samples(self._h, *cells, B, S, *res))
    return _tril_scale(out)

  def predict(self, x, library=None, n_samples: int = 1, batch: Optional[int] = None, want_x_params: bool = True, want=None):
    """Eval-mode forward of a whole host matrix in one call (smx_predict): arrays over ALL cells, with a leading draw
    axis for z_sample / l_sample / x_params / y_params -- the layout of forward_samples with n = every cell.
    want_x_params=False: everything but the gene output's parameter planes (what a lazy result keeps on the device side).
    want: only the named outputs leave the device (see `_outputs`; the clustering scores ask for the latent means alone).
    x may be scipy.sparse (smx_predict_csr: the same results bit for bit)."""
    cfg = self.cfg
    xa = _csr3(x, cfg.n_genes) if _sparse(x) else _f32(x)
    N, S = (xa[0].size - 1 if isinstance(xa, tuple) else xa.shape[0]), int(n_samples)
    B = min(int(batch or self.max_batch), self.max_batch)
    la = None if library is None else _f32(library, (N, 2))
    out, res = self._outputs(N, S, want_x_params and (want is None or "x_params" in want), want)
    if isinstance(xa, tuple):
      check(self.lib.smx_predict_csr(self._h, *_csr_ptrs(xa), _fp(la), N, B, S, *res))
    else:
      check(self.lib.smx_predict(self._h, _fp(xa), _fp(la), N, B, S, *res))
    return _tril_scale(out)

  STATS = {"mean": 0, "variance": 1, "mean_over_samples": 2, "log_prob": 3, "sample": 4}

  def predict_stat(self, x, stat: str, library=None, n_samples: int = 1, batch: Optional[int] = None, count_only: bool = False,
                   target=None, out=None, seed: int = 0, n: int = 1, genes=None):
    """A statistic of the gene output over a whole host matrix (smx_predict_stat): the same passes and draws as predict(), but only the
    statistic leaves the device.  'mean' / 'variance' [n_samples, N, G]; 'mean_over_samples' [N, G]; 'log_prob' [n_samples, N] of `target`
    (default: of x itself).  count_only: the count distribution without the zero-inflation wrapper.  `out`: a float32 array of the
    result's shape to write into (a reused array saves the first-touch page faults of a fresh one).  x and target may be scipy.sparse
    (smx_predict_stat_csr).  'sample': [n, n_samples, N, G], n posterior-predictive draws of the gene output per Monte-Carlo draw and cell
    under the integer `seed` (smx_predict_sample / _csr: drawn on the device, the same bits at any batch size and from dense or sparse x).
    genes ('mean_over_samples' only): gene indices -- [N, len(genes)] leaves the device, the same bits as those columns (smx_predict_stat_cols)."""
    cfg = self.cfg
    if genes is not None:
      return self._predict_stat_cols(x, stat, library, n_samples, batch, count_only, target, out, genes)
    xa = _csr3(x, cfg.n_genes) if _sparse(x) else _f32(x)
    N, S, G = (xa[0].size - 1 if isinstance(xa, tuple) else xa.shape[0]), int(n_samples), cfg.n_genes
    B = min(int(batch or self.max_batch), self.max_batch)
    la = None if library is None else _f32(library, (N, 2))
    code = self.STATS[stat]
    shape = (N, G) if code == 2 else (S, N) if code == 3 else (int(n), S, N, G) if code == 4 else (S, N, G)
    if code == 4 and (int(n) < 1 or target is not None):
      raise ValueError("'sample' takes n >= 1 and no target")
    if out is None:
      out = np.empty(shape, np.float32)
    elif out.dtype != np.float32 or tuple(out.shape) != shape or not out.flags.c_contiguous:
      raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
    if code == 4:
      sd = int(seed) & 0xFFFFFFFFFFFFFFFF
      if isinstance(xa, tuple):
        check(self.lib.smx_predict_sample_csr(self._h, *_csr_ptrs(xa), _fp(la), N, B, S, int(bool(count_only)), sd, int(n), _fp(out)))
      else:
        check(self.lib.smx_predict_sample(self._h, _fp(xa), _fp(la), N, B, S, int(bool(count_only)), sd, int(n), _fp(out)))
      return out
    tc = _csr3(target, G, N) if (target is not None and _sparse(target)) else None
    ta = None if (target is None or tc is not None) else _f32(target, (N, G))
    if isinstance(xa, tuple) or tc is not None:
      if not isinstance(xa, tuple):   # (a dense input with a CSR target: the CSR entry point takes both)
        import scipy.sparse as sp
        xa = _csr3(sp.csr_matrix(xa), G)
      xc = xa
      tp = _csr_ptrs(tc) if tc is not None else (None, None, None)
      check(self.lib.smx_predict_stat_csr(self._h, *_csr_ptrs(xc), _fp(la), N, B, S, code, int(bool(count_only)), _fp(ta), *tp, _fp(out)))
    else:
      check(self.lib.smx_predict_stat(self._h, _fp(xa), _fp(la), N, B, S, code, int(bool(count_only)), _fp(ta), _fp(out)))
    return out

  def _predict_stat_cols(self, x, stat, library, n_samples, batch, count_only, target, out, genes):
    cfg = self.cfg
    if stat != "mean_over_samples" or target is not None:
      raise ValueError("genes= goes with 'mean_over_samples' (and no target)")
    idx = gene_indices(genes, cfg.n_genes)
    xa = _csr3(x, cfg.n_genes) if _sparse(x) else _f32(x)
    N, S = (xa[0].size - 1 if isinstance(xa, tuple) else xa.shape[0]), int(n_samples)
    B = min(int(batch or self.max_batch), self.max_batch)
    la = None if library is None else _f32(library, (N, 2))
    shape = (N, idx.size)
    if out is None:
      out = np.empty(shape, np.float32)
    elif out.dtype != np.float32 or tuple(out.shape) != shape or not out.flags.c_contiguous:
      raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    if isinstance(xa, tuple):
      check(self.lib.smx_predict_stat_cols_csr(self._h, *_csr_ptrs(xa), _fp(la), N, B, S, int(bool(count_only)), ip, idx.size, _fp(out)))
    else:
      check(self.lib.smx_predict_stat_cols(self._h, _fp(xa), _fp(la), N, B, S, int(bool(count_only)), ip, idx.size, _fp(out)))
    return out

  def predict_impute(self, x, original, library=None, n_samples: int = 1, batch: Optional[int] = None, count_only: bool = False):
    """The imputation scores of predict_stat(x, 'mean_over_samples') against `original`, reduced on the device (smx_predict_impute): x is
    the CORRUPTED matrix the prediction is made from.  Returns dict(cell_median [N] float32: np.median(|original - mean|) of every cell;
    cell_changed [N] int32: sum(original row) != sum(x row); global_lohi [2] float32: the two middle order statistics of all N G absolute
    differences).  x and original may each be scipy.sparse; the bits do not depend on that, on the batch size or on the chunking."""
    cfg = self.cfg
    G = cfg.n_genes
    xa = _csr3(x, G) if _sparse(x) else _f32(x)
    N, S = (xa[0].size - 1 if isinstance(xa, tuple) else xa.shape[0]), int(n_samples)
    if not isinstance(xa, tuple) and (xa.ndim != 2 or xa.shape[1] != G):
      raise ValueError(f"expected rows [n_cells, {G}], got {xa.shape}")
    if original is None:
      raise ValueError("predict_impute needs the original counts")
    oc = _csr3(original, G, N) if _sparse(original) else None
    oa = None if oc is not None else _f32(original, (N, G))
    B = min(int(batch or self.max_batch), self.max_batch)
    la = None if library is None else _f32(library, (N, 2))
    med, chg, lohi = np.empty((N,), np.float32), np.empty((N,), np.int32), np.empty((2,), np.float32)
    res = (_fp(med), chg.ctypes.data_as(C.POINTER(C.c_int32)), _fp(lohi))
    if isinstance(xa, tuple) or oc is not None:
      xp = (None,) + _csr_ptrs(xa) if isinstance(xa, tuple) else (_fp(xa), None, None, None)
      op = _csr_ptrs(oc) if oc is not None else (None, None, None)
      check(self.lib.smx_predict_impute_csr(self._h, *xp, _fp(la), N, B, S, int(bool(count_only)), _fp(oa), *op, *res))
    else:
      check(self.lib.smx_predict_impute(self._h, _fp(xa), _fp(la), N, B, S, int(bool(count_only)), _fp(oa), *res))
    return dict(cell_median=med, cell_changed=chg, global_lohi=lohi)

  def predict_correlate(self, x, prot_rank2, prot_unit, library=None, n_samples: int = 1, batch: Optional[int] = None, count_only: bool = False,
                        genes=None):
    """The correlation sums of predict_stat(x, 'mean_over_samples') against P prepared protein columns, reduced on the device
    (smx_predict_correlate): prot_rank2 [P, N] int32 (doubled average ranks), prot_unit [P, N] float64 (centred, unit norm).  Returns
    dict(sp_Sa, sp_Saa [G'] int64, sp_Sab [G', P] int64, pe_mean, pe_Sxx [G'] float64, pe_Sxy [G', P] float64, nonfinite [G'] int32) for
    the genes asked for (None: all) -- `distributions.correlations_from_sums` closes them.  x may be scipy.sparse; the bits do not depend
    on that, on the batch size or on the chunking.  More than 2^20 cells: the library refuses (SmxError)."""
    cfg = self.cfg
    G = cfg.n_genes
    xa = _csr3(x, G) if _sparse(x) else _f32(x)
    N, S = (xa[0].size - 1 if isinstance(xa, tuple) else xa.shape[0]), int(n_samples)
    if not isinstance(xa, tuple) and (xa.ndim != 2 or xa.shape[1] != G):
      raise ValueError(f"expected rows [n_cells, {G}], got {xa.shape}")
    idx = None if genes is None else gene_indices(genes, G)
    pr, pu = _col_operands(prot_rank2, prot_unit, N)
    B = min(int(batch or self.max_batch), self.max_batch)
    la = None if library is None else _f32(library, (N, 2))
    out, res = _col_outputs(G if idx is None else idx.size, pr.shape[0])
    sel = (None, 0) if idx is None else (_ip(idx), idx.size)
    if isinstance(xa, tuple):
      check(self.lib.smx_predict_correlate_csr(self._h, *_csr_ptrs(xa), _fp(la), N, B, S, int(bool(count_only)), *sel, _ip(pr), _dp(pu), pr.shape[0], *res))
    else:
      check(self.lib.smx_predict_correlate(self._h, _fp(xa), _fp(la), N, B, S, int(bool(count_only)), *sel, _ip(pr), _dp(pu), pr.shape[0], *res))
    return out

  def decode(self, z, l=None):
    """Decoder + output heads from given latents (eval mode)."""
    cfg = self.cfg
    za = _f32(z)
    B = za.shape[0]
    if za.shape[1] != cfg.latent_dim:
      raise ValueError(f"z must be [batch, {cfg.latent_dim}]")
    la = None if l is None else _f32(np.reshape(l, (B,)))
    xp = np.empty((cfg.k, B, cfg.n_genes), np.float32)
    ys = [np.empty((B, label_planes(llk, P) * P), np.float32) for P, llk in cfg.head_labels]
    check(self.lib.smx_decode(self._h, _fp(za), _fp(la), B, _fp(xp), _fps(ys)))
    return dict(x_params=xp, y_params=ys)

  def marginal_llk(self, row_ids=None, x=None, library=None, n_samples: int = 100):
    """Importance-weighted log p(x) per cell and the mean reconstruction log-likelihood (GPU).  x may be scipy.sparse
    (smx_marginal_llk_csr)."""
    if row_ids is None and _sparse(x):
      xc = _csr3(x, self.cfg.n_genes)
      B = xc[0].size - 1
      la = None if library is None else _f32(library, (B, 2))
      mllk, llk = np.empty(B, np.float32), np.empty(B, np.float32)
      check(self.lib.smx_marginal_llk_csr(self._h, *_csr_ptrs(xc), _fp(la), B, int(n_samples), _fp(mllk), _fp(llk)))
      return mllk, llk
    B, keep, cells = self._cells(row_ids, x, library)
    mllk, llk = np.empty(B, np.float32), np.empty(B, np.float32)
    check(self.lib.smx_marginal_llk(self._h, *cells, B, int(n_samples), _fp(mllk), _fp(llk)))
    return mllk, llk

  # ---- resident-matrix preprocessing ---------------------------------------
  def generate_lognormal(self, n_cells: int, seed: int = 8, rank: int = 0, storage: str = "u16", density: float = 0.14):
    """The rank's shard of BASELINE configs[4] generated on the device (smx_dataset_generate_lognormal): nothing crosses
    PCIe; rows are those of one virtual matrix keyed by the global cell id rank * n_cells + row."""
    if storage not in ("u16", "f32"):
      raise ValueError("storage must be 'u16' or 'f32'")
    check(self.lib.smx_dataset_generate_lognormal(self._h, int(seed), int(rank), int(n_cells), 1 if storage == "u16" else 0, float(density)))
    self.n_cells = int(n_cells)

  def dataset_library(self):
    """get_library_size (data/utils.py:231-263) over the resident matrix on the GPU; fills the resident
    library prior and returns (local_mean, local_var)."""
    st = np.zeros(2, np.float32)
    check(self.lib.smx_dataset_library(self._h, _fp(st)))
    return float(st[0]), float(st[1])

  def dataset_corrupt(self, dropout_rate: float = 0.2, retain_rate: float = 0.2, seed: int = 8) -> int:
    """'binomial' artificial corruption (data/utils.py:168-228) in place on the resident matrix with the
    counter RNG (oracle: corrupt_philox).  Returns the number of corrupted entries."""
    n = C.c_int64(0)
    check(self.lib.smx_dataset_corrupt(self._h, float(dropout_rate), float(retain_rate), int(seed), C.byref(n)))
    return int(n.value)

  def dataset_read(self, row0: int = 0, n_rows: int = None, library: bool = False):
    """Rows of the resident matrix, their constants sum_g lgamma(x+1), and optionally the library prior."""
    n = int(self.lib.smx_dataset_size(self._h)) - int(row0) if n_rows is None else int(n_rows)
    X = np.empty((n, self.cfg.n_genes), np.float32)
    rc = np.empty(n, np.float32)
    lb = np.empty((n, 2), np.float32) if library else None
    check(self.lib.smx_dataset_read(self._h, int(row0), n, _fp(X), _fp(rc), _fp(lb) if library else None))
    return (X, rc, lb) if library else (X, rc)

  def score_llk(self, targets, row_ids=None, x=None, library=None, n_samples: int = 10):
    """Posterior-predictive log-likelihood per cell (Posterior.cal_llk, posterior.py:919-938), on the GPU.
    `targets`: list of [B, G] matrices (None = the input cells).  Returns [len(targets), 2, B]:
    [:, 0] under the output distribution, [:, 1] under its count distribution without zero inflation.
    x and the targets may be scipy.sparse: a call holds one batch (<= max_batch rows), densified here as a row block."""
    if _sparse(x):
      x = x.toarray()
    targets = [t.toarray() if _sparse(t) else t for t in targets]
    B, cells_keep, cells = self._cells(row_ids, x, library)
    keep = [None if t is None else _f32(t, (B, self.cfg.n_genes)) for t in targets]
    arr = (C.POINTER(C.c_float) * len(keep))(*[_fp(t) if t is not None else C.POINTER(C.c_float)() for t in keep])
    out = np.empty((len(keep), 2, B), np.float32)
    check(self.lib.smx_score_llk(self._h, *cells, arr, len(keep), B, int(n_samples), _fp(out)))
    return out

  # ---- noise injection (parity tests) ----------------------------------------------
  def set_noise(self, stream: int, data):
    a = _f32(data)
    if a.ndim == 1:
      a = a.reshape(-1, 1)
    check(self.lib.smx_set_noise(self._h, int(stream), _fp(a), a.shape[0], a.shape[1]))

  def clear_noise(self):
    check(self.lib.smx_clear_noise(self._h))

  # ---- data parallel ------------------------------------------------------------------
  @staticmethod
  def comm_unique_id() -> bytes:
    lib = _hip.load()
    buf = (C.c_uint8 * 128)()
    check(lib.smx_comm_unique_id(buf))
    return bytes(buf)

  def comm_init(self, rank: int, world: int, uid: bytes):
    buf = (C.c_uint8 * 128).from_buffer_copy(uid)
    check(self.lib.smx_comm_init(self._h, int(rank), int(world), buf))

  def comm_p2p_export(self, world: int) -> bytes:
    """This rank's two IPC handles (flat gradient buffer | communication region) for the hand-written two-shot all-reduce
    over peer-mapped buffers (smx_comm_p2p_export); gather every rank's 128 bytes in rank order, then comm_p2p_init."""
    buf = (C.c_uint8 * 128)()
    check(self.lib.smx_comm_p2p_export(self._h, int(world), buf))
    return bytes(buf)

  def comm_p2p_init(self, rank: int, world: int, all_handles: bytes):
    if len(all_handles) != 128 * world:
      raise ValueError("all_handles must hold world x 128 bytes in rank order")
    buf = (C.c_uint8 * len(all_handles)).from_buffer_copy(all_handles)
    check(self.lib.smx_comm_p2p_init(self._h, int(rank), int(world), buf))

  def comm_p2p_error(self) -> int:
    """Non-zero after a wait on a peer timed out in the peer-to-peer exchange (cleared by the call)."""
    e = C.c_int32(0)
    check(self.lib.smx_comm_p2p_error(self._h, C.byref(e)))
    return int(e.value)

  def comm_time_allreduce(self, iters: int = 50):
    """(microseconds per all-reduce of the flat gradient buffer ALONE, its bytes), through the path the steps take (every rank calls it)."""
    us, n = C.c_float(0.0), C.c_int64(0)
    check(self.lib.smx_comm_time_allreduce(self._h, int(iters), C.byref(us), C.byref(n)))
    return float(us.value), 4 * int(n.value)

  @property
  def world(self) -> int:
    return self.lib.smx_comm_world(self._h)

  @property
  def rank(self) -> int:
    return self.lib.smx_comm_rank(self._h)

  @property
  def comm_form(self) -> int:
    """How a training step exchanges its gradients: 0 no collective, 1 one all-reduce, 2 the two-bucket chain (the heads' bucket reduced,
    normed and applied on the communication stream), 3 the hand-written exchange (one launch per all-reduce), 4 its two-bucket form of
    round 4 (include/sisua_hip.h: smx_comm_form)."""
    return self.lib.smx_comm_form(self._h)

  FORM_NAMES = {0: "none", 1: "one all-reduce", 2: "two-bucket chain", 3: "hand-written exchange", 4: "hand-written exchange, two buckets"}

  def comm_set_form(self, form: int):
    """Ask for an exchange form (smx_comm_set_form: 1 / 2 / 3, or 0 = the library's rule).  A collective call for form 2: every rank."""
    check(self.lib.smx_comm_set_form(self._h, int(form)))

  def opt_gather(self):
    """Flag opt_shard: all-gather the heads' Adam moments (a collective: every rank calls it, between training calls); afterwards
    get_params(2 | 3) returns the job's moments on every rank (include/sisua_hip.h: smx_opt_gather)."""
    check(self.lib.smx_opt_gather(self._h))

  def set_sync_bn(self, on: bool = True):
    """SyncBatchNorm under data parallelism (global-batch statistics; one small extra all-reduce per BatchNorm pass)."""
    check(self.lib.smx_comm_set_sync_bn(self._h, int(bool(on))))

  @staticmethod
  def comm_library() -> dict:
    """Paths of the bound RCCL and of the HIP runtime both libraries run on, and the RCCL version code."""
    lib = _hip.load()
    a, b, v = C.create_string_buffer(4096), C.create_string_buffer(4096), C.c_int32()
    check(lib.smx_comm_library(a, 4096, b, 4096, C.byref(v)))
    return dict(rccl=a.value.decode(), hip=b.value.decode(), rccl_version=int(v.value))

  @staticmethod
  def comm_init_local(engines: Sequence["Engine"]):
    """Test hook: loopback communicator over engines of this process (rank i = engines[i]); afterwards each engine
    must be driven by its own host thread, all of them running the same number of equal-size steps."""
    lib = _hip.load()
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    check(lib.smx_comm_init_local(arr, len(engines)))

  def set_flag(self, name: str, value: bool):
    """Code-path switch (smx_set_flag).  Training step: head_loss, head_fused, head_sweep, front, bwd_front, head_bwd, wgrad, scvi_fused, twin, label_ride,
    act_epilogue; data parallel: opt_shard (the heads' optimiser state sharded over the ranks; opt_gather()); scoring: stacked_scoring; "bf16x3" (products of the output head from bf16 MFMAs on three-way split operands):
    True / False, or -1 for the default (by the head's width)."""
    v = -1 if (name == "bf16x3" and not isinstance(value, bool) and int(value) < 0) else int(bool(value))
    check(self.lib.smx_set_flag(self._h, name.encode(), v))

  # ---- padding audit (tests) ---------------------------------------------------------------
  def pad_audit(self, which: int):
    """Elements outside the logical extent of the tensors that are not exactly zero (smx_pad_audit): which 0 parameters, 1 gradients,
    2 / 3 the optimiser's slots, 4 the work buffers of the last pass.  Returns (n_bad, name of the first offender or None, its offset)."""
    n, t, off = C.c_int64(0), C.c_int32(-1), C.c_int64(-1)
    name = C.create_string_buffer(64)
    check(self.lib.smx_pad_audit(self._h, int(which), C.byref(n), C.byref(t), C.byref(off), name, 64))
    return int(n.value), (name.value.decode() if n.value else None), int(off.value)

  def pad_poke(self, which: int, tensor, value: float = 1.0):
    """Write `value` into the first padded element of a tensor (name or index) of buffer `which` (smx_pad_poke); SmxError when the tensor
    has no padding.  Exists to show that pad_audit sees a violation."""
    index = self.index[tensor] if isinstance(tensor, str) else int(tensor)
    check(self.lib.smx_pad_poke(self._h, int(which), index, float(value)))

  # ---- measurement ----------------------------------------------------------------------
  def timing_enable(self, kernel: Optional[str]):
    check(self.lib.smx_timing_enable(self._h, kernel.encode() if kernel else None))

  def timing_read(self):
    ms, n = C.c_double(), C.c_int64()
    check(self.lib.smx_timing_read(self._h, C.byref(ms), C.byref(n)))
    return ms.value, n.value

  def loss_bytes_per_cell(self) -> int:
    return int(self.lib.smx_loss_bytes_per_cell(self._h))

  def head_fused_bytes(self, batch: int) -> int:
    """Algorithmic bytes of one launch of the fused output head when a training step of `batch` cells takes it, else 0."""
    return int(self.lib.smx_head_fused_bytes(self._h, int(batch)))

  def head_dw_late(self) -> bool:
    """The last training step left the output head's dW / db to the decoder's BatchNorm-backward launch (smx_head_dw_late)."""
    return bool(self.lib.smx_head_dw_late(self._h))

  def bwd_seam_steps(self) -> int:
    """Steps of the last train_steps call that ran the decoder's and the encoder's BatchNorm-backward launches as one launch (smx_bwd_seam_steps)."""
    return int(self.lib.smx_bwd_seam_steps(self._h))

  def lazy_adam_steps(self) -> int:
    """Steps of the last train_steps call whose optimiser launch was left to the next step's forward launches (smx_lazy_adam_steps)."""
    return int(self.lib.smx_lazy_adam_steps(self._h))

  def synchronize(self):
    check(self.lib.smx_synchronize())


# ---- kernel-level helpers (tests) -----------------------------------------------------
def k_count_llk(likelihood: str, x, planes, direct: bool = False, want_grads: bool = True):
  lib = _hip.require_gpu()
  x = _f32(x)
  B, G = x.shape
  pl = _f32(planes)
  k = pl.shape[0]
  llk = np.empty(B, np.float32)
  grads = np.empty((k, B, G), np.float32) if want_grads else None
  check(lib.smx_k_count_llk(_hip.LIKELIHOODS[likelihood], int(direct), _fp(x), _fp(pl), B, G, _fp(llk), _fp(grads)))
  return llk, grads


def k_head_fused(likelihood: str, x, d, W, bias, grad_scale: float = 1.0, u16: bool = False, reps: int = 0):
  """The fused output head (smx_headfused.hip) over host arrays: x [B][G], d [B][128], W [128][k][G], bias [k][G] ->
  dict(llk [B], dW, db, dd [B][128], sumsq, us)."""
  lib = _hip.require_gpu()
  x, d, W, bias = _f32(x), _f32(d), _f32(W), _f32(bias)
  B, G = x.shape
  k = W.shape[1]
  assert d.shape == (B, 128) and W.shape == (128, k, G) and bias.shape == (k, G)
  llk = np.empty(B, np.float32)
  dW, db, dd = np.empty((128, k, G), np.float32), np.empty((k, G), np.float32), np.empty((B, 128), np.float32)
  sumsq, us = np.zeros(1, np.float32), np.zeros(1, np.float32)
  check(lib.smx_k_head_fused(_hip.LIKELIHOODS[likelihood], int(u16), _fp(x), _fp(d), _fp(W), _fp(bias), B, G, float(grad_scale), int(reps),
                             _fp(llk), _fp(dW), _fp(db), _fp(dd), _fp(sumsq), _fp(us)))
  return dict(llk=llk, dW=dW, db=db, dd=dd, sumsq=float(sumsq[0]), us=float(us[0]))


def k_head_fused_stress(likelihood: str, x, d, W, bias, launches: int, grad_scale: float = 1.0, u16: bool = False):
  """`launches` launches of the fused output head on the same inputs, each compared bit for bit on the device with the first:
  (launches that differed, index of the first differing output word or -1)."""
  lib = _hip.require_gpu()
  x, d, W, bias = _f32(x), _f32(d), _f32(W), _f32(bias)
  B, G = x.shape
  k = W.shape[1]
  assert d.shape == (B, 128) and W.shape == (128, k, G) and bias.shape == (k, G)
  n, first = C.c_int32(0), C.c_int64(-1)
  check(lib.smx_k_head_fused_stress(_hip.LIKELIHOODS[likelihood], int(u16), _fp(x), _fp(d), _fp(W), _fp(bias), B, G, float(grad_scale), int(launches),
                                    C.byref(n), C.byref(first)))
  return int(n.value), int(first.value)


def k_adam(params, grads, m, v, step: int, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, clipnorm=100.0):
  """The optimiser launch by itself over lists of arrays (updated copies are returned): (params, m, v, norms)."""
  lib = _hip.require_gpu()
  sizes = np.array([int(np.size(p)) for p in params], dtype=np.int32)
  cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).ravel() for x in xs]))
  P, G, M, V = cat(params), cat(grads), cat(m), cat(v)
  norms = np.empty(len(sizes), np.float32)
  check(lib.smx_k_adam(len(sizes), sizes.ctypes.data_as(C.POINTER(C.c_int32)), _fp(P), _fp(G), _fp(M), _fp(V), int(step),
                       float(lr), float(beta1), float(beta2), float(eps), float(clipnorm), _fp(norms)))
  cut = np.cumsum(sizes)[:-1]
  shp = [np.shape(p) for p in params]
  un = lambda flat: [a.reshape(sh) for a, sh in zip(np.split(flat, cut), shp)]
  return un(P), un(M), un(V), norms


def k_opt(rule: str, params, grads, m, v, step: int, lr=1e-3, clipnorm=100.0, **hp):
  """The optimiser launch by itself under any rule of Engine.set_optimizer (smx_k_opt); m / v are the rule's slots 2 / 3.  Updated copies
  are returned: (params, m, v, norms)."""
  lib = _hip.require_gpu()
  name, full = optimizers.canonical(rule, **hp)
  hv = optimizers.hp_vector(name, full)
  sizes = np.array([int(np.size(p)) for p in params], dtype=np.int32)
  cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).ravel() for x in xs]))
  P, G, M, V = cat(params), cat(grads), cat(m), cat(v)
  norms = np.empty(len(sizes), np.float32)
  check(lib.smx_k_opt(optimizers.RULES[name][0], _fp(hv), len(hv), len(sizes), sizes.ctypes.data_as(C.POINTER(C.c_int32)), _fp(P), _fp(G),
                      _fp(M), _fp(V), int(step), float(lr), float(clipnorm), _fp(norms)))
  cut = np.cumsum(sizes)[:-1]
  shp = [np.shape(p) for p in params]
  un = lambda flat: [a.reshape(sh) for a, sh in zip(np.split(flat, cut), shp)]
  return un(P), un(M), un(V), norms


OPT_CARRIERS = {"launch": 0, "sweep": 1, "shard": 2, "body512": 3}   # smx_opt_carrier


def k_opt_carrier(rule: str, params, grads, m, v, step: int, carrier="launch", wgs=0, world=0, use_sq=False, sq=None, lr=1e-3, clipnorm=100.0,
                  grad_scale=1.0, t0=0, tied=(), tied_inv=1.0, hp_raw=None, **hp):
  """Clip + update by one of the launches that carry the optimiser's chunk body (smx_k_opt_carrier): the optimiser launch, the background
  sweep with `wgs` workgroups, the sharded chain of `world` simulated ranks, the 512-thread body.  Lists of arrays as k_opt's.  `use_sq`: the
  norms without the norm pass -- `sq[i]` holds tensor i's sum-of-squares slots, or None for the sweep of its own gradient (what lies behind a
  tensor's slots in the device array is NaN).  `tied`: up to two tensor indices whose sum of squares is multiplied by `tied_inv`.  `hp_raw`: a
  hyper-parameter vector handed to the library as it is, in place of **hp.  Returns dict(params, m, v: the whole padded flat buffers;
  offsets, sizes, pads: where tensor i lies in them; norms; lr_t: the device's step size; guards_ok; unused_ok)."""
  lib = _hip.require_gpu()
  if hp_raw is None:
    name, full = optimizers.canonical(rule, **hp)
    hv = optimizers.hp_vector(name, full)
  else:
    name, hv = rule.lower(), np.ascontiguousarray(hp_raw, dtype=np.float32)
  sizes = np.array([int(np.size(p)) for p in params], dtype=np.int32)
  pads = (sizes.astype(np.int64) + 63) // 64 * 64
  offsets = np.concatenate([[0], np.cumsum(pads)[:-1]])
  total = int(pads.sum())
  cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).ravel() for x in xs]))
  P, G, M, V = cat(params), cat(grads), cat(m), cat(v)
  first, count, slots = np.zeros(len(sizes), np.int32), np.zeros(len(sizes), np.int32), [np.full(8, np.nan, np.float32)]
  for i, s in enumerate(sq or []):
    if s is not None:
      first[i], count[i] = sum(len(x) for x in slots), np.size(s)
      slots += [np.asarray(s, np.float32).ravel(), np.full(8, np.nan, np.float32)]
  slots = np.ascontiguousarray(np.concatenate(slots))
  tied = list(tied) + [-1, -1]
  ip = np.array([optimizers.RULES[name][0], len(sizes), OPT_CARRIERS[carrier], wgs, world, int(bool(use_sq)), step, t0, tied[0], tied[1], len(slots)], np.int32)
  fp = np.array([lr, clipnorm, grad_scale, tied_inv], np.float32)
  o = dict(params=np.empty(total, np.float32), m=np.empty(total, np.float32), v=np.empty(total, np.float32), norms=np.empty(len(sizes), np.float32),
           offsets=offsets, sizes=sizes.astype(np.int64), pads=pads)
  lr_t, ok, same = C.c_float(0), C.c_int32(0), C.c_int32(0)
  check(lib.smx_k_opt_carrier(_ip(ip), _fp(fp), _fp(hv), len(hv), _ip(sizes), _fp(P), _fp(G), _fp(M), _fp(V), _ip(first), _ip(count), _fp(slots),
                              _fp(o["params"]), _fp(o["m"]), _fp(o["v"]), _fp(o["norms"]), C.byref(lr_t), C.byref(ok), C.byref(same)))
  o.update(lr_t=np.float32(lr_t.value), guards_ok=bool(ok.value), unused_ok=bool(same.value))
  return o


def k_gemm(A, B, trans_a=False, trans_b=False, split_k=1, tile=0):
  lib = _hip.require_gpu()
  A, B = _f32(A), _f32(B)
  M, K = (A.shape[1], A.shape[0]) if trans_a else A.shape
  N = B.shape[0] if trans_b else B.shape[1]
  Cm = np.empty((M, N), np.float32)
  check(lib.smx_k_gemm(int(trans_a), int(trans_b), _fp(A), _fp(B), M, N, K, int(split_k), int(tile), _fp(Cm)))
  return Cm


def k_row_select(rows, n_genes: Optional[int] = None):
  """smx_k_row_select: the two middle order statistics of the first n_genes entries of every row of `rows` [n, ld] (non-negative or NaN) -> (lo, hi) [n]"""
  lib = _hip.require_gpu()
  r = _f32(rows)
  n, ld = r.shape
  G = ld if n_genes is None else int(n_genes)
  lo, hi = np.empty((n,), np.float32), np.empty((n,), np.float32)
  check(lib.smx_k_row_select(_fp(r), n, G, ld, _fp(lo), _fp(hi)))
  return lo, hi


def _ip(a):
  return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dp(a):
  return a.ctypes.data_as(C.POINTER(C.c_double))


def _col_operands(prot_rank2, prot_unit, N):
  pr, pu = np.ascontiguousarray(prot_rank2, dtype=np.int32), np.ascontiguousarray(prot_unit, dtype=np.float64)
  if pr.ndim != 2 or pr.shape[0] < 1 or pr.shape[1] != N or pu.shape != pr.shape:
    raise ValueError(f"prot_rank2 and prot_unit must both be [P >= 1, {N}], got {pr.shape} and {pu.shape}")
  return pr, pu


def _col_outputs(n, P):
  """The result arrays of the correlation sums for n genes and P proteins, and their pointers in the order of smx_predict_correlate's outputs"""
  out = dict(sp_Sa=np.empty((n,), np.int64), sp_Saa=np.empty((n,), np.int64), sp_Sab=np.empty((n, P), np.int64),
             pe_mean=np.empty((n,), np.float64), pe_Sxx=np.empty((n,), np.float64), pe_Sxy=np.empty((n, P), np.float64),
             nonfinite=np.empty((n,), np.int32))
  lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
  return out, (lp(out["sp_Sa"]), lp(out["sp_Saa"]), lp(out["sp_Sab"]), _dp(out["pe_mean"]), _dp(out["pe_Sxx"]), _dp(out["pe_Sxy"]),
               _ip(out["nonfinite"]))


def k_col_rank2(cols):
  """smx_k_col_rank2: cols [n_cols, N] (gene-major) -> (rank2 [n_cols, N] int32 = 2 x the average ranks of every column, nonfinite [n_cols] int32)"""
  lib = _hip.require_gpu()
  c = _f32(cols)
  n, N = c.shape
  rank2, nonfinite = np.empty((n, N), np.int32), np.empty((n,), np.int32)
  check(lib.smx_k_col_rank2(_fp(c), n, N, _ip(rank2), _ip(nonfinite)))
  return rank2, nonfinite


def k_col_correlate(cols, prot_rank2, prot_unit):
  """smx_k_col_correlate: the kernels of Engine.predict_correlate on host columns cols [n_cols, N] -> its dict of sums"""
  lib = _hip.require_gpu()
  c = _f32(cols)
  n, N = c.shape
  pr, pu = _col_operands(prot_rank2, prot_unit, N)
  out, res = _col_outputs(n, pr.shape[0])
  check(lib.smx_k_col_correlate(_fp(c), n, N, _ip(pr), _dp(pu), pr.shape[0], *res))
  return out


def k_cluster_silhouette(Z, labels, n_labels: int):
  """smx_cluster_silhouette: cells Z [N, D] float32, classes labels [N] in 0 .. n_labels - 1 -> (a [N], b [N]) float64, the mean distance of
  every cell to its own class and to the nearest other one"""
  lib = _hip.require_gpu()
  z = _f32(Z)
  y = np.ascontiguousarray(labels, dtype=np.int32)
  if z.ndim != 2 or y.shape != (z.shape[0],):
    raise ValueError(f"Z must be [cells, D] and labels [cells], got {z.shape} and {y.shape}")
  a, b = np.empty((z.shape[0],), np.float64), np.empty((z.shape[0],), np.float64)
  check(lib.smx_cluster_silhouette(_fp(z), z.shape[0], z.shape[1], _ip(y), int(n_labels), _dp(a), _dp(b)))
  return a, b


def k_cluster_kmeans(Z, init_idx, max_iter: int = 300, all_labels: bool = False):
  """smx_cluster_kmeans: Lloyd's iterations on cells Z [N, D] float32 from the initial centres Z[init_idx [n_init, K]], every restart in one
  call -> dict(labels [N], centres [K, D], inertia [n_init], n_iter [n_init], best, and labels_all [n_init, N] when asked)"""
  lib = _hip.require_gpu()
  z = _f32(Z)
  idx = np.ascontiguousarray(init_idx, dtype=np.int32)
  if z.ndim != 2 or idx.ndim != 2:
    raise ValueError(f"Z must be [cells, D] and init_idx [n_init, K], got {z.shape} and {idx.shape}")
  (N, D), (R, K) = z.shape, idx.shape
  out = dict(labels=np.empty((N,), np.int32), centres=np.empty((K, D), np.float64), inertia=np.empty((R,), np.float64),
             n_iter=np.empty((R,), np.int32))
  best = C.c_int32(-1)
  every = np.empty((R, N), np.int32) if all_labels else None
  check(lib.smx_cluster_kmeans(_fp(z), N, D, K, _ip(idx), R, int(max_iter), _ip(out["labels"]), _dp(out["centres"]), _dp(out["inertia"]),
                               _ip(out["n_iter"]), C.byref(best), None if every is None else _ip(every)))
  out["best"] = int(best.value)
  if every is not None:
    out["labels_all"] = every
  return out


def _gmm_matrix(X, K=None):
  """X [cells, C] as contiguous float32, within the limits of smx_gmm.hip (checked here so that a refusal never asks for the device)"""
  x = np.asarray(X)
  if x.ndim != 2 or x.shape[0] < 1:
    raise ValueError(f"X must be [cells >= 1, C], got {x.shape}")
  if not (1 <= x.shape[1] <= 4096):
    raise ValueError(f"the number of columns must be 1 .. 4096, got {x.shape[1]}")
  if x.shape[0] >= 2 ** 31:
    raise ValueError(f"n_cells must be below 2^31, got {x.shape[0]}")
  if K is not None and not (2 <= int(K) <= 8):
    raise ValueError(f"the number of components must be 2 .. 8, got {K}")
  x = _f32(x)
  if not np.all(np.isfinite(x)) or np.any(x < 0):
    raise ValueError("Only support non-negative values: X holds a negative or non-finite entry")
  return x


def gmm_n_train(x, remove_zeros: bool = True) -> np.ndarray:
  """int64 [C]: the size of every column's training set -- with remove_zeros the positive cells plus ONE sample 0 if any cell was zero"""
  if not remove_zeros:
    return np.full((x.shape[1],), x.shape[0], np.int64)
  n_pos = np.count_nonzero(x > 0, axis=0).astype(np.int64)
  return n_pos + (n_pos < x.shape[0])


def k_gmm1d_fit(X, init_raw, max_iter: int = 120, tol: float = 1e-3, reg_covar: float = 1e-6, remove_zeros: bool = True,
                log_norm: bool = True, all_params: bool = False, stats: bool = False) -> dict:
  """smx_gmm1d_fit: one 1-D mixture of K Gaussians per column of X [cells, C] (non-negative), restart r of column c started from the raw
  values init_raw [C, R, K] of K training cells -> dict(lower_bound, n_iter, converged [C, R]; best, n_train, col_sum [C]; weights, means,
  variances [C, K] of the best restart; params_all [C, R, 3, K] when asked; stats: launches, round_trips, kernel_ms, loop_ms, call_ms)"""
  seeds = np.asarray(init_raw)
  if seeds.ndim != 3:
    raise ValueError(f"init_raw must be [C, R, K], got {seeds.shape}")
  Cn, R, K = seeds.shape
  x = _gmm_matrix(X, K)
  if Cn != x.shape[1]:
    raise ValueError(f"init_raw is for {Cn} columns and X has {x.shape[1]}")
  if not (1 <= R <= 64):
    raise ValueError(f"the number of restarts must be 1 .. 64, got {R}")
  max_iter, tol, reg_covar = int(max_iter), float(tol), float(reg_covar)
  if max_iter < 1 or not (tol > 0 and np.isfinite(tol)) or not (reg_covar >= 0 and np.isfinite(reg_covar)):
    raise ValueError(f"max_iter >= 1, tol > 0 and reg_covar >= 0 are required, got {max_iter}, {tol} and {reg_covar}")
  seeds = _f32(seeds)
  if not np.all(np.isfinite(seeds)) or np.any(seeds < 0):
    raise ValueError("init_raw holds a negative or non-finite value")
  n_train = gmm_n_train(x, remove_zeros)
  if np.any(n_train < K):
    c = int(np.argmax(n_train < K))
    raise ValueError(f"column {c} has {int(n_train[c])} training samples, fewer than the {K} components")
  lib = _hip.require_gpu()
  N, Cn = x.shape
  out = dict(lower_bound=np.empty((Cn, R), np.float64), n_iter=np.empty((Cn, R), np.int32), converged=np.empty((Cn, R), np.int32),
             best=np.empty((Cn,), np.int32), weights=np.empty((Cn, K), np.float64), means=np.empty((Cn, K), np.float64),
             variances=np.empty((Cn, K), np.float64), n_train=np.empty((Cn,), np.int64), col_sum=np.empty((Cn,), np.float64))
  every = np.empty((Cn, R, 3, K), np.float64) if all_params else None
  st = np.zeros((5,), np.float64) if stats else None
  check(lib.smx_gmm1d_fit(_fp(x), N, Cn, K, _fp(seeds), R, max_iter, tol, reg_covar, int(bool(remove_zeros)), int(bool(log_norm)),
                          _dp(out["lower_bound"]), _ip(out["n_iter"]), _ip(out["converged"]), _ip(out["best"]), _dp(out["weights"]),
                          _dp(out["means"]), _dp(out["variances"]), out["n_train"].ctypes.data_as(C.POINTER(C.c_int64)), _dp(out["col_sum"]),
                          None if every is None else _dp(every), None if st is None else _dp(st)))
  if every is not None:
    out["params_all"] = every
  if st is not None:
    out["stats"] = dict(launches=int(st[0]), round_trips=int(st[1]), kernel_ms=float(st[2]), loop_ms=float(st[3]), call_ms=float(st[4]))
  return out


def k_gmm1d_predict(X, weights, means, variances, order, positive_component: int, threshold, log_norm: bool = True, score: bool = False):
  """smx_gmm1d_predict: X [cells, C] under the mixtures weights, means, variances [C, K] -> (prob [cells, C] float64, the mean responsibility
  of the components order[c, positive_component:]; bin [cells, C] float32, normalised value >= threshold[c]; score [cells, C] float64, the
  log-likelihood, or None)"""
  w, m, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (weights, means, variances))
  if w.ndim != 2 or m.shape != w.shape or v.shape != w.shape:
    raise ValueError(f"weights, means and variances must all be [C, K], got {w.shape}, {m.shape} and {v.shape}")
  Cn, K = w.shape
  x = _gmm_matrix(X, K)
  o = np.ascontiguousarray(order, dtype=np.int32)
  thr = np.ascontiguousarray(threshold, dtype=np.float64)
  if x.shape[1] != Cn:
    raise ValueError(f"Number of classes mis-match: fitted with {Cn} columns, X has {x.shape[1]}")
  if o.shape != (Cn, K) or not np.array_equal(np.sort(o, axis=1), np.tile(np.arange(K, dtype=np.int32), (Cn, 1))):
    raise ValueError("order must be [C, K], a permutation of 0 .. K - 1 per column")
  if thr.shape != (Cn,) or np.any(np.isnan(thr)):
    raise ValueError("threshold must be [C] without NaN")
  if not (1 <= int(positive_component) < K):
    raise ValueError(f"positive_component must be 1 .. K - 1 = {K - 1}, got {positive_component}")
  if not (np.all(np.isfinite(w)) and np.all(w > 0) and np.all(np.isfinite(m)) and np.all(np.isfinite(v)) and np.all(v > 0)):
    raise ValueError("weights and variances must be positive and finite, means finite")
  lib = _hip.require_gpu()
  N = x.shape[0]
  prob, bins = np.empty((N, Cn), np.float64), np.empty((N, Cn), np.float32)
  sc = np.empty((N, Cn), np.float64) if score else None
  check(lib.smx_gmm1d_predict(_fp(x), N, Cn, K, _dp(w), _dp(m), _dp(v), _ip(o), int(positive_component), _dp(thr), int(bool(log_norm)),
                              _dp(prob), _fp(bins), None if sc is None else _dp(sc)))
  return prob, bins, sc


ILL_DEFINED_COVARIANCE = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance "
                          "caused by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or "
                          "scale the input data.")


def k_gmm_full_fit(Z, init_labels, max_iter: int = 100, tol: float = 1e-3, reg_covar: float = 1e-6, all_params: bool = False,
                   n_components=None) -> dict:
  """smx_gmm_full_fit: scikit-learn's full-covariance EM loop on cells Z [N, D] from the starting labelings init_labels [R, N] (or [N]), K =
  n_components (default: the largest label + 1) -> dict(lower_bound, n_iter, converged, status [R]; best; weights [K], means [K, D],
  covariances, chol_inv [K, D, D] and labels [N] of the best restart; with all_params weights_all [R, K], means_all [R, K, D],
  covariances_all [R, K, D, D]).  A restart with status 1 met an ill-defined covariance; ValueError when every restart did."""
  z = _f32(Z)
  lab = np.asarray(init_labels)
  if lab.ndim == 1:
    lab = lab[None, :]
  if z.ndim != 2 or lab.ndim != 2 or lab.shape[1] != z.shape[0]:
    raise ValueError(f"Z must be [cells, D] and init_labels [R, cells], got {z.shape} and {lab.shape}")
  lab = np.ascontiguousarray(lab, dtype=np.int32)
  K = (int(lab.max()) + 1 if lab.size else 0) if n_components is None else int(n_components)
  (N, D), R = z.shape, lab.shape[0]
  lib = _hip.require_gpu()
  out = dict(lower_bound=np.empty((R,), np.float64), n_iter=np.empty((R,), np.int32), converged=np.empty((R,), np.int32),
             status=np.zeros((R,), np.int32), weights=np.empty((max(K, 0),), np.float64), means=np.empty((max(K, 0), D), np.float64),
             covariances=np.empty((max(K, 0), D, D), np.float64), chol_inv=np.empty((max(K, 0), D, D), np.float64), labels=np.empty((N,), np.int32))
  best = C.c_int32(-1)
  every = np.empty((R, max(K, 0) * (1 + D + D * D)), np.float64) if all_params else None
  rc = lib.smx_gmm_full_fit(_fp(z), N, D, K, _ip(lab), R, int(max_iter), float(tol), float(reg_covar), _dp(out["lower_bound"]), _ip(out["n_iter"]),
                            _ip(out["converged"]), _ip(out["status"]), C.byref(best), _dp(out["weights"]), _dp(out["means"]),
                            _dp(out["covariances"]), _dp(out["chol_inv"]), _ip(out["labels"]), None if every is None else _dp(every))
  if rc == -1 and R >= 1 and bool(np.all(out["status"] == 1)):   # (SMX_ERR_INVALID with every status set: every restart failed)
    raise ValueError(ILL_DEFINED_COVARIANCE)
  check(rc)
  out["best"] = int(best.value)
  if every is not None:
    out["weights_all"] = every[:, :K].copy()
    out["means_all"] = every[:, K:K + K * D].reshape(R, K, D).copy()
    out["covariances_all"] = every[:, K + K * D:].reshape(R, K, D, D).copy()
  return out


def k_gmm_full_predict(Z, weights, means, chol_inv, resp: bool = False, score: bool = False) -> dict:
  """smx_gmm_full_predict: cells Z [N, D] under the mixture weights [K], means [K, D], chol_inv [K, D, D] (lower triangular: the inverse of
  the Cholesky factor of every covariance) -> dict(labels [N] int32; resp [N, K] and score [N] float64 when asked)"""
  w, m, li = (np.ascontiguousarray(a, dtype=np.float64) for a in (weights, means, chol_inv))
  if w.ndim != 1 or m.ndim != 2 or m.shape[0] != w.shape[0] or li.shape != (m.shape[0], m.shape[1], m.shape[1]):
    raise ValueError(f"weights, means and chol_inv must be [K], [K, D] and [K, D, D], got {w.shape}, {m.shape} and {li.shape}")
  K, D = m.shape
  z = _f32(Z)
  if z.ndim != 2 or z.shape[1] != D:
    raise ValueError(f"the mixture has {D} features, Z is {z.shape}")
  lib = _hip.require_gpu()
  N = z.shape[0]
  out = dict(labels=np.empty((N,), np.int32))
  if resp:
    out["resp"] = np.empty((N, K), np.float64)
  if score:
    out["score"] = np.empty((N,), np.float64)
  check(lib.smx_gmm_full_predict(_fp(z), N, D, K, _dp(w), _dp(m), _dp(li), _ip(out["labels"]), _dp(out["resp"]) if resp else None,
                                 _dp(out["score"]) if score else None))
  return out


PREP_FUNCS = {None: 0, "identity": 0, "log1p": 1, "expm1": 2}   # smx_prep_*: the f of a view f(x / row_div)


def _prep_input(x, func, row_div, block_rows):
  """The shared arguments of smx_prep_stats / smx_prep_apply, checked here so that a refusal never asks for the device:
  -> (dense float32 [N, G] or None, (indptr, cols, vals) or None, N, G, func id, row_div float32 [N] or None)"""
  if func not in PREP_FUNCS:
    raise ValueError(f"func must be one of 'identity', 'log1p', 'expm1', got {func!r}")
  if getattr(x, "ndim", 0) != 2 or x.shape[0] < 1 or x.shape[1] < 1:
    raise ValueError(f"expected a matrix [cells >= 1, genes >= 1], got shape {getattr(x, 'shape', None)}")
  if int(block_rows) < 0:
    raise ValueError(f"block_rows must be >= 0 (0: the library's choice), got {block_rows}")
  N, G = x.shape
  dense, csr = (None, _csr3(x, G)) if _sparse(x) else (_f32(x), None)
  rd = None if row_div is None else _f32(row_div, (N,))
  if rd is not None and not (np.isfinite(rd).all() and (rd != 0).all()):
    raise ValueError("row_div must be finite and non-zero")
  return dense, csr, N, G, PREP_FUNCS[func], rd


def k_prep_stats(x, func=None, row_div=None, col_mask=None, row_thresh=None, block_rows: int = 0) -> dict:
  """smx_prep_stats: the statistics of the view f(x / row_div) of a dense or scipy.sparse matrix [N, G] -> dict(total [N] float64 (over the
  genes col_mask keeps), n_genes [N] int32, sum / sumsq [G] float64, n_cells [G] int64, and with row_thresh [N]: n_above [G] int64)"""
  dense, csr, N, G, f, rd = _prep_input(x, func, row_div, block_rows)
  mask = None if col_mask is None else np.ascontiguousarray(col_mask, dtype=np.uint8)
  if mask is not None and mask.shape != (G,):
    raise ValueError(f"col_mask must be [{G}], got {mask.shape}")
  thr = None if row_thresh is None else _f32(row_thresh, (N,))
  if thr is not None and np.isnan(thr).any():
    raise ValueError("row_thresh holds a NaN")
  lib = _hip.require_gpu()
  out = dict(total=np.empty((N,), np.float64), n_genes=np.empty((N,), np.int32), sum=np.empty((G,), np.float64),
             sumsq=np.empty((G,), np.float64), n_cells=np.empty((G,), np.int64))
  if thr is not None:
    out["n_above"] = np.empty((G,), np.int64)
  lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_prep_stats(_fp(dense), *ptrs, N, G, int(block_rows), f, _fp(rd),
                           None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(thr), _dp(out["total"]),
                           _ip(out["n_genes"]), _dp(out["sum"]), _dp(out["sumsq"]), lp(out["n_cells"]),
                           None if thr is None else lp(out["n_above"])))
  return out


def k_prep_apply(x, func=None, row_div=None, mean=None, std=None, max_value=None, block_rows: int = 0):
  """smx_prep_apply: the view f(x / row_div) written out as float32, then (v - mean) / std and the clip from above at max_value where
  given.  A scipy.sparse matrix without mean / std / max_value comes back as CSR of the same structure (only the stored values cross);
  everything else comes back dense [N, G]."""
  dense, csr, N, G, f, rd = _prep_input(x, func, row_div, block_rows)
  if (mean is None) != (std is None):
    raise ValueError("mean and std go together")
  mu, sd = (None, None) if mean is None else (_f32(mean, (G,)), _f32(std, (G,)))
  if max_value is not None and np.isnan(max_value):
    raise ValueError("max_value is NaN")
  clip, mv = (0, 0.0) if max_value is None else (1, float(max_value))
  lib = _hip.require_gpu()
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  if csr is not None and mu is None and not clip:
    import scipy.sparse as sp
    vals = np.empty_like(csr[2])
    check(lib.smx_prep_apply(None, *ptrs, N, G, int(block_rows), f, _fp(rd), None, None, 0, 0.0, None, _fp(vals)))
    return sp.csr_matrix((vals, csr[1].copy(), csr[0].copy()), shape=(N, G))
  out = np.empty((N, G), np.float32)
  check(lib.smx_prep_apply(_fp(dense), *ptrs, N, G, int(block_rows), f, _fp(rd), _fp(mu), _fp(sd), clip, mv, _fp(out), None))
  return out


PCA_MAX_GENES = 8192        # smx_pca_cov / smx_pca_project: the covariance takes 8 G^2 bytes
PCA_MAX_COMPONENTS = 128    # smx_pca_project, per call
KNN_MAX_D, KNN_MAX_K = 128, 256


def _pca_input(x, block_rows):
  """The matrix of smx_pca_cov / smx_pca_project, checked here so that a refusal never asks for the device"""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  if G > PCA_MAX_GENES:
    raise ValueError(f"PCA of {G} columns is not built: the covariance route takes at most {PCA_MAX_GENES} "
                     "(8 G^2 bytes); select genes first, e.g. with filter_highly_variable_genes")
  return dense, csr, N, G


def k_pca_cov(x, block_rows: int = 0):
  """smx_pca_cov: a dense or scipy.sparse matrix [N >= 2, G <= 8192] -> (mean [G], cov [G, G]) float64, the two-pass covariance with
  n - 1 in the denominator"""
  dense, csr, N, G = _pca_input(x, block_rows)
  if N < 2:
    raise ValueError(f"a covariance needs at least 2 cells, got {N}")
  lib = _hip.require_gpu()
  mean, cov = np.empty((G,), np.float64), np.empty((G, G), np.float64)
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_pca_cov(_fp(dense), *ptrs, N, G, int(block_rows), _dp(mean), _dp(cov)))
  return mean, cov


def k_pca_project(x, mean, components, block_rows: int = 0):
  """smx_pca_project: (x - mean) . components^T for mean [G] and components [C <= 128, G] float64 -> [N, C] float32"""
  dense, csr, N, G = _pca_input(x, block_rows)
  mu, w = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(components, dtype=np.float64)
  if mu.shape != (G,) or w.ndim != 2 or w.shape[1] != G or not 1 <= w.shape[0] <= PCA_MAX_COMPONENTS:
    raise ValueError(f"mean must be [{G}] and components [1 .. {PCA_MAX_COMPONENTS}, {G}], got {mu.shape} and {w.shape}")
  if not (np.isfinite(mu).all() and np.isfinite(w).all()):
    raise ValueError("mean and components must be finite")
  lib = _hip.require_gpu()
  out = np.empty((N, w.shape[0]), np.float32)
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_pca_project(_fp(dense), *ptrs, N, G, int(block_rows), _dp(mu), _dp(w), w.shape[0], _fp(out)))
  return out


def k_knn(Z, k: int):
  """smx_knn: cells Z [N, D] float32 -> (idx [N, k] int32, dist [N, k] float64), the k other cells nearest to each by (d2, index)"""
  z = _f32(Z)
  k = int(k)
  if z.ndim != 2 or not 1 <= z.shape[1] <= KNN_MAX_D:
    raise ValueError(f"Z must be [cells, 1 <= D <= {KNN_MAX_D}], got {z.shape}")
  if not 1 <= k <= KNN_MAX_K or k >= z.shape[0]:
    raise ValueError(f"k must be in 1 .. {KNN_MAX_K} and below the number of cells ({z.shape[0]}), got {k}")
  if not np.isfinite(z).all():
    raise ValueError("Z holds an entry that is not finite")
  lib = _hip.require_gpu()
  idx, dist = np.empty((z.shape[0], k), np.int32), np.empty((z.shape[0], k), np.float64)
  check(lib.smx_knn(_fp(z), z.shape[0], z.shape[1], k, _ip(idx), _dp(dist)))
  return idx, dist


def k_knn_umap(idx, dist):
  """smx_knn_umap: a neighbour table idx / dist [N, K] whose column 0 is the cell itself -> (rho [N], sigma [N], weight [N, K]) float64"""
  ix, d = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float64)
  if ix.ndim != 2 or d.shape != ix.shape or not 2 <= ix.shape[1] <= KNN_MAX_K + 1 or ix.shape[0] < 1:
    raise ValueError(f"idx and dist must both be [cells, 2 <= K <= {KNN_MAX_K + 1}], got {ix.shape} and {d.shape}")
  N, K = ix.shape
  if ix.min() < 0 or ix.max() >= N:
    raise ValueError("idx holds an index outside 0 .. cells - 1")
  if not (np.isfinite(d).all() and (d >= 0).all()):
    raise ValueError("dist must be finite and non-negative")
  lib = _hip.require_gpu()
  rho, sigma, weight = np.empty((N,), np.float64), np.empty((N,), np.float64), np.empty((N, K), np.float64)
  check(lib.smx_knn_umap(_ip(ix), _dp(d), N, K, _dp(rho), _dp(sigma), _dp(weight)))
  return rho, sigma, weight


TSNE_MAX_COMPONENTS = 3


def k_tsne_affinities(idx, dist, perplexity: float):
  """smx_tsne_affinities: smx_knn's table idx / dist [N, k] (the k other cells) -> (cond_p [N, k], beta [N]) float64, scikit-learn's
  binary search for the perplexity, per row"""
  ix, d = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float64)
  if ix.ndim != 2 or d.shape != ix.shape or not 1 <= ix.shape[1] <= KNN_MAX_K:
    raise ValueError(f"idx and dist must both be [cells, 1 <= k <= {KNN_MAX_K}], got {ix.shape} and {d.shape}")
  N, k = ix.shape
  if N < 4 or k >= N:
    raise ValueError(f"t-SNE needs at least 4 cells and k below their number, got {N} cells and k = {k}")
  perplexity = float(perplexity)
  if not (np.isfinite(perplexity) and 1.0 <= perplexity < N):
    raise ValueError(f"perplexity must be in 1 .. below the number of cells ({N}), got {perplexity}")
  if ix.min() < 0 or ix.max() >= N:
    raise ValueError("idx holds an index outside 0 .. cells - 1")
  if not (np.isfinite(d).all() and (d >= 0).all()):
    raise ValueError("dist must be finite and non-negative")
  lib = _hip.require_gpu()
  cond_p, beta = np.empty((N, k), np.float64), np.empty((N,), np.float64)
  check(lib.smx_tsne_affinities(_ip(ix), _dp(d), N, k, perplexity, _dp(cond_p), _dp(beta)))
  return cond_p, beta


def _tsne_problem(P, Y):
  """The joint P (scipy.sparse CSR [N, N], sorted columns, entries > 0) and an embedding Y [N, 1 .. 3] as the t-SNE entries take them,
  checked here so that a refusal never asks for the device -> (indptr int64, cols int32, p float64, y float64)"""
  import scipy.sparse as sp
  if not sp.issparse(P) or P.format != "csr" or P.ndim != 2 or P.shape[0] != P.shape[1]:
    raise ValueError(f"P must be a square scipy.sparse CSR matrix, got {type(P).__name__} of shape {getattr(P, 'shape', None)}")
  N = P.shape[0]
  if not 4 <= N < 2 ** 31:
    raise ValueError(f"t-SNE needs at least 4 cells, got {N}")
  y = np.ascontiguousarray(Y, dtype=np.float64)
  if y.ndim != 2 or y.shape[0] != N or not 1 <= y.shape[1] <= TSNE_MAX_COMPONENTS:
    raise ValueError(f"Y must be [{N}, 1 .. {TSNE_MAX_COMPONENTS}], got {y.shape}")
  if not np.isfinite(y).all():
    raise ValueError("Y holds an entry that is not finite")
  indptr, cols = np.ascontiguousarray(P.indptr, dtype=np.int64), np.ascontiguousarray(P.indices, dtype=np.int32)
  p = np.ascontiguousarray(P.data, dtype=np.float64)
  if indptr.shape != (N + 1,) or indptr[0] != 0 or (np.diff(indptr) < 0).any() or indptr[-1] != cols.size or p.size != cols.size:
    raise ValueError("P's indptr does not describe its entries")
  if cols.size and (cols.min() < 0 or cols.max() >= N):
    raise ValueError("P holds a column outside 0 .. cells - 1")
  inner = np.ones(cols.size, bool)
  inner[indptr[:-1][indptr[:-1] < cols.size]] = False   # (the first entry of a row has no entry in front of it)
  if (np.diff(cols.astype(np.int64), prepend=-1)[inner] <= 0).any():
    raise ValueError("the columns of a row of P must increase strictly (sort_indices, sum_duplicates)")
  if not (np.isfinite(p).all() and (p > 0).all()):
    raise ValueError("every stored entry of P must be finite and positive (eliminate_zeros)")
  return indptr, cols, p, y


def k_tsne_gradient(P, Y, exaggeration: float = 1.0):
  """smx_tsne_gradient: one evaluation of the exact t-SNE objective at Y [N, C] for the joint P (CSR) -> (grad [N, C], KL, Z) float64"""
  indptr, cols, p, y = _tsne_problem(P, Y)
  exaggeration = float(exaggeration)
  if not (np.isfinite(exaggeration) and exaggeration > 0):
    raise ValueError(f"exaggeration must be finite and positive, got {exaggeration}")
  lib = _hip.require_gpu()
  grad, kl, Z = np.empty_like(y), C.c_double(), C.c_double()
  check(lib.smx_tsne_gradient(indptr.ctypes.data_as(C.POINTER(C.c_int64)), _ip(cols), _dp(p), y.shape[0], y.shape[1], _dp(y), exaggeration,
                              _dp(grad), C.byref(kl), C.byref(Z)))
  return grad, kl.value, Z.value


def k_tsne_fit(P, Y0, max_iter: int = 1000, early_exaggeration: float = 12.0, learning_rate: float = 200.0, min_grad_norm: float = 1e-7,
               n_iter_without_progress: int = 300):
  """smx_tsne_fit: scikit-learn's descent of the exact objective from Y0 [N, C], resident on the device -> dict(Y, update, gains
  [N, C] float64, kl_trace [max_iter] (NaN where the iteration did not report), n_iter)"""
  indptr, cols, p, y0 = _tsne_problem(P, Y0)
  max_iter, nwp = int(max_iter), int(n_iter_without_progress)
  ee, lr, mgn = float(early_exaggeration), float(learning_rate), float(min_grad_norm)
  if max_iter < 1 or nwp < 0:
    raise ValueError(f"max_iter must be >= 1 and n_iter_without_progress >= 0, got {max_iter} and {nwp}")
  if not (np.isfinite(ee) and ee > 0 and np.isfinite(lr) and lr > 0 and mgn >= 0):
    raise ValueError(f"early_exaggeration and learning_rate must be finite and positive and min_grad_norm >= 0, got {ee}, {lr}, {mgn}")
  lib = _hip.require_gpu()
  Y, update, gains = np.empty_like(y0), np.empty_like(y0), np.empty_like(y0)
  trace, n_iter = np.empty((max_iter,), np.float64), np.zeros((1,), np.int32)
  check(lib.smx_tsne_fit(indptr.ctypes.data_as(C.POINTER(C.c_int64)), _ip(cols), _dp(p), y0.shape[0], y0.shape[1], _dp(y0), max_iter, ee, lr,
                         mgn, nwp, _dp(Y), _dp(trace), _ip(n_iter), _dp(update), _dp(gains)))
  return dict(Y=Y, update=update, gains=gains, kl_trace=trace, n_iter=int(n_iter[0]))


MI_MAX_NEIGHBORS = 8        # smx_mutual_info: the register list of the cc sweep
MI_MAX_CELLS = 1 << 20


def _mi_tables(N):
  """(digamma(n), log(n)) for n = 0 .. N, float64: the two tables the device adds entries of (entry 0 is never read)"""
  from scipy.special import digamma
  n = np.arange(N + 1, dtype=np.float64)
  psi, logn = np.zeros(N + 1), np.zeros(N + 1)
  psi[1:], logn[1:] = digamma(n[1:]), np.log(n[1:])
  return psi, logn


def _mi_check(N, n_neighbors):
  k = int(n_neighbors)
  if not 2 <= N <= MI_MAX_CELLS:
    raise ValueError(f"mutual information takes 2 .. 2^20 cells, got {N}")
  if k < 1 or k > MI_MAX_NEIGHBORS:
    raise ValueError(f"n_neighbors must be in 1 .. {MI_MAX_NEIGHBORS} (MI_MAX_NEIGHBORS: the register list of the device's sweep), got {k}")
  if k >= N:
    raise ValueError(f"n_neighbors = {k} must be below the number of cells ({N})")
  return k


def _mi_cols(cols, discrete, what):
  c = np.ascontiguousarray(cols, dtype=np.float64)
  d = np.ascontiguousarray(discrete, dtype=bool).astype(np.uint8)
  if c.ndim != 2 or c.shape[0] < 1 or d.shape != (c.shape[0],):
    raise ValueError(f"{what} columns must be [columns >= 1, cells] with one discrete flag each, got {c.shape} and {d.shape}")
  bad = np.flatnonzero(~np.isfinite(c).all(axis=1))
  if bad.size:
    raise ValueError(f"{what} column {int(bad[0])} holds a value that is not finite")
  return c, d


def mutual_info(xcols, x_discrete, ycols, y_discrete, n_neighbors: int = 3, gene_chunk: int = 0):
  """smx_mutual_info: prepared columns xcols [G, N] and ycols [P, N] float64 (gene-major) with their discrete flags -> the mutual
  information [G, P] float64 of every pair, by scikit-learn's three kNN estimators.  gene_chunk: genes on the device at a time (0: the
  library's choice); it changes no bit."""
  x, xd = _mi_cols(xcols, x_discrete, "gene")
  y, yd = _mi_cols(ycols, y_discrete, "protein")
  if x.shape[1] != y.shape[1]:
    raise ValueError(f"genes and proteins must share their cells, got {x.shape[1]} and {y.shape[1]}")
  N = x.shape[1]
  k = _mi_check(N, n_neighbors)
  if int(gene_chunk) < 0:
    raise ValueError(f"gene_chunk must be >= 0, got {gene_chunk}")
  lib = _hip.require_gpu()
  psi, logn = _mi_tables(N)
  mi = np.empty((x.shape[0], y.shape[0]), np.float64)
  u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
  check(lib.smx_mutual_info(_dp(x), u8(xd), _dp(y), u8(yd), N, x.shape[0], y.shape[0], k, int(gene_chunk), _dp(psi), _dp(logn), _dp(mi)))
  return mi


RANK_MAX_CELLS = 1 << 20     # smx_group_ranksums: 2 N^2 and N^3 stay inside int64
RANK_MAX_GROUPS = 256        # smx_group_ranksums: the LDS accumulators
MOMENT_MAX_GROUPS = 65535    # smx_group_moments
MOMENT_MAX_ACC = 1 << 26     # smx_group_moments: n_groups x (n_genes rounded up to 4)


def _group_labels(labels, N, n_groups, max_groups):
  """labels [N] of integers in 0 .. n_groups - 1 -> int32, checked here so that a refusal never asks for the device"""
  K = int(n_groups)
  if not 1 <= K <= max_groups:
    raise ValueError(f"n_groups must be in 1 .. {max_groups}, got {n_groups}")
  lab = np.asarray(labels)
  if lab.shape != (N,) or lab.dtype.kind not in "iu":
    raise ValueError(f"labels must be integers [{N}], got {lab.dtype} {lab.shape}")
  if lab.min() < 0 or lab.max() >= K:
    raise ValueError(f"labels must lie in 0 .. {K - 1}")
  return np.ascontiguousarray(lab, dtype=np.int32), K


def k_group_moments(x, labels, n_groups: int, block_rows: int = 0) -> dict:
  """smx_group_moments: a dense or scipy.sparse matrix [N, G] and labels [N] in 0 .. n_groups - 1 -> dict(count [K] int64, and per group
  and gene sum [K, G] float64, css [K, G] float64 (the centred sum of squares about sum / count) and nnz [K, G] int64 (values != 0))"""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  lab, K = _group_labels(labels, N, n_groups, MOMENT_MAX_GROUPS)
  if K * ((G + 3) // 4 * 4) > MOMENT_MAX_ACC:
    raise ValueError(f"{K} groups x {G} genes pass the {MOMENT_MAX_ACC} accumulators of the group moments; take the genes in parts")
  lib = _hip.require_gpu()
  out = dict(count=np.empty((K,), np.int64), sum=np.empty((K, G), np.float64), css=np.empty((K, G), np.float64),
             nnz=np.empty((K, G), np.int64))
  lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_group_moments(_fp(dense), *ptrs, N, G, int(block_rows), _ip(lab), K, lp(out["count"]), _dp(out["sum"]), _dp(out["css"]),
                              lp(out["nnz"])))
  return out


def k_group_ranksums(cols, labels, n_groups: int, reference: int = -1):
  """smx_group_ranksums: cols [n_cols, N] float32 (gene-major, finite) and labels [N] in 0 .. n_groups - 1 -> (rank2_sum [K, n_cols] int64,
  tie_term int64: [n_cols] against the rest (reference = -1), [K, n_cols] against a reference group, whose own rows are 0)"""
  c = _f32(cols)
  if c.ndim != 2 or c.shape[0] < 1 or not 1 <= c.shape[1] <= RANK_MAX_CELLS:
    raise ValueError(f"cols must be [n_cols >= 1, 1 .. {RANK_MAX_CELLS} cells], got {c.shape}")
  n, N = c.shape
  lab, K = _group_labels(labels, N, n_groups, RANK_MAX_GROUPS)
  ref = int(reference)
  if not -1 <= ref < K:
    raise ValueError(f"reference must be -1 (the rest) or a group 0 .. {K - 1}, got {reference}")
  bad = np.flatnonzero(~np.isfinite(c).all(axis=1))
  if bad.size:
    raise ValueError(f"column {int(bad[0])} holds a value that is not finite")
  lib = _hip.require_gpu()
  rank2, tie = np.empty((K, n), np.int64), np.empty((n,) if ref < 0 else (K, n), np.int64)
  lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
  check(lib.smx_group_ranksums(_fp(c), n, N, _ip(lab), K, ref, lp(rank2), lp(tie)))
  return rank2, tie


MBK_MAX_CLUSTERS = 256       # smx_mbkmeans_*
MBK_MAX_GENES = 32768
MBK_MAX_SEED_ROWS = 65536    # smx_mbkmeans_seed: one workgroup scans the block
MBK_MAX_TRIALS = 16
MBK_MAX_RESIDENT = 1 << 31   # smx_mbkmeans_seed / _step hold their block whole: rows x (genes rounded up to 4)


def _mbk_input(x, n_clusters, block_rows=0, resident=False):
  """The shared arguments of smx_mbkmeans_*, checked here so that a refusal never asks for the device -> (dense, csr, N, G, K)"""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  K = int(n_clusters)
  if not 2 <= K <= MBK_MAX_CLUSTERS:
    raise ValueError(f"n_clusters must be in 2 .. {MBK_MAX_CLUSTERS}, got {n_clusters}")
  if G > MBK_MAX_GENES or N >= 2 ** 31:
    raise ValueError(f"mini-batch k-means takes up to {MBK_MAX_GENES} columns and fewer than 2^31 rows, got {(N, G)}")
  if resident and (N + 63) // 64 * 64 * ((G + 3) // 4 * 4) > MBK_MAX_RESIDENT:
    raise ValueError(f"a block of {N} x {G} passes the {MBK_MAX_RESIDENT} entries held on the device at once; take fewer rows per block")
  if not np.isfinite(dense if csr is None else csr[2]).all():
    raise ValueError("x holds an entry that is not finite")
  return dense, csr, N, G, K


def _mbk_centres(centres, K, G):
  c = np.ascontiguousarray(centres, dtype=np.float64)
  if c.ndim != 2 or c.shape[1] != G:
    raise ValueError(f"centres must be [n_clusters, {G}], got {c.shape}")
  return c


def k_mbkmeans_seed(x, K: int, first: int, u) -> dict:
  """smx_mbkmeans_seed: scikit-learn's k-means++ seeding of a dense or scipy.sparse block x [n, G] (taken as float32) with unit weights;
  first: the first centre's row, u [K - 1, T] float64 in [0, 1): the draws of every further centre's T local trials ->
  dict(indices [K] int32, centres [K, G] float64 (the chosen rows), potential [K] float64 (after each pick))"""
  dense, csr, N, G, K = _mbk_input(x, K, resident=True)
  uu = np.ascontiguousarray(u, dtype=np.float64)
  if uu.ndim != 2 or uu.shape[0] != K - 1 or not 1 <= uu.shape[1] <= MBK_MAX_TRIALS:
    raise ValueError(f"u must be [{K - 1}, 1 .. {MBK_MAX_TRIALS}], got {uu.shape}")
  if not ((uu >= 0) & (uu < 1)).all():
    raise ValueError("u must lie in [0, 1)")
  if not K <= N <= MBK_MAX_SEED_ROWS:
    raise ValueError(f"the seeding takes a block of n_clusters = {K} .. {MBK_MAX_SEED_ROWS} rows, got {N}")
  if not 0 <= int(first) < N:
    raise ValueError(f"first must be a row 0 .. {N - 1}, got {first}")
  lib = _hip.require_gpu()
  out = dict(indices=np.empty((K,), np.int32), centres=np.empty((K, G), np.float64), potential=np.empty((K,), np.float64))
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_mbkmeans_seed(_fp(dense), *ptrs, N, G, K, uu.shape[1], int(first), _dp(uu), _ip(out["indices"]), _dp(out["centres"]),
                              _dp(out["potential"])))
  return out


def k_mbkmeans_step(x, centres, counts, want_labels: bool = True) -> dict:
  """smx_mbkmeans_step: one mini-batch step of a block x [n, G] without the reassignment: the labels against centres [K, G], then for every
  centre with m > 0 rows centre = (centre * count + the sum of its rows in row order) / (count + m) and count += m ->
  dict(centres [K, G], counts [K] float64 (new arrays), inertia (of the labels, before the update), labels [n] int32 or None)"""
  c = np.array(centres, dtype=np.float64, order="C", ndmin=2)
  dense, csr, N, G, K = _mbk_input(x, c.shape[0], resident=True)
  c = _mbk_centres(c, K, G)
  cnt = np.array(counts, dtype=np.float64, order="C")
  if cnt.shape != (K,) or not (np.isfinite(cnt).all() and (cnt >= 0).all()):
    raise ValueError(f"counts must be [{K}], finite and >= 0")
  lib = _hip.require_gpu()
  labels, inertia = (np.empty((N,), np.int32) if want_labels else None), C.c_double()
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_mbkmeans_step(_fp(dense), *ptrs, N, G, K, _dp(c), _dp(cnt), None if labels is None else _ip(labels), C.byref(inertia)))
  return dict(centres=c, counts=cnt, inertia=inertia.value, labels=labels)


def k_mbkmeans_predict(x, centres, block_rows: int = 0, want_distance: bool = False):
  """smx_mbkmeans_predict: the nearest of centres [K, G] for every row of a dense or scipy.sparse x [N, G], streamed in blocks of block_rows
  rows (0: the library's choice; it changes no bit) -> labels [N] int32, or (labels, squared distance [N] float64) with want_distance"""
  c = np.ascontiguousarray(centres, dtype=np.float64)
  dense, csr, N, G, K = _mbk_input(x, c.shape[0] if c.ndim == 2 else 0, block_rows)
  c = _mbk_centres(c, K, G)
  lib = _hip.require_gpu()
  labels, dist = np.empty((N,), np.int32), (np.empty((N,), np.float64) if want_distance else None)
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_mbkmeans_predict(_fp(dense), *ptrs, N, G, int(block_rows), K, _dp(c), _ip(labels), None if dist is None else _dp(dist)))
  return (labels, dist) if want_distance else labels


LR_MAX_CLASSES = 256        # smx_logreg_*
LR_MAX_GENES = 32768
LR_MAX_RESIDENT = 1 << 31    # the matrix is held whole: rows (rounded up to 64) x (genes rounded up to 4)


def _lr_input(x, labels, n_classes, block_rows=0, resident=True, every_class=False):
  """The shared arguments of smx_logreg_*, checked here so that a refusal never asks for the device -> (dense, csr, N, G, K, form, labels
  int32 or None).  Two classes take the binary form (one logit row), three and more the multinomial one."""
  dense, csr, N, G, _, _ = _prep_input(x, None, None, block_rows)
  K = int(n_classes)
  if not 2 <= K <= LR_MAX_CLASSES:
    raise ValueError(f"logistic regression takes 2 .. {LR_MAX_CLASSES} classes, got {n_classes}")
  if G > LR_MAX_GENES or N >= 2 ** 31:
    raise ValueError(f"logistic regression takes up to {LR_MAX_GENES} columns and fewer than 2^31 rows, got {(N, G)}")
  if resident and (N + 63) // 64 * 64 * ((G + 3) // 4 * 4) > LR_MAX_RESIDENT:
    raise ValueError(f"a matrix of {N} x {G} passes the {LR_MAX_RESIDENT} entries held on the device at once")
  if not np.isfinite(dense if csr is None else csr[2]).all():
    raise ValueError("x holds an entry that is not finite")
  lab = None
  if labels is not None:
    lab = np.asarray(labels)
    if lab.shape != (N,) or lab.dtype.kind not in "iu":
      raise ValueError(f"labels must be [{N}] integers, got {lab.dtype} {lab.shape}")
    if lab.min() < 0 or lab.max() >= K:
      raise ValueError(f"labels must lie in 0 .. {K - 1}")
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    empty = np.flatnonzero(np.bincount(lab, minlength=K) == 0)
    if every_class and empty.size:
      raise ValueError(f"class {int(empty[0])} has no row")
  return dense, csr, N, G, K, int(K == 2), lab


def _lr_params(W, b, Kz, G, what="W"):
  w, bb = np.ascontiguousarray(W, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
  if w.shape != (Kz, G) or bb.shape != (Kz,):
    raise ValueError(f"{what} must be [{Kz}, {G}] and its intercept [{Kz}], got {w.shape} and {bb.shape}")
  if not (np.isfinite(w).all() and np.isfinite(bb).all()):
    raise ValueError(f"{what} or its intercept holds a value that is not finite")
  return w, bb


def _lr_penalty(C_):
  c = float(C_)
  if not (np.isfinite(c) and c > 0):
    raise ValueError(f"C must be finite and > 0, got {C_}")
  return c


def k_logreg_eval(x, labels, n_classes: int, W, b, C_: float = 1.0, fit_intercept: bool = True) -> dict:
  """smx_logreg_eval: the mean-form objective F = (1/N) sum_i loss_i + ||W||^2 / (2 C N) and its gradient at (W [Kz, G], b [Kz]) float64,
  Kz = 1 logit row for two classes (the binary form), n_classes otherwise; x dense or scipy.sparse [N, G] (taken as float32), labels [N]
  integers in 0 .. n_classes - 1 (not every class needs a row) -> dict(F, gW [Kz, G], gb [Kz]).  fit_intercept=False: b is taken as 0 and gb is 0."""
  dense, csr, N, G, K, form, lab = _lr_input(x, labels, n_classes)
  Kz = 1 if form else K
  w, bb = _lr_params(W, b, Kz, G)
  c = _lr_penalty(C_)
  lib = _hip.require_gpu()
  F, gW, gb = C.c_double(), np.empty((Kz, G), np.float64), np.empty((Kz,), np.float64)
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_logreg_eval(_fp(dense), *ptrs, N, G, _ip(lab), K, form, c, int(bool(fit_intercept)), _dp(w), _dp(bb), C.byref(F), _dp(gW),
                            _dp(gb)))
  return dict(F=F.value, gW=gW, gb=gb)


def k_logreg_fit(x, labels, n_classes: int, C_: float = 1.0, fit_intercept: bool = True, tol: float = 1e-4, max_iter: int = 100,
                 W0=None, b0=None) -> dict:
  """smx_logreg_fit: the minimiser of k_logreg_eval's F by L-BFGS (memory 10, Armijo backtracking) on the device, from zero or from the
  warm start (W0, b0); every class needs a row; stops at max|g| <= tol or after max_iter iterations ->
  dict(W [Kz, G], b [Kz], F, gmax, n_iter, n_eval, converged)"""
  dense, csr, N, G, K, form, lab = _lr_input(x, labels, n_classes, every_class=True)
  Kz = 1 if form else K
  c = _lr_penalty(C_)
  if not float(tol) > 0 or not np.isfinite(float(tol)):
    raise ValueError(f"tol must be finite and > 0, got {tol}")
  if int(max_iter) < 1:
    raise ValueError(f"max_iter must be >= 1, got {max_iter}")
  if (W0 is None) != (b0 is None):
    raise ValueError("the warm start is W0 and b0, or neither")
  w0, bb0 = (None, None) if W0 is None else _lr_params(W0, b0, Kz, G, "W0")
  lib = _hip.require_gpu()
  W, b = np.empty((Kz, G), np.float64), np.empty((Kz,), np.float64)
  F, gmax, n_iter, n_eval, conv = C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_logreg_fit(_fp(dense), *ptrs, N, G, _ip(lab), K, form, c, int(bool(fit_intercept)), float(tol), int(max_iter),
                           None if w0 is None else _dp(w0), None if bb0 is None else _dp(bb0), _dp(W), _dp(b), C.byref(F), C.byref(gmax), C.byref(n_iter), C.byref(n_eval), C.byref(conv)))
  return dict(W=W, b=b, F=F.value, gmax=gmax.value, n_iter=n_iter.value, n_eval=n_eval.value, converged=bool(conv.value))


def k_logreg_decision(x, W, b, n_classes: int, block_rows: int = 0):
  """smx_logreg_decision: the logits x.w + b of every row, float64 [N, n_classes], or [N] for two classes (W [1, G]); the matrix is
  streamed in blocks of block_rows rows (0: the library's choice; it changes no bit)"""
  dense, csr, N, G, K, form, _ = _lr_input(x, None, n_classes, block_rows, resident=False)
  Kz = 1 if form else K
  w, bb = _lr_params(W, b, Kz, G)
  lib = _hip.require_gpu()
  z = np.empty((N, Kz), np.float64)
  ptrs = (None, None, None) if csr is None else _csr_ptrs(csr)
  check(lib.smx_logreg_decision(_fp(dense), *ptrs, N, G, int(block_rows), K, form, _dp(w), _dp(bb), _dp(z)))
  return z[:, 0] if form else z


LOUVAIN_MAX_VERTICES, LOUVAIN_MAX_ENTRIES = 2 ** 24, 2 ** 31 - 1


def louvain_table_degree() -> int:
  """smx_louvain_table_degree: rows of up to this many stored entries are moved by one wave with a hash table in LDS, longer ones by one
  workgroup with a sort.  Needs no device."""
  return int(_hip.load().smx_louvain_table_degree())


def _louvain_graph(indptr, cols, weights, n):
  """The CSR arguments of smx_louvain*, shape- and range-checked so that a refusal never asks for the device; symmetry is the caller's
  (sisua_amd.communities) and the library's to check"""
  n = int(n)
  ip, cj = np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(cols, dtype=np.int32)
  if not 1 <= n <= LOUVAIN_MAX_VERTICES:
    raise ValueError(f"the graph must have 1 .. 2^24 vertices, got {n}")
  if ip.shape != (n + 1,) or ip[0] != 0 or (np.diff(ip) < 0).any() or cj.shape != (int(ip[-1]),) or ip[-1] > LOUVAIN_MAX_ENTRIES:
    raise ValueError(f"indptr must be [{n + 1}] from 0, not decreasing, and cols [indptr[-1] <= 2^31 - 1]")
  if cj.size and (cj.min() < 0 or cj.max() >= n):
    raise ValueError("cols holds an index outside 0 .. n - 1")
  w = None
  if weights is not None:
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != cj.shape or not (np.isfinite(w).all() and (w >= 0).all()):
      raise ValueError("weights must be one per entry, finite and >= 0")
  return ip, cj, w, n


def k_louvain(indptr, cols, weights, n, resolution: float = 1.0, tol: float = 1e-7, max_sweeps: int = 100, max_levels: int = 32) -> dict:
  """smx_louvain: the communities of the symmetric CSR graph (indptr [n + 1], cols, weights float64 or None for unit weights) ->
  dict(labels int64 [n] (ids by decreasing size, ties to the lowest member), n_communities, n_levels, and per level run modularity,
  level_size, sweeps, colours)"""
  ip, cj, w, n = _louvain_graph(indptr, cols, weights, n)
  resolution, tol, max_sweeps, max_levels = float(resolution), float(tol), int(max_sweeps), int(max_levels)
  if not (np.isfinite(resolution) and resolution >= 0 and np.isfinite(tol) and tol >= 0):
    raise ValueError(f"resolution and tol must be finite and >= 0, got {resolution} and {tol}")
  if max_sweeps < 1 or not 1 <= max_levels <= 4096:
    raise ValueError(f"max_sweeps >= 1 and 1 <= max_levels <= 4096 are required, got {max_sweeps} and {max_levels}")
  lib = _hip.require_gpu()
  labels, nc, nl = np.empty((n,), np.int32), C.c_int32(), C.c_int32()
  q, size = np.zeros((max_levels,), np.float64), np.zeros((max_levels,), np.int64)
  sweeps, colours = np.zeros((max_levels,), np.int32), np.zeros((max_levels,), np.int32)
  check(lib.smx_louvain(ip.ctypes.data_as(C.POINTER(C.c_int64)), _ip(cj), None if w is None else _dp(w), n, resolution, tol, max_sweeps,
                        max_levels, _ip(labels), C.byref(nc), C.byref(nl), _dp(q), size.ctypes.data_as(C.POINTER(C.c_int64)), _ip(sweeps),
                        _ip(colours)))
  L = nl.value
  return dict(labels=labels.astype(np.int64), n_communities=int(nc.value), n_levels=int(L), modularity=q[:L], level_size=size[:L],
              sweeps=sweeps[:L], colours=colours[:L])


def k_modularity(indptr, cols, weights, n, labels, resolution: float = 1.0) -> float:
  """smx_louvain_modularity: Q of the partition labels [n] (ids in 0 .. n - 1) of the graph, with smx_louvain's integers and sum order"""
  ip, cj, w, n = _louvain_graph(indptr, cols, weights, n)
  lab = np.ascontiguousarray(labels, dtype=np.int32)
  if lab.shape != (n,) or lab.min() < 0 or lab.max() >= n:
    raise ValueError(f"labels must be [{n}] ids in 0 .. {n - 1}")
  resolution = float(resolution)
  if not (np.isfinite(resolution) and resolution >= 0):
    raise ValueError(f"resolution must be finite and >= 0, got {resolution}")
  lib = _hip.require_gpu()
  q = C.c_double()
  check(lib.smx_louvain_modularity(ip.ctypes.data_as(C.POINTER(C.c_int64)), _ip(cj), None if w is None else _dp(w), n, _ip(lab), resolution,
                                   C.byref(q)))
  return float(q.value)


def k_mi_cells(x, x_discrete: bool, y, y_discrete: bool, n_neighbors: int = 3) -> dict:
  """smx_k_mi_cells: ONE pair of prepared columns x, y [N] -> the per-cell quantities of its estimator and its value `mi`:
  cc: r [N] float64, nx, ny [N] int32;  cd (either discrete): kept, k, count, m [N] int32 (k and m 0 where not kept), r;
  dd: a, b (the labels' values), n_ab [R]: the non-empty cells of the contingency table sorted by (a, b)"""
  xv, yv = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
  if xv.ndim != 1 or xv.shape != yv.shape:
    raise ValueError(f"x and y must both be [cells], got {xv.shape} and {yv.shape}")
  if not (np.isfinite(xv).all() and np.isfinite(yv).all()):
    raise ValueError("x or y holds a value that is not finite")
  N = xv.shape[0]
  k = _mi_check(N, n_neighbors)
  lib = _hip.require_gpu()
  psi, logn = _mi_tables(N)
  cells, radius, mi = np.empty((4, N), np.int32), np.empty((N,), np.float64), C.c_double()
  check(lib.smx_k_mi_cells(_dp(xv), int(bool(x_discrete)), _dp(yv), int(bool(y_discrete)), N, k, _dp(psi), _dp(logn), _ip(cells), _dp(radius),
                           C.byref(mi)))
  if x_discrete and y_discrete:
    heads = np.flatnonzero(cells[2] > 0)
    at = cells[3][heads]
    return dict(a=xv[at], b=yv[at], n_ab=cells[2][heads].copy(), mi=mi.value)
  if not x_discrete and not y_discrete:
    return dict(r=radius, nx=cells[0] - 1, ny=cells[1] - 1, mi=mi.value)
  return dict(kept=(cells[1] > 0).astype(np.int32), k=cells[0].copy(), count=cells[3].copy(), m=cells[2].copy(), r=radius, mi=mi.value)


def k_noise(seed, stream, step, cell_ids, width, p=0.0, sample=0):
  lib = _hip.require_gpu()
  ids = np.ascontiguousarray(cell_ids, dtype=np.int64)
  mult = np.empty((ids.size, width), np.float32)
  nrm = np.empty((ids.size, width), np.float32)
  check(lib.smx_k_noise(int(seed), int(stream), int(step), int(sample), ids.ctypes.data_as(C.POINTER(C.c_int64)),
                        ids.size, int(width), float(p), _fp(mult), _fp(nrm)))
  return mult, nrm


def _bn_vec(a, Hp):
  """A per-column vector as the BatchNorm entries take it: [Hp] float32 (a shorter one is padded with zeros), None stays None"""
  if a is None:
    return None
  a = np.asarray(a, np.float32).ravel()
  if a.size < Hp:
    a = np.concatenate([a, np.zeros(Hp - a.size, np.float32)])
  return np.ascontiguousarray(a[:Hp])


def _bn_slabs(x, wide):
  """slabs [S][B][ld] (or [B][ld]) / wide [S][Hp][128] -> (array, S, rows, ld)"""
  x = _f32(x)
  if x.ndim == 2:
    x = x[None]
  if x.ndim != 3 or (wide and x.shape[2] != 128):
    raise ValueError("slabs are [S][B][ld], wide ones [S][Hp][128]")
  return x, x.shape[0], x.shape[1], x.shape[2]


def k_bn_fwd(pre, B, H, Hp, gamma=None, beta=None, bias=None, moving_mean=None, moving_var=None, batchnorm=True, training=True,
             update_moving=True, momentum=0.99, eps=1e-3, leak=0.0, act="relu", drop_p=0.0, mask=None, seed=0, stream=0, step=0,
             rows=None, cell_base=0, wide=False, world=0):
  """The forward BatchNorm launch by itself (smx_k_bn_fwd): `pre` = slabs [S][B][ld], or with `wide` the column-major [S][Hp][128].
  Returns dict(out, xhat [B][Hp]; inv_std, batch_mean, batch_var, moving_mean, moving_var [Hp]; guards_ok).  What the launch does not
  write (batch statistics in evaluation mode, everything of BatchNorm without it) comes back as NaN."""
  lib = _hip.require_gpu()
  pre, S, r, ld = _bn_slabs(pre, wide)
  if (wide and r != Hp) or (not wide and r != B):
    raise ValueError("slab rows do not match B (wide: Hp)")
  g, b, bi, mm, mv = (_bn_vec(v, Hp) for v in (gamma, beta, bias, moving_mean, moving_var))
  m = None if mask is None else _f32(mask)
  rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
  ip = np.array([S, B, H, Hp, Hp if wide else ld, int(wide), int(batchnorm), int(training), int(update_moving), _hip.HIDDEN_ACTIVATIONS[act],
                 0 if m is None else m.shape[1], stream, step, cell_base, world], np.int32)
  fp = np.array([momentum, eps, leak, drop_p], np.float32)
  o = dict(out=np.empty((B, Hp), np.float32), xhat=np.empty((B, Hp), np.float32))
  for k in ("inv_std", "batch_mean", "batch_var", "moving_mean", "moving_var"):
    o[k] = np.empty(Hp, np.float32)
  ok = C.c_int32(0)
  check(lib.smx_k_bn_fwd(_ip(ip), _fp(fp), _fp(pre), _fp(g), _fp(b), _fp(bi), _fp(mm), _fp(mv), _fp(m), None if rw is None else _ip(rw), int(seed),
                         _fp(o["out"]), _fp(o["xhat"]), _fp(o["inv_std"]), _fp(o["batch_mean"]), _fp(o["batch_var"]), _fp(o["moving_mean"]),
                         _fp(o["moving_var"]), C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def k_bn_bwd(dout, out, xhat, B, H, Hp, inv_std=None, gamma=None, beta=None, batchnorm=True, training=True, leak=0.0, act="relu", drop_p=0.0,
             mask=None, seed=0, stream=0, step=0, rows=None, cell_base=0, wide=False, world=0):
  """The backward BatchNorm launch by itself (smx_k_bn_bwd) on its inputs: the d out slabs (laid out as k_bn_fwd's), the forward's out and
  xhat [B][Hp], inv_std, gamma, beta.  Returns dict(dpre [B][Hp]; dgamma, dbeta [max(world, 1)][Hp]; dbias [Hp]; guards_ok)."""
  lib = _hip.require_gpu()
  dout, S, r, ld = _bn_slabs(dout, wide)
  if (wide and r != Hp) or (not wide and r != B):
    raise ValueError("slab rows do not match B (wide: Hp)")
  out, xhat = _f32(out, (B, Hp)), _f32(xhat, (B, Hp))
  iv, g, b = (_bn_vec(v, Hp) for v in (inv_std, gamma, beta))
  m = None if mask is None else _f32(mask)
  rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
  ip = np.array([S, B, H, Hp, Hp if wide else ld, int(wide), int(batchnorm), int(training), _hip.HIDDEN_ACTIVATIONS[act],
                 0 if m is None else m.shape[1], stream, step, cell_base, world], np.int32)
  fp = np.array([leak, drop_p], np.float32)
  nw = max(int(world), 1)
  o = dict(dpre=np.empty((B, Hp), np.float32), dgamma=np.empty((nw, Hp), np.float32), dbeta=np.empty((nw, Hp), np.float32),
           dbias=np.empty(Hp, np.float32))
  ok = C.c_int32(0)
  check(lib.smx_k_bn_bwd(_ip(ip), _fp(fp), _fp(dout), _fp(out), _fp(xhat), _fp(iv), _fp(g), _fp(b), _fp(m), None if rw is None else _ip(rw),
                         int(seed), _fp(o["dpre"]), _fp(o["dgamma"]), _fp(o["dbeta"]), _fp(o["dbias"]), C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def _scvi_layout(G, k, Gp, plane_stride, ld):
  """The step's layout of the scVI head's planes unless overridden: Gp = G rounded up to 32, plane_stride = Gp, ld = k Gp"""
  Gp = (int(G) + 31) // 32 * 32 if Gp is None else int(Gp)
  ps = Gp if plane_stride is None else int(plane_stride)
  return Gp, ps, (k - 1) * ps + Gp if ld is None else int(ld)


def k_scvi_head_train(raw, x, hl, Wl, bl, library, G, likelihood="zinbd", rows=None, x_identity=False, eps=None, clip_library=1e3,
                      grad_scale=1.0, kl_weight=0.0, ldl=2, Gp=None, plane_stride=None, ld=None, seed=0, stream=65, step=0, cell_base=0, omit=()):
  """The row-local training launch of the scVI gene head by itself (smx_k_scvi_head_train).  raw [B][ld] in the step's layout (plane c of a
  row at c * plane_stride); x [n_x][Gp] counts, float32 or uint16 (the dtype picks the kernel's load path); hl [B][Kl]; Wl [Kl][2]; bl [2];
  library [n_lib][2]; rows [B] (optional; with x_identity the rows of x are the minibatch's already); eps [B] the injected library noise
  (None: drawn on the device).  Returns every output of the kernel: draw [B][ld]; llk_part, l, sig, eps, kl, dl [B]; latl, dlatl [B][ldl];
  guards_ok.  A word the kernel did not write comes back as NaN.  omit: names of outputs handed to the launcher as NULL (it refuses)."""
  lib = _hip.require_gpu()
  k = 3 if likelihood == "zinbd" else 2
  Gp, ps, ld = _scvi_layout(G, k, Gp, plane_stride, ld)
  raw = _f32(raw)
  B = raw.shape[0]
  raw = _f32(raw.reshape(B, -1), (B, ld))
  u16 = np.asarray(x).dtype == np.uint16
  x = np.ascontiguousarray(x, dtype=np.uint16 if u16 else np.float32)
  if x.ndim != 2 or x.shape[1] < Gp:
    raise ValueError(f"x must be [rows][>= Gp = {Gp}], got {x.shape}")
  hl, Wl = _f32(hl), _f32(Wl)
  if hl.ndim != 2 or hl.shape[0] != B or Wl.shape != (hl.shape[1], 2):
    raise ValueError(f"hl must be [B, Kl] and Wl [Kl, 2], got {hl.shape} and {Wl.shape}")
  bl, library = _f32(bl, (2,)), _f32(library)
  if library.ndim != 2 or library.shape[1] != 2:
    raise ValueError(f"library must be [n, 2], got {library.shape}")
  rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
  ep = None if eps is None else _f32(eps, (B,))
  ip = np.array([B, G, Gp, ps, ld, _hip.LIKELIHOODS[likelihood], int(u16), x.shape[0], x.shape[1], hl.shape[1], hl.shape[1], 2, library.shape[0],
                 int(bool(x_identity)), ldl, stream, step, cell_base], np.int32)
  fp = np.array([clip_library, grad_scale, kl_weight], np.float32)
  o = dict(draw=np.empty((B, ld), np.float32), latl=np.empty((B, ldl), np.float32), dlatl=np.empty((B, ldl), np.float32))
  for name in ("llk_part", "l", "sig", "eps", "kl", "dl"):
    o[name] = np.empty(B, np.float32)
  p = {name: (None if name in omit else _fp(a)) for name, a in o.items()}
  ok = C.c_int32(0)
  check(lib.smx_k_scvi_head_train(_ip(ip), _fp(fp), _fp(raw), x.ctypes.data_as(C.c_void_p), _fp(hl), _fp(Wl), _fp(bl), _fp(library),
                                  None if rw is None else _ip(rw), _fp(ep), int(seed), p["draw"], p["llk_part"], p["l"], p["sig"], p["eps"], p["kl"],
                                  p["latl"], p["dlatl"], p["dl"], C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def k_scvi_head_fwd(raw, l, G, k=3, clip_library=1e3, Gp=None, plane_stride=None, ld=None, omit=()):
  """The separate forward launch of the scVI gene head (smx_k_scvi_head_fwd): raw [B][ld], l [B] -> dict(planes [B][ld], rho_raw [B][Gp],
  guards_ok)"""
  lib = _hip.require_gpu()
  Gp, ps, ld = _scvi_layout(G, k, Gp, plane_stride, ld)
  raw = _f32(raw)
  B = raw.shape[0]
  raw, l = _f32(raw.reshape(B, -1), (B, ld)), _f32(l, (B,))
  ip, fp = np.array([B, G, Gp, ps, ld, k], np.int32), np.array([clip_library], np.float32)
  o = dict(planes=np.empty((B, ld), np.float32), rho_raw=np.empty((B, Gp), np.float32))
  p = {name: (None if name in omit else _fp(a)) for name, a in o.items()}
  ok = C.c_int32(0)
  check(lib.smx_k_scvi_head_fwd(_ip(ip), _fp(fp), _fp(raw), _fp(l), p["planes"], p["rho_raw"], C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o


def k_scvi_head_bwd(planes, dplanes, rho_raw, l, G, k=3, clip_library=1e3, Gp=None, plane_stride=None, ld=None, omit=()):
  """The separate backward launch of the scVI gene head (smx_k_scvi_head_bwd) on its inputs: planes, dplanes [B][ld], rho_raw [B][Gp],
  l [B] -> dict(draw [B][ld], dl [B], guards_ok)"""
  lib = _hip.require_gpu()
  Gp, ps, ld = _scvi_layout(G, k, Gp, plane_stride, ld)
  planes = _f32(planes)
  B = planes.shape[0]
  planes, dplanes = _f32(planes.reshape(B, -1), (B, ld)), _f32(np.asarray(dplanes).reshape(B, -1), (B, ld))
  rho_raw, l = _f32(rho_raw, (B, Gp)), _f32(l, (B,))
  ip, fp = np.array([B, G, Gp, ps, ld, k], np.int32), np.array([clip_library], np.float32)
  o = dict(draw=np.empty((B, ld), np.float32), dl=np.empty(B, np.float32))
  p = {name: (None if name in omit else _fp(a)) for name, a in o.items()}
  ok = C.c_int32(0)
  check(lib.smx_k_scvi_head_bwd(_ip(ip), _fp(fp), _fp(planes), _fp(dplanes), _fp(rho_raw), _fp(l), p["draw"], p["dl"], C.byref(ok)))
  o["guards_ok"] = bool(ok.value)
  return o
