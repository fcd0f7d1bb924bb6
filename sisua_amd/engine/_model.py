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
from sisua_amd.engine._args import _csr3, _csr_ptrs, _dp, _f32, _fp, _fps, _ip, _matrix_ptrs, _ptr, _sparse
from sisua_amd.engine._correlate import _col_operands, _col_outputs

STREAM_INPUT_DROPOUT = 0
STREAM_ENC_DROPOUT = 16
STREAM_ENCL_DROPOUT = 32
STREAM_DEC_DROPOUT = 48
STREAM_EPS_Z = 64
STREAM_EPS_L = 65


def _check_u16(a):
  if a.size and (a.min() < 0 or a.max() > 65535 or not np.array_equal(a, np.floor(a))):
    raise ValueError("storage='u16' needs integer counts in [0, 65535]")


def _tril_scale(out):
  """A full-covariance posterior's results: z_scale = the marginal standard deviations sqrt(diag(L L^T)) of the factor the device returned."""
  L = out.get("scale_tril")
  if L is not None:
    out["z_scale"][...] = np.sqrt(np.square(L, dtype=np.float64).sum(-1))
  return out


def _out_f32(out, shape):
  """A result array of `shape`: a fresh one, or the caller's `out` once it is seen to be C-contiguous float32 of that shape."""
  if out is None:
    return np.empty(shape, np.float32)
  if out.dtype != np.float32 or tuple(out.shape) != shape or not out.flags.c_contiguous:
    raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
  return out


def _host_rows(x, n_genes: int, n_rows: Optional[int] = None):
  """Host rows as the (dense, csr) pair `_matrix_ptrs` takes: float32 [N, G] (shape-checked where n_rows is given) or, from scipy.sparse,
  their `_csr3` triple."""
  if _sparse(x):
    return None, _csr3(x, n_genes, n_rows)
  return _f32(x, None if n_rows is None else (n_rows, n_genes)), None


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
    check(self.lib.smx_set_schedule(self._h, _SCHED_TARGETS[target], rec.kind, _dp(p), len(p)))
    return rec

  def get_schedule(self, target: str):
    """The schedule in force for 'beta' or 'lr' as an interpolation.Schedule record (const at the config's value by default)."""
    kind, n = C.c_int32(), C.c_int32()
    check(self.lib.smx_get_schedule(self._h, _SCHED_TARGETS[target], C.byref(kind), None, 0, C.byref(n)))
    p = np.zeros(max(n.value, 1), np.float64)
    check(self.lib.smx_get_schedule(self._h, _SCHED_TARGETS[target], C.byref(kind), _dp(p), len(p),
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
      check(self.lib.smx_dataset_upload_u16(self._h, _ptr(X), n, *side, int(cell_id_base)))
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
    return (labs, lib_arr, mask_arr), (_fps(labs), _fp(lib_arr), _ptr(mask_arr))

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
    self._step_check(fn(self._h, _ip(ids), ids.size, C.byref(m) if metrics else None))
    return m.as_dict() if metrics else None

  def train_steps(self, order, n_steps: int, batch: int, graph: bool = False, metrics: bool = False):
    """order = None: the row ids made resident by stage_steps(order, n_steps, batch) (no host-to-device copy in this call)."""
    if order is None:
      ptr = None
    else:
      ids = self._ids(order)
      if ids.size != n_steps * batch:
        raise ValueError("order must hold n_steps * batch row ids")
      ptr = _ip(ids)
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
    check(self.lib.smx_train_stage(self._h, _ip(ids), int(n_steps), int(batch)))

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
    self._step_check(self.lib.smx_eval_step(self._h, _ip(ids), ids.size, C.byref(m)))
    return m.as_dict()

  def _cells(self, row_ids, x, library):
    """The cells of a call: resident row ids, or host rows x [B, G] with their library prior [B, 2] (optional): (B, the arrays, their
    pointers (row ids, rows, library)); the caller keeps the arrays alive through the call."""
    if row_ids is not None:
      ids = self._ids(row_ids)
      return ids.size, (ids,), (_ip(ids), None, None)
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

  def _staged(self, x, library, batch):
    """The input of a predict-family call, staged once: (rows, N, B, la) -- rows: the (dense, csr) pair `_matrix_ptrs` takes, float32
    [N, G] or, from scipy.sparse, the `_csr3` triple; the cells per pass (`batch`, at most max_batch); the library prior [N, 2] or None."""
    rows = _host_rows(x, self.cfg.n_genes)
    N = rows[0].shape[0] if rows[1] is None else rows[1][0].size - 1
    B = min(int(batch or self.max_batch), self.max_batch)
    la = None if library is None else _f32(library, (N, 2))
    return rows, N, B, la

  def predict(self, x, library=None, n_samples: int = 1, batch: Optional[int] = None, want_x_params: bool = True, want=None):
    """Eval-mode forward of a whole host matrix in one call (smx_predict): arrays over ALL cells, with a leading draw
    axis for z_sample / l_sample / x_params / y_params -- the layout of forward_samples with n = every cell.
    want_x_params=False: everything but the gene output's parameter planes (what a lazy result keeps on the device side).
    want: only the named outputs leave the device (see `_outputs`; the clustering scores ask for the latent means alone).
    x may be scipy.sparse (the same results bit for bit)."""
    (rows, N, B, la), S = self._staged(x, library, batch), int(n_samples)
    out, res = self._outputs(N, S, want_x_params and (want is None or "x_params" in want), want)
    check(self.lib.smx_predict(self._h, *_matrix_ptrs(*rows), _fp(la), N, B, S, *res))
    return _tril_scale(out)

  STATS = {"mean": 0, "variance": 1, "mean_over_samples": 2, "log_prob": 3, "sample": 4}

  def predict_stat(self, x, stat: str, library=None, n_samples: int = 1, batch: Optional[int] = None, count_only: bool = False,
                   target=None, out=None, seed: int = 0, n: int = 1, genes=None):
    """A statistic of the gene output over a whole host matrix (smx_predict_stat): the same passes and draws as predict(), but only the
    statistic leaves the device.  'mean' / 'variance' [n_samples, N, G]; 'mean_over_samples' [N, G]; 'log_prob' [n_samples, N] of `target`
    (default: of x itself).  count_only: the count distribution without the zero-inflation wrapper.  `out`: a float32 array of the
    result's shape to write into (a reused array saves the first-touch page faults of a fresh one).  x and target may each be scipy.sparse.
    'sample': [n, n_samples, N, G], n posterior-predictive draws of the gene output per Monte-Carlo draw and cell
    under the integer `seed` (smx_predict_sample: drawn on the device, the same bits at any batch size and from dense or sparse x).
    genes ('mean_over_samples' only): gene indices -- [N, len(genes)] leaves the device, the same bits as those columns (smx_predict_stat_cols)."""
    cfg = self.cfg
    if genes is not None:
      return self._predict_stat_cols(x, stat, library, n_samples, batch, count_only, target, out, genes)
    (rows, N, B, la), S, G = self._staged(x, library, batch), int(n_samples), cfg.n_genes
    code = self.STATS[stat]
    shape = (N, G) if code == 2 else (S, N) if code == 3 else (int(n), S, N, G) if code == 4 else (S, N, G)
    if code == 4 and (int(n) < 1 or target is not None):
      raise ValueError("'sample' takes n >= 1 and no target")
    out = _out_f32(out, shape)
    if code == 4:
      check(self.lib.smx_predict_sample(self._h, *_matrix_ptrs(*rows), _fp(la), N, B, S, int(bool(count_only)), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        int(n), _fp(out)))
      return out
    trows = (None, None) if target is None else _host_rows(target, G, N)   # (no target: the log_prob of the input rows themselves)
    check(self.lib.smx_predict_stat(self._h, *_matrix_ptrs(*rows), _fp(la), N, B, S, code, int(bool(count_only)), *_matrix_ptrs(*trows), _fp(out)))
    return out

  def _predict_stat_cols(self, x, stat, library, n_samples, batch, count_only, target, out, genes):
    cfg = self.cfg
    if stat != "mean_over_samples" or target is not None:
      raise ValueError("genes= goes with 'mean_over_samples' (and no target)")
    idx = gene_indices(genes, cfg.n_genes)
    (rows, N, B, la), S = self._staged(x, library, batch), int(n_samples)
    out = _out_f32(out, (N, idx.size))
    check(self.lib.smx_predict_stat_cols(self._h, *_matrix_ptrs(*rows), _fp(la), N, B, S, int(bool(count_only)), _ip(idx), idx.size, _fp(out)))
    return out

  def predict_impute(self, x, original, library=None, n_samples: int = 1, batch: Optional[int] = None, count_only: bool = False):
    """The imputation scores of predict_stat(x, 'mean_over_samples') against `original`, reduced on the device (smx_predict_impute): x is
    the CORRUPTED matrix the prediction is made from.  Returns dict(cell_median [N] float32: np.median(|original - mean|) of every cell;
    cell_changed [N] int32: sum(original row) != sum(x row); global_lohi [2] float32: the two middle order statistics of all N G absolute
    differences).  x and original may each be scipy.sparse; the bits do not depend on that, on the batch size or on the chunking."""
    cfg = self.cfg
    G = cfg.n_genes
    (rows, N, B, la), S = self._staged(x, library, batch), int(n_samples)
    if rows[1] is None and (rows[0].ndim != 2 or rows[0].shape[1] != G):
      raise ValueError(f"expected rows [n_cells, {G}], got {rows[0].shape}")
    if original is None:
      raise ValueError("predict_impute needs the original counts")
    orows = _host_rows(original, G, N)
    med, chg, lohi = np.empty((N,), np.float32), np.empty((N,), np.int32), np.empty((2,), np.float32)
    check(self.lib.smx_predict_impute(self._h, *_matrix_ptrs(*rows), _fp(la), N, B, S, int(bool(count_only)), *_matrix_ptrs(*orows),
                                      _fp(med), _ip(chg), _fp(lohi)))
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
    (rows, N, B, la), S = self._staged(x, library, batch), int(n_samples)
    if rows[1] is None and (rows[0].ndim != 2 or rows[0].shape[1] != G):
      raise ValueError(f"expected rows [n_cells, {G}], got {rows[0].shape}")
    idx = None if genes is None else gene_indices(genes, G)
    pr, pu = _col_operands(prot_rank2, prot_unit, N)
    out, res = _col_outputs(G if idx is None else idx.size, pr.shape[0])
    sel = (None, 0) if idx is None else (_ip(idx), idx.size)
    check(self.lib.smx_predict_correlate(self._h, *_matrix_ptrs(*rows), _fp(la), N, B, S, int(bool(count_only)), *sel, _ip(pr), _dp(pu),
                                         pr.shape[0], *res))
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
    """Importance-weighted log p(x) per cell and the mean reconstruction log-likelihood (GPU).  x may be scipy.sparse."""
    if row_ids is not None:
      ids = self._ids(row_ids)
      B, cells = ids.size, (_ip(ids), None, None, None, None, None)
    else:
      rows, B, _, la = self._staged(x, library, None)
      cells = (None, *_matrix_ptrs(*rows), _fp(la))
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
