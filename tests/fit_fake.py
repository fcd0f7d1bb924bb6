"""A recording stand-in for `sisua_amd.models.Engine` and the cases of tests/golden/fit_transcript.npz: what SingleCellModel._fit asks of
the engine and the control plane, with no device.  The stand-in implements only what `_fit`, `_ensure_engine`, `_apply_schedules`,
`_validate` and `_checkpoint` call and records every call.  Its per-step metrics are a pure function of the GLOBAL step index, dyadic
rationals with small numerators, so that every float32 sum over an epoch is exact: the per-epoch means do not depend on how the loop
chunked the steps.  A case's transcript (`transcript`) holds what does not depend on chunking -- chunk boundaries follow the host thread's
timing -- as a dict of arrays.  CPU only; shared by tests/golden/make_fit_transcript.py and tests/test_fit_loop_host.py."""
import warnings

import numpy as np
import scipy.sparse as sp

from sisua_amd import interpolation

N_TRAIN, N_VALID, N_GENES, BATCH = 53, 19, 12, 8
METRIC_KEYS = ("loss", "nllk_x", "nllk_y", "kl", "kl_l", "tc", "dtc_loss", "nllk_o")
_MOD_DIV = ((16, 4), (8, 2), (4, 1), (32, 8), (5, 1), (3, 2), (7, 4), (11, 8))   # key i at step s: (s % mod) / div


def step_metrics(steps) -> dict:
  s = np.asarray(steps, np.int64)
  return {k: ((s % mod) / div).astype(np.float32) for k, (mod, div) in zip(METRIC_KEYS, _MOD_DIV)}


def fake_engine(step=0, world=1, nan_at=None, eval_losses=None):
  """A stand-in Engine class (install: monkeypatch.setattr(sisua_amd.models, "Engine", cls)).  step: the step count a new instance starts
  at (a restored model); world: its communicator's size; nan_at: the global step whose nan_flag is raised; eval_losses: the loss of the
  k-th validation pass (the last one repeats)."""

  class FakeEngine:
    instances = []

    def __init__(self, cfg, max_batch=256, device=0, init=True):
      self.cfg, self.max_batch, self.device, self.world = cfg, int(max_batch), device, world
      self.step = int(step)
      self.calls, self.uploads, self.orders, self.batch_sizes, self.evals = [], [], [], [], []
      self.n_gather = self._last_n = 0
      self._passes = []   # the step count of every validation pass so far
      type(self).instances.append(self)

    def set_train_draws(self, n_draws):
      self.calls.append(f"set_train_draws({int(n_draws)})")

    def set_optimizer(self, name="adam", **hp):
      self.calls.append(f"set_optimizer({name}, {sorted(hp.items())})")

    def set_sync_bn(self, on=True):
      self.calls.append(f"set_sync_bn({bool(on)})")

    def set_schedule(self, target, value):
      rec = interpolation.as_schedule(value, target)
      self.calls.append(f"set_schedule({target}, {rec.kind}, {rec.params})")
      return rec

    def upload(self, X, labels=(), library=None, label_mask=None, cell_id_base=0, storage="f32"):
      dense = np.asarray(X.toarray() if sp.issparse(X) else X, np.float32)
      self.uploads.append(dict(X=dense, sparse=bool(sp.issparse(X)), labels=[np.asarray(a, np.float32) for a in labels],
                               library=np.asarray(library, np.float32), mask=np.asarray(label_mask, bool),
                               cell_id_base=int(cell_id_base), storage=str(storage)))

    def train_steps(self, order, n_steps, batch, graph=False, metrics=False):
      order = np.asarray(order)
      assert order.dtype == np.int32 and order.size == n_steps * batch and n_steps >= 1
      self.orders.append(order.copy())
      self.batch_sizes += [int(batch)] * int(n_steps)
      steps = np.arange(self.step, self.step + n_steps)
      self.step += int(n_steps)
      self._last_n = int(n_steps)
      m = {k: float(v[-1]) for k, v in step_metrics(steps).items()}
      m["nan_flag"] = int(nan_at is not None and nan_at in steps)
      return m if metrics else None

    def metrics_history(self, n_steps):
      assert n_steps == self._last_n
      return step_metrics(np.arange(self.step - n_steps, self.step))

    def eval_step(self, row_ids):
      if not self._passes or self._passes[-1] != self.step:
        self._passes.append(self.step)
      self.evals.append((self.step, np.asarray(row_ids).copy()))
      k = len(self._passes) - 1
      loss = float(eval_losses[min(k, len(eval_losses) - 1)]) if eval_losses else (64 - self.step % 64) / 4.0
      return dict(loss=loss, nan_flag=0)

    def opt_gather(self):
      self.n_gather += 1

    def close(self):
      self.calls.append("close()")

  return FakeEngine


class StubPlane:
  """A ready control plane of `world` ranks whose collectives only count."""

  def __init__(self, rank, world=2):
    self.rank, self.world, self.n_barrier, self.n_sum = rank, world, 0, 0

  def barrier(self):
    self.n_barrier += 1

  def sum_array(self, a):
    self.n_sum += 1
    return np.asarray(a) * self.world   # (every rank holds the same value)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _counts(n, seed):
  rng = np.random.default_rng(seed)
  x = (rng.poisson(2.0, size=(n, N_GENES)) * (rng.uniform(size=(n, N_GENES)) < 0.4)).astype(np.float32)
  x[:, 0] += 1
  return x


def _datasets(M, sparse=False, labels=False, drop_remainder=True, shuffle=1000, valid=False, batch_size=BATCH):
  from sisua_amd.data import SingleCellOMIC
  out = []
  for n, seed in ((N_TRAIN, 3), (N_VALID, 4)):
    x = _counts(n, seed)
    sco = SingleCellOMIC(sp.csr_matrix(x) if sparse else x, name="toy")
    omics = ["transcriptomic"]
    if labels:
      sco.add_omic("proteomic", np.eye(3, dtype=np.float32)[(np.arange(n) * 7 + seed) % 3])
      omics.append("proteomic")
    out.append((sco, sco.create_dataset(omics, labels_percent=0.5 if labels else 0, batch_size=batch_size, drop_remainder=drop_remainder,
                                        shuffle=shuffle)))
  (sco, train), (_, va) = out
  return sco, train, (va if valid else None)


def _model(M, sco, labels=False, input_dropout=0.0):
  kw = dict(labels=[sco.get_rv("proteomic", "onehot")]) if labels else {}
  return M.VAE(outputs=sco.get_rv("transcriptomic", "zinb"), encoder=M.NetConf([16], input_dropout=input_dropout), decoder=M.NetConf([16]), **kw)


_ES_LOSSES = [10.0, 8.0, 7.9, 7.5, 7.5, 7.6, 7.45, 7.44, 7.0, 6.0, 5.0, 4.0]   # strict improvements at passes 0-3, 6, 7, ...; past the threshold at 0, 1 only
_ES = dict(earlystop_patience=2, earlystop_threshold=0.1, valid_freq=3, epochs=6)
_NOVAL = dict(drop_remainder=True)
_VAL = dict(drop_remainder=False, valid=True)
_DP = dict(data=_VAL, fit=dict(epochs=2, valid_freq=5, sync_bn=True), engine=dict(world=2))

# name -> dict(data=<_datasets kwargs>, model=<_model kwargs>, engine=<fake_engine kwargs>, fit=<fit kwargs> or a list of them (several
# fits of one model), ckpt=<pass a recording checkpoint>, plane=<rank of a StubPlane>, strip=<drop the dataset's label arrays>)
CASES = {
    "first_chunk": dict(data=_NOVAL, fit=dict(epochs=5)),
    "verbose": dict(data=_NOVAL, fit=dict(epochs=5, verbose=True)),
    "ragged_valid": dict(data=_VAL, fit=dict(epochs=4, valid_freq=5), ckpt=True),
    "max_iter": dict(data=_NOVAL, fit=dict(epochs=5, max_iter=10)),
    "resume_epochs": dict(data=_NOVAL, engine=dict(step=9), fit=dict(epochs=2)),
    "resume_total": dict(data=_NOVAL, engine=dict(step=9), fit=dict(epochs=4, epochs_are_total=True, max_iter=30)),
    "resume_max_iter": dict(data=_NOVAL, engine=dict(step=9), fit=dict(epochs=5, epochs_are_total=False, max_iter=4)),
    "earlystop_min3": dict(data=_VAL, engine=dict(eval_losses=_ES_LOSSES), fit=dict(earlystop_min_epoch=3, **_ES), ckpt=True),
    "earlystop": dict(data=_VAL, engine=dict(eval_losses=_ES_LOSSES), fit=dict(earlystop_min_epoch=-1, **_ES), ckpt=True),
    "valid_at_end": dict(data=_VAL, fit=dict(epochs=2, valid_freq=0), ckpt=True),
    "ckpt_at_end": dict(data=_NOVAL, fit=dict(epochs=2), ckpt=True),
    "shuffle0": dict(data=dict(drop_remainder=False, shuffle=0), fit=dict(epochs=3)),
    "shuffle1000": dict(data=dict(drop_remainder=False, shuffle=1000), fit=dict(epochs=3)),
    "csr": dict(data=dict(sparse=True, **_VAL), fit=dict(epochs=2, valid_freq=4)),
    "csr_input_dropout": dict(data=dict(sparse=True, **_VAL), model=dict(input_dropout=0.25), fit=dict(epochs=2, valid_freq=4)),
    "csr_u16": dict(data=dict(sparse=True, **_VAL), fit=dict(epochs=2, valid_freq=4, storage="u16")),
    "labels": dict(data=dict(labels=True, **_VAL), model=dict(labels=True), fit=dict(epochs=2, valid_freq=6)),
    "too_few_omics": dict(data=dict(labels=True, **_NOVAL), model=dict(labels=True), fit=dict(epochs=1), strip=True),
    "dp_global_rank0": dict(plane=0, **_DP),
    "dp_global_rank1": dict(plane=1, **_DP),
    "dp_per_rank": dict(plane=1, **dict(_DP, fit=dict(epochs=2, valid_freq=5, dp_batch="per_rank"))),
    "dp_indivisible": dict(plane=0, **dict(_DP, data=dict(batch_size=9, **_VAL))),
    "dp_bad": dict(plane=0, **dict(_DP, fit=dict(epochs=2, dp_batch="each"))),
    # (valid_freq=12 without a validation set: chunks end at multiples of 12 whatever the host thread's timing, so the message names 12)
    "nan_terminate": dict(data=_NOVAL, engine=dict(nan_at=11), fit=dict(epochs=5, valid_freq=12, terminate_on_nan=True)),
    "nan_warn": dict(data=_NOVAL, engine=dict(nan_at=11), fit=dict(epochs=5, valid_freq=12, terminate_on_nan=False)),
    "rmsprop": dict(data=_NOVAL, fit=dict(epochs=1, optimizer="rmsprop", learning_rate=2e-3)),
    "adam_after_sgd": dict(data=_NOVAL, fit=[dict(epochs=1, optimizer="sgd"), dict(epochs=1, optimizer="adam"), dict(epochs=1)]),
}


def transcript(name, M, install) -> dict:
  """The transcript of case `name`: M is sisua_amd.models, install(cls) puts the stand-in in place of M.Engine (monkeypatch.setattr in a
  test).  A dict of arrays, strings as unicode arrays -- what np.savez stores without pickling."""
  case = CASES[name]
  cls = fake_engine(**case.get("engine", {}))
  install(cls)
  sco, train, valid = _datasets(M, **case["data"])
  model = _model(M, sco, **case.get("model", {}))
  if case.get("strip"):
    train.arrays = train.arrays[:1]
  cp = StubPlane(case["plane"]) if "plane" in case else None
  ckpts = []
  fits = case["fit"] if isinstance(case["fit"], list) else [case["fit"]]
  error = ""
  with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter("always")
    try:
      for kw in fits:
        kw = dict(kw, distributed=cp if cp is not None else False)
        if case.get("ckpt"):
          kw["checkpoint"] = lambda: ckpts.append(model.step)
        model.fit(train, valid=valid, metadata=sco, **kw)
    except Exception as err:   # (the transcript holds its type and message)
      error = f"{type(err).__name__}: {err}"
  strs = lambda v: np.array(list(v), dtype=str) if len(v) else np.zeros(0, "<U1")
  ints = lambda v: np.asarray(list(v), np.int64)
  out = {"error": np.array(error), "warnings": strs([f"{w.category.__name__}: {w.message}" for w in caught]),
         "n_engines": ints([len(cls.instances)]), "checkpoints": ints(ckpts), "final_step": ints([model.step]), "device": ints([model.device])}
  if cp is not None:
    out["plane"] = ints([cp.n_barrier, cp.n_sum])
  for i, e in enumerate(cls.instances):
    p = f"engine{i}/"
    out[p + "calls"] = strs(e.calls)
    out[p + "max_batch_world_gather"] = ints([e.max_batch, e.world, e.n_gather])
    out[p + "order"] = np.concatenate(e.orders).astype(np.int32) if e.orders else np.zeros(0, np.int32)
    out[p + "batch_sizes"] = ints(e.batch_sizes)
    out[p + "eval_at"] = ints([s for s, _ in e.evals])
    out[p + "eval_ids"] = np.concatenate([ids for _, ids in e.evals]).astype(np.int32) if e.evals else np.zeros(0, np.int32)
    out[p + "eval_sizes"] = ints([len(ids) for _, ids in e.evals])
    for j, u in enumerate(e.uploads):
      q = f"{p}upload{j}/"
      out[q + "X"], out[q + "library"], out[q + "mask"] = u["X"], u["library"], u["mask"]
      out[q + "how"] = strs([u["storage"], "sparse" if u["sparse"] else "dense", str(u["cell_id_base"]), str(len(u["labels"]))])
      for l, a in enumerate(u["labels"]):
        out[f"{q}labels{l}"] = a
  for tag, hist in (("train_history", model.train_history), ("valid_history", model.valid_history)):
    out[tag] = strs(sorted(hist))
    for k, v in hist.items():
      out[f"{tag}/{k}"] = np.asarray(v, np.float64)
  return out
