"""The host-side parts of `SingleCellModel._fit` (sisua_amd/models.py), which is their sequence: who this rank is and which cells it
owns, the one resident matrix, the step range of the call, the epoch feed, the per-epoch history and the early-stop state.  The minibatch
schedule is a pure function of the optimiser step count (iteration `it` visits batch `it % steps_per_epoch` of the shuffle order of epoch
`it // steps_per_epoch`): that is what makes a resumed run bit-identical and data-parallel ranks agree, and it lives here.  Host code only:
no engine, no device (tests/test_fit_loop_host.py)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from sisua_amd.data import as_csr, epoch_order, is_sparse, iter_batches, shard_range
from sisua_amd.parallel import env_rank_world


def resolve_ranks(distributed, device: int):
  """fit's `distributed` -> (control plane or None, rank, local_rank, world): 'auto' / True read the launcher's environment, a ready
  control plane (tests: LocalControlPlane) brings its own rank and world, anything else is a single process."""
  if distributed in ("auto", True):
    return (None,) + tuple(env_rank_world())
  if hasattr(distributed, "rank") and hasattr(distributed, "world"):
    return distributed, distributed.rank, device, distributed.world
  return None, 0, 0, 1


def rank_shard(n_obs: int, B: int, drop_rem: bool, rank: int, world: int, dp_batch: str):
  """(per-rank batch, drop_remainder, lo, hi): rank r keeps cells [lo, hi) and draws `B / world` (dp_batch='global': the global batch is
  preserved) or `B` ('per_rank') of them per step."""
  if world <= 1:
    return B, drop_rem, 0, n_obs
  if dp_batch == "global":
    if B % world:
      raise ValueError(f"batch_size {B} is not divisible by the {world} ranks (dp_batch='global')")
    B = B // world
  elif dp_batch != "per_rank":
    raise ValueError("dp_batch must be 'global' or 'per_rank'")
  lo, hi = shard_range(n_obs, rank, world)
  return B, True, lo, hi   # (drop_remainder: every rank runs the same number of equal-size steps)


def join_rows(train, valid, lo: int, hi: int, n_lab: int):
  """Train (this rank's shard [lo, hi)) and validation cells as ONE resident matrix, validation rows offset by hi - lo:
  (X, label arrays, library, mask, whether the counts are sparse).  Sparse counts stay sparse: the rows are joined as CSR."""
  X = train.arrays[0][lo:hi]
  labs = [train.arrays[1 + j][lo:hi] for j in range(n_lab)]
  lib, mask = train.library[lo:hi], train.mask[lo:hi]
  sparse_x = is_sparse(X) or (valid is not None and is_sparse(valid.arrays[0]))
  if valid is not None:
    if sparse_x:
      import scipy.sparse as sp
      X = sp.vstack([as_csr(sp.csr_matrix(a), copy=False) for a in (X, valid.arrays[0])], format="csr")
    else:
      X = np.concatenate([X, valid.arrays[0]], 0)
    labs = [np.concatenate([a, valid.arrays[1 + j]], 0) for j, a in enumerate(labs)]
    lib = np.concatenate([lib, valid.library], 0)
    mask = np.concatenate([mask, valid.mask], 0)
  return X, labs, lib, mask, sparse_x


def default_storage(sparse_x: bool, input_dropout: float) -> str:
  """'csr' for sparse counts -- unless the model has input dropout: the sparse store cannot key it, such a model keeps the float32 store,
  filled from the CSR rows."""
  return "csr" if (sparse_x and not input_dropout > 0) else "f32"


def steps_per_epoch(n_cells: int, B: int, drop_rem: bool) -> int:
  return n_cells // B if drop_rem else -(-n_cells // B)


def epoch_batches(n_cells, B, drop_rem, shuffle, seed, ep):
  """The batches (row ids) of epoch `ep`: a pure function of (seed, epoch)."""
  return iter_batches(epoch_order(n_cells, ep, shuffle, seed), B, drop_rem)


class StepPlan:
  """The step range of one fit call and the length of its library calls.  `it0` is the engine's step, `ep0` its epoch, `it_end` where the
  call ends: `epochs` more epochs from `ep0` (epochs_are_total: epochs of the whole schedule), capped by `max_iter`.

  One library call covers every step up to the next event on the host's side -- a validation pass, the end of the schedule, a ragged batch,
  a progress line -- across epoch boundaries (at 26 steps per epoch a call per epoch left the device idle for ~8 % of the time between
  calls)."""

  def __init__(self, step, spe, epochs, max_iter, epochs_are_total, valid_freq, max_chunk):
    self.spe, self.max_chunk = spe, max_chunk
    self.valid_freq = valid_freq if valid_freq and valid_freq > 0 else 0
    self.it0 = int(step)
    self.ep0 = self.it0 // spe
    self.it_end = (int(epochs) if epochs_are_total else self.ep0 + int(epochs)) * spe
    if max_iter and max_iter > 0:
      # a resumed run (`epochs_are_total`: the schedule counts from step 0 of the experiment, train.py) keeps the ORIGINAL
      # cap: max_iter is then an absolute step count as well, not `max_iter` more steps from the restored one
      self.it_end = min(self.it_end, int(max_iter) if epochs_are_total else self.it0 + int(max_iter))
    self.first_call = True

  def want(self, it: int) -> int:
    """Steps of the library call that starts at step `it`."""
    until_valid = self.valid_freq - (it % self.valid_freq) if self.valid_freq else self.it_end - it
    want = max(1, min(self.it_end - it, until_valid, self.max_chunk))
    if self.first_call and want > 2 * self.spe:
      # the call's FIRST chunk is two epochs: the device starts after two epochs' schedule instead of after the ~20 a valid_freq of 500 spans
      # (4-6 ms of a 50-epoch fit), and the host thread prepares the rest while it runs; later chunks are as long as before
      want = 2 * self.spe - (it % self.spe)
    self.first_call = False
    return want

  def epochs_ahead(self, it: int) -> int:
    """How many epochs past the current one the call that starts at `it` will walk: what to prepare while the device runs."""
    nxt = min(self.it_end - it, self.valid_freq or self.max_chunk, self.max_chunk)
    return 2 + max(nxt, 0) // max(self.spe, 1)


class EpochFeed:
  """The batches of every epoch that starts before step `it_end`, prepared ahead on one host thread (`prepare`: epoch_batches); `gather`
  cuts the next library call's row ids out of them.  A context manager: leaving it cancels what is still queued and joins the thread."""

  def __init__(self, n_cells, B, drop_rem, shuffle, seed, it_end):
    self.n_cells, self.B, self.drop_rem, self.shuffle, self.seed, self.it_end = n_cells, B, drop_rem, shuffle, seed, it_end
    self.spe = steps_per_epoch(n_cells, B, drop_rem)
    self.pool = ThreadPoolExecutor(max_workers=1)
    self.cache, self.pending = {}, {}

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    for f in self.pending.values():
      f.cancel()
    self.pool.shutdown(wait=True)

  def prepare(self, ep):   # prepared on the host thread while the device runs the epoch before
    return epoch_batches(self.n_cells, self.B, self.drop_rem, self.shuffle, self.seed, ep)

  def batches_of(self, ep):
    if ep not in self.cache:
      self.cache[ep] = self.pending.pop(ep).result() if ep in self.pending else self.prepare(ep)
    return self.cache[ep]

  def prefetch(self, ep_from, ep_to):   # on the host thread, while the device runs the chunk just launched
    for ep in range(ep_from, ep_to):
      if ep not in self.cache and ep not in self.pending and ep * self.spe < self.it_end:
        self.pending[ep] = self.pool.submit(self.prepare, ep)

  def _run(self, b, pos, room, bs):
    """(length, batch size) of the run of equal-size batches of epoch `b` from `pos`, at most `room` long; `bs`: the size so far or None."""
    if self.drop_rem:   # every batch has B cells: the run's length is arithmetic
      return min(self.spe - pos, room), self.B
    take = 0
    while pos + take < self.spe and take < room and (bs is None or len(b[pos + take]) == bs):
      if bs is None:
        bs = len(b[pos])   # a ragged last batch (drop_remainder=False, the reference's default for fit(SingleCellOMIC)) is a step of its own
      take += 1
    return take, bs

  def gather(self, it: int, want: int):
    """(order, n, bs): the row ids of the n <= want steps from step `it` on, all of batch size bs, walking over epoch boundaries."""
    parts, n, bs, j = [], 0, None, it
    while n < want:
      ep, pos = divmod(j, self.spe)
      if n > 0 and ep not in self.cache and ep in self.pending and not self.pending[ep].done():
        break   # (the host thread is still preparing that epoch: launch what is gathered instead of waiting for it)
      b = self.batches_of(ep)
      take, bs = self._run(b, pos, want - n, bs)
      if take == 0:
        break
      parts += b[pos:pos + take]
      n += take
      j += take
      if pos + take < self.spe:   # stopped inside the epoch (ragged batch ahead or enough steps)
        break
    for ep in [k for k in self.cache if k < it // self.spe]:   # (epochs already walked)
      del self.cache[ep]
    return np.concatenate(parts).astype(np.int32), n, bs


class EpochHistory:
  """`train_history[k]`: one value per epoch, the float32 mean over the epoch's steps of the per-step scalars the device keeps
  (smx_metrics_history), cut at the epoch boundaries after each library call."""

  def __init__(self, hist: dict, spe: int):
    self.hist, self.spe, self.acc = hist, spe, {}

  def add(self, it: int, n: int, h: dict):
    """The n steps from step `it` on; h[key] holds their scalars.  Every key at once: one reduction per epoch, not one per key and epoch."""
    keys = list(h)
    H = np.stack([np.asarray(h[k], np.float32) for k in keys])   # [key][step]
    s0 = 0
    while s0 < n:
      ep_here = (it + s0) // self.spe
      s1 = min(n, (ep_here + 1) * self.spe - it)
      done = it + s1 == (ep_here + 1) * self.spe   # the epoch is complete: one value per epoch, the mean over its steps
      if done and not self.acc:
        for k, mean in zip(keys, H[:, s0:s1].mean(axis=1)):
          self.hist.setdefault(k, []).append(float(mean))
      else:
        for i_k, k in enumerate(keys):
          self.acc.setdefault(k, []).append(H[i_k, s0:s1])
        if done:
          self.flush()
      s0 = s1

  def flush(self):
    """The mean over the steps that ran of an epoch that is open: the schedule ended (max_iter, early stop) inside it."""
    for k, seg in self.acc.items():
      self.hist.setdefault(k, []).append(float(np.mean(np.concatenate(seg))))
    self.acc = {}


class EarlyStop:
  """Best validation loss so far and the count of passes without an improvement by `threshold` (relative)."""

  def __init__(self, threshold, patience, min_epoch):
    self.threshold, self.patience, self.min_epoch = float(threshold), patience, int(min_epoch)
    self.best, self.bad = np.inf, 0

  def update(self, vl: float, epoch: int):
    """One validation pass -> (checkpoint: the loss is the best so far, strictly; stop: `patience` passes without improvement, from
    `min_epoch` on)."""
    improved = vl < self.best * (1.0 - self.threshold) if np.isfinite(self.best) else True
    better = vl < self.best
    if better:
      self.best = vl
    self.bad = 0 if improved else self.bad + 1
    return better, bool(self.patience and self.bad >= int(self.patience) and epoch >= self.min_epoch)
