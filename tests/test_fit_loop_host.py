"""The host side of SingleCellModel._fit without a device: every case of tests/golden/fit_transcript.npz (written from the loop as it was
before it was split into sisua_amd/fit_loop.py; tests/golden/make_fit_transcript.py) replayed against the recording stand-in engine of
tests/fit_fake.py, and the parts of fit_loop alone -- the epoch feed against the naive enumeration of the schedule, the per-epoch history
against float64 means under the worst-case float32 summation bound, the early-stop state against a restatement.  CPU only."""
import os
import threading

import numpy as np
import pytest

from sisua_amd import data
from tests import fit_fake as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_transcript.npz")


@pytest.fixture(scope="module")
def golden():
  z = np.load(GOLDEN)
  return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(F.CASES))
def test_fit_matches_the_transcript(monkeypatch, golden, name):
  import sisua_amd.models as M
  got = F.transcript(name, M, lambda cls: monkeypatch.setattr(M, "Engine", cls))
  want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
  assert want and sorted(got) == sorted(want)
  for k, v in want.items():
    g = np.asarray(got[k])
    assert g.shape == v.shape and g.dtype.kind == v.dtype.kind and np.array_equal(g, v), (k, g, v)


def test_the_transcript_covers_what_it_is_meant_to(golden):
  """The fixture's own claims: the cases take the branches they are named for."""
  g = lambda k: golden[k]
  assert set(g("first_chunk/engine0/batch_sizes")) == {8} and len(g("first_chunk/train_history/loss")) == 5
  assert set(g("ragged_valid/engine0/batch_sizes")) == {8, 5} and len(g("ragged_valid/engine0/batch_sizes")) == 28
  assert list(np.unique(g("ragged_valid/engine0/eval_at"))) == [5, 10, 15, 20, 25]
  assert g("max_iter/final_step")[0] == 10 and len(g("max_iter/train_history/loss")) == 2   # (the tail flush)
  assert [int(g(f"resume_{c}/final_step")[0]) for c in ("epochs", "total", "max_iter")] == [18, 24, 13]
  assert list(g("earlystop/checkpoints")) == [3, 6, 9, 12] and g("earlystop/final_step")[0] == 12
  assert list(g("earlystop_min3/checkpoints")) == [3, 6, 9, 12, 21, 24] and g("earlystop_min3/final_step")[0] == 24
  assert list(np.unique(g("valid_at_end/engine0/eval_at"))) == [14] and list(g("ckpt_at_end/checkpoints")) == [12]
  assert [str(g(f"{c}/engine0/upload0/how")[0]) for c in ("csr", "csr_input_dropout", "csr_u16", "labels")] == ["csr", "f32", "u16", "f32"]
  assert str(g("labels/engine0/upload0/how")[3]) == "1" and g("labels/engine0/upload0/labels0").shape == (72, 3)
  assert str(g("too_few_omics/error")).startswith("ValueError: VAE needs 2 omics")
  for rank in (0, 1):   # shard [26 r, 26 r + 26), 4 cells per rank and step, every rank's own order, cell ids from lo
    c = f"dp_global_rank{rank}/"
    assert list(g(c + "engine0/upload0/how"))[:3] == ["f32", "dense", str(26 * rank)] and g(c + "engine0/upload0/X").shape == (26 + 19, 12)
    assert set(g(c + "engine0/batch_sizes")) == {4} and g(c + "final_step")[0] == 12 and list(g(c + "engine0/max_batch_world_gather"))[1:] == [2, 1]
    order = data.epoch_order(26, 0, 1000, 1 + 7919 * rank)
    assert np.array_equal(g(c + "engine0/order")[:24], order[:24])
  assert set(g("dp_per_rank/engine0/batch_sizes")) == {8}
  assert "not divisible" in str(g("dp_indivisible/error")) and "dp_batch must be" in str(g("dp_bad/error"))
  assert str(g("nan_terminate/error")) == "FloatingPointError: non-finite loss or gradient norm at iteration 12"
  assert list(g("nan_warn/warnings")) == ["UserWarning: non-finite loss or gradient norm at iteration 12"] and g("nan_warn/final_step")[0] == 30
  assert [c for c in g("rmsprop/engine0/calls") if c.startswith("set_optimizer")][0].startswith("set_optimizer(rmsprop")
  assert [c.split(",")[0] for c in g("adam_after_sgd/engine0/calls") if c.startswith("set_optimizer")] == ["set_optimizer(sgd", "set_optimizer(adam"]


# ---- the epoch feed --------------------------------------------------------------------------------------------------------------
def _naive_steps(n_cells, B, drop_rem, shuffle, seed, it0, n_steps):
  from sisua_amd.fit_loop import steps_per_epoch
  spe = steps_per_epoch(n_cells, B, drop_rem)
  return [data.iter_batches(data.epoch_order(n_cells, j // spe, shuffle, seed), B, drop_rem)[j % spe] for j in range(it0, it0 + n_steps)]


def _walk(feed, it0, wants, prefetch=True):
  """Drive a feed as _fit does: gather, then prefetch what the next call will walk.  -> [(order, n, bs, want)]"""
  it, out = it0, []
  with feed:
    if prefetch:
      feed.prefetch(it // feed.spe, it // feed.spe + 2)
    for want in wants:
      order, n, bs = feed.gather(it, want)
      out.append((order, n, bs, want))
      it += n
      if prefetch:
        feed.prefetch((it - 1) // feed.spe, (it - 1) // feed.spe + 3)
  return out


def _check_walk(out, n_cells, B, drop_rem, shuffle, seed, it0):
  total = sum(n for _, n, _, _ in out)
  ref = _naive_steps(n_cells, B, drop_rem, shuffle, seed, it0, total)
  j = 0
  for order, n, bs, want in out:
    assert 1 <= n <= want and order.dtype == np.int32 and order.size == n * bs
    for s in range(n):   # step by step: the batch the schedule names, all of one size
      assert len(ref[j]) == bs and np.array_equal(order[s * bs:(s + 1) * bs], ref[j]), (j, want)
      j += 1
  return total


@pytest.mark.parametrize("seed", range(12))
def test_epoch_feed_is_the_naive_enumeration(seed):
  from sisua_amd.fit_loop import EpochFeed
  rng = np.random.default_rng(seed)
  n_cells, B = int(rng.integers(9, 70)), int(rng.integers(1, 9))
  drop_rem, shuffle = bool(seed % 2), int(rng.choice([0, 5, 1000]))
  it0 = int(rng.integers(0, 40))
  wants = [1] * 3 + [int(w) for w in rng.choice([1, 2, 3, 7, 20, 200], size=14)] if seed % 3 else [1] * 25
  feed = EpochFeed(n_cells, B, drop_rem, shuffle, 11 + seed, it_end=10 ** 9)
  out = _walk(feed, it0, wants, prefetch=seed % 4 != 3)
  _check_walk(out, n_cells, B, drop_rem, shuffle, 11 + seed, it0)
  if drop_rem and seed % 4 == 3:   # (nothing prefetched: nothing is ever "not ready", every chunk is as long as asked)
    assert [n for _, n, _, _ in out] == wants
  assert all(k >= (it0 + sum(n for _, n, _, _ in out[:-1])) // feed.spe for k in feed.cache)   # epochs already walked are evicted


def test_epoch_feed_launches_what_is_gathered_when_the_next_epoch_is_not_ready():
  from sisua_amd.fit_loop import EpochFeed
  gate = threading.Event()

  class SlowFeed(EpochFeed):
    def prepare(self, ep):
      if ep >= 1 and threading.current_thread() is not threading.main_thread():
        assert gate.wait(30)
      return super().prepare(ep)

  feed = SlowFeed(30, 4, True, 1000, 3, it_end=10 ** 9)   # 7 steps per epoch
  with feed:
    feed.prefetch(0, 3)
    try:
      first = feed.gather(0, 20)    # epoch 0 is waited for (nothing gathered yet); epoch 1 is not ready: the chunk ends at the boundary
    finally:
      gate.set()                  # (whatever happened: the host thread is let go before the feed joins it)
    assert first[1] == 7
    second = feed.gather(7, 20)   # (a chunk's first epoch is always waited for)
    third = feed.gather(7 + second[1], 1)
  out = [first + (20,), second + (20,), third + (1,)]
  assert second[1] >= 7
  _check_walk(out, 30, 4, True, 1000, 3, 0)


# ---- the per-epoch history ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_epoch_history_does_not_depend_on_the_chunking(seed):
  from sisua_amd.fit_loop import EpochHistory
  rng = np.random.default_rng(100 + seed)
  spe, it0 = int(rng.integers(3, 30)), int(rng.integers(0, 50))
  total = int(rng.integers(2 * spe, 6 * spe))
  keys = ("loss", "kl", "nllk_x")
  full = {k: (rng.standard_normal(total) * 10 ** rng.uniform(-2, 3)).astype(np.float32) for k in keys}
  chunkings = [[1] * total, [total]]
  for _ in range(5):
    cuts = np.sort(rng.choice(np.arange(1, total), size=int(rng.integers(1, min(total - 1, 12))), replace=False))
    chunkings.append(list(np.diff(np.concatenate([[0], cuts, [total]]))))
  first_ep, last_ep = it0 // spe, (it0 + total - 1) // spe
  hists = []
  for sizes in chunkings:
    hist, s = {}, 0
    eh = EpochHistory(hist, spe)
    for n in sizes:
      eh.add(it0 + s, int(n), {k: v[s:s + n] for k, v in full.items()})
      s += int(n)
    eh.flush()
    eh.flush()   # (nothing open: nothing appended)
    hists.append(hist)
    assert sorted(hist) == sorted(keys) and all(len(hist[k]) == last_ep - first_ep + 1 for k in keys)
    for k in keys:
      for i, ep in enumerate(range(first_ep, last_ep + 1)):   # the tail flush included: the mean over the steps that ran
        seg = full[k][max(ep * spe, it0) - it0:min((ep + 1) * spe, it0 + total) - it0].astype(np.float64)
        assert abs(hist[k][i] - seg.mean()) <= spe * 2.0 ** -24 * np.abs(seg).max(), (k, ep, sizes)


# ---- the early-stop state --------------------------------------------------------------------------------------------------------
def _early_stop_restated(losses, epochs, threshold, patience, min_epoch):
  best, bad, out = np.inf, 0, []
  for vl, ep in zip(losses, epochs):
    improved = (not np.isfinite(best)) or vl < best * (1.0 - threshold)
    ckpt = vl < best
    best = min(best, vl)
    bad = 0 if improved else bad + 1
    out.append((ckpt, bool(patience) and bad >= patience and ep >= min_epoch))
  return out


@pytest.mark.parametrize("seed", range(10))
def test_early_stop_state(seed):
  from sisua_amd.fit_loop import EarlyStop
  rng = np.random.default_rng(200 + seed)
  n = 40
  losses = list(np.round(10.0 * np.exp(-0.05 * np.arange(n)) + rng.normal(0, 0.3, n), 1))   # (rounded: equal values occur)
  for i in rng.choice(n, 4, replace=False):
    losses[i] = np.inf
  losses[5] = losses[4]                      # an equal value
  losses[7] = min(losses[:7]) * 0.999        # an improvement smaller than the threshold
  if seed % 2:
    losses[0] = np.inf
  epochs = list(np.cumsum(rng.integers(0, 2, n)))
  threshold, patience, min_epoch = [0.001, 0.05, 0.1][seed % 3], [0, 2, 3, 20][seed % 4], [-1, 3, 8][seed % 3]
  es = EarlyStop(threshold, patience, min_epoch)
  got = [es.update(float(vl), int(ep)) for vl, ep in zip(losses, epochs)]
  assert got == _early_stop_restated(losses, epochs, threshold, patience, min_epoch)
