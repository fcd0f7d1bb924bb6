// smx_backward.hip -- the backward pass of a training step as a launch sequence, and what rides with it: the heads' optimiser update as riders of
// the BatchNorm-backward launches, as a background sweep, or as the data-parallel chain; the FactorVAE discriminator's backward.
#include "smx_model.h"

namespace smx {

// Single GPU: once the head products have written dW / db of the output and label heads (3/4 of the parameters),
// their clip + Adam update rides along with the next BatchNorm-backward launch, which leaves most CUs idle; the
// optimiser launch at the end of the step then covers only the encoder / latent / decoder chunks.
// optimiser arguments of a launch that carries chunks of the heads' update as riders (norms from the products' partials, or from the
// sums the reduce riders of an earlier launch left)
static void fill_rider_adam(smx_model* m, AdamArgs& a) {
  fill_adam_args(m, a);
  a.use_sq = 1;
  for (size_t t = 0; t < m->tensors.size(); ++t) {
    a.sq_first[t] = m->sq_first[t]; a.sq_count[t] = m->sq_count[t];
    if (m->sq_reduced[t]) { a.sq_first[t] = m->sq_total_first + (int)t * SMX_SQR_PER_TENSOR; a.sq_count[t] = m->sq_reduced[t]; }   // (summed by the launch before)
  }
  a.master = nullptr; a.with_metrics = 0;
}

// wide panels: the latent head's backward product (four workgroups of its own) takes the first adam_ride_b of the waiting chunks;
// `store` must stay alive until the product is launched
static void take_adam_riders(smx_model* m, GemmArgs& h, AdamArgs& store) {
  const int n = std::min(m->adam_ride_b, m->adam_rest_to - m->adam_rest_from);
  m->adam_ride_b = 0;
  if (n <= 0) return;
  fill_rider_adam(m, store);
  h.ride_adam = &store; h.ride_first = m->adam_rest_from; h.ride_count = n;
  if (m->adam_early_from < 0) m->adam_early_from = m->adam_rest_from;
  m->adam_rest_from += n;
  m->adam_early_to = m->adam_rest_from;
}

static void attach_early_adam(smx_model* m, BnBwdArgs& b) {
  if (!m->adam_early_pending) {
    // the second part of the heads' update: riders of the NEXT BatchNorm-backward launch of the step (see below)
    if (m->adam_ride_b > 0) { m->adam_rest_to = std::max(m->adam_rest_from, m->adam_rest_to - m->adam_ride_b); m->adam_ride_b = 0; }   // (no product took its share)
    if (m->adam_rest_to > m->adam_rest_from) {
      fill_rider_adam(m, b.adam);
      b.adam_first = m->adam_rest_from; b.adam_count = m->adam_rest_to - m->adam_rest_from;
      if (m->adam_early_from < 0) m->adam_early_from = m->adam_rest_from;
      m->adam_early_to = m->adam_rest_to;
      m->adam_rest_from = m->adam_rest_to = 0;
    }
    return;
  }
  m->adam_early_pending = false;
  const bool off = tuning_on("no_adam_early");   // (read per step, like no_dw_late: a test flips it between engines)
  // (the riders carry Adam only -- smx_adam.h: SMX_OPT_SWITCH --: under another rule every chunk stays with the optimiser launch or the sweep)
  if (off || m->opt_rule != SMX_OPT_ADAM || dp_active(m) || !m->sq_slots || m->chunk_first_head >= m->n_chunks || tuning_on("no_sq_partials")) return;
  for (size_t t = (size_t)m->t_outW[0]; t < m->tensors.size(); ++t)   // head tensors are the last ones of the manifest
    if (m->sq_count[t] == 0 && m->tensors[t].count > SMX_SQ_SMALL_TENSOR) return;
  // riders use half of a 512-thread BatchNorm workgroup: fine while the heads' update is a few MB (C2: 22 MB, hidden
  // under the launch), but at the 20 000-gene width it ran at 2.8 TB/s against 6.2 TB/s for the optimiser's own launch.
  // There only the heads' sum-of-squares slots are reduced here (one rider workgroup per tensor with many slots:
  // 30 000 for the output head at 20 000 genes), so that each of the optimiser's ~1900 workgroups for that tensor
  // reads ONE number instead of sweeping all of them (225 MB of L2 reads, 66 -> 5x us of the optimiser launch).
  if ((long)(m->n_chunks - m->chunk_first_head) * m->chunks_floats > 512L * 4096) {
    fill_adam_args(m, b.adam);
    for (size_t t = 0; t < m->tensors.size(); ++t) { b.adam.sq_first[t] = m->sq_first[t]; b.adam.sq_count[t] = m->sq_count[t]; }
    for (size_t t = (size_t)m->t_outW[0]; t < m->tensors.size(); ++t) {
      const int cnt = m->sq_count[t];
      const int R = std::min(SMX_SQR_PER_TENSOR, (cnt + SMX_SQR_MIN_SLOTS - 1) / SMX_SQR_MIN_SLOTS);
      if (cnt <= SMX_SQR_MIN_SLOTS || b.sqr_count + R > SMX_SQR_MAX) continue;
      const int seg = ((cnt + R - 1) / R + 255) / 256 * 256;
      int r = 0;
      for (int lo = 0; lo < cnt; lo += seg, ++r) {
        const int i = b.sqr_count++;
        b.sqr_first[i] = m->sq_first[t] + lo; b.sqr_n[i] = std::min(seg, cnt - lo); b.sqr_dst[i] = (int)t * SMX_SQR_PER_TENSOR + r;
      }
      m->sq_reduced[t] = (char)r;   // the optimiser reads r partial sums for this tensor
    }
    b.sq_total = m->sq_slots + m->sq_total_first;
    // ... and a share of the heads' chunks rides with the NEXT BatchNorm-backward launch as full 512-thread workgroups (the norms are
    // single numbers by then): SMX_ADAM_WIDE_SHARE of them, the optimiser launch keeps the rest
    static const float share = (float)tuning("adam_wide_share", 0.3f);
    // ... and SMX_ADAM_WIDE_SHARE_B of them before that with the latent head's backward product (take_adam_riders)
    static const float share_b = (float)tuning("adam_wide_share_b", 0.1f);
    const int early_to = m->lab_deferred ? m->chunk_first_label : m->n_chunks;
    const int n = (int)((early_to - m->chunk_first_head) * std::min(std::max(share, 0.f), 1.f));
    const int nb = std::min((int)((early_to - m->chunk_first_head) * std::min(std::max(share_b, 0.f), 1.f)), early_to - m->chunk_first_head - n);
    if (n + nb > 0) { m->adam_rest_from = m->chunk_first_head; m->adam_rest_to = m->chunk_first_head + n + nb; m->adam_ride_b = nb; }
    return;
  }
  fill_adam_args(m, b.adam);
  b.adam.use_sq = 1;
  for (size_t t = 0; t < m->tensors.size(); ++t) { b.adam.sq_first[t] = m->sq_first[t]; b.adam.sq_count[t] = m->sq_count[t]; }
  b.adam.master = nullptr; b.adam.with_metrics = 0;
  // (label heads whose weight gradients come with the grouped launch at the END of the backward pass stay with the
  // optimiser launch)
  const int early_to = m->lab_deferred ? m->chunk_first_label : m->n_chunks;
  // the riders (22 MB of optimiser traffic at the benchmark size) set the duration of the launch that carries them (10 us against
  // 6 for its own work) while the NEXT BatchNorm-backward launch of the step leaves the chip as idle: split them over the two
  // (SMX_ADAM_SPLIT = share of the first, default 0.5; a step with one such launch keeps them all, the final launch takes what
  // nobody carried)
  static const float split_chain = (float)tuning("adam_split", 0.5f);
  // (dw_late_now: the decoder's last layer's launch carried the head's dW instead of riders -- this is the launch behind it, with a one-layer decoder
  // the encoder's and the last such launch of the step; what it leaves goes to the optimiser launch: adam_split_late, SMX_ADAM_SPLIT_LATE_DEFAULT)
  const float split = m->dw_late_now ? (float)tuning("adam_split_late", SMX_ADAM_SPLIT_LATE_DEFAULT) : split_chain;
  const int total = early_to - m->chunk_first_head;
  const int first = std::max(1, std::min(total, (int)(total * std::min(std::max(split, 0.f), 1.f) + 0.5f)));
  b.adam_first = m->chunk_first_head;
  b.adam_count = first;
  m->adam_early_from = m->chunk_first_head; m->adam_early_to = m->chunk_first_head + first;
  m->adam_rest_from = m->chunk_first_head + first; m->adam_rest_to = early_to;
  // ... of which SMX_ADAM_SPLIT_B of the total go with the latent head's backward product between the two (take_adam_riders)
  static const float split_b = (float)tuning("adam_split_b", 0.f);
  m->adam_ride_b = std::min((int)(total * std::min(std::max(split_b, 0.f), 1.f)), m->adam_rest_to - m->adam_rest_from);
}

// ---- wide panels, one GPU, eager steps: the heads' update as a background sweep ----
// dW / db of the output head are final when smx_headfused.hip's launch ends, and nobody reads the head's parameters before the NEXT step's
// output head: clip + Adam for the head's chunks (3/4 of the parameters at the C5 width) run on a second stream as `wgs` persistent
// workgroups beside the backward chain, the optimiser launch (which skips them) and the next step's encoder and decoder -- launches that
// leave most of the memory system idle.  The next reader of the head (forward_pass, below the decoder) and the end of every
// smx_train_steps call wait for the sweep's event, so every other entry point finds the stream order it always had.
// What it reads stays put meanwhile: the head's gradients and sum-of-squares slots are rewritten by the next output head only, and the
// step state of parity p by the optimiser launch of the step after next.
// It pays from ~6 M head parameters: a second queue with work in it costs every launch of the main stream ~1.5 us (the step at 4096 genes:
// 99.8 -> 117.3 us with the sweep, at 12 000: 139.9 -> 145.3, at 20 000: 181.6 -> 177.7; tools/head_fused_width_ab.py), which the hidden update
// has to buy back.  Workgroups: one per SMX_HEAD_SWEEP_CHUNKS_PER_WG chunks -- the sweep should last most of the window between two output heads.
static int head_sweep_wgs(const smx_model* m) {
  if (!m->flags.head_sweep) return 0;
  const int chunks = m->n_chunks - m->chunk_first_head;
  if (chunks < (int)tuning("adam_sweep_min_chunks", SMX_HEAD_SWEEP_MIN_CHUNKS)) return 0;
  const int forced = (int)tuning("adam_sweep_wgs", 0);
  return forced > 0 ? forced : std::min(std::max(chunks / SMX_HEAD_SWEEP_CHUNKS_PER_WG, 64), 256);
}
// the main stream behind the sweep (its event)
int head_sweep_join(smx_model* m) {
  if (!m->sweep_pending) return SMX_OK;
  m->sweep_pending = false;
  SMX_HIP(hipStreamWaitEvent(m->st, m->ev_sweep, 0));
  return SMX_OK;
}
// decided where the output head is launched (forward_pass), acted on where its gradients are known to be final (backward_pass)
// (With label heads -- SISUA, SCALAR, observed outputs: round 6 -- the sweep covers the OUTPUT head's chunks only: the label heads' gradients come from the
// grouped launch of the backward pass, which the second stream does not wait for; their chunks stay with the optimiser launch.)
static int head_sweep_end(const smx_model* m) { return m->n_heads > 0 ? m->chunk_first_label : m->n_chunks; }
bool head_sweep_ok(smx_model* m) {
  if (head_sweep_wgs(m) <= 0 || dp_active(m) || m->capturing || !m->timing_label.empty() || m->use_injected) return false;
  if (!m->sq_slots || m->chunk_first_head >= head_sweep_end(m) || tuning_on("no_sq_partials") || tuning_on("no_adam_early")) return false;
  const size_t t_end = m->n_heads > 0 ? (size_t)m->t_labW[0] : m->tensors.size();
  for (size_t t = (size_t)m->t_outW[0] + 1; t < t_end; ++t)   // (W_out's slots come from the output head's launch itself)
    if (m->sq_count[t] == 0 && m->tensors[t].count > SMX_SQ_SMALL_TENSOR) return false;
  return true;
}
int head_sweep_prepare(smx_model* m) {
  // one GPU: both ends of these events are queues of THIS device -- the kernels' own agent-scope release / acquire orders their memory, and the
  // system-scope fence an event record carries by default costs ~1.5 us at either end of the output head (c5-shard 156 -> 153 us, same bits;
  // knob event_system_fence).  With a communicator attached (peers read what the chain's collective sends) the default stays.
  const int mode = (dp_active(m) || tuning_on("event_system_fence")) ? 1 : 0;
  if (m->st_side && m->ev_mode == mode) return SMX_OK;
  if (!m->st_side) {
    int lo = 0, hi = 0;
    SMX_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    SMX_HIP(hipStreamCreateWithPriority(&m->st_side, hipStreamNonBlocking, lo));
  }
  if (m->ev_sweep) { hipEventDestroy(m->ev_sweep); m->ev_sweep = nullptr; }
  if (m->ev_hf) { hipEventDestroy(m->ev_hf); m->ev_hf = nullptr; }
  const unsigned fl = hipEventDisableTiming | (mode ? 0u : (unsigned)hipEventDisableSystemFence);
  SMX_HIP(hipEventCreateWithFlags(&m->ev_sweep, fl));
  SMX_HIP(hipEventCreateWithFlags(&m->ev_hf, fl));
  m->ev_mode = mode;
  return SMX_OK;
}
// behind the output head's launch (ev_hf) on the second stream
static int head_sweep_start(smx_model* m) {
  AdamArgs a;
  fill_rider_adam(m, a);
  static const bool skip = tuning_on("skip_head_adam");   // timing only (WRONG results): the heads are never updated -- what their update costs the step
  if (!skip) {
    SMX_HIP(hipStreamWaitEvent(m->st_side, m->ev_hf, 0));
    SMX_CHECK(launch_adam_sweep(m->st_side, a, m->chunk_first_head, head_sweep_end(m) - m->chunk_first_head, head_sweep_wgs(m)));
    SMX_HIP(hipEventRecord(m->ev_sweep, m->st_side));
    m->sweep_pending = true;
  }
  // the optimiser launch skips these chunks; no launch of the backward chain carries any of them
  m->adam_early_from = m->chunk_first_head; m->adam_early_to = head_sweep_end(m);
  m->adam_early_pending = false; m->adam_rest_from = m->adam_rest_to = 0; m->adam_ride_b = 0;
  return SMX_OK;
}

// Data parallel, two buckets (smx_comm.hip: dp_chain_ok): the heads' part of the step as ONE chain on the communication stream, started
// where the heads' gradients are final (`after`: an event of the model's stream recorded there) --
//   all-reduce of the head bucket (its own communicator)  ->  the chunks' sums of squares of the REDUCED gradient  ->  clip + Adam of the
//   heads' chunks (the sweep above, norms from those sums)
// -- and joined where the background sweep is joined: in front of the next step's output head and at the end of every smx_train_steps
// call.  The model's stream all-reduces the front bucket [encoder / latent / decoder | BatchNorm statistics | ELBO scalars] itself and
// updates the front chunks; it never waits for the communication stream inside a step (round 4's two-bucket form did, twice: +32-35 us on
// one rank).  Same arithmetic as the one-bucket step element by element (sum over ranks in RCCL's order, norm of the reduced gradient,
// clip, Adam); the per-tensor norm is summed per chunk, then over the tensor's chunks, as the optimiser launch does.
int dp_chain_start(smx_model* m) {
  if (m->chain_started) return SMX_OK;
  SMX_CHECK(head_sweep_prepare(m));
  SMX_HIP(hipEventRecord(m->ev_hf, m->st));
  SMX_HIP(hipStreamWaitEvent(m->st_comm, m->ev_hf, 0));
  AdamArgs a;
  fill_adam_args(m, a);
  a.use_sq = 0; a.master = nullptr; a.with_metrics = 0;
  const int first = m->chunk_first_head, count = m->n_chunks - m->chunk_first_head;
  const int forced = (int)tuning("adam_sweep_wgs", 0);
  const int wgs = forced > 0 ? forced : std::min(std::max(count / SMX_HEAD_SWEEP_CHUNKS_PER_WG, 64), 256);
  if (m->flags.opt_shard && (m->world > 1 || m->dp_force) && dp_shard_available(m)) {
    // The heads' optimiser state SHARDED over the ranks (flag opt_shard): the bucket is world slices of equal length (cut
    // at a 64-float boundary, through chunks where it falls; the flat buffers end in SMX_SHARD_SLACK floats so that the last slice exists);
    //   reduce-scatter (rank r gets the sums of slice r)  ->  per chunk, the sum of squares of its part inside the slice  ->  all-reduce of
    //   those partials (a few KB: the chunks' sums of squares of the whole reduced gradient, hence every tensor's norm, on every rank)  ->
    //   clip + Adam of the slice  ->  all-gather of the updated parameters.
    // The same bytes on the wire as the all-reduce (a ring all-reduce IS these two halves); clip + Adam read and write 28 bytes per parameter
    // of 1 / world of the heads instead of all of them (BASELINE configs[4] on 8 GPUs: 215 -> 27 MB per GPU and step).  Every updated element
    // is computed by ONE rank and copied: the replicas stay bit-identical.  The moments outside the slice go stale: smx_opt_gather.
    const size_t slice = (((size_t)m->bucket1_count + m->world - 1) / m->world + 63) / 64 * 64;
    SMX_REQUIRE((size_t)m->world * slice <= (size_t)m->bucket1_count + SMX_SHARD_SLACK, "opt_shard: too many ranks for the buffers' slack");
    SMX_CHECK(dp_reduce_scatter(m, m->grads + m->bucket1_off, slice, m->st_comm, true));
    a.partial = m->shard_partial;
    a.shard_lo = (long)(m->bucket1_off + (size_t)m->rank * slice);
    a.shard_hi = (long)std::min(m->bucket1_off + ((size_t)m->rank + 1) * slice, m->bucket1_off + (size_t)m->bucket1_count);
    SMX_CHECK(launch_grad_sqsum_shard(m->st_comm, a, first, count));
    SMX_CHECK(dp_allreduce_buf(m, m->shard_partial + first, (size_t)count, m->st_comm, true));
    SMX_CHECK(launch_head_norms(m->st_comm, a, first, count));
    if (a.shard_hi > a.shard_lo) SMX_CHECK(launch_adam_shard(m->st_comm, a, first, count, wgs));
    SMX_CHECK(dp_all_gather(m, m->params + m->bucket1_off, slice, m->st_comm, true));
    m->opt_stale = true;
  } else {
    SMX_CHECK(dp_allreduce(m, m->bucket1_off, m->bucket1_count, m->st_comm, true));
    SMX_CHECK(launch_grad_sqsum_range(m->st_comm, a, first, count));
    SMX_CHECK(launch_adam_sweep(m->st_comm, a, first, count, wgs));
  }
  SMX_HIP(hipEventRecord(m->ev_sweep, m->st_comm));
  m->sweep_pending = true;
  m->chain_started = true;
  // the optimiser launch skips these chunks; no launch of the backward chain carries any of them
  m->adam_early_from = m->chunk_first_head; m->adam_early_to = m->n_chunks;
  m->adam_rest_from = m->adam_rest_to = 0; m->adam_ride_b = 0;
  return SMX_OK;
}

// backward through an MLP.  d(out of last layer) arrives as `n_slabs` slabs in m->slab.
// Leaves d(input of first layer) as slabs in m->slab unless o.skip_input_grad.
struct MlpBwdOpts {
  bool skip_input_grad = false;             // the first layer's input is data: no d input
  int* out_slabs = nullptr;                 // receives the slabs of d(input of the first layer)
  const char* label = "";                   // Timed label of the first layer's weight gradient when it reads X
  const EpiLatentBwd* lat_epi = nullptr;    // d z feeds the latent head only: its backward runs in the epilogue of the d z product
  GemmArgs* defer_dw0 = nullptr;            // receives the first layer's weight gradient instead of launching it
  // front: the LAST layer's BatchNorm-backward launch computes its incoming gradient itself (fD fW^T as dot
  // products) instead of reading slabs.  defer: weight-gradient products that nothing later in the backward pass
  // reads are appended there instead of being launched (the caller runs them as ONE grouped launch at the end).
  const BnBwdArgs* front = nullptr;
  std::vector<GemmArgs>* defer = nullptr;
  // twin / twin_front: another MLP whose last layer's BatchNorm-backward (also with a gradient front) is independent of
  // this one's: both in ONE launch (*twin_done); the caller then walks the twin with last_bn_done = true.
  std::vector<MlpLayer>* twin = nullptr; const BnBwdArgs* twin_front = nullptr; bool* twin_done = nullptr;
  bool last_bn_done = false;
  // the LAST layer's wide BatchNorm-backward launch also carries the output head's dW / db (bn_wide_bwd_dw_kernel; dw_late below)
  const HeadBwdArgs* head_dw = nullptr;
};
// ---- the seam form: the decoder's carrier launch (dw_late) and the encoder's fold_dz launch behind it as ONE launch (smx_bn.hip: bn_bwd_seam_kernel) ----
// Both are latency-bound links of the step's chain, and the second one's 16 chain workgroups wait for nothing but the 64 KB of d pre_dec the first
// one's columns write: held in one launch they start their independent prologue at once and wait inside it (smx_handoff.h).  Taken when dw_late_now
// and fold_dz_now hold, the carrier's layer is the decoder's only one (its d pre IS the fold's zD), on one GPU without SyncBatchNorm, outside a
// timed step and outside graph capture (the wait's target is an argument).  Knob no_bwd_seam (read per step): the two launches.
// The head's optimiser riders read what the carrier's dW tiles write, so they cannot ride here: their chunks go with the optimiser launch (or the
// lazy set of the next step's first launch), as under the knob no_adam_early -- the same update, bit for bit.
static bool seam_wanted(const smx_model* m, const Pass& ps) {
  return m->dw_late_now && m->fold_dz_now && m->dec.size() == 1 && !dp_active(m) && !m->comm && !m->local && !m->p2p && m->world == 1 && !m->sync_bn && !sync_bn_on(m, ps.training) &&
         m->timing_label.empty() && !m->capturing && !m->lazy_rest_pending && m->enc.back().out_p / 8 <= HANDOFF_MAX_WAITERS && !tuning_on("no_bwd_seam");
}
// the carrier alone after all (the encoder's launch did not take it along)
static int seam_flush(smx_model* m) {
  if (!m->seam_pending) return SMX_OK;
  m->seam_pending = false;
  return launch_bn_wide_bwd_dw(m->st, m->seam_dec, m->seam_head);
}
static int seam_launch(smx_model* m, const BnBwdArgs& enc) {
  m->seam_pending = false;
  if (!m->seam_state) {
    SMX_HIP(hipMalloc((void**)&m->seam_state, HANDOFF_STATE_BYTES));
    m->seam_epochs = 0;
  }
  if (m->seam_epochs == 0) SMX_HIP(hipMemsetAsync(m->seam_state, 0, HANDOFF_STATE_BYTES, m->st));   // once per library call: the counter counts within it
  BwdSeamArgs sm;
  sm.seam.counter = m->seam_state; sm.seam.error = m->seam_state + HANDOFF_MAX_SHARDS * HANDOFF_SHARD_STRIDE;
  sm.seam.shards = HANDOFF_MAX_SHARDS;
  sm.seam.target = (unsigned)m->seam_dec.Hp * (m->seam_epochs + 1);
  sm.seam.timeout_ticks = (long long)(std::min(std::max((double)tuning("bwd_seam_timeout_s", 2.0), 0.01), 60.0) * 1e8);
  sm.preread = tuning_on("bwd_seam_preread") ? 1 : 0;
  sm.cons_first = tuning_on("bwd_seam_cons_first") ? 1 : 0;
  SMX_CHECK(launch_bn_bwd_seam(m->st, m->seam_dec, enc, m->seam_head, sm));
  ++m->seam_epochs; ++m->seam_steps;
  return SMX_OK;
}

static int mlp_backward(smx_model* m, std::vector<MlpLayer>& mlp, const Pass& ps, Mat in0, bool in_is_x, int n_slabs, const MlpBwdOpts& o) {
  auto make_b = [&](MlpLayer& L, int slabs, const BnBwdArgs* front) {
    BnBwdArgs b;
    b.dout = m->slab; b.n_slabs = slabs; b.slab_stride = (long)ps.B * L.out_p; b.ld = L.out_p;
    b.out = L.out_buf; b.xhat = L.xhat; b.inv_std = L.inv_std;
    b.B = ps.B; b.H = L.out; b.Hp = L.out_p; b.batchnorm = L.bn >= 0; b.training = ps.training; b.leak = L.leak;
    b.drop_scale = (ps.training && L.drop_p > 0.f) ? 1.f / (1.f - L.drop_p) : 1.f;
    b.dpre = L.dpre;
    if (L.bn >= 0) { b.gamma = P_(m, L.tGamma); b.dgamma = G_(m, L.tGamma); b.dbeta = G_(m, L.tBeta); }
    else b.dbias = G_(m, L.tBias);
    if (L.act != SMX_ACT_RELU) {   // the GEN_ACT forms: the keep mask from the forward's source (make_bn of forward_pass)
      b.act = L.act;
      if (L.bn >= 0) b.beta = P_(m, L.tBeta);
      b.drop_p = ps.training ? L.drop_p : 0.f;
      b.nk = make_key(m, L.stream, ps.sample, true);
      if (&mlp == &m->dec) b.nk.draw_rows = (uint32_t)ps.draw_rows;
      b.rows = ps.rows; b.cell_base = ps.cell_base;
      if (const Injected* ij = inj(m, L.stream)) { b.inj_mask = ij->d; b.inj_ld = ij->ld; }
    }
    if (front) {
      b.front = 1; b.fD = front->fD; b.fld = front->fld; b.fW = front->fW; b.fldw = front->fldw; b.fK = front->fK;
      b.fold_dz = front->fold_dz; b.zD = front->zD; b.zld = front->zld; b.zW = front->zW; b.zldw = front->zldw; b.zlb = front->zlb;
    }
    if (&mlp == &m->dec && &L == &mlp.back() && m->wide_dd_slabs > 0 && !front) {   // the one-launch head's slabs, column-major
      b.dout = m->wide_dd_src; b.n_slabs = m->wide_dd_slabs; b.slab_stride = m->wide_dd_stride; b.wide = 1;
    }
    return b;
  };
  if (o.twin_done) *o.twin_done = false;
  BnBwdArgs carried;            // gradient front handed from layer i + 1 to layer i (hidden layers up to 64 wide)
  bool have_carried = false;
  bool dw_carried = false;      // o.head_dw went with the last layer's launch
  bool dpre_done = false;       // layer i's d pre-activation was written by the d in product of layer i + 1 (activation epilogue)
  for (int i = (int)mlp.size() - 1; i >= 0; --i) {
    MlpLayer& L = mlp[i];
    const TensorInfo& tw = m->tensors[L.tW];
    const bool last = (i == (int)mlp.size() - 1);
    BnBwdArgs b = make_b(L, n_slabs, (o.front && last) ? o.front : (have_carried ? &carried : nullptr));
    have_carried = false;
    const bool dpre_ready = dpre_done;
    dpre_done = false;
    // (the seam form: the decoder's carrier launch is waiting for the encoder's fold_dz launch -- this one, or it goes out alone first)
    const bool seam = m->seam_pending && &mlp == &m->enc && last && b.front && b.fold_dz && !o.last_bn_done && !dpre_ready && !(sync_bn_on(m, ps.training) && L.bn >= 0) &&
                      !(m->metrics_before_allreduce && m->have_pending_metrics) && bn_bwd_seam_supported(m->seam_dec, b, m->seam_head);
    if (m->seam_pending && &mlp != &m->dec && !seam) SMX_CHECK(seam_flush(m));
    if ((last && o.last_bn_done) || dpre_ready) {
      // (this layer's BatchNorm-backward ran beside the other MLP's / its d pre-activation came with the product above)
    } else if (sync_bn_on(m, ps.training) && L.bn >= 0) {   // the ELBO scalars then go with a launch of their own (optimizer_pass)
      Timed t(m, "bn_bwd");
      m->adam_early_pending = false;
      const BnSyncArgs y = sync_args(m);
      SMX_CHECK(launch_bn_sync_bwd(m->st, b, y, 0));
      SMX_CHECK(dp_allreduce_buf(m, m->sync_buf, (size_t)y.world * 2 * L.out_p, m->st));
      SMX_CHECK(launch_bn_sync_bwd(m->st, b, y, 1));
    } else {
      if (m->metrics_before_allreduce && m->have_pending_metrics) {
        b.metrics = m->pending_metrics; b.with_metrics = 1; m->have_pending_metrics = false;
      }
      // (the carrier WRITES dW_out and its slots: the head's riders wait -- adam_early_pending stays set -- for the next BatchNorm-backward launch)
      const HeadBwdArgs* hd = (last && o.head_dw && bn_wide_bwd_dw_supported(b, *o.head_dw)) ? o.head_dw : nullptr;
      // (the seam form: the head's riders would read what the launch's dW tiles write -- their chunks stay with the optimiser launch / the lazy set)
      if (seam) m->adam_early_pending = false;
      else if (!hd) attach_early_adam(m, b);
      // (the carrier has rider slots and no riders of this step -- they wait for the encoder's launch --: W_enc's chunks of the step BEFORE, which
      // the forward pass left pending for this launch (fwd_encoder: lazy_w_late), ride here with that step's arguments.  Nothing since this step's
      // first launch reads W_enc, and its gradient and slots are rewritten by the weight-gradient launch, behind this one)
      const bool w_rides = hd && b.adam_count == 0 && b.sqr_count == 0 && m->lazy_w_pending && !m->lazy_rest_pending;
      if (w_rides) { b.adam = m->lazy_args; b.adam_first = m->lazy_w_first; b.adam_count = m->lazy_w_n; }
      // a step that leaves its optimiser launch to the next step's forward launches (smx_step.hip: lazy_adam_wanted): what that launch's extra
      // workgroups did -- the ELBO scalars, closing the step -- rides with the encoder's first BatchNorm-backward launch instead
      // (lazy_l1: only a step whose first launch took the form the update needs -- every other step's launches stay exactly as they were)
      if (m->lazy_want && m->lazy_l1 && !m->lazy_closed && &mlp == &m->enc && m->have_pending_metrics) {
        b.metrics = m->pending_metrics; b.with_metrics = 1; m->have_pending_metrics = false;
        if (!b.adam.params) fill_adam_args(m, b.adam);
        fill_step_close(m, b.adam);
        b.close = 1; m->lazy_closed = true;
      }
      Timed t(m, "bn_bwd");
      const bool dual = last && b.front && b.fK <= 64 && o.twin && o.twin_front && o.twin_front->fK <= 64 && !o.twin->empty() && m->flags.twin && bn_dual_supported(ps.B) &&
                        bn_bwd_front_supported(ps.B, o.twin_front->fK) && o.twin->back().out_p % 8 == 0 &&
                        !(sync_bn_on(m, ps.training) && o.twin->back().bn >= 0);
      if (hd && &mlp == &m->dec && (w_rides || !m->lazy_w_pending) && seam_wanted(m, ps)) {
        // held back: the encoder's fold_dz launch takes the carrier along (seam_launch) -- nothing is launched in between
        m->seam_dec = b; m->seam_head = *hd; m->seam_pending = true;
        dw_carried = true;
        if (w_rides) m->lazy_w_pending = false;
      } else if (hd) {
        SMX_CHECK(launch_bn_wide_bwd_dw(m->st, b, *hd));
        dw_carried = true;
        if (w_rides) m->lazy_w_pending = false;
      } else if (seam) {
        SMX_CHECK(seam_launch(m, b));
      } else if (dual) {
        const BnBwdArgs b2 = make_b(o.twin->back(), 0, o.twin_front);
        SMX_CHECK(launch_bn_act_bwd_dual(m->st, b, b2));
        if (o.twin_done) *o.twin_done = true;
      } else {
        SMX_CHECK(launch_bn_act_bwd(m->st, b));
      }
    }
    // dW = in^T * dpre
    const bool first_x = (i == 0 && in_is_x);
    const Mat in = (i == 0) ? in0 : Mat{mlp[i - 1].out_buf, mlp[i - 1].out_p};
    // (dpre_ready: no bias / activation backward launch ran -- the bias gradient is the column sum of d pre)
    GemmArgs g = dense_wgrad(m, in, {L.dpre, L.out_p}, L.tW, dpre_ready ? G_(m, L.tBias) : nullptr, L.in_p, L.out_p, ps.B);
    if (first_x) x_gather(m, ps, g);
    if (i == 0 && o.skip_input_grad) {
      if (o.defer_dw0) *o.defer_dw0 = g;   // the caller launches it (possibly grouped with another first-layer gradient)
      else {
        Timed t(m, first_x ? o.label : "gemm_mlp_dw");
        SMX_CHECK(launch_gemm(m->st, g));
      }
      n_slabs = 0;
      break;
    }
    // hidden layers 32 / 64 / 128 wide: the layer below takes d in = dpre W^T as the gradient front of its BatchNorm-backward
    // launch (dot products over K = this layer's width) and d W joins the grouped launch at the end -- no product launch
    if (o.defer && i > 0 && !(i == 0 && o.lat_epi) && m->flags.bwd_front && (L.out_p == 32 || L.out_p == 64 || L.out_p == 128) && mlp[i - 1].act == SMX_ACT_RELU &&
        bn_bwd_front_supported(ps.B, L.out_p) && mlp[i - 1].out_p % 8 == 0 && (tw.ld % 4) == 0 && (L.out_p % 4) == 0 &&
        !(sync_bn_on(m, ps.training) && mlp[i - 1].bn >= 0)) {
      o.defer->push_back(g);
      carried = BnBwdArgs();
      carried.fD = L.dpre; carried.fld = L.out_p; carried.fW = P_(m, L.tW); carried.fldw = tw.ld; carried.fK = L.out_p;
      have_carried = true;
      n_slabs = 0;
      continue;
    }
    // d in = dpre * W^T  -> slabs; independent of dW: one grouped launch for both
    GemmArgs h = dense_dgrad({L.dpre, L.out_p}, {P_(m, L.tW), tw.ld}, m->slab, ps.B, L.in_p, L.out_p);
    h.split_k = suggest_split_k(ps.B, L.in_p, L.out_p);
    SMX_REQUIRE((size_t)h.split_k * (size_t)h.slab_stride <= m->slab_cap, "split-K slabs exceed the slab buffer");
    if (i == 0 && o.lat_epi) {  // d z feeds the latent head only: run its backward in the epilogue
      h.epi = 2; h.lb = *o.lat_epi; h.split_k = 1; h.tile = TILE_32x32_K4;
    }
    // the layer below has neither BatchNorm nor dropout: its activation's derivative goes into this product's store path
    // and the result IS its d pre-activation (its bias gradient: the column sums its weight-gradient product takes along)
    if (i > 0 && m->flags.act_epilogue && mlp[i - 1].bn < 0 && !(ps.training && mlp[i - 1].drop_p > 0.f) && h.split_k <= 1 &&
        mlp[i - 1].act == SMX_ACT_RELU) {
      MlpLayer& Lo = mlp[i - 1];
      h.split_k = 1; h.act = 2; h.leak = Lo.leak; h.act_out = Lo.out_buf; h.act_ld = Lo.out_p;
      h.C = Lo.dpre; h.ldc = Lo.out_p; h.slab_stride = 0;
      dpre_done = true;
    }
    int effs[2] = {1, 1};
    if (o.defer && i == 0 && o.lat_epi && m->fold_dz_now) {
      // fold_dz: no launch here -- the encoder's last BatchNorm-backward launch computes d z and the latent head's backward itself
      // (BnBwdArgs::fold_dz, smx_bn.hip: fold_dz_tile); d W joins the final grouped launch as before
      o.defer->push_back(g);
    } else if (o.defer && i == 0 && o.lat_epi) {   // d z (+ latent-head backward) alone; d W joins the final grouped launch
      o.defer->push_back(g);
      AdamArgs riders;
      if (m->adam_ride_b > 0) take_adam_riders(m, h, riders);
      Timed t(m, "gemm_mlp_bwd");
      SMX_CHECK(launch_gemm_group(m->st, &h, 1, effs + 1));
    } else {
      GemmArgs pair[2] = {g, h};
      Timed t(m, "gemm_mlp_bwd");
      SMX_CHECK(launch_gemm_group(m->st, pair, 2, effs));
    }
    const int eff = effs[1];
    n_slabs = eff;
  }
  if (o.out_slabs) *o.out_slabs = n_slabs;
  SMX_REQUIRE(!o.head_dw || dw_carried, "the output head's dW found no launch to carry it");
  return SMX_OK;
}

// a weight gradient of the discriminator over `rows` rows (b3: flag bf16x3 -- through the direct-operand 32 x 32-tile kernel of smx_headbwd.hip);
// beside: the layer's input gradient in the same launch (wgrad_dgemm_kernel)
static int disc_wgrad(smx_model* m, const GemmArgs& g, int rows, bool b3, const GemmArgs* beside = nullptr) {
  if (!(b3 && m->flags.wgrad && wgrad_supported(g, rows))) return launch_gemm(m->st, g);
  // a square 1000 x 1000 gradient: as up to 8 column groups of 128 in the panel form (smx_panel.h role 0: a workgroup takes 32
  // rows with the group's four column tiles -- the A tile is split once per group instead of once per 32 columns)
  if (g.M >= 512 && g.N % 128 == 0 && g.N / 128 <= SMX_GROUP_MAX && g.N > 128 && !tuning_on("no_panel")) {
    GemmArgs part[SMX_GROUP_MAX];
    int counts[SMX_GROUP_MAX];
    const int ng = g.N / 128, per = ((g.M + 31) / 32) * 8;
    for (int k = 0; k < ng; ++k) {
      part[k] = g;
      part[k].B = g.B + 128 * k; part[k].C = g.C + 128 * k; part[k].N = 128; part[k].panel_hint = 1;
      if (g.colsum) part[k].colsum = g.colsum + 128 * k;
      if (g.sq_part) { part[k].sq_part = g.sq_part + (long)per * k; part[k].sq_count = &counts[k]; }
    }
    const int rc = launch_wgrad_group(m->st, part, ng, rows, 1, beside);
    if (rc == SMX_OK && g.sq_part && g.sq_count) *g.sq_count = per * ng;
    return rc;
  }
  return launch_wgrad_group(m->st, &g, 1, rows, 1, beside);
}

// One backward sweep of the discriminator over the first `rows` rows of the stacked batch with upstream `up`
// [rows][32] on the logits.  with_grads: the discriminator's own gradients (its objective; nothing flows into z);
// otherwise only d objective / d z, left in m->dz_tc (the VAE objective's TC term; the weights are constants of it).
int factor_sweep(smx_model* m, const Pass& ps, int rows, const float* up, bool with_grads) {
  const MlpLayer& last = m->disc.back();
  // flag bf16x3: the weight gradients (K = the stacked minibatch) through the direct-operand 32 x 32-tile kernel of
  // smx_headbwd.hip, the 1000-deep input gradients through smx_dgemm.hip -- both from bf16 MFMAs on split operands
  const bool b3 = b3_on(m, ps.B) && !tuning_on("no_dgemm");
  const TensorInfo& two = m->tensors[m->t_discoutW];
  if (with_grads) {
    const GemmArgs gw = dense_wgrad(m, {last.out_buf, last.out_p}, {up, 32}, m->t_discoutW, G_(m, m->t_discoutb), last.out_p, two.ld, rows);
    Timed t(m, "disc_bwd");
    SMX_CHECK(disc_wgrad(m, gw, rows, b3));
  }
  int n_slabs = 1;
  {
    const GemmArgs gh = dense_dgrad({up, 32}, {P_(m, m->t_discoutW), two.ld}, m->slab, rows, last.out_p, two.ld);
    Timed t(m, "disc_bwd");
    SMX_CHECK(launch_gemm(m->st, gh, &n_slabs));
  }
  // The discriminator's layers have neither BatchNorm nor dropout: below the top layer the activation's derivative runs
  // in the store path of the d-input product above (which then writes the layer's d pre-activation directly) and the bias
  // gradient is the column sum its weight-gradient product takes along -- no bias / activation backward launch per
  // layer (flag act_epilogue).  Without gradients (the TC sweep) the d pre-activations ping-pong between two scratch
  // buffers, as a product must not write the operand it reads.
  float* pong[2] = {m->disc_dpre, m->slab};
  int pp = 0;
  bool ready = false;
  float* dpre_i = nullptr;
  for (int i = (int)m->disc.size() - 1; i >= 0; --i) {
    MlpLayer& L = m->disc[i];
    const TensorInfo& tw = m->tensors[L.tW];
    if (!ready) {
      dpre_i = with_grads ? L.dpre : pong[pp];
      BnBwdArgs b;
      b.dout = m->slab; b.n_slabs = n_slabs; b.slab_stride = (long)rows * L.out_p; b.ld = L.out_p;
      b.out = L.out_buf; b.B = rows; b.H = L.out; b.Hp = L.out_p; b.batchnorm = 0; b.training = 1; b.drop_scale = 1.f; b.leak = L.leak;
      b.dpre = dpre_i;
      b.dbias = with_grads ? G_(m, L.tBias) : m->disc_db;
      Timed t(m, "disc_bwd");
      SMX_CHECK(launch_bn_act_bwd(m->st, b));
    }
    const float* in = (i == 0) ? m->zz : m->disc[i - 1].out_buf;
    const int ld_in = (i == 0) ? m->Dp : m->disc[i - 1].out_p;
    if (with_grads) {
      const GemmArgs g = dense_wgrad(m, {in, ld_in}, {dpre_i, L.out_p}, L.tW, ready ? G_(m, L.tBias) : nullptr, L.in_p, L.out_p, rows);
      Timed t(m, "disc_bwd");
      SMX_CHECK(disc_wgrad(m, g, rows, b3));
      if (i == 0) break;   // z is a constant of the discriminator's objective
    }
    GemmArgs h = dense_dgrad({dpre_i, L.out_p}, {P_(m, L.tW), tw.ld}, m->slab, rows, L.in_p, L.out_p);
    ready = false;
    if (i == 0) { h.C = m->dz_tc; h.ldc = m->Dp; h.slab_stride = 0; h.tile = TILE_32x32_K4; }   // (into z: one plain store, no slabs)
    else {
      h.split_k = suggest_split_k(rows, L.in_p, L.out_p);
      if (b3) { GemmArgs probe = h; probe.split_k = 1; if (dgemm_supported(probe)) h.split_k = 1; }   // (the direct form splits K over its waves)
      SMX_REQUIRE((size_t)h.split_k * (size_t)h.slab_stride <= m->slab_cap, "split-K slabs exceed the slab buffer");
      if (m->flags.act_epilogue && h.split_k <= 1 && (with_grads || pong[pp ^ 1] != dpre_i)) {
        MlpLayer& Lo = m->disc[i - 1];
        float* next = with_grads ? Lo.dpre : pong[pp ^= 1];
        h.split_k = 1; h.act = 2; h.leak = Lo.leak; h.act_out = Lo.out_buf; h.act_ld = Lo.out_p;
        h.C = next; h.ldc = Lo.out_p; h.slab_stride = 0;
        ready = true;
      }
    }
    {
      Timed t(m, "disc_bwd");
      if (b3 && dgemm_supported(h)) { SMX_CHECK(launch_dgemm(m->st, h)); n_slabs = 1; }
      else SMX_CHECK(launch_gemm(m->st, h, &n_slabs));
    }
    if (ready) dpre_i = h.C;
  }
  return SMX_OK;
}

// Both backward sweeps of the discriminator as rows of ONE chain of products: rows [0, 2B) carry the discriminator's own objective
// (its weight gradients contract over exactly these rows), rows [2B, 3B) the VAE objective's TC term on the rows of z (they only
// pass through the weights: d objective / d z in the end).  The input gradients of a layer are then one launch of 3B rows
// instead of one of 2B and one of B (each a latency chain of ~8 us whatever its row count), the activation's derivative for
// the extra rows reads the forward output of row - 2B (GemmArgs::act_wrap), every bias gradient is the column sum of its
// weight-gradient product.  Needs the store-path activation (flag act_epilogue); without it: the two sweeps of factor_sweep.
static int factor_backward_stacked(smx_model* m, const Pass& ps) {
  const int B = ps.B, R2 = 2 * B, R3 = 3 * B;
  const MlpLayer& last = m->disc.back();
  const TensorInfo& two = m->tensors[m->t_discoutW];
  const bool b3 = b3_on(m, ps.B) && !tuning_on("no_dgemm");
  const float* up = m->u_d;   // [3B][32]
  static const bool beside_on = !tuning_on("fvae_no_beside");
  // beside: the layer's input gradient in the same launch (wgrad_dgemm_kernel) where both forms apply, right after it otherwise
  auto input_grad = [&](const GemmArgs& h) -> int {
    if (b3 && dgemm_supported(h)) return launch_dgemm(m->st, h);
    return launch_gemm(m->st, h);
  };
  Timed t(m, "disc_bwd");
  {   // the logit layer: weight gradient over the discriminator's rows, then the input gradient of all 3B rows -> d pre of the last hidden layer
    SMX_CHECK(disc_wgrad(m, dense_wgrad(m, {last.out_buf, last.out_p}, {up, 32}, m->t_discoutW, G_(m, m->t_discoutb), last.out_p, two.ld, R2), R2, b3));
    MlpLayer& Ll = m->disc.back();
    GemmArgs gh = dense_dgrad({up, 32}, {P_(m, m->t_discoutW), two.ld}, Ll.dpre, R3, last.out_p, two.ld);
    gh.slab_stride = 0;   // (written as the layer's d pre-activation, no slabs)
    gh.act = 2; gh.leak = Ll.leak; gh.act_out = Ll.out_buf; gh.act_ld = Ll.out_p; gh.act_wrap = R2;
    SMX_CHECK(launch_gemm(m->st, gh));
  }
  for (int i = (int)m->disc.size() - 1; i >= 0; --i) {
    MlpLayer& L = m->disc[i];
    const TensorInfo& tw = m->tensors[L.tW];
    const float* in = (i == 0) ? m->zz : m->disc[i - 1].out_buf;
    const int ld_in = (i == 0) ? m->Dp : m->disc[i - 1].out_p;
    // weight gradient (+ bias gradient as its column sum) over the discriminator's 2B rows
    const GemmArgs g = dense_wgrad(m, {in, ld_in}, {L.dpre, L.out_p}, L.tW, G_(m, L.tBias), L.in_p, L.out_p, R2);
    GemmArgs h;   // input gradient (a plain store, no slabs)
    if (i == 0) {   // into z: only the TC rows (z is a constant of the discriminator's objective)
      h = dense_dgrad({L.dpre + (size_t)R2 * L.out_p, L.out_p}, {P_(m, L.tW), tw.ld}, m->dz_tc, B, L.in_p, L.out_p);
      h.ldc = m->Dp; h.tile = TILE_32x32_K4;
    } else {
      MlpLayer& Lo = m->disc[i - 1];
      h = dense_dgrad({L.dpre, L.out_p}, {P_(m, L.tW), tw.ld}, Lo.dpre, R3, L.in_p, L.out_p);
      h.ldc = Lo.out_p; h.act = 2; h.leak = Lo.leak; h.act_out = Lo.out_buf; h.act_ld = Lo.out_p; h.act_wrap = R2;
    }
    h.slab_stride = 0;
    if (beside_on && b3 && m->flags.wgrad && wgrad_supported(g, R2) && dgemm_supported(h) && h.b_nmajor) SMX_CHECK(disc_wgrad(m, g, R2, b3, &h));
    else { SMX_CHECK(disc_wgrad(m, g, R2, b3)); SMX_CHECK(input_grad(h)); }
  }
  return SMX_OK;
}

int factor_backward(smx_model* m, const Pass& ps) {
  if (m->flags.act_epilogue && !tuning_on("fvae_two_sweeps")) return factor_backward_stacked(m, ps);
  SMX_CHECK(factor_sweep(m, ps, 2 * ps.B, m->u_d, true));                          // discriminator objective -> the discriminator's tensors
  SMX_CHECK(factor_sweep(m, ps, ps.B, m->u_d + (size_t)2 * ps.B * 32, false));     // gamma TC (+ alpha CE) -> d z
  return SMX_OK;
}

// ---- backward_pass: its stages in launch order; BwdPass is what crosses their boundaries ----
struct BwdPass {
  KlWeight klw{nullptr, 0.f, 0.f, 0};   // beta / B_global of this step
  int lat_ld = 0;
  long dd_stride = 0;                   // one slab of d d (the gradient of the decoder's output)
  const float* dparams = nullptr;       // gradient of the planes the output products wrote (scvi: of the raw planes)
  bool hbwd = false;                    // the output head's two products ran as the one wide launch (smx_headbwd.hip)
  int n_slabs = 0;                      // slabs of d d in m->slab
  std::vector<GemmArgs> lab_dw;         // the label heads' weight gradients, when their d d rode with the output head's launch
  std::vector<GemmArgs> tail;           // products that only the optimiser reads: ONE grouped launch at the end
  EpiLatentBwd le;
  bool bfront = false, lfront = false;  // the encoder's / library encoder's last BatchNorm-backward launch takes its gradient as a front (gf / gfl)
  BnBwdArgs gf, gfl;
  int dh_slabs = 1;                     // slabs of d h the encoder's backward sums
  bool twin_done = false;               // the library encoder's last BatchNorm-backward ran beside the encoder's
  GemmArgs dw0[2]; int n_dw0 = 0;       // the first-layer weight gradients of the encoder and the library encoder
  HeadBwdArgs hb_late;                  // m->dw_late_now: the head's arguments for the decoder's BatchNorm-backward launch, which carries its dW / db
};

// label heads (SISUA / MISA): d d += d Y W_lab^T as extra slabs of the output head's launch, the head's weight gradient with the
// grouped launch at the end of the backward pass -- instead of a grouped launch of their own here (8.6 us at C4)
static void ride_label_heads(smx_model* m, BwdPass& p, HeadBwdArgs& hb) {
  if (!(m->n_heads > 0 && m->flags.label_ride && !m->fvae && !m->scvi && !(m->head_fused && m->head_loss))) return;
  bool ok = true;
  for (int j = 0; j < m->n_heads; ++j) ok = ok && (m->tensors[m->t_labW[j]].ld % 32) == 0;
  ok = ok && (size_t)(hb.n_slices + m->n_heads) * (size_t)p.dd_stride <= m->slab_cap;
  if (!ok) return;
  for (int j = 0; j < m->n_heads; ++j) {
    const TensorInfo& tl = m->tensors[m->t_labW[j]];
    hb.xA[j] = m->laby_draw[j]; hb.xlda[j] = tl.ld; hb.xW[j] = P_(m, m->t_labW[j]); hb.xldw[j] = tl.ld; hb.xK[j] = tl.ld;
  }
  hb.n_extra = m->n_heads;
  p.n_slabs += m->n_heads;
  m->lab_deferred = true;
}

// a wide head (the bf16 x 3 regime): d d = dP W^T (K = every gene of every plane) as one workgroup per K slice + a reduce
// launch (smx_bigk.hip) -- ONE slab for the BatchNorm-backward launch; d W / d b stay with the 32 x 32-tile kernel
static int dd_bigk(smx_model* m, const Pass& ps, BwdPass& p, bool* done) {
  const MlpLayer& dL = m->dec.back();
  const long ldp = (long)m->k * m->Gp;
  BigKArgs bk;
  bk.A = p.dparams; bk.lda = ldp; bk.Bm = P_(m, m->t_outW[0]); bk.ldb = m->tensors[m->t_outW[0]].ld; bk.b_kmajor = 0;
  bk.M = ps.B; bk.N = dL.out_p; bk.K = (int)ldp; bk.ldc = dL.out_p; bk.slab_stride = p.dd_stride;
  bk.part = m->bigk_part; bk.out = m->slab;
  bk.n_slices = bigk_slices(bk.K, SMX_BIGK_MAX_SLICES, &bk.k_chunk);
  if (!(bigk_supported(bk) && (size_t)bk.n_slices * (size_t)bk.slab_stride <= m->bigk_floats)) return SMX_OK;
  if (m->n_heads == 0 && !(sync_bn_on(m, ps.training) && dL.bn >= 0) && bn_wide_supported(ps.B, dL.out_p, bk.n_slices) && (size_t)bk.n_slices * 128 * 128 <= m->bigk_floats) {
    bk.colmajor = 1; bk.slab_stride = 128L * 128;   // (no reduce launch: as behind the one-launch head)
    m->wide_dd_slabs = bk.n_slices; m->wide_dd_src = m->bigk_part; m->wide_dd_stride = bk.slab_stride;
  }
  SMX_CHECK(launch_bigk(m->st, bk));
  *done = true;
  p.n_slabs = 1;
  return SMX_OK;
}

// dW_out / db / the sum-of-squares slots leave the chain: the head's launch computes d d only and the decoder's BatchNorm-backward launch -- the
// next on the chain, which waits for d d alone and leaves most of the chip idle -- carries the dW tiles (bn_wide_bwd_dw_kernel, the same role-0 body:
// the same bits).  Where: the column-major d d slabs of a narrow panel (dd_wide), the plain bf16 x 3 form, a ReLU layer below the head; nobody that takes
// the head's gradients as final in bwd_heads_final (the data-parallel chain and exchange, the background sweep); no SyncBatchNorm.  Knob no_dw_late
// (read per step): the head's launch with both roles, as before.
static bool dw_late(smx_model* m, const Pass& ps, const HeadBwdArgs& hb, bool dd_wide, bool fused_done, bool bigk) {
  const MlpLayer& dL = m->dec.back();
  return dd_wide && !fused_done && !bigk && hb.bf16x3 && !hb.sep && hb.n_extra == 0 && dL.act == SMX_ACT_RELU && !dp_active(m) && head_sweep_wgs(m) <= 0 &&
         !sync_bn_on(m, ps.training) && !tuning_on("no_dw_late");
}

// ---- output head: count heads with raw planes -- both products of the output head in one launch of the wide direct-operand kernel
// (smx_headbwd.hip); SMX_NO_HEAD_BWD=1 or a 'share'd scvi plane: the grouped LDS-tiled products of bwd_head_group
// (scvi: the planes are separate head tensors -- the kernel's SEP form)
static int bwd_out_head(smx_model* m, const Pass& ps, BwdPass& p) {
  const MlpLayer& dL = m->dec.back();
  const long ldp = (long)m->k * m->Gp;
  HeadBwdArgs hb;
  hb.D = dL.out_buf; hb.ldd = dL.out_p; hb.dP = p.dparams; hb.ldp = ldp; hb.W = P_(m, m->t_outW[0]); hb.ldw = m->tensors[m->t_outW[0]].ld;
  hb.dW = G_(m, m->t_outW[0]); hb.db = G_(m, m->t_outb[0]);
  if (m->scvi) {
    hb.sep = 1;
    for (int ch = 0; ch < m->k; ++ch) {
      hb.Wp[ch] = P_(m, m->t_outW[ch]); hb.dWp[ch] = G_(m, m->t_outW[ch]); hb.dbp[ch] = G_(m, m->t_outb[ch]);
      if ((hb.sqp[ch] = sq_part_of(m, m->t_outW[ch]))) hb.sq_countp[ch] = &m->sq_count[(size_t)m->t_outW[ch]];
    }
  }
  hb.B = ps.B; hb.Hp = dL.out_p; hb.Gp = m->Gp; hb.n_planes = m->k;
  hb.bf16x3 = b3_on(m, ps.B) ? 1 : 0;
  hb.n_slices = head_bwd_slices(ldp, ldp <= 8192 ? 16 : 32, &hb.k_chunk);
  hb.slab = m->slab; hb.slab_stride = p.dd_stride;
  SMX_REQUIRE((size_t)hb.n_slices * (size_t)p.dd_stride <= m->slab_cap, "split-K slabs exceed the slab buffer");
  if (!m->scvi && (hb.sq_part = sq_part_of(m, m->t_outW[0]))) hb.sq_count = &m->sq_count[(size_t)m->t_outW[0]];
  p.n_slabs = hb.n_slices;
  ride_label_heads(m, p, hb);
  // at most 128 cells, no label slabs: d d's slabs column-major, summed by the decoder's BatchNorm-backward launch as one workgroup per
  // column (bn_wide_bwd_kernel; <= 16 slabs: the additions in the order of the 8-column launch, the same bits)
  const bool dd_wide = !(m->head_fused && m->head_loss) && m->n_heads == 0 && hb.n_extra == 0 && !hb.sep && hb.n_slices <= 16 && !(sync_bn_on(m, ps.training) && dL.bn >= 0) &&
                       bn_wide_supported(ps.B, dL.out_p, hb.n_slices) && (size_t)hb.n_slices * 128 * (size_t)dL.out_p <= m->slab_cap;
  Timed t(m, "gemm_out_bwd");
  const bool fused_done = m->head_fused && m->head_loss && !hb.sep && hb.n_extra == 0;   // (forward_pass ran smx_headfused.hip: dW, db, the sum of squares and d d are there)
  if (fused_done) {
    m->head_fused_bwd_done = true;
    p.n_slabs = 1;
    if (hb.sq_count) *hb.sq_count = m->head_fused_sq;
  }
  bool bigk = false;
  if (!fused_done && hb.bf16x3 && !hb.sep && hb.n_extra == 0 && m->bigk_part && dL.out_p <= 128 && !tuning_on("no_bigk")) SMX_CHECK(dd_bigk(m, ps, p, &bigk));
  hb.skip_dd = bigk ? 1 : 0;
  if (dd_wide && !fused_done && !bigk) {
    hb.dd_colmajor = 1; hb.slab_stride = 128L * dL.out_p;
    m->wide_dd_slabs = hb.n_slices; m->wide_dd_src = m->slab; m->wide_dd_stride = hb.slab_stride;
  }
  if (dw_late(m, ps, hb, dd_wide, fused_done, bigk)) {
    p.hb_late = hb; p.hb_late.skip_dd = 1; p.hb_late.dd_colmajor = 0;
    m->dw_late_now = true;
    hb.skip_dw = 1;
  }
  // ... and then d W / d b with one workgroup per (gene tile, plane) that holds every row of H (smx_panel.h): the panel is
  // transformed and split once, not once per 32 rows of H
  if (fused_done) {}
  else if (bigk && panel_dw_supported(hb)) SMX_CHECK(launch_panel_dw(m->st, hb));
  else if (!(hb.skip_dw && hb.skip_dd)) SMX_CHECK(launch_out_head_bwd(m->st, hb));
  return SMX_OK;
}

// ---- the heads' products the launch above did not take: weight gradient and input gradient of every head read the same dP and are
// independent -- one grouped launch (dW tiles + split-K dX slabs side by side)
static int bwd_head_group(smx_model* m, const Pass& ps, BwdPass& p) {
  const Mat D{m->dec.back().out_buf, m->dec.back().out_p};
  const long ldp = (long)m->k * m->Gp;
  std::vector<GemmArgs> grp;
  std::vector<int> is_dx;
  for (int ch = 0; ch < (m->scvi ? m->k : 1) && !p.hbwd; ++ch) {
    if (m->scvi && !m->out_has_W[ch]) {   // no Dense head: the per-gene vector's gradient is the column sum of the plane's d raw
      SMX_CHECK(launch_plane_colsum(m->st, p.dparams + (long)ch * m->Gp, ldp, G_(m, m->t_outb[ch]), ps.B, m->Gp, m->out_single[ch] ? m->G : 0));
      continue;
    }
    const Mat dP{p.dparams + (m->scvi ? (long)ch * m->Gp : 0), ldp}, W{P_(m, m->t_outW[ch]), m->tensors[m->t_outW[ch]].ld};
    const int ncols = m->scvi ? m->Gp : (int)ldp;
    GemmArgs g = dense_wgrad(m, D, dP, m->t_outW[ch], G_(m, m->t_outb[ch]), D.ld, ncols, ps.B);   // dW = d^T dP, db = colsum(dP)
    g.tile = TILE_128x32;
    grp.push_back(g); is_dx.push_back(0);
    GemmArgs h = dense_dgrad(dP, W, nullptr, ps.B, D.ld, ncols);   // dd += dP W^T
    h.split_k = suggest_split_k(ps.B, D.ld, ncols);
    h.tile = TILE_32x32_K4;
    grp.push_back(h); is_dx.push_back(1);
  }
  for (int j = 0; j < m->n_heads; ++j) {
    const int ld = (int)m->tensors[m->t_labW[j]].ld;
    const GemmArgs g = dense_wgrad(m, D, {m->laby_draw[j], ld}, m->t_labW[j], G_(m, m->t_labb[j]), D.ld, ld, ps.B);
    if (m->lab_deferred) { p.lab_dw.push_back(g); continue; }   // (d d rode with the output head's backward launch)
    grp.push_back(g); is_dx.push_back(0);
    grp.push_back(dense_dgrad({m->laby_draw[j], ld}, {P_(m, m->t_labW[j]), ld}, nullptr, ps.B, D.ld, ld)); is_dx.push_back(1);
  }
  // slab slots: split factors are known up front (launch_gemm_group recomputes the same values)
  for (size_t i = 0; i < grp.size(); ++i) {
    if (!is_dx[i]) continue;
    GemmArgs& h = grp[i];
    const int BK = 128;  // K4 tile for split products; single-slab products may take either tile
    int eff = 1;
    if (h.split_k > 1) {
      const int chunk = round_up((h.K + h.split_k - 1) / h.split_k, BK);
      eff = (h.K + chunk - 1) / chunk;
    }
    h.C = m->slab + (long)p.n_slabs * p.dd_stride;
    p.n_slabs += eff;
    SMX_REQUIRE((size_t)p.n_slabs * (size_t)p.dd_stride <= m->slab_cap, "split-K slabs exceed the slab buffer");
  }
  if (grp.empty()) return SMX_OK;
  Timed t(m, p.hbwd ? "gemm_lab_bwd" : "gemm_out_bwd");
  for (size_t i = 0; i < grp.size(); i += SMX_GROUP_MAX) {
    const int n = (int)std::min<size_t>(SMX_GROUP_MAX, grp.size() - i);
    SMX_CHECK(launch_gemm_group(m->st, grp.data() + i, n));
  }
  return SMX_OK;
}

// ---- dW / db of every head are final: their optimiser update starts -- riders of the launches below, the background sweep, or the data-parallel chain
static int bwd_heads_final(smx_model* m) {
  m->adam_early_pending = true;
  if (m->head_fused_bwd_done && m->ev_hf_fresh) SMX_CHECK(head_sweep_start(m));
  else if (!m->head_fused_bwd_done && !m->scvi && m->sq_count[(size_t)m->t_outW[0]] > 0 && !tuning_on("no_sweep_unfused") && head_sweep_ok(m)) {
    // (round 6) ... and behind the SEPARATE head products of a wide panel too (decoder layers other than 128 units: 128 x 20 000 with 256 units
    // 350 -> 330 us per step): the same sweep, started behind an event of this stream recorded here.  (scVI's three head tensors: 276.4 against
    // 277.4 us with it -- its riders stay.)  The tensor's norm is then summed from the products' slots directly instead of from the reduce
    // riders' partial sums: where the clip bites, the last bits of the update differ between the two forms.
    SMX_CHECK(head_sweep_prepare(m));
    SMX_HIP(hipEventRecord(m->ev_hf, m->st));
    SMX_CHECK(head_sweep_start(m));
  }
  m->ev_hf_fresh = false;
  m->head_fused_bwd_done = false;
  if (dp_chain_ok(m)) {   // head gradients are final (label heads whose weight gradient rides with the last launch of the pass: optimizer_pass)
    if (!m->lab_deferred) SMX_CHECK(dp_chain_start(m));
  } else if (dp_overlap(m)) {  // (the hand-written exchange) head gradients are final: reduce them while the rest of backward runs
    SMX_HIP(hipEventRecord(m->ev_c1, m->st));
    SMX_HIP(hipStreamWaitEvent(m->st_comm, m->ev_c1, 0));
    SMX_CHECK(dp_allreduce(m, m->bucket1_off, m->bucket1_count, m->st_comm));
    m->bucket1_in_flight = true;
  }
  return SMX_OK;
}

// ---- decoder MLP; the latent head's backward runs in the epilogue of the d z product (mixture / full-covariance posterior: a launch of its own) ----
static int bwd_decoder(smx_model* m, const Pass& ps, BwdPass& p) {
  const smx_config& c = m->cfg;
  EpiLatentBwd& le = p.le;
  le.lat = m->latbuf; le.ld = p.lat_ld; le.sig = m->sig; le.eps = m->eps; le.klw = p.klw;
  le.D = m->D; le.Dp = m->Dp; le.stochastic = m->stochastic; le.relu = (c.latent_activation == SMX_ACT_RELU);
  le.dlat = m->dlat;
  if (m->fvae) le.dz_add = m->dz_tc;
  if (m->scale) {
    le.dklz = m->dklz;
    ScalePriorArgs sp;
    sp.z = m->z; sp.B = ps.B; sp.D = m->D; sp.Dp = m->Dp; sp.C = c.n_components;
    sp.logits = P_(m, m->t_prLogits); sp.loc = P_(m, m->t_prLoc); sp.scale_raw = P_(m, m->t_prScale);
    sp.resp = m->resp; sp.klw = p.klw;
    sp.g_logits = G_(m, m->t_prLogits); sp.g_loc = G_(m, m->t_prLoc); sp.g_scale = G_(m, m->t_prScale);
    sp.tie_mixtures = m->flags.tie_mixtures; sp.tie_loc = m->flags.tie_loc; sp.tie_scale = m->flags.tie_scale; sp.tril = m->scale_tril;
    sp.tril_part = m->tril_part; sp.tril_part_floats = m->tril_part_floats;
    SMX_CHECK(launch_scale_prior_bwd(m->st, sp));
  }
  // Products that only the optimiser reads (the weight gradients of the first decoder layer, of the latent head and of
  // the first encoder layers) run as ONE grouped launch at the end; the last encoder layer's BatchNorm-backward
  // launch computes d h = d lat W_lat^T itself.  SMX_NO_BWD_FRONT=1: the separate launches of before.
  const MlpLayer& eL = m->enc.back();
  p.bfront = m->flags.bwd_front && !sync_bn_on(m, ps.training) && bn_bwd_front_supported(ps.B, p.lat_ld) && eL.out_p % 8 == 0 &&
             eL.act == SMX_ACT_RELU;   // (the gradient fronts build ReLU in)
  // fold_dz (round 6): the d z product and the latent head's backward inside the encoder's last BatchNorm-backward launch -- the plain
  // reparameterised latent of VAE / SISUA at D <= 32, a first decoder layer of 128 units, at most 128 cells, below the wide-panel width,
  // no second MLP sharing the launch (scvi)
  // (a property of the MODEL, not of the step: at a wide panel the optimiser's chunks may ride with the d z launch -- how many is scheduling
  // state --, so wide panels keep that launch whatever rides with it this step; the fold's rounding never depends on what else is going on)
  const bool wide_panel = m->Gp >= std::min(4096, head_fused_min_genes());
  m->fold_dz_now = p.bfront && !m->mixpost && !m->latent_tril && !m->scvi && !m->scale && !m->fvae && m->stochastic && !wide_panel && !m->dec.empty() &&
                   m->dec[0].out_p == 128 && m->dec[0].in_p == m->Dp && (m->tensors[m->dec[0].tW].ld % 4) == 0 && m->tensors[m->dec[0].tW].ld >= 128 &&
                   bn_bwd_fold_supported(ps.B, p.lat_ld, m->Dp);
  MlpBwdOpts o;
  o.defer = p.bfront ? &p.tail : nullptr;
  o.head_dw = m->dw_late_now ? &p.hb_late : nullptr;
  if (!m->mixpost && !m->latent_tril) {
    o.lat_epi = &le;
    return mlp_backward(m, m->dec, ps, {m->z, m->Dp}, false, p.n_slabs, o);
  }
  // d z leaves the decoder as slabs, a launch of its own turns it into d lat
  int dz_slabs = 1;
  o.out_slabs = &dz_slabs;
  SMX_CHECK(mlp_backward(m, m->dec, ps, {m->z, m->Dp}, false, p.n_slabs, o));
  Timed t(m, "latent_bwd");
  if (m->mixpost) {   // mixture-density posterior: every component's parameters through log q, the picked component's through z as well
    MixLatArgs ma;
    ma.lat = m->latbuf; ma.ld = p.lat_ld; ma.B = ps.B; ma.D = m->D; ma.Dp = m->Dp; ma.C = c.n_components;
    ma.z = m->z; ma.eps = m->eps; ma.resp = m->resp; ma.pick = m->zpick;
    ma.dz = m->slab; ma.dz_slabs = dz_slabs; ma.dz_slab_stride = (long)ps.B * m->dec[0].in_p; ma.ldz = m->dec[0].in_p;
    ma.klw = p.klw; ma.dlat = m->dlat;
    SMX_CHECK(launch_mixlat_bwd(m->st, ma));
  } else {   // the full-covariance posterior
    LatentTrilArgs ta;
    ta.lat = m->latbuf; ta.ld = p.lat_ld; ta.B = ps.B; ta.D = m->D; ta.Dp = m->Dp;
    ta.z = m->z; ta.diag = m->sig; ta.eps = m->eps;
    ta.dz = m->slab; ta.dz_slabs = dz_slabs; ta.dz_slab_stride = (long)ps.B * m->dec[0].in_p; ta.ldz = m->dec[0].in_p;
    ta.klw = p.klw; ta.dlat = m->dlat;
    SMX_CHECK(launch_latent_tril_bwd(m->st, ta));
  }
  return SMX_OK;
}

// ---- latent head: its weight gradient and d h = d lat * W_lat^T (a gradient front of the encoder's backward, or one grouped launch here) ----
static int bwd_latent_head(smx_model* m, const Pass& ps, BwdPass& p) {
  const MlpLayer& eL = m->enc.back();
  const Mat dlat{m->dlat, p.lat_ld}, W{P_(m, m->t_latW), m->tensors[m->t_latW].ld};
  GemmArgs pair[2];
  pair[0] = dense_wgrad(m, {eL.out_buf, eL.out_p}, dlat, m->t_latW, G_(m, m->t_latb), eL.out_p, p.lat_ld, ps.B);
  if (p.bfront) {
    BnBwdArgs& gf = p.gf;
    p.tail.push_back(pair[0]);
    gf.fD = dlat.p; gf.fld = dlat.ld; gf.fW = W.p; gf.fldw = W.ld; gf.fK = p.lat_ld;
    if (m->fold_dz_now) {
      const MlpLayer& d0 = m->dec[0];
      gf.fold_dz = 1; gf.zD = d0.dpre; gf.zld = d0.out_p; gf.zW = P_(m, d0.tW); gf.zldw = (int)m->tensors[d0.tW].ld; gf.zlb = p.le;
    }
    return SMX_OK;
  }
  // independent: one grouped launch
  GemmArgs& h = pair[1] = dense_dgrad(dlat, W, m->slab, ps.B, eL.out_p, p.lat_ld);
  int effs[2] = {1, 1};
  if (p.lat_ld > 128) {   // (a wide latent head -- the mixture-density posterior's (1 + 2 C) planes, the tril posterior's 1 + D: d h contracts over all of them)
    h.split_k = suggest_split_k(ps.B, eL.out_p, p.lat_ld);
    SMX_REQUIRE((size_t)std::max(h.split_k, 1) * (size_t)h.slab_stride <= m->slab_cap, "split-K slabs exceed the slab buffer");
  }
  Timed t(m, "gemm_lat_bwd");
  SMX_CHECK(launch_gemm_group(m->st, pair, 2, effs));
  p.dh_slabs = effs[1];
  return SMX_OK;
}

// ---- encoder.  scvi: the library encoder's last BatchNorm-backward takes its incoming gradient d h_l = d latl W_latl^T as a front
// too (K = 32) -- and then runs beside the encoder's in ONE launch when d latl is there already (the row-local head
// launch of the forward pass leaves it); the library head's weight gradient joins the grouped launch at the end
static int bwd_encoder(smx_model* m, const Pass& ps, BwdPass& p) {
  if (m->scvi) {
    const MlpLayer& lL = m->encl.back();
    const TensorInfo& tw = m->tensors[m->t_latlW];
    p.lfront = p.bfront && bn_bwd_front_supported(ps.B, 32) && lL.out_p % 8 == 0 && (tw.ld % 4) == 0 && lL.act == SMX_ACT_RELU;
    p.gfl.fD = m->dlatl; p.gfl.fld = 32; p.gfl.fW = P_(m, m->t_latlW); p.gfl.fldw = tw.ld; p.gfl.fK = 32;
  }
  const bool twin_bwd = m->scvi && p.lfront && m->scvi_fused;
  MlpBwdOpts o;
  o.skip_input_grad = true; o.label = "gemm_enc_dw"; o.defer_dw0 = &p.dw0[p.n_dw0++];
  o.front = p.bfront ? &p.gf : nullptr; o.defer = p.bfront ? &p.tail : nullptr;
  o.twin = twin_bwd ? &m->encl : nullptr; o.twin_front = twin_bwd ? &p.gfl : nullptr; o.twin_done = &p.twin_done;
  return mlp_backward(m, m->enc, ps, {ps.Xsrc, m->Gp}, true, p.dh_slabs, o);
}

// ---- scvi library branch ----
static int bwd_library(smx_model* m, const Pass& ps, BwdPass& p) {
  if (!m->scvi_fused) {
    LibLatentArgs ll;
    ll.latl = m->latlbuf; ll.ld = 32; ll.B = ps.B; ll.library = ps.lib; ll.rows = ps.rows;
    ll.sig = m->lsig; ll.eps = m->leps; ll.dl = m->dl; ll.klw = p.klw; ll.dlatl = m->dlatl;
    SMX_CHECK(launch_lib_latent_bwd(m->st, ll));
  }
  const MlpLayer& lL = m->encl.back();
  const Mat dlatl{m->dlatl, 32};
  const GemmArgs g = dense_wgrad(m, {lL.out_buf, lL.out_p}, dlatl, m->t_latlW, G_(m, m->t_latlb), lL.out_p, 32, ps.B);
  if (p.lfront) {
    p.tail.push_back(g);
  } else {
    // weight and input gradient of the library head: independent, one grouped launch
    GemmArgs pair[2] = {g, dense_dgrad(dlatl, {P_(m, m->t_latlW), m->tensors[m->t_latlW].ld}, m->slab, ps.B, lL.out_p, 32)};
    SMX_CHECK(launch_gemm_group(m->st, pair, 2));
  }
  MlpBwdOpts o;
  o.skip_input_grad = true; o.label = "gemm_encl_dw"; o.defer_dw0 = &p.dw0[p.n_dw0++];
  o.front = p.lfront ? &p.gfl : nullptr; o.defer = p.bfront ? &p.tail : nullptr; o.last_bn_done = p.twin_done;
  return mlp_backward(m, m->encl, ps, {ps.Xsrc, m->Gp}, true, 1, o);
}

// ---- tail: the deferred weight gradients -- with the first-layer ones (gather + log1p of the same resident rows) of the encoder and, for
// scvi, the library encoder -- are independent: one grouped launch
static int bwd_tail(smx_model* m, const Pass& ps, BwdPass& p) {
  std::vector<GemmArgs>& tail = p.tail;
  for (int q = 0; q < p.n_dw0; ++q) tail.push_back(p.dw0[q]);
  Timed t(m, "gemm_enc_dw");
  // every product here contracts over the minibatch: the wide direct-operand kernel takes them all in one launch
  // (SMX_NO_WGRAD=1, input dropout or an unsupported shape: the LDS-tiled products)
  bool wg_ok = m->flags.wgrad && tail.size() <= SMX_GROUP_MAX;
  for (const GemmArgs& g : tail) wg_ok = wg_ok && wgrad_supported(g, ps.B);
  if (wg_ok) SMX_CHECK(launch_wgrad_group(m->st, tail.data(), (int)tail.size(), ps.B, b3_on(m, ps.B) ? 1 : 0));
  else if (tail.size() == 1) SMX_CHECK(launch_gemm(m->st, tail[0]));
  else
    for (size_t q = 0; q < tail.size(); q += SMX_GROUP_MAX)
      SMX_CHECK(launch_gemm_group(m->st, tail.data() + q, (int)std::min<size_t>(SMX_GROUP_MAX, tail.size() - q)));
  return SMX_OK;
}

int backward_pass(smx_model* m, const Pass& ps) {
  std::fill(m->sq_count.begin(), m->sq_count.end(), 0);   // the products of this step report what they wrote
  std::fill(m->sq_reduced.begin(), m->sq_reduced.end(), 0);
  m->adam_early_pending = false; m->adam_rest_from = m->adam_rest_to = 0; m->adam_ride_b = 0;
  if (!m->chain_started) m->adam_early_from = -1;   // (forward_pass may have sent the heads' chunks down the data-parallel chain already)
  m->lab_deferred = false; m->dw_late_now = false;
  if (m->fvae) SMX_CHECK(factor_backward(m, ps));   // first: it uses the slab buffer the head's backward fills next
  const MlpLayer& dL = m->dec.back();
  BwdPass p;
  p.klw = kl_weight(m, ps, 1.f / (float)ps.global_batch, 0);
  p.lat_ld = m->lat_planes * m->Dp; p.dd_stride = (long)ps.B * dL.out_p; p.dparams = m->dP;
  if (m->scvi) {
    ScviHeadArgs sh = scvi_head_args(m, ps);
    sh.dplanes = m->dP; sh.draw = m->draw; sh.dl = m->dl;
    if (!m->scvi_fused) SMX_CHECK(launch_scvi_head_bwd(m->st, sh));   // (the row-local head launch of the forward pass left d raw and d l)
    p.dparams = m->draw;
  }
  const bool all_heads = m->out_has_W[1] && (m->k < 3 || m->out_has_W[2]);   // (scvi with a 'share'd plane: the grouped products)
  p.hbwd = m->flags.head_bwd && head_bwd_supported(ps.B, dL.out_p, m->Gp) && m->k >= 2 && m->k <= 3 && all_heads;
  if (p.hbwd) SMX_CHECK(bwd_out_head(m, ps, p));
  SMX_CHECK(bwd_head_group(m, ps, p));
  SMX_CHECK(bwd_heads_final(m));
  SMX_CHECK(bwd_decoder(m, ps, p));
  SMX_CHECK(lazy_flush(m));   // (W_enc's chunks of the step before, if the decoder's launch did not take them after all: ahead of this step's weight gradients)
  for (const GemmArgs& g : p.lab_dw) p.tail.push_back(g);
  SMX_CHECK(bwd_latent_head(m, ps, p));
  SMX_CHECK(bwd_encoder(m, ps, p));
  if (m->scvi) SMX_CHECK(bwd_library(m, ps, p));
  return bwd_tail(m, ps, p);
}

}  // namespace smx
