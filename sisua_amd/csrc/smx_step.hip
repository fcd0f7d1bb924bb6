// smx_step.hip -- one training / evaluation step: forward (smx_forward.hip), backward (smx_backward.hip), (all-reduce), the optimiser pass;
// eager and captured-graph execution, the ELBO scalars' read-back, the training / evaluation entry points.
#include "smx_model.h"

namespace smx {

__global__ void bn_moving_update_kernel(float* moving, const float* batch_sum, int n, float inv_world, float momentum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) moving[i] = moving[i] * momentum + batch_sum[i] * inv_world * (1.f - momentum);
}

// everything of AdamArgs that does not depend on which launch carries the chunks
void fill_adam_args(smx_model* m, AdamArgs& a) {
  const smx_config& c = m->cfg;
  a.params = m->params; a.grads = m->grads; a.m = m->adam_m; a.v = m->adam_v;
  a.chunks = m->chunks; a.n_chunks = m->n_chunks; a.n_launch = m->n_chunks; a.gap_from = m->n_chunks; a.gap_len = 0;
  a.partial = m->partial; a.tensor_norm = m->tensor_norm;
  // norms from the products' partials when every large tensor has them (single GPU: under data parallelism the
  // norm is that of the all-reduced gradient, which only a pass after the collective can give)
  a.use_sq = (m->sq_slots != nullptr && !dp_active(m) && !tuning_on("no_sq_partials")) ? 1 : 0;
  for (size_t t = 0; t < m->tensors.size() && a.use_sq; ++t) {
    a.sq_first[t] = m->sq_first[t]; a.sq_count[t] = m->sq_count[t];
    if (m->sq_count[t] == 0 && m->tensors[t].count > SMX_SQ_SMALL_TENSOR) a.use_sq = 0;
    if (m->sq_reduced[t]) { a.sq_first[t] = m->sq_total_first + (int)t * SMX_SQR_PER_TENSOR; a.sq_count[t] = m->sq_reduced[t]; }   // riders have summed the slots
  }
  a.sq_slots = m->sq_slots;
  a.state = cur_state(m); a.clipnorm = c.clipnorm;
  opt_scalars(m->opt_rule, m->opt_hp, a); a.t0 = m->opt_t0;   // (the rule of smx_set_optimizer: Adam with the config's betas and epsilon unless set)
  // the likelihood / KL / label kernels already scale by 1 / (batch * world), so the SUM all-reduce leaves the
  // global-mean gradient: nothing more to divide by (it used to be divided by world once more here)
  a.grad_scale = 1.f;
  if (m->scale && (m->flags.tie_loc || m->flags.tie_scale)) {
    a.tied_t0 = m->flags.tie_loc ? m->t_prLoc : -1; a.tied_t1 = m->flags.tie_scale ? m->t_prScale : -1;
    a.tied_inv = 1.f / (float)c.n_components;
  }
}

void fill_step_close(smx_model* m, AdamArgs& a) {
  a.state = cur_state(m);
  a.master = master_state(m); a.sched = m->sched_tab; a.batch = m->seq_batch;
  if (dp_active(m)) { a.hist_dp = m->mhist; a.tail_metrics = m->grads + m->tail_off_metrics; }
  a.prepare_next = m->seq_prepare_next;
  if (a.prepare_next) { a.next_state = m->state3 + (m->par ^ 1); a.next_rows = m->rows2[m->par ^ 1]; a.order = m->order; }
}

// ---- the lazy encoder update ----
// The optimiser launch is the last of the step's ten dependent launches, and between two steps of one train_steps call only ONE launch needs its
// largest tensor soon: the next step's first, the gathered encoder product, which loads exactly W_enc.  A step that is not the call's last therefore
// leaves the launch out (lazy_adam_wanted + what mlp_forward / mlp_backward report of the step); the next step's forward pass applies it:
//   launch 1 (gemm_ride_kernel, tile form): every tile workgroup updates its block of W_enc in REGISTERS while staging it (adam_apply4 on the
//            quads it loads anyway, beside the matching quads of the gradient and both moments; nothing of them stored); trailing workgroups
//            apply every pending chunk but W_enc's in place -- tensors first read by launches 2..5;
//   a later forward product that reads neither W_enc nor its gradient (the latent head's) carries W_enc's own chunks in place.
// The same function calls as the optimiser launch (adam_tensor_clip<256>, adam_apply4, adam_chunk_body<256>): every result bit for bit.
// Knob no_lazy_adam; smx_lazy_adam_steps counts the steps that took the form.
bool lazy_adam_wanted(smx_model* m, bool prepare_next) {
  if (!prepare_next || m->capturing || tuning_on("no_lazy_adam")) return false;
  if (m->comm || m->local || m->p2p || dp_active(m) || m->sync_bn || m->flags.opt_shard) return false;   // one GPU
  if (!m->timing_label.empty() || m->use_injected) return false;   // (per-kernel timings keep the unfolded path)
  if (m->opt_rule != SMX_OPT_ADAM) return false;                  // the riders carry Adam only
  if (m->scvi || m->fvae || m->enc.empty()) return false;         // ONE encoder reads X, once per step
  if (!m->sq_slots || tuning_on("no_sq_partials")) return false;
  return true;
}

// W_enc's chunks in the table (smx_model.hip builds it tensor by tensor, SMX chunks_floats floats each)
static void lazy_w_chunks(const smx_model* m, int* first, int* n) {
  const int tW = m->enc[0].tW;
  int f = 0;
  for (int t = 0; t < tW; ++t) f += (int)((m->tensors[t].count + m->chunks_floats - 1) / m->chunks_floats);
  *first = f; *n = (int)((m->tensors[tW].count + m->chunks_floats - 1) / m->chunks_floats);
}

// the step's optimiser launch as `a` describes it: left to the next step?  (the last gate: everything of the predicate that only the step's
// own launches could tell)
static bool lazy_defer(smx_model* m, const AdamArgs& a) {
  if (!m->lazy_want || !m->lazy_l1 || !m->lazy_closed || m->have_pending_metrics || !a.use_sq || a.form != OPT_ADAM || !a.prepare_next) return false;
  int wf, wn;
  lazy_w_chunks(m, &wf, &wn);
  if (wn <= 0 || wf + wn > a.gap_from) return false;   // (W_enc's chunks before the heads' gap: launch index == chunk index)
  m->lazy_args = a;
  m->lazy_args.master = nullptr; m->lazy_args.with_metrics = 0;   // (both rode with the encoder's BatchNorm-backward launch)
  m->lazy_w_first = wf; m->lazy_w_n = wn;
  m->lazy_rest_pending = m->lazy_w_pending = true;
  ++m->lazy_steps;
  return true;
}

int lazy_flush(smx_model* m) {
  if (!m->lazy_rest_pending && !m->lazy_w_pending) return SMX_OK;
  AdamArgs a = m->lazy_args;
  if (!m->lazy_rest_pending) { a.gap_from = 0; a.gap_len = m->lazy_w_first; a.n_launch = m->lazy_w_n; }   // W_enc's chunks alone
  m->lazy_rest_pending = m->lazy_w_pending = false;
  return launch_adam(m->st, a);
}

bool lazy_ride_tile(smx_model* m, const GemmArgs& g, GemmRide& r) {
  if (!m->lazy_rest_pending || !m->lazy_w_pending || m->capturing) return false;
  const TensorInfo& tw = m->tensors[m->enc[0].tW];
  if (g.B != m->params + tw.offset || g.ldb != (int)tw.ld || (size_t)g.K * (size_t)g.ldb > tw.count || g.N > g.ldb || !gemm_ride_tile_supported(g)) return false;   // (the tile's quads lie inside the tensor)
  r.adam = &m->lazy_args;
  r.count = m->lazy_args.n_launch - m->lazy_w_n; r.skip_from = m->lazy_w_first; r.skip_len = m->lazy_w_n;
  r.tile = 1; r.w_off = (long)tw.offset;
  memset(&r.w_chunk, 0, sizeof(r.w_chunk));
  r.w_chunk.tensor = m->enc[0].tW; r.w_chunk.offset = (int32_t)tw.offset; r.w_chunk.count = (int32_t)std::min<size_t>(tw.count, (size_t)m->chunks_floats);
  r.w_chunk.first_chunk = m->lazy_w_first; r.w_chunk.n_chunks = m->lazy_w_n; r.w_chunk.tensor_count = (int32_t)tw.count;
  return true;   // (the caller clears lazy_rest_pending once the launch is out)
}

bool lazy_ride_w(smx_model* m, GemmRide& r) {
  if (m->lazy_rest_pending || !m->lazy_w_pending || m->capturing) return false;
  r.adam = &m->lazy_args;
  r.count = m->lazy_w_n; r.skip_from = 0; r.skip_len = m->lazy_w_first; r.tile = 0;
  return true;   // (the caller clears lazy_w_pending once the launch is out)
}

int optimizer_pass(smx_model* m) {
  const smx_config& c = m->cfg;
  if (dp_active(m) && m->have_pending_metrics) {   // no BatchNorm-backward launch took them along
    SMX_CHECK(launch_metrics(m->st, m->pending_metrics));
    m->have_pending_metrics = false;
  }
  const bool chain = dp_chain_ok(m);
  if (chain) {
    Timed t(m, "allreduce");
    SMX_CHECK(dp_chain_start(m));   // (a no-op when the forward or the backward pass started it)
    SMX_CHECK(dp_allreduce(m, 0, m->bucket1_off, m->st));   // front bucket [encoder / latent / decoder | BatchNorm statistics | ELBO scalars]
  } else if (dp_active(m)) {
    Timed t(m, "allreduce");
    if (m->bucket1_in_flight) {
      // front bucket [encoder/latent/decoder grads | BN stats | metrics] behind the head bucket on the
      // communication stream; the optimiser waits for both
      SMX_HIP(hipEventRecord(m->ev_c2, m->st));
      SMX_HIP(hipStreamWaitEvent(m->st_comm, m->ev_c2, 0));
      SMX_CHECK(dp_allreduce(m, 0, m->bucket1_off, m->st_comm));
      SMX_HIP(hipEventRecord(m->ev_c3, m->st_comm));
      SMX_HIP(hipStreamWaitEvent(m->st, m->ev_c3, 0));
      m->bucket1_in_flight = false;
    } else {
      SMX_CHECK(dp_allreduce(m, 0, m->grads_count, m->st));   // one all-reduce of the whole flat buffer
    }
  }
  AdamArgs a;
  fill_adam_args(m, a);
  if (chain) a.sq_chunks = m->chunk_first_head;   // (the heads' chunks have their norm pass on the communication stream)
  m->chain_started = false;
  if (dp_active(m) && m->bn_total && m->world > 1) {
    if (!a.use_sq) {   // (the usual case under data parallelism: the gradient-norm launch takes the update along)
      a.bn_moving = m->bn_moving; a.bn_batch = m->grads + m->tail_off_bn; a.bn_total = (int)m->bn_total;
      a.bn_inv_world = 1.f / (float)m->world; a.bn_momentum = c.bn_momentum;
    } else {
      hipLaunchKernelGGL(bn_moving_update_kernel, dim3((unsigned)((m->bn_total + 255) / 256)), dim3(256), 0, m->st,
                         m->bn_moving, m->grads + m->tail_off_bn, (int)m->bn_total, 1.f / (float)m->world,
                         c.bn_momentum);
    }
  }
  if (m->adam_early_from >= 0) {   // the head chunks have ridden along already
    a.gap_from = m->adam_early_from; a.gap_len = m->adam_early_to - m->adam_early_from;
    a.n_launch = m->n_chunks - a.gap_len;
  } else {
    a.gap_from = m->n_chunks; a.gap_len = 0; a.n_launch = m->n_chunks;
  }
  m->adam_early_from = -1;
  if (m->have_pending_metrics) { a.metrics = m->pending_metrics; a.with_metrics = 1; m->have_pending_metrics = false; }
  fill_step_close(m, a);
  if (m->lazy_closed) a.master = nullptr;   // (a rider of the encoder's BatchNorm-backward launch has closed the step)
  if (lazy_defer(m, a)) return SMX_OK;      // the next step's forward launches apply it (the lazy encoder update, above)
  Timed t(m, "adam");
  SMX_CHECK(launch_adam(m->st, a));
  return SMX_OK;
}

// sparse store: expand the rows of this pass into the dense tile the readers of X take (they then index it with
// identity rows; everything else -- labels, library prior, label mask, lgx1, noise keys -- keeps the resident row ids)
int csr_stage(smx_model* m, Pass& ps) {
  if (!m->x_csr || ps.Xsrc != m->X) return SMX_OK;
  SMX_REQUIRE(ps.rows != nullptr && ps.B <= m->Rmax, "sparse store: resident rows only");
  SMX_REQUIRE(!(ps.training && m->cfg.input_dropout > 0.f), "sparse store: input dropout is keyed by the dense store's rows (use the float32 / uint16 store)");
  SMX_CHECK(launch_csr_expand(m->st, m->csr_indptr, m->csr_cols, m->csr_vals, ps.rows, 0, ps.B, m->Gp, m->xbatch));
  ps.Xsrc = m->xbatch; ps.xrows = nullptr; ps.x_u16 = 0;
  return SMX_OK;
}

// the whole training step as a launch sequence on m->st (capturable).
//   with_begin:   launch the state/row-id preparation kernel first (graph replay: every step, cursor kept in
//                 the master state; eager: only the first step of a train_steps call)
//   prepare_next: the optimiser kernel prepares the other parity's state + row ids for the step after
int train_sequence(smx_model* m, int B, bool with_begin, bool begin_from_master, uint32_t cursor, bool prepare_next) {
  Pass ps;
  ps.B = B; ps.rows = cur_rows(m); ps.xrows = ps.rows; ps.Xsrc = m->X; ps.x_u16 = m->x_u16; ps.lib = m->library; ps.lgx1 = m->lgx1;
  ps.cell_base = (uint32_t)m->cell_base; ps.training = 1; ps.sample = 0; ps.global_batch = B * m->world;
  ps.draw_rows = m->train_draws > 1 ? B / m->train_draws : 0;   // (B: the stacked rows, draws x cells)
  m->seq_batch = B; m->seq_prepare_next = prepare_next ? 1 : 0;
  m->lazy_want = lazy_adam_wanted(m, prepare_next); m->lazy_l1 = false; m->lazy_closed = false;
  Timed t(m, "step");
  if (with_begin) {
    AdamArgs o;
    opt_scalars(m->opt_rule, m->opt_hp, o);
    SMX_CHECK(launch_step_begin(m->st, master_state(m), cur_state(m), m->order, cur_rows(m), B, begin_from_master ? 1 : 0,
                                cursor, m->sched_tab, o.b1, o.b2, o.form, m->opt_t0));
  }
  m->chain_started = false;
  { Timed null_pair(m, "null"); }  // an event pair around nothing: the timing method's own overhead
  SMX_CHECK(csr_stage(m, ps));     // sparse store: this minibatch's rows as a dense tile (no-op otherwise)
  SMX_CHECK(forward_pass(m, ps, Loss::Train));
  SMX_CHECK(backward_pass(m, ps));
  SMX_CHECK(optimizer_pass(m));
  return SMX_OK;
}

// the seam form's error word (smx_backward.hip, smx_handoff.h): non-zero after a wait inside the fused BatchNorm-backward launch gave up -- that
// step's encoder gradients were never written.  Read wherever the step's scalars are read; reported once, then cleared.
static unsigned* seam_error_word(smx_model* m) { return m->seam_state + HANDOFF_MAX_SHARDS * HANDOFF_SHARD_STRIDE; }
int seam_error_check(smx_model* m) {
  if (!m->seam_state) return SMX_OK;
  unsigned e = 0;
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_HIP(hipMemcpy(&e, seam_error_word(m), sizeof(e), hipMemcpyDeviceToHost));
  if (!e) return SMX_OK;
  SMX_HIP(hipMemset(seam_error_word(m), 0, sizeof(e)));
  set_error("BatchNorm-backward seam: the encoder's workgroups gave up waiting for the decoder's d pre-activation inside the fused launch (knob no_bwd_seam runs the two launches)");
  return SMX_ERR_HIP;
}

int read_metrics(smx_model* m, smx_metrics* out) {
  if (!out) return SMX_OK;
  // into pinned memory (two real DMA copies; into pageable arrays the runtime stages each one synchronously)
  const size_t nt = m->tensors.size();
  if (!m->metrics_pin) SMX_HIP(hipHostMalloc((void**)&m->metrics_pin, (8 + nt + 2) * sizeof(float), hipHostMallocDefault));
  float* h = m->metrics_pin;
  float* norms_p = m->metrics_pin + 8;
  unsigned* p2p_err = reinterpret_cast<unsigned*>(m->metrics_pin + 8 + nt);
  *p2p_err = 0u;
  unsigned* seam_err = p2p_err + 1;
  *seam_err = 0u;
  SMX_HIP(hipMemcpyAsync(h, m->grads + m->tail_off_metrics, 8 * sizeof(float), hipMemcpyDeviceToHost, m->st));
  SMX_HIP(hipMemcpyAsync(norms_p, m->tensor_norm, nt * sizeof(float), hipMemcpyDeviceToHost, m->st));
  if (m->p2p && m->p2p->error) SMX_HIP(hipMemcpyAsync(p2p_err, m->p2p->error, sizeof(unsigned), hipMemcpyDeviceToHost, m->st));
  if (m->seam_state) SMX_HIP(hipMemcpyAsync(seam_err, seam_error_word(m), sizeof(unsigned), hipMemcpyDeviceToHost, m->st));
  SMX_HIP(hipStreamSynchronize(m->st));
  if (*seam_err) SMX_CHECK(seam_error_check(m));
  if (*p2p_err) {   // a bounded wait of the peer-to-peer exchange gave up on this rank or on a peer: every rank's step is garbage
    set_error(*p2p_err == 1u ? "peer-to-peer all-reduce: a wait on a peer's flag timed out (SMX_P2P_TIMEOUT_S)" :
                               "peer-to-peer all-reduce: a peer reported a timed-out wait");
    return SMX_ERR_COMM;
  }
  std::vector<float> norms(norms_p, norms_p + nt);
  out->loss = h[0]; out->nllk_x = h[1]; out->nllk_y = h[2]; out->kl = h[3]; out->kl_l = h[4];
  float mx = 0.f;
  for (float v : norms) mx = (v > mx || v != v) ? v : mx;
  out->grad_norm_max = mx;
  out->nan_flag = !(isfinite(h[0]) && isfinite(h[1]) && isfinite(h[3]) && isfinite(mx));
  out->step = (int32_t)m->h_next;
  out->tc = h[5]; out->dtc_loss = h[6]; out->nllk_o = h[7];
  if (m->n_observed && !isfinite(h[7])) out->nan_flag = 1;
  if (m->fvae && !(isfinite(h[5]) && isfinite(h[6]))) out->nan_flag = 1;
  return SMX_OK;
}

int upload_order(smx_model* m, const int32_t* order, size_t n, size_t n_steps) {
  if (n_steps > m->mhist_cap) {
    SMX_HIP(hipStreamSynchronize(m->st));
    drop_graphs(m);
    if (m->mhist) hipFree(m->mhist);
    m->mhist = nullptr; m->mhist_cap = 0;
    SMX_CHECK(dmalloc(&m->mhist, (n_steps * 2 + 64) * 8));
    m->mhist_cap = n_steps * 2 + 64;
  }
  m->mhist_steps = (int32_t)n_steps;
  if (n > m->order_cap) {
    SMX_HIP(hipStreamSynchronize(m->st));
    drop_graphs(m);
    if (m->order) hipFree(m->order);
    m->order = nullptr;
    m->order_cap = n * 2 + (size_t)m->Bmax;
    SMX_CHECK(dmalloc(&m->order, m->order_cap));
  }
  // the schedule table: (beta, lr) of each of the call's steps, by cursor (a captured graph keeps reading this buffer: it goes with the graphs)
  if (n_steps > m->sched_cap) {
    SMX_HIP(hipStreamSynchronize(m->st));
    drop_graphs(m);
    if (m->sched_tab) hipFree(m->sched_tab);
    m->sched_tab = nullptr;
    m->sched_cap = n_steps * 2 + 64;
    SMX_CHECK(dmalloc(&m->sched_tab, m->sched_cap));
  }
  // through a pinned buffer of the model's own: the copy is then a real asynchronous DMA (from pageable memory the runtime
  // stages it synchronously: ~80 us for 10 KB, 4 us per step of a 20-step call).  The buffer is reused only after the
  // previous call's copy has run (an event; by then normally long done).  The row ids, then the schedule table (2 floats per step)
  const size_t need = n + 2 * n_steps;
  if (need > m->order_pin_cap) {
    if (m->order_pin_busy) { SMX_HIP(hipEventSynchronize(m->ev_order)); m->order_pin_busy = false; }
    if (m->order_pin) hipHostFree(m->order_pin);
    m->order_pin = nullptr; m->order_pin_cap = 0;
    SMX_HIP(hipHostMalloc((void**)&m->order_pin, (need * 2 + (size_t)m->Bmax) * sizeof(int32_t), hipHostMallocDefault));
    m->order_pin_cap = need * 2 + (size_t)m->Bmax;
  }
  if (!m->ev_order) SMX_HIP(hipEventCreateWithFlags(&m->ev_order, hipEventDisableTiming));
  if (m->order_pin_busy) { SMX_HIP(hipEventSynchronize(m->ev_order)); m->order_pin_busy = false; }
  memcpy(m->order_pin, order, n * sizeof(int32_t));
  float* tab = reinterpret_cast<float*>(m->order_pin + n);
  sched_fill(m, tab, n_steps);
  SMX_HIP(hipMemcpyAsync(m->order, m->order_pin, n * sizeof(int32_t), hipMemcpyHostToDevice, m->st));
  SMX_HIP(hipMemcpyAsync(m->sched_tab, tab, n_steps * sizeof(float2), hipMemcpyHostToDevice, m->st));
  SMX_HIP(hipEventRecord(m->ev_order, m->st));
  m->order_pin_busy = true;
  SMX_HIP(hipMemsetAsync(&master_state(m)->cursor, 0, sizeof(uint32_t), m->st));
  return SMX_OK;
}

int check_rows(smx_model* m, const int32_t* ids, size_t n) {
  SMX_REQUIRE(m->X != nullptr, "no dataset uploaded (smx_dataset_upload)");
  for (size_t i = 0; i < n; ++i)
    if (ids[i] < 0 || (int64_t)ids[i] >= m->N) { set_error("row id out of range"); return SMX_ERR_INVALID; }
  return SMX_OK;
}

int launch_train(smx_model* m, int B, bool use_graph, int s_idx, int n_steps) {
  // With a communicator the RCCL all-reduce is captured too (RCCL supports stream capture);
  // SMX_NO_GRAPH_COMM=1 or a failed capture falls back to eager launches for good.
  static const bool no_graph_comm = tuning_on("no_graph_comm");
  // (the peer-to-peer exchange carries its epoch as a kernel argument: never captured)
  if (use_graph && !m->local && !m->p2p && !(m->comm && (no_graph_comm || m->graph_comm_failed)) && !m->use_injected && m->timing_label.empty()) {
    auto it = m->graphs.find(B);
    if (it == m->graphs.end()) {
      hipGraph_t graph = nullptr;
      SMX_HIP(hipStreamBeginCapture(m->st, hipStreamCaptureModeThreadLocal));
      m->capturing = true;
      m->par = 0;
      int rc = train_sequence(m, B, true, true, 0, false);
      m->capturing = false;
      hipError_t e = hipStreamEndCapture(m->st, &graph);
      hipGraphExec_t exec = nullptr;
      if (rc == SMX_OK && e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      if (graph) hipGraphDestroy(graph);
      if (rc != SMX_OK || e != hipSuccess) {
        (void)hipGetLastError();
        if (m->comm) {  // capture with the collective failed: run this and all later steps eagerly
          m->graph_comm_failed = true;
          SMX_CHECK(train_sequence(m, B, true, true, 0, false));
          m->h_next += 1;
          return SMX_OK;
        }
        if (rc != SMX_OK) return rc;
        set_error(std::string("graph capture failed: ") + hipGetErrorString(e));
        return SMX_ERR_HIP;
      }
      it = m->graphs.emplace(B, exec).first;
    }
    m->par = 0;
    m->audit_rows = B; if (m->fvae) m->audit_disc_rows = 2 * B;   // (a replay runs none of the host code that records them)
    SMX_HIP(hipGraphLaunch(it->second, m->st));
  } else {
    // eager: the preparation kernel runs once per call; afterwards each optimiser kernel prepares the
    // other parity's state + row ids, so a step is not fronted by a 1-workgroup latency kernel
    const bool first = (s_idx == 0), last = (s_idx == n_steps - 1);
    if (first) m->par = 0; else m->par ^= 1;
    const int rc = train_sequence(m, B, first, false, (uint32_t)s_idx, !last);
    if (rc != SMX_OK) {   // an update of the step before still pending: as the ordinary launch, before the error goes up
      (void)lazy_flush(m);
      return rc;
    }
  }
  m->h_next += 1;
  return SMX_OK;
}

int setup_pass(smx_model* m, Pass& ps, const CellSrc& src, int32_t batch, int training, int sample, int draw_rows) {
  const int32_t* row_ids = src.row_ids;
  const float *host_x = src.rows.x, *host_library = src.host_library;
  SMX_REQUIRE(batch > 0 && batch <= (draw_rows > 0 ? m->Rmax : m->Bmax), "batch must be in 1..max_batch");
  ps.B = batch; ps.training = training; ps.sample = sample; ps.global_batch = batch; ps.draw_rows = draw_rows;
  if (row_ids) {
    SMX_CHECK(check_rows(m, row_ids, (size_t)batch));
    // (through pinned staging of the library's own: measured, no gain -- 512 bytes from a pageable array take the runtime's fast path)
    SMX_HIP(hipMemcpyAsync(cur_rows(m), row_ids, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice, m->st));
    ps.rows = cur_rows(m); ps.xrows = ps.rows; ps.Xsrc = m->X; ps.x_u16 = m->x_u16; ps.lib = m->library; ps.lgx1 = m->lgx1; ps.cell_base = (uint32_t)m->cell_base;
    SMX_CHECK(csr_stage(m, ps));
  } else {
    SMX_REQUIRE(host_x || src.rows.csr.indptr, "need row_ids or host rows");
    SMX_REQUIRE(!m->scvi || host_library, "scvi needs host_library with host rows");
    if (host_x) {
      SMX_HIP(hipMemsetAsync(m->hostX, 0, (size_t)batch * m->Gp * sizeof(float), m->st));
      SMX_HIP(hipMemcpy2DAsync(m->hostX, (size_t)m->Gp * sizeof(float), host_x, (size_t)m->G * sizeof(float),
                               (size_t)m->G * sizeof(float), (size_t)batch, hipMemcpyHostToDevice, m->st));
      SMX_CHECK(launch_row_stats(m->st, m->hostX, 0, m->Gp, batch, m->G, m->hostLgx1, nullptr));
    } else SMX_CHECK(csr_host_rows(m, src.rows.csr, 0, (size_t)batch, m->hostX, m->hostLgx1));   // (CSR rows, checked by the entry's host_rows: the tile and the constants from one launch)
    if (host_library) SMX_HIP(hipMemcpy(m->hostLib, host_library, (size_t)batch * 2 * sizeof(float), hipMemcpyHostToDevice));
    ps = host_rows_pass(batch, m->hostX, m->hostLib, m->hostLgx1);
    ps.training = training; ps.sample = sample; ps.draw_rows = draw_rows;
  }
  return SMX_OK;
}

// several draws per cell (smx_set_train_draws): what the step cannot take along
int check_draws(smx_model* m) {
  if (m->train_draws == 1) return SMX_OK;
  SMX_REQUIRE(m->world == 1, "several draws per cell are single-GPU only: smx_set_train_draws(m, 1) before a data-parallel step");
  SMX_REQUIRE(!m->use_injected, "injected noise (smx_set_noise) covers one draw: smx_set_train_draws(m, 1) first");
  return SMX_OK;
}

// the routing capacities of stacked passes (set_row_caps) for the life of a train / eval call with several draws; every other pass -- one
// draw, predict, scoring -- routes by the max_batch capacities, as on an engine that never took several draws
struct DrawCaps {
  smx_model* m;
  explicit DrawCaps(smx_model* m_) : m(m_) { if (m->train_draws > 1) set_row_caps(m, (size_t)m->train_draws * m->Bmax); }
  ~DrawCaps() { if (m->train_draws > 1) set_row_caps(m, (size_t)m->Bmax); }
};

// the row ids of n_steps minibatches of `batch` cells as the stacked rows of train_draws draws each, draw-major (row r of a step is
// draw r / batch of cell r % batch); empty with one draw
std::vector<int32_t> tile_draws(const smx_model* m, const int32_t* ids, int n_steps, int batch) {
  std::vector<int32_t> out;
  const int S = m->train_draws;
  if (S == 1) return out;
  out.resize((size_t)n_steps * S * batch);
  for (int t = 0; t < n_steps; ++t)
    for (int s = 0; s < S; ++s)
      memcpy(out.data() + ((size_t)t * S + s) * batch, ids + (size_t)t * batch, (size_t)batch * sizeof(int32_t));
  return out;
}

}  // namespace smx

extern "C" {

int smx_set_train_draws(smx_model* m, int32_t n_draws) {
  SMX_REQUIRE(m, "null model");
  SMX_REQUIRE(n_draws >= 1, "smx_set_train_draws: the number of draws must be >= 1");
  SMX_REQUIRE(n_draws == 1 || !m->fvae, "smx_set_train_draws: FactorVAE / SemiFVAE train with one draw (permute_dims over stacked draws has no agreed reading)");
  SMX_REQUIRE(n_draws == 1 || m->world == 1, "smx_set_train_draws: several draws per cell are single-GPU only (data parallel world > 1)");
  SMX_REQUIRE((int64_t)n_draws * m->Bmax <= (int64_t)1 << 20, "smx_set_train_draws: draws x max_batch exceeds 2^20 stacked rows");
  if (n_draws == m->train_draws) return SMX_OK;
  SMX_CHECK(smx::head_sweep_join(m));
  SMX_HIP(hipStreamSynchronize(m->st));
  smx::drop_graphs(m);   // (a captured step bakes the stacked batch and the buffers in)
  // (all or nothing: a failed grow leaves the buffers, Rmax and the draw count as they were)
  if ((int64_t)n_draws * m->Bmax > m->Rmax) SMX_CHECK(smx::alloc_rows(m, (size_t)n_draws * m->Bmax));
  m->train_draws = n_draws;
  m->staged_steps = 0;
  return SMX_OK;
}

int smx_set_optimizer(smx_model* m, int32_t rule, const float* hp, int32_t n_hp) {
  SMX_REQUIRE(m, "null model");
  const float adam_hp[3] = {m->cfg.adam_beta1, m->cfg.adam_beta2, m->cfg.adam_eps};
  float res[4];
  SMX_CHECK(smx::opt_resolve(rule, hp, n_hp, adam_hp, res));
  SMX_CHECK(smx::head_sweep_join(m));
  SMX_HIP(hipStreamSynchronize(m->st));
  smx::drop_graphs(m);   // (a captured step bakes the rule and t0 into its launches' arguments)
  // the rule starts fresh: both slot buffers whole (the SMX_SHARD_SLACK tail included), on every rank alike -- nothing is stale after this
  const long n = (long)(m->flat_count + SMX_SHARD_SLACK);
  SMX_CHECK(smx::launch_opt_fill(m->st, m->adam_m, n, 0.f));
  SMX_CHECK(smx::launch_opt_fill(m->st, m->adam_v, n, 0.f));
  if (rule == SMX_OPT_ADAGRAD && res[0] != 0.f) {
    // the accumulator's initial value goes into the LOGICAL elements only: the padding stays exactly zero (smx_model.h), its gradient being zero
    std::vector<float> h((size_t)n, 0.f);
    for (const TensorInfo& t : m->tensors)
      for (int r = 0; r < t.rows; ++r)
        for (int ch = 0; ch < t.chunks; ++ch)
          std::fill_n(h.begin() + (long)(t.offset + (size_t)r * t.ld + (size_t)ch * t.chunk_wp), t.chunk_w, res[0]);
    SMX_HIP(hipStreamSynchronize(m->st));
    SMX_HIP(hipMemcpy(m->adam_v, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  SMX_HIP(hipStreamSynchronize(m->st));
  m->opt_stale = false;
  m->opt_rule = rule;
  for (int i = 0; i < 4; ++i) m->opt_hp[i] = res[i];
  m->opt_t0 = m->h_next;
  return SMX_OK;
}

int smx_get_optimizer(const smx_model* m, int32_t* rule, float* hp, int32_t* t0) {
  SMX_REQUIRE(m, "null model");
  if (rule) *rule = m->opt_rule;
  if (hp) for (int i = 0; i < SMX_OPT_MAX_HP; ++i) hp[i] = m->opt_hp[i];
  if (t0) *t0 = (int32_t)m->opt_t0;
  return SMX_OK;
}

int smx_train_step(smx_model* m, const int32_t* row_ids, int32_t batch, smx_metrics* out) {
  return smx_train_steps(m, row_ids, 1, batch, 0, out);
}
int smx_train_step_graph(smx_model* m, const int32_t* row_ids, int32_t batch, smx_metrics* out) {
  return smx_train_steps(m, row_ids, 1, batch, 1, out);
}

int smx_train_steps(smx_model* m, const int32_t* order, int32_t n_steps, int32_t batch, int use_graph, smx_metrics* out) {
  SMX_REQUIRE(m && n_steps > 0, "bad arguments");
  SMX_REQUIRE(batch > 0 && batch <= m->Bmax, "batch must be in 1..max_batch");
  SMX_CHECK(smx::check_draws(m));
  if (order) {
    SMX_CHECK(check_rows(m, order, (size_t)n_steps * batch));
    const std::vector<int32_t> tiled = smx::tile_draws(m, order, n_steps, batch);
    SMX_CHECK(upload_order(m, tiled.empty() ? order : tiled.data(), (size_t)n_steps * batch * m->train_draws, (size_t)n_steps));
  } else {
    SMX_REQUIRE(m->staged_steps == n_steps && m->staged_batch == batch && m->staged_draws == m->train_draws,
              "order = NULL: no ids staged for this n_steps x batch (smx_train_stage) and draw count");
  }
  m->staged_steps = 0;   // (staged ids serve one call)
  // flag opt_shard: the heads' Adam moments outside this rank's slice are stale.  Steps that will NOT take the sharded chain (a captured graph,
  // the flag switched off since) update every element from its moments: gather them first (a collective -- every rank takes the same branch:
  // the flag, the communicator and use_graph are the job's, not a rank's)
  if (m->opt_stale && (use_graph || !(m->flags.opt_shard && smx::dp_chain_ok(m) && smx::dp_shard_available(m)))) SMX_CHECK(smx_opt_gather(m));
  int rc = SMX_OK;
  ++m->params_epoch;   // (the parameters are about to change)
  smx::DrawCaps caps(m);
  m->lazy_steps = 0;
  m->seam_steps = 0; m->seam_epochs = 0;   // (the seam's counter counts within this call: its first step that takes the form zeroes it)
  for (int s = 0; s < n_steps && rc == SMX_OK; ++s) rc = launch_train(m, batch * m->train_draws, use_graph != 0, s, n_steps);
  { const int rf = smx::lazy_flush(m); if (rc == SMX_OK) rc = rf; }   // (nothing is pending here: the call's last step keeps its optimiser launch)
  { const int rj = smx::head_sweep_join(m); if (rc == SMX_OK) rc = rj; }   // every other entry point sees one stream
  if (rc != SMX_OK) return rc;
  if (m->use_injected) { m->use_injected = false; }
  // a non-finite loss / gradient norm is REPORTED (out->nan_flag), not an error of the call: terminate_on_nan
  // (configs/base.yaml:59) is the caller's decision
  SMX_CHECK(read_metrics(m, out));
  return SMX_OK;
}

int smx_train_stage(smx_model* m, const int32_t* order, int32_t n_steps, int32_t batch) {
  SMX_REQUIRE(m && order && n_steps > 0, "bad arguments");
  SMX_REQUIRE(batch > 0 && batch <= m->Bmax, "batch must be in 1..max_batch");
  SMX_CHECK(smx::check_draws(m));
  SMX_CHECK(check_rows(m, order, (size_t)n_steps * batch));
  const std::vector<int32_t> tiled = smx::tile_draws(m, order, n_steps, batch);
  SMX_CHECK(upload_order(m, tiled.empty() ? order : tiled.data(), (size_t)n_steps * batch * m->train_draws, (size_t)n_steps));
  m->staged_steps = n_steps; m->staged_batch = batch; m->staged_draws = m->train_draws;
  return SMX_OK;
}

int smx_metrics_history(smx_model* m, int32_t n_steps, float* host) {
  SMX_REQUIRE(m && host && n_steps > 0 && n_steps <= m->mhist_steps, "no such history (steps of the last smx_train_steps call)");
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_CHECK(smx::seam_error_check(m));
  SMX_HIP(hipMemcpy(host, m->mhist, (size_t)n_steps * 8 * sizeof(float), hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_eval_step(smx_model* m, const int32_t* row_ids, int32_t batch, smx_metrics* out) {
  SMX_REQUIRE(m && row_ids, "bad arguments");
  SMX_CHECK(smx::check_draws(m));
  Pass ps;
  smx::DrawCaps caps(m);
  if (m->train_draws > 1) {   // the same draws as training, in eval mode: draw s of every cell keyed by sample index s
    SMX_REQUIRE(batch > 0 && batch <= m->Bmax, "batch must be in 1..max_batch");
    SMX_CHECK(check_rows(m, row_ids, (size_t)batch));
    const std::vector<int32_t> tiled = smx::tile_draws(m, row_ids, 1, batch);
    SMX_CHECK(setup_pass(m, ps, {tiled.data(), {}, nullptr}, batch * m->train_draws, 0, 0, batch));
    SMX_HIP(hipStreamSynchronize(m->st));   // (the row ids went from `tiled`, a host vector about to go)
  } else {
    SMX_CHECK(setup_pass(m, ps, {row_ids, {}, nullptr}, batch, 0, 0));
  }
  SMX_CHECK(forward_pass(m, ps, Loss::Eval));
  SMX_CHECK(read_metrics(m, out));
  return SMX_OK;
}

}  // extern "C"
