// smx_forward.hip -- the forward pass of a training / evaluation step as a launch sequence: encoders, latent draw, decoder, output and label heads,
// losses, ELBO scalars; the FactorVAE discriminator's forward.
#include "smx_model.h"

namespace smx {

// shapes / modes under which the decoder's first BatchNorm launch takes the latent sample and its product along
// (forward_pass adds what depends on injected noise)
static bool front_shapes_ok(smx_model* m, const Pass& ps) {
  const int lat_ld = m->lat_planes * m->Dp;
  return m->flags.front && !m->scale && !m->mixpost && !m->latent_tril && !sync_bn_on(m, ps.training) && bn_front_supported(ps.B, m->Dp) &&
         (m->Dp == 32 || m->Dp == 64) && m->dec[0].in_p == m->Dp && m->dec[0].out_p % 8 == 0 && (lat_ld % 4) == 0 &&
         m->dec[0].act == SMX_ACT_RELU;   // (the front forms build ReLU in)
}

// twin: another MLP whose FIRST layer consumes the same input (scvi: the library encoder beside the encoder).  When the
// shapes allow, both first layers run as ONE product launch and ONE BatchNorm launch (side by side along the output
// columns); *twin_done tells the caller, who then continues the twin from its second layer (first_layer = 1).
struct MlpFwdOpts {
  const char* label = "";                   // Timed label of the first layer's product when it reads X
  const LatentArgs* front = nullptr;        // the first layer's BatchNorm launch draws the latent sample and forms the product itself
  int first_layer = 0;
  std::vector<MlpLayer>* twin = nullptr;
  bool* twin_done = nullptr;
};
static int mlp_forward(smx_model* m, std::vector<MlpLayer>& mlp, const Pass& ps, Mat in0, bool in_is_x, const MlpFwdOpts& o = MlpFwdOpts()) {
  const float* in = in0.p;
  int ld = in0.ld;
  const size_t nl = mlp.size();
  auto make_gemm = [&](MlpLayer& L, const float* a_in, int a_ld, bool first_x, float* slab) {
    GemmArgs g = dense_fwd({a_in, a_ld}, {P_(m, L.tW), (int)m->tensors[L.tW].ld}, slab, L.out_p, nullptr, ps.B, L.out_p, L.in_p);
    g.slab_stride = (long)ps.B * L.out_p;
    g.split_k = suggest_split_k(ps.B, L.out_p, L.in_p);
    if (first_x) x_gather(m, ps, g);
    return g;
  };
  auto make_bn = [&](MlpLayer& L, const float* slab, int eff, long slab_stride) {
    BnFwdArgs b;
    b.pre = slab; b.n_slabs = eff; b.slab_stride = slab_stride; b.ld = L.out_p;
    b.B = ps.B; b.H = L.out; b.Hp = L.out_p; b.batchnorm = L.bn >= 0; b.training = ps.training; b.leak = L.leak; b.act = L.act;
    if (L.bn >= 0) {
      b.gamma = P_(m, L.tGamma); b.beta = P_(m, L.tBeta);
      b.moving_mean = m->bn_moving + m->bn_off[L.bn]; b.moving_var = b.moving_mean + L.out_p;
      b.batch_mean = m->grads + m->tail_off_bn + m->bn_off[L.bn]; b.batch_var = b.batch_mean + L.out_p;
      b.update_moving = (m->world == 1);
      b.momentum = m->cfg.bn_momentum; b.eps = m->cfg.bn_eps;
    } else {
      b.bias = P_(m, L.tBias);
    }
    b.xhat = L.xhat; b.inv_std = L.inv_std; b.out = L.out_buf;
    b.drop_p = ps.training ? L.drop_p : 0.f;
    b.nk = make_key(m, L.stream, ps.sample, true);
    if (&mlp == &m->dec) b.nk.draw_rows = (uint32_t)ps.draw_rows;   // (decoder dropout: a stream of the draw side)
    b.rows = ps.rows; b.cell_base = ps.cell_base;
    if (const Injected* ij = inj(m, L.stream)) { b.inj_mask = ij->d; b.inj_ld = ij->ld; }
    return b;
  };
  if (o.twin_done) *o.twin_done = false;
  for (size_t i = (size_t)o.first_layer; i < nl; ++i) {
    if (i > 0 && i == (size_t)o.first_layer) { in = mlp[i - 1].out_buf; ld = mlp[i - 1].out_p; }
    MlpLayer& L = mlp[i];
    const TensorInfo& tw = m->tensors[L.tW];
    GemmArgs g = make_gemm(L, in, ld, i == 0 && in_is_x, m->slab);
    static const bool no_ahead = tuning_on("no_noise_ahead");
    const bool no_twin = !m->flags.twin;
    const bool sync = sync_bn_on(m, ps.training) && L.bn >= 0;
    // hidden -> hidden layers 32 / 64 / 128 wide: the BatchNorm launch stages the layer's INPUT tile [B][K] in LDS and forms its
    // own columns as dot products -- the same front the first decoder layer uses for the latent sample, here as a plain
    // copy (no product launch; the reference's default networks are [64, 64], configs/base.yaml:10-17)
    LatentArgs dense_la;
    const bool dense_front = m->flags.front && !sync && !(o.front != nullptr && i == 0) && !(i == 0 && in_is_x) && L.leak == 0.f && L.act == SMX_ACT_RELU &&
                             (L.in_p == 32 || L.in_p == 64 || (L.in_p == 128 && ps.B <= 128)) && bn_front_supported(ps.B, L.in_p) && L.out_p % 8 == 0 &&
                             (ld % 4) == 0;
    if (dense_front) {
      dense_la.stochastic = 0; dense_la.relu = 0; dense_la.training = ps.training;
      dense_la.lat = in; dense_la.ld = ld; dense_la.B = ps.B; dense_la.D = L.in; dense_la.Dp = L.in_p;
    }
    const LatentArgs* front_i = (o.front != nullptr && i == 0) ? o.front : (dense_front ? &dense_la : nullptr);
    const bool with_front = front_i != nullptr;   // the BatchNorm launch produces its own input (latent sample / input tile + product)
    int eff = 1;
    SMX_REQUIRE((size_t)std::max(g.split_k, 1) * (size_t)g.slab_stride <= m->slab_cap, "split-K slabs exceed the slab buffer");
    // ---- the twin's first layer beside this one: one product launch, one BatchNorm launch ----
    bool dual = false;
    GemmArgs g2;
    if (o.twin && i == 0 && !with_front && !sync && !no_twin && in_is_x && !o.twin->empty() && bn_dual_supported(ps.B) &&
        !(ps.training && m->cfg.input_dropout > 0.f) && (*o.twin)[0].in_p == L.in_p && L.leak == 0.f && (*o.twin)[0].leak == 0.f &&
        L.act == SMX_ACT_RELU && (*o.twin)[0].act == SMX_ACT_RELU) {
      MlpLayer& T = (*o.twin)[0];
      float* slab2 = m->slab + (size_t)std::max(g.split_k, 1) * (size_t)g.slab_stride;
      g2 = make_gemm(T, in, ld, true, slab2);
      dual = ((size_t)std::max(g.split_k, 1) * ((size_t)g.slab_stride + (size_t)g2.slab_stride) <= m->slab_cap);
    }
    // layers without BatchNorm and without dropout (the FactorVAE discriminator; plain autoencoders at evaluation): bias
    // and activation in the product's own store path -- no bias / activation launch
    const bool epi_act = m->flags.act_epilogue && !dual && !with_front && !sync && L.bn < 0 && !(ps.training && L.drop_p > 0.f) &&
                         g.split_k <= 1 && !m->use_injected && L.act == SMX_ACT_RELU;   // (other activations: the BatchNorm launch without BatchNorm)
    if (epi_act) {
      if (i == 0 && in_is_x) SMX_CHECK(lazy_flush(m));   // (this product reads the layer's bias: nothing may ride on it)
      g.bias = P_(m, L.tBias); g.act = 1; g.leak = L.leak; g.C = L.out_buf; g.ldc = L.out_p; g.split_k = 1;
      Timed t(m, (i == 0 && in_is_x) ? o.label : "gemm_mlp_fwd");
      // a deep contraction (the discriminator's 1000-wide layers): the direct-operand bf16 x 3 form (smx_dgemm.hip)
      if (b3_on(m, ps.B) && dgemm_supported(g) && !tuning_on("no_dgemm")) SMX_CHECK(launch_dgemm(m->st, g));
      else SMX_CHECK(launch_gemm(m->st, g));
      in = L.out_buf; ld = L.out_p;
      continue;
    }
    // wide panel (the bf16 x 3 regime): the first layer's product as one workgroup per K slice + a reduce launch (smx_bigk.hip)
    bool bigk = false;
    BigKArgs bk;
    if (i == 0 && in_is_x && !dual && !with_front && m->bigk_part && !g.xf.drop_p && !g.xf.inj_mask && L.out_p <= 128 &&
        b3_on(m, ps.B) && !tuning_on("no_bigk")) {
      bk.A = in; bk.lda = ld; bk.a_u16 = ps.x_u16; bk.log1p = m->cfg.log_norm; bk.rows = ps.xrows;
      bk.Bm = P_(m, L.tW); bk.ldb = tw.ld; bk.b_kmajor = 1;
      bk.M = ps.B; bk.N = L.out_p; bk.K = L.in_p; bk.ldc = L.out_p; bk.slab_stride = (long)ps.B * L.out_p;
      bk.part = m->bigk_part; bk.out = m->slab;
      bk.n_slices = bigk_slices(bk.K, SMX_BIGK_MAX_SLICES, &bk.k_chunk);
      bigk = bk.log1p && bigk_supported(bk) && (size_t)bk.n_slices * (size_t)bk.slab_stride <= m->bigk_floats;
      // ... and no reduce launch: column-major slabs, summed by the BatchNorm launch (bn_wide_fwd_kernel)
      if (bigk && !sync && bn_wide_supported(ps.B, L.out_p, bk.n_slices) && (size_t)bk.n_slices * 128 * 128 <= m->bigk_floats) {
        bk.colmajor = 1; bk.slab_stride = 128L * 128;
      }
    }
    // the first product that reads X: the launch the lazy encoder update is built around (smx_step.hip).  Only the plain gathered form below
    // can apply the step before's pending update; before any other form it goes as the ordinary optimiser launch.
    const bool x_first = (i == 0 && in_is_x);
    const bool x_plain = x_first && &mlp == &m->enc && !bigk && !dual && !with_front;
    if (x_first && !x_plain) SMX_CHECK(lazy_flush(m));
    if (bigk) {
      Timed t(m, o.label);
      SMX_CHECK(launch_bigk(m->st, bk));
      eff = 1;
    } else if (dual) {
      Timed t(m, o.label);
      SMX_CHECK(launch_gemm_dual(m->st, g, g2, &eff));
    } else if (!with_front) {
      // the gathered first layer at up to 128 cells: its (at most 16) split-K slabs column-major, summed by a BatchNorm launch of one
      // workgroup per column -- every load 16 bytes of a contiguous 512-byte column instead of 4 bytes of a 32-byte row piece, the additions
      // in the same order (slab 0, 1, ...): the same bits (bn_wide_fwd_kernel)
      if (i == 0 && in_is_x && !sync && g.use_xform && g.tile == TILE_AUTO && g.split_k <= 16 && bn_wide_supported(ps.B, L.out_p, g.split_k) &&
          (size_t)g.split_k * 128 * (size_t)L.out_p <= m->slab_cap && !tuning_on("xf_tile")) {
        g.c_colmajor = 1; g.slab_stride = 128L * L.out_p;
      }
      // INVARIANT of the riding form: no workgroup of this launch writes anything a tile workgroup of this launch reads.  The tile workgroups
      // read X, the row ids, W_enc, its gradient, both its moments, its sum-of-squares slots and the pending step's state; they update W_enc in
      // registers and store slabs only.  The riders write parameters / moments / norms of every OTHER pending tensor -- none of them read here
      // (the product takes no bias: g.bias is null whenever the layer is split or has BatchNorm, and the bias epilogue form is flushed above).
      // W_enc's own chunks ride with the latent head's product (fwd_encoder), which reads neither W_enc nor its gradient; the gradient buffer is
      // rewritten only by this step's weight-gradient launch, later in stream order.
      GemmRide ride;
      const bool riding = x_plain && g.bias == nullptr && lazy_ride_tile(m, g, ride);
      if (x_first && !riding) SMX_CHECK(lazy_flush(m));
      Timed t(m, (i == 0 && in_is_x) ? o.label : "gemm_mlp_fwd");
      SMX_CHECK(launch_gemm(m->st, g, &eff, riding ? &ride : nullptr));
      if (riding) m->lazy_rest_pending = false;
      if (x_plain && ps.training && g.bias == nullptr && gemm_ride_tile_supported(g)) m->lazy_l1 = true;   // (the next step's product takes the same form)
    }
    BnFwdArgs b = make_bn(L, m->slab, eff, g.slab_stride);
    if (bigk && bk.colmajor) { b.pre = bk.part; b.n_slabs = bk.n_slices; b.slab_stride = bk.slab_stride; b.wide = 1; }
    else if (!bigk && !dual && !with_front && g.c_colmajor) b.wide = 1;
    if (!no_ahead && !sync && i == 0 && in_is_x && &mlp == &m->enc && ps.training && ps.draw_rows == 0 && front_shapes_ok(m, ps) &&
        !with_front && b.n_jobs == 0) {
      // the decoder's front launch (latent sample + first decoder layer) computes the whole latent tile in EVERY one of
      // its workgroups: its Philox draws (eps: ~1.2 us at batch 128, twice that at 256; dropout ~1 us) are made here
      // instead, once, by extra workgroups on CUs this launch leaves idle
      auto add = [&](float* dst, int ld, int width, int normal, float p, int stream) {
        NoiseJob& j = b.jobs[b.n_jobs++];
        j.dst = dst; j.ld = ld; j.width = width; j.normal = normal; j.p = p;
        j.stream = (uint32_t)((stream & 0xFF) | ((ps.sample & 0xFFFFFF) << 8));
      };
      const MlpLayer& d0 = m->dec[0];
      if (d0.drop_p > 0.f && !inj(m, d0.stream)) { add(d0.noise, d0.out_p, d0.out, 0, d0.drop_p, d0.stream); m->ahead_front_drop = true; }
      if (m->stochastic && !inj(m, ST_EPS_Z)) { add(m->noise_eps, m->Dp, m->D, 1, 0.f, ST_EPS_Z); m->ahead_front_eps = true; }
      if (b.n_jobs) b.nk.step_ptr = &cur_state(m)->step;
    }
    if (dual) {
      MlpLayer& T = (*o.twin)[0];
      const BnFwdArgs b2 = make_bn(T, g2.C, eff, g2.slab_stride);
      Timed t(m, "bn_fwd");
      SMX_CHECK(launch_bn_act_fwd_dual(m->st, b, b2));
      if (o.twin_done) *o.twin_done = true;
    } else if (with_front) {
      if (m->ahead_front_drop && o.front != nullptr && i == 0 && !b.inj_mask && b.drop_p > 0.f) { b.inj_mask = L.noise; b.inj_ld = L.out_p; }
      b.front = 1; b.lat = *front_i; b.W = P_(m, L.tW); b.ldw = tw.ld; b.n_jobs = 0;
      Timed t(m, "bn_fwd");
      SMX_CHECK(launch_bn_act_fwd(m->st, b));
    } else if (sync) {
      Timed t(m, "bn_fwd");
      b.n_jobs = 0;
      const BnSyncArgs y = sync_args(m);
      SMX_REQUIRE((size_t)y.world * 2 * L.out_p <= m->sync_cap, "SyncBatchNorm buffer too small");
      SMX_CHECK(launch_bn_sync_fwd(m->st, b, y, 0));
      SMX_CHECK(dp_allreduce_buf(m, m->sync_buf, (size_t)y.world * 2 * L.out_p, m->st));
      SMX_CHECK(launch_bn_sync_fwd(m->st, b, y, 1));
    } else {
      Timed t(m, "bn_fwd");
      SMX_CHECK(launch_bn_act_fwd(m->st, b));
    }
    in = L.out_buf; ld = L.out_p;
  }
  return SMX_OK;
}

// Training steps of the count heads with raw parameter planes (VAE / DCA / SISUA): output product + likelihood +
// dP in ONE wide kernel, P never materialised (smx_headloss.hip).  SMX_NO_HEAD_LOSS=1 keeps the product / loss
// kernel pair (what eval, predict and the scoring paths always use).
bool use_head_loss(const smx_model* m, int B) {
  if (!m->flags.head_loss || m->scvi || m->dec.empty() || m->k < 2) return false;   // (k = 1: the 'mse' output, product + loss kernel pair)
  return head_loss_supported(B, m->dec.back().out_p, m->Gp);
}

// Whether a training step of B cells takes the ONE-launch output head (smx_headfused.hip): the one predicate behind forward_pass's
// choice and smx_head_fused_bytes (two copies of it had drifted apart).  flags.head_bwd is part of it: the fused launch
// never stores dP, so the separate-launch backward forms (head_bwd = 0) cannot follow it.  Label heads do not stand in the way since
// round 5: their products run as the grouped launch of the backward pass (they cannot ride with a head launch that is not there).
// ... the launch's d d as column-major slabs that the decoder's BatchNorm-backward launch sums itself (no reduce launch, nothing in m->slab): at most 128
// cells, no label slabs beside them, no SyncBatchNorm on that layer
static bool head_fused_wide_dd(const smx_model* m, int B, bool training) {
  const MlpLayer& dL = m->dec.back();
  return m->n_heads == 0 && !(sync_bn_on(m, training) && dL.bn >= 0) && bn_wide_supported(B, dL.out_p, head_fused_grid(m->Gp)) &&
         (size_t)head_fused_grid(m->Gp) * 128 * 128 <= m->bigk_floats;
}
bool head_fused_ok(const smx_model* m, int B) {
  if (!use_head_loss(m, B) || !m->flags.head_fused || !m->flags.head_bwd || !m->hf_tab || !m->bigk_part) return false;
  // FactorVAE (round 6): the discriminator's passes use m->slab between the head's launch and the decoder's backward -- fine where the head's d d
  // does not live there (the column-major slab form); with an observed output beside the genes (its d d arrives as a further slab) the separate launches stay
  if (m->fvae && !head_fused_wide_dd(m, B, true)) return false;
  if (m->k > 3 || !m->out_has_W[1] || (m->k == 3 && !m->out_has_W[2])) return false;
  const MlpLayer& dL = m->dec.back();
  const TensorInfo& tw = m->tensors[m->t_outW[0]];
  return b3_on(m, B) && dL.out_p == 128 && tw.ld == (long)m->k * m->Gp && head_fused_supported(B, dL.out_p, m->Gp, m->k) && head_bwd_supported(B, dL.out_p, m->Gp) &&
         (size_t)head_fused_grid(m->Gp) * (size_t)B * 128 <= m->bigk_floats;
}

// arguments of the row-local scvi head launch of a training step; returns whether that launch applies
// (out == nullptr: only the test)
static bool scvi_train_args(smx_model* m, const Pass& ps, ScviTrainArgs* out) {
  const smx_config& c = m->cfg;
  if (!m->scvi || !m->flags.scvi_fused || m->encl.empty()) return false;
  const MlpLayer& lL = m->encl.back();
  const TensorInfo& twl = m->tensors[m->t_latlW];
  ScviTrainArgs a;
  const long ldp = (long)m->k * m->Gp;
  a.raw = m->raw; a.ld = ldp; a.plane_stride = m->Gp; a.B = ps.B; a.G = m->G; a.Gp = m->Gp; a.likelihood = c.likelihood;
  a.X = ps.Xsrc; a.ldx = m->Gp; a.x_u16 = ps.x_u16; a.rows = ps.rows; a.x_identity = (ps.rows != nullptr && ps.xrows == nullptr) ? 1 : 0;
  a.clip_library = c.clip_library; a.grad_scale = -1.f / (float)ps.global_batch;
  a.draw = m->draw; a.llk_part = m->llk_part;
  a.hl = lL.out_buf; a.ldh = lL.out_p; a.Kl = lL.out_p;
  a.Wl = P_(m, m->t_latlW); a.ldwl = twl.ld; a.bl = P_(m, m->t_latlb);
  a.library = ps.lib; a.cell_base = ps.cell_base;
  a.nk = draw_key(m, ST_EPS_L, ps);
  if (const Injected* ij = inj(m, ST_EPS_L)) { a.inj_eps = ij->d; a.inj_ld = ij->ld; }
  a.klw = kl_weight(m, ps, (float)ps.global_batch, 1);
  a.latl = m->latlbuf; a.ldl = 32; a.l = m->lsmp; a.sig = m->lsig; a.eps = m->leps; a.kl = m->kl_l;
  a.dlatl = m->dlatl; a.dl = m->dl;
  if (!scvi_head_train_supported(a)) return false;
  if (out) *out = a;
  return true;
}

// ---- forward_pass: its stages in launch order; FwdPass is what crosses their boundaries ----
struct FwdPass {
  Fwd mode = Fwd::Full;
  bool with_loss = false, backward = false;
  float inv_gb = 0.f;
  bool twin_done = false;                      // the library encoder's first layer ran beside the encoder's
  bool front_ok = false; LatentArgs front_la;  // the decoder's first BatchNorm launch draws the latent sample itself
  int n_llk_chunks = 0;                        // partial sums per cell left by the likelihood launch
};

// ---- encoder, latent head ----
static int fwd_encoder(smx_model* m, const Pass& ps, FwdPass& f) {
  if (f.mode == Fwd::Resample) return SMX_OK;
  MlpFwdOpts o;
  o.label = "gemm_enc_fwd"; o.twin = m->scvi ? &m->encl : nullptr; o.twin_done = &f.twin_done;
  SMX_CHECK(mlp_forward(m, m->enc, ps, {ps.Xsrc, m->Gp}, true, o));
  m->encl_twinned = f.twin_done;
  const MlpLayer& eL = m->enc.back();
  const int lat_ld = m->lat_planes * m->Dp;
  const GemmArgs g = dense_fwd({eL.out_buf, eL.out_p}, {P_(m, m->t_latW), m->tensors[m->t_latW].ld}, m->latbuf, lat_ld, P_(m, m->t_latb), ps.B, lat_ld, eL.out_p);
  // W_enc's own chunks of the lazy encoder update (smx_step.hip): riders of this launch, which reads neither W_enc nor its gradient and leaves
  // most of the chip idle -- unless the step before ran the decoder's BatchNorm-backward launch as the head's dW carrier (dw_late_now is still
  // that step's, and this step takes the same form): that launch has rider slots and no riders, is longer than a chunk workgroup lives
  // (this one is not: it grew from 4.6 to 7.3 us under the tracer with them) and precedes the weight gradients too -- the chunks wait for
  // it (mlp_backward; knob lazy_w_fwd: here in any case)
  const bool lazy_w_late = m->lazy_w_pending && !m->lazy_rest_pending && m->dw_late_now && !tuning_on("lazy_w_fwd");
  GemmRide ride;
  const bool riding = !lazy_w_late && lazy_ride_w(m, ride);
  if (!riding && !lazy_w_late) SMX_CHECK(lazy_flush(m));
  Timed t(m, "gemm_lat_fwd");
  SMX_CHECK(launch_gemm(m->st, g, nullptr, riding ? &ride : nullptr));
  if (riding) m->lazy_w_pending = false;
  return SMX_OK;
}

// ---- latent draw: mixture posterior, full-covariance posterior, or the plain one (here or with the decoder); the SCALE prior ----
static int fwd_latent(smx_model* m, const Pass& ps, FwdPass& f) {
  const smx_config& c = m->cfg;
  const int lat_ld = m->lat_planes * m->Dp;
  const bool encode_only = f.mode == Fwd::EncodeOnly || f.mode == Fwd::EncodeRaw;
  if (m->mixpost) {   // SCALE read literally: the draw from the mixture-density posterior and its Monte-Carlo KL (never the fused front)
    MixLatArgs ma;
    ma.lat = m->latbuf; ma.ld = lat_ld; ma.B = ps.B; ma.D = m->D; ma.Dp = m->Dp; ma.C = c.n_components;
    latent_noise(m, ps, ma); ma.nk_pick = draw_key(m, ST_MIX_PICK, ps);
    ma.z = m->z; ma.eps = m->eps; ma.zmean = m->zmean; ma.zstd = m->sig; ma.kl = m->kl; ma.resp = m->resp; ma.pick = m->zpick;
    Timed t(m, "latent_fwd");
    SMX_CHECK(launch_mixlat_fwd(m->st, ma));
  }
  if (m->latent_tril) {   // RVmeta(D, 'mvntril'): z = mu + L eps and the analytic KL (never the fused front); evaluation passes keep the factor
    LatentTrilArgs ta;
    ta.lat = m->latbuf; ta.ld = lat_ld; ta.B = ps.B; ta.D = m->D; ta.Dp = m->Dp;
    latent_noise(m, ps, ta);
    ta.z = m->z; ta.diag = m->sig; ta.eps = m->eps; ta.kl = m->kl; ta.factor = ps.training ? nullptr : m->ltril;
    Timed t(m, "latent_fwd");
    SMX_CHECK(launch_latent_tril_fwd(m->st, ta));
  }
  LatentArgs la;
  la.stochastic = m->stochastic; la.relu = (c.latent_activation == SMX_ACT_RELU); la.training = ps.training;
  la.lat = m->latbuf; la.ld = lat_ld; la.B = ps.B; la.D = m->D; la.Dp = m->Dp;
  latent_noise(m, ps, la);
  if (m->ahead_front_eps && !la.inj_eps) { la.inj_eps = m->noise_eps; la.inj_ld = m->Dp; }
  la.z = m->z; la.sig = m->sig; la.eps = m->eps; la.kl = m->kl;
  // The latent sample + KL and the first decoder product run INSIDE the decoder's first BatchNorm launch (two
  // launches fewer) when the shapes allow; SMX_NO_FRONT=1 keeps the three-launch form.
  f.front_ok = !encode_only && front_shapes_ok(m, ps) && (!la.inj_eps || (la.inj_ld % 4) == 0);
  f.front_la = la;
  if (f.front_ok || m->mixpost || m->latent_tril) {
    // (launched below with the decoder / drawn above)
  } else if (f.mode == Fwd::EncodeRaw && !m->scale) {
    // (the stacked scoring pass draws from the head's raw output itself: sigma, z and the KL of draw 0 would be a launch nobody reads)
  } else {
    Timed t(m, "latent_fwd");
    SMX_CHECK(launch_latent_fwd(m->st, la));
  }
  if (m->scale) {   // Monte-Carlo KL against the mixture prior at the z just drawn (overwrites the analytic KL)
    ScalePriorArgs sp;
    sp.z = m->z; sp.sig = m->sig; sp.eps = m->eps; sp.B = ps.B; sp.D = m->D; sp.Dp = m->Dp; sp.C = c.n_components;
    sp.logits = P_(m, m->t_prLogits); sp.loc = P_(m, m->t_prLoc); sp.scale_raw = P_(m, m->t_prScale);
    sp.kl = m->kl; sp.resp = m->resp; sp.dklz = m->dklz; sp.tril = m->scale_tril;
    SMX_CHECK(launch_scale_prior_fwd(m->st, sp));
  }
  return SMX_OK;
}

// ---- scvi library latent ----
static int fwd_library(smx_model* m, const Pass& ps, FwdPass& f) {
  const bool resample = f.mode == Fwd::Resample;
  if (!resample) {
    MlpFwdOpts o;
    o.label = "gemm_encl_fwd"; o.first_layer = f.twin_done ? 1 : 0;
    SMX_CHECK(mlp_forward(m, m->encl, ps, {ps.Xsrc, m->Gp}, true, o));
  }
  // training step: the library latent (its head as dot products, the sample, KL_l) is part of the row-local head
  // launch below (smx_scvi.hip); otherwise the product + lib_latent_fwd pair
  m->scvi_fused = f.backward && f.mode == Fwd::Full && scvi_train_args(m, ps, nullptr);
  if (m->scvi_fused) return SMX_OK;
  if (!resample) {
    const MlpLayer& lL = m->encl.back();
    SMX_CHECK(launch_gemm(m->st, dense_fwd({lL.out_buf, lL.out_p}, {P_(m, m->t_latlW), m->tensors[m->t_latlW].ld}, m->latlbuf, 32, P_(m, m->t_latlb), ps.B, 32, lL.out_p)));
  }
  LibLatentArgs ll;
  ll.latl = m->latlbuf; ll.ld = 32; ll.B = ps.B; ll.library = ps.lib; ll.rows = ps.rows; ll.cell_base = ps.cell_base;
  ll.nk = draw_key(m, ST_EPS_L, ps);
  if (const Injected* ij = inj(m, ST_EPS_L)) { ll.inj_eps = ij->d; ll.inj_ld = ij->ld; }
  ll.clip_library = m->cfg.clip_library;
  ll.l = m->lsmp; ll.sig = m->lsig; ll.eps = m->leps; ll.kl = m->kl_l;
  SMX_CHECK(launch_lib_latent_fwd(m->st, ll));
  return SMX_OK;
}

// ---- output head: the products of its planes (scvi: with the row-local head behind them), unless the likelihood launch forms them itself ----
static int fwd_out_head(smx_model* m, const Pass& ps, FwdPass& f) {
  const Mat D{m->dec.back().out_buf, m->dec.back().out_p};
  const long ldp = (long)m->k * m->Gp;
  if (!m->scvi) {
    m->head_loss = f.backward && use_head_loss(m, ps.B);
    if (m->head_loss) return SMX_OK;   // the product runs below, fused with the likelihood
    const GemmArgs g = dense_fwd(D, {P_(m, m->t_outW[0]), m->tensors[m->t_outW[0]].ld}, m->P, (int)ldp, P_(m, m->t_outb[0]), ps.B, (int)ldp, D.ld);
    Timed t(m, "gemm_out_fwd");
    SMX_CHECK(launch_gemm(m->st, g));
    return SMX_OK;
  }
  GemmArgs hg[3];
  int n_hg = 0;
  for (int ch = 0; ch < m->k; ++ch) {
    if (!m->out_has_W[ch]) {   // dispersion / inflation = 'share' (scvi.py:66-86): the per-gene vector in every row of the raw plane
      SMX_CHECK(launch_plane_fill(m->st, m->raw + (long)ch * m->Gp, ldp, P_(m, m->t_outb[ch]), ps.B, m->Gp, m->out_single[ch] ? 1 : 0));
      continue;
    }
    hg[n_hg++] = dense_fwd(D, {P_(m, m->t_outW[ch]), m->tensors[m->t_outW[ch]].ld}, m->raw + (long)ch * m->Gp, (int)ldp, P_(m, m->t_outb[ch]), ps.B, m->Gp, D.ld);
  }
  {
    // the heads read the same decoder output: pairs of them side by side in one launch
    const bool no_twin = !m->flags.twin;
    Timed t(m, "gemm_out_fwd");
    int ch = 0;
    for (; !no_twin && ch + 1 < n_hg; ch += 2) SMX_CHECK(launch_gemm_dual(m->st, hg[ch], hg[ch + 1]));
    for (; ch < n_hg; ++ch) SMX_CHECK(launch_gemm(m->st, hg[ch]));
  }
  if (!m->scvi_fused) return launch_scvi_head_fwd(m->st, scvi_head_args(m, ps));
  ScviTrainArgs st;
  scvi_train_args(m, ps, &st);
  // (timing mode: the idempotent launch repeated inside one event pair, as for the other likelihood kernels)
  const int reps = (!m->capturing && m->timing_label == "loss") ? m->timing_reps : 1;
  Timed t(m, "loss");
  for (int r = 0; r < reps; ++r) SMX_CHECK(launch_scvi_head_train(m->st, st));
  return SMX_OK;
}

// ---- label heads (raw outputs) ----
static int fwd_label_heads(smx_model* m, const Pass& ps) {
  const MlpLayer& dL = m->dec.back();
  for (int j = 0; j < m->n_heads; ++j) {
    const int ld = (int)m->tensors[m->t_labW[j]].ld;
    SMX_CHECK(launch_gemm(m->st, dense_fwd({dL.out_buf, dL.out_p}, {P_(m, m->t_labW[j]), ld}, m->laby_raw[j], ld, P_(m, m->t_labb[j]), ps.B, ld, dL.out_p)));
  }
  return SMX_OK;
}

// ---- losses ----
// a wide panel: the whole head -- product, likelihood, dW / db and the per-workgroup slabs of d d -- in ONE launch + the ordered
// sum of the slabs (smx_headfused.hip); backward_pass then finds its head products done
static int fwd_head_fused(smx_model* m, const Pass& ps, FwdPass& f, const HeadLossArgs& hl) {
  const MlpLayer& dL = m->dec.back();
  HeadFusedArgs hf;
  hf.D = dL.out_buf; hf.ldd = dL.out_p; hf.W = hl.W; hf.ldw = hl.ldw; hf.bias = hl.bias;
  hf.X = ps.Xsrc; hf.ldx = m->Gp; hf.rows = ps.xrows; hf.x_u16 = ps.x_u16;
  hf.dW = G_(m, m->t_outW[0]); hf.db = G_(m, m->t_outb[0]);
  hf.part = m->bigk_part; hf.slab_stride = (long)ps.B * dL.out_p; hf.llk_part = m->llk_part;
  // without label heads (their d d arrives as further slabs) the decoder's BatchNorm-backward launch sums the workgroups' slabs itself
  const bool wide_dd = head_fused_wide_dd(m, ps.B, ps.training != 0);
  if (wide_dd) { hf.part_colmajor = 1; hf.slab_stride = 128L * 128; }
  hf.sq_part = sq_part_of(m, m->t_outW[0]);
  hf.dtab = m->hf_tab;
  hf.B = ps.B; hf.G = m->G; hf.Gp = m->Gp; hf.likelihood = m->cfg.likelihood; hf.grad_scale = -f.inv_gb;
  const int reps = (!m->capturing && m->timing_label == "out_head") ? m->timing_reps : 1;   // idempotent
  int n_slabs = 0;
  // this step's update of the heads: a sweep on the second stream, started behind this launch -- its event is the launch's own completion
  // signal (no marker packet for the stream's next launch to wait behind; knob no_hf_ext_event: hipEventRecord)
  const bool sweep_ev = hf.sq_part && head_sweep_ok(m);
  const bool ext_ev = sweep_ev && reps == 1 && !tuning_on("no_hf_ext_event");
  if (sweep_ev) SMX_CHECK(head_sweep_prepare(m));
  {
    Timed t(m, "out_head");
    for (int r = 0; r < reps; ++r) SMX_CHECK(launch_head_fused(m->st, hf, &n_slabs, &m->head_fused_sq, ext_ev ? m->ev_hf : nullptr));
  }
  if (sweep_ev) {
    if (!ext_ev) SMX_HIP(hipEventRecord(m->ev_hf, m->st));
    m->ev_hf_fresh = true;
  }
  // data parallel, two buckets: without label heads every gradient of the head bucket is final HERE -- its chain (all-reduce, norms,
  // clip + Adam) runs beside the whole backward pass, the optimiser launch and the next step's encoder and decoder
  if (m->n_heads == 0 && dp_chain_ok(m)) SMX_CHECK(dp_chain_start(m));
  m->wide_dd_slabs = wide_dd ? n_slabs : 0; m->wide_dd_src = m->bigk_part; m->wide_dd_stride = hf.slab_stride;
  if (!wide_dd) SMX_CHECK(launch_head_fused_reduce(m->st, hf, n_slabs, m->slab));
  f.n_llk_chunks = head_fused_chunks(m->Gp);
  m->head_fused = true;
  return SMX_OK;
}

// training steps of the count heads with raw planes: the output product fused with the likelihood, or the whole head in one launch
static int fwd_head_loss(smx_model* m, const Pass& ps, FwdPass& f) {
  const MlpLayer& dL = m->dec.back();
  HeadLossArgs hl;
  hl.H = dL.out_buf; hl.ldh = dL.out_p; hl.W = P_(m, m->t_outW[0]); hl.ldw = m->tensors[m->t_outW[0]].ld; hl.bias = P_(m, m->t_outb[0]);
  hl.X = ps.Xsrc; hl.x_u16 = ps.x_u16; hl.ldx = m->Gp; hl.rows = ps.xrows;
  hl.dP = m->dP; hl.ldp = (long)m->k * m->Gp; hl.plane_stride = m->Gp; hl.llk_part = m->llk_part;
  hl.B = ps.B; hl.G = m->G; hl.Gp = m->Gp; hl.Hp = dL.out_p; hl.likelihood = m->cfg.likelihood; hl.grad_scale = -f.inv_gb;
  hl.bf16x3 = b3_on(m, ps.B) ? 1 : 0;
  f.n_llk_chunks = head_loss_chunks(m->Gp);
  const bool product_timing = !m->capturing && m->timing_label == "out_head_product";
  if (head_fused_ok(m, ps.B) && !product_timing) return fwd_head_fused(m, ps, f, hl);
  if (product_timing) {
    // timing mode: the product alone (P stored, no counts, no likelihood) -- what the fused kernel's time is
    // compared with to attribute the rest to the likelihood (bench.py, roofline)
    HeadLossArgs po = hl;
    po.product_only = 1; po.dP = m->P;
    Timed t(m, "out_head_product");
    for (int r = 0; r < m->timing_reps; ++r) SMX_CHECK(launch_out_head_loss(m->st, po));
  }
  const int reps = (!m->capturing && m->timing_label == "out_head") ? m->timing_reps : 1;   // idempotent
  Timed t(m, "out_head");
  for (int r = 0; r < reps; ++r) SMX_CHECK(launch_out_head_loss(m->st, hl));
  return SMX_OK;
}

// the likelihood of the gene output: with the scvi head's launch above, with the output product, or from the planes in m->P
static int fwd_gene_loss(smx_model* m, const Pass& ps, FwdPass& f) {
  f.n_llk_chunks = loss_chunks(m->Gp, ps.B);
  if (m->scvi && m->scvi_fused) { f.n_llk_chunks = 1; return SMX_OK; }   // the row-local head launch left one partial per cell
  if (m->head_loss) return fwd_head_loss(m, ps, f);
  LossArgs lo;
  lo.likelihood = m->cfg.likelihood; lo.direct = m->scvi; lo.backward = f.backward;
  lo.X = ps.Xsrc; lo.x_u16 = ps.x_u16; lo.ldx = m->Gp; lo.rows = ps.xrows;
  lo.P = m->P; lo.ldp = (long)m->k * m->Gp; lo.plane_stride = m->Gp; lo.dP = m->dP; lo.llk_part = m->llk_part;
  lo.B = ps.B; lo.G = m->G; lo.Gp = m->Gp; lo.grad_scale = -f.inv_gb;
  // timing mode: the (idempotent) kernel is launched SMX_LOSS_TIMING_REPEAT times inside one event pair so
  // the pair's own ~5 us overhead can be separated from the per-launch time (bench.py)
  const int reps = (!m->capturing && m->timing_label == "loss") ? m->timing_reps : 1;
  Timed t(m, "loss");
  for (int r = 0; r < reps; ++r) SMX_CHECK(launch_count_loss(m->st, lo));
  return SMX_OK;
}

static int fwd_label_losses(smx_model* m, const Pass& ps, const FwdPass& f) {
  const smx_config& c = m->cfg;
  for (int j = 0; j < m->n_heads; ++j) {
    const TensorInfo& tw = m->tensors[m->t_labW[j]];
    LabelArgs lb;
    lb.kind = c.label_llk[j]; lb.C = c.label_components[j]; lb.raw = m->laby_raw[j]; lb.ld = tw.ld; lb.Y = m->Y[j]; lb.ldy = m->lab_Pp[j];
    lb.rows = ps.rows; lb.mask = m->mask; lb.B = ps.B; lb.P = c.label_dim[j]; lb.Pp = m->lab_Pp[j];
    // an observed output variable (outputs[1:]): weight 1, every cell, its own accumulator; a label variable: alpha, the label mask
    const bool obs = j < m->n_observed;
    lb.observed = obs ? 1 : 0;
    lb.grad_scale = obs ? -f.inv_gb : -c.alpha * f.inv_gb; lb.draw = m->laby_draw[j];
    lb.llk = obs ? m->llk_o : m->llk_y; lb.add = obs ? (j > 0) : (j > m->n_observed);
    lb.backward = f.backward;
    SMX_CHECK(launch_label_loss(m->st, lb));
  }
  return SMX_OK;
}

// ---- the ELBO scalars: launched here, or handed to a later launch of the training step ----
static int fwd_metrics(smx_model* m, const Pass& ps, const FwdPass& f) {
  const smx_config& c = m->cfg;
  MetricsArgs me;
  me.llk_part = m->llk_part; me.n_chunks = f.n_llk_chunks; me.rows = ps.rows;
  me.lgx1 = llk_has_count_const(c.likelihood) ? ps.lgx1 : nullptr;   // (the count likelihoods' data-only constant sum_g lgamma(x + 1); not 'mse' / 'bernoulli' / 'normal')
  me.llk_y = c.n_labels > m->n_observed ? m->llk_y : nullptr;
  me.llk_o = m->n_observed ? m->llk_o : nullptr;
  if (m->fvae) { me.tc = m->tc_cell; me.dl = m->dl_cell; me.gamma = c.gamma; }
  me.kl = m->stochastic ? m->kl : nullptr; me.kl_l = m->scvi ? m->kl_l : nullptr;
  me.B = ps.B; me.alpha = c.alpha; me.inv_global_batch = f.inv_gb;
  { const KlWeight w = kl_weight(m, ps, f.inv_gb, 0); me.beta = w.beta; me.beta_ptr = w.beta_ptr; }
  me.out = m->grads + m->tail_off_metrics;
  if (f.backward && !dp_active(m)) { me.hist = m->mhist; me.state = cur_state(m); }
  if (f.backward) {
    // training step: the scalars come from one extra workgroup of a later launch -- of the optimiser kernel, or,
    // under data parallelism (they must be in the flat buffer BEFORE the all-reduce), of the first
    // BatchNorm-backward launch
    m->pending_metrics = me;
    m->have_pending_metrics = true;
    m->metrics_before_allreduce = dp_active(m);
    return SMX_OK;
  }
  Timed t(m, "metrics");
  SMX_CHECK(launch_metrics(m->st, me));
  return SMX_OK;
}

int forward_pass(smx_model* m, const Pass& ps, Loss loss, Fwd mode) {
  FwdPass f;
  f.mode = mode; f.with_loss = loss != Loss::None; f.backward = loss == Loss::Train; f.inv_gb = 1.f / (float)ps.global_batch;
  m->audit_rows = ps.B;
  m->head_loss = false; m->head_fused = false; m->ev_hf_fresh = false; m->wide_dd_slabs = 0;
  m->ahead_front_eps = m->ahead_front_drop = false;
  m->scvi_fused = false; m->encl_twinned = false;
  if (mode != Fwd::DecodeOnly) {
    SMX_CHECK(fwd_encoder(m, ps, f));
    SMX_CHECK(fwd_latent(m, ps, f));
    if (m->scvi) SMX_CHECK(fwd_library(m, ps, f));
  }
  if (mode == Fwd::EncodeOnly || mode == Fwd::EncodeRaw) return SMX_OK;
  MlpFwdOpts dec;
  dec.front = f.front_ok ? &f.front_la : nullptr;
  SMX_CHECK(mlp_forward(m, m->dec, ps, {m->z, m->Dp}, false, dec));
  SMX_CHECK(head_sweep_join(m));   // (the heads' update of the step before, if it is still under way on the second stream)
  SMX_CHECK(fwd_out_head(m, ps, f));
  SMX_CHECK(fwd_label_heads(m, ps));
  if (!f.with_loss) return SMX_OK;
  SMX_CHECK(fwd_gene_loss(m, ps, f));
  SMX_CHECK(fwd_label_losses(m, ps, f));
  if (m->fvae) SMX_CHECK(factor_forward(m, ps, f.backward));
  return fwd_metrics(m, ps, f);
}

// ---- FactorVAE discriminator (fvae.py:9-18; Kim & Mnih 2018, Algorithm 2) -------------------------------------------
// forward: stacked batch [z ; permute_dims(z)] through the discriminator, then the head (TC estimate, discriminator
// loss, SemiFVAE's cross-entropy, both upstream gradients).  Runs after the latent sample exists; m->slab is free then.
int factor_forward(smx_model* m, const Pass& ps, bool backward) {
  const smx_config& c = m->cfg;
  const int B = ps.B, B2 = 2 * ps.B;
  SMX_REQUIRE(B2 <= 2 * m->Bmax, "batch exceeds max_batch");
  m->audit_disc_rows = B2;
  PermuteArgs pa;
  pa.z = m->z; pa.ldz = m->Dp; pa.zz = m->zz; pa.ld = m->Dp; pa.B = B; pa.D = m->D;
  pa.nk = make_key(m, ST_PERMUTE, ps.sample, ps.training != 0);
  pa.rows = ps.rows; pa.cell_base = ps.cell_base;
  if (const Injected* ij = inj(m, ST_PERMUTE)) { pa.inj_u = ij->d; pa.inj_ld = ij->ld; }
  {
    Timed t(m, "disc_permute");
    SMX_CHECK(launch_permute_dims(m->st, pa));
  }
  Pass p2 = ps;
  p2.B = B2; p2.rows = nullptr; p2.training = 1;   // (no BatchNorm / dropout in the discriminator: the mode is immaterial)
  MlpFwdOpts o;
  o.label = "disc_fwd";
  SMX_CHECK(mlp_forward(m, m->disc, p2, {m->zz, m->Dp}, false, o));
  const MlpLayer& last = m->disc.back();
  const TensorInfo& tw = m->tensors[m->t_discoutW];
  GemmArgs g = dense_fwd({last.out_buf, last.out_p}, {P_(m, m->t_discoutW), tw.ld}, m->slab, tw.ld, nullptr, B2, tw.ld, last.out_p);
  g.slab_stride = (long)B2 * tw.ld;
  g.split_k = suggest_split_k(B2, tw.ld, last.out_p);
  SMX_REQUIRE((size_t)std::max(g.split_k, 1) * (size_t)g.slab_stride <= m->slab_cap, "split-K slabs exceed the slab buffer");
  int eff = 1;
  {
    Timed t(m, "disc_fwd");
    SMX_CHECK(launch_gemm(m->st, g, &eff));
  }
  DiscHeadArgs h;
  h.logits = m->slab; h.n_slabs = eff; h.slab_stride = g.slab_stride; h.ld = tw.ld;
  h.bias = P_(m, m->t_discoutb); h.n_out = tw.cols; h.B = B;
  h.gamma = c.gamma; h.alpha = c.alpha; h.inv_gb = 1.f / (float)ps.global_batch; h.backward = backward ? 1 : 0;
  const int jd = m->n_observed;   // SemiFVAE's label variable: behind the observed outputs in the target order
  const bool semi = c.n_labels > jd;
  if (semi && m->Y[jd] && ps.Xsrc == m->X) {   // (resident cells: their labels are; a pass over host data has none)
    for (int j = jd; j < c.n_labels; ++j) {
      h.Y[h.n_groups] = m->Y[j]; h.ldy[h.n_groups] = m->lab_Pp[j];
      h.gstart[h.n_groups + 1] = h.gstart[h.n_groups] + c.label_dim[j];
      ++h.n_groups;
    }
    h.rows = ps.rows; h.mask = m->mask;
  }
  h.u_tc = m->u_d + (size_t)2 * B * 32; h.u_d = m->u_d;   // (one buffer: rows [0, 2B) the discriminator's objective, [2B, 3B) the TC term)
  h.tc_cell = m->tc_cell; h.dl_cell = m->dl_cell; h.llk_y = semi ? m->llk_y : nullptr;
  Timed t(m, "disc_head");
  SMX_CHECK(launch_disc_head(m->st, h));
  return SMX_OK;
}

}  // namespace smx
