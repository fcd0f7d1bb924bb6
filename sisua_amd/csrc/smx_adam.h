// smx_adam.h -- the optimiser's workgroup body (per-tensor clipnorm + Adam, or the rule smx_set_optimizer chose, over one chunk of the
// flat buffer),
// shared by the optimiser launch (smx_adam.hip), by the launches that carry chunks as riders -- the BatchNorm-backward kernels
// (smx_bn.hip) and the latent head's backward product (smx_gemm.hip) -- and by the heads' background sweep on the second stream
// (adam_sweep_body; smx_backward.hip: head_sweep_*).  Also the bodies of the ELBO scalars and of the sum-of-squares reductions, which
// ride on the optimiser's and the BatchNorm-backward launches (metrics_body, sq_reduce_body).
#pragma once
#include "smx_device.h"
#include "smx_internal.h"

namespace smx {

typedef float smx_f32x4 __attribute__((ext_vector_type(4)));

// the chunk's tensor: its gradient norm (written once per tensor, by the tensor's first chunk) and the factor its gradients are scaled by.
// Every thread of the workgroup calls it (two barriers); the first 256 threads sum in the same order whatever NT is.
// (adam_tensor_clip_at: the tensor's slot range handed in -- a caller that knows its tensor on the host passes it as kernel arguments instead of
// indexing a.sq_count / a.sq_first by a value it would have to load first; the gathered encoder product's riding form, smx_gemm.hip)
template <int NT = 256, bool AT = true>
__device__ inline float adam_tensor_clip_at(const AdamArgs& a, const OptChunk& ch, int chunk, const int cnt_at, const int first_at) {
  __shared__ float sh[4];
  float s = 0.f;
  if (NT > 256 && threadIdx.x >= 256) {
  } else if (a.use_sq) {
    const int cnt = AT ? cnt_at : a.sq_count[ch.tensor];
    const int first = AT ? first_at : a.sq_first[ch.tensor];
    if (cnt > 0) {   // partial sums written by the weight-gradient product's workgroups
      // (a thread's slots eight at a time in flight -- unconditional loads from a clamped index, masked at the add, added in the same order
      // as one by one: same bits.  As a rider of a 5-10 us launch a workgroup's LIFE is what counts, and 7 dependent round trips for the
      // 1672 slots of the one-launch output head were most of it)
      const float* sl = a.sq_slots + first;
      for (int k0 = threadIdx.x; k0 < cnt; k0 += 8 * 256) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = sl[min(k0 + 256 * u, cnt - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k0 + 256 * u < cnt) s += q[u];
      }
    } else {         // small tensor (bias, BatchNorm scale / shift): sweep its whole gradient
      const float4* t4 = reinterpret_cast<const float4*>(a.grads + a.chunks[ch.first_chunk].offset);
      for (int k = threadIdx.x; k < ch.tensor_count / 4; k += 256) {
        const float4 q = t4[k];
        s += (q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w);
      }
    }
  } else {
    for (int k = threadIdx.x; k < ch.n_chunks; k += 256) s += a.partial[ch.first_chunk + k];
  }
  s = wave_sum(s);   // (the first four waves' sums, in block_sum's order; later waves stand by)
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x < 256) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  if (ch.tensor == a.tied_t0 || ch.tensor == a.tied_t1) s *= a.tied_inv;   // (C identical rows of one shared variable)
  const float norm = sqrtf(s) * a.grad_scale;
  float clip = a.grad_scale;
  if (a.clipnorm > 0.f && norm > a.clipnorm) clip *= a.clipnorm / norm;
  if (threadIdx.x == 0 && chunk == ch.first_chunk) a.tensor_norm[ch.tensor] = norm;
  return clip;
}
template <int NT = 256>
__device__ inline float adam_tensor_clip(const AdamArgs& a, const OptChunk& ch, int chunk) {
  return adam_tensor_clip_at<NT, false>(a, ch, chunk, 0, 0);
}

// one quad of a tensor: the update itself.  Every contraction is SPELLED: the launches that carry this body (optimiser, riders, sweep, the sharded
// chain) must give the same bits, and which multiply-adds the compiler fuses depends on the code around them (round 6: inlined into the output
// head's launch -- tools/dev/head_lazy_update.patch -- the unspelled form differed from the sweep's in the last bit of some elements).
__device__ inline void adam_apply4(float b1, float b2, float eps, float clip, float lr_t, const smx_f32x4& g, smx_f32x4& m, smx_f32x4& v, smx_f32x4& p) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float ge = g[e] * clip;
    m[e] = __builtin_fmaf(b1, m[e], (1.f - b1) * ge);
    v[e] = __builtin_fmaf(b2, v[e], ((1.f - b2) * ge) * ge);
    p[e] = __builtin_fmaf(-(lr_t * m[e]), frcp(fsqrt(v[e]) + eps), p[e]);   // v_sqrt + v_rcp (1 ulp each) instead of 22 instructions
  }
}
__device__ inline void adam_apply4(const AdamArgs& a, float clip, float lr_t, const smx_f32x4& g, smx_f32x4& m, smx_f32x4& v, smx_f32x4& p) {
  adam_apply4(a.b1, a.b2, a.eps, clip, lr_t, g, m, v, p);
}

// the other rules (smx_set_optimizer; the forms of TensorFlow's training ops): slot 2 = m, slot 3 = v as OptSlots
// say -- a rule reads and writes only the slots it uses.  Spelled like adam_apply4, for the same reason.
template <int F> struct OptSlots {
  static constexpr bool m = F == OPT_ADAM || F == OPT_SGD_MOM || F == OPT_SGD_NESTEROV || F == OPT_RMSPROP_MOM || F == OPT_ADAMAX;
  static constexpr bool v = F == OPT_ADAM || F == OPT_RMSPROP || F == OPT_RMSPROP_MOM || F == OPT_ADAGRAD || F == OPT_ADAMAX;
};
template <int F>
__device__ __attribute__((always_inline)) inline void opt_apply1(const AdamArgs& a, float lr_t, float ge, float& m, float& v, float& p) {
#pragma clang fp contract(off)
  const float b1 = a.b1, b2 = a.b2, eps = a.eps, mu = a.momentum;
  if constexpr (F == OPT_SGD) {                      // w -= lr g
    p = __builtin_fmaf(-lr_t, ge, p);
  } else if constexpr (F == OPT_SGD_MOM) {           // a = momentum a - lr g;  w += a
    m = __builtin_fmaf(mu, m, -(lr_t * ge));
    p = p + m;
  } else if constexpr (F == OPT_SGD_NESTEROV) {      // a = momentum a - lr g;  w += momentum a - lr g
    m = __builtin_fmaf(mu, m, -(lr_t * ge));
    p = p + __builtin_fmaf(mu, m, -(lr_t * ge));
  } else if constexpr (F == OPT_RMSPROP) {           // ms = rho ms + (1 - rho) g^2;  w -= lr g / (sqrt(ms) + eps)
    v = __builtin_fmaf(b1, v, ((1.f - b1) * ge) * ge);
    p = __builtin_fmaf(-(lr_t * ge), frcp(fsqrt(v) + eps), p);
  } else if constexpr (F == OPT_RMSPROP_MOM) {       // ms as above;  mom = momentum mom + lr g / sqrt(ms + eps);  w -= mom
    v = __builtin_fmaf(b1, v, ((1.f - b1) * ge) * ge);
    m = __builtin_fmaf(mu, m, (lr_t * ge) * frcp(fsqrt(v + eps)));
    p = p - m;
  } else if constexpr (F == OPT_ADAGRAD) {           // acc += g^2;  w -= lr g / (sqrt(acc) + eps)
    v = __builtin_fmaf(ge, ge, v);
    p = __builtin_fmaf(-(lr_t * ge), frcp(fsqrt(v) + eps), p);
  } else {                                           // Adamax: m = b1 m + (1 - b1) g;  u = max(b2 u, |g|);  w -= lr_t m / (u + eps)
    m = __builtin_fmaf(b1, m, (1.f - b1) * ge);
    v = fmaxf(b2 * v, fabsf(ge));
    p = __builtin_fmaf(-(lr_t * m), frcp(v + eps), p);
  }
}
template <int F>
__device__ __attribute__((always_inline)) inline void opt_apply4(const AdamArgs& a, float clip, float lr_t, const smx_f32x4& g, smx_f32x4& m, smx_f32x4& v, smx_f32x4& p) {
  if constexpr (F == OPT_ADAM) {
    adam_apply4(a, clip, lr_t, g, m, v, p);
  } else {   // (element by element with constant indices: a loop over a vector's elements left the vectors in scratch memory here)
    float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
    opt_apply1<F>(a, lr_t, g[0] * clip, m0, v0, p0);
    opt_apply1<F>(a, lr_t, g[1] * clip, m1, v1, p1);
    opt_apply1<F>(a, lr_t, g[2] * clip, m2, v2, p2);
    opt_apply1<F>(a, lr_t, g[3] * clip, m3, v3, p3);
    m = smx_f32x4{m0, m1, m2, m3}; v = smx_f32x4{v0, v1, v2, v3}; p = smx_f32x4{p0, p1, p2, p3};
  }
}

// CALL(F) for the chunk's rule F = a.form: the one branch a carrier takes per chunk (a.form is uniform over the launch).  ALL = false: Adam
// only -- the riders of the BatchNorm-backward and latent-head launches, and the Adam instantiations of the optimiser's own kernels, hold
// no code of the other rules (with it, the same Adam instructions ran 0.9 us per C2 step slower: DESIGN.md 4d)
#define SMX_OPT_SWITCH(ALL, form, CALL)                                                                                               \
  if constexpr (!(ALL)) {                                                                                                             \
    CALL(OPT_ADAM);                                                                                                                   \
  } else {                                                                                                                            \
    switch (form) {                                                                                                                   \
      case OPT_SGD: CALL(OPT_SGD); break;                                                                                             \
      case OPT_SGD_MOM: CALL(OPT_SGD_MOM); break;                                                                                     \
      case OPT_SGD_NESTEROV: CALL(OPT_SGD_NESTEROV); break;                                                                           \
      case OPT_RMSPROP: CALL(OPT_RMSPROP); break;                                                                                     \
      case OPT_RMSPROP_MOM: CALL(OPT_RMSPROP_MOM); break;                                                                             \
      case OPT_ADAGRAD: CALL(OPT_ADAGRAD); break;                                                                                     \
      case OPT_ADAMAX: CALL(OPT_ADAMAX); break;                                                                                       \
      default: CALL(OPT_ADAM); break;                                                                                                 \
    }                                                                                                                                 \
  }

// clip + Adam for one chunk of the flat buffer; NT = 256 threads, or 512 as a rider of a 512-thread launch (the tensor's norm is
// summed by the first 256 threads in the same order either way: both forms give the same bits).  A thread's first operands are
// requested BEFORE the norm is reduced and each later round's before the current round's arithmetic: a workgroup lives for 2-4
// rounds, so the reduction's barrier and the first loads' latency were a third of its life.  (Nontemporal loads / stores of the
// moments, to keep the weights in the last-level cache, measured slower: c5-shard 198.0 -> 200.0 us, C2 80.4 -> 81.7.)
// the element loop of a chunk under the rule F: under Adam a thread's next quads are requested before the current quad's arithmetic
template <int NT, int F>
__device__ __attribute__((always_inline)) inline void opt_chunk_loop(const AdamArgs& a, float clip, float lr_t, int i, int n4, const smx_f32x4* g4, smx_f32x4* m4, smx_f32x4* v4,
                                      smx_f32x4* p4, smx_f32x4 g, smx_f32x4 m, smx_f32x4 v, smx_f32x4 p) {
  constexpr bool UM = OptSlots<F>::m, UV = OptSlots<F>::v;
  if constexpr (F != OPT_ADAM) {   // (the other rules one quad at a time)
    for (; i < n4; i += NT) {
      if (UM) m = m4[i];
      if (UV) v = v4[i];
      p = p4[i];
      opt_apply4<F>(a, clip, lr_t, g4[i], m, v, p);
      if (UM) m4[i] = m;
      if (UV) v4[i] = v;
      p4[i] = p;
    }
    return;
  }
  while (i < n4) {
    const int j = i + NT;
    smx_f32x4 gn = g, mn = m, vn = v, pn = p;
    if (j < n4) { gn = g4[j]; if (UM) mn = m4[j]; if (UV) vn = v4[j]; pn = p4[j]; }
    opt_apply4<F>(a, clip, lr_t, g, m, v, p);
    if (UM) m4[i] = m;
    if (UV) v4[i] = v;
    p4[i] = p;
    g = gn; m = mn; v = vn; p = pn; i = j;
  }
}
template <int NT, int F>
__device__ __attribute__((always_inline)) inline void opt_chunk_body(const AdamArgs& a, int chunk) {
  const OptChunk ch = a.chunks[chunk];
  const smx_f32x4* g4 = reinterpret_cast<const smx_f32x4*>(a.grads + ch.offset);
  smx_f32x4* m4 = reinterpret_cast<smx_f32x4*>(a.m + ch.offset);
  smx_f32x4* v4 = reinterpret_cast<smx_f32x4*>(a.v + ch.offset);
  smx_f32x4* p4 = reinterpret_cast<smx_f32x4*>(a.params + ch.offset);
  const int n4 = ch.count / 4;
  const int i = threadIdx.x;
  smx_f32x4 g = {0.f, 0.f, 0.f, 0.f}, m = g, v = g, p = g;
  const float lr_t = a.state->lr_t;   // (ahead of the norm's barriers: behind them it was a round trip of its own)
  if (F == OPT_ADAM && i < n4) { g = g4[i]; m = m4[i]; v = v4[i]; p = p4[i]; }
  const float clip = adam_tensor_clip<NT>(a, ch, chunk);
  opt_chunk_loop<NT, F>(a, clip, lr_t, i, n4, g4, m4, v4, p4, g, m, v, p);
}
// (one whole body per rule: a body shared by the rules up to the element loop raised the register counts by up to 6)
template <int NT = 256, bool ALL = false>
__device__ inline void adam_chunk_body(const AdamArgs& a, int chunk) {
#define SMX_OPT_BODY(F) opt_chunk_body<NT, F>(a, chunk)
  SMX_OPT_SWITCH(ALL, a.form, SMX_OPT_BODY)
#undef SMX_OPT_BODY
}

// the background sweep's workgroup (smx_adam.hip: adam_sweep_kernel): chunks first + blockIdx.x, + gridDim.x, ... -- the tensor's factor is
// worked out when the tensor changes (the output head's matrix is ~1900 chunks of one tensor), and a thread keeps two quads of every operand in
// flight; element by element the same arithmetic as adam_chunk_body: the same bits
// a chunk of the sweep under the rule F: two quads of every operand in flight
template <int NT, int F>
__device__ __attribute__((always_inline)) inline void opt_sweep_chunk(const AdamArgs& a, float clip, float lr_t, int n4, const smx_f32x4* g4, smx_f32x4* m4, smx_f32x4* v4,
                                       smx_f32x4* p4) {
  constexpr bool UM = OptSlots<F>::m, UV = OptSlots<F>::v;
  const smx_f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < n4; i += 2 * NT) {
    const int j = i + NT;
    const bool two = j < n4;
    const int jj = two ? j : i;
    const smx_f32x4 g0 = g4[i], m0 = UM ? m4[i] : z, v0 = UV ? v4[i] : z, p0 = p4[i];
    const smx_f32x4 g1 = g4[jj], m1 = UM ? m4[jj] : z, v1 = UV ? v4[jj] : z, p1 = p4[jj];
    smx_f32x4 m = m0, v = v0, p = p0;
    opt_apply4<F>(a, clip, lr_t, g0, m, v, p);
    if (UM) m4[i] = m;
    if (UV) v4[i] = v;
    p4[i] = p;
    if (two) {
      m = m1; v = v1; p = p1;
      opt_apply4<F>(a, clip, lr_t, g1, m, v, p);
      if (UM) m4[j] = m;
      if (UV) v4[j] = v;
      p4[j] = p;
    }
  }
}
template <int NT, bool ALL = false>
__device__ inline void adam_sweep_body(const AdamArgs& a, int first, int count) {
  int cur_t = -1;
  float clip = 0.f;
  const float lr_t = a.state->lr_t;
  for (int c = (int)blockIdx.x; c < count; c += (int)gridDim.x) {
    const int chunk = first + c;
    const OptChunk ch = a.chunks[chunk];
    if (ch.tensor != cur_t || chunk == ch.first_chunk) { clip = adam_tensor_clip<NT>(a, ch, chunk); cur_t = ch.tensor; }
    const smx_f32x4* g4 = reinterpret_cast<const smx_f32x4*>(a.grads + ch.offset);
    smx_f32x4* m4 = reinterpret_cast<smx_f32x4*>(a.m + ch.offset);
    smx_f32x4* v4 = reinterpret_cast<smx_f32x4*>(a.v + ch.offset);
    smx_f32x4* p4 = reinterpret_cast<smx_f32x4*>(a.params + ch.offset);
    const int n4 = ch.count / 4;
#define SMX_OPT_SWEEP(F) opt_sweep_chunk<NT, F>(a, clip, lr_t, n4, g4, m4, v4, p4)
    SMX_OPT_SWITCH(ALL, a.form, SMX_OPT_SWEEP)
#undef SMX_OPT_SWEEP
  }
}

__device__ inline float adam_lr_t(float lr, float b1, float b2, uint32_t t /* 1-based */) {
  return lr * sqrtf(1.f - powf(b2, (float)t)) / (1.f - powf(b1, (float)t));
}
// the step size of the step with index `step` under the rule `form`, whose state began at step t0: t = step + 1 - t0 (t0 = 0 for Adam unless
// the rule was switched: Adam's bits as before).  Adamax: lr / (1 - b1^t); the rules without bias correction: lr.
__device__ inline float opt_lr_t(int form, float lr, float b1, float b2, uint32_t step, uint32_t t0) {
  const uint32_t t = step >= t0 ? step + 1u - t0 : 1u;
  if (form == OPT_ADAM) return adam_lr_t(lr, b1, b2, t);
  if (form == OPT_ADAMAX) return lr / (1.f - powf(b1, (float)t));
  return lr;
}

// closing the step (a.master != nullptr), by the first 256 threads of ONE workgroup: the master counter, and -- prepare_next -- the other parity's
// state and row ids for the step after.  Nobody reads next_state / next_rows during this step, so the workgroup may be the optimiser launch's
// last one or a rider of any backward launch of the step (BnBwdArgs::close: a step whose optimiser launch is left out, smx_step.hip).
template <bool ALL>
__device__ inline void step_close_body(const AdamArgs& a) {
  const uint32_t step = a.state->step, cur = a.state->cursor;
  if (a.hist_dp && threadIdx.x < 8) a.hist_dp[(long)cur * 8 + threadIdx.x] = a.tail_metrics[threadIdx.x];
  const float2 w = a.prepare_next && threadIdx.x == 0 ? a.sched[cur + 1] : make_float2(0.f, 0.f);   // (beta, lr) of the next step, requested by cursor beside its row ids
  if (a.prepare_next)
    for (int i = threadIdx.x; i < a.batch; i += 256) a.next_rows[i] = a.order[(long)(cur + 1) * a.batch + i];
  if (threadIdx.x == 0) {
    a.master->next = step + 1;
    if (a.prepare_next) {
      a.next_state->step = step + 1;
      a.next_state->cursor = cur + 1;
      a.next_state->beta = w.x;
      a.next_state->lr = w.y;
      a.next_state->lr_t = opt_lr_t(ALL ? a.form : (int)OPT_ADAM, w.y, a.b1, a.b2, step + 1, a.t0);
    }
  }
}

// the ELBO scalars of a step (a-15) in one 256-thread workgroup: the metrics launch, or a rider of the optimiser's or a BatchNorm-backward launch
__device__ inline void metrics_body(const MetricsArgs& a) {
  // ONE workgroup riding with another launch: its life is that launch's.  Every load is part of a batch (a thread's 32 likelihood partials at
  // a time; the per-cell terms and the history cursor beside them), the seven sums meet in LDS behind ONE pair of barriers -- as a sweep of
  // eight loads per round, a remainder loop of dependent loads and a block_sum per term it was ~15 memory round trips and 14 barriers in a
  // row.  The additions keep their order: the same bits.
  __shared__ float sh[7][4];
  float sx = 0.f, sy = 0.f, sk = 0.f, sl = 0.f, st = 0.f, sd = 0.f, so = 0.f;
  const int tid = (int)threadIdx.x;
  const uint32_t cursor = a.hist ? a.state->cursor : 0u;
  // the per-cell terms of this thread's first cell (minibatches of up to 256 cells: every cell), requested ahead of the sweep
  float c_lg = 0.f, c_y = 0.f, c_o = 0.f, c_k = 0.f, c_l = 0.f, c_t = 0.f, c_d0 = 0.f, c_d1 = 0.f;
  {
    const int b = min(tid, a.B - 1);
    if (a.lgx1) c_lg = a.lgx1[a.rows ? a.rows[b] : b];
    if (a.llk_y) c_y = a.llk_y[b];
    if (a.llk_o) c_o = a.llk_o[b];
    if (a.kl) c_k = a.kl[b];
    if (a.kl_l) c_l = a.kl_l[b];
    if (a.tc) { c_t = a.tc[b]; c_d0 = a.dl[b]; c_d1 = a.dl[a.B + b]; }
  }
  // only the batch total of the count log-likelihood is needed: a flat, coalesced sweep of [B][n_chunks]; part[u] takes the elements
  // tid + 256 u + 2048 k of the full rounds (k ascending), part[0] then the remainder one by one -- as the loop this replaces
  const int total = a.B * a.n_chunks;
  {
    float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nfull = (total > tid + 7 * 256) ? (total - 1 - tid - 7 * 256) / 2048 + 1 : 0;   // rounds with all eight elements in range
    for (int k0 = 0; k0 < nfull; k0 += 4) {
      float v[4][8];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int u = 0; u < 8; ++u) v[kk][u] = a.llk_part[min(tid + (k0 + kk) * 2048 + u * 256, total - 1)];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        if (k0 + kk < nfull) {
#pragma unroll
          for (int u = 0; u < 8; ++u) part[u] += v[kk][u];
        }
    }
    {
      const int i0 = tid + nfull * 2048;   // fewer than eight elements are left for this thread
      float v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = a.llk_part[min(max(i0 + r * 256, 0), total - 1)];
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (i0 + r * 256 < total) part[0] += v[r];
    }
    sx = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
  }
  if (tid < a.B) {
    if (a.lgx1) sx -= c_lg;
    if (a.llk_y) sy += c_y;
    if (a.llk_o) so += c_o;
    if (a.kl) sk += c_k;
    if (a.kl_l) sl += c_l;
    if (a.tc) { st += c_t; sd += c_d0 + c_d1; }
  }
  for (int b = tid + 256; b < a.B; b += 256) {
    if (a.lgx1) sx -= a.lgx1[a.rows ? a.rows[b] : b];
    if (a.llk_y) sy += a.llk_y[b];
    if (a.llk_o) so += a.llk_o[b];
    if (a.kl) sk += a.kl[b];
    if (a.kl_l) sl += a.kl_l[b];
    if (a.tc) { st += a.tc[b]; sd += a.dl[b] + a.dl[a.B + b]; }
  }
  // seven block sums (wave_sum, then the four waves as (0 + 1) + (2 + 3): block_sum's order) behind one pair of barriers
  sx = wave_sum(sx); sy = wave_sum(sy); sk = wave_sum(sk); sl = wave_sum(sl); st = wave_sum(st); sd = wave_sum(sd); so = wave_sum(so);
  __syncthreads();
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    sh[0][w] = sx; sh[1][w] = sy; sh[2][w] = sk; sh[3][w] = sl; sh[4][w] = st; sh[5][w] = sd; sh[6][w] = so;
  }
  __syncthreads();
  if (tid == 0) {
    auto tot = [&](int k) { return (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]); };
    sx = tot(0); sy = tot(1); sk = tot(2); sl = tot(3);
    st = a.tc ? tot(4) : st; sd = a.tc ? tot(5) : sd; so = a.llk_o ? tot(6) : so;
    const float s = a.inv_global_batch;
    float o[8];
    const float beta = a.beta_ptr ? *a.beta_ptr : a.beta;
    o[0] = (a.gamma * st - (sx + so + a.alpha * sy - beta * (sk + sl))) * s;
    o[1] = -sx * s;
    o[2] = -sy * s;
    o[3] = sk * s;
    o[4] = sl * s;
    o[5] = st * s; o[6] = a.tc ? (sd - a.alpha * sy) * s : 0.f; o[7] = -so * s;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.out[i] = o[i];
    if (a.hist) {
      float* h = a.hist + (long)cursor * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) h[i] = o[i];
    }
  }
}

// sum of a range of sum-of-squares slots (fixed order: deterministic); 256 threads
__device__ inline void sq_reduce_body(const float* sl, int cnt, float* dst) {
  __shared__ float sh[4];
  float p[4] = {0.f, 0.f, 0.f, 0.f};
  int i = threadIdx.x;
  for (; i + 3 * 256 < cnt; i += 4 * 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) p[u] += sl[i + u * 256];
  }
  for (; i < cnt; i += 256) p[0] += sl[i];
  const float s = block_sum((p[0] + p[1]) + (p[2] + p[3]), sh);
  if (threadIdx.x == 0) *dst = s;
}

}  // namespace smx
