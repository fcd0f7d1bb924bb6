// smx_adam.hip -- the per-step launches around the optimiser (gfx950): step begin, the ELBO scalars (a-15), per-tensor clipnorm +
// Adam (or the rule of smx_set_optimizer) over the flat buffer (a-16) as one launch, a background sweep or a sharded chain, and the norms.  The workgroup bodies they
// share with the riders of other launches are smx_adam.h's.
#include "smx_internal.h"
#include "smx_adam.h"

namespace smx {

// ===========================================================================
// per-step scalars, metrics
// ===========================================================================
// (adam_lr_t / opt_lr_t: smx_adam.h, beside the step's closing body that shares them)
__global__ void step_begin_kernel(StepState* master, StepState* dst, const int32_t* order, int32_t* rows, int batch,
                                  int cursor_from_master, uint32_t cursor, const float2* sched, float b1, float b2, int form, uint32_t t0) {
  const uint32_t cur = cursor_from_master ? master->cursor : cursor;
  if (order)
    for (int i = threadIdx.x; i < batch; i += blockDim.x) rows[i] = order[(long)cur * batch + i];
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t step = master->next;
    const float2 w = sched[cur];   // (beta, lr) of this step (smx_set_schedule)
    dst->step = step;
    dst->cursor = cur;
    dst->beta = w.x;
    dst->lr = w.y;
    dst->lr_t = opt_lr_t(form, w.y, b1, b2, step, t0);
    if (cursor_from_master) master->cursor = cur + 1;
  }
}
int launch_step_begin(hipStream_t st, StepState* master, StepState* dst, const int32_t* order, int32_t* rows,
                      int batch, int cursor_from_master, uint32_t cursor, const float2* sched, float b1, float b2, int form, uint32_t t0) {
  if (!sched) { set_error("step_begin: no schedule table"); return SMX_ERR_INVALID; }
  hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(256), 0, st, master, dst, order, rows, batch, cursor_from_master,
                     cursor, sched, b1, b2, form, t0);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

__global__ __launch_bounds__(256) void metrics_kernel(MetricsArgs a) { metrics_body(a); }
int launch_metrics(hipStream_t st, const MetricsArgs& a) {
  hipLaunchKernelGGL(metrics_kernel, dim3(1), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ===========================================================================
// optimiser: per-tensor clipnorm + Adam over the flat buffer
// ===========================================================================
__global__ __launch_bounds__(256) void grad_sqsum_kernel(AdamArgs a) {
  const int extra = (int)blockIdx.x - (a.sq_chunks >= 0 ? a.sq_chunks : a.n_chunks);
  if (extra >= 0) {   // extra workgroups: the ELBO scalars of this step, then the moving BatchNorm statistics (data parallel)
    if (a.with_metrics && extra == 0) { metrics_body(a.metrics); return; }
    const int i = (extra - (a.with_metrics ? 1 : 0)) * 256 + (int)threadIdx.x;
    if (i < a.bn_total) a.bn_moving[i] = a.bn_moving[i] * a.bn_momentum + a.bn_batch[i] * a.bn_inv_world * (1.f - a.bn_momentum);
    return;
  }
  __shared__ float sh[4];
  const OptChunk ch = a.chunks[blockIdx.x];
  float s = 0.f;
  const float4* g4 = reinterpret_cast<const float4*>(a.grads + ch.offset);
  for (int i = threadIdx.x; i < ch.count / 4; i += 256) {
    const float4 g = g4[i];
    s += (g.x * g.x + g.y * g.y) + (g.z * g.z + g.w * g.w);
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
}

// ALL = false: Adam (the rule a model is created with) without a line of the other rules' code; ALL = true: every rule (AdamArgs.form)
template <bool ALL>
__global__ __launch_bounds__(256) void adam_update_kernel(AdamArgs a) {
  if ((int)blockIdx.x == a.n_launch && a.use_sq && a.with_metrics) {  // use_sq form: the ELBO scalars ride along here
    metrics_body(a.metrics);
    return;
  }
  if ((int)blockIdx.x < a.n_launch) {
    adam_chunk_body<256, ALL>(a, (int)blockIdx.x >= a.gap_from ? (int)blockIdx.x + a.gap_len : (int)blockIdx.x);
    return;
  }
  // the LAST workgroup closes the step (nobody reads next_state / next_rows during this step).  As a duty of workgroup 0 behind its chunk --
  // state -> row ids -> stores: two more dependent round trips and a powf -- it was the launch's critical path.
  if (a.master) step_close_body<ALL>(a);
}

// the heads' update as a background sweep beside the launches that follow the output head (smx_backward.hip: head_sweep_*): a FIXED
// number of workgroups walk the chunks, so the sweep never holds more than a few wave slots per CU and the small dependent
// launches of the main stream are placed at once
template <int NT, bool ALL>
__global__ __launch_bounds__(NT) void adam_sweep_kernel(AdamArgs a, int first, int count) {
  adam_sweep_body<NT, ALL>(a, first, count);
}
// the chunks' sums of squares for a RANGE of chunks (data parallel, chained form: the heads' chunks on the communication stream behind
// their bucket's all-reduce; the optimiser launch's own pass then covers the front chunks only)
__global__ __launch_bounds__(256) void grad_sqsum_range_kernel(AdamArgs a, int first) {
  __shared__ float sh[4];
  const int chunk = first + (int)blockIdx.x;
  const OptChunk ch = a.chunks[chunk];
  float s = 0.f;
  const float4* g4 = reinterpret_cast<const float4*>(a.grads + ch.offset);
  for (int i = threadIdx.x; i < ch.count / 4; i += 256) {
    const float4 g = g4[i];
    s += (g.x * g.x + g.y * g.y) + (g.z * g.z + g.w * g.w);
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) a.partial[chunk] = s;
}
int launch_grad_sqsum_range(hipStream_t st, const AdamArgs& a, int first, int count) {
  if (count <= 0) return SMX_OK;
  hipLaunchKernelGGL(grad_sqsum_range_kernel, dim3((unsigned)count), dim3(256), 0, st, a, first);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
int launch_adam_sweep(hipStream_t st, const AdamArgs& a, int first, int count, int wgs) {
  if (count <= 0) return SMX_OK;
  // (norms from the products' sum-of-squares partials, or -- use_sq = 0 -- from a.partial, filled by launch_grad_sqsum_range before)
  if (wgs <= 0) { set_error("adam sweep: no workgroups"); return SMX_ERR_INVALID; }
  if (a.form == OPT_ADAM)   // (512-thread workgroups: 181-184 us per c5-shard step against 175-176)
    hipLaunchKernelGGL((adam_sweep_kernel<256, false>), dim3((unsigned)std::min(wgs, count)), dim3(256), 0, st, a, first, count);
  else
    hipLaunchKernelGGL((adam_sweep_kernel<256, true>), dim3((unsigned)std::min(wgs, count)), dim3(256), 0, st, a, first, count);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ---- flag opt_shard (data parallel, chained form): the heads' optimiser state sharded over the ranks --------------------------------------
// This rank owns the floats [shard_lo, shard_hi) of the head bucket -- a slice cut at a 64-float boundary, through chunks where it falls.
// (1) per chunk, the sum of squares of the chunk's part inside the slice (0 for a chunk outside it): summed over the ranks these are the
//     chunks' sums of squares of the whole reduced gradient;  (2) the tensors' norms from them, on every rank, for the metrics;
// (3) clip + Adam of the elements inside the slice, the tensor's norm from the summed partials (adam_tensor_clip's use_sq = 0 path).
__device__ inline void shard_range(const AdamArgs& a, const OptChunk& ch, int& i_lo, int& i_hi) {
  const long n4 = ch.count / 4;
  const long lo = (a.shard_lo - (long)ch.offset) / 4, hi = (a.shard_hi - (long)ch.offset + 3) / 4;   // (offsets and bounds are multiples of 4)
  i_lo = (int)(lo < 0 ? 0 : (lo > n4 ? n4 : lo));
  i_hi = (int)(hi < 0 ? 0 : (hi > n4 ? n4 : hi));
}
__global__ __launch_bounds__(256) void grad_sqsum_shard_kernel(AdamArgs a, int first) {
  __shared__ float sh[4];
  const int chunk = first + (int)blockIdx.x;
  const OptChunk ch = a.chunks[chunk];
  int i_lo, i_hi;
  shard_range(a, ch, i_lo, i_hi);
  float s = 0.f;
  const float4* g4 = reinterpret_cast<const float4*>(a.grads + ch.offset);
  for (int i = i_lo + (int)threadIdx.x; i < i_hi; i += 256) {
    const float4 g = g4[i];
    s += (g.x * g.x + g.y * g.y) + (g.z * g.z + g.w * g.w);
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) a.partial[chunk] = s;
}
// one workgroup per tensor of the chunk range [first, first + count): the b-th tensor is found by walking the chunk table
__global__ __launch_bounds__(256) void head_norms_kernel(AdamArgs a, int first, int count) {
  __shared__ float sh[4];
  int c = first;
  for (int b = 0; b < (int)blockIdx.x && c < first + count; ++b) c += a.chunks[c].n_chunks;
  if (c >= first + count) return;
  const OptChunk ch = a.chunks[c];
  float s = 0.f;
  for (int k = threadIdx.x; k < ch.n_chunks; k += 256) s += a.partial[ch.first_chunk + k];
  s = block_sum(s, sh);
  if (ch.tensor == a.tied_t0 || ch.tensor == a.tied_t1) s *= a.tied_inv;
  if (threadIdx.x == 0) a.tensor_norm[ch.tensor] = sqrtf(s) * a.grad_scale;
}
// the elements [i_lo, i_hi) of a chunk under the rule F
template <int F>
__device__ __attribute__((always_inline)) inline void opt_shard_range(const AdamArgs& a, float clip, float lr_t, int i_lo, int i_hi, const smx_f32x4* g4, smx_f32x4* m4,
                                       smx_f32x4* v4, smx_f32x4* p4) {
  constexpr bool UM = OptSlots<F>::m, UV = OptSlots<F>::v;
  const smx_f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = i_lo + (int)threadIdx.x; i < i_hi; i += 256) {
    smx_f32x4 m = UM ? m4[i] : z, v = UV ? v4[i] : z, p = p4[i];
    opt_apply4<F>(a, clip, lr_t, g4[i], m, v, p);
    if (UM) m4[i] = m;
    if (UV) v4[i] = v;
    p4[i] = p;
  }
}
template <bool ALL>
__global__ __launch_bounds__(256) void adam_shard_kernel(AdamArgs a, int first, int count) {
  int cur_t = -1;
  float clip = 0.f;
  const float lr_t = a.state->lr_t;
  for (int c = (int)blockIdx.x; c < count; c += (int)gridDim.x) {
    const int chunk = first + c;
    const OptChunk ch = a.chunks[chunk];
    int i_lo, i_hi;
    shard_range(a, ch, i_lo, i_hi);
    if (i_lo >= i_hi) continue;   // (block-uniform) a chunk of another rank's slice
    if (ch.tensor != cur_t) {     // the factor of this chunk's tensor, from the summed partials (the launcher insists on use_sq = 0; every thread takes part: two barriers)
      clip = adam_tensor_clip<256>(a, ch, -1);   // (chunk -1: tensor_norm is head_norms_kernel's to write)
      cur_t = ch.tensor;
    }
    const smx_f32x4* g4 = reinterpret_cast<const smx_f32x4*>(a.grads + ch.offset);
    smx_f32x4* m4 = reinterpret_cast<smx_f32x4*>(a.m + ch.offset);
    smx_f32x4* v4 = reinterpret_cast<smx_f32x4*>(a.v + ch.offset);
    smx_f32x4* p4 = reinterpret_cast<smx_f32x4*>(a.params + ch.offset);
#define SMX_OPT_RANGE(F) opt_shard_range<F>(a, clip, lr_t, i_lo, i_hi, g4, m4, v4, p4)
    SMX_OPT_SWITCH(ALL, a.form, SMX_OPT_RANGE)
#undef SMX_OPT_RANGE
  }
}
int launch_grad_sqsum_shard(hipStream_t st, const AdamArgs& a, int first, int count) {
  if (count <= 0) return SMX_OK;
  hipLaunchKernelGGL(grad_sqsum_shard_kernel, dim3((unsigned)count), dim3(256), 0, st, a, first);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
int launch_head_norms(hipStream_t st, const AdamArgs& a, int first, int count) {
  if (count <= 0) return SMX_OK;
  hipLaunchKernelGGL(head_norms_kernel, dim3((unsigned)std::min(count, SMX_MAX_TENSORS)), dim3(256), 0, st, a, first, count);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
int launch_adam_shard(hipStream_t st, const AdamArgs& a, int first, int count, int wgs) {
  if (count <= 0) return SMX_OK;
  if (wgs <= 0 || a.use_sq || a.shard_hi <= a.shard_lo || (a.shard_lo % 4) || (a.shard_hi % 4)) { set_error("adam shard: bad arguments"); return SMX_ERR_INVALID; }
  if (a.form == OPT_ADAM)
    hipLaunchKernelGGL((adam_shard_kernel<false>), dim3((unsigned)std::min(wgs, count)), dim3(256), 0, st, a, first, count);
  else
    hipLaunchKernelGGL((adam_shard_kernel<true>), dim3((unsigned)std::min(wgs, count)), dim3(256), 0, st, a, first, count);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// Two launches.  A single-launch form (per-tensor arrival counters, the chunk's gradient kept in registers
// while the workgroup waits for its tensor's other chunks) was measured at 39 us against 16 us for this pair:
// an agent-scope acquire/release round across the 8 XCDs costs far more than a kernel boundary (1.5 us).
int launch_adam(hipStream_t st, const AdamArgs& a) {
  if (a.use_sq) {   // norms come from the weight-gradient products: no pass over the gradient buffer
    const dim3 grid(a.n_launch + (a.with_metrics ? 1 : 0) + (a.master ? 1 : 0));
    if (a.form == OPT_ADAM) hipLaunchKernelGGL(adam_update_kernel<false>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(adam_update_kernel<true>, grid, dim3(256), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  hipLaunchKernelGGL(grad_sqsum_kernel, dim3((a.sq_chunks >= 0 ? a.sq_chunks : a.n_chunks) + (a.with_metrics ? 1 : 0) + (a.bn_total + 255) / 256), dim3(256), 0, st, a);
  if (a.form == OPT_ADAM) hipLaunchKernelGGL(adam_update_kernel<false>, dim3(a.n_launch + (a.master ? 1 : 0)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(adam_update_kernel<true>, dim3(a.n_launch + (a.master ? 1 : 0)), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// the slots of a rule that starts fresh (smx_set_optimizer): every float of [0, n) set to `value`
__global__ __launch_bounds__(256) void opt_fill_kernel(float* dst, long n, float value) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = value;
}
int launch_opt_fill(hipStream_t st, float* dst, long n, float value) {
  if (n <= 0) return SMX_OK;
  hipLaunchKernelGGL(opt_fill_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 4096)), dim3(256), 0, st, dst, n, value);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

}  // namespace smx
