// smx_loss.hip -- the count likelihoods over smx_loss.h's elementwise terms (gfx950):
//  count_loss  NB / ZINB / NBD / ZINBD / Bernoulli / normal log-likelihood, forward + gradient wrt the parameter planes, one pass over B x G
//              (the bandwidth-bound kernel the roofline is quoted on: SURVEY.md 8d, rows a-10/a-11)
//  label_loss  the masked NB / one-hot label heads of SISUA (a-13), the Bernoulli / normal heads and the mixture (tril) label head
// One unit for both: count_loss calls count_elem only on its diagnostic path (likelihood -2), with x = 0.  Without the label heads'
// calls beside it the compiler specialises count_elem<ZINB / ZINBD> to that constant, and all 24 ZINB / ZINBD count_loss kernels change.
#include "smx_internal.h"
#include "smx_loss.h"

namespace smx {

// grid (n_chunks, B); thread = VEC consecutive genes of one cell (VEC*4-byte accesses).
template <int VEC> struct VecT;
template <> struct VecT<4> { typedef float4 T; };
template <> struct VecT<2> { typedef float2 T; };
template <> struct VecT<1> { typedef float T; };

template <int VEC>
__device__ inline void vload(const float* p, float (&v)[VEC]) {
  const typename VecT<VEC>::T t = *reinterpret_cast<const typename VecT<VEC>::T*>(p);
  const float* f = reinterpret_cast<const float*>(&t);
#pragma unroll
  for (int i = 0; i < VEC; ++i) v[i] = f[i];
}
template <int VEC>
__device__ inline void vstore(float* p, const float (&v)[VEC]) {
  typename VecT<VEC>::T t;
  float* f = reinterpret_cast<float*>(&t);
#pragma unroll
  for (int i = 0; i < VEC; ++i) f[i] = v[i];
  *reinterpret_cast<typename VecT<VEC>::T*>(p) = t;
}

template <int LK, int DIRECT, int BWD, int VEC, int BLOCK = 256, int U16 = 0>   // U16: counts from the compact uint16 store
__global__ __launch_bounds__(BLOCK) void count_loss_kernel(LossArgs a) {
  constexpr int K = (LK == SMX_LLK_MSE || LK == SMX_LLK_BERNOULLI) ? 1 : (LK == SMX_LLK_ZINB || LK == SMX_LLK_ZINBD) ? 3 : 2;
  constexpr int LKC = LK == SMX_LLK_MSE ? SMX_LLK_NB : LK;
  // every wave's non-zero counts go through ONE compacted pass of the lgamma / digamma code (smx_loss.h: lgamma_digamma_diff_queue);
  // 'bernoulli' / 'normal' have no lgamma / digamma
  __shared__ float2 lq[(LK == SMX_LLK_MSE || LK == SMX_LLK_BERNOULLI || LK == SMX_LLK_NORMAL) ? 1 : BLOCK * VEC];
  const float inv_g = 1.f / (float)a.G;   // SMX_LLK_MSE: -log p = mean over the genes of (x - mean)^2
  const int b = blockIdx.y;
  const int g0 = (blockIdx.x * BLOCK + threadIdx.x) * VEC;
  const bool in = g0 < a.Gp;   // (lanes beyond the row carry zero counts)
  float acc = 0.f;
  float xs[VEC], a0[VEC], a1[VEC], a2[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) { xs[e] = 0.f; a0[e] = 0.f; a1[e] = 0.f; a2[e] = 0.f; }
  if (in) {
    const long src = a.rows ? a.rows[b] : b;
    const float* pb = a.P + (long)b * a.ldp + g0;
    if (U16) {
      const uint16_t* xh = reinterpret_cast<const uint16_t*>(a.X) + src * a.ldx + g0;
      if (VEC == 4) { const ushort4 h = *reinterpret_cast<const ushort4*>(xh); xs[0] = h.x; xs[1 % VEC] = h.y; xs[2 % VEC] = h.z; xs[3 % VEC] = h.w; }
      else if (VEC == 2) { const ushort2 h = *reinterpret_cast<const ushort2*>(xh); xs[0] = h.x; xs[1 % VEC] = h.y; }
      else xs[0] = (float)xh[0];
    } else {
      vload<VEC>(a.X + src * a.ldx + g0, xs);
    }
    vload<VEC>(pb, a0);
    if (K >= 2) vload<VEC>(pb + a.plane_stride, a1);
    if (K == 3) vload<VEC>(pb + 2 * a.plane_stride, a2);
  }
  float r0[VEC], r1[VEC], r2[VEC];
  if (a.likelihood < 0 || LK == SMX_LLK_MSE) {   // (launch-uniform) the diagnostics and the deterministic output: element by element
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float llk = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
      if (a.likelihood == -1) {  // diagnostic: same traffic, no arithmetic
        d0 = a0[e] + xs[e]; d1 = K >= 2 ? a1[e] : 0.f; d2 = K == 3 ? a2[e] : 0.f; acc += d0;
      } else if (a.likelihood == -2) {  // diagnostic: every count treated as 0 (no lgamma work)
        count_elem<LKC, DIRECT>(0.f, a0[e], K >= 2 ? a1[e] : 0.f, K == 3 ? a2[e] : 0.f, llk, d0, d1, d2);
        acc += llk + xs[e];
      } else if (in && g0 + e < a.G) {
        const float df = xs[e] - a0[e];
        llk = -(df * df) * inv_g; d0 = 2.f * df * inv_g;
        acc += llk;
      }
      r0[e] = d0 * a.grad_scale; r1[e] = d1 * a.grad_scale; r2[e] = d2 * a.grad_scale;
    }
  } else {
    float llk[VEC], d0[VEC], d1[VEC], d2[VEC], xq[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) xq[e] = (in && g0 + e < a.G) ? xs[e] : 0.f;
    count_elem_vec<LKC, DIRECT, VEC>(xq, a0, a1, a2, llk, d0, d1, d2, lq);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const bool ok = in && g0 + e < a.G;
      acc += ok ? llk[e] : 0.f;
      r0[e] = ok ? d0[e] * a.grad_scale : 0.f; r1[e] = ok ? d1[e] * a.grad_scale : 0.f; r2[e] = ok ? d2[e] * a.grad_scale : 0.f;
    }
  }
  if (BWD && in) {
    float* db = a.dP + (long)b * a.ldp + g0;
    vstore<VEC>(db, r0);
    if (K >= 2) vstore<VEC>(db + a.plane_stride, r1);
    if (K == 3) vstore<VEC>(db + 2 * a.plane_stride, r2);
  }
  // one partial per wave, no workgroup barrier: the consumer sums [n_chunks * waves] values per cell
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0)
    a.llk_part[((long)b * gridDim.x + blockIdx.x) * (BLOCK / 64) + (threadIdx.x >> 6)] = acc;
}

static int loss_block() { return 256; }
// Elements per lane: 4-byte accesses win while the launch is latency-bound (one wave of workgroups), 8-byte
// from ~0.4 M elements (47 % of the HBM peak at 128 x 20 000 against 38 %), 16-byte from ~8 M (64 % at 1024 x
// 20 000) -- tools/loss_roofline.py.  SMX_LOSS_VEC forces a width.
static int loss_vec(int B, int Gp) {
  static const int forced = (int)tuning("loss_vec", 0);
  if (forced == 1 || forced == 2 || forced == 4) return forced;
  const long n = (long)B * Gp;
  return n < 400000 ? 1 : (n < 8000000 ? 2 : 4);
}
static int loss_grid_x(int Gp, int vec) { return (Gp + loss_block() * vec - 1) / (loss_block() * vec); }
// number of partial sums per cell the loss kernel writes (one per wave)
int loss_chunks(int Gp, int B) { return loss_grid_x(Gp, loss_vec(B, Gp)) * (loss_block() / 64); }
int loss_chunks_max(int Gp) { return loss_grid_x(Gp, 1) * (loss_block() / 64); }

template <int LK, int DIRECT>
static void launch_loss_t(hipStream_t st, const LossArgs& a, dim3 grid) {
  const int v = loss_vec(a.B, a.Gp);
#define SMX_LOSS_LAUNCH(B_, V_) do { \
    if (a.x_u16) hipLaunchKernelGGL((count_loss_kernel<LK, DIRECT, B_, V_, 256, 1>), grid, dim3(256), 0, st, a); \
    else hipLaunchKernelGGL((count_loss_kernel<LK, DIRECT, B_, V_, 256>), grid, dim3(256), 0, st, a); } while (0)
  if (a.backward) { if (v == 4) SMX_LOSS_LAUNCH(1, 4); else if (v == 2) SMX_LOSS_LAUNCH(1, 2); else SMX_LOSS_LAUNCH(1, 1); }
  else { if (v == 4) SMX_LOSS_LAUNCH(0, 4); else if (v == 2) SMX_LOSS_LAUNCH(0, 2); else SMX_LOSS_LAUNCH(0, 1); }
#undef SMX_LOSS_LAUNCH
}

int launch_count_loss(hipStream_t st, const LossArgs& a) {
  if (a.B <= 0 || a.Gp % 4 || a.ldx % 4 || a.ldp % 4 || a.plane_stride % 4) {
    set_error("count_loss: bad shapes");
    return SMX_ERR_INVALID;
  }
  dim3 grid(loss_grid_x(a.Gp, loss_vec(a.B, a.Gp)), a.B);
  switch (a.likelihood) {
    case SMX_LLK_NB: launch_loss_t<SMX_LLK_NB, 0>(st, a, grid); break;
    case SMX_LLK_ZINB: launch_loss_t<SMX_LLK_ZINB, 0>(st, a, grid); break;
    case SMX_LLK_NBD:
      if (a.direct) launch_loss_t<SMX_LLK_NBD, 1>(st, a, grid); else launch_loss_t<SMX_LLK_NBD, 0>(st, a, grid);
      break;
    case SMX_LLK_ZINBD:
      if (a.direct) launch_loss_t<SMX_LLK_ZINBD, 1>(st, a, grid); else launch_loss_t<SMX_LLK_ZINBD, 0>(st, a, grid);
      break;
    case SMX_LLK_MSE: launch_loss_t<SMX_LLK_MSE, 0>(st, a, grid); break;
    case SMX_LLK_BERNOULLI: launch_loss_t<SMX_LLK_BERNOULLI, 0>(st, a, grid); break;
    case SMX_LLK_NORMAL: launch_loss_t<SMX_LLK_NORMAL, 0>(st, a, grid); break;
    default: set_error("count_loss: unknown likelihood"); return SMX_ERR_INVALID;
  }
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}


// ===========================================================================
// SISUA label heads: one wave per cell, lanes over the label columns (P is tens of columns); unlabelled cells
// (mask == 0, 90 % of them at labels_percent = 0.1) contribute nothing and only zero their gradient rows.
// ===========================================================================
__global__ __launch_bounds__(256) void label_loss_kernel(LabelArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const long src = a.rows ? a.rows[b] : b;
  const float* y = a.Y + src * a.ldy;
  const float* raw = a.raw + (long)b * a.ld;
  const float m = a.observed ? 1.f : a.mask ? (a.mask[src] ? 1.f : 0.f) : 0.f;
  const float gs = a.grad_scale * m;
  float llk = 0.f;
  if (m == 0.f) {   // wave-uniform
    if (a.backward) {
      const int width = ((a.kind == SMX_LABEL_NB || a.kind == SMX_LABEL_NBD || a.kind == SMX_LABEL_NORMAL) ? 2 : (a.kind == SMX_LABEL_ZINB || a.kind == SMX_LABEL_ZINBD) ? 3 :
                         (a.kind == SMX_LABEL_MIXNB || a.kind == SMX_LABEL_MIXGAUSS) ? 3 * a.C : a.kind == SMX_LABEL_MIXZINB ? 4 * a.C : 1) * a.Pp;
      for (int p = lane; p < width; p += 64) a.draw[(long)b * a.ld + p] = 0.f;
    }
  } else if (a.kind == SMX_LABEL_MIXNB || a.kind == SMX_LABEL_MIXGAUSS || a.kind == SMX_LABEL_MIXZINB) {
    // MISA: log p(y_p) = logsumexp_c(log softmax(mix)_c + log f_c(y_p)); f_c = NB(exp(r_c), l_c) with planes C mixture logits,
    // C log total_counts, C logits -- or, for continuous labels ('mixgaussian', vae.py:86-92), f_c = Normal(loc_c,
    // softplus(s_c + softplus_inverse(1))) with planes C mixture logits, C locations, C raw scales.
    // Gradients: d mix_c = resp_c - pi_c, d (component parameters) = resp_c * d log f_c.
    const int C = a.C;
    // MISA(zero_inflated=True) (vae.py:76-84): f_c = ZINB with a fourth group of C gate-logit planes.
    const bool gauss = a.kind == SMX_LABEL_MIXGAUSS, zi = a.kind == SMX_LABEL_MIXZINB;   // (launch-uniform)
    for (int p = lane; p < a.Pp; p += 64) {
      float e[4], d0[4], d1[4], dg[4], mx[4];
      float am = -3.0e38f, jm = -3.0e38f;
      const bool live = p < a.P;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        e[c] = 0.f; d0[c] = 0.f; d1[c] = 0.f; dg[c] = 0.f; mx[c] = 0.f;
        if (c < C && live) {
          float d2;
          mx[c] = raw[c * a.Pp + p];
          if (gauss) {
            const float mu = raw[(C + c) * a.Pp + p];
            const SpSg s = softplus_sigmoid(raw[(2 * C + c) * a.Pp + p] + SMX_SOFTPLUS_INV_1);   // sp = sigma, sg = d sigma / d raw
            const float inv = frcp(s.sp), zz = (y[p] - mu) * inv;
            e[c] = -0.5f * zz * zz - flog(s.sp) - 0.9189385332046727f;   // 0.5 log(2 pi)
            d0[c] = zz * inv;
            d1[c] = (zz * zz - 1.f) * inv * s.sg;
          } else if (zi)
          count_elem<SMX_LLK_ZINB, 0>(y[p], raw[(C + c) * a.Pp + p], raw[(2 * C + c) * a.Pp + p], raw[(3 * C + c) * a.Pp + p], e[c], d0[c], d1[c], dg[c]);
          else
          count_elem<SMX_LLK_NB, 0>(y[p], raw[(C + c) * a.Pp + p], raw[(2 * C + c) * a.Pp + p], 0.f, e[c], d0[c], d1[c], d2);
          am = fmaxf(am, mx[c]);
          jm = fmaxf(jm, mx[c] + e[c]);
        }
      }
      float sa = 0.f, sj = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C && live) { sa += expf(mx[c] - am); sj += expf(mx[c] + e[c] - jm); }
      const float lse_a = am + logf(sa), lse_j = jm + logf(sj);
      if (live) llk += lse_j - lse_a - (gauss ? 0.f : lgammaf(y[p] + 1.f));
      if (a.backward) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < C) {
            const float resp = live ? expf(mx[c] + e[c] - lse_j) : 0.f, pi = live ? expf(mx[c] - lse_a) : 0.f;
            a.draw[(long)b * a.ld + c * a.Pp + p] = (resp - pi) * gs;
            a.draw[(long)b * a.ld + (C + c) * a.Pp + p] = resp * d0[c] * gs;
            a.draw[(long)b * a.ld + (2 * C + c) * a.Pp + p] = resp * d1[c] * gs;
            if (zi) a.draw[(long)b * a.ld + (3 * C + c) * a.Pp + p] = resp * dg[c] * gs;
          }
      }
    }
    llk = wave_sum(llk);
  } else if (a.kind == SMX_LABEL_NB || a.kind == SMX_LABEL_NBD || a.kind == SMX_LABEL_ZINB || a.kind == SMX_LABEL_ZINBD) {
    // a count posterior over the head's columns, planes as for the gene output (the elementwise likelihood of smx_loss.h)
    const bool zi = a.kind == SMX_LABEL_ZINB || a.kind == SMX_LABEL_ZINBD;   // (launch-uniform)
    for (int p = lane; p < a.Pp; p += 64) {
      float d0 = 0.f, d1 = 0.f, d2 = 0.f;
      if (p < a.P) {
        float e;
        const float p2 = zi ? raw[2 * a.Pp + p] : 0.f;
        if (a.kind == SMX_LABEL_NB) count_elem<SMX_LLK_NB, 0>(y[p], raw[p], raw[a.Pp + p], 0.f, e, d0, d1, d2);
        else if (a.kind == SMX_LABEL_NBD) count_elem<SMX_LLK_NBD, 0>(y[p], raw[p], raw[a.Pp + p], 0.f, e, d0, d1, d2);
        else if (a.kind == SMX_LABEL_ZINB) count_elem<SMX_LLK_ZINB, 0>(y[p], raw[p], raw[a.Pp + p], p2, e, d0, d1, d2);
        else count_elem<SMX_LLK_ZINBD, 0>(y[p], raw[p], raw[a.Pp + p], p2, e, d0, d1, d2);
        llk += e - lgammaf(y[p] + 1.f);
      }
      if (a.backward) {
        a.draw[(long)b * a.ld + p] = d0 * gs; a.draw[(long)b * a.ld + a.Pp + p] = d1 * gs;
        if (zi) a.draw[(long)b * a.ld + 2 * a.Pp + p] = d2 * gs;
      }
    }
    llk = wave_sum(llk);
  } else if (a.kind == SMX_LABEL_BERNOULLI) {
    // (the operations of smx_loss.h's bernoulli_elem, the gene output's form)
    // every label dimension its own binary variable, one plane of logits l (TFP Bernoulli.log_prob, any y in [0, 1]):
    // log p(y) = y l - softplus(l), d / d l = y - sigmoid(l); softplus and sigmoid from one exp(-|l|): no overflow at saturation
    for (int p = lane; p < a.Pp; p += 64) {
      float d = 0.f;
      if (p < a.P) {
        const float l = raw[p];
        const SpSg s = softplus_sigmoid(l);
        llk += y[p] * l - s.sp;
        d = y[p] - s.sg;
      }
      if (a.backward) a.draw[(long)b * a.ld + p] = d * gs;
    }
    llk = wave_sum(llk);
  } else if (a.kind == SMX_LABEL_NORMAL) {
    // (the operations of smx_loss.h's normal_elem, the gene output's form)
    // an independent normal per label dimension, planes loc m | raw scale s, sigma = softplus(s + softplus^-1(1)) ([3P-recall] odin's
    // 'softplus1', the scale activation of the latents and of one 'mixgaussian' component above):
    // log p(y) = -z^2 / 2 - log sigma - log(2 pi) / 2, z = (y - m) / sigma; d m = z / sigma, d s = (z^2 - 1) / sigma * sigmoid(s + softplus^-1(1))
    for (int p = lane; p < a.Pp; p += 64) {
      float d0 = 0.f, d1 = 0.f;
      if (p < a.P) {
        const SpSg s = softplus_sigmoid(raw[a.Pp + p] + SMX_SOFTPLUS_INV_1);   // sp = sigma, sg = d sigma / d s
        const float inv = frcp(s.sp), zz = (y[p] - raw[p]) * inv;
        llk += -0.5f * zz * zz - flog(s.sp) - 0.9189385332046727f;   // 0.5 log(2 pi)
        d0 = zz * inv;
        d1 = (zz * zz - 1.f) * inv * s.sg;
      }
      if (a.backward) { a.draw[(long)b * a.ld + p] = d0 * gs; a.draw[(long)b * a.ld + a.Pp + p] = d1 * gs; }
    }
    llk = wave_sum(llk);
  } else {
    float mx = -3.0e38f, ysum = 0.f;
    for (int p = lane; p < a.P; p += 64) { mx = fmaxf(mx, raw[p]); ysum += y[p]; }
    mx = wave_max(mx);
    ysum = wave_sum(ysum);
    float se = 0.f;
    for (int p = lane; p < a.P; p += 64) se += expf(raw[p] - mx);
    se = wave_sum(se);
    const float lse = mx + logf(se);
    for (int p = lane; p < a.Pp; p += 64) {
      float d = 0.f;
      if (p < a.P) {
        const float lp = raw[p] - lse;
        llk += y[p] * lp;
        d = y[p] - expf(lp) * ysum;
      }
      if (a.backward) a.draw[(long)b * a.ld + p] = d * gs;
    }
    llk = wave_sum(llk);
  }
  if (lane == 0) a.llk[b] = (a.add ? a.llk[b] : 0.f) + m * llk;
}
// MISA's 'mixtril' head (sisua/models/vae.py:58, the class's own example): ONE C-component mixture over the whole label vector,
// component c = MultivariateNormalTriL(loc_c, L_c), diag(L) = softplus(raw) + 1e-5 (TFP's FillScaleTriL), strict lower triangle = raw.
// Planes of width Pp (config.label_planes): C logit planes (column 0), C location planes, per component P planes = the columns of L
// (plane j, row p >= j).  One wave per cell, lane p = label dimension p (P <= 64); a component's L sits in LDS as [P][P + 1]:
//   u = L^-1 (y - mu)   forward substitution: lane j publishes u_j, the lanes below subtract L[p][j] u_j
//   w = L^-T u          back substitution through the column view
//   log N = -1/2 |u|^2 - sum log L_pp - P/2 log 2 pi;   d mu = w,   d L[p][j] = w_p u_j - [p == j] / L_pp
// and the mixture over components as in label_loss_kernel: d logit_c = resp_c - pi_c, component gradients times resp_c.
// One workgroup per cell, one WAVE per component (the components' substitution chains side by side instead of one after the other
// in a single wave: 30 -> 16 us per launch at 38 label dimensions and two components); wave c keeps its factor in its own LDS tile,
// the components' log densities meet in LDS, every wave then writes its own component's gradient planes.
__global__ __launch_bounds__(256) void label_tril_kernel(LabelArgs a) {
  extern __shared__ float Lsm[];   // C x [P][P + 1] | e [4]
  const int lane = threadIdx.x & 63, c = threadIdx.x >> 6, b = blockIdx.x;   // (blockDim = 64 C)
  const long src = a.rows ? a.rows[b] : b;
  const float* raw = a.raw + (long)b * a.ld;
  float* draw = a.draw + (long)b * a.ld;
  const float m = a.observed ? 1.f : a.mask ? (a.mask[src] ? 1.f : 0.f) : 0.f;
  const float gs = a.grad_scale * m;
  const int C = a.C, P = a.P, Pp = a.Pp, ldl = P + 1;
  if (m == 0.f) {   // (block-uniform)
    if (a.backward) for (int i = threadIdx.x; i < C * (2 + P) * Pp; i += 64 * C) draw[i] = 0.f;
    if (threadIdx.x == 0) a.llk[b] = a.add ? a.llk[b] : 0.f;
    return;
  }
  float* Ls = Lsm + c * P * ldl;
  float* esh = Lsm + C * P * ldl;
  const bool live = lane < P;
  const float yv = live ? a.Y[src * a.ldy + lane] : 0.f;
  const float mxc = raw[c * Pp];
  const float mu = live ? raw[(C + c) * Pp + lane] : 0.f;
  float lpp = 1.f, sg = 0.f;
  for (int j0 = 0; j0 < P; j0 += 8) {   // plane j = column j of L, coalesced over the rows; eight planes' loads in flight at once
    float v8[8];                        // (one load per plane, each followed by its LDS store, was a chain of P memory round trips)
#pragma unroll
    for (int t = 0; t < 8; ++t) v8[t] = (live && j0 + t < P) ? raw[(2 * C + c * P + j0 + t) * Pp + lane] : 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int j = j0 + t;
      float v = v8[t];
      if (j == lane) { const SpSg sp = softplus_sigmoid(v); v = sp.sp + 1e-5f; lpp = v; sg = sp.sg; }
      if (live && j < P) Ls[lane * ldl + j] = j <= lane ? v : 0.f;
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier();   // (the tile is this wave's own)
  const float inv = frcp(lpp);
  // (pivots broadcast by v_readlane: with __shfl = ds_bpermute a substitution step took two LDS round trips.  Fully unrolled forms with
  // the factor in registers measured SLOWER: the unrolled code's predicated steps beyond P are thousands of serial instructions)
  float r = yv - mu, u = 0.f;
  for (int j = 0; j < P; ++j) {
    const float lj = live ? Ls[lane * ldl + j] : 0.f;
    const float uj = lane_bcast(r * inv, j);
    if (lane == j) u = uj;
    else if (lane > j) r -= lj * uj;
  }
  float sw = u, w = 0.f;
  for (int i = P - 1; i >= 0; --i) {
    const float li = live ? Ls[i * ldl + lane] : 0.f;   // (zero above the diagonal: lanes beyond i add nothing)
    const float wi = lane_bcast(sw * inv, i);
    if (lane == i) w = wi;
    else if (lane < i) sw -= li * wi;
  }
  const float quad = wave_sum(live ? u * u : 0.f), logdet = wave_sum(live ? flog(lpp) : 0.f);
  const float ec = -0.5f * quad - logdet - 0.9189385332046727f * (float)P;
  if (lane == 0) { esh[c] = ec; esh[4 + c] = mxc; }
  __syncthreads();
  float am = -3.0e38f, jm = -3.0e38f;
  for (int q = 0; q < C; ++q) { am = fmaxf(am, esh[4 + q]); jm = fmaxf(jm, esh[4 + q] + esh[q]); }
  float sa = 0.f, sj = 0.f;
  for (int q = 0; q < C; ++q) { sa += expf(esh[4 + q] - am); sj += expf(esh[4 + q] + esh[q] - jm); }   // (component order: every wave the same bits)
  const float lse_a = am + logf(sa), lse_j = jm + logf(sj);
  if (threadIdx.x == 0) a.llk[b] = (a.add ? a.llk[b] : 0.f) + (lse_j - lse_a);
  if (!a.backward) return;
  const float resp = expf(mxc + ec - lse_j), pi = expf(mxc - lse_a);
  for (int p = lane; p < Pp; p += 64) {
    draw[c * Pp + p] = p == 0 ? (resp - pi) * gs : 0.f;
    draw[(C + c) * Pp + p] = p < P ? resp * w * gs : 0.f;   // (p == lane here: P <= 64)
  }
  for (int j = 0; j < P; ++j) {
    const float uj = lane_bcast(u, j);
    float d = 0.f;
    if (live && j < lane) d = w * uj;
    else if (live && j == lane) d = (w * uj - inv) * sg;
    for (int p = lane; p < Pp; p += 64) draw[(2 * C + c * P + j) * Pp + p] = p < P ? resp * d * gs : 0.f;
  }
}

int launch_label_loss(hipStream_t st, const LabelArgs& a) {
  if (a.kind == SMX_LABEL_MIXTRIL) {
    if (a.P < 1 || a.P > 64 || a.C < 2 || a.C > 4) { set_error("label_loss: 'mixtril' heads take 1..64 label dimensions and 2..4 components"); return SMX_ERR_INVALID; }
    const size_t lds = ((size_t)a.C * a.P * (a.P + 1) + 8) * sizeof(float);   // (66.6 KB at C = 4, P = 64)
    static const bool big_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&label_tril_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024) == hipSuccess;
    if (lds > 64 * 1024 && !big_ok) { set_error("label_loss: cannot reserve the LDS of the 'mixtril' head"); return SMX_ERR_HIP; }
    hipLaunchKernelGGL(label_tril_kernel, dim3(a.B), dim3(64 * a.C), lds, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  hipLaunchKernelGGL(label_loss_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

}  // namespace smx
