// smx_sample.hip -- posterior-predictive draws of the gene output from the parameter planes of a pass: smx_predict_stat's walk with
// stat 4 (smx_predict_sample, smx_predict.hip) and the kernel-test entry smx_k_plane_sample.  DESIGN.md section 4j.
//
// One draw x ~ p(x | planes) per (sample k, draw s, cell, gene), float32:
//   nb / zinb    Poisson(Gamma(shape = exp(p0), scale = exp(p1)));   nbd / zinbd   Poisson(Gamma(shape = theta, scale = mu / theta)),
//   mu, theta as plane_moments reads them; zero-inflated: kept with probability 1 - sigmoid(p2), else 0 (count_only: no gate);
//   bernoulli    u < sigmoid(p0);   normal   loc + softplus1(raw) n;   mse   the location itself.
//
// COUNTERS.  Every random word is a word of philox4x32_10(c0, c1, c2, c3; key = the call's seed) with
//   c0 = gene,  c1 = row of the call's input,  c2 = sample k,  c3 = ST_PREDICTIVE | attempt << 8 | draw s << 16,
// so a draw depends on (seed, k, s, row, gene, attempt) alone: not on the batch size, the chunking, the store the rows came from or the lane.
//   attempt 0                      the fixed block: .x gate uniform (bernoulli: its uniform), .y the u^(1/shape) boost of a shape below 1,
//                                  .z the uniform of the Poisson inversion, (.x, .y) the normal of the 'normal' output
//   attempt 1 .. 16                Marsaglia-Tsang proposals of the Gamma draw: (.x, .y) the normal, .z the uniform
//   attempt 17 .. 40               PTRS proposals of the Poisson draw: .x U, .y V; attempt 17's (.x, .y) is the normal of the rounded-normal form
// Each loop ends after its constant number of attempts with a deterministic value (the Gamma's mean, the rounded rate), and every accept
// test is written so that a NaN never passes: a NaN plane falls through to the fall-back and comes out NaN.
#include "smx_model.h"

namespace smx {

enum { SAMPLE_GAMMA_ATTEMPTS = 16, SAMPLE_PTRS_ATTEMPTS = 24, SAMPLE_INVERSION_STEPS = 64 };
enum { AT_FIXED = 0, AT_GAMMA = 1, AT_POISSON = AT_GAMMA + SAMPLE_GAMMA_ATTEMPTS };
static_assert(AT_POISSON + SAMPLE_PTRS_ATTEMPTS <= 256, "the attempt index has 8 bits of the counter");
#define SAMPLE_INVERSION_BELOW 10.f       // rates under it: inversion by the pmf recurrence (PTRS needs a rate of at least 10)
#define SAMPLE_NORMAL_FROM 4194304.f      // 2^22: rates from it on: the rounded normal (float32's spacing there is 1 / 2, the deviation 2048)

struct SampleCtr { uint32_t gene, row, k, hi, k0, k1; };   // hi: ST_PREDICTIVE | draw << 16
__device__ inline U4 sample_block(const SampleCtr& c, uint32_t attempt) {
  return philox4x32_10(c.gene, c.row, c.k, c.hi | (attempt << 8), c.k0, c.k1);
}
// a uniform strictly inside (0, 1): 23 bits and a half (exact in float32, so neither end is reached by rounding)
__device__ inline float u23(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }
// one standard normal of a word pair (Box-Muller: normal4's first component)
__device__ inline float normal1(uint32_t wx, uint32_t wy) {
  const float u1 = ((float)(wx >> 8) + 1.0f) * 5.9604644775390625e-08f;
  return __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1)) * __builtin_amdgcn_cosf(u24(wy));
}

// Gamma(shape, 1): Marsaglia & Tsang (2000), "A simple method for generating gamma variables"; below shape 1 the draw of shape + 1
// times u^(1 / shape).  Acceptance is above 95 % at every shape >= 1; after the last attempt the mean of the proposal's law.
__device__ inline float gamma_unit(const SampleCtr& c, float shape, float u_boost) {
  const bool low = shape < 1.f;
  const float a = low ? shape + 1.f : shape;
  const float d = a - 0.33333334f, cc = 1.f / sqrtf(9.f * d);
  float g = a;
  for (int t = 0; t < SAMPLE_GAMMA_ATTEMPTS; ++t) {
    const U4 w = sample_block(c, AT_GAMMA + t);
    const float x = normal1(w.x, w.y), u = u23(w.z);
    const float t1 = 1.f + cc * x, v = t1 * t1 * t1, x2 = x * x;
    if (v > 0.f && (u < 1.f - 0.0331f * x2 * x2 || logf(u) < 0.5f * x2 + d * (1.f - v + logf(v)))) { g = d * v; break; }
  }
  return low ? g * expf(logf(u_boost) / shape) : g;   // (shape 0: u^inf = 0)
}

// log of the Poisson pmf at an integer k >= 0 for the PTRS test, without lgamma: Stirling's series, and the two large terms k log(rate / k)
// and k - rate taken together through log1p (each is ~|k - rate|, their sum ~(k - rate)^2 / 2k: no cancellation at rates of 10^6)
__device__ inline float poisson_log_pmf(float k, float rate) {
  if (k == 0.f) return -rate;
  const float dk = k - rate, ik = 1.f / k, ik2 = ik * ik;
  const float corr = ik * (0.083333336f - ik2 * (0.0027777778f - ik2 * 0.00079365081f));
  return dk + k * log1pf(-dk * ik) - 0.5f * logf(6.2831855f * k) - corr;
}

// Poisson(rate).  Below 10: inversion from 0 by p(k + 1) = p(k) rate / (k + 1) -- single-cell rates are mostly below 1, where the first
// comparison ends it.  The search also stops where the pmf has fallen under the uniform's resolution past the mode (rounding in the
// running difference must not walk a lane out to the step bound).  From 10: PTRS (Hoermann 1993, "The transformed rejection method for
// generating Poisson random variables"), after the last attempt the rounded rate.  From 2^22: the rounded normal.
__device__ inline float poisson_draw(const SampleCtr& c, float rate, float u_inv) {
  if (!(rate < INFINITY) || rate < 0.f) return NAN;   // (NaN and inf)
  if (rate < SAMPLE_INVERSION_BELOW) {
    float p = expf(-rate), u = u_inv, k = 0.f;
    for (int i = 0; i < SAMPLE_INVERSION_STEPS; ++i) {
      if (u <= p || (p < 3e-9f && k > rate)) break;
      u -= p; k += 1.f; p *= rate / k;
    }
    return k;
  }
  const float sr = sqrtf(rate);
  if (rate >= SAMPLE_NORMAL_FROM) {
    const U4 w = sample_block(c, AT_POISSON);
    return fmaxf(rintf(rate + sr * normal1(w.x, w.y)), 0.f);
  }
  const float b = 0.931f + 2.53f * sr, a = -0.059f + 0.02483f * b, inv_alpha = 1.1239f + 1.1328f / (b - 3.4f), vr = 0.9277f - 3.6224f / (b - 2.f);
  float k = rintf(rate);
  for (int t = 0; t < SAMPLE_PTRS_ATTEMPTS; ++t) {
    const U4 w = sample_block(c, AT_POISSON + t);
    const float U = u23(w.x) - 0.5f, V = u23(w.y), us = 0.5f - fabsf(U);
    const float kk = floorf((2.f * a / us + b) * U + rate + 0.43f);
    if (us >= 0.07f && V <= vr) { k = kk; break; }
    if (kk < 0.f || (us < 0.013f && V > us)) continue;
    if (logf(V * inv_alpha / (a / (us * us) + b)) <= poisson_log_pmf(kk, rate)) { k = kk; break; }
  }
  return k;
}

// One gene per lane, planes read once per (draw, cell, gene) and kept in registers over the n_k samples; grid (genes / 256, cells, draws).
// Lanes of a wave part ways in the rejection loops only.
__global__ __launch_bounds__(256) void plane_sample_kernel(SampleArgs a) {
  const int g = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, s = blockIdx.z;
  if (g >= a.G) return;
  const int lk = a.lk;
  const bool count = lk <= SMX_LLK_ZINBD, gated = (lk == SMX_LLK_ZINB || lk == SMX_LLK_ZINBD) && !a.count_only;
  const float* p = a.P + ((long)s * a.B + b) * a.ldp + g;
  const float p0 = p[0], p1 = (lk == SMX_LLK_MSE || lk == SMX_LLK_BERNOULLI) ? 0.f : p[a.plane_stride], p2 = gated ? p[2 * a.plane_stride] : 0.f;
  float shape = 0.f, scale = 0.f, pi = 0.f;   // count outputs: the Gamma's parameters, the gate probability; bernoulli: pi = P(1); normal: scale
  if (lk == SMX_LLK_NB || lk == SMX_LLK_ZINB) { shape = expf(p0); scale = expf(p1); }
  else if (count) {
    const float mu = a.direct ? p0 : softplus_sigmoid(p0).sp, th = a.direct ? p1 : softplus_sigmoid(p1 + SMX_SOFTPLUS_INV_1).sp;
    shape = th; scale = mu / th;
  } else if (lk == SMX_LLK_NORMAL) scale = softplus_sigmoid(p1 + SMX_SOFTPLUS_INV_1).sp;
  if (gated) pi = 1.f / (1.f + expf(-p2));
  if (lk == SMX_LLK_BERNOULLI) pi = 1.f / (1.f + expf(-p0));
  SampleCtr c{(uint32_t)g, a.row0 + (uint32_t)b, 0u, (uint32_t)ST_PREDICTIVE | ((a.s0 + (uint32_t)s) << 16), a.k0, a.k1};
  float* d = a.dst + (long)s * a.dst_draw + (long)b * a.G + g;
  for (int k = 0; k < a.n_k; ++k) {
    c.k = (uint32_t)k;
    float x = p0;   // 'mse'
    if (lk != SMX_LLK_MSE) {
      const U4 w = sample_block(c, AT_FIXED);
      if (count) {
        if (pi != pi) x = NAN;
        else if (gated && u24(w.x) < pi) x = 0.f;
        else {
          const float gm = gamma_unit(c, shape, u23(w.y));
          x = poisson_draw(c, (gm == 0.f && scale == scale) ? 0.f : gm * scale, u23(w.z));   // (a Gamma draw that underflowed is 0 whatever the scale)
        }
      } else if (lk == SMX_LLK_BERNOULLI) x = pi != pi ? NAN : (u24(w.x) < pi ? 1.f : 0.f);
      else { x = p0 + scale * normal1(w.x, w.y); if (!(fabsf(x) < INFINITY)) x = NAN; }   // (an infinite location or scale: NaN)
    }
    d[(long)k * a.dst_k] = x;
  }
}

int launch_plane_sample(hipStream_t st, const SampleArgs& a) {
  SMX_REQUIRE(a.P && a.dst && a.B > 0 && a.B <= 65535 && a.Sn > 0 && a.Sn <= 65535 && a.G > 0 && a.n_k > 0, "plane_sample: bad shape");
  SMX_REQUIRE((uint64_t)a.s0 + (uint64_t)a.Sn <= 65536, "plane_sample: the draw index has 16 bits of the counter");
  hipLaunchKernelGGL(plane_sample_kernel, dim3((unsigned)((a.G + 255) / 256), (unsigned)a.B, (unsigned)a.Sn), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

}  // namespace smx

extern "C" {

int smx_k_plane_sample(int likelihood, int direct, int count_only, const float* planes, int32_t rows, int32_t G, uint64_t seed, int32_t n_k,
                       float* out) {
  SMX_REQUIRE(planes && out && rows > 0 && rows <= 65535 && G > 0 && n_k > 0, "bad arguments");
  SMX_REQUIRE(likelihood >= SMX_LLK_NB && likelihood <= SMX_LLK_NORMAL, "unknown likelihood");
  const int k = llk_planes(likelihood), Gp = round_up(G, 32);
  DeviceScratch buf;
  float *dPl, *dOut;
  SMX_CHECK(buf.get(&dPl, (size_t)rows * k * Gp));
  SMX_CHECK(buf.get(&dOut, (size_t)n_k * rows * G));
  for (int c = 0; c < k; ++c)
    if (hipMemcpy2D(dPl + (size_t)c * Gp, (size_t)k * Gp * 4, planes + (size_t)c * rows * G, (size_t)G * 4, (size_t)G * 4, (size_t)rows,
                    hipMemcpyHostToDevice) != hipSuccess) { set_error("smx_k_plane_sample: copy of the planes failed"); return SMX_ERR_HIP; }
  SampleArgs a;
  a.P = dPl; a.ldp = (long)k * Gp; a.plane_stride = Gp; a.B = rows; a.Sn = 1; a.G = G; a.lk = likelihood; a.direct = direct ? 1 : 0;
  a.count_only = count_only ? 1 : 0; a.n_k = n_k; a.k0 = (uint32_t)(seed & 0xFFFFFFFFu); a.k1 = (uint32_t)(seed >> 32);
  a.dst = dOut; a.dst_k = (long)rows * G; a.dst_draw = 0;
  SMX_CHECK(launch_plane_sample(nullptr, a));
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, dOut, (size_t)n_k * rows * G * 4, hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("smx_k_plane_sample: the kernel or the copy of its result failed"); return SMX_ERR_HIP;
  }
  return SMX_OK;
}

}  // extern "C"
