// smx_latent.hip -- the latent heads (gfx950): the diagonal-Gaussian head (softplus1, reparameterised sample (Philox), analytic KL:
// a-7; deterministic DCA latent: a-14), the mixture posterior, the SCALE prior (diagonal and tril), scVI's library latent.
#include "smx_internal.h"

namespace smx {

// ===========================================================================
// Latent head.  One wave per cell, lanes over latent dims.
// ===========================================================================
// one lane = 4 consecutive latent dims of one cell (one Philox block, 16-byte accesses); the Dp/4 lanes of a
// cell are adjacent, so the KL sum is a short shuffle reduction.  Dp/4 is a power of two <= 64 (Dp in {32, 64,
// 128, 256}); other widths take the scalar kernel below.
__global__ __launch_bounds__(64) void latent_fwd_quad_kernel(LatentArgs a) {
  const int dq = a.Dp >> 2;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  const int b = idx / dq, d0 = (idx % dq) * 4;
  float kl = 0.f;
  if (b < a.B) {
    float zz[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {1.f, 1.f, 1.f, 1.f}, ee[4] = {0.f, 0.f, 0.f, 0.f};
    const float4 m4 = *reinterpret_cast<const float4*>(a.lat + (long)b * a.ld + d0);
    const float mu[4] = {m4.x, m4.y, m4.z, m4.w};
    if (a.stochastic) {
      const float4 s4 = *reinterpret_cast<const float4*>(a.lat + (long)b * a.ld + a.Dp + d0);
      const float sr[4] = {s4.x, s4.y, s4.z, s4.w};
      float4 n4;
      if (a.inj_eps) n4 = *reinterpret_cast<const float4*>(a.inj_eps + (long)b * a.inj_ld + d0);
      else n4 = normal4(philox_row(a.nk, (uint32_t)b, a.cell_base + (uint32_t)(a.rows ? a.rows[b] : b), (uint32_t)(d0 >> 2)));
      const float nn[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (d0 + e < a.D) {
          const float xs = sr[e] + SMX_SOFTPLUS_INV_1;
          const float sg = latent_sigma(xs);
          ss[e] = sg; ee[e] = nn[e];
          zz[e] = mu[e] + sg * nn[e];
          kl += 0.5f * (sg * sg + mu[e] * mu[e] - 1.f - 2.f * log_sigma_fast(xs, sg));
        }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (d0 + e < a.D) zz[e] = a.relu ? fmaxf(mu[e], 0.f) : mu[e];
    }
    const long o = (long)b * a.Dp + d0;
    *reinterpret_cast<float4*>(a.z + o) = make_float4(zz[0], zz[1], zz[2], zz[3]);
    if (a.sig) {
      *reinterpret_cast<float4*>(a.sig + o) = make_float4(ss[0], ss[1], ss[2], ss[3]);
      *reinterpret_cast<float4*>(a.eps + o) = make_float4(ee[0], ee[1], ee[2], ee[3]);
    }
  }
  for (int off = 1; off < dq; off <<= 1) kl += __shfl_xor(kl, off, 64);
  if (b < a.B && (idx % dq) == 0 && a.kl) a.kl[b] = kl;
}

__global__ __launch_bounds__(256) void latent_fwd_kernel(LatentArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  float kl = 0.f;
  const uint32_t cell = a.cell_base + (uint32_t)(a.rows ? a.rows[b] : b);
  for (int d = lane; d < a.Dp; d += 64) {
    const long o = (long)b * a.Dp + d;
    float z = 0.f, sig = 1.f, eps = 0.f;
    if (d < a.D) {
      const float mu = a.lat[(long)b * a.ld + d];
      if (a.stochastic) {
        const float xs = a.lat[(long)b * a.ld + a.Dp + d] + SMX_SOFTPLUS_INV_1;
        sig = latent_sigma(xs);
        if (a.inj_eps) eps = a.inj_eps[(long)b * a.inj_ld + d];
        else {
          const float4 n = normal4(philox_row(a.nk, (uint32_t)b, cell, (uint32_t)(d >> 2)));
          eps = (d & 3) == 0 ? n.x : (d & 3) == 1 ? n.y : (d & 3) == 2 ? n.z : n.w;
        }
        z = mu + sig * eps;
        kl += 0.5f * (sig * sig + mu * mu - 1.f - 2.f * log_sigma_fast(xs, sig));
      } else {
        z = a.relu ? fmaxf(mu, 0.f) : mu;
      }
    }
    a.z[o] = z;
    if (a.sig) { a.sig[o] = sig; a.eps[o] = eps; }
  }
  kl = wave_sum(kl);
  if (lane == 0 && a.kl) a.kl[b] = kl;
}

int launch_latent_fwd(hipStream_t st, const LatentArgs& a) {
  const int dq = a.Dp >> 2;
  if (dq >= 1 && dq <= 64 && (dq & (dq - 1)) == 0 && (a.ld % 4) == 0 && (!a.inj_eps || (a.inj_ld % 4) == 0)) {
    hipLaunchKernelGGL(latent_fwd_quad_kernel, dim3((a.B * dq + 63) / 64), dim3(64), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  hipLaunchKernelGGL(latent_fwd_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ---- SCALE with a mixture-density POSTERIOR (MixLatArgs): one wave per cell, lane d = latent dimension d ----------------------
__device__ inline void mixlat_softmax(const MixLatArgs& a, const float* lat, int lane, float& logpi, float& pi) {
  const float lg = lane < a.C ? lat[lane] : -3.0e38f;
  const float mx = wave_max(lg);
  const float ex = lane < a.C ? fexp(lg - mx) : 0.f;
  const float se = wave_sum(ex);
  logpi = lg - mx - flog(se);
  pi = ex * frcp(se);
}
__global__ __launch_bounds__(256) void mixlat_fwd_kernel(MixLatArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const float HALF_LOG_2PI = 0.9189385332046727f;
  const float* lat = a.lat + (long)b * a.ld;
  const uint32_t cell = a.cell_base + (uint32_t)(a.rows ? a.rows[b] : b);
  float logpi, pi;
  mixlat_softmax(a, lat, lane, logpi, pi);
  // the component: the first c whose running sum of pi reaches the cell's uniform (sums in component order)
  const float u = u24(philox_row(a.nk_pick, (uint32_t)b, cell, 0u).x);
  int k = 0;
  float run = 0.f;
  for (int c = 0; c < a.C; ++c) {
    run += lane_bcast(pi, c);
    k += (run < u) ? 1 : 0;
  }
  k = min(k, a.C - 1);
  const bool live = lane < a.D;
  float eps = 0.f;
  if (live) {
    if (a.inj_eps) eps = a.inj_eps[(long)b * a.inj_ld + lane];
    else {
      const float4 n = normal4(philox_row(a.nk, (uint32_t)b, cell, (uint32_t)(lane >> 2)));
      eps = (lane & 3) == 0 ? n.x : (lane & 3) == 1 ? n.y : (lane & 3) == 2 ? n.z : n.w;
    }
  }
  float mu[8], sg[8];
  float z = 0.f, mean = 0.f, second = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    mu[c] = 0.f; sg[c] = 1.f;
    if (c < a.C) {   // (uniform)
      if (live) { mu[c] = lat[(1 + c) * a.Dp + lane]; sg[c] = softplusf(lat[(1 + a.C + c) * a.Dp + lane] + SMX_SOFTPLUS_INV_1); }
      const float pc = lane_bcast(pi, c);
      mean += pc * mu[c];
      second += pc * (sg[c] * sg[c] + mu[c] * mu[c]);
      if (c == k) z = mu[c] + sg[c] * eps;
    }
  }
  float comp_mine = -3.0e38f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c < a.C) {
      const float dzm = (z - mu[c]) * frcp(sg[c]);
      const float t = wave_sum(live ? -0.5f * dzm * dzm - flog(sg[c]) - HALF_LOG_2PI : 0.f) + lane_bcast(logpi, c);
      if (lane == c) comp_mine = t;
    }
  }
  const float cmx = wave_max(comp_mine);
  const float log_q = cmx + flog(wave_sum(lane < a.C ? fexp(comp_mine - cmx) : 0.f));
  const float log_p = wave_sum(live ? -0.5f * z * z - HALF_LOG_2PI : 0.f);
  if (lane < 32) a.resp[(long)b * 32 + lane] = lane < a.C ? fexp(comp_mine - log_q) : 0.f;
  if (lane == 0) { a.kl[b] = log_q - log_p; a.pick[b] = k; }
  for (int d = lane; d < a.Dp; d += 64) {   // (d == lane for d < D <= 64)
    const long o = (long)b * a.Dp + d;
    a.z[o] = d < a.D ? z : 0.f;
    a.eps[o] = d < a.D ? eps : 0.f;
    a.zmean[o] = d < a.D ? mean : 0.f;
    a.zstd[o] = d < a.D ? fsqrt(fmaxf(second - mean * mean, 0.f)) : 1.f;
  }
}
// d lat from d z: log q depends on z and on every component's parameters, z on the picked component's (mu_k, sigma_k) only
__global__ __launch_bounds__(256) void mixlat_bwd_kernel(MixLatArgs a) {
  const float kls = kl_scale_of(a.klw);
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const float* lat = a.lat + (long)b * a.ld;
  float* dl = a.dlat + (long)b * a.ld;
  float logpi, pi;
  mixlat_softmax(a, lat, lane, logpi, pi);
  const float rme = lane < a.C ? a.resp[(long)b * 32 + lane] : 0.f;
  const int k = a.pick[b];
  const bool live = lane < a.D;
  float dz = 0.f;
  if (live) for (int s = 0; s < a.dz_slabs; ++s) dz += a.dz[(long)s * a.dz_slab_stride + (long)b * a.ldz + lane];
  const float z = live ? a.z[(long)b * a.Dp + lane] : 0.f, eps = live ? a.eps[(long)b * a.Dp + lane] : 0.f;
  float mu[8], sg[8], sraw[8];
  float dqz = 0.f;   // d log q / d z_d = -sum_c r_c (z - mu_c) / sigma_c^2
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    mu[c] = 0.f; sg[c] = 1.f; sraw[c] = 0.f;
    if (c < a.C) {
      if (live) { mu[c] = lat[(1 + c) * a.Dp + lane]; sraw[c] = lat[(1 + a.C + c) * a.Dp + lane]; sg[c] = softplusf(sraw[c] + SMX_SOFTPLUS_INV_1); }
      const float is = frcp(sg[c]);
      dqz -= lane_bcast(rme, c) * (z - mu[c]) * is * is;
    }
  }
  const float g = dz + kls * (z + dqz);
  for (int d = lane; d < a.Dp; d += 64) dl[d] = d < a.C ? kls * (rme - pi) : 0.f;   // plane 0: logits (d == lane)
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c < a.C) {
      const float rc = lane_bcast(rme, c), is = frcp(sg[c]);
      const float dzm = (z - mu[c]) * is;
      float dmu = kls * rc * dzm * is, dsg = kls * rc * (dzm * dzm - 1.f) * is;
      if (c == k) { dmu += g; dsg += g * eps; }
      for (int d = lane; d < a.Dp; d += 64) {
        dl[(1 + c) * a.Dp + d] = d < a.D ? dmu : 0.f;
        dl[(1 + a.C + c) * a.Dp + d] = d < a.D ? dsg * sigmoidf(sraw[c] + SMX_SOFTPLUS_INV_1) : 0.f;
      }
    }
  }
}
static bool mixlat_ok(const MixLatArgs& a) {
  return a.B > 0 && a.C >= 2 && a.C <= 8 && a.D >= a.C && a.D <= 64 && a.Dp <= 64 && a.ld == (1 + 2 * a.C) * a.Dp && a.lat && a.z && a.eps && a.resp && a.pick;
}
int launch_mixlat_fwd(hipStream_t st, const MixLatArgs& a) {
  if (!mixlat_ok(a) || !a.kl || !a.zmean || !a.zstd) { set_error("mixlat_fwd: bad arguments (2..8 components <= latent_dim <= 64)"); return SMX_ERR_INVALID; }
  hipLaunchKernelGGL(mixlat_fwd_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
int launch_mixlat_bwd(hipStream_t st, const MixLatArgs& a) {
  if (!mixlat_ok(a) || !a.dz || !a.dlat || a.dz_slabs < 1) { set_error("mixlat_bwd: bad arguments"); return SMX_ERR_INVALID; }
  hipLaunchKernelGGL(mixlat_bwd_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ---- RVmeta(D, 'mvntril'): the full-covariance posterior (LatentTrilArgs) ------------------------------------------------------------
// Half a wave per cell (two cells per wave64, SMX_LTRIL_CELLS per workgroup), lane i of the half = row i of L (D <= 32 = Dp).  Lane i reads
// row i of the raw factor as eight 16-byte loads; a triangular mat-vec is at most 528 FMAs per cell.  The whole workgroup runs to the end
// (cells past B and rows past D compute on zeros): half_wave_sum needs both halves of a wave.
#define SMX_LTRIL_CELLS 8
// row i of the raw factor of cell b (plane 1 + i; zeros for a row past D, whose plane does not exist)
__device__ inline void ltril_row(const LatentTrilArgs& a, int b, int i, bool on, float (&r)[32]) {
  const float4* row = reinterpret_cast<const float4*>(a.lat + (long)b * a.ld + (long)(1 + (on ? i : 0)) * 32);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 q = row[k];
    r[4 * k] = on ? q.x : 0.f; r[4 * k + 1] = on ? q.y : 0.f; r[4 * k + 2] = on ? q.z : 0.f; r[4 * k + 3] = on ? q.w : 0.f;
  }
}
// z = mu + L eps with the diagonal path's eps (lane i draws eps_i; eps_j for j < i from one LDS row of the cell, read as broadcasts);
// KL = 1/2 (|L|_F^2 + |mu|^2 - D) - sum_i log L_ii as one half-wave sum of the rows' terms
__global__ __launch_bounds__(256) void latent_tril_fwd_kernel(LatentTrilArgs a) {
  __shared__ float4 se4[SMX_LTRIL_CELLS][8];
  const int i = threadIdx.x & 31, c = threadIdx.x >> 5;
  const int b = blockIdx.x * SMX_LTRIL_CELLS + c;
  const bool cell_on = b < a.B, on = cell_on && i < a.D;
  const int bb = cell_on ? b : a.B - 1;
  float raw[32];
  ltril_row(a, bb, i, on, raw);
  const float mu = on ? a.lat[(long)bb * a.ld + i] : 0.f;
  float eps = 0.f;
  if (on) {
    if (a.inj_eps) eps = a.inj_eps[(long)b * a.inj_ld + i];
    else {
      const uint32_t cell = a.cell_base + (uint32_t)(a.rows ? a.rows[b] : b);
      const float4 n = normal4(philox_row(a.nk, (uint32_t)b, cell, (uint32_t)(i >> 2)));
      eps = (i & 3) == 0 ? n.x : (i & 3) == 1 ? n.y : (i & 3) == 2 ? n.z : n.w;
    }
  }
  reinterpret_cast<float*>(se4[c])[i] = eps;
  __syncthreads();
  float acc = 0.f, fro = 0.f, rii = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 e4 = se4[c][k];
    const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * k + t;
      if (j < i) { acc += raw[j] * ev[t]; fro += raw[j] * raw[j]; }
      else if (j == i) rii = raw[j];
    }
  }
  const float lii = softplusf(rii) + 1e-5f;
  const float z = mu + acc + lii * eps;
  const float kl = half_wave_sum(on ? 0.5f * (fro + lii * lii + mu * mu - 1.f) - flog(lii) : 0.f);
  if (cell_on) {
    const long o = (long)b * a.Dp + i;   // (Dp = 32: lane i owns column i of the padded rows)
    a.z[o] = on ? z : 0.f;
    a.diag[o] = on ? lii : 1.f;
    a.eps[o] = eps;
    if (i == 0 && a.kl) a.kl[b] = kl;
    if (a.factor && on) {
      float* f = a.factor + ((long)b * a.D + i) * a.D;
#pragma unroll
      for (int j = 0; j < 32; ++j)
        if (j < a.D) f[j] = j < i ? raw[j] : j == i ? lii : 0.f;
    }
  }
}
// d mu = dz + k mu;  d raw_ij = dz_i eps_j + k L_ij (j < i);  d raw_ii = (dz_i eps_i + k (L_ii - 1 / L_ii)) sigmoid(raw_ii);  j > i: 0.
// dz summed over its slabs; lane i stores its row of d raw whole (eight 16-byte stores)
__global__ __launch_bounds__(256) void latent_tril_bwd_kernel(LatentTrilArgs a) {
  const float kls = kl_scale_of(a.klw);
  const int i = threadIdx.x & 31, c = threadIdx.x >> 5;
  const int b = blockIdx.x * SMX_LTRIL_CELLS + c;
  if (b >= a.B) return;   // (no cross-lane step below)
  const bool on = i < a.D;
  float raw[32], e[32];
  ltril_row(a, b, i, on, raw);
  const float4* erow = reinterpret_cast<const float4*>(a.eps + (long)b * a.Dp);   // (the same row in every lane of the half: broadcasts)
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 q = erow[k];
    e[4 * k] = q.x; e[4 * k + 1] = q.y; e[4 * k + 2] = q.z; e[4 * k + 3] = q.w;
  }
  float dz = 0.f;
  if (on) for (int s = 0; s < a.dz_slabs; ++s) dz += a.dz[(long)s * a.dz_slab_stride + (long)b * a.ldz + i];
  const float mu = on ? a.lat[(long)b * a.ld + i] : 0.f;
  const float lii = on ? a.diag[(long)b * a.Dp + i] : 1.f;
  float* dl = a.dlat + (long)b * a.ld;
  dl[i] = on ? dz + kls * mu : 0.f;   // plane 0
  if (!on) return;
  float rii = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) if (j == i) rii = raw[j];
  const float sg = softplus_sigmoid(rii).sg;
#pragma unroll
  for (int j = 0; j < 32; ++j)
    raw[j] = j < i ? dz * e[j] + kls * raw[j] : j == i ? (dz * e[j] + kls * (lii - frcp(lii))) * sg : 0.f;
  float4* drow = reinterpret_cast<float4*>(dl + (long)(1 + i) * 32);
#pragma unroll
  for (int k = 0; k < 8; ++k) drow[k] = make_float4(raw[4 * k], raw[4 * k + 1], raw[4 * k + 2], raw[4 * k + 3]);
}
static bool latent_tril_ok(const LatentTrilArgs& a) {
  return a.B > 0 && a.D >= 1 && a.D <= 32 && a.Dp == 32 && a.ld == (1 + a.D) * a.Dp && a.lat && a.z && a.diag && a.eps &&
         (!a.inj_eps || a.inj_ld >= a.D);
}
int launch_latent_tril_fwd(hipStream_t st, const LatentTrilArgs& a) {
  if (!latent_tril_ok(a)) { set_error("latent_tril_fwd: bad arguments (1 <= latent_dim <= 32, a head of 1 + latent_dim planes of width 32)"); return SMX_ERR_INVALID; }
  hipLaunchKernelGGL(latent_tril_fwd_kernel, dim3((a.B + SMX_LTRIL_CELLS - 1) / SMX_LTRIL_CELLS), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
int launch_latent_tril_bwd(hipStream_t st, const LatentTrilArgs& a) {
  if (!latent_tril_ok(a) || !a.dz || !a.dlat || a.dz_slabs < 1 || a.ldz < a.D) { set_error("latent_tril_bwd: bad arguments"); return SMX_ERR_INVALID; }
  hipLaunchKernelGGL(latent_tril_bwd_kernel, dim3((a.B + SMX_LTRIL_CELLS - 1) / SMX_LTRIL_CELLS), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

__global__ __launch_bounds__(256) void latent_bwd_kernel(LatentArgs a) {
  const float kls = kl_scale_of(a.klw);
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.B * a.Dp) return;
  const int b = idx / a.Dp, d = idx % a.Dp;
  float dz = 0.f;
  for (int s = 0; s < a.dz_slabs; ++s) dz += a.dz[(long)s * a.dz_slab_stride + idx];
  if (a.stochastic) {
    float dmu = 0.f, ds = 0.f;
    if (d < a.D) {
      const float mu = a.lat[(long)b * a.ld + d];
      const float sraw = a.lat[(long)b * a.ld + a.Dp + d];
      const float sig = a.sig[idx], eps = a.eps[idx];
      dmu = dz + kls * mu;
      ds = (dz * eps + kls * (sig - frcp(sig))) * sigmoidf(sraw + SMX_SOFTPLUS_INV_1);
    }
    a.dlat[(long)b * a.ld + d] = dmu;
    a.dlat[(long)b * a.ld + a.Dp + d] = ds;
  } else {
    float g = 0.f;
    if (d < a.D) g = (a.relu && !(a.lat[(long)b * a.ld + d] > 0.f)) ? 0.f : dz;
    a.dlat[(long)b * a.ld + d] = g;
  }
}

int launch_latent_bwd(hipStream_t st, const LatentArgs& a) {
  hipLaunchKernelGGL(latent_bwd_kernel, dim3((a.B * a.Dp + 255) / 256), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ---- SCALE: Gaussian-mixture prior, one-sample Monte-Carlo KL (scale.py:13-49; Xiong et al. 2019) -------------------
// one wave per cell; lanes over the latent dims; the C (<= 32) components are walked serially (C D ~ 100 terms)
__global__ __launch_bounds__(256) void scale_prior_fwd_kernel(ScalePriorArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const float HALF_LOG_2PI = 0.9189385332046727f;
  // log softmax of the mixture logits (lane c holds logit c)
  const float lg = lane < a.C ? a.logits[lane] : -3.0e38f;
  const float lmx = wave_max(lg);
  const float lse = lmx + flog(wave_sum(lane < a.C ? fexp(lg - lmx) : 0.f));
  float comp_mine = -3.0e38f;          // lane c keeps component c's joint log density
  if (a.D <= 64) {
    // (eight components' parameters requested together: a load pair per component inside the loop was a chain of C dependent
    // memory round trips -- 13 us per launch at 10 components)
    const bool live = lane < a.D;
    const float zd = live ? a.z[(long)b * a.Dp + lane] : 0.f;
    for (int c0 = 0; c0 < a.C; c0 += 8) {
      float sr[8], lc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool on = live && c0 + k < a.C;
        sr[k] = on ? a.scale_raw[(long)(c0 + k) * a.Dp + lane] : 0.f;
        lc[k] = on ? a.loc[(long)(c0 + k) * a.Dp + lane] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (c0 + k < a.C) {   // (uniform)
          const float s = softplusf(sr[k] + SMX_SOFTPLUS_INV_1);
          const float u = (zd - lc[k]) * frcp(s);
          const float t = wave_sum(live ? -0.5f * u * u - flog(s) - HALF_LOG_2PI : 0.f) + (a.logits[c0 + k] - lse);
          if (lane == c0 + k) comp_mine = t;
        }
      }
    }
  } else
  for (int c = 0; c < a.C; ++c) {
    float t = 0.f;
    for (int d = lane; d < a.D; d += 64) {
      const float s = softplusf(a.scale_raw[(long)c * a.Dp + d] + SMX_SOFTPLUS_INV_1);
      const float u = (a.z[(long)b * a.Dp + d] - a.loc[(long)c * a.Dp + d]) * frcp(s);
      t += -0.5f * u * u - flog(s) - HALF_LOG_2PI;
    }
    t = wave_sum(t) + (a.logits[c] - lse);
    if (lane == c) comp_mine = t;
  }
  const float cmx = wave_max(comp_mine);
  const float log_p = cmx + flog(wave_sum(lane < a.C ? fexp(comp_mine - cmx) : 0.f));
  const float resp = lane < a.C ? fexp(comp_mine - log_p) : 0.f;
  if (lane < 32) a.resp[(long)b * 32 + lane] = resp;
  float lq = 0.f;
  for (int d = lane; d < a.D; d += 64) {
    const float e = a.eps[(long)b * a.Dp + d];
    lq += -0.5f * e * e - flog(a.sig[(long)b * a.Dp + d]) - HALF_LOG_2PI;
  }
  lq = wave_sum(lq);
  if (lane == 0) a.kl[b] = lq - log_p;
  // d(-log p)/dz_d = sum_c resp_c (z_d - m_cd) / s_cd^2
  for (int d = lane; d < a.Dp; d += 64) {
    float g = 0.f;
    const float zd = a.z[(long)b * a.Dp + d];
    for (int c0 = 0; c0 < a.C; c0 += 8) {   // (every lane takes part in the broadcasts; padded dims contribute nothing)
      float sr[8], lc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool on = d < a.D && c0 + k < a.C;
        sr[k] = on ? a.scale_raw[(long)(c0 + k) * a.Dp + d] : 0.f;
        lc[k] = on ? a.loc[(long)(c0 + k) * a.Dp + d] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (c0 + k < a.C) {
          const float rc = lane_bcast(resp, c0 + k);
          const float s = softplusf(sr[k] + SMX_SOFTPLUS_INV_1);
          g += (d < a.D) ? rc * (zd - lc[k]) * frcp(s * s) : 0.f;
        }
      }
    }
    a.dklz[(long)b * a.Dp + d] = g;
  }
}
// ---- covariance = 'tril' (scale.py:28,35): component c = N(m_c, L_c L_c^T), diag L = softplus(raw) + 1e-5, strict lower triangle raw ----
// One wave per cell, lane p = latent dimension p (D <= 32); the component's factor sits in the wave's LDS tile [D][D + 1].
//   u = L^-1 (z - m) forward substitution, w = L^-T u back substitution;  log N = -1/2 |u|^2 - sum log L_pp - D/2 log 2 pi
//   d(-log p)/dz = sum_c resp_c w_c.  Two sweeps over the components (densities -> responsibilities, then the gradient): C D^2 is small.
// lane p fetches row p of L_c: eight 16-byte loads, all in flight at once (a load per entry, each followed by its LDS store, was a
// chain of D dependent memory round trips per component: 566 us per step at D = 32, C = 10)
struct TrilRow { float4 q[8]; };
__device__ inline TrilRow tril_fetch(const ScalePriorArgs& a, int c, int lane) {
  TrilRow r;
  const float4* row = reinterpret_cast<const float4*>(a.scale_raw + ((long)c * a.D + (lane < a.D ? lane : 0)) * a.Dp);   // (Dp = 32)
#pragma unroll
  for (int k = 0; k < 8; ++k) r.q[k] = row[k];
  return r;
}
__device__ inline void tril_store(const ScalePriorArgs& a, const TrilRow& r, int lane, float* L, float& lpp, float& sg) {
  const int D = a.D, ldl = D + 1;
  lpp = 1.f; sg = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float e[4] = {r.q[k].x, r.q[k].y, r.q[k].z, r.q[k].w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * k + t;
      float v = e[t];
      if (j == lane) { const SpSg s = softplus_sigmoid(v); v = s.sp + 1e-5f; lpp = v; sg = s.sg; }
      if (lane < D && j < D) L[lane * ldl + j] = j <= lane ? v : 0.f;
    }
  }
}
__device__ inline void tril_load(const ScalePriorArgs& a, int c, int lane, float* L, float& lpp, float& sg) {
  const TrilRow r = tril_fetch(a, c, lane);
  tril_store(a, r, lane, L, lpp, sg);
}
// The two substitutions with the factor in REGISTERS (lane p: row p and column p, read once from the LDS tile) and the pivot
// broadcast by v_readlane: a step is multiply -> readlane -> fused multiply-add.  (Its first form read L from LDS inside the loop and
// broadcast with __shfl = ds_bpermute, two LDS round trips per step: ~330 cycles per step, 9 us per 32-dimensional solve.)
struct TrilRegs { float row[32]; float col[32]; };
__device__ inline void tril_regs(int D, int lane, const float* L, TrilRegs& t) {
  const int ldl = D + 1;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    t.row[j] = (lane < D && j < D) ? L[lane * ldl + j] : 0.f;    // (zero above the diagonal)
    t.col[j] = (lane < D && j < D) ? L[j * ldl + lane] : 0.f;    // L[j][lane]: zero for j < lane
  }
}
__device__ inline void tril_solve(int D, int lane, const TrilRegs& t, float lpp, float r, float& u, float& w) {
  const float inv = frcp(lpp);
  u = 0.f; w = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    if (j < D) {   // (uniform)
      const float uj = lane_bcast(r * inv, j);
      if (lane == j) u = uj;
      else if (lane > j) r -= t.row[j] * uj;
    }
  }
  float s = u;
#pragma unroll
  for (int i = 31; i >= 0; --i) {
    if (i < D) {
      const float wi = lane_bcast(s * inv, i);
      if (lane == i) w = wi;
      else if (lane < i) s -= t.col[i] * wi;
    }
  }
}
// forward: one WORKGROUP per cell, one wave per component (SMX_TRILF_WAVES at a time): a component's substitutions are ~4 000
// dependent instructions of one wave -- ten of them in a row per cell took 97 us, side by side they take one's time
#define SMX_TRILF_WAVES 12
__global__ __launch_bounds__(64 * SMX_TRILF_WAVES) void scale_prior_tril_fwd_kernel(ScalePriorArgs a) {
  extern __shared__ float sm[];   // waves x [D][D + 1] | w of every component [C][D] | joint log density of every component [32]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.x;
  const int D = a.D;
  float* L = sm + wv * D * (D + 1);
  float* Wc = sm + SMX_TRILF_WAVES * D * (D + 1);
  float* comp = Wc + a.C * D;
  const float HALF_LOG_2PI = 0.9189385332046727f;
  const float lg = lane < a.C ? a.logits[lane] : -3.0e38f;
  const float lmx = wave_max(lg);
  const float lse = lmx + flog(wave_sum(lane < a.C ? fexp(lg - lmx) : 0.f));
  const float zd = lane < D ? a.z[(long)b * a.Dp + lane] : 0.f;
  for (int c = wv; c < a.C; c += SMX_TRILF_WAVES) {
    float lpp, sg, u, w;
    tril_load(a, c, lane, L, lpp, sg);
    __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier();
    TrilRegs tr;
    tril_regs(D, lane, L, tr);
    tril_solve(D, lane, tr, lpp, zd - (lane < D ? a.loc[(long)c * a.Dp + lane] : 0.f), u, w);
    if (lane < D) Wc[c * D + lane] = w;
    const float t = wave_sum(lane < D ? -0.5f * u * u - flog(lpp) - HALF_LOG_2PI : 0.f) + (a.logits[c] - lse);
    if (lane == 0) comp[c] = t;
    __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier();   // (the tile is rewritten by this wave's next component)
  }
  __syncthreads();
  if (wv != 0) return;
  const float comp_mine = lane < a.C ? comp[lane] : -3.0e38f;
  const float cmx = wave_max(comp_mine);
  const float log_p = cmx + flog(wave_sum(lane < a.C ? fexp(comp_mine - cmx) : 0.f));
  const float resp = lane < a.C ? fexp(comp_mine - log_p) : 0.f;
  if (lane < 32) a.resp[(long)b * 32 + lane] = resp;
  float lq = 0.f;
  if (lane < D) {
    const float e = a.eps[(long)b * a.Dp + lane];
    lq = -0.5f * e * e - flog(a.sig[(long)b * a.Dp + lane]) - HALF_LOG_2PI;
  }
  lq = wave_sum(lq);
  if (lane == 0) a.kl[b] = lq - log_p;
  float g = 0.f;   // d(-log p)/dz = sum_c resp_c w_c
  for (int c = 0; c < a.C; ++c) g += lane_bcast(resp, c) * (lane < D ? Wc[c * D + lane] : 0.f);
  for (int d = lane; d < a.Dp; d += 64) a.dklz[(long)b * a.Dp + d] = d < D ? g : 0.f;   // (d == lane for d < D <= 32)
}
// gradients of the prior's parameters: a workgroup per (component, group of SMX_TRILB_CELLS cells) -- the factor once in registers,
// waves over the group's cells, lane p = row p -- leaves its partial sums in `part`; scale_prior_tril_reduce_kernel adds the groups
// in order (deterministic) and applies the diagonal's derivative.  (One workgroup per component walking all cells: 99 - 142 us.)
#define SMX_TRILB_WAVES 8
#define SMX_TRILB_CELLS 8
__global__ __launch_bounds__(64 * SMX_TRILB_WAVES) void scale_prior_tril_bwd_kernel(ScalePriorArgs a, float* gpart) {
  extern __shared__ float sm[];   // L [D][D + 1] | partial sums [waves][D][D + 2]
  const int c = blockIdx.x, grp = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int D = a.D, ldl = D + 1, lda = D + 2;
  float* L = sm;
  float* part = sm + D * ldl;
  float lpp = 1.f, sg = 0.f;
  if (wv == 0) tril_load(a, c, lane, L, lpp, sg);
  __syncthreads();
  if (wv != 0 && lane < D) { lpp = L[lane * ldl + lane]; }
  TrilRegs tr;
  tril_regs(D, lane, L, tr);
  float acc[32];   // row p of sum_b r (w u^T); [j = p] also carries the -r / L_pp term
#pragma unroll
  for (int j = 0; j < 32; ++j) acc[j] = 0.f;
  float g_loc = 0.f, g_lg = 0.f;
  const float mloc = lane < D ? a.loc[(long)c * a.Dp + lane] : 0.f;
  const float invl = frcp(lpp);
  const int b_end = min(a.B, (grp + 1) * SMX_TRILB_CELLS);
  for (int b = grp * SMX_TRILB_CELLS + wv; b < b_end; b += SMX_TRILB_WAVES) {
    const float rc = a.resp[(long)b * 32 + c];
    float u, w;
    tril_solve(D, lane, tr, lpp, (lane < D ? a.z[(long)b * a.Dp + lane] : 0.f) - mloc, u, w);
    g_loc += rc * w;
    g_lg += rc;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      if (j < D) {   // (uniform)
        const float uj = lane_bcast(u, j);
        acc[j] += rc * (w * uj - (j == lane ? invl : 0.f));
      }
    }
  }
  if (lane < D) {
#pragma unroll
    for (int j = 0; j < 32; ++j)
      if (j < D) part[(wv * D + lane) * lda + j] = acc[j];
    part[(wv * D + lane) * lda + D] = g_loc;
  }
  if (lane == 0) part[(wv * D) * lda + D + 1] = g_lg;
  __syncthreads();
  // this group's sums over its waves (wave order) -> gpart[c][grp][D][D + 2]
  float* out = gpart + ((long)c * gridDim.y + grp) * D * lda;
  for (int i = threadIdx.x; i < D * lda; i += 64 * SMX_TRILB_WAVES) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < SMX_TRILB_WAVES; ++q) t += part[q * D * lda + i];
    out[i] = t;
  }
}
__global__ __launch_bounds__(256) void scale_prior_tril_reduce_kernel(ScalePriorArgs a, const float* gpart, int n_grp) {
  const float kls = kl_scale_of(a.klw);
  const int c = blockIdx.x;
  const int D = a.D, lda = D + 2;
  const float* base = gpart + (long)c * n_grp * D * lda;
  for (int i = threadIdx.x; i < D * lda; i += 256) {   // one thread per entry of the component's [D][D + 2] sums, the groups in order
    float t = 0.f;
    for (int q0 = 0; q0 < n_grp; q0 += 8) {   // eight groups' loads in flight, added in group order
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = q0 + k < n_grp ? base[(long)(q0 + k) * D * lda + i] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) t += v[k];
    }
    const int p = i / lda, j = i - p * lda;
    if (j < D) {
      float g = 0.f;
      if (j < p) g = -kls * t;
      else if (j == p) g = -kls * t * sigmoidf(a.scale_raw[((long)c * D + p) * a.Dp + p]);
      a.g_scale[((long)c * D + p) * a.Dp + j] = g;
    } else if (j == D) {
      a.g_loc[(long)c * a.Dp + p] = -kls * t;
    } else if (p == 0) {   // j == D + 1: the sum of the responsibilities
      float mx = -3.0e38f;
      for (int q = 0; q < a.C; ++q) mx = fmaxf(mx, a.logits[q]);
      float se = 0.f;
      for (int q = 0; q < a.C; ++q) se += fexp(a.logits[q] - mx);
      a.g_logits[c] = kls * ((float)a.B * fexp(a.logits[c] - mx) * frcp(se) - t);
    }
  }
  for (int i = threadIdx.x; i < D * (a.Dp - D); i += 256) {   // the padded columns
    const int p = i / (a.Dp - D), j = D + i % (a.Dp - D);
    a.g_scale[((long)c * D + p) * a.Dp + j] = 0.f;
  }
  for (int d = D + (int)threadIdx.x; d < a.Dp; d += 256) a.g_loc[(long)c * a.Dp + d] = 0.f;
}

int launch_scale_prior_fwd(hipStream_t st, const ScalePriorArgs& a) {
  if (a.C < 2 || a.C > 32 || a.B <= 0) { set_error("scale prior: 2..32 components"); return SMX_ERR_INVALID; }
  if (a.tril) {
    if (a.D < 1 || a.D > 32) { set_error("scale prior: full-covariance components take at most 32 latent dimensions"); return SMX_ERR_INVALID; }
    if (a.Dp != 32) { set_error("scale prior: full-covariance components expect a 32-wide padded latent"); return SMX_ERR_INVALID; }
    hipLaunchKernelGGL(scale_prior_tril_fwd_kernel, dim3(a.B), dim3(64 * SMX_TRILF_WAVES), (size_t)(SMX_TRILF_WAVES * a.D * (a.D + 1) + a.C * a.D + 32) * sizeof(float), st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  hipLaunchKernelGGL(scale_prior_fwd_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
// gradients of the prior's parameters: one workgroup per component, lanes over the latent dims, waves over the cells
__global__ __launch_bounds__(256) void scale_prior_bwd_kernel(ScalePriorArgs a) {
  const float kls = kl_scale_of(a.klw);
  __shared__ float sh[4][3][64];
  const int c = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d0 = 0; d0 < a.Dp; d0 += 64) {
    const int d = d0 + lane;
    float g_loc = 0.f, g_sc = 0.f, g_lg = 0.f;
    const bool live = d < a.D;
    const float raw = live ? a.scale_raw[(long)c * a.Dp + d] : 0.f;
    const float s = softplusf(raw + SMX_SOFTPLUS_INV_1), m = live ? a.loc[(long)c * a.Dp + d] : 0.f;
    const float is = frcp(s);
    for (int b0 = w; b0 < a.B; b0 += 32) {   // eight of this wave's cells at a time: their loads in flight together
      float rcv[8], zv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int b = b0 + 4 * k;
        rcv[k] = b < a.B ? a.resp[(long)b * 32 + c] : 0.f;
        zv[k] = (b < a.B && live) ? a.z[(long)b * a.Dp + d] : m;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {   // (cell order as before: the sums keep their bits)
        if (b0 + 4 * k < a.B) {
          const float rc = rcv[k];
          if (live) {
            const float u = (zv[k] - m) * is;
            g_loc += rc * u * is;
            g_sc += rc * (u * u - 1.f) * is;
          }
          if (d0 == 0 && lane == 0) g_lg += rc;
        }
      }
    }
    sh[w][0][lane] = g_loc; sh[w][1][lane] = g_sc; sh[w][2][lane] = g_lg;
    __syncthreads();
    if (w == 0) {
      const float t0 = (sh[0][0][lane] + sh[1][0][lane]) + (sh[2][0][lane] + sh[3][0][lane]);
      const float t1 = (sh[0][1][lane] + sh[1][1][lane]) + (sh[2][1][lane] + sh[3][1][lane]);
      if (d < a.Dp) {
        a.g_loc[(long)c * a.Dp + d] = live ? -kls * t0 : 0.f;
        a.g_scale[(long)c * a.Dp + d] = live ? -kls * t1 * sigmoidf(raw + SMX_SOFTPLUS_INV_1) : 0.f;
      }
      if (d0 == 0 && lane == 0) {
        const float rsum = (sh[0][2][0] + sh[1][2][0]) + (sh[2][2][0] + sh[3][2][0]);
        // softmax(logits)_c * B - sum_b resp_bc
        float mx = -3.0e38f;
        for (int q = 0; q < a.C; ++q) mx = fmaxf(mx, a.logits[q]);
        float se = 0.f;
        for (int q = 0; q < a.C; ++q) se += fexp(a.logits[q] - mx);
        a.g_logits[c] = kls * ((float)a.B * fexp(a.logits[c] - mx) * frcp(se) - rsum);
      }
    }
    __syncthreads();
  }
}
// tied mixture parameters (scale.py:29-33): one location / one scale vector shared by every component = a [C][D] tensor whose rows
// are equal and all receive the SUM of the rows' gradients (in component order); fixed uniform weights = no logits gradient
__global__ __launch_bounds__(256) void scale_prior_tie_kernel(ScalePriorArgs a) {
  for (int d = threadIdx.x; d < a.Dp; d += 256) {
    if (a.tie_loc) {
      float t = 0.f;
      for (int c = 0; c < a.C; ++c) t += a.g_loc[(long)c * a.Dp + d];
      for (int c = 0; c < a.C; ++c) a.g_loc[(long)c * a.Dp + d] = t;
    }
    if (a.tie_scale) {
      float t = 0.f;
      for (int c = 0; c < a.C; ++c) t += a.g_scale[(long)c * a.Dp + d];
      for (int c = 0; c < a.C; ++c) a.g_scale[(long)c * a.Dp + d] = t;
    }
  }
  if (a.tie_mixtures && (int)threadIdx.x < a.C) a.g_logits[threadIdx.x] = 0.f;
}

int launch_scale_prior_bwd(hipStream_t st, const ScalePriorArgs& a) {
  if (a.tril) {
    if (a.D < 1 || a.D > 32 || a.tie_mixtures || a.tie_loc || a.tie_scale) { set_error("scale prior: full-covariance components take at most 32 latent dimensions and no tied parameters"); return SMX_ERR_INVALID; }
    const int n_grp = (a.B + SMX_TRILB_CELLS - 1) / SMX_TRILB_CELLS;
    if (!a.tril_part || (size_t)a.C * n_grp * a.D * (a.D + 2) > a.tril_part_floats) { set_error("scale prior: no scratch for the full-covariance gradients"); return SMX_ERR_INVALID; }
    hipLaunchKernelGGL(scale_prior_tril_bwd_kernel, dim3(a.C, n_grp), dim3(64 * SMX_TRILB_WAVES), (size_t)(a.D * (a.D + 1) + SMX_TRILB_WAVES * a.D * (a.D + 2)) * sizeof(float), st, a, a.tril_part);
    hipLaunchKernelGGL(scale_prior_tril_reduce_kernel, dim3(a.C), dim3(256), 0, st, a, a.tril_part, n_grp);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  hipLaunchKernelGGL(scale_prior_bwd_kernel, dim3(a.C), dim3(256), 0, st, a);
  if (a.tie_mixtures || a.tie_loc || a.tie_scale) hipLaunchKernelGGL(scale_prior_tie_kernel, dim3(1), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ---- scvi library latent (scvi.py:37-45, 88-106, 117) -------------------------
__global__ void lib_latent_fwd_kernel(LibLatentArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const long src = a.rows ? a.rows[b] : b;
  const float mu = a.latl[(long)b * a.ld], xs = a.latl[(long)b * a.ld + 1] + SMX_SOFTPLUS_INV_1, sig = softplusf(xs);
  float eps;
  if (a.inj_eps) eps = a.inj_eps[(long)b * a.inj_ld];
  else eps = normal4(philox_row(a.nk, (uint32_t)b, a.cell_base + (uint32_t)src, 0u)).x;
  const float mp = a.library[src * 2], vp = a.library[src * 2 + 1];
  const float sp = sqrtf(vp);
  a.l[b] = mu + sig * eps;
  a.sig[b] = sig;
  a.eps[b] = eps;
  a.kl[b] = lib_log_ratio(sp, sig, xs) + (sig * sig + (mu - mp) * (mu - mp)) / (2.f * vp) - 0.5f;
}
int launch_lib_latent_fwd(hipStream_t st, const LibLatentArgs& a) {
  hipLaunchKernelGGL(lib_latent_fwd_kernel, dim3((a.B + 255) / 256), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
__global__ void lib_latent_bwd_kernel(LibLatentArgs a) {
  const float kls = kl_scale_of(a.klw);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const long src = a.rows ? a.rows[b] : b;
  const float mu = a.latl[(long)b * a.ld], sraw = a.latl[(long)b * a.ld + 1];
  const float sig = a.sig[b], eps = a.eps[b];
  const float mp = a.library[src * 2], vp = a.library[src * 2 + 1];
  const float dl = a.dl[b];
  for (int j = 2; j < a.ld; ++j) a.dlatl[(long)b * a.ld + j] = 0.f;
  a.dlatl[(long)b * a.ld] = dl + kls * (mu - mp) / vp;
  a.dlatl[(long)b * a.ld + 1] = lib_dsraw(dl, eps, kls, sig, vp, sraw + SMX_SOFTPLUS_INV_1);
}
int launch_lib_latent_bwd(hipStream_t st, const LibLatentArgs& a) {
  hipLaunchKernelGGL(lib_latent_bwd_kernel, dim3((a.B + 255) / 256), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

}  // namespace smx
