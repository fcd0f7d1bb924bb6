// smx_bn.hip -- (split-K slab sum) -> BatchNorm -> ReLU -> Dropout and its backward (gfx950): the register-resident forms (with the
// latent head or the d lat product in front), two layers in one launch, the wide forms over column-major slabs, SyncBatchNorm.
// The backward launches carry the step's ELBO scalars and optimiser chunks as riders (smx_adam.h).
#include "smx_internal.h"
#include "smx_adam.h"
#include "smx_handoff.h"

namespace smx {

SMX_STAMP_TABLE

}
#include "smx_headdw.h"   // (behind the stamp table: the carried role's stamps go to this unit's)
namespace smx {

// ===========================================================================
// BatchNorm + ReLU + Dropout.  A workgroup owns BN_COLS columns and all rows:
// thread = (column c = tid % BN_COLS, row lane rl = tid / BN_COLS); rows are walked
// in chunks of BN_RL * BN_RPT with every slab load of a chunk in flight at once
// (the kernel is a latency chain, not a bandwidth problem).
// ===========================================================================
#ifndef SMX_BN_COLS
#define SMX_BN_COLS 8
#endif
constexpr int BN_COLS = SMX_BN_COLS;
constexpr int BN_RL = 64;
constexpr int BN_RPT_DEFAULT = 2;   // rows per thread; the register-resident kernels exist for 2, 4, 8, 16 (B <= 1024)
constexpr int BN_THREADS = BN_COLS * BN_RL;   // one wave per BN_COLS... waves = BN_THREADS / 64
constexpr int BN_WAVES = BN_THREADS / 64;

// column sum over the workgroup: lanes of a wave that share a column are 4 apart (xor 4..32),
// then the 4 waves meet in LDS; fixed order -> deterministic
__device__ inline float bn_col_reduce(float v, float* sh /*[BN_WAVES][BN_COLS]*/) {
  const int c = threadIdx.x % BN_COLS, w = threadIdx.x >> 6;
  static_assert(BN_COLS == 8, "bn_col_reduce: the lanes of a column are 8 apart");
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false));   // row_ror:8 = lane ^ 8 (were three ds_bpermute round trips)
  v = xor32_add(xor16_add(v));
  __syncthreads();
  if ((threadIdx.x & 63) < BN_COLS) sh[w * BN_COLS + c] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < BN_WAVES; q += 4)
    t += (sh[q * BN_COLS + c] + sh[(q + 1) * BN_COLS + c]) + (sh[(q + 2) * BN_COLS + c] + sh[(q + 3) * BN_COLS + c]);
  return t;
}

// sum of the split-K slabs for BN_RPT rows of one column, loads issued together.
// Up to SLAB_FLIGHT slabs' values of a thread (RPT rows each) are requested in ONE batch -- unconditional loads from a clamped slab index,
// left out at the add -- so that a column's sum costs one memory round trip, not one per batch of 8 plus one per remaining slab (the
// decoder's 12 slabs at BASELINE configs[1]: 5 dependent round trips, 4.6 of the launch's 9 us; tools/c2_stamps.sh).  The adds keep
// their order (slab 0, 1, ...): the same bits.
constexpr int SLAB_FLIGHT = 16;
template <int NR>
struct SlabBatch { float t[SLAB_FLIGHT][NR]; };
template <int NR>
__device__ inline void slab_issue(const float* base, int s0, int n_slabs, long slab_stride, int ld, int col, int r0, int rl, int B, SlabBatch<NR>& sb) {
#pragma unroll
  for (int q = 0; q < SLAB_FLIGHT; ++q) {
    const int s = min(s0 + q, n_slabs - 1);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int r = min(r0 + rl + BN_RL * i, B - 1);
      sb.t[q][i] = base[(long)s * slab_stride + (long)r * ld + col];
    }
  }
}
template <int NR>
__device__ inline void slab_accumulate(const SlabBatch<NR>& sb, int s0, int n_slabs, int r0, int rl, int B, float (&acc)[NR]) {
#pragma unroll
  for (int q = 0; q < SLAB_FLIGHT; ++q)
    if (s0 + q < n_slabs) {   // (block-uniform)
#pragma unroll
      for (int i = 0; i < NR; ++i) acc[i] += (r0 + rl + BN_RL * i < B) ? sb.t[q][i] : 0.f;
    }
}
template <int BN_RPT>
__device__ inline void slab_sum(const float* base, int n_slabs, long slab_stride, int ld, int col, int r0, int rl,
                                int B, float (&acc)[BN_RPT]) {
#pragma unroll
  for (int i = 0; i < BN_RPT; ++i) acc[i] = 0.f;
  if (BN_RPT <= 2) {   // (32 values in flight per lane)
    for (int s = 0; s < n_slabs; s += SLAB_FLIGHT) {
      SlabBatch<BN_RPT> sb;
      slab_issue<BN_RPT>(base, s, n_slabs, slab_stride, ld, col, r0, rl, B, sb);
      slab_accumulate<BN_RPT>(sb, s, n_slabs, r0, rl, B, acc);
    }
    return;
  }
  constexpr int SU = BN_RPT <= 4 ? 4 : 2;   // slabs per batch of loads: 16 values in flight per lane
  int s = 0;
  for (; s + SU <= n_slabs; s += SU) {
    float t[SU][BN_RPT];
#pragma unroll
    for (int q = 0; q < SU; ++q)
#pragma unroll
      for (int i = 0; i < BN_RPT; ++i) {
        const int r = r0 + rl + BN_RL * i;
        t[q][i] = r < B ? base[(long)(s + q) * slab_stride + (long)r * ld + col] : 0.f;
      }
#pragma unroll
    for (int q = 0; q < SU; ++q)
#pragma unroll
      for (int i = 0; i < BN_RPT; ++i) acc[i] += t[q][i];
  }
  for (; s < n_slabs; ++s)
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) {
      const int r = r0 + rl + BN_RL * i;
      if (r < B) acc[i] += base[(long)s * slab_stride + (long)r * ld + col];
    }
}

// extra workgroups of the BN launch: Philox multipliers / normals for later layers, 4 columns per thread
__device__ inline void noise_fill(const BnFwdArgs& a, int job_block) {
  const NoiseJob& j = a.jobs[job_block / SMX_NOISE_BLOCKS_PER_JOB];
  const int sub = job_block % SMX_NOISE_BLOCKS_PER_JOB;
  const int wq = (j.width + 3) >> 2;
  NoiseKey nk = a.nk;
  nk.stream = j.stream;
  const float scale = j.p > 0.f ? 1.f / (1.f - j.p) : 1.f;
  for (int idx = sub * BN_THREADS + threadIdx.x; idx < a.B * wq; idx += SMX_NOISE_BLOCKS_PER_JOB * BN_THREADS) {
    const int r = idx / wq, c0 = (idx % wq) * 4;
    const uint32_t cell = a.cell_base + (uint32_t)(a.rows ? a.rows[r] : r);
    const U4 w = philox_block(nk, cell, (uint32_t)(c0 >> 2));
    const float4 v = j.normal ? normal4(w) : dropout_mult4(w, j.p, scale);
    *reinterpret_cast<float4*>(j.dst + (long)r * j.ld + c0) = v;
  }
}

// RPT > 0: B <= BN_RL * RPT, every value of the column stays in registers (RPT rows per thread);
// RPT == 0: any B, the normalised values make a round trip through xhat
// the latent tile of the whole minibatch into LDS (row stride Dp + 4), one thread per 4 latent dims of a cell; the
// first workgroup also leaves z / sigma / eps / KL in memory for the backward pass (same arithmetic, same Philox
// blocks as latent_fwd_quad_kernel)
template <int MAXIT>
__device__ inline void latent_tile_to_lds(const LatentArgs& a, float* zs, bool store) {
  const int dq = a.Dp >> 2, ldz = a.Dp + 4;   // (rows 16-byte aligned: the dot products read the tile four k at a time)
  const int dsh = __builtin_ctz((unsigned)dq), dmask = dq - 1;   // dq is a power of two (bn_front_supported): shifts, not the ~35-instruction integer division per index
  const int total = a.B * dq;
  // every load of every iteration first (left as a loop the compiler waits for each iteration's loads in turn:
  // MAXIT serial round trips to data the previous launch has just written)
  float4 m4[MAXIT], s4[MAXIT], n4[MAXIT];
  uint32_t cell[MAXIT];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int total_r = (total + 63) & ~63;
  // Unconditional loads from a clamped index under block-uniform branches only: a lane-predicated load sits in a block of its own, and the
  // row id's `cell_base + rows[b]` inside such a block made the compiler wait for EVERY outstanding load of the iteration before the next
  // iteration's loads were issued -- two serial memory round trips ahead of the first dot product (tools/c2_stamps.sh).  The row id is only
  // read when the normals are drawn here (not when an earlier launch drew them: inj_eps).
  const bool need_cell = a.stochastic && !a.inj_eps;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    m4[it] = z4; s4[it] = z4; n4[it] = z4; cell[it] = 0;
    if (it * BN_THREADS >= total_r) continue;   // block-uniform
    const int idx = min((int)threadIdx.x + it * BN_THREADS, total - 1);
    const int b = idx >> dsh, d0 = (idx & dmask) * 4;
    m4[it] = *reinterpret_cast<const float4*>(a.lat + (long)b * a.ld + d0);
    if (a.stochastic) s4[it] = *reinterpret_cast<const float4*>(a.lat + (long)b * a.ld + a.Dp + d0);
    if (a.stochastic && a.inj_eps) n4[it] = *reinterpret_cast<const float4*>(a.inj_eps + (long)b * a.inj_ld + d0);
    cell[it] = (uint32_t)b;
    if (need_cell && a.rows) cell[it] = (uint32_t)a.rows[b];
  }
  SMX_STAMP(1, 7);   // the tile's loads issued
#ifdef SMX_STAMPS
  if (m4[0].x == 12345.678f && s4[0].x == 1.f) zs[0] = n4[0].x;   // (the first iteration's operands have arrived)
  SMX_STAMP(1, 8);
#endif
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int idx = threadIdx.x + it * BN_THREADS;
    if (it * BN_THREADS >= ((total + 63) & ~63)) break;   // block-uniform
    const int b = idx >> dsh, d0 = (idx & dmask) * 4;
    float kl = 0.f;
    if (idx < total) {
      float4 zq = z4, sq = make_float4(1.f, 1.f, 1.f, 1.f), eq = z4;
      const float4 mq = m4[it];
      if (a.stochastic) {
        float4 nq = n4[it];
        if (!a.inj_eps) nq = normal4(philox_row(a.nk, (uint32_t)b, a.cell_base + cell[it], (uint32_t)(d0 >> 2)));
        const float4 sr = s4[it];
        auto one = [&](int e, float mu, float s_raw, float nn, float& z, float& s, float& en) {
          if (d0 + e < a.D) {
            const float xs = s_raw + SMX_SOFTPLUS_INV_1;
            const float sg = latent_sigma(xs);
            s = sg; en = nn;
            z = mu + sg * nn;
            if (store) kl += 0.5f * (sg * sg + mu * mu - 1.f - 2.f * log_sigma_fast(xs, sg));   // (block-uniform: the KL term belongs to the workgroup that stores)
          }
        };
        one(0, mq.x, sr.x, nq.x, zq.x, sq.x, eq.x);
        one(1, mq.y, sr.y, nq.y, zq.y, sq.y, eq.y);
        one(2, mq.z, sr.z, nq.z, zq.z, sq.z, eq.z);
        one(3, mq.w, sr.w, nq.w, zq.w, sq.w, eq.w);
      } else {
        auto one = [&](int e, float mu, float& z) { if (d0 + e < a.D) z = a.relu ? fmaxf(mu, 0.f) : mu; };
        one(0, mq.x, zq.x); one(1, mq.y, zq.y); one(2, mq.z, zq.z); one(3, mq.w, zq.w);
      }
      *reinterpret_cast<float4*>(zs + b * ldz + d0) = zq;
      if (store) {
        const long o = (long)b * a.Dp + d0;
        *reinterpret_cast<float4*>(a.z + o) = zq;
        if (a.sig) {
          *reinterpret_cast<float4*>(a.sig + o) = sq;
          *reinterpret_cast<float4*>(a.eps + o) = eq;
        }
      }
    }
    if (store && a.kl && idx < ((total + 63) & ~63)) {   // the dq lanes of a cell are adjacent (dq a power of two <= 16)
      for (int off = 1; off < dq; off <<= 1) kl += __shfl_xor(kl, off, 64);
      if (idx < total && (idx & dmask) == 0) a.kl[b] = kl;
    }
  }
  SMX_STAMP(1, 9);   // sample + KL computed, LDS / global stores issued
}

template <int RPT, int FRONT, bool GEN_ACT = false>
__device__ inline void bn_act_fwd_body(const BnFwdArgs& a, const int bid) {
  constexpr bool SMALL = RPT > 0;
  constexpr int BN_RPT = SMALL ? RPT : BN_RPT_DEFAULT;
  extern __shared__ __attribute__((aligned(16))) float zs[];   // FRONT: [B][Dp + 4] | this workgroup's columns of W [8][Dp + 4]
  if (bid >= a.Hp / BN_COLS) {
    // FRONT = 1: ONE extra workgroup leaves z / sigma / eps / KL in memory for the backward pass and does nothing else -- as a duty of column
    // block 0 the stores and the KL arithmetic made that workgroup the launch's longest
    if constexpr (FRONT == 1) latent_tile_to_lds<BN_RPT * 2>(a.lat, zs, true);
    else noise_fill(a, bid - a.Hp / BN_COLS);
    return;
  }
  __shared__ float sh[BN_WAVES * BN_COLS];
  SMX_STAMP(FRONT ? 1 : 0, 0);   // entry
  if (FRONT) preload(a.lat.lat, a.lat.ld, a.lat.Dp, a.lat.D, a.lat.B, a.lat.stochastic, a.lat.inj_eps, a.lat.inj_ld, a.lat.rows, a.lat.z, a.lat.sig, a.lat.eps,
                     a.lat.kl, a.W, a.ldw, a.B, a.H, a.Hp, a.gamma, a.beta, a.inj_mask, a.inj_ld, a.batchnorm, a.training);
  else preload(a.pre, a.n_slabs, a.slab_stride, a.ld, a.B, a.H, a.Hp, a.gamma, a.beta, a.bias, a.inj_mask, a.inj_ld, a.xhat, a.out, a.batchnorm, a.training);
  const int c = threadIdx.x % BN_COLS, rl = threadIdx.x / BN_COLS;
  const int col = bid * BN_COLS + c;
  const bool live = col < a.H;  // padded columns produce zeros
  const float bias = (!a.batchnorm && a.bias && live) ? a.bias[col] : 0.f;
  const float gamma_pre = (a.batchnorm && live) ? a.gamma[col] : 0.f, beta_pre = (a.batchnorm && live) ? a.beta[col] : 0.f;   // (requested ahead of pass 1)
  // ... and the moving statistics the column's first thread updates at the end: read there, they were a memory round trip of their own between
  // the last reduction and the thread's exit -- the workgroup's life
  float mm_pre = 0.f, mv_pre = 0.f;
  if (a.batchnorm && a.training && a.update_moving && live && rl == 0) { mm_pre = a.moving_mean[col]; mv_pre = a.moving_var[col]; }
  constexpr int CH = BN_RL * BN_RPT;
  float vreg[BN_RPT];
  // FRONT = 1: input tile up to 64 wide; FRONT = 2: exactly 128 wide (hidden -> hidden layers of 128-unit networks: the
  // column of W costs 128 registers, fine at one workgroup per CU)
  constexpr int FK = FRONT == 2 ? 128 : 64;
  float wcol[FRONT == 1 ? 64 : 1];   // FRONT = 2 reads its column of W from LDS inside the dot products (128 registers spilled)
  const float* wcol_lds = nullptr;
  if (FRONT) {
    // this workgroup's [Dp][8] tile of W: one coalesced pass, left in LDS TRANSPOSED ([8 columns][Dp + 4]: a thread's column is a run of
    // 16-byte reads; as [Dp][8] it was Dp 4-byte reads, and the input tile's rows -- stride Dp + 1 -- one 4-byte read per multiply-add)
    const int lds_ld = a.lat.Dp + 4;
    float* ws = zs + a.B * lds_ld;
    float wl[FRONT == 2 ? 2 : 1];
#pragma unroll
    for (int u = 0; u < (FRONT == 2 ? 2 : 1); ++u) {
      const int t = (int)threadIdx.x + u * BN_THREADS;
      wl[u] = (t < a.lat.Dp * BN_COLS) ? a.W[(long)(t / BN_COLS) * a.ldw + bid * BN_COLS + (t % BN_COLS)] : 0.f;
    }
    if constexpr (FRONT == 2) {   // a plain input tile (hidden layers): every load first, then LDS
      constexpr int MAXIT = BN_RPT * 4;
      const int kq = a.lat.Dp >> 2, ldz = lds_ld, total = a.B * kq;
      const int ksh = __builtin_ctz((unsigned)kq), kmask = kq - 1;   // (Dp = 128)
      float4 t4[MAXIT];
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int idx = threadIdx.x + it * BN_THREADS;
        t4[it] = idx < total ? *reinterpret_cast<const float4*>(a.lat.lat + (long)(idx >> ksh) * a.lat.ld + (idx & kmask) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int idx = threadIdx.x + it * BN_THREADS;
        if (idx < total) {
          *reinterpret_cast<float4*>(zs + (idx >> ksh) * ldz + (idx & kmask) * 4) = t4[it];
        }
      }
    } else {
      latent_tile_to_lds<BN_RPT * 2>(a.lat, zs, false);   // B Dp / 4 quads over 512 threads: <= 2 RPT iterations (the extra workgroup stores)
    }
#pragma unroll
    for (int u = 0; u < (FRONT == 2 ? 2 : 1); ++u) {
      const int t = (int)threadIdx.x + u * BN_THREADS;
      if (t < a.lat.Dp * BN_COLS) ws[(t % BN_COLS) * lds_ld + t / BN_COLS] = wl[u];
    }
    __syncthreads();
    SMX_STAMP(1, 1);   // latent tile (sample + KL) and the W tile are in LDS
    if constexpr (FRONT == 1) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float4 w4 = (4 * v < a.lat.Dp) ? *reinterpret_cast<const float4*>(ws + c * lds_ld + 4 * v) : make_float4(0.f, 0.f, 0.f, 0.f);
        wcol[4 * v] = w4.x; wcol[4 * v + 1] = w4.y; wcol[4 * v + 2] = w4.z; wcol[4 * v + 3] = w4.w;
      }
    } else {
      wcol_lds = ws + c * lds_ld;
    }
    SMX_STAMP(1, 2);   // the thread's column of W in registers
  }

  // dropout multipliers drawn ahead by an earlier launch (or injected): loaded now, used after the reductions
  const bool drop = a.training && a.drop_p > 0.f;
  float mpre[BN_RPT];
  if (SMALL && drop && a.inj_mask) {
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) {
      const int r = rl + BN_RL * i;
      mpre[i] = r < a.B ? a.inj_mask[(long)r * a.inj_ld + col] : 0.f;
    }
  }
  // pass 1: slab sum (+ bias), column sum
  float s1 = 0.f;
  for (int r0 = 0; r0 < a.B; r0 += CH) {
    float acc[BN_RPT];
    if (FRONT) {
      const int ldz = a.lat.Dp + 4;
#pragma unroll
      for (int i = 0; i < BN_RPT; ++i) {
        const int r = min(r0 + rl + BN_RL * i, a.B - 1);
        const float4* z4 = reinterpret_cast<const float4*>(zs + r * ldz);
        float t = 0.f;
        if (FRONT == 2) {
#pragma unroll 4
          for (int v = 0; v < FK / 4; ++v) {
            const float4 z = z4[v], w = *reinterpret_cast<const float4*>(wcol_lds + 4 * v);
            t = fmaf(z.x, w.x, t); t = fmaf(z.y, w.y, t); t = fmaf(z.z, w.z, t); t = fmaf(z.w, w.w, t);
          }
        } else if (a.lat.Dp <= 32) {
#pragma unroll
          for (int v = 0; v < 8; ++v) {
            const float4 z = z4[v];
            t = fmaf(z.x, wcol[4 * v], t); t = fmaf(z.y, wcol[4 * v + 1], t); t = fmaf(z.z, wcol[4 * v + 2], t); t = fmaf(z.w, wcol[4 * v + 3], t);
          }
        } else {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const float4 z = z4[v];
            t = fmaf(z.x, wcol[4 * v], t); t = fmaf(z.y, wcol[4 * v + 1], t); t = fmaf(z.z, wcol[4 * v + 2], t); t = fmaf(z.w, wcol[4 * v + 3], t);
          }
        }
        acc[i] = t;
      }
    } else
    slab_sum(a.pre, a.n_slabs, a.slab_stride, a.ld, col, r0, rl, a.B, acc);
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) {
      const int r = r0 + rl + BN_RL * i;
      const float v = acc[i] + bias;
      if (SMALL) vreg[i] = v;
      if (r < a.B) {
        if (!SMALL) a.xhat[(long)r * a.Hp + col] = v;
        s1 += v;
      }
    }
  }
  float mean = 0.f, inv = 1.f, gamma = 1.f, beta = 0.f;
  SMX_STAMP(FRONT ? 1 : 0, 3);   // pass 1: slab sum / dot products
  if (a.batchnorm) {
    gamma = gamma_pre;
    beta = beta_pre;
    float var;
    if (a.training) {
      s1 = bn_col_reduce(s1, sh);
      SMX_STAMP(FRONT ? 1 : 0, 4);   // column sums
      mean = s1 / (float)a.B;
      float s2 = 0.f;
      if (SMALL) {
#pragma unroll
        for (int i = 0; i < BN_RPT; ++i)
          if (rl + BN_RL * i < a.B) { const float d = vreg[i] - mean; s2 = __builtin_fmaf(d, d, s2); }
      } else {
        for (int r = rl; r < a.B; r += BN_RL) {
          const float d = a.xhat[(long)r * a.Hp + col] - mean;
          s2 = __builtin_fmaf(d, d, s2);
        }
      }
      s2 = bn_col_reduce(s2, sh);
      SMX_STAMP(FRONT ? 1 : 0, 5);   // column variances
      var = s2 / (float)a.B;
      if (rl == 0) {
        if (a.batch_mean) { a.batch_mean[col] = mean; a.batch_var[col] = var; }
        if (a.update_moving && live) {
          // (two products and a sum each, NOT fused: the arithmetic of every build so far -- round 5's compiler paired the two updates
          // into packed multiplies and a packed add; spelled out since the library is built without that pairing, sisua_amd/build.py)
#pragma clang fp contract(off)
          a.moving_mean[col] = mm_pre * a.momentum + mean * (1.f - a.momentum);
          a.moving_var[col] = mv_pre * a.momentum + var * (1.f - a.momentum);
        }
      }
    } else {
      mean = live ? a.moving_mean[col] : 0.f;
      var = live ? a.moving_var[col] : 1.f;
    }
    inv = rsqrtf(var + a.eps);
    if (rl == 0 && a.inv_std) a.inv_std[col] = inv;
  }
  const float scale = drop ? 1.f / (1.f - a.drop_p) : 1.f;
  auto finish = [&](int r, float v, float mahead) {
#pragma clang fp contract(off)
    const long o = (long)r * a.Hp + col;
    float y = v;
    if (a.batchnorm) {
      v = (v - mean) * inv;
      y = __builtin_fmaf(gamma, v, beta);
    }
    if (a.batchnorm || SMALL) a.xhat[o] = v;
    float h;
    if constexpr (GEN_ACT) h = act_fwd(a.act, y);
    else {
      h = fmaxf(y, 0.f);
      if (a.leak != 0.f) h += a.leak * fminf(y, 0.f);
    }
    if (drop) {
      float mult;
      if (a.inj_mask) mult = SMALL ? mahead : a.inj_mask[(long)r * a.inj_ld + col];
      else {
        const uint32_t cell = a.cell_base + (uint32_t)(a.rows ? a.rows[r] : r);
        const U4 w = philox_row(a.nk, (uint32_t)r, cell, (uint32_t)(col >> 2));
        mult = dropout_mult1(w, col & 3, a.drop_p, scale);
      }
      h *= mult;
    }
    a.out[o] = live ? h : 0.f;
  };
  if (SMALL) {
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i)
      if (rl + BN_RL * i < a.B) finish(rl + BN_RL * i, vreg[i], mpre[i]);
  } else {
    for (int r = rl; r < a.B; r += BN_RL) finish(r, a.xhat[(long)r * a.Hp + col], 0.f);
  }
  SMX_STAMP(FRONT ? 1 : 0, 6);   // normalise, ReLU, dropout, stores issued
}

template <int RPT, int FRONT = 0>
__global__ __launch_bounds__(BN_THREADS) void bn_act_fwd_kernel(BnFwdArgs a) { bn_act_fwd_body<RPT, FRONT>(a, (int)blockIdx.x); }
// hidden layers whose activation is not ReLU (BnFwdArgs::act; smx_act.h): the plain forms only (no front)
template <int RPT>
__global__ __launch_bounds__(BN_THREADS) void bn_act_fwd_gen_kernel(BnFwdArgs a) { bn_act_fwd_body<RPT, 0, true>(a, (int)blockIdx.x); }
// two independent layers over the same minibatch in ONE launch (scvi: first layers of the encoder and of the library
// encoder): blocks [0, na) belong to a (its column blocks, then its noise jobs), the rest to b
template <int RPT>
__global__ __launch_bounds__(BN_THREADS) void bn_act_fwd_dual_kernel(BnFwdArgs a, BnFwdArgs b, int na) {
  if ((int)blockIdx.x < na) bn_act_fwd_body<RPT, 0>(a, (int)blockIdx.x);
  else bn_act_fwd_body<RPT, 0>(b, (int)blockIdx.x - na);
}


__global__ void bn_wide_fwd_kernel(BnFwdArgs a);   // (below: the forms that sum a wide panel's column-major slabs themselves)
__global__ void bn_wide_bwd_kernel(BnBwdArgs a);
__global__ void bn_wide_fwd_gen_kernel(BnFwdArgs a);
__global__ void bn_wide_bwd_gen_kernel(BnBwdArgs a);

bool bn_front_supported(int B, int Dp) {
  const int dq = Dp >> 2;
  return B > 0 && B <= BN_RL * 4 && Dp >= 4 && (Dp <= 64 || Dp == 128) && (Dp % 4) == 0 && (dq & (dq - 1)) == 0 && ((size_t)B * (Dp + 4) + (size_t)8 * (Dp + 4)) * sizeof(float) <= 96 * 1024;
}

int launch_bn_act_fwd(hipStream_t st, const BnFwdArgs& a_in) {
  BnFwdArgs a = a_in;
  const bool gen = a.act != SMX_ACT_RELU;   // (GEN_ACT forms: the plain and wide ones)
  if (gen && (a.act < SMX_ACT_RELU || a.act > SMX_ACT_SOFTPLUS || a.front)) { set_error("bn_act_fwd: activations other than ReLU take no front"); return SMX_ERR_INVALID; }
  if (a.front) {
    if (!bn_front_supported(a.B, a.lat.Dp) || a.n_jobs || !a.W || (a.lat.ld % 4) || (a.lat.inj_eps && (a.lat.inj_ld % 4)) ||
        (a.lat.Dp > 32 && a.lat.Dp != 64 && a.lat.Dp != 128)) {
      set_error("bn_act_fwd: latent front not applicable");
      return SMX_ERR_INVALID;
    }
    if (a.Hp % BN_COLS) { set_error("bn_act_fwd: bad shapes"); return SMX_ERR_INVALID; }
    const size_t lds = ((size_t)a.B * (a.lat.Dp + 4) + (size_t)BN_COLS * (a.lat.Dp + 4)) * sizeof(float);
    static const bool big_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&bn_act_fwd_kernel<4, 1>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
    if (lds > 64 * 1024 && !big_ok) { set_error("bn_act_fwd: cannot reserve the dynamic LDS of the latent front"); return SMX_ERR_HIP; }
    if (a.lat.Dp == 128) {   // (B <= 128 by the LDS bound of bn_front_supported)
      static const bool big2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bn_act_fwd_kernel<2, 2>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
      if (a.B > BN_RL * 2 || a.lat.stochastic || a.lat.relu || a.lat.z || (lds > 64 * 1024 && !big2)) {   // (plain input tiles only)
        set_error("bn_act_fwd: 128-wide front not applicable");
        return SMX_ERR_INVALID;
      }
      hipLaunchKernelGGL((bn_act_fwd_kernel<2, 2>), dim3(a.Hp / BN_COLS), dim3(BN_THREADS), lds, st, a);
    } else if (a.B <= BN_RL * 2) hipLaunchKernelGGL((bn_act_fwd_kernel<2, 1>), dim3(a.Hp / BN_COLS + (a.lat.z ? 1 : 0)), dim3(BN_THREADS), lds, st, a);
    else hipLaunchKernelGGL((bn_act_fwd_kernel<4, 1>), dim3(a.Hp / BN_COLS + (a.lat.z ? 1 : 0)), dim3(BN_THREADS), lds, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  if (a.Hp % BN_COLS || a.B <= 0) { set_error("bn_act_fwd: bad shapes"); return SMX_ERR_INVALID; }
  if (a.wide) {
    if (a.B > 128 || a.Hp > 128 || !a.pre || !a.xhat || a.slab_stride < (long)a.Hp * 128 || (a.slab_stride % 4)) { set_error("bn_act_fwd: wide slabs take at most 128 x 128"); return SMX_ERR_INVALID; }
    if (gen) hipLaunchKernelGGL(bn_wide_fwd_gen_kernel, dim3(a.Hp + a.n_jobs * SMX_NOISE_BLOCKS_PER_JOB), dim3(BN_THREADS), 0, st, a);
    else hipLaunchKernelGGL(bn_wide_fwd_kernel, dim3(a.Hp + a.n_jobs * SMX_NOISE_BLOCKS_PER_JOB), dim3(BN_THREADS), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  const int grid = a.Hp / BN_COLS + a.n_jobs * SMX_NOISE_BLOCKS_PER_JOB;
  if (gen) {
    if (a.B <= BN_RL * 2) hipLaunchKernelGGL(bn_act_fwd_gen_kernel<2>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    else if (a.B <= BN_RL * 4) hipLaunchKernelGGL(bn_act_fwd_gen_kernel<4>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    else if (a.B <= BN_RL * 8) hipLaunchKernelGGL(bn_act_fwd_gen_kernel<8>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    else if (a.B <= BN_RL * 16) hipLaunchKernelGGL(bn_act_fwd_gen_kernel<16>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    else hipLaunchKernelGGL(bn_act_fwd_gen_kernel<0>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  if (a.B <= BN_RL * 2) hipLaunchKernelGGL(bn_act_fwd_kernel<2>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  else if (a.B <= BN_RL * 4) hipLaunchKernelGGL(bn_act_fwd_kernel<4>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  else if (a.B <= BN_RL * 8) hipLaunchKernelGGL(bn_act_fwd_kernel<8>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  else if (a.B <= BN_RL * 16) hipLaunchKernelGGL(bn_act_fwd_kernel<16>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  else hipLaunchKernelGGL(bn_act_fwd_kernel<0>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// two layers over the same minibatch, one launch (no latent front, no SyncBatchNorm; register-resident forms only)
bool bn_dual_supported(int B) { return B > 0 && B <= BN_RL * 4; }
int launch_bn_act_fwd_dual(hipStream_t st, const BnFwdArgs& a, const BnFwdArgs& b) {
  if (a.front || b.front || b.n_jobs || a.B != b.B || !bn_dual_supported(a.B) || a.Hp % BN_COLS || b.Hp % BN_COLS || a.act != SMX_ACT_RELU ||
      b.act != SMX_ACT_RELU) {
    set_error("bn_act_fwd_dual: bad shapes (or an activation other than ReLU)");
    return SMX_ERR_INVALID;
  }
  const int na = a.Hp / BN_COLS + a.n_jobs * SMX_NOISE_BLOCKS_PER_JOB;
  const int grid = na + b.Hp / BN_COLS;
  if (a.B <= BN_RL * 2) hipLaunchKernelGGL(bn_act_fwd_dual_kernel<2>, dim3(grid), dim3(BN_THREADS), 0, st, a, b, na);
  else hipLaunchKernelGGL(bn_act_fwd_dual_kernel<4>, dim3(grid), dim3(BN_THREADS), 0, st, a, b, na);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ---- fold_dz: d lat [B][64 + 4] into `tile` (LDS), computed by the workgroup itself (BnBwdArgs::fold_dz) ------------------------------------
// 8 waves; wave w owns the cells 16 w .. 16 w + 15.  d z [128 x 32] = zD [128 x 128] zW^T as v_mfma_f32_16x16x32_bf16 on three-way split
// operands (six of the nine cross products: f32 accuracy, smx_device.h): A = the wave's rows of zD straight from global memory in the
// operand's layout (lane: row lane & 15, eight consecutive k from 8 (lane >> 4)), B = zW's bf16 x 3 image in LDS (split once per
// workgroup: 32 x 128 values over 512 threads).  The latent head's backward runs on the accumulators in place; its
// operand loads (mu, s_raw, sigma, eps) were requested at entry.  `wimg`: 3 x 32 rows of 136 bf16.
typedef float bnf_f32x4 __attribute__((ext_vector_type(4)));
__device__ inline bnf_f32x4 bnf_mfma16x3(const Split8& a, const Split8& b, bnf_f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t2, b.t0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t0, b.t2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t1, b.t1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t1, b.t0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t0, b.t1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t0, b.t0, acc, 0, 0, 0);
  return acc;
}
#define SMX_FOLD_WROW 136   /* bf16 per row of the W image: 128 + 8 (rows 272 bytes apart: 16-byte reads of 16 rows spread over the banks) */
#define SMX_FOLD_WIMG_BYTES (3 * 32 * SMX_FOLD_WROW * 2)
// SEAM (bn_bwd_seam_kernel): zD is written by other workgroups of THIS launch -- everything that does not read it first ((1), (2) and
// what the caller requested before), then the wait of smx_handoff.h, then (3) behind its acquire.  false: the wait gave up (nothing stored).
template <bool SEAM = false>
__device__ inline bool fold_dz_tile(const BnBwdArgs& a, const int bid, float* tile, const int ldd, unsigned char* wimg, const BwdSeamArgs* sm = nullptr, int* seam_ok = nullptr) {
  const EpiLatentBwd& e = a.zlb;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, kg = lane >> 4;
  // (1) what the latent backward reads at the accumulators' positions -- cell 16 w + 4 kg + r, latent dim 16 nb + li -- requested first (64-byte runs per
  // 16 lanes; the same unconditional loads from clamped rows as gemm_body's EPI = 2)
  float e_mu[2][4], e_sr[2][4], e_sg[2][4], e_ep[2][4];
  const float kls = kl_scale_of(e.klw);   // (the step's KL weight, requested with them)
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long b = min(16 * w + 4 * kg + r, a.B - 1);
      const int d = 16 * nb + li;
      e_mu[nb][r] = e.lat[b * e.ld + d];
      e_sr[nb][r] = e.lat[b * e.ld + e.Dp + d];
      e_sg[nb][r] = e.sig[b * e.Dp + d];
      e_ep[nb][r] = e.eps[b * e.Dp + d];
    }
  // (2) zW -> bf16 x 3 image: thread -> row d = tid >> 4, k = 8 (tid & 15) .. + 7
  {
    const int d = tid >> 4, k0 = (tid & 15) * 8;
    const float4 lo = *reinterpret_cast<const float4*>(a.zW + (long)d * a.zldw + k0), hi = *reinterpret_cast<const float4*>(a.zW + (long)d * a.zldw + k0 + 4);
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const Split8 sp = split3x8(x);
    smx_bf16x8* row = reinterpret_cast<smx_bf16x8*>(wimg + ((long)d * SMX_FOLD_WROW + k0) * 2);
    row[0] = sp.t0;
    row[(32 * SMX_FOLD_WROW * 2) / 16] = sp.t1;
    row[(2 * 32 * SMX_FOLD_WROW * 2) / 16] = sp.t2;
  }
  if constexpr (SEAM) {
    if (sm->preread) {   // (diagnostic: every line of zD into this CU's L1 ahead of the wait -- what a missing acquire would then read)
      for (int i = tid; i < a.B * 4; i += BN_THREADS) { const float t = a.zD[(long)(i >> 2) * a.zld + (i & 3) * 32]; asm volatile("" ::"v"(t)); }
    }
    if (!handoff_wait<true>(sm->seam, seam_ok)) return false;
  }
  // (3) the wave's rows of zD in the A operand's layout
  Split8 A[4];
  {
    const float* zr = a.zD + (long)min(16 * w + li, a.B - 1) * a.zld + 8 * kg;
    float4 v[8];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { v[2 * ks] = *reinterpret_cast<const float4*>(zr + 32 * ks); v[2 * ks + 1] = *reinterpret_cast<const float4*>(zr + 32 * ks + 4); }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float x[8] = {v[2 * ks].x, v[2 * ks].y, v[2 * ks].z, v[2 * ks].w, v[2 * ks + 1].x, v[2 * ks + 1].y, v[2 * ks + 1].z, v[2 * ks + 1].w};
      A[ks] = split3x8(x);
    }
  }
  __syncthreads();
  // (4) d z: two 16 x 16 tiles per wave (latent dims 0-15, 16-31), K = 128 in four steps
  bnf_f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const smx_bf16x8* row = reinterpret_cast<const smx_bf16x8*>(wimg + ((long)(16 * nb + li) * SMX_FOLD_WROW + 32 * ks + 8 * kg) * 2);
      Split8 Bq;
      Bq.t0 = row[0]; Bq.t1 = row[(32 * SMX_FOLD_WROW * 2) / 16]; Bq.t2 = row[(2 * 32 * SMX_FOLD_WROW * 2) / 16];
      acc[nb] = bnf_mfma16x3(A[ks], Bq, acc[nb]);
    }
  // (5) the latent head's backward on the accumulators where they are (gemm_body's EPI = 2, the plain stochastic form): d mu | d s_raw into the tile
  // (rows of 16 w .. 16 w + 15: this wave's own) and, from workgroup 0, once to memory for the weight-gradient launch
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = 16 * w + 4 * kg + r, d = 16 * nb + li;
      const bool live = d < e.D;
      const float dz = acc[nb][r];
      const float o0 = live ? dz + kls * e_mu[nb][r] : 0.f;
      // (FLOOR, DESIGN.md 4t: below raw = -87.9 sigmoidf is 0 and this is -0 where the value is -kls; sigma >= 2^-126 from the forward keeps it from NaN)
      const float o1 = live ? (dz * e_ep[nb][r] + kls * (e_sg[nb][r] - frcp(e_sg[nb][r]))) * sigmoidf(e_sr[nb][r] + SMX_SOFTPLUS_INV_1) : 0.f;
      if (b < a.B) {
        tile[b * ldd + d] = o0;
        tile[b * ldd + e.Dp + d] = o1;
        if (bid == 0) { e.dlat[(long)b * e.ld + d] = o0; e.dlat[(long)b * e.ld + e.Dp + d] = o1; }
      }
    }
  return true;
}

// GEN_ACT forms: the multiplier the forward applied to element (r, col) -- from the same source, bit for bit (BnBwdArgs::act)
__device__ inline float bn_keep(const BnBwdArgs& a, int r, int col) {
  if (!(a.drop_p > 0.f)) return a.drop_scale;
  if (a.inj_mask) return a.inj_mask[(long)r * a.inj_ld + col];
  const uint32_t cell = a.cell_base + (uint32_t)(a.rows ? a.rows[r] : r);
  return dropout_mult1(philox_row(a.nk, (uint32_t)r, cell, (uint32_t)(col >> 2)), col & 3, a.drop_p, a.drop_scale);
}
// ... and d out -> d y of that element: xv is the layer's xhat (y itself without BatchNorm)
__device__ inline float bn_gen_dy(const BnBwdArgs& a, int r, int col, float dout, float xv, float gamma, float beta) {
  const float y = a.batchnorm ? __builtin_fmaf(gamma, xv, beta) : xv;   // (the forward's y, bit for bit)
  return dout * bn_keep(a, r, col) * act_grad(a.act, act_fwd(a.act, y));
}

template <int RPT, int FRONT, bool GEN_ACT = false, bool SEAM = false>
__device__ inline void bn_act_bwd_body(const BnBwdArgs& a, const int bid, const BwdSeamArgs* sm = nullptr) {
  constexpr bool SMALL = RPT > 0;
  constexpr int BN_RPT = SMALL ? RPT : BN_RPT_DEFAULT;
  static_assert(!SEAM || (FRONT == 1 && !GEN_ACT), "the seam form is the fold_dz front's");
  extern __shared__ __attribute__((aligned(16))) float ds[];   // FRONT: d lat tile [B][fK + 4] | this workgroup's rows of W [8][fK + 4]
  if constexpr (!SEAM) {   // (bn_bwd_seam_kernel deals its riders itself)
    const int nb = a.Hp / BN_COLS, extra = bid - nb;
    if (extra >= 0) {
      const int e = extra - (a.with_metrics ? 1 : 0);
      if (e >= 0 && e < a.adam_count) { adam_chunk_body<BN_THREADS>(a.adam, a.adam_first + e); return; }   // optimiser chunks of the heads: every thread of the workgroup
      if (threadIdx.x >= 256) return;                   // the other riders are 256-thread bodies
      if (e < 0) metrics_body(a.metrics);                                                 // ELBO scalars
      else {                                                                              // or only their gradient norms
        const int i = e - a.adam_count;
        if (i < a.sqr_count) sq_reduce_body(a.adam.sq_slots + a.sqr_first[i], a.sqr_n[i], a.sq_total + a.sqr_dst[i]);
        else step_close_body<false>(a.adam);                                              // the LAST rider (a.close) closes the step
      }
      return;
    }
  }
  __shared__ float sh[BN_WAVES * BN_COLS];
  SMX_STAMP(FRONT ? 3 : 2, 0);   // entry
  if (FRONT) preload(a.fD, a.fld, a.fW, a.fldw, a.fK, a.diag, a.out, a.xhat, a.inv_std, a.gamma, a.B, a.H, a.Hp, a.batchnorm, a.training, a.drop_scale);
  else preload(a.dout, a.n_slabs, a.slab_stride, a.ld, a.out, a.xhat, a.inv_std, a.gamma, a.B, a.H, a.Hp, a.batchnorm, a.training, a.drop_scale, a.dpre, a.leak);
  const int c = threadIdx.x % BN_COLS, rl = threadIdx.x / BN_COLS;
  const int col = bid * BN_COLS + c;
  const bool live = col < a.H;
  constexpr int CH = BN_RL * BN_RPT;
  float dyreg[BN_RPT], xhreg[BN_RPT];
  float s1 = 0.f, s2 = 0.f;
  // (register-resident forms) what the activation mask and the BatchNorm formula need of the forward pass, requested FIRST: these loads
  // used to follow the dot products / slab sums -- a memory round trip of their own behind them (tools/c2_stamps.sh)
  float outpre[BN_RPT], xhpre[BN_RPT];
  float gamma_pre = 0.f, inv_pre = 0.f;
  if (SMALL) {
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) {
      const long o = (long)min(rl + BN_RL * i, a.B - 1) * a.Hp + col;
      if constexpr (!GEN_ACT) outpre[i] = a.out[o];
      xhpre[i] = (GEN_ACT || a.batchnorm) ? a.xhat[o] : 0.f;
    }
    if (a.batchnorm) { gamma_pre = live ? a.gamma[col] : 0.f; inv_pre = a.inv_std[col]; }
  }
  float gamma_g = 0.f, beta_g = 0.f;   // (GEN_ACT: y = gamma xhat + beta inside the row loop)
  if constexpr (GEN_ACT) {
    if (a.batchnorm && live) { gamma_g = a.gamma[col]; beta_g = a.beta[col]; }
  }
  constexpr int FK = FRONT == 2 ? 128 : 64;   // FRONT = 2: K = 128 exactly (see bn_act_fwd_body)
  float wrow[FRONT ? FK : 1];
  if (FRONT) {
    const int ldd = a.fK + 4, kq = a.fK >> 2;   // (rows 16-byte aligned: the dot products read the tile four k at a time)
    const int ksh = __builtin_ctz((unsigned)kq), kmask = kq - 1;   // fK is 32, 64 or 128 (bn_bwd_front_supported)
    // this workgroup's 8 rows of W_lat: ONE coalesced pass into LDS (every thread loading its own row from global
    // memory is 8 different cache lines per quarter-wave: 5 us), then each thread copies its row to registers
    float* ws = ds + a.B * ldd;                  // [BN_COLS][fK + 4]
    const int ldw_s = a.fK + 4;
    float4 wl = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool wl_on = (int)threadIdx.x < BN_COLS * kq && !(a.diag & 64);   // (8 rows x fK / 4 <= 256 float4: one per thread)
    if (wl_on) wl = *reinterpret_cast<const float4*>(a.fW + (long)(bid * BN_COLS + ((int)threadIdx.x >> ksh)) * a.fldw + ((int)threadIdx.x & kmask) * 4);
    if (FRONT == 1 && a.fold_dz) {   // (block-uniform) the tile is computed here: d z product + latent backward (fold_dz_tile)
      if constexpr (SEAM) {
        __shared__ int seam_ok;
        if (!fold_dz_tile<true>(a, bid, ds, ldd, reinterpret_cast<unsigned char*>(ws + BN_COLS * ldw_s), sm, &seam_ok)) return;
      } else
      fold_dz_tile(a, bid, ds, ldd, reinterpret_cast<unsigned char*>(ws + BN_COLS * ldw_s));
      if ((int)threadIdx.x < BN_COLS * kq) *reinterpret_cast<float4*>(&ws[((int)threadIdx.x >> ksh) * ldw_s + ((int)threadIdx.x & kmask) * 4]) = wl;
    } else
    {   // all loads of the tile in flight at once (B fK / 4 float4 over 512 threads), then LDS
      constexpr int MAXIT = BN_RPT * (FK / 32);
      float4 tl[MAXIT];
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int idx = threadIdx.x + it * BN_THREADS;
        tl[it] = (idx < a.B * kq && !(a.diag & 32)) ? *reinterpret_cast<const float4*>(a.fD + (long)(idx >> ksh) * a.fld + (idx & kmask) * 4)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int idx = threadIdx.x + it * BN_THREADS;
        if (idx < a.B * kq) {
          *reinterpret_cast<float4*>(ds + (idx >> ksh) * ldd + (idx & kmask) * 4) = tl[it];
        }
      }
      if ((int)threadIdx.x < BN_COLS * kq) *reinterpret_cast<float4*>(&ws[((int)threadIdx.x >> ksh) * ldw_s + ((int)threadIdx.x & kmask) * 4]) = wl;
    }
    __syncthreads();
    SMX_STAMP(3, 1);   // the gradient tile and the rows of W are in LDS
#pragma unroll
    for (int v = 0; v < FK / 4; ++v) {
      const float4 t = (4 * v < a.fK) ? *reinterpret_cast<const float4*>(&ws[c * ldw_s + 4 * v]) : make_float4(0.f, 0.f, 0.f, 0.f);
      wrow[4 * v] = t.x; wrow[4 * v + 1] = t.y; wrow[4 * v + 2] = t.z; wrow[4 * v + 3] = t.w;
    }
    SMX_STAMP(3, 2);   // the thread's row of W in registers
  }
  for (int r0 = 0; r0 < a.B; r0 += CH) {
    float acc[BN_RPT];
    if (FRONT) {
      const int ldd = a.fK + 4;
#pragma unroll
      for (int i = 0; i < BN_RPT; ++i) {
        const int r = min(r0 + rl + BN_RL * i, a.B - 1);
        const float4* d4 = reinterpret_cast<const float4*>(ds + r * ldd);
        float t = 0.f;
        auto dots = [&](auto nv) {
#pragma unroll
          for (int v = 0; v < decltype(nv)::value; ++v) {
            const float4 d = d4[v];
            t = fmaf(d.x, wrow[4 * v], t); t = fmaf(d.y, wrow[4 * v + 1], t); t = fmaf(d.z, wrow[4 * v + 2], t); t = fmaf(d.w, wrow[4 * v + 3], t);
          }
        };
        if (a.diag & 16) t = ds[r * ldd] + wrow[0] + wrow[63];
        else if (FRONT == 2) dots(std::integral_constant<int, FK / 4>());
        else if (a.fK <= 32) dots(std::integral_constant<int, 8>());
        else dots(std::integral_constant<int, 16>());
        acc[i] = t;
      }
    } else
    slab_sum(a.dout, a.n_slabs, a.slab_stride, a.ld, col, r0, rl, a.B, acc);
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i) {
      const int r = r0 + rl + BN_RL * i;
      float dy = 0.f, xh = 0.f;
      if (r < a.B) {
        const long o = (long)r * a.Hp + col;
        if constexpr (GEN_ACT) {
          const float xv = SMALL ? xhpre[i] : a.xhat[o];
          dy = live ? bn_gen_dy(a, r, col, acc[i], xv, gamma_g, beta_g) : 0.f;
          if (a.batchnorm) xh = xv;
        } else {
        const float ov = SMALL ? outpre[i] : a.out[o];
        dy = (live && ov > 0.f) ? acc[i] * a.drop_scale : 0.f;
        if (a.leak != 0.f && live && !(ov > 0.f)) dy = acc[i] * a.leak;
        if (a.batchnorm) xh = SMALL ? xhpre[i] : a.xhat[o];
        }
        if (!SMALL) a.dpre[o] = dy;
        s1 += dy;
        { // (product, then sum: not fused -- see the moving statistics of bn_act_fwd_body)
#pragma clang fp contract(off)
          s2 += dy * xh;
        }
      }
      if (SMALL) { dyreg[i] = dy; xhreg[i] = xh; }
    }
  }
  SMX_STAMP(FRONT ? 3 : 2, 3);   // slab sum / dot products, activation mask, the loads of out and xhat
  s1 = bn_col_reduce(s1, sh);
  SMX_STAMP(FRONT ? 3 : 2, 4);
  if (!a.batchnorm) {
    if (rl == 0 && a.dbias && live) a.dbias[col] = s1;
    if (SMALL) {
#pragma unroll
      for (int i = 0; i < BN_RPT; ++i)
        if (rl + BN_RL * i < a.B) a.dpre[(long)(rl + BN_RL * i) * a.Hp + col] = dyreg[i];
    }
    return;
  }
  s2 = bn_col_reduce(s2, sh);
  SMX_STAMP(FRONT ? 3 : 2, 5);
  const float gamma = SMALL ? gamma_pre : (live ? a.gamma[col] : 0.f);
  const float inv = SMALL ? inv_pre : a.inv_std[col];
  if (rl == 0) { a.dgamma[col] = live ? s2 : 0.f; a.dbeta[col] = live ? s1 : 0.f; }
  const float invB = 1.f / (float)a.B;
  auto finish = [&](int r, float dy, float xh) {
    float d;
    if (a.training) d = (gamma * inv) * __builtin_fmaf(-__builtin_fmaf(xh, s2, s1), invB, dy);
    else d = dy * gamma * inv;
    a.dpre[(long)r * a.Hp + col] = d;
  };
  if (SMALL) {
#pragma unroll
    for (int i = 0; i < BN_RPT; ++i)
      if (rl + BN_RL * i < a.B) finish(rl + BN_RL * i, dyreg[i], xhreg[i]);
  } else {
    for (int r = rl; r < a.B; r += BN_RL) finish(r, a.dpre[(long)r * a.Hp + col], a.xhat[(long)r * a.Hp + col]);
  }
  SMX_STAMP(FRONT ? 3 : 2, 6);   // stores issued
}

template <int RPT, int FRONT = 0>
__global__ __launch_bounds__(BN_THREADS) void bn_act_bwd_kernel(BnBwdArgs a) { bn_act_bwd_body<RPT, FRONT>(a, (int)blockIdx.x); }
template <int RPT>
__global__ __launch_bounds__(BN_THREADS) void bn_act_bwd_gen_kernel(BnBwdArgs a) { bn_act_bwd_body<RPT, 0, true>(a, (int)blockIdx.x); }
// two independent layers in ONE launch, both with the gradient front (scvi: last layers of the encoder and of the
// library encoder): blocks [0, na) belong to a (column blocks, then its riders), the rest to b (no riders)
template <int RPT>
__global__ __launch_bounds__(BN_THREADS) void bn_act_bwd_dual_kernel(BnBwdArgs a, BnBwdArgs b, int na) {
  if ((int)blockIdx.x < na) bn_act_bwd_body<RPT, 1>(a, (int)blockIdx.x);
  else bn_act_bwd_body<RPT, 1>(b, (int)blockIdx.x - na);
}

// fold_dz: the latent tile is [B][64] = mu | s_raw halves of 32; the d z tile [B][36] and the rows it overwrites live in the tile's own space
bool bn_bwd_fold_supported(int B, int fK, int Dp) { return B > 0 && B <= 128 && fK == 64 && Dp == 32 && !tuning_on("no_fold_dz"); }
bool bn_bwd_front_supported(int B, int K) {
  return B > 0 && B <= BN_RL * 4 && (K == 32 || K == 64 || (K == 128 && B <= BN_RL * 2)) && ((size_t)B * (K + 4) + 8 * (K + 4)) * sizeof(float) <= 96 * 1024;
}

int launch_bn_act_bwd(hipStream_t st, const BnBwdArgs& a_in) {
  BnBwdArgs a = a_in;
  const bool gen = a.act != SMX_ACT_RELU;
  if (gen && (a.act < SMX_ACT_RELU || a.act > SMX_ACT_SOFTPLUS || a.front || !a.xhat || (a.batchnorm && !a.beta))) {
    set_error("bn_act_bwd: activations other than ReLU take no gradient front and need xhat (and beta)");
    return SMX_ERR_INVALID;
  }
  if (a.front) {
    if (!bn_bwd_front_supported(a.B, a.fK) || !a.fD || !a.fW || (a.fld % 4) || (a.fldw % 4) || a.Hp % BN_COLS) {
      set_error("bn_act_bwd: gradient front not applicable");
      return SMX_ERR_INVALID;
    }
    const int grid = a.Hp / BN_COLS + (a.with_metrics ? 1 : 0) + a.adam_count + a.sqr_count + (a.close ? 1 : 0);
    size_t lds = ((size_t)a.B * (a.fK + 4) + (size_t)BN_COLS * (a.fK + 4)) * sizeof(float);
    if (a.fold_dz) {
      const EpiLatentBwd& e = a.zlb;
      if (!bn_bwd_fold_supported(a.B, a.fK, e.Dp) || !a.zD || !a.zW || (a.zld % 4) || (a.zldw % 4) || a.zldw < 128 || a.zld < 128 || !e.lat || !e.sig || !e.eps || !e.dlat ||
          !e.stochastic || e.dklz || e.dz_add || (e.ld % 4) || e.ld < 2 * e.Dp || a.B > BN_RL * 2) {
        set_error("bn_act_bwd: fold_dz not applicable");
        return SMX_ERR_INVALID;
      }
      lds += SMX_FOLD_WIMG_BYTES;
      static const bool fold_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&bn_act_bwd_kernel<2, 1>),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
      if (lds > 64 * 1024 && !fold_ok) { set_error("bn_act_bwd: cannot reserve the dynamic LDS of fold_dz"); return SMX_ERR_HIP; }
    }
    static const bool big_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&bn_act_bwd_kernel<4, 1>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
    if (lds > 64 * 1024 && !big_ok) { set_error("bn_act_bwd: cannot reserve the dynamic LDS of the gradient front"); return SMX_ERR_HIP; }
    if (a.fK == 128) {
      static const bool big2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bn_act_bwd_kernel<2, 2>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
      if (lds > 64 * 1024 && !big2) { set_error("bn_act_bwd: cannot reserve the dynamic LDS of the gradient front"); return SMX_ERR_HIP; }
      hipLaunchKernelGGL((bn_act_bwd_kernel<2, 2>), dim3(grid), dim3(BN_THREADS), lds, st, a);
    } else if (a.B <= BN_RL * 2) hipLaunchKernelGGL((bn_act_bwd_kernel<2, 1>), dim3(grid), dim3(BN_THREADS), lds, st, a);
    else hipLaunchKernelGGL((bn_act_bwd_kernel<4, 1>), dim3(grid), dim3(BN_THREADS), lds, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  if (a.Hp % BN_COLS || a.B <= 0) { set_error("bn_act_bwd: bad shapes"); return SMX_ERR_INVALID; }
  if (a.wide) {
    if (a.B > 128 || a.Hp > 128 || !a.dout || a.slab_stride < (long)a.Hp * 128 || (a.slab_stride % 4)) { set_error("bn_act_bwd: wide slabs take at most 128 x 128"); return SMX_ERR_INVALID; }
    if (gen) hipLaunchKernelGGL(bn_wide_bwd_gen_kernel, dim3(a.Hp + (a.with_metrics ? 1 : 0) + a.adam_count + a.sqr_count + (a.close ? 1 : 0)), dim3(BN_THREADS), 0, st, a);
    else hipLaunchKernelGGL(bn_wide_bwd_kernel, dim3(a.Hp + (a.with_metrics ? 1 : 0) + a.adam_count + a.sqr_count + (a.close ? 1 : 0)), dim3(BN_THREADS), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  const int grid = a.Hp / BN_COLS + (a.with_metrics ? 1 : 0) + a.adam_count + a.sqr_count + (a.close ? 1 : 0);
  if (gen) {
    if (a.B <= BN_RL * 2) hipLaunchKernelGGL(bn_act_bwd_gen_kernel<2>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    else if (a.B <= BN_RL * 4) hipLaunchKernelGGL(bn_act_bwd_gen_kernel<4>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    else if (a.B <= BN_RL * 8) hipLaunchKernelGGL(bn_act_bwd_gen_kernel<8>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    else if (a.B <= BN_RL * 16) hipLaunchKernelGGL(bn_act_bwd_gen_kernel<16>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    else hipLaunchKernelGGL(bn_act_bwd_gen_kernel<0>, dim3(grid), dim3(BN_THREADS), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
  if (a.B <= BN_RL * 2) hipLaunchKernelGGL(bn_act_bwd_kernel<2>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  else if (a.B <= BN_RL * 4) hipLaunchKernelGGL(bn_act_bwd_kernel<4>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  else if (a.B <= BN_RL * 8) hipLaunchKernelGGL(bn_act_bwd_kernel<8>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  else if (a.B <= BN_RL * 16) hipLaunchKernelGGL(bn_act_bwd_kernel<16>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  else hipLaunchKernelGGL(bn_act_bwd_kernel<0>, dim3(grid), dim3(BN_THREADS), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// both layers with the gradient front (their incoming gradients as dot products of an LDS tile)
int launch_bn_act_bwd_dual(hipStream_t st, const BnBwdArgs& a_in, const BnBwdArgs& b_in) {
  BnBwdArgs a = a_in, b = b_in;
  a.diag = b.diag = 0;
  auto ok = [](const BnBwdArgs& x) {
    return x.front && x.fK <= 64 && bn_bwd_front_supported(x.B, x.fK) && x.fD && x.fW && !(x.fld % 4) && !(x.fldw % 4) && !(x.Hp % BN_COLS);
  };
  if (!ok(a) || !ok(b) || a.B != b.B || !bn_dual_supported(a.B) || b.with_metrics || b.adam_count || b.sqr_count || a.act != SMX_ACT_RELU || b.act != SMX_ACT_RELU) {
    set_error("bn_act_bwd_dual: gradient fronts not applicable");
    return SMX_ERR_INVALID;
  }
  const int na = a.Hp / BN_COLS + (a.with_metrics ? 1 : 0) + a.adam_count + a.sqr_count + (a.close ? 1 : 0);
  const int grid = na + b.Hp / BN_COLS;
  auto need = [](const BnBwdArgs& x) { return ((size_t)x.B * (x.fK + 4) + (size_t)BN_COLS * (x.fK + 4)) * sizeof(float); };
  const size_t lds = need(a) > need(b) ? need(a) : need(b);
  static const bool big_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&bn_act_bwd_dual_kernel<4>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
  if (lds > 64 * 1024 && !big_ok) { set_error("bn_act_bwd_dual: cannot reserve the dynamic LDS of the gradient fronts"); return SMX_ERR_HIP; }
  if (a.B <= BN_RL * 2) hipLaunchKernelGGL(bn_act_bwd_dual_kernel<2>, dim3(grid), dim3(BN_THREADS), lds, st, a, b, na);
  else hipLaunchKernelGGL(bn_act_bwd_dual_kernel<4>, dim3(grid), dim3(BN_THREADS), lds, st, a, b, na);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ===========================================================================
// BatchNorm launches that sum the HUNDREDS of slabs of a wide-panel product themselves (BASELINE.json configs[4]: the encoder front's
// 209 K slices, the fused output head's 250 workgroups, each with a [128][128] partial sum).  Until round 5 a reduce launch
// (bigk_reduce_kernel) stood between the product and the 16-workgroup BatchNorm launch: two latency-bound launches (5-6 us + 6-7 us) for
// 14-16 MB of slabs and 64 KB of result.  Here the producers leave their slabs COLUMN-major ([slab][column][128 rows]: a column of a slab
// is 512 contiguous bytes) and ONE workgroup per column sums its column over the slabs -- 16-byte loads, every slab of a thread in flight
// at once -- and finishes the BatchNorm pass on the 128 sums.  The additions keep the order of the launches they replace (thread sg of 16
// sums the slabs sg, sg + 16, ...; the 16 partial sums in sg order; the column statistics as the balanced tree over rows (r, r + 64) of
// bn_col_reduce): bit for bit the same results (tests/test_gpu_configs.py).  Minibatches of at most 128 cells.
// ===========================================================================
__device__ inline void wide_slab_column(const float* part, long slab_stride, int n_slabs, int col, float* sh /*[16][128]*/) {
  const int rq = threadIdx.x & 31, sg = threadIdx.x >> 5;   // rows 4 rq .. + 3; slabs sg, sg + 16, ...
  const float4* p = reinterpret_cast<const float4*>(part) + (long)col * 32 + rq;
  const long s4 = slab_stride >> 2;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int z0 = sg; z0 < n_slabs; z0 += 256) {
    float4 v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[(long)min(z0 + 16 * u, n_slabs - 1) * s4];
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (z0 + 16 * u < n_slabs) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
  }
  *reinterpret_cast<float4*>(sh + sg * 128 + 4 * rq) = acc;
}
// the column's value of row r (threads 0 .. 127 after the barrier)
__device__ inline float wide_row_value(const float* sh, int r) {
  float v = sh[r];
#pragma unroll
  for (int u = 1; u < 16; ++u) v += sh[u * 128 + r];
  return v;
}
// sum over the 64 pairs (r, r + 64) held by the lanes of wave 0: the balanced tree of bn_col_reduce
__device__ inline float wide_tree64(float p) { return wave_sum(p); }   // (lane ^ 1, 2, 4, 8 by DPP, 16 and 32 by row / half exchanges: that tree)

// (Which multiply-adds the compiler fuses in bn_act_fwd_body / bn_act_bwd_body<2, 0> was read off their ISA; the kernels below spell the
// same operations out with contraction switched off, so that the two forms stay equal bit for bit.)
template <bool GEN_ACT>
__device__ inline void bn_wide_fwd_body(const BnFwdArgs& a) {
#pragma clang fp contract(off)
  const int bid = (int)blockIdx.x;
  if (bid >= a.Hp) { noise_fill(a, bid - a.Hp); return; }
  __shared__ __attribute__((aligned(16))) float sh[16 * 128];
  __shared__ float vs[128], st[2];
  preload(a.pre, a.n_slabs, a.slab_stride, a.B, a.H, a.Hp, a.gamma, a.beta, a.bias, a.inj_mask, a.inj_ld, a.xhat, a.out, a.batchnorm, a.training, a.drop_p,
          a.batch_mean, a.batch_var, a.moving_mean, a.moving_var, a.inv_std, a.update_moving, a.rows, a.leak);   // (one batch: smx_device.h)
  const int col = bid, r = (int)threadIdx.x;
  const bool live = col < a.H, rowt = r < 128, on = rowt && r < a.B;
  const float bias = (!a.batchnorm && a.bias && live) ? a.bias[col] : 0.f;
  const float gamma = (a.batchnorm && live) ? a.gamma[col] : 0.f, beta = (a.batchnorm && live) ? a.beta[col] : 0.f;
  const bool drop = a.training && a.drop_p > 0.f;
  float mpre = 0.f;
  if (drop && a.inj_mask && on) mpre = a.inj_mask[(long)r * a.inj_ld + col];
  float mm_pre = 0.f, mv_pre = 0.f;   // (the moving statistics thread 0 updates at the end, requested now)
  if (a.batchnorm && a.training && a.update_moving && live && r == 0) { mm_pre = a.moving_mean[col]; mv_pre = a.moving_var[col]; }
  SMX_STAMP(0, 0);
  wide_slab_column(a.pre, a.slab_stride, a.n_slabs, col, sh);
  SMX_STAMP(0, 3);   // the thread's slabs summed, partial sums in LDS
  __syncthreads();
  float v = 0.f;
  if (rowt) { v = wide_row_value(sh, r) + bias; vs[r] = v; }
  float mean = 0.f, inv = 1.f;
  if (a.batchnorm) {
    float var;
    if (a.training) {
      __syncthreads();
      if (r < 64) {   // wave 0: rows r and r + 64, summed and squared in the form of bn_act_fwd_body (the same contractions: the same bits)
        const float v0 = vs[r], v1 = vs[r + 64];
        float s1 = 0.f;
        if (r < a.B) s1 += v0;
        if (r + 64 < a.B) s1 += v1;
        s1 = wide_tree64(s1);
        const float mu = s1 / (float)a.B;
        float s2 = 0.f;
        if (r < a.B) { const float d = v0 - mu; s2 = d * d; }
        if (r + 64 < a.B) { const float d = v1 - mu; s2 = __builtin_fmaf(d, d, s2); }
        s2 = wide_tree64(s2);
        if (r == 0) { st[0] = mu; st[1] = s2 / (float)a.B; }
      }
      __syncthreads();
      mean = st[0];
      var = st[1];
      if (r == 0) {
        if (a.batch_mean) { a.batch_mean[col] = mean; a.batch_var[col] = var; }
        if (a.update_moving && live) {
          a.moving_mean[col] = mm_pre * a.momentum + mean * (1.f - a.momentum);
          a.moving_var[col] = mv_pre * a.momentum + var * (1.f - a.momentum);
        }
      }
    } else {
      mean = live ? a.moving_mean[col] : 0.f;
      var = live ? a.moving_var[col] : 1.f;
    }
    inv = rsqrtf(var + a.eps);
    if (r == 0 && a.inv_std) a.inv_std[col] = inv;
  }
  SMX_STAMP(0, 5);   // column statistics
  if (!on) return;
  const float scale = drop ? 1.f / (1.f - a.drop_p) : 1.f;
  const long o = (long)r * a.Hp + col;
  float y = v;
  if (a.batchnorm) {
    v = (v - mean) * inv;
    y = __builtin_fmaf(gamma, v, beta);
  }
  a.xhat[o] = v;
  float h;
  if constexpr (GEN_ACT) h = act_fwd(a.act, y);
  else {
    h = fmaxf(y, 0.f);
    if (a.leak != 0.f) h += a.leak * fminf(y, 0.f);
  }
  if (drop) {
    float mult = mpre;
    if (!a.inj_mask) {
      const uint32_t cell = a.cell_base + (uint32_t)(a.rows ? a.rows[r] : r);
      const U4 w = philox_row(a.nk, (uint32_t)r, cell, (uint32_t)(col >> 2));
      mult = dropout_mult1(w, col & 3, a.drop_p, scale);
    }
    h *= mult;
  }
  a.out[o] = live ? h : 0.f;
  SMX_STAMP(0, 6);   // stores issued
}
__global__ __launch_bounds__(BN_THREADS) void bn_wide_fwd_kernel(BnFwdArgs a) { bn_wide_fwd_body<false>(a); }
__global__ __launch_bounds__(BN_THREADS) void bn_wide_fwd_gen_kernel(BnFwdArgs a) { bn_wide_fwd_body<true>(a); }

// `lds`: BN_WIDE_BWD_SMEM_FLOATS floats, 16-byte aligned, of the calling kernel (bn_wide_bwd_dw_kernel hands over a view of a larger array)
constexpr int BN_WIDE_BWD_SMEM_FLOATS = 16 * 128 + 128 + 128 + 4;   // sh | vs | xs | st
// SEAM (bn_bwd_seam_kernel): `bid` is the column; d pre is stored write-through and published to the launch's waiting workgroups
// (smx_handoff.h) -- every thread reaches the publish.
template <bool GEN_ACT, bool SEAM = false>
__device__ inline void bn_wide_bwd_body(const BnBwdArgs& a, float* lds, const int bid, const BwdSeamArgs* sm = nullptr) {
#pragma clang fp contract(off)
  if constexpr (!SEAM) {
    const int extra = bid - a.Hp;
    if (extra >= 0) {   // the riders of bn_act_bwd_body
      const int e = extra - (a.with_metrics ? 1 : 0);
      if (e >= 0 && e < a.adam_count) { adam_chunk_body<BN_THREADS>(a.adam, a.adam_first + e); return; }
      if (threadIdx.x >= 256) return;
      if (e < 0) metrics_body(a.metrics);
      else {
        const int i = e - a.adam_count;
        if (i < a.sqr_count) sq_reduce_body(a.adam.sq_slots + a.sqr_first[i], a.sqr_n[i], a.sq_total + a.sqr_dst[i]);
        else step_close_body<false>(a.adam);
      }
      return;
    }
  }
  float* const sh = lds;
  float* const vs = lds + 16 * 128; float* const xs = vs + 128; float* const st = xs + 128;
  preload(a.dout, a.n_slabs, a.slab_stride, a.out, a.xhat, a.inv_std, a.gamma, a.B, a.H, a.Hp, a.batchnorm, a.training, a.drop_scale, a.dpre, a.dgamma, a.dbeta);
  const int col = bid, r = (int)threadIdx.x;
  const bool live = col < a.H, rowt = r < 128, on = rowt && r < a.B;
  // what the activation mask and the BatchNorm formula need of the forward pass, requested ahead of the slabs
  float ov = 0.f, xh = 0.f, gamma = 0.f, inv = 0.f;
  float xv = 0.f, beta = 0.f;   // (GEN_ACT: xhat of every layer, beta)
  if (on) {
    const long o = (long)r * a.Hp + col;
    if constexpr (GEN_ACT) {
      xv = a.xhat[o];
      if (a.batchnorm) xh = xv;
    } else {
      ov = a.out[o];
      if (a.batchnorm) xh = a.xhat[o];
    }
  }
  if (a.batchnorm) { gamma = live ? a.gamma[col] : 0.f; inv = a.inv_std[col]; }
  if constexpr (GEN_ACT) {
    if (a.batchnorm && live) beta = a.beta[col];
  }
  SMX_STAMP(2, 0);
  wide_slab_column(a.dout, a.slab_stride, a.n_slabs, col, sh);
  SMX_STAMP(2, 3);
  __syncthreads();
  float dy = 0.f;
  if (on) {
    const float acc = wide_row_value(sh, r);
    if constexpr (GEN_ACT) dy = live ? bn_gen_dy(a, r, col, acc, xv, gamma, beta) : 0.f;
    else {
      dy = (live && ov > 0.f) ? acc * a.drop_scale : 0.f;
      if (a.leak != 0.f && live && !(ov > 0.f)) dy = acc * a.leak;
    }
  }
  if (rowt) { vs[r] = dy; xs[r] = xh; }
  __syncthreads();
  if (r < 64) {   // wave 0: rows r and r + 64 in the form of bn_act_bwd_body
    float s1 = 0.f, s2 = 0.f;
    if (r < a.B) { const float d0 = vs[r]; s1 += d0; s2 += d0 * xs[r]; }
    if (r + 64 < a.B) { const float d1 = vs[r + 64]; s1 += d1; s2 += d1 * xs[r + 64]; }
    s1 = wide_tree64(s1);
    if (a.batchnorm) s2 = wide_tree64(s2);
    if (r == 0) { st[0] = s1; st[1] = s2; }
  }
  __syncthreads();
  const float s1 = st[0], s2 = st[1];
  SMX_STAMP(2, 5);
  if (!a.batchnorm) {
    if (r == 0 && a.dbias && live) a.dbias[col] = s1;
    if constexpr (SEAM) {
      if (on) handoff_store(a.dpre + (long)r * a.Hp + col, dy);
      handoff_publish(sm->seam, col);
    } else
    if (on) a.dpre[(long)r * a.Hp + col] = dy;
    return;
  }
  if (r == 0) { a.dgamma[col] = live ? s2 : 0.f; a.dbeta[col] = live ? s1 : 0.f; }
  if constexpr (SEAM) {
    if (on) {
      const float invB = 1.f / (float)a.B;
      float d;
      if (a.training) d = (gamma * inv) * __builtin_fmaf(-__builtin_fmaf(xh, s2, s1), invB, dy);
      else d = dy * gamma * inv;
      handoff_store(a.dpre + (long)r * a.Hp + col, d);
    }
    handoff_publish(sm->seam, col);
    return;
  }
  if (!on) return;
  const float invB = 1.f / (float)a.B;
  float d;
  if (a.training) d = (gamma * inv) * __builtin_fmaf(-__builtin_fmaf(xh, s2, s1), invB, dy);
  else d = dy * gamma * inv;
  a.dpre[(long)r * a.Hp + col] = d;
  SMX_STAMP(2, 6);
}
__global__ __launch_bounds__(BN_THREADS) void bn_wide_bwd_kernel(BnBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[BN_WIDE_BWD_SMEM_FLOATS];
  bn_wide_bwd_body<false>(a, lds, (int)blockIdx.x);
}
__global__ __launch_bounds__(BN_THREADS) void bn_wide_bwd_gen_kernel(BnBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[BN_WIDE_BWD_SMEM_FLOATS];
  bn_wide_bwd_body<true>(a, lds, (int)blockIdx.x);
}

// ---- bn_wide_bwd_kernel that also CARRIES the output head's dW / db / sum-of-squares slots (role 0 of out_head_bwd_kernel: smx_headdw.h) --------------
// Only the optimiser reads those, while the chain waits for the head's launch: its two roles are bound by instruction issue and add
// (4.0 + 4.9 -> 8.6 us at 128 x 1998 x 128), and this launch -- 128 light column workgroups -- leaves most of the chip idle.  Blocks
// [0, Hp): the BatchNorm columns (the chain waits for these: dispatched first); then the riders as bn_wide_bwd_body indexes them; the LAST
// h.n_w blocks: the head's dW tiles, block index rebased to 0.  A kernel of its own: role 0 needs 64 KB of LDS for two planes' partial tiles,
// every other bn_wide_bwd launch keeps its 9 KB.  One array, each body its view (the maximum of the two, not their sum).
// The plain (not SEP) bf16 x 3 form with 2 or 3 planes.  The head's arguments are a second by-value argument, never indexed at run time
// (wgrad_group_kernel's note on scratch copies, smx_headbwd.hip).
template <int NP>
__global__ __launch_bounds__(BN_THREADS) void bn_wide_bwd_dw_kernel(BnBwdArgs a, HeadBwdArgs h) {
  static_assert(SMX_HEAD_DW_SMEM_FLOATS >= BN_WIDE_BWD_SMEM_FLOATS && BN_THREADS == 512, "bn_wide_bwd_dw: role 0 is a 512-thread body with the larger LDS need");
  __shared__ __attribute__((aligned(16))) float lds[SMX_HEAD_DW_SMEM_FLOATS];
  const int first_dw = (int)gridDim.x - h.n_w;
  if ((int)blockIdx.x >= first_dw) {   // (block-uniform)
    preload(h.D, h.ldd, h.dP, h.ldp, h.dW, h.ldw, h.db, h.B, h.Gp, h.sq_part, h.n_w, h.n_ht, h.n_gt, h.diag, h.Hp, h.n_planes);   // (one batch: smx_device.h)
    head_dw_body<NP, 0, 1>(h, (int)blockIdx.x - first_dw, lds);
    return;
  }
  bn_wide_bwd_body<false>(a, lds, (int)blockIdx.x);
}

// a: a wide BatchNorm-backward launch as launch_bn_act_bwd takes it (ReLU); h: the head's arguments as launch_out_head_bwd takes them (its d d fields unread)
bool bn_wide_bwd_dw_supported(const BnBwdArgs& a, const HeadBwdArgs& h) {
  return a.wide && !a.front && a.act == SMX_ACT_RELU && a.Hp % BN_COLS == 0 && a.B > 0 && a.B <= 128 && a.Hp <= 128 &&
         !h.sep && h.bf16x3 && h.n_extra == 0 && (h.n_planes == 2 || h.n_planes == 3) && h.B == a.B && h.B > 0 && h.Hp % 32 == 0 && h.Gp % 32 == 0;
}
int launch_bn_wide_bwd_dw(hipStream_t st, const BnBwdArgs& a, const HeadBwdArgs& h_in) {
  HeadBwdArgs h = h_in;
  if (!bn_wide_bwd_dw_supported(a, h) || !a.dout || a.slab_stride < (long)a.Hp * 128 || (a.slab_stride % 4) || !h.D || !h.dP || !h.dW || !h.db || h.ldd < h.Hp ||
      h.ldp < (long)h.n_planes * h.Gp || h.ldw < (long)h.n_planes * h.Gp) {
    set_error("bn_wide_bwd_dw: bad shapes");
    return SMX_ERR_INVALID;
  }
  h.n_ht = h.Hp / 32; h.n_gt = h.Gp / 32; h.n_ct = (h.B + 31) / 32;
  h.n_w = h.n_ht * ((h.n_gt + 7) / 8 * 8);
  h.skip_dd = 1; h.skip_dw = 0; h.diag = 0;
  { static const int dg = (int)tuning("head_bwd_diag", 0); if (dg) h.diag = dg; }   // (timing only: bit 1 = the dW tiles return at once)
  if (h.sq_count) *h.sq_count = h.n_ht * h.n_gt * 8;
  const dim3 grid((unsigned)(a.Hp + (a.with_metrics ? 1 : 0) + a.adam_count + a.sqr_count + (a.close ? 1 : 0) + h.n_w));
  if (h.n_planes == 3) hipLaunchKernelGGL(bn_wide_bwd_dw_kernel<3>, grid, dim3(BN_THREADS), 0, st, a, h);
  else hipLaunchKernelGGL(bn_wide_bwd_dw_kernel<2>, grid, dim3(BN_THREADS), 0, st, a, h);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ---- the carrier above and the encoder's fold_dz launch behind it in ONE launch (smx_handoff.h; smx_backward.hip: the seam form) ----------------------
// The encoder's enc.Hp / 8 chain workgroups (at most HANDOFF_MAX_WAITERS) wait for nothing but d pre_dec, the 64 KB the decoder's Hp column
// workgroups write: in one launch they run everything that does not read it -- argument fields, the W_dec image, their rows of W_lat, the latent
// head's operands, out / xhat / gamma / inv_std of their columns -- while the columns work, and wait inside the launch.  The same device
// functions as the two launches, SEAM forms: the same additions in the same order, the same bits.  Block order: the Hp columns, the chain
// workgroups straight behind them (sm.cons_first: ahead of them -- results do not depend on it, smx_handoff.h: Progress), then the riders that read
// nothing the launch writes -- the ELBO scalars (enc.with_metrics), W_enc's lazy chunks (dec.adam*), the step's close (enc.close) --, then the
// head's dW tiles.  The head's optimiser riders read what the tiles write: they are not here (smx_backward.hip).  One LDS array, each body its view.
template <int NP>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_seam_kernel(BnBwdArgs dec, BnBwdArgs enc, HeadBwdArgs h, BwdSeamArgs sm) {
  extern __shared__ __attribute__((aligned(16))) float ds[];
  const int b = (int)blockIdx.x, np = dec.Hp, nc = enc.Hp / BN_COLS;
  const int first_dw = (int)gridDim.x - h.n_w;
  if (b >= first_dw) {   // (block-uniform, like every branch below)
    preload(h.D, h.ldd, h.dP, h.ldp, h.dW, h.ldw, h.db, h.B, h.Gp, h.sq_part, h.n_w, h.n_ht, h.n_gt, h.diag, h.Hp, h.n_planes);
    head_dw_body<NP, 0, 1>(h, b - first_dw, ds);
    return;
  }
  if (b < np + nc) {
    const bool cons = sm.cons_first ? b < nc : b >= np;
    if (cons) bn_act_bwd_body<2, 1, false, true>(enc, sm.cons_first ? b : b - np, &sm);
    else bn_wide_bwd_body<false, true>(dec, ds, sm.cons_first ? b - nc : b, &sm);
    return;
  }
  int e = b - np - nc;
  if (enc.with_metrics) {
    if (e == 0) { if (threadIdx.x < 256) metrics_body(enc.metrics); return; }
    --e;
  }
  if (e < dec.adam_count) { adam_chunk_body<BN_THREADS>(dec.adam, dec.adam_first + e); return; }
  if (enc.close && threadIdx.x < 256) step_close_body<false>(enc.adam);
}

bool bn_bwd_seam_supported(const BnBwdArgs& dec, const BnBwdArgs& enc, const HeadBwdArgs& h) {
  return bn_wide_bwd_dw_supported(dec, h) && !dec.with_metrics && !dec.close && dec.sqr_count == 0 && dec.dpre &&
         enc.front && enc.fold_dz && enc.act == SMX_ACT_RELU && enc.B == dec.B && enc.B <= BN_RL * 2 && enc.Hp % BN_COLS == 0 &&
         enc.Hp / BN_COLS <= HANDOFF_MAX_WAITERS && enc.adam_count == 0 && enc.sqr_count == 0 && enc.zD == dec.dpre && enc.zld == dec.Hp && dec.Hp == 128 &&
         bn_bwd_front_supported(enc.B, enc.fK) && bn_bwd_fold_supported(enc.B, enc.fK, enc.zlb.Dp);
}
int launch_bn_bwd_seam(hipStream_t st, const BnBwdArgs& dec, const BnBwdArgs& enc_in, const HeadBwdArgs& h_in, const BwdSeamArgs& sm) {
  HeadBwdArgs h = h_in;
  BnBwdArgs enc = enc_in;
  enc.diag = 0;
  const EpiLatentBwd& e = enc.zlb;
  if (!bn_bwd_seam_supported(dec, enc, h) || !dec.dout || dec.slab_stride < (long)dec.Hp * 128 || (dec.slab_stride % 4) || !h.D || !h.dP || !h.dW || !h.db || h.ldd < h.Hp ||
      h.ldp < (long)h.n_planes * h.Gp || h.ldw < (long)h.n_planes * h.Gp || !enc.fD || !enc.fW || (enc.fld % 4) || (enc.fldw % 4) || !enc.zW || (enc.zld % 4) || (enc.zldw % 4) ||
      enc.zldw < 128 || !e.lat || !e.sig || !e.eps || !e.dlat || !e.stochastic || e.dklz || e.dz_add || (e.ld % 4) || e.ld < 2 * e.Dp ||
      !sm.seam.counter || !sm.seam.error || sm.seam.target == 0 || sm.seam.shards < 1 || sm.seam.shards > HANDOFF_MAX_SHARDS || (sm.seam.shards & (sm.seam.shards - 1))) {
    set_error("bn_bwd_seam: bad shapes");
    return SMX_ERR_INVALID;
  }
  h.n_ht = h.Hp / 32; h.n_gt = h.Gp / 32; h.n_ct = (h.B + 31) / 32;
  h.n_w = h.n_ht * ((h.n_gt + 7) / 8 * 8);
  h.skip_dd = 1; h.skip_dw = 0; h.diag = 0;
  if (h.sq_count) *h.sq_count = h.n_ht * h.n_gt * 8;
  size_t lds = ((size_t)enc.B * (enc.fK + 4) + (size_t)BN_COLS * (enc.fK + 4)) * sizeof(float) + SMX_FOLD_WIMG_BYTES;
  lds = std::max(lds, (size_t)SMX_HEAD_DW_SMEM_FLOATS * sizeof(float));
  static_assert(SMX_HEAD_DW_SMEM_FLOATS >= BN_WIDE_BWD_SMEM_FLOATS, "bn_bwd_seam: the column body's view fits the head's");
  static const bool ok3 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bn_bwd_seam_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
  static const bool ok2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bn_bwd_seam_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
  if (!ok3 || !ok2 || lds > 96 * 1024) { set_error("bn_bwd_seam: cannot reserve the dynamic LDS"); return SMX_ERR_HIP; }
  const dim3 grid((unsigned)(dec.Hp + enc.Hp / BN_COLS + (enc.with_metrics ? 1 : 0) + dec.adam_count + (enc.close ? 1 : 0) + h.n_w));
  if (h.n_planes == 3) hipLaunchKernelGGL(bn_bwd_seam_kernel<3>, grid, dim3(BN_THREADS), lds, st, dec, enc, h, sm);
  else hipLaunchKernelGGL(bn_bwd_seam_kernel<2>, grid, dim3(BN_THREADS), lds, st, dec, enc, h, sm);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

bool bn_wide_supported(int B, int Hp, int n_slabs) { return B > 0 && B <= 128 && Hp > 0 && Hp <= 128 && n_slabs > 0 && !tuning_on("no_bn_wide"); }

// ===========================================================================
// SyncBatchNorm (opt-in under data parallelism, SURVEY.md 8e caveat i): statistics over the GLOBAL minibatch.
// Each BatchNorm pass is cut in two around one small all-reduce: the first launch leaves this rank's column
// statistics in its own slot of a [world][2][Hp] buffer (zeros in the other slots, so that the sum all-reduce
// is an all-gather), the second combines the slots in rank order -- Chan's pairwise form, no E[x^2] - E[x]^2
// cancellation -- and finishes the pass.  Equal batch sizes on every rank.  Plain row loops: the values make the
// round trip through xhat / dpre (the register-resident forms are for the single collective-free launch).
// ===========================================================================
__global__ __launch_bounds__(BN_THREADS) void bn_sync_stats_fwd_kernel(BnFwdArgs a, BnSyncArgs y) {
  __shared__ float sh[BN_WAVES * BN_COLS];
  const int c = threadIdx.x % BN_COLS, rl = threadIdx.x / BN_COLS;
  const int col = blockIdx.x * BN_COLS + c;
  float s1 = 0.f;
  for (int r0 = 0; r0 < a.B; r0 += BN_RL * 2) {
    float acc[2];
    slab_sum<2>(a.pre, a.n_slabs, a.slab_stride, a.ld, col, r0, rl, a.B, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = r0 + rl + BN_RL * i;
      if (r < a.B) { a.xhat[(long)r * a.Hp + col] = acc[i]; s1 += acc[i]; }
    }
  }
  s1 = bn_col_reduce(s1, sh);
  const float mean = s1 / (float)a.B;
  float s2 = 0.f;
  for (int r = rl; r < a.B; r += BN_RL) { const float d = a.xhat[(long)r * a.Hp + col] - mean; s2 += d * d; }
  s2 = bn_col_reduce(s2, sh);
  if (rl == 0)
    for (int r = 0; r < y.world; ++r) {
      y.gather[((long)r * 2 + 0) * a.Hp + col] = r == y.rank ? mean : 0.f;
      y.gather[((long)r * 2 + 1) * a.Hp + col] = r == y.rank ? s2 : 0.f;
    }
}

template <bool GEN_ACT>
__device__ inline void bn_sync_apply_fwd_body(const BnFwdArgs& a, const BnSyncArgs& y) {
  const int c = threadIdx.x % BN_COLS, rl = threadIdx.x / BN_COLS;
  const int col = blockIdx.x * BN_COLS + c;
  const bool live = col < a.H;
  float mean = 0.f;
  for (int r = 0; r < y.world; ++r) mean += y.gather[((long)r * 2) * a.Hp + col];
  mean /= (float)y.world;
  float m2 = 0.f;
  for (int r = 0; r < y.world; ++r) {
    const float d = y.gather[((long)r * 2) * a.Hp + col] - mean;
    m2 += y.gather[((long)r * 2 + 1) * a.Hp + col] + (float)a.B * d * d;
  }
  const float var = m2 / ((float)a.B * (float)y.world);
  const float inv = rsqrtf(var + a.eps);
  const float gamma = live ? a.gamma[col] : 0.f, beta = live ? a.beta[col] : 0.f;
  if (rl == 0) {
    if (a.batch_mean) { a.batch_mean[col] = mean; a.batch_var[col] = var; }
    if (a.inv_std) a.inv_std[col] = inv;
  }
  const bool drop = a.training && a.drop_p > 0.f;
  const float scale = drop ? 1.f / (1.f - a.drop_p) : 1.f;
  for (int r = rl; r < a.B; r += BN_RL) {
    const long o = (long)r * a.Hp + col;
    const float v = (a.xhat[o] - mean) * inv;
    a.xhat[o] = v;
    float h;
    if constexpr (GEN_ACT) h = act_fwd(a.act, __builtin_fmaf(gamma, v, beta));   // (the y bn_gen_dy recomputes)
    else h = fmaxf(gamma * v + beta, 0.f);
    if (drop) {
      float mult;
      if (a.inj_mask) mult = a.inj_mask[(long)r * a.inj_ld + col];
      else {
        const uint32_t cell = a.cell_base + (uint32_t)(a.rows ? a.rows[r] : r);
        mult = dropout_mult1(philox_row(a.nk, (uint32_t)r, cell, (uint32_t)(col >> 2)), col & 3, a.drop_p, scale);
      }
      h *= mult;
    }
    a.out[o] = live ? h : 0.f;
  }
}
__global__ __launch_bounds__(BN_THREADS) void bn_sync_apply_fwd_kernel(BnFwdArgs a, BnSyncArgs y) { bn_sync_apply_fwd_body<false>(a, y); }
__global__ __launch_bounds__(BN_THREADS) void bn_sync_apply_fwd_gen_kernel(BnFwdArgs a, BnSyncArgs y) { bn_sync_apply_fwd_body<true>(a, y); }

template <bool GEN_ACT>
__device__ inline void bn_sync_stats_bwd_body(const BnBwdArgs& a, const BnSyncArgs& y) {
  __shared__ float sh[BN_WAVES * BN_COLS];
  const int c = threadIdx.x % BN_COLS, rl = threadIdx.x / BN_COLS;
  const int col = blockIdx.x * BN_COLS + c;
  const bool live = col < a.H;
  float gamma_g = 0.f, beta_g = 0.f;
  if constexpr (GEN_ACT) {
    if (live) { gamma_g = a.gamma[col]; beta_g = a.beta[col]; }
  }
  float s1 = 0.f, s2 = 0.f;
  for (int r0 = 0; r0 < a.B; r0 += BN_RL * 2) {
    float acc[2];
    slab_sum<2>(a.dout, a.n_slabs, a.slab_stride, a.ld, col, r0, rl, a.B, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = r0 + rl + BN_RL * i;
      if (r < a.B) {
        const long o = (long)r * a.Hp + col;
        float dy;
        if constexpr (GEN_ACT) dy = live ? bn_gen_dy(a, r, col, acc[i], a.xhat[o], gamma_g, beta_g) : 0.f;
        else dy = (live && a.out[o] > 0.f) ? acc[i] * a.drop_scale : 0.f;
        a.dpre[o] = dy;
        s1 += dy;
        s2 += dy * a.xhat[o];
      }
    }
  }
  s1 = bn_col_reduce(s1, sh);
  s2 = bn_col_reduce(s2, sh);
  if (rl == 0) {
    // this rank's share of the parameter gradients: the gradient all-reduce sums the shares
    a.dgamma[col] = live ? s2 : 0.f;
    a.dbeta[col] = live ? s1 : 0.f;
    for (int r = 0; r < y.world; ++r) {
      y.gather[((long)r * 2 + 0) * a.Hp + col] = r == y.rank ? s1 : 0.f;
      y.gather[((long)r * 2 + 1) * a.Hp + col] = r == y.rank ? s2 : 0.f;
    }
  }
}
__global__ __launch_bounds__(BN_THREADS) void bn_sync_stats_bwd_kernel(BnBwdArgs a, BnSyncArgs y) { bn_sync_stats_bwd_body<false>(a, y); }
__global__ __launch_bounds__(BN_THREADS) void bn_sync_stats_bwd_gen_kernel(BnBwdArgs a, BnSyncArgs y) { bn_sync_stats_bwd_body<true>(a, y); }

__global__ __launch_bounds__(BN_THREADS) void bn_sync_apply_bwd_kernel(BnBwdArgs a, BnSyncArgs y) {
  const int c = threadIdx.x % BN_COLS, rl = threadIdx.x / BN_COLS;
  const int col = blockIdx.x * BN_COLS + c;
  const bool live = col < a.H;
  float s1 = 0.f, s2 = 0.f;
  for (int r = 0; r < y.world; ++r) {
    s1 += y.gather[((long)r * 2 + 0) * a.Hp + col];
    s2 += y.gather[((long)r * 2 + 1) * a.Hp + col];
  }
  const float gamma = live ? a.gamma[col] : 0.f;
  const float inv = a.inv_std[col];
  const float invN = 1.f / ((float)a.B * (float)y.world);
  for (int r = rl; r < a.B; r += BN_RL) {
    const long o = (long)r * a.Hp + col;
    a.dpre[o] = gamma * inv * (a.dpre[o] - invN * (s1 + a.xhat[o] * s2));
  }
}

int launch_bn_sync_fwd(hipStream_t st, const BnFwdArgs& a, const BnSyncArgs& y, int phase) {
  if (a.Hp % BN_COLS || a.B <= 0 || !a.batchnorm || !a.training || y.world < 1 || !y.gather) { set_error("bn_sync_fwd: bad arguments"); return SMX_ERR_INVALID; }
  if (a.leak != 0.f) { set_error("bn_sync_fwd: no leaky form (the only leaky layers, the discriminator's, have no BatchNorm)"); return SMX_ERR_INVALID; }
  if (phase == 0) hipLaunchKernelGGL(bn_sync_stats_fwd_kernel, dim3(a.Hp / BN_COLS), dim3(BN_THREADS), 0, st, a, y);
  else if (a.act != SMX_ACT_RELU) hipLaunchKernelGGL(bn_sync_apply_fwd_gen_kernel, dim3(a.Hp / BN_COLS), dim3(BN_THREADS), 0, st, a, y);
  else hipLaunchKernelGGL(bn_sync_apply_fwd_kernel, dim3(a.Hp / BN_COLS), dim3(BN_THREADS), 0, st, a, y);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
int launch_bn_sync_bwd(hipStream_t st, const BnBwdArgs& a, const BnSyncArgs& y, int phase) {
  if (a.Hp % BN_COLS || a.B <= 0 || !a.batchnorm || !a.training || y.world < 1 || !y.gather) { set_error("bn_sync_bwd: bad arguments"); return SMX_ERR_INVALID; }
  if (a.leak != 0.f) { set_error("bn_sync_bwd: no leaky form (the only leaky layers, the discriminator's, have no BatchNorm)"); return SMX_ERR_INVALID; }
  if (a.act != SMX_ACT_RELU && (!a.xhat || !a.beta)) { set_error("bn_sync_bwd: activations other than ReLU need xhat and beta"); return SMX_ERR_INVALID; }
  if (phase == 0 && a.act != SMX_ACT_RELU) hipLaunchKernelGGL(bn_sync_stats_bwd_gen_kernel, dim3(a.Hp / BN_COLS), dim3(BN_THREADS), 0, st, a, y);
  else if (phase == 0) hipLaunchKernelGGL(bn_sync_stats_bwd_kernel, dim3(a.Hp / BN_COLS), dim3(BN_THREADS), 0, st, a, y);
  else hipLaunchKernelGGL(bn_sync_apply_bwd_kernel, dim3(a.Hp / BN_COLS), dim3(BN_THREADS), 0, st, a, y);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

}  // namespace smx

#ifdef SMX_STAMPS
extern "C" int smx_dbg_stamps_bn(long long* out) {   // development builds only (tools/c2_stamps.sh): this unit's stamp table [16][16]
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(smx::smx_tu_stamps), sizeof(long long) * 256) == hipSuccess ? 0 : -1;
}
#endif
