// smx_headdw.h -- role 0 of the output head's backward (dW_out = d^T dP, db, the tensor's sum-of-squares slots; smx_headbwd.hip has the
// scheme) as a device function: a 32 x 32 tile per workgroup of 512 threads, 8 waves split the minibatch, the planes' eight partial
// tiles meet in LDS.  Two kernels call it: out_head_bwd_kernel (smx_headbwd.hip), beside the d d role, and bn_wide_bwd_dw_kernel
// (smx_bn.hip), which carries it in the decoder's BatchNorm-backward launch -- only the optimiser reads these results, the chain
// does not wait for them.  One body: the same instructions, the same order of additions, the same bits from either launch.
// Include it BEHIND the unit's SMX_STAMP_TABLE (its stamps go to the including unit's table, slot 4).
#pragma once
#include "smx_device.h"
#include "smx_internal.h"

namespace smx {

#define SMX_HEAD_DW_SMEM_FLOATS (2 * 8 * 1024)   // two planes' eight partial tiles (64 KB)

// `bid`: the tile's block index in [0, a.n_w) -- blocks 8 apart share an XCD: the (H / 32) workgroups of a gene tile are 8 blocks apart
// SEP: the planes are separate tensors (scvi's heads); B3: bf16 MFMAs on three-way split operands (smx_device.h)
template <int NP, int SEP, int B3>
__device__ __forceinline__ void head_dw_body(const HeadBwdArgs& a, const int bid, float* red /*[SMX_HEAD_DW_SMEM_FLOATS]*/) {
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = lane & 31, hh = lane >> 5;
  // accumulator register r of a 32 x 32 tile is row (r & 3) + 8 (r >> 2) + 4 hh, column i; wave q finishes r = 2q, 2q + 1
  int rowof[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) { const int r = 2 * q + j; rowof[j] = (r & 3) + 8 * (r >> 2) + 4 * hh; }
  const int xcd = bid & 7, idx = bid >> 3;
  const int ht = idx % a.n_ht, gt = (idx / a.n_ht) * 8 + xcd;
  if (gt >= a.n_gt || (a.diag & 1)) return;
  const int h0 = ht * 32, g0 = gt * 32;
  smx_f32x16 acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
  float csum[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) csum[p] = 0.f;
  SMX_STAMP(4, 0);   // entry (role 0: a dW tile)
  for (int kc = 0; kc < a.B; kc += 128) {
    const int k0 = kc + 16 * q + 8 * hh;
    if (kc + 16 * q >= a.B) break;   // wave-uniform
    float av[8], bv[NP][8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int cell = min(k0 + s, a.B - 1);
      av[s] = a.D[(long)cell * a.ldd + h0 + i];
#pragma unroll
      for (int p = 0; p < NP; ++p) bv[p][s] = a.dP[(long)cell * a.ldp + (long)p * a.Gp + g0 + i];
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (B3) {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bool on = k0 + s < a.B;     // K is the (ragged) minibatch axis: cells beyond it contribute nothing
        av[s] = on ? av[s] : 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) { bv[p][s] = on ? bv[p][s] : 0.f; csum[p] += bv[p][s]; }
      }
      const Split8 sa = split3x8(av);
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p] = mfma_bf16x3(sa, split3x8(bv[p]), acc[p]);
    } else {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bool on = k0 + s < a.B;       // K is the (ragged) minibatch axis: cells beyond it contribute nothing
        const float av_s = on ? av[s] : 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const float b = on ? bv[p][s] : 0.f;
          csum[p] += b;
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av_s, b, acc[p], 0, 0, 0);
        }
      }
    }
  }
  SMX_STAMP(4, 1);   // the products over the minibatch (loads in flight included)
  float sq = 0.f;
  // planes 0 and 1 go through LDS TOGETHER (two slots of eight partial tiles), the third plane behind them: three barriers for three planes
  // (one for two) instead of five (three); the partial tiles of a plane are added in the same order as one plane at a time
  auto park = [&](int p, float* slot) {
#pragma unroll
    for (int r = 0; r < 16; ++r) slot[(q * 16 + r) * 64 + lane] = acc[p][r];
  };
  auto finish = [&](int p, const float* slot) {
    if (SEP) sq = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = 2 * q + j;
      float t = slot[(0 * 16 + r) * 64 + lane];
#pragma unroll
      for (int w = 1; w < 8; ++w) t += slot[(w * 16 + r) * 64 + lane];
      const int h = h0 + rowof[j];
      if (SEP) a.dWp[p][(long)h * a.ldw + g0 + i] = t;
      else a.dW[(long)h * a.ldw + (long)p * a.Gp + g0 + i] = t;   // rows >= H and columns >= G are zero by construction
      sq += t * t;
    }
    if (SEP && a.sqp[p]) {
      const float sw = wave_sum(sq);
      if (lane == 0) a.sqp[p][((long)ht * a.n_gt + gt) * 8 + q] = sw;
    }
  };
  park(0, red); park(1, red + 8 * 1024);
  __syncthreads();
  finish(0, red); finish(1, red + 8 * 1024);
  if constexpr (NP == 3) {
    __syncthreads();
    park(2, red);
    __syncthreads();
    finish(2, red);
  }
  if (!SEP && a.sq_part) {
    sq = wave_sum(sq);
    if (lane == 0) a.sq_part[((long)ht * a.n_gt + gt) * 8 + q] = sq;   // 8 slots per (H tile, gene tile): <= 4 per 32 x 32 tile
  }
  if (ht == 0) {   // bias gradient: column sums of dP over the whole minibatch (each lane holds its K slice's part)
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NP; ++p) red[(q * NP + p) * 64 + lane] = csum[p];
    __syncthreads();
    if (q < NP && lane < 32) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) t += red[(w * NP + q) * 64 + lane] + red[(w * NP + q) * 64 + 32 + lane];
      if (SEP) {   // (q is wave-uniform; the pointer array is indexed with constants only)
        float* dbq = q == 0 ? a.dbp[0] : (q == 1 ? a.dbp[1] : a.dbp[2]);
        dbq[g0 + lane] = t;
      } else a.db[(long)q * a.Gp + g0 + lane] = t;
    }
  }
  SMX_STAMP(4, 2);   // the planes' partial tiles summed, dW / db / sum of squares stored
}

}  // namespace smx
