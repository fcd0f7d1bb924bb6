// smx_block.h -- the workgroup building blocks of the model-free analysis kernels (smx_impute, smx_correlate, smx_cluster, smx_gmm,
// smx_gmm_full, smx_knn, smx_tsne, smx_umap, smx_mi, smx_rankgroups, smx_mbkmeans, smx_louvain, smx_data, smx_prep), for 256-thread workgroups of four waves.  These pieces carry the entries'
// determinism promises (the same bits for every chunking, exact ranks, exact order statistics), so each exists once:
//   sums    the lanes of a wave by halving (lane l += lane l + 32, 16, .. 1: the result in lane 0), then the four waves as
//           (0 + 1) + (2 + 3).  NOT the order of smx_device.h's float wave_sum / block_sum (the training step's), which stay where they are.
//   scans   inclusive over the lanes of a wave, add and max.
//   keys    the order-preserving unsigned pattern of a float32 / float64, -0 as +0.
//   sort    a stable LSD radix sort of cell indices by a key functor, and the tie-run pass over its result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smx {

// what a wave wrote to its own LDS words is read back by its other lanes (the project's idiom: smx_loss.h)
__device__ inline void wave_lds_sync() { __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier(); }

// ---- fixed-order sums ----------------------------------------------------------------------------------------------------------------
template <class T>
__device__ inline T halving_wave_sum(T v) {   // the wave's sum in lane 0 (the other lanes hold partial sums)
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the workgroup's sum in every thread; sh4: 4 words of LDS, free for reuse once every thread has its result (the first barrier of the
// next call comes after every read of this one)
template <class T>
__device__ inline T halving_block_sum(T v, T* sh4) {
  v = halving_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}

// the sum of x [n]: thread t adds x[t], x[t + 256], ... in this order, then the workgroup's sum -- an order that is a function of n alone
template <class T>
__device__ inline T halving_column_sum(const T* x, long n, T* sh4) {
  T v = 0;
  for (long i = threadIdx.x; i < n; i += 256) v += x[i];
  return halving_block_sum(v, sh4);
}

// the wave's float64 sum in EVERY lane: the xor butterfly (lane l += lane l ^ 32, 16, .. 1)
__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- inclusive scans over the lanes of a wave ----------------------------------------------------------------------------------------
__device__ inline unsigned wave_scan_add(unsigned v) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ inline double wave_scan_add(double v) {   // lane l: ((v_0 + ..) ..) in the doubling order of the scan -- a function of l alone
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ inline unsigned wave_scan_max(unsigned v) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (lane >= o) v = max(v, t);
  }
  return v;
}

// ---- order-preserving keys: negative values below positive ones, -0 as +0 ------------------------------------------------------------
__device__ inline uint32_t order_key(float v) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline uint64_t order_key(double v) {
  uint64_t u = (uint64_t)__double_as_longlong(v);
  if (u == 0x8000000000000000ull) u = 0ull;
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

// an infinity or a NaN: the exponent all ones
__device__ inline bool is_nonfinite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }
__device__ inline bool is_nonfinite(double v) { return ((uint64_t)__double_as_longlong(v) & 0x7FF0000000000000ull) == 0x7FF0000000000000ull; }

// ---- column radix sort ---------------------------------------------------------------------------------------------------------------
struct SortShared { unsigned hist[4][256]; unsigned wtot[4]; };

// The cell indices `init` [N] (NULL: the identity) sorted by key(cell), stable, `passes` 8-bit LSD passes over the ping-pong arrays A and B
// in global memory (4 N bytes each: cache-resident; pass p writes A when p is even, B when odd).  A wave owns a contiguous quarter of the
// positions: its digit counts are its own LDS histogram, the offsets come from one scan over (digit, wave), and inside a tile of 64 the
// order among equal digits is a ballot -- no workgroup barrier inside a pass.  Returns the array that holds the result.  Called by all
// 256 threads.
template <class KeyFn>
__device__ inline unsigned* block_radix_sort(KeyFn key, int N, int passes, const unsigned* init, unsigned* A, unsigned* B, SortShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int seg = (N + 255) / 256 * 64;   // wave w owns the positions [p0, p1): whole tiles of 64, in order
  const int p0 = min(N, w * seg), p1 = min(N, p0 + seg);
  const unsigned* src = init;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 8 * pass;
    unsigned* dst = (pass & 1) ? B : A;
    for (int i = tid; i < 1024; i += 256) (&sh.hist[0][0])[i] = 0;
    __syncthreads();
    for (int p = p0 + lane; p < p1; p += 64) atomicAdd(&sh.hist[w][(unsigned)(key(src ? src[p] : (unsigned)p) >> shift) & 255u], 1u);
    __syncthreads();
    {   // thread = digit: where each wave's entries of the digit go = entries of smaller digits + those of earlier waves
      const unsigned h0 = sh.hist[0][tid], h1 = sh.hist[1][tid], h2 = sh.hist[2][tid], h3 = sh.hist[3][tid];
      const unsigned tot = h0 + h1 + h2 + h3;
      const unsigned inc = wave_scan_add(tot);
      if (lane == 63) sh.wtot[w] = inc;
      __syncthreads();
      unsigned exc = inc - tot;
      for (int q = 0; q < w; ++q) exc += sh.wtot[q];
      sh.hist[0][tid] = exc; sh.hist[1][tid] = exc + h0; sh.hist[2][tid] = exc + h0 + h1; sh.hist[3][tid] = exc + h0 + h1 + h2;
    }
    __syncthreads();
    for (int p = p0; p < p1; p += 64) {   // (wave-uniform bounds: every lane takes part in the ballots)
      const bool on = p + lane < p1;
      unsigned i = 0, d = 0;
      if (on) {
        i = src ? src[p + lane] : (unsigned)(p + lane);
        d = (unsigned)(key(i) >> shift) & 255u;
      }
      unsigned long long peers = __ballot(on);   // the tile's lanes with this lane's digit
      for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long mb = __ballot(bit);
        peers &= bit ? mb : ~mb;
      }
      const unsigned before = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
      unsigned o = 0;
      if (on) {
        o = sh.hist[w][d];
        dst[o + before] = i;
      }
      wave_lds_sync();
      if (on && before == 0) sh.hist[w][d] = o + (unsigned)__popcll(peers);
      wave_lds_sync();
    }
    __syncthreads();   // (the pass's stores are drained: the next pass reads them through the CU's own cache)
    src = dst;
  }
  return const_cast<unsigned*>(src);
}

// Runs of equal keys over the sorted order S [N]: a max-scan of the run heads gives every position its run's start.  Calls
// emit(j, cell, start) for every position j; the run's tail stores its position at A[start], so after the call A[start] is the run's last
// position for every thread.  A is not S.  Called by all 256 threads.
template <class KeyFn, class EmitFn>
__device__ inline void block_tie_runs(KeyFn key, EmitFn emit, int N, const unsigned* S, unsigned* A, SortShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned carry = 0;
  for (int t0 = 0; t0 < N; t0 += 256) {
    const int j = t0 + tid;
    const bool on = j < N;
    unsigned ci = 0;
    bool head = false, tail = false;
    if (on) {
      ci = S[j];
      const auto kj = key(ci);
      head = j == 0 || key(S[j - 1]) != kj;
      tail = j == N - 1 || key(S[j + 1]) != kj;
    }
    const unsigned v = wave_scan_max(head ? (unsigned)j : 0u);
    if (lane == 63) sh.wtot[w] = v;
    __syncthreads();
    unsigned start = max(v, carry);
    for (int q = 0; q < w; ++q) start = max(start, sh.wtot[q]);
    carry = max(carry, max(max(sh.wtot[0], sh.wtot[1]), max(sh.wtot[2], sh.wtot[3])));
    if (on) {
      emit(j, ci, start);
      if (tail) A[start] = (unsigned)j;
    }
    __syncthreads();
  }
}

}  // namespace smx
