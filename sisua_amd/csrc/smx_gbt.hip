// smx_gbt.hip -- gradient-boosted classification trees on a histogram of the count matrix: what the reference's
// SingleCellOMIC.get_importance_matrix (_single_cell_analysis.py:1107-1145), Posterior.cal_importance and cal_dci ask of scikit-learn's
// GradientBoostingClassifier (loss='log_loss', criterion='friedman_mse', no subsampling), with every sum an integer so that the result is
// one answer whatever the order (tests/gbt_ref.py restates it in NumPy).  Model-free entries: they upload, compute,
// download and free their own buffers.
//   the bins          one workgroup per column radix-sorts it (block_radix_sort, float32 keys).  At most 256 distinct values: a bin per
//                     value; more: a cut between the sorted positions p - 1 and p, p = floor(j N / 256), j = 1 .. 255, where the values
//                     differ.  A threshold is the float32 midpoint a/2 + b/2 (a where that rounds to b).  The bin matrix is one byte per
//                     entry, feature-major [G][ldn]: a workgroup of the sweep reads its feature's cells as consecutive bytes.
//   the statistics    per stage and class the residual y_k - p_k and the curvature p_k (1 - p_k) as rint(v 2^40) int64.
//   a tree level      the K trees of a stage grow together, four launches per level: (1) per (class, node) the sums of r and h and the
//                     count, integer LDS atomics per 4096 cells, then integer global atomics; (2) the sweep: workgroup (feature, pass)
//                     streams the cells once and fills the (class, node, bin) histograms of the pass's GBT_PASS (class, node) pairs in
//                     LDS (int64 sums, uint32 counts: 12 B x 256 x 16 = 48 KiB), a wave per pair scans the bins (a lane 4 bins, the lanes
//                     by the doubling scan -- integers) and keeps the feature's best candidate: improvement SL SL / nL + SR SR / nR -
//                     S S / n in float64 from the integers, in that order without contraction, the largest, then the lowest bin; (3) a
//                     workgroup per (class, node) takes the largest over the features, then the lowest feature -- a total order, so the
//                     shape of the reduction changes nothing -- and writes the node record; (4) the cells move to their children.
//                     The pass size changes which workgroup holds a pair, never a sum.
//   the stage loop    softmax / sigmoid -> statistics and the loss (a workgroup's 256 losses by halving, the workgroups in order), the
//                     D + 1 levels, raw += learning_rate * leaf value.  The host reads two scalars per stage.
// A tree is kept in heap order: node t has the children 2 t + 1 and 2 t + 2, M = 2^(max_depth + 1) - 1 slots, an unreached slot has n = 0.
// No float atomics and no float accumulation across workgroups except the loss (fixed order).  Every loop is bounded by N, G, K, the 256
// bins, the depth or the number of stages.
#include "smx_model.h"
#include "smx_prep.h"    // the block streamer of the count matrix
#include "smx_block.h"   // the column sort, the scans, the fixed-order sums

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace smx {

#define GBT_MAX_CELLS (1 << 20)
#define GBT_MAX_GENES 32768
#define GBT_MAX_CLASSES 32
#define GBT_MAX_DEPTH 6
#define GBT_BINS 256
#define GBT_THR (GBT_BINS - 1)
#define GBT_PASS 16                              // (class, node) pairs of one pass of the sweep: 16 x 256 x 12 B = 48 KiB of LDS
#define GBT_LEVEL_NODES 64                       // nodes of the deepest level
#define GBT_STAT_CELLS 4096                      // cells per workgroup of the node sums
#define GBT_MAX_RESIDENT ((size_t)1 << 31)       // the float32 matrix is held whole while it is binned: rows x ld floats
#define GBT_SORT_WORDS ((size_t)1 << 27)         // words of one ping-pong array of the column sort (512 MB): columns go in chunks
#define GBT_MAX_Q ((int64_t)1 << 41)             // |q_r|, q_h of smx_gbt_grow: 2^20 of them stay inside int64
#define GBT_QUANTUM 0x1p40

typedef unsigned long long u64;

struct GbtTrees {   // each [trees][M]
  int32_t* feature; float* threshold; int32_t* left; int32_t* right; double* value; int32_t* n; double* improvement; int32_t* sbin;
};

__device__ __forceinline__ long long wave_scan_add_i64(long long v) {   // inclusive over the lanes; integers: the order is immaterial
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// is p one of floor(j N / 256), j = 1 .. 255 ?
__device__ __forceinline__ bool gbt_quantile_pos(long p, long N) {
  const long j = (p * GBT_BINS + N - 1) / N;
  return j >= 1 && j < GBT_BINS && (j * N) / GBT_BINS == p;
}

// column col0 + blockIdx.x of tile [N][ld]: thr [G][255], nthr [G], bins [G][ldn].  A, B: [gridDim.x][N] words each.
__global__ __launch_bounds__(256) void gbt_bin_kernel(const float* __restrict__ tile, int N, long ld, int col0, long ldn, unsigned* A,
                                                      unsigned* B, float* __restrict__ thr, int32_t* __restrict__ nthr,
                                                      uint8_t* __restrict__ bins) {
  __shared__ SortShared sh;
  __shared__ unsigned heads, wt[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long g = col0 + (long)blockIdx.x;
  const float* col = tile + g;
  auto key = [&](unsigned c) { return order_key(col[(long)c * ld]); };
  const unsigned* S = block_radix_sort(key, N, 4, nullptr, A + (size_t)blockIdx.x * N, B + (size_t)blockIdx.x * N, sh);
  if (tid == 0) heads = 0;
  __syncthreads();
  unsigned mine = 0;
  for (int j = tid; j < N; j += 256) mine += (j > 0 && key(S[j]) != key(S[j - 1])) ? 1u : 0u;
  if (mine) atomicAdd(&heads, mine);
  __syncthreads();
  const bool every = heads + 1u <= (unsigned)GBT_BINS;   // a bin per distinct value
  unsigned carry = 0;
  for (int t0 = 0; t0 < N; t0 += 256) {
    const int j = t0 + tid;
    const bool on = j < N;
    unsigned c = 0;
    float va = 0.f, vb = 0.f;
    bool cut = false;
    if (on) {
      c = S[j];
      if (j > 0) {
        va = col[(long)S[j - 1] * ld] + 0.f;   // (-0 as +0)
        vb = col[(long)c * ld] + 0.f;
        cut = order_key(va) != order_key(vb) && (every || gbt_quantile_pos(j, N));
      }
    }
    const unsigned inc = wave_scan_add(cut ? 1u : 0u);
    if (lane == 63) wt[w] = inc;
    __syncthreads();
    unsigned bin = carry + inc;
    for (int q = 0; q < w; ++q) bin += wt[q];
    carry += (wt[0] + wt[1]) + (wt[2] + wt[3]);
    if (on && bin < (unsigned)GBT_BINS) {   // (always: at most 255 cuts)
      bins[g * ldn + c] = (uint8_t)bin;
      if (cut) {
        const float mid = __fadd_rn(__fmul_rn(va, 0.5f), __fmul_rn(vb, 0.5f));
        thr[g * GBT_THR + (bin - 1)] = mid == vb ? va : mid;
      }
    }
    __syncthreads();
  }
  if (tid == 0) nthr[g] = (int32_t)carry;
}

// tot [K][64][3] += the sums of q_r and q_h and the count of the cells of class blockIdx.y's nodes base .. base + L - 1
__global__ __launch_bounds__(256) void gbt_node_stats_kernel(const uint8_t* __restrict__ node, const int64_t* __restrict__ qr,
                                                             const int64_t* __restrict__ qh, int N, long ldn, int base, int L,
                                                             u64* __restrict__ tot) {
  __shared__ u64 s[GBT_LEVEL_NODES * 3];
  const int k = blockIdx.y;
  for (int t = threadIdx.x; t < GBT_LEVEL_NODES * 3; t += 256) s[t] = 0ull;
  __syncthreads();
  const long i0 = (long)blockIdx.x * GBT_STAT_CELLS, i1 = min((long)N, i0 + GBT_STAT_CELLS);
  for (long i = i0 + threadIdx.x; i < i1; i += 256) {
    const int loc = (int)node[k * ldn + i] - base;
    if (loc < 0 || loc >= L) continue;
    atomicAdd(&s[loc * 3], (u64)qr[(long)k * N + i]);
    atomicAdd(&s[loc * 3 + 1], (u64)qh[(long)k * N + i]);
    atomicAdd(&s[loc * 3 + 2], 1ull);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < L * 3; t += 256)
    if (s[t]) atomicAdd(&tot[(long)k * GBT_LEVEL_NODES * 3 + t], s[t]);
}

__device__ __forceinline__ double gbt_improvement(long long SL, unsigned nL, long long S, unsigned n) {
  const double a = (double)SL, b = (double)(S - SL), c = (double)S;
  return __dsub_rn(__dadd_rn(__ddiv_rn(__dmul_rn(a, a), (double)nL), __ddiv_rn(__dmul_rn(b, b), (double)(n - nL))),
                   __ddiv_rn(__dmul_rn(c, c), (double)n));
}

// feature blockIdx.x, the pairs q = k L + local node of [P blockIdx.y, P blockIdx.y + P): cimp / cbin [K L][G], the feature's best
// candidate of each pair (-inf, -1: none)
__global__ __launch_bounds__(256) void gbt_hist_kernel(const uint8_t* __restrict__ bins, const uint8_t* __restrict__ node,
                                                       const int64_t* __restrict__ qr, const int32_t* __restrict__ nthr,
                                                       const u64* __restrict__ tot, int N, long ldn, int K, int G, int base, int L, int P,
                                                       int msl, double* __restrict__ cimp, int32_t* __restrict__ cbin) {
  __shared__ u64 hs[GBT_PASS * GBT_BINS];
  __shared__ unsigned hc[GBT_PASS * GBT_BINS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long g = blockIdx.x;
  const int q0 = (int)blockIdx.y * P, q1 = min(q0 + P, K * L);   // (P <= GBT_PASS, checked by the host)
  const int klo = q0 / L, khi = (q1 - 1) / L;
  for (int t = tid; t < (q1 - q0) * GBT_BINS; t += 256) { hs[t] = 0ull; hc[t] = 0u; }
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    const int b = bins[g * ldn + i];
    for (int k = klo; k <= khi; ++k) {
      const int loc = (int)node[k * ldn + i] - base;
      if (loc < 0 || loc >= L) continue;
      const int q = k * L + loc;
      if (q < q0 || q >= q1) continue;
      atomicAdd(&hs[(q - q0) * GBT_BINS + b], (u64)qr[(long)k * N + i]);
      atomicAdd(&hc[(q - q0) * GBT_BINS + b], 1u);
    }
  }
  __syncthreads();
  const int nb = nthr[g] + 1;
  for (int q = q0 + w; q < q1; q += 4) {   // (wave-uniform)
    const int k = q / L, loc = q - k * L;
    const u64* tt = tot + ((long)k * GBT_LEVEL_NODES + loc) * 3;
    const long long S = (long long)tt[0];
    const unsigned n = (unsigned)tt[2];
    double best = -INFINITY;
    int bb = -1;
    if (n > 0) {   // (wave-uniform)
      long long s4[4], ls = 0;
      unsigned c4[4], lc = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ls += (long long)hs[(q - q0) * GBT_BINS + 4 * lane + e];
        lc += hc[(q - q0) * GBT_BINS + 4 * lane + e];
        s4[e] = ls; c4[e] = lc;
      }
      const long long xs = wave_scan_add_i64(ls) - ls;
      const unsigned xc = wave_scan_add(lc) - lc;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int b = 4 * lane + e;
        const unsigned nL = xc + c4[e];
        if (b < nb - 1 && nL >= (unsigned)msl && n - nL >= (unsigned)msl) {   // (msl >= 1: neither side is empty)
          const double imp = gbt_improvement(xs + s4[e], nL, S, n);
          if (imp > best) { best = imp; bb = b; }
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double oi = __shfl_xor(best, off, 64);
        const int ob = __shfl_xor(bb, off, 64);
        if (oi > best || (oi == best && ob >= 0 && (bb < 0 || ob < bb))) { best = oi; bb = ob; }
      }
    }
    if (lane == 0) { cimp[(long)q * G + g] = best; cbin[(long)q * G + g] = bb; }
  }
}

// pair blockIdx.x = k L + local node: the node record of tree k's slot base + local node.  final: the level max_depth, leaves only.
__global__ __launch_bounds__(256) void gbt_split_kernel(const double* __restrict__ cimp, const int32_t* __restrict__ cbin, int G, int base,
                                                        int L, int M, int final_level, long mss, long msl, double scale,
                                                        const float* __restrict__ thr, const u64* __restrict__ tot, GbtTrees T) {
  __shared__ double si[4];
  __shared__ int sg[4], sb[4];
  const int q = blockIdx.x, k = q / L, loc = q - k * L, t = base + loc, tid = threadIdx.x;
  const u64* tt = tot + ((long)k * GBT_LEVEL_NODES + loc) * 3;
  const long n = (long)(unsigned)tt[2];
  if (n == 0) return;   // (uniform: no cell reaches the slot)
  double best = -INFINITY;
  int bg = -1, bb = -1;
  if (!final_level && n >= mss && n >= 2 * msl) {   // (uniform)
    for (int g = tid; g < G; g += 256) {
      const double v = cimp[(long)q * G + g];
      if (v > best) { best = v; bg = g; bb = cbin[(long)q * G + g]; }   // (rising g: the lowest feature of equal ones)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double oi = __shfl_xor(best, off, 64);
      const int og = __shfl_xor(bg, off, 64), ob = __shfl_xor(bb, off, 64);
      if (oi > best || (oi == best && og >= 0 && (bg < 0 || og < bg))) { best = oi; bg = og; bb = ob; }
    }
    if ((tid & 63) == 0) { si[tid >> 6] = best; sg[tid >> 6] = bg; sb[tid >> 6] = bb; }
    __syncthreads();
    if (tid == 0)
      for (int w = 1; w < 4; ++w)
        if (si[w] > best || (si[w] == best && sg[w] >= 0 && (bg < 0 || sg[w] < bg))) { best = si[w]; bg = sg[w]; bb = sb[w]; }
  }
  if (tid != 0) return;
  const long o = (long)k * M + t;
  T.n[o] = (int32_t)n;
  if (bg >= 0 && bb >= 0 && best > 0.0) {
    T.feature[o] = bg; T.sbin[o] = bb; T.threshold[o] = thr[(long)bg * GBT_THR + bb];
    T.left[o] = 2 * t + 1; T.right[o] = 2 * t + 2;
    T.improvement[o] = __dmul_rn(best, 0x1p-80);
  } else {
    const long long Sr = (long long)tt[0], Sh = (long long)tt[1];
    T.value[o] = Sh == 0 ? 0.0 : __dmul_rn(scale, __ddiv_rn((double)Sr, (double)Sh));
  }
}

// the cells of the nodes that split go to their children
__global__ __launch_bounds__(256) void gbt_reassign_kernel(const uint8_t* __restrict__ bins, uint8_t* __restrict__ node, int N, long ldn,
                                                           int M, GbtTrees T) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  if (i >= N) return;
  const int nd = node[k * ldn + i];
  if (nd >= M) return;
  const int f = T.feature[(long)k * M + nd];
  if (f < 0 || 2 * nd + 2 >= M) return;
  node[k * ldn + i] = (uint8_t)((int)bins[(long)f * ldn + i] <= T.sbin[(long)k * M + nd] ? 2 * nd + 1 : 2 * nd + 2);
}

__global__ __launch_bounds__(256) void gbt_update_kernel(const uint8_t* __restrict__ node, int N, long ldn, int Kz, int M, GbtTrees T,
                                                         double lr, double* __restrict__ raw) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  if (i >= N) return;
  const int nd = min((int)node[k * ldn + i], M - 1);
  raw[i * Kz + k] = __dadd_rn(raw[i * Kz + k], __dmul_rn(lr, T.value[(long)k * M + nd]));
}

__global__ __launch_bounds__(256) void gbt_fill_kernel(double* __restrict__ raw, long n, int Kz, const double* __restrict__ init) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n * Kz) raw[i] = init[i % Kz];
}

__global__ __launch_bounds__(256) void gbt_tree_init_kernel(GbtTrees T, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { T.feature[i] = -1; T.left[i] = -1; T.right[i] = -1; T.sbin[i] = -1; }
}

// row i of raw [N][Kz]: the probabilities, the quantised statistics (qr != NULL) and the workgroup's sum of the losses
__global__ __launch_bounds__(256) void gbt_stats_kernel(const double* __restrict__ raw, const int32_t* __restrict__ y, int N, int Kz, int binary,
                                                        int64_t* __restrict__ qr, int64_t* __restrict__ qh, double* __restrict__ losspart) {
  __shared__ double s4[4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double loss = 0.0;
  if (i < N) {
    const int yi = y[i];
    if (binary) {
      const double z = raw[i], p = __ddiv_rn(1.0, __dadd_rn(1.0, exp(-z))), hit = yi == 1 ? 1.0 : 0.0;
      loss = __dsub_rn(__dadd_rn(log1p(exp(-fabs(z))), fmax(z, 0.0)), __dmul_rn(hit, z));
      if (qr) {
        qr[i] = llrint(__dmul_rn(__dsub_rn(hit, p), GBT_QUANTUM));
        qh[i] = llrint(__dmul_rn(__dmul_rn(p, __dsub_rn(1.0, p)), GBT_QUANTUM));
      }
    } else {
      const double* z = raw + i * Kz;
      double m = z[0], s = 0.0;
      for (int k = 1; k < Kz; ++k) m = fmax(m, z[k]);
      for (int k = 0; k < Kz; ++k) s = __dadd_rn(s, exp(__dsub_rn(z[k], m)));   // (in class order)
      loss = __dsub_rn(__dadd_rn(m, log(s)), z[yi]);
      if (qr)
        for (int k = 0; k < Kz; ++k) {
          const double p = __ddiv_rn(exp(__dsub_rn(z[k], m)), s), hit = yi == k ? 1.0 : 0.0;
          qr[(long)k * N + i] = llrint(__dmul_rn(__dsub_rn(hit, p), GBT_QUANTUM));
          qh[(long)k * N + i] = llrint(__dmul_rn(__dmul_rn(p, __dsub_rn(1.0, p)), GBT_QUANTUM));
        }
    }
  }
  loss = halving_block_sum(loss, s4);
  if (threadIdx.x == 0) losspart[blockIdx.x] = loss;
}

// ONE workgroup: out[0], out[1] = the sums of the training and the validation losses
__global__ __launch_bounds__(256) void gbt_close_kernel(const double* __restrict__ lt, long nt, const double* __restrict__ lv, long nv,
                                                        double* __restrict__ out) {
  __shared__ double s4[4];
  const double a = halving_column_sum(lt, nt, s4);
  const double b = halving_column_sum(lv, nv, s4);
  if (threadIdx.x == 0) { out[0] = a; out[1] = b; }
}

// rows [0, nb) of the tile, global rows row0 + .: raw [.][Kz] += learning_rate * the leaf values of the stages [s0, s1), stage by stage
__global__ __launch_bounds__(256) void gbt_walk_kernel(const float* __restrict__ tile, long nb, long ld, long row0, GbtTrees T, int M, int s0,
                                                       int s1, int Kz, double lr, double* __restrict__ raw) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nb * Kz) return;
  const long r = idx / Kz;
  const int k = (int)(idx - r * Kz);
  const float* x = tile + r * ld;
  double acc = raw[(row0 + r) * Kz + k];
  for (int s = s0; s < s1; ++s) {
    const long o = ((long)s * Kz + k) * M;
    int nd = 0;
    for (int d = 0; d < GBT_MAX_DEPTH; ++d) {   // (the host checked: features inside the matrix, children inside the tree)
      const int f = T.feature[o + nd];
      if (f < 0) break;
      nd = x[f] <= T.threshold[o + nd] ? T.left[o + nd] : T.right[o + nd];
    }
    acc = __dadd_rn(acc, __dmul_rn(lr, T.value[o + nd]));
  }
  raw[(row0 + r) * Kz + k] = acc;
}

namespace {

struct GbtGrow {   // what the launches of a level share
  int N = 0, G = 0, K = 0, D = 0, M = 0, P = GBT_PASS;
  long ldn = 0, mss = 2, msl = 1;
  double scale = 1.0;
  uint8_t *bins = nullptr, *node = nullptr;
  int32_t *nthr = nullptr, *cbin = nullptr;
  float* thr = nullptr;
  int64_t *qr = nullptr, *qh = nullptr;
  u64* tot = nullptr;
  double* cimp = nullptr;
};

GbtTrees trees_at(const GbtTrees& T, long off) {
  return GbtTrees{T.feature + off, T.threshold + off, T.left + off, T.right + off, T.value + off, T.n + off, T.improvement + off, T.sbin + off};
}

int trees_alloc(DeviceScratch& buf, GbtTrees* T, size_t n) {
  SMX_CHECK(buf.get(&T->feature, n)); SMX_CHECK(buf.get(&T->threshold, n)); SMX_CHECK(buf.get(&T->left, n)); SMX_CHECK(buf.get(&T->right, n));
  SMX_CHECK(buf.get(&T->value, n)); SMX_CHECK(buf.get(&T->n, n)); SMX_CHECK(buf.get(&T->improvement, n)); SMX_CHECK(buf.get(&T->sbin, n));
  hipLaunchKernelGGL(gbt_tree_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, *T, (long)n);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

int trees_download(const GbtTrees& T, size_t n, int32_t* feature, float* threshold, int32_t* left, int32_t* right, double* value, int32_t* nn,
                   double* improvement) {
  SMX_HIP(hipMemcpy(feature, T.feature, n * 4, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(threshold, T.threshold, n * 4, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(left, T.left, n * 4, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(right, T.right, n * 4, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(value, T.value, n * 8, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(nn, T.n, n * 4, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(improvement, T.improvement, n * 8, hipMemcpyDeviceToHost));
  return SMX_OK;
}

int gbt_check_shape(const char* who, int64_t N, int32_t G, int32_t depth, int64_t mss, int64_t msl, int32_t pass_pairs) {
  const std::string w(who);
  SMX_REQUIRE(N >= 1 && N <= GBT_MAX_CELLS, (w + ": 1 <= n_rows <= 2^20").c_str());
  SMX_REQUIRE(G >= 1 && G <= GBT_MAX_GENES, (w + ": 1 <= n_genes <= 32768").c_str());
  SMX_REQUIRE(depth >= 1 && depth <= GBT_MAX_DEPTH, (w + ": 1 <= max_depth <= 6").c_str());
  SMX_REQUIRE(mss >= 2 && msl >= 1, (w + ": min_samples_split >= 2 and min_samples_leaf >= 1").c_str());
  SMX_REQUIRE(pass_pairs >= 0 && pass_pairs <= GBT_PASS, (w + ": pass_pairs is 0 (the library's choice) or 1 .. 16").c_str());
  return SMX_OK;
}

// the buffers of the levels; bins, nthr, thr, qr, qh are the caller's
int gbt_grow_alloc(DeviceScratch& buf, GbtGrow* gw) {
  gw->M = (2 << gw->D) - 1;
  SMX_CHECK(buf.get(&gw->node, (size_t)gw->K * gw->ldn));
  SMX_CHECK(buf.get(&gw->tot, (size_t)gw->K * GBT_LEVEL_NODES * 3));
  const size_t pairs = (size_t)gw->K << (gw->D - 1);   // of the deepest level that is swept
  SMX_CHECK(buf.get(&gw->cimp, pairs * gw->G));
  SMX_CHECK(buf.get(&gw->cbin, pairs * gw->G));
  return SMX_OK;
}

// the K trees of one stage into T [K][M] (initialised), the cells' leaves into gw.node: 4 D + 2 launches, nothing read back
int gbt_grow_stage(const GbtGrow& gw, const GbtTrees& T) {
  const unsigned cells = (unsigned)((gw.N + 255) / 256), chunks = (unsigned)((gw.N + GBT_STAT_CELLS - 1) / GBT_STAT_CELLS);
  SMX_HIP(hipMemsetAsync(gw.node, 0, (size_t)gw.K * gw.ldn, nullptr));
  for (int level = 0; level <= gw.D; ++level) {
    const int base = (1 << level) - 1, L = 1 << level, last = level == gw.D;
    SMX_HIP(hipMemsetAsync(gw.tot, 0, sizeof(u64) * gw.K * GBT_LEVEL_NODES * 3, nullptr));
    hipLaunchKernelGGL(gbt_node_stats_kernel, dim3(chunks, (unsigned)gw.K), dim3(256), 0, nullptr, gw.node, gw.qr, gw.qh, gw.N, gw.ldn, base, L,
                       gw.tot);
    if (!last)
      hipLaunchKernelGGL(gbt_hist_kernel, dim3((unsigned)gw.G, (unsigned)((gw.K * L + gw.P - 1) / gw.P)), dim3(256), 0, nullptr, gw.bins, gw.node,
                         gw.qr, gw.nthr, gw.tot, gw.N, gw.ldn, gw.K, gw.G, base, L, gw.P, (int)std::min<long>(gw.msl, (long)GBT_MAX_CELLS + 1),
                         gw.cimp, gw.cbin);
    hipLaunchKernelGGL(gbt_split_kernel, dim3((unsigned)(gw.K * L)), dim3(256), 0, nullptr, gw.cimp, gw.cbin, gw.G, base, L, gw.M, last, gw.mss,
                       gw.msl, gw.scale, gw.thr, gw.tot, T);
    if (!last)
      hipLaunchKernelGGL(gbt_reassign_kernel, dim3(cells, (unsigned)gw.K), dim3(256), 0, nullptr, gw.bins, gw.node, gw.N, gw.ldn, gw.M, T);
    SMX_HIP(hipGetLastError());
  }
  return SMX_OK;
}

struct GbtMatrix { PrepInput in; PrepStage st; };

// the shared matrix arguments; every entry must be finite
int gbt_check_matrix(const char* who, const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows,
                     int32_t n_genes, int32_t block_rows, GbtMatrix* mx) {
  const std::string w(who);
  SMX_REQUIRE(n_rows >= 1 && n_rows <= GBT_MAX_CELLS, (w + ": 1 <= n_rows <= 2^20").c_str());
  SMX_REQUIRE(n_genes >= 1 && n_genes <= GBT_MAX_GENES, (w + ": 1 <= n_genes <= 32768").c_str());
  SMX_CHECK(prep_check_input(who, x, indptr, cols, vals, n_rows, n_genes, block_rows, 0, nullptr, &mx->in));
  const long N = mx->in.N;
  const size_t n_val = x ? (size_t)N * (size_t)n_genes : (size_t)(indptr[N] - indptr[0]);
  const float* v = x ? x : vals + indptr[0];
  for (size_t i = 0; i < n_val; ++i) SMX_REQUIRE(std::isfinite(v[i]), (w + ": a matrix value that is not finite").c_str());
  return SMX_OK;
}

// the whole matrix in one tile
int gbt_resident(const char* who, DeviceScratch& buf, GbtMatrix* mx) {
  PrepInput& in = mx->in;
  in.block = (in.N + SMX_PREP_SLICE - 1) / SMX_PREP_SLICE * SMX_PREP_SLICE;
  SMX_REQUIRE((size_t)in.block * (size_t)in.ld <= GBT_MAX_RESIDENT,
              (std::string(who) + ": rows x n_genes <= 2^31 (the matrix is held whole)").c_str());
  if (!in.x) in.max_nnz = (size_t)(in.csr.indptr[in.N] - in.csr.indptr[0]);
  SMX_CHECK(prep_stage_alloc(buf, in, &mx->st, true));
  SMX_CHECK(prep_load_block(in, mx->st, 0, in.N));
  return SMX_OK;
}

// tile [N][ld] -> thr [G][255], nthr [G], bins [G][ldn] (all zeroed by their allocation), the columns in chunks
int gbt_bin_device(const float* tile, long N, int G, long ld, long ldn, float* thr, int32_t* nthr, uint8_t* bins) {
  const long per = std::max<long>(1, std::min<long>((long)G, (long)(GBT_SORT_WORDS / (size_t)N)));
  DeviceScratch sortbuf;
  unsigned *A, *B;
  SMX_CHECK(sortbuf.get(&A, (size_t)per * N));
  SMX_CHECK(sortbuf.get(&B, (size_t)per * N));
  for (long c0 = 0; c0 < G; c0 += per) {
    const long nc = std::min(per, (long)G - c0);
    hipLaunchKernelGGL(gbt_bin_kernel, dim3((unsigned)nc), dim3(256), 0, nullptr, tile, (int)N, ld, (int)c0, ldn, A, B, thr, nthr, bins);
    SMX_HIP(hipGetLastError());
  }
  SMX_HIP(hipDeviceSynchronize());   // (the sort's arrays are freed on the way out)
  return SMX_OK;
}

long gbt_ldn(long N) { return (N + 63) & ~63L; }

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_gbt_bin(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                float* thresholds, int32_t* n_thresholds, uint8_t* bins) {
  GbtMatrix mx;
  SMX_CHECK(gbt_check_matrix("gbt_bin", x, indptr, cols, vals, n_rows, n_genes, 0, &mx));
  SMX_REQUIRE(thresholds && n_thresholds && bins, "gbt_bin: null output");
  const long N = mx.in.N, ldn = gbt_ldn(N);
  const int G = mx.in.G;
  DeviceScratch buf;
  SMX_CHECK(gbt_resident("gbt_bin", buf, &mx));
  float* dThr; int32_t* dN; uint8_t* dBins;
  SMX_CHECK(buf.get(&dThr, (size_t)G * GBT_THR));
  SMX_CHECK(buf.get(&dN, (size_t)G));
  SMX_CHECK(buf.get(&dBins, (size_t)G * ldn));
  SMX_CHECK(gbt_bin_device(mx.st.tile, N, G, mx.in.ld, ldn, dThr, dN, dBins));
  SMX_HIP(hipMemcpy(thresholds, dThr, (size_t)G * GBT_THR * 4, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(n_thresholds, dN, (size_t)G * 4, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy2D(bins, (size_t)N, dBins, (size_t)ldn, (size_t)N, (size_t)G, hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_gbt_grow(const uint8_t* bins, const int32_t* n_thresholds, const float* thresholds, const int64_t* q_r, const int64_t* q_h,
                 int64_t n_rows, int32_t n_genes, int32_t n_trees, int32_t max_depth, int64_t min_samples_split, int64_t min_samples_leaf,
                 double scale, int32_t pass_pairs, int32_t* feature, float* threshold, int32_t* left, int32_t* right, double* value,
                 int32_t* n, double* improvement, int32_t* leaf) {
  SMX_CHECK(gbt_check_shape("gbt_grow", n_rows, n_genes, max_depth, min_samples_split, min_samples_leaf, pass_pairs));
  SMX_REQUIRE(n_trees >= 1 && n_trees <= GBT_MAX_CLASSES, "gbt_grow: 1 <= n_trees <= 32");
  SMX_REQUIRE(bins && n_thresholds && thresholds && q_r && q_h, "gbt_grow: null input");
  SMX_REQUIRE(feature && threshold && left && right && value && n && improvement && leaf, "gbt_grow: null output");
  SMX_REQUIRE(std::isfinite(scale), "gbt_grow: scale must be finite");
  const long N = (long)n_rows, ldn = gbt_ldn(N);
  const int G = n_genes, K = n_trees;
  for (int g = 0; g < G; ++g) {
    SMX_REQUIRE(n_thresholds[g] >= 0 && n_thresholds[g] <= GBT_THR, "gbt_grow: a threshold count outside 0 .. 255");
    for (long i = 0; i < N; ++i) SMX_REQUIRE((int)bins[(size_t)g * N + i] <= n_thresholds[g], "gbt_grow: a bin beyond its column's thresholds");
  }
  for (size_t i = 0; i < (size_t)K * N; ++i)
    SMX_REQUIRE(q_r[i] >= -GBT_MAX_Q && q_r[i] <= GBT_MAX_Q && q_h[i] >= 0 && q_h[i] <= GBT_MAX_Q, "gbt_grow: |q_r| <= 2^41 and 0 <= q_h <= 2^41");
  DeviceScratch buf;
  GbtGrow gw;
  gw.N = (int)N; gw.G = G; gw.K = K; gw.D = max_depth; gw.ldn = ldn; gw.mss = (long)min_samples_split; gw.msl = (long)min_samples_leaf;
  gw.scale = scale; gw.P = pass_pairs ? pass_pairs : GBT_PASS;
  SMX_CHECK(buf.get(&gw.bins, (size_t)G * ldn));
  SMX_HIP(hipMemcpy2D(gw.bins, (size_t)ldn, bins, (size_t)N, (size_t)N, (size_t)G, hipMemcpyHostToDevice));
  SMX_CHECK(buf.put(&gw.nthr, n_thresholds, (size_t)G));
  SMX_CHECK(buf.put(&gw.thr, thresholds, (size_t)G * GBT_THR));
  SMX_CHECK(buf.put(&gw.qr, q_r, (size_t)K * N));
  SMX_CHECK(buf.put(&gw.qh, q_h, (size_t)K * N));
  SMX_CHECK(gbt_grow_alloc(buf, &gw));
  GbtTrees T;
  const size_t nt = (size_t)K * gw.M;
  SMX_CHECK(trees_alloc(buf, &T, nt));
  SMX_CHECK(gbt_grow_stage(gw, T));
  SMX_HIP(hipDeviceSynchronize());
  SMX_CHECK(trees_download(T, nt, feature, threshold, left, right, value, n, improvement));
  std::vector<uint8_t> hn((size_t)K * ldn);
  SMX_HIP(hipMemcpy(hn.data(), gw.node, hn.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < K; ++k)
    for (long i = 0; i < N; ++i) leaf[(size_t)k * N + i] = hn[(size_t)k * ldn + i];
  return SMX_OK;
}

int smx_gbt_fit(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                const int32_t* labels, int32_t n_classes, const float* xv, const int64_t* v_indptr, const int32_t* v_cols, const float* v_vals,
                int64_t n_val, const int32_t* labels_val, int32_t n_estimators, double learning_rate, int32_t max_depth,
                int64_t min_samples_split, int64_t min_samples_leaf, int32_t n_iter_no_change, double tol, int32_t pass_pairs,
                const double* init, int32_t* feature, float* threshold, int32_t* left, int32_t* right, double* value, int32_t* n,
                double* improvement, int32_t* n_estimators_out, double* train_score, double* val_score) {
  GbtMatrix mx, mv;
  SMX_CHECK(gbt_check_matrix("gbt_fit", x, indptr, cols, vals, n_rows, n_genes, 0, &mx));
  SMX_CHECK(gbt_check_shape("gbt_fit", n_rows, n_genes, max_depth, min_samples_split, min_samples_leaf, pass_pairs));
  SMX_REQUIRE(n_classes >= 2 && n_classes <= GBT_MAX_CLASSES, "gbt_fit: 2 <= n_classes <= 32");
  SMX_REQUIRE(n_estimators >= 1, "gbt_fit: n_estimators >= 1");
  SMX_REQUIRE(std::isfinite(learning_rate) && learning_rate > 0.0, "gbt_fit: learning_rate must be finite and > 0");
  SMX_REQUIRE(labels && init, "gbt_fit: null labels or init");
  SMX_REQUIRE(feature && threshold && left && right && value && n && improvement && n_estimators_out && train_score, "gbt_fit: null output");
  const bool early = n_iter_no_change > 0;
  const long N = mx.in.N, ldn = gbt_ldn(N);
  const int G = mx.in.G, K = n_classes, binary = K == 2, Kz = binary ? 1 : K;
  {
    std::vector<long> count((size_t)K, 0);
    for (long i = 0; i < N; ++i) {
      SMX_REQUIRE(labels[i] >= 0 && labels[i] < K, "gbt_fit: a label outside 0 .. n_classes - 1");
      ++count[(size_t)labels[i]];
    }
    for (int k = 0; k < K; ++k) SMX_REQUIRE(count[(size_t)k] > 0, "gbt_fit: a class without a row");
  }
  for (int k = 0; k < Kz; ++k) SMX_REQUIRE(std::isfinite(init[k]), "gbt_fit: an initial score that is not finite");
  long Nv = 0;
  if (early) {
    SMX_REQUIRE(std::isfinite(tol), "gbt_fit: tol must be finite");
    SMX_REQUIRE(labels_val && val_score, "gbt_fit: early stopping takes the validation rows, their labels and val_score");
    SMX_CHECK(gbt_check_matrix("gbt_fit (validation rows)", xv, v_indptr, v_cols, v_vals, n_val, n_genes, 0, &mv));
    Nv = mv.in.N;
    for (long i = 0; i < Nv; ++i) SMX_REQUIRE(labels_val[i] >= 0 && labels_val[i] < K, "gbt_fit: a validation label outside 0 .. n_classes - 1");
  }
  DeviceScratch buf;
  GbtGrow gw;
  gw.N = (int)N; gw.G = G; gw.K = Kz; gw.D = max_depth; gw.ldn = ldn; gw.mss = (long)min_samples_split; gw.msl = (long)min_samples_leaf;
  gw.scale = binary ? 1.0 : (double)(K - 1) / (double)K; gw.P = pass_pairs ? pass_pairs : GBT_PASS;
  SMX_CHECK(buf.get(&gw.thr, (size_t)G * GBT_THR));
  SMX_CHECK(buf.get(&gw.nthr, (size_t)G));
  SMX_CHECK(buf.get(&gw.bins, (size_t)G * ldn));
  {
    DeviceScratch whole;   // the float32 matrix is needed for the bins alone
    SMX_CHECK(gbt_resident("gbt_fit", whole, &mx));
    SMX_CHECK(gbt_bin_device(mx.st.tile, N, G, mx.in.ld, ldn, gw.thr, gw.nthr, gw.bins));
  }
  if (early) SMX_CHECK(gbt_resident("gbt_fit (validation rows)", buf, &mv));
  SMX_CHECK(buf.get(&gw.qr, (size_t)Kz * N));
  SMX_CHECK(buf.get(&gw.qh, (size_t)Kz * N));
  SMX_CHECK(gbt_grow_alloc(buf, &gw));
  const int M = gw.M;
  const size_t nt = (size_t)n_estimators * Kz * M;
  GbtTrees T;
  SMX_CHECK(trees_alloc(buf, &T, nt));
  int32_t *dY, *dYv = nullptr;
  double *dInit, *dRaw, *dRawV = nullptr, *dLoss, *dLossV = nullptr, *dOut;
  const unsigned rows_grid = (unsigned)((N + 255) / 256), val_grid = (unsigned)((Nv + 255) / 256);
  SMX_CHECK(buf.put(&dY, labels, (size_t)N));
  SMX_CHECK(buf.put(&dInit, init, (size_t)Kz));
  SMX_CHECK(buf.get(&dRaw, (size_t)N * Kz));
  SMX_CHECK(buf.get(&dLoss, (size_t)rows_grid));
  SMX_CHECK(buf.get(&dOut, (size_t)2));
  hipLaunchKernelGGL(gbt_fill_kernel, dim3((unsigned)((N * Kz + 255) / 256)), dim3(256), 0, nullptr, dRaw, N, Kz, dInit);
  if (early) {
    SMX_CHECK(buf.put(&dYv, labels_val, (size_t)Nv));
    SMX_CHECK(buf.get(&dRawV, (size_t)Nv * Kz));
    SMX_CHECK(buf.get(&dLossV, (size_t)val_grid));
    hipLaunchKernelGGL(gbt_fill_kernel, dim3((unsigned)((Nv * Kz + 255) / 256)), dim3(256), 0, nullptr, dRawV, Nv, Kz, dInit);
  }
  hipLaunchKernelGGL(gbt_stats_kernel, dim3(rows_grid), dim3(256), 0, nullptr, dRaw, dY, (int)N, Kz, binary, gw.qr, gw.qh, dLoss);
  SMX_HIP(hipGetLastError());
  const double factor = binary ? 2.0 : 1.0;
  std::vector<double> history((size_t)std::max(1, n_iter_no_change), INFINITY);
  int done = 0;
  for (int i = 0; i < n_estimators; ++i) {
    const GbtTrees Ti = trees_at(T, (long)i * Kz * M);
    SMX_CHECK(gbt_grow_stage(gw, Ti));
    hipLaunchKernelGGL(gbt_update_kernel, dim3(rows_grid, (unsigned)Kz), dim3(256), 0, nullptr, gw.node, (int)N, ldn, Kz, M, Ti, learning_rate, dRaw);
    hipLaunchKernelGGL(gbt_stats_kernel, dim3(rows_grid), dim3(256), 0, nullptr, dRaw, dY, (int)N, Kz, binary, gw.qr, gw.qh, dLoss);
    if (early) {
      hipLaunchKernelGGL(gbt_walk_kernel, dim3((unsigned)((Nv * Kz + 255) / 256)), dim3(256), 0, nullptr, mv.st.tile, Nv, mv.in.ld, 0L, T, M, i,
                         i + 1, Kz, learning_rate, dRawV);
      hipLaunchKernelGGL(gbt_stats_kernel, dim3(val_grid), dim3(256), 0, nullptr, dRawV, dYv, (int)Nv, Kz, binary, (int64_t*)nullptr,
                         (int64_t*)nullptr, dLossV);
    }
    hipLaunchKernelGGL(gbt_close_kernel, dim3(1), dim3(256), 0, nullptr, dLoss, (long)rows_grid, dLossV, early ? (long)val_grid : 0L, dOut);
    SMX_HIP(hipGetLastError());
    double out[2];
    SMX_HIP(hipMemcpy(out, dOut, sizeof(out), hipMemcpyDeviceToHost));
    train_score[i] = factor * (out[0] / (double)N);
    done = i + 1;
    if (!std::isfinite(train_score[i])) { set_error("gbt_fit: the training loss is not finite"); return SMX_ERR_NAN; }
    if (early) {
      const double vl = factor * (out[1] / (double)Nv);
      val_score[i] = vl;
      bool better = false;   // scikit-learn's rule: better than ANY of the last n_iter_no_change losses by tol
      for (double h : history) better = better || vl + tol < h;
      if (!better) break;
      history[(size_t)i % history.size()] = vl;
    }
  }
  SMX_HIP(hipDeviceSynchronize());
  SMX_CHECK(trees_download(T, nt, feature, threshold, left, right, value, n, improvement));
  *n_estimators_out = done;
  return SMX_OK;
}

int smx_gbt_decision(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                     int32_t block_rows, int32_t n_stages, int32_t n_outputs, int32_t max_depth, const int32_t* feature, const float* threshold,
                     const int32_t* left, const int32_t* right, const double* value, const double* init, double learning_rate, double* raw) {
  GbtMatrix mx;
  SMX_CHECK(gbt_check_matrix("gbt_decision", x, indptr, cols, vals, n_rows, n_genes, block_rows, &mx));
  SMX_REQUIRE(max_depth >= 1 && max_depth <= GBT_MAX_DEPTH, "gbt_decision: 1 <= max_depth <= 6");
  SMX_REQUIRE(n_stages >= 0 && n_outputs >= 1 && n_outputs <= GBT_MAX_CLASSES, "gbt_decision: n_stages >= 0 and 1 <= n_outputs <= 32");
  SMX_REQUIRE(feature && threshold && left && right && value && init && raw, "gbt_decision: null trees, init or output");
  SMX_REQUIRE(std::isfinite(learning_rate), "gbt_decision: learning_rate must be finite");
  const PrepInput& in = mx.in;
  const long N = in.N;
  const int Kz = n_outputs, M = (2 << max_depth) - 1, G = in.G;
  const size_t nt = (size_t)n_stages * Kz * M;
  for (size_t t = 0; t < nt; ++t) {   // a walk stays inside the matrix and the tree, and goes down
    const int nd = (int)(t % (size_t)M);
    SMX_REQUIRE(feature[t] >= -1 && feature[t] < G, "gbt_decision: a feature outside -1 .. n_genes - 1");
    if (feature[t] >= 0)
      SMX_REQUIRE(left[t] > nd && left[t] < M && right[t] > nd && right[t] < M, "gbt_decision: a child outside its tree");
  }
  DeviceScratch buf;
  SMX_CHECK(prep_stage_alloc(buf, in, &mx.st, true));
  GbtTrees T{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  SMX_CHECK(buf.put(&T.feature, feature, std::max<size_t>(nt, 1)));
  SMX_CHECK(buf.put(&T.threshold, threshold, std::max<size_t>(nt, 1)));
  SMX_CHECK(buf.put(&T.left, left, std::max<size_t>(nt, 1)));
  SMX_CHECK(buf.put(&T.right, right, std::max<size_t>(nt, 1)));
  SMX_CHECK(buf.put(&T.value, value, std::max<size_t>(nt, 1)));
  double *dInit, *dRaw;
  SMX_CHECK(buf.put(&dInit, init, (size_t)Kz));
  SMX_CHECK(buf.get(&dRaw, (size_t)N * Kz));
  hipLaunchKernelGGL(gbt_fill_kernel, dim3((unsigned)((N * Kz + 255) / 256)), dim3(256), 0, nullptr, dRaw, N, Kz, dInit);
  for (long r0 = 0; r0 < N && n_stages > 0; r0 += in.block) {
    const long nb = std::min(in.block, N - r0);
    SMX_CHECK(prep_load_block(in, mx.st, r0, nb));
    hipLaunchKernelGGL(gbt_walk_kernel, dim3((unsigned)((nb * Kz + 255) / 256)), dim3(256), 0, nullptr, mx.st.tile, nb, in.ld, r0, T, M, 0, n_stages,
                       Kz, learning_rate, dRaw);
    SMX_HIP(hipGetLastError());
    SMX_HIP(hipDeviceSynchronize());   // the next block's copy overwrites the tile
  }
  SMX_HIP(hipMemcpy(raw, dRaw, (size_t)N * Kz * 8, hipMemcpyDeviceToHost));
  return SMX_OK;
}

}  // extern "C"
