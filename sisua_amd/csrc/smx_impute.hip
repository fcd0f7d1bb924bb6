// smx_impute.hip -- the imputation scores of predict()'s gene output (sisua/analysis/imputation_benchmarks.py:102-127), reduced where the
// mean over the draws already is: per cell the median of d[g] = |original[g] - mean[g]| and the flag sum(original) != sum(corrupted);
// over all N x G entries the two middle order statistics of d.  Every selection is EXACT: a non-negative float32 (and a NaN with a clear
// sign bit, which sorts above +inf) orders as its uint32 pattern, so an order statistic is found digit by digit from integer histograms --
// no float atomics, no sort, and no dependence on the order in which the entries are counted.
//   row kernel     one workgroup per cell.  A pass over the row computes d (kept for the global selection), the two row sums and the
//                  row's share of the global level-1 histogram (11 bits, in LDS, flushed with 64-bit integer atomics).  Then four 8-bit
//                  radix passes (256 LDS bins each, the bins scanned by one wave) find the order statistic (G - 1) / 2; the next one
//                  (even G) is the same value when enough entries tie with it, else the smallest larger pattern (one more pass).  The
//                  passes re-read the row from global memory (8 KB at 1998 genes, 80 KB at 20 000: cache-resident), so every G the
//                  model takes has the same form and the LDS use is 10 KB whatever G is.
//   level kernel   levels 2 and 3 of the global selection (10 bits each) for the two ranks' prefixes at once, over d.
//   column gather  [rows][n_sel] of the mean over the draws (smx_predict_stat_cols).
// THE ROW SUMS are accumulated in float64 in a fixed order (smx_block.h's block sum).  The reference compares float32 np.sum(row) of the two rows: for integer
// counts with row sums below 2^24 (every count matrix this project reads) every partial sum of either form is an exact integer, so the
// two comparisons agree.  Every loop is bounded by G or by the element count; nothing waits on device memory.
#include "smx_model.h"
#include "smx_block.h"   // the wave scan and the fixed-order block sum

namespace smx {

struct SelShared { unsigned hist[256]; unsigned prefix, rank, eq, below, minv; };

// order statistic k (0-based) of the G patterns key(0) .. key(G - 1) by the whole 256-thread workgroup -> its pattern; cnt_le = how many
// patterns are <= it.  Block-uniform control flow; the caller's LDS may be reused after the call returns.
template <class Key>
__device__ inline unsigned block_select(const Key& key, int G, unsigned k, SelShared& sh, unsigned& cnt_le) {
  const int tid = threadIdx.x;
  unsigned prefix = 0, mask = 0, rank = k, below = 0, eq = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    sh.hist[tid] = 0;
    __syncthreads();
    for (int g = tid; g < G; g += 256) {
      const unsigned v = key(g);
      if ((v & mask) == prefix) atomicAdd(&sh.hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {   // wave 0: four bins per lane, an inclusive scan across the lanes; exactly one lane holds the rank
      const unsigned c0 = sh.hist[4 * tid], c1 = sh.hist[4 * tid + 1], c2 = sh.hist[4 * tid + 2], c3 = sh.hist[4 * tid + 3];
      const unsigned s = c0 + c1 + c2 + c3;
      const unsigned inc = wave_scan_add(s);
      const unsigned exc = inc - s;
      if (rank >= exc && rank < inc) {
        unsigned r = rank - exc, b = 4u * tid, c = c0, bl = exc;
        if (r >= c) { r -= c; bl += c; ++b; c = c1; }
        if (b == 4u * tid + 1 && r >= c) { r -= c; bl += c; ++b; c = c2; }
        if (b == 4u * tid + 2 && r >= c) { r -= c; bl += c; ++b; c = c3; }
        sh.prefix = prefix | (b << shift); sh.rank = r; sh.eq = c; sh.below = below + bl;
      }
    }
    __syncthreads();
    prefix = sh.prefix; rank = sh.rank; eq = sh.eq; below = sh.below;
    mask |= 255u << shift;
  }
  cnt_le = below + eq;
  return prefix;
}

// the two middle order statistics (G - 1) / 2 and G / 2 of the row's patterns
template <class Key>
__device__ inline void block_middle(const Key& key, int G, SelShared& sh, unsigned& lo, unsigned& hi) {
  const unsigned k1 = (unsigned)(G - 1) / 2u, k2 = (unsigned)G / 2u;
  unsigned cnt_le;
  lo = block_select(key, G, k1, sh, cnt_le);
  hi = lo;
  if (k2 != k1 && cnt_le <= k2) {   // (block-uniform) fewer than k2 + 1 patterns are <= lo: the next one up is the smallest larger pattern
    unsigned mn = 0xFFFFFFFFu;
    for (int g = threadIdx.x; g < G; g += 256) {
      const unsigned v = key(g);
      if (v > lo && v < mn) mn = v;
    }
    if (threadIdx.x == 0) sh.minv = 0xFFFFFFFFu;
    __syncthreads();
    atomicMin(&sh.minv, mn);
    __syncthreads();
    hi = sh.minv;
  }
}

struct DiffKey {   // pattern of |original - mean| (fabsf clears the sign bit: no -0, a NaN sorts above +inf)
  const float* o; const float* mu;
  __device__ unsigned operator()(int g) const { return __float_as_uint(fabsf(o[g] - mu[g])); }
};
struct PlainKey {   // pattern of a non-negative (or NaN) value, -0 as +0.  (The raw pattern, not smx_block.h's order_key: a NaN with the
                    // sign bit set stays above +inf here and would fall below every number there.)
  const float* r;
  __device__ unsigned operator()(int g) const { const unsigned v = __float_as_uint(r[g]); return v == 0x80000000u ? 0u : v; }
};

__global__ __launch_bounds__(256) void impute_row_kernel(ImputeRowArgs a) {
  __shared__ SelShared sh;
  __shared__ unsigned h1[SMX_IMP_L1_BINS];
  __shared__ double sd[4];
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const float* o = a.orig + row * a.ldo;
  const float* mu = a.mean + row * a.ldm;
  const float* c = a.cor + row * a.ldc;
  float* d = a.d ? a.d + row * (long)a.G : nullptr;
  if (a.d_only) {   // (block-uniform)
    for (int g = tid; g < a.G; g += 256) d[g] = fabsf(o[g] - mu[g]);
    return;
  }
  for (int i = tid; i < SMX_IMP_L1_BINS; i += 256) h1[i] = 0;
  __syncthreads();
  double so = 0.0, sc = 0.0;
  int nan = 0;
  for (int g = tid; g < a.G; g += 256) {
    const float og = o[g], dv = fabsf(og - mu[g]);
    const unsigned v = __float_as_uint(dv);
    if (d) d[g] = dv;
    atomicAdd(&h1[v >> 20], 1u);
    nan |= v > 0x7F800000u;
    so += (double)og; sc += (double)c[g];
  }
  so = halving_block_sum(so, sd);
  sc = halving_block_sum(sc, sd);
  nan = __syncthreads_or(nan);
  for (int i = tid; i < SMX_IMP_L1_BINS; i += 256)
    if (h1[i]) atomicAdd(&a.hist[i], (unsigned long long)h1[i]);
  unsigned lo, hi;
  block_middle(DiffKey{o, mu}, a.G, sh, lo, hi);
  if (tid == 0) {
    a.median[row] = nan ? __uint_as_float(0x7FC00000u) : 0.5f * (__uint_as_float(lo) + __uint_as_float(hi));
    a.changed[row] = so != sc ? 1 : 0;
    if (nan) atomicOr(&a.hist[SMX_IMP_L1_BINS + 2 * SMX_IMP_LN_BINS], 1ull);
  }
}

__global__ __launch_bounds__(256) void row_select_kernel(const float* rows, int G, long ld, float* lo_out, float* hi_out) {
  __shared__ SelShared sh;
  unsigned lo, hi;
  block_middle(PlainKey{rows + (long)blockIdx.x * ld}, G, sh, lo, hi);
  if (threadIdx.x == 0) { lo_out[blockIdx.x] = __uint_as_float(lo); hi_out[blockIdx.x] = __uint_as_float(hi); }
}

struct LevelArgs { const float* d; long n; unsigned prefix0, prefix1, mask; int shift; unsigned long long* hist; };
// (a workgroup's LDS counts are 32-bit: it sees at most n / gridDim.x + 256 entries, and n entries of 4 bytes are resident in device memory)
__global__ __launch_bounds__(256) void impute_level_kernel(LevelArgs a) {
  __shared__ unsigned h[2 * SMX_IMP_LN_BINS];
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * SMX_IMP_LN_BINS; i += 256) h[i] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + tid; i < a.n; i += (long)gridDim.x * 256) {
    const unsigned v = __float_as_uint(a.d[i]), b = (v >> a.shift) & (SMX_IMP_LN_BINS - 1);
    if ((v & a.mask) == a.prefix0) atomicAdd(&h[b], 1u);
    if ((v & a.mask) == a.prefix1) atomicAdd(&h[SMX_IMP_LN_BINS + b], 1u);
  }
  __syncthreads();
  for (int i = tid; i < 2 * SMX_IMP_LN_BINS; i += 256)
    if (h[i]) atomicAdd(&a.hist[i], (unsigned long long)h[i]);
}

__global__ __launch_bounds__(256) void gather_cols_kernel(const float* src, long ld, long rows, const int32_t* idx, int n_sel, float* dst) {
  const long total = rows * n_sel;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / n_sel;
    dst[i] = src[r * ld + idx[i - r * n_sel]];
  }
}

int launch_impute_rows(hipStream_t st, const ImputeRowArgs& a, int rows) {
  SMX_REQUIRE(a.mean && a.orig && a.cor && a.G > 0 && rows > 0 && (a.d_only ? a.d != nullptr : (a.median && a.changed && a.hist)), "impute_rows: bad arguments");
  hipLaunchKernelGGL(impute_row_kernel, dim3((unsigned)rows), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

int launch_impute_level(hipStream_t st, const float* d, long n, const unsigned* prefix, unsigned mask, int shift, unsigned long long* hist) {
  SMX_REQUIRE(d && n > 0 && hist && (shift == 10 || shift == 0), "impute_level: bad arguments");
  const LevelArgs a{d, n, prefix[0], prefix[1], mask, shift, hist};
  hipLaunchKernelGGL(impute_level_kernel, dim3((unsigned)std::min<long>(2048, (n + 4095) / 4096)), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

int launch_gather_cols(hipStream_t st, const float* src, long ld, long rows, const int32_t* idx, int n_sel, float* dst) {
  SMX_REQUIRE(src && idx && dst && rows > 0 && n_sel > 0, "gather_cols: bad arguments");
  hipLaunchKernelGGL(gather_cols_kernel, dim3((unsigned)std::min<long>(1024, (rows * n_sel + 255) / 256)), dim3(256), 0, st, src, ld, rows, idx, n_sel, dst);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

}  // namespace smx

extern "C" {

int smx_k_row_select(const float* rows, int32_t n_rows, int32_t G, int32_t ld, float* lo, float* hi) {
  SMX_REQUIRE(rows && lo && hi && n_rows > 0 && G > 0 && ld >= G, "bad arguments");
  const size_t n = (size_t)n_rows * (size_t)ld;
  DeviceScratch buf;
  float *dR, *dLo;
  SMX_CHECK(buf.get(&dR, n));
  SMX_CHECK(buf.get(&dLo, 2 * (size_t)n_rows));
  if (hipMemcpy(dR, rows, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { set_error("smx_k_row_select: copy of the rows failed"); return SMX_ERR_HIP; }
  hipLaunchKernelGGL(row_select_kernel, dim3((unsigned)n_rows), dim3(256), 0, nullptr, dR, (int)G, (long)ld, dLo, dLo + n_rows);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(lo, dLo, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hi, dLo + n_rows, (size_t)n_rows * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("smx_k_row_select: the kernel or the copy of its result failed"); return SMX_ERR_HIP;
  }
  return SMX_OK;
}

}  // extern "C"
