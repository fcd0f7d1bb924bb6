// smx_correlate.hip -- gene x protein correlation matrices (SingleCellOMIC.get_correlation, _single_cell_analysis.py:1199-1245: one pearsonr
// and one spearmanr per pair) of predict()'s gene output, reduced where the mean over the draws already is.  Three kernels:
//   transposing keep   after the walk's chunk, the selected columns of the mean [rows][G] are written gene-major into cols [Gc][N] through a
//                      32 x 32 LDS tile (reads coalesced along the genes, writes along the cells): a gene's N values are contiguous and do
//                      not depend on the batch size or the chunking.
//   column ranks       one workgroup per gene: rank2[i] = 2 x (average rank of cell i), an int32 in 2 .. 2N.  The float32 pattern maps to an
//                      order-preserving unsigned key (-0 as +0); the cell indices go through smx_block.h's stable radix sort, four 8-bit
//                      passes (the key is looked up from the column), then through its tie-run pass: every position gets its run's start,
//                      the run's end is stored at the start, and rank2 = start + end + 2.  One form for every N <= 2^20.
//   column sums        one workgroup per gene reads the column and its ranks and, for every protein, accumulates
//                      Spearman: Sa = sum a, Saa = sum a a, Sab[p] = sum a b_p in 64-bit integers (a, b_p doubled average ranks: 4 N^3 < 2^63
//                      at N = 2^20), exact in any order;
//                      Pearson: the mean, then Sxx = sum (x - mean)^2 and Sxy[p] = sum (x - mean) yhat_p in float64 FMAs -- per-thread strided
//                      partials, then smx_block.h's fixed-order block sum: an order that is a function of N alone.
//                      The proteins pass through registers four at a time, so any P works.
// No float atomics; every loop is bounded by N or P.  The ranks are a pure function of the column, the integer sums of the ranks, and the
// float64 sums of the column and N: nothing depends on the batch size, the chunking of the walk or the gene chunk.
#include "smx_model.h"
#include "smx_block.h"   // the radix sort, the tie-run pass, the keys and the fixed-order sums

namespace smx {

__global__ __launch_bounds__(256) void keep_cols_kernel(const float* src, long ld, int rows, const int32_t* idx, int n_sel, float* dst, long N,
                                                        long c0) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int j0 = (int)blockIdx.x * 32, r0 = (int)blockIdx.y * 32;
  const int col = j0 + tx < n_sel ? idx[j0 + tx] : -1;
  for (int k = ty; k < 32; k += 8)
    if (col >= 0 && r0 + k < rows) tile[k][tx] = src[(long)(r0 + k) * ld + col];
  __syncthreads();
  for (int k = ty; k < 32; k += 8)
    if (j0 + k < n_sel && r0 + tx < rows) dst[(long)(j0 + k) * N + c0 + r0 + tx] = tile[tx][k];
}

__global__ __launch_bounds__(256) void col_rank2_kernel(const float* cols, int N, unsigned* sortA, unsigned* sortB, int32_t* rank2,
                                                        int32_t* nonfinite) {
  __shared__ SortShared sh;
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * N;
  const float* x = cols + base;
  unsigned* A = sortA + base;
  int32_t* rk = rank2 + base;
  int bad = 0;
  for (int i = tid; i < N; i += 256) bad |= is_nonfinite(x[i]);
  const auto key = [x](unsigned i) { return order_key(x[i]); };
  const unsigned* S = block_radix_sort(key, N, 4, nullptr, A, sortB + base, sh);   // (four passes: the result is in B)
  block_tie_runs(key, [rk](int, unsigned ci, unsigned start) { rk[ci] = (int32_t)start; }, N, S, A, sh);
  for (int j = tid; j < N; j += 256) {
    const unsigned ci = S[j], s = (unsigned)rk[ci];
    rk[ci] = (int32_t)(s + A[s] + 2u);
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) nonfinite[blockIdx.x] = bad ? 1 : 0;
}

#define SMX_COR_PT 4   // proteins per register tile

__global__ __launch_bounds__(256) void col_correlate_kernel(CorrelateArgs a) {
  __shared__ double sd[4];
  __shared__ long long si[4];
  const int tid = threadIdx.x, N = a.N, P = a.P;
  const long g = blockIdx.x;
  const float* x = a.cols + g * N;
  const int32_t* r = a.rank2 + g * N;
  double s = 0.0;
  long long sa = 0, saa = 0;
  for (int i = tid; i < N; i += 256) {
    const long long v = r[i];
    s += (double)x[i]; sa += v; saa += v * v;
  }
  const double mean = halving_block_sum(s, sd) / (double)N;
  sa = halving_block_sum(sa, si);
  saa = halving_block_sum(saa, si);
  if (tid == 0) { a.pe_mean[g] = mean; a.sp_Sa[g] = sa; a.sp_Saa[g] = saa; }
  for (int p0 = 0; p0 < P; p0 += SMX_COR_PT) {
    const int np = min(SMX_COR_PT, P - p0);
    double sxx = 0.0, sxy[SMX_COR_PT] = {0.0, 0.0, 0.0, 0.0};
    long long sab[SMX_COR_PT] = {0, 0, 0, 0};
    for (int i = tid; i < N; i += 256) {
      const double dx = (double)x[i] - mean;
      const long long v = r[i];
      sxx = fma(dx, dx, sxx);
#pragma unroll
      for (int q = 0; q < SMX_COR_PT; ++q)
        if (q < np) {
          const long at = (long)(p0 + q) * N + i;
          sxy[q] = fma(dx, a.prot_unit[at], sxy[q]);
          sab[q] += v * (long long)a.prot_rank2[at];
        }
    }
    if (p0 == 0) {
      sxx = halving_block_sum(sxx, sd);
      if (tid == 0) a.pe_Sxx[g] = sxx;
    }
#pragma unroll
    for (int q = 0; q < SMX_COR_PT; ++q)
      if (q < np) {   // (block-uniform)
        const double dy = halving_block_sum(sxy[q], sd);
        const long long iy = halving_block_sum(sab[q], si);
        if (tid == 0) { a.pe_Sxy[g * P + p0 + q] = dy; a.sp_Sab[g * P + p0 + q] = iy; }
      }
  }
}

int launch_keep_cols(hipStream_t st, const float* src, long ld, long rows, const int32_t* idx, int n_sel, float* dst, long N, long c0) {
  SMX_REQUIRE(src && idx && dst && rows > 0 && n_sel > 0 && c0 >= 0 && c0 + rows <= N && N <= SMX_COR_MAX_CELLS, "keep_cols: bad arguments");
  hipLaunchKernelGGL(keep_cols_kernel, dim3((unsigned)((n_sel + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, st, src, ld, (int)rows, idx,
                     n_sel, dst, N, c0);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

int launch_col_rank2(hipStream_t st, const float* cols, int n_cols, long N, unsigned* sortA, unsigned* sortB, int32_t* rank2, int32_t* nonfinite) {
  SMX_REQUIRE(cols && sortA && sortB && rank2 && nonfinite && n_cols > 0 && N > 0 && N <= SMX_COR_MAX_CELLS, "col_rank2: bad arguments");
  hipLaunchKernelGGL(col_rank2_kernel, dim3((unsigned)n_cols), dim3(256), 0, st, cols, (int)N, sortA, sortB, rank2, nonfinite);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

int launch_col_correlate(hipStream_t st, const CorrelateArgs& a, int n_cols) {
  SMX_REQUIRE(a.cols && a.rank2 && a.prot_rank2 && a.prot_unit && a.sp_Sa && a.sp_Saa && a.sp_Sab && a.pe_mean && a.pe_Sxx && a.pe_Sxy &&
              n_cols > 0 && a.N > 0 && a.N <= SMX_COR_MAX_CELLS && a.P > 0, "col_correlate: bad arguments");
  hipLaunchKernelGGL(col_correlate_kernel, dim3((unsigned)n_cols), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

// ranks and sums of n kept columns (device) -> the caller's host arrays from their element 0 on.  `sums`: (2 + P) float64, then (2 + P) int64,
// then one int32 per column (correlate_sums_bytes).  The protein operands are on the device already.
int correlate_kept(hipStream_t st, const CorrelateWork& w, int n, long N, int P, const CorrelateOut& o) {
  const size_t nn = (size_t)n, nP = nn * (size_t)P;
  CorrelateArgs a;
  a.cols = w.cols; a.rank2 = w.rank2; a.N = (int)N; a.P = P; a.prot_rank2 = w.prot_rank2; a.prot_unit = w.prot_unit;
  a.pe_mean = reinterpret_cast<double*>(w.sums); a.pe_Sxx = a.pe_mean + nn; a.pe_Sxy = a.pe_Sxx + nn;
  a.sp_Sa = reinterpret_cast<long long*>(a.pe_Sxy + nP); a.sp_Saa = a.sp_Sa + nn; a.sp_Sab = a.sp_Saa + nn;
  int32_t* nf = reinterpret_cast<int32_t*>(a.sp_Sab + nP);
  SMX_CHECK(launch_col_rank2(st, w.cols, n, N, w.sortA, w.sortB, w.rank2, nf));
  SMX_CHECK(launch_col_correlate(st, a, n));
  auto out = [&](void* dst, const void* src, size_t bytes) -> int {
    SMX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return SMX_OK;
  };
  SMX_CHECK(out(o.pe_mean, a.pe_mean, nn * 8)); SMX_CHECK(out(o.pe_Sxx, a.pe_Sxx, nn * 8)); SMX_CHECK(out(o.pe_Sxy, a.pe_Sxy, nP * 8));
  SMX_CHECK(out(o.sp_Sa, a.sp_Sa, nn * 8)); SMX_CHECK(out(o.sp_Saa, a.sp_Saa, nn * 8)); SMX_CHECK(out(o.sp_Sab, a.sp_Sab, nP * 8));
  SMX_CHECK(out(o.nonfinite, nf, nn * 4));
  SMX_HIP(hipStreamSynchronize(st));
  return SMX_OK;
}

}  // namespace smx

extern "C" {

int smx_k_col_rank2(const float* cols, int32_t n_cols, int64_t n_cells, int32_t* rank2, int32_t* nonfinite) {
  SMX_REQUIRE(cols && rank2 && nonfinite && n_cols > 0 && n_cells > 0, "bad arguments");
  SMX_REQUIRE(n_cells <= SMX_COR_MAX_CELLS, "column ranks take at most 2^20 cells");
  const size_t n = (size_t)n_cols * (size_t)n_cells;
  DeviceScratch buf;
  float* d;   // cols | rank2 | sort A | sort B | nonfinite
  SMX_CHECK(buf.get(&d, 4 * n + (size_t)n_cols));
  int32_t* dr = reinterpret_cast<int32_t*>(d + n);
  unsigned* ds = reinterpret_cast<unsigned*>(d + 2 * n);
  int32_t* dn = reinterpret_cast<int32_t*>(d + 4 * n);
  if (hipMemcpy(d, cols, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { set_error("smx_k_col_rank2: copy of the columns failed"); return SMX_ERR_HIP; }
  SMX_CHECK(launch_col_rank2(nullptr, d, n_cols, (long)n_cells, ds, ds + n, dr, dn));
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(rank2, dr, n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(nonfinite, dn, (size_t)n_cols * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("smx_k_col_rank2: the kernel or the copy of its result failed"); return SMX_ERR_HIP;
  }
  return SMX_OK;
}

int smx_k_col_correlate(const float* cols, int32_t n_cols, int64_t n_cells, const int32_t* prot_rank2, const double* prot_unit, int32_t P,
                        int64_t* sp_Sa, int64_t* sp_Saa, int64_t* sp_Sab, double* pe_mean, double* pe_Sxx, double* pe_Sxy, int32_t* nonfinite) {
  SMX_REQUIRE(cols && prot_rank2 && prot_unit && sp_Sa && sp_Saa && sp_Sab && pe_mean && pe_Sxx && pe_Sxy && nonfinite && n_cols > 0 &&
              n_cells > 0 && P > 0, "bad arguments");
  SMX_REQUIRE(n_cells <= SMX_COR_MAX_CELLS, "column correlations take at most 2^20 cells");
  const size_t n = (size_t)n_cols * (size_t)n_cells, pn = (size_t)P * (size_t)n_cells;
  DeviceScratch buf;
  double* dp;   // protein unit columns | their ranks (int32)
  float* d;     // cols | rank2 | sort A | sort B
  char* ds;     // the sums
  SMX_CHECK(buf.get(&dp, pn + (pn + 1) / 2));
  SMX_CHECK(buf.get(&d, 4 * n));
  SMX_CHECK(buf.get(&ds, correlate_sums_bytes((size_t)n_cols, (size_t)P)));
  int32_t* dpr = reinterpret_cast<int32_t*>(dp + pn);
  if (hipMemcpy(d, cols, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dp, prot_unit, pn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dpr, prot_rank2, pn * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("smx_k_col_correlate: copy of the operands failed"); return SMX_ERR_HIP;
  }
  CorrelateWork w;
  w.cols = d; w.rank2 = reinterpret_cast<int32_t*>(d + n); w.sortA = reinterpret_cast<unsigned*>(d + 2 * n); w.sortB = w.sortA + n;
  w.prot_rank2 = dpr; w.prot_unit = dp; w.sums = ds;
  const CorrelateOut o{reinterpret_cast<long long*>(sp_Sa), reinterpret_cast<long long*>(sp_Saa), reinterpret_cast<long long*>(sp_Sab), pe_mean, pe_Sxx,
                       pe_Sxy, nonfinite};
  return correlate_kept(nullptr, w, n_cols, (long)n_cells, P, o);
}

}  // extern "C"
