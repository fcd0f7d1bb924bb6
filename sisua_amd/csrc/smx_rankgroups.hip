// smx_rankgroups.hip -- the matrix work of "which genes mark this group of cells?" (the reference's SingleCellOMIC.rank_vars_groups, a proxy
// to scanpy.tl.rank_genes_groups: _single_cell_analysis.py:862-918).  Model-free entries: they upload, compute, download and free their own
// buffers.  The device does what is of size N x G; the closing formulas (Welch's t, the rank-sum z, p-values, the FDR step-up, the ranking)
// are host NumPy / SciPy on [K][G] arrays (sisua_amd/rank_groups.py).
//   group moments     the host matrix streams through smx_prep.h's tile in blocks of rows, twice: the sums and the non-zero counts of every
//                     (group, gene), then the squares of the float64 differences from the group's mean (sum / count, the IEEE division).
//                     One wave per (256 genes, group), a thread per 4 consecutive genes (a 16-byte load per row).  The wave reads 64 labels
//                     at a time, a ballot names the rows of its group, and only those rows are loaded, four in flight, and added IN ROW
//                     ORDER onto accumulators that persist across blocks: the sum of (group, gene) is ((x_r1 + x_r2) + x_r3) ... over the
//                     group's global rows in order, whatever the block size and whatever form the matrix crossed in.  No atomics.
//   group rank sums   one 256-thread workgroup per gene.  Against the rest: all N cells are sorted (smx_block.h's stable radix sort on the
//                     order-preserving key, -0 as +0), the tie-run pass gives every position its run's start and every start its run's
//                     end, and the doubled average rank start + end + 2 of a position goes to its cell's group.  Against a reference
//                     group the ranks are those within the cells of g and of the reference, for every other group g -- still ONE sort per
//                     gene, by (value, label), and a prefix count of the reference's cells over the sorted order (group_ranksum_ref_kernel).
//                     Sorting each comparison's cell list through the sort's `init` argument was built and measured beside it: equal at
//                     a small reference, 1.4x (12 groups) to 4x (64 groups) slower at a reference of half the cells
//                     (profiles/rank_groups_ref_ab.txt).  Accumulation is in 64-bit integers with LDS atomics (they commute): 2 R_g
//                     <= 2 N^2 = 2^41 and sum (t^3 - t) <= N^3 = 2^60 at N = 2^20.
// Every loop is bounded by a block's rows or by N.
#include "smx_model.h"
#include "smx_prep.h"    // the block streamer of the count matrix
#include "smx_block.h"   // the radix sort, the tie-run pass, the keys and the fixed-order sums

#include <algorithm>
#include <vector>

namespace smx {

#define SMX_RG_MAX_CELLS (1l << 20)            // the rank sums: 2 N^2 and N^3 stay inside int64
#define SMX_RG_MAX_GROUPS 256                  // the rank sums' LDS accumulators
#define SMX_RG_MAX_MOMENT_GROUPS 65535         // the moments' grid.y
#define SMX_RG_MAX_ACC ((size_t)1 << 26)       // the moments' accumulators: n_groups x (n_genes rounded up to 4) entries of 24 bytes
#define SMX_RG_SORT_BYTES ((size_t)256 << 20)  // columns and sort arrays on the device at a time

// pass 0: sum and nnz of (group blockIdx.y, genes 4 t .. 4 t + 3) over the tile's rows of the group, in row order; pass 1: css likewise
__global__ __launch_bounds__(64) void group_moment_kernel(const float* __restrict__ tile, long nb, long ld, long row0,
                                                          const int32_t* __restrict__ labels, const long long* __restrict__ count, int pass,
                                                          double* __restrict__ sum, double* __restrict__ css, long long* __restrict__ nnz) {
  const int lane = threadIdx.x, k = blockIdx.y;
  const long g = ((long)blockIdx.x * 64 + lane) * 4;
  const bool live = g < ld;   // (ld is a multiple of 4; a dead lane still reads labels and votes)
  const long o = (long)k * ld + g;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, mu[4] = {0.0, 0.0, 0.0, 0.0};
  long long z[4] = {0, 0, 0, 0};
  if (live) {
    const double n = (double)count[k];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (pass == 0) { s[q] = sum[o + q]; z[q] = nnz[o + q]; }
      else { s[q] = css[o + q]; mu[q] = sum[o + q] / n; }   // (an empty group has no row: its mean is never used)
    }
  }
  for (long t0 = 0; t0 < nb; t0 += 64) {
    const long r = t0 + lane;
    unsigned long long mask = __ballot(r < nb && labels[row0 + r] == k);
    while (mask) {   // (wave-uniform) the next four rows of the group: loads first, then the sums in row order
      int idx[4];
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        idx[u] = mask ? __ffsll((unsigned long long)mask) - 1 : -1;
        mask &= mask - 1ull;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        v[u] = (idx[u] >= 0 && live) ? *reinterpret_cast<const float4*>(tile + (t0 + idx[u]) * ld + g) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (idx[u] >= 0) {
          const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (pass == 0) { s[q] += (double)e[q]; z[q] += e[q] != 0.f ? 1 : 0; }
            else { const double d = (double)e[q] - mu[q]; s[q] = fma(d, d, s[q]); }
          }
        }
    }
  }
  if (live) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (pass == 0) { sum[o + q] = s[q]; nnz[o + q] = z[q]; }
      else css[o + q] = s[q];
    }
  }
}

struct RankSumArgs {
  const float* cols;           // [n][N] gene-major
  const int32_t* labels;       // [N]
  const long long* count;      // [K]
  int N, K, ref, n;            // n: the columns of this launch
  long stride;                 // sort entries per column: N + 1
  unsigned *A, *B, *C;         // [n][stride]: the sort's ping-pong arrays; every position's run start
  unsigned *D, *E, *F;         // [n][stride]: with a reference
  long long* rank2_sum;        // [K][n]
  long long* tie;              // [n], or [K][n] with a reference
};

// every group against the rest: ranks over all N cells
__global__ __launch_bounds__(256) void group_ranksum_kernel(RankSumArgs a) {
  __shared__ SortShared sh;
  __shared__ unsigned long long acc[SMX_RG_MAX_GROUPS];
  __shared__ long long s4[4];
  const int tid = threadIdx.x, N = a.N;
  const long gene = blockIdx.x, base = gene * a.stride;
  const float* x = a.cols + gene * N;
  const int32_t* lab = a.labels;
  unsigned *A = a.A + base, *Cs = a.C + base;
  acc[tid] = 0ull;   // (256 threads, 256 words; the sort's first barrier comes before any use)
  const auto key = [x](unsigned i) { return order_key(x[i]); };
  const unsigned* S = block_radix_sort(key, N, 4, nullptr, A, a.B + base, sh);   // (four passes: the result is in B)
  block_tie_runs(key, [Cs](int j, unsigned, unsigned start) { Cs[j] = start; }, N, S, A, sh);
  long long tie = 0;
  for (int j = tid; j < N; j += 256) {
    const unsigned s = Cs[j], e = A[s];
    atomicAdd(&acc[lab[S[j]]], (unsigned long long)(s + e + 2u));
    if ((unsigned)j == s) {
      const long long t = (long long)(e - s) + 1;
      tie += t * t * t - t;
    }
  }
  tie = halving_block_sum(tie, s4);   // (its barriers also order the LDS atomics before the reads below)
  for (int k = tid; k < a.K; k += 256) a.rank2_sum[(long)k * a.n + gene] = (long long)acc[k];
  if (tid == 0) a.tie[gene] = tie;
}

// With a reference, ONE sort per gene: the cells ordered by (value, label), the runs of equal values and, inside them, of equal (value,
// label), and D[j] = the reference's cells among the sorted positions before j.  A cell of group g in the run [s, e] has, among the cells
// of g and of the reference, 2 x (cells below) + (cells tied) + 1 = its doubled rank within g alone + D[s] + D[e + 1]; the doubled ranks
// within g alone add up to n_g (n_g + 1).  A run with c_g cells of g and c_r of the reference gives the comparison a tie run of c_g + c_r.
__global__ __launch_bounds__(256) void group_ranksum_ref_kernel(RankSumArgs a) {
  __shared__ SortShared sh;
  __shared__ unsigned long long acc[SMX_RG_MAX_GROUPS], tacc[SMX_RG_MAX_GROUPS];
  __shared__ long long s4[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, N = a.N, ref = a.ref;
  const long gene = blockIdx.x, base = gene * a.stride;
  const float* x = a.cols + gene * N;
  const int32_t* lab = a.labels;
  unsigned *A = a.A + base, *B = a.B + base, *Cs = a.C + base, *D = a.D + base, *E = a.E + base, *F = a.F + base;
  acc[tid] = 0ull; tacc[tid] = 0ull;   // (the sort's first barrier comes before any use)
  const auto key = [x](unsigned i) { return order_key(x[i]); };
  const auto key2 = [x, lab](unsigned i) { return ((uint64_t)order_key(x[i]) << 8) | (uint64_t)(unsigned)lab[i]; };
  const unsigned* S = block_radix_sort(key2, N, 5, nullptr, A, B, sh);   // (five passes: the result is in A)
  block_tie_runs(key, [Cs](int j, unsigned, unsigned start) { Cs[j] = start; }, N, S, B, sh);
  block_tie_runs(key2, [E](int j, unsigned, unsigned start) { E[j] = start; }, N, S, F, sh);
  unsigned carry = 0;
  for (int t0 = 0; t0 < N; t0 += 256) {
    const int j = t0 + tid;
    const unsigned f = (j < N && lab[S[j]] == ref) ? 1u : 0u;
    const unsigned inc = wave_scan_add(f);
    if (lane == 63) sh.wtot[w] = inc;
    __syncthreads();
    unsigned pre = carry + inc - f;
    for (int q = 0; q < w; ++q) pre += sh.wtot[q];
    if (j < N) D[j] = pre;
    carry += (sh.wtot[0] + sh.wtot[1]) + (sh.wtot[2] + sh.wtot[3]);
    __syncthreads();
  }
  if (tid == 0) D[N] = carry;
  __syncthreads();
  long long tref = 0;
  for (int j = tid; j < N; j += 256) {
    const unsigned s = Cs[j], e = B[s], lo = D[s], hi = D[e + 1];
    const int l = lab[S[j]];
    const long long cr = (long long)(hi - lo), tr = cr * cr * cr - cr;
    if ((unsigned)j == s) tref += tr;
    if (l != ref) {
      atomicAdd(&acc[l], (unsigned long long)(lo + hi));
      if (E[j] == (unsigned)j) {   // the head of the group's cells in this run
        const long long t = (long long)(F[j] - (unsigned)j) + 1 + cr;
        atomicAdd(&tacc[l], (unsigned long long)(t * t * t - t - tr));
      }
    }
  }
  tref = halving_block_sum(tref, s4);   // (its barriers also order the LDS atomics before the reads below)
  for (int k = tid; k < a.K; k += 256) {
    const long long n = a.count[k];
    if (k == ref || n == 0) continue;   // (those rows stay 0)
    a.rank2_sum[(long)k * a.n + gene] = n * (n + 1) + (long long)acc[k];
    a.tie[(long)k * a.n + gene] = tref + (long long)tacc[k];
  }
}

namespace {

int check_labels(const char* who, const int32_t* labels, int64_t n_cells, int32_t n_groups, std::vector<long long>* count) {
  const std::string w(who);
  SMX_REQUIRE(labels != nullptr, (w + ": null labels").c_str());
  count->assign((size_t)n_groups, 0);
  for (int64_t i = 0; i < n_cells; ++i) {
    SMX_REQUIRE(labels[i] >= 0 && labels[i] < n_groups, (w + ": a label outside 0 .. n_groups - 1").c_str());
    ++(*count)[(size_t)labels[i]];
  }
  return SMX_OK;
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_group_moments(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                      int32_t block_rows, const int32_t* labels, int32_t n_groups, int64_t* count, double* sum, double* css, int64_t* nnz) {
  PrepInput in;
  SMX_CHECK(prep_check_input("group_moments", x, indptr, cols, vals, n_cells, n_genes, block_rows, 0, nullptr, &in));
  SMX_REQUIRE(count && sum && css && nnz, "group_moments: null output");
  SMX_REQUIRE(n_groups >= 1 && n_groups <= SMX_RG_MAX_MOMENT_GROUPS, "group_moments: 1 <= n_groups <= 65535");
  SMX_REQUIRE((size_t)n_groups * (size_t)in.ld <= SMX_RG_MAX_ACC, "group_moments: n_groups x n_genes <= 2^26");
  std::vector<long long> cnt;
  SMX_CHECK(check_labels("group_moments", labels, n_cells, n_groups, &cnt));
  const long N = in.N, ld = in.ld;
  const size_t K = (size_t)n_groups, G = (size_t)in.G, acc = K * (size_t)ld;
  DeviceScratch buf;
  PrepStage st;
  SMX_CHECK(prep_stage_alloc(buf, in, &st, true));
  int32_t* dLab; long long *dCnt, *dNnz; double *dSum, *dCss;
  SMX_CHECK(buf.put(&dLab, labels, (size_t)N));
  SMX_CHECK(buf.put(&dCnt, (const long long*)cnt.data(), K));
  SMX_CHECK(buf.get(&dSum, acc)); SMX_CHECK(buf.get(&dCss, acc)); SMX_CHECK(buf.get(&dNnz, acc));   // (dmalloc zeroes)
  const dim3 grid((unsigned)((ld / 4 + 63) / 64), (unsigned)n_groups);
  const bool one_block = in.block >= N;
  for (int pass = 0; pass < 2; ++pass)
    for (long r0 = 0; r0 < N; r0 += in.block) {
      const long nb = std::min(in.block, N - r0);
      if (pass == 0 || !one_block) SMX_CHECK(prep_load_block(in, st, r0, nb));   // (a matrix of one block is still in the tile)
      hipLaunchKernelGGL(group_moment_kernel, grid, dim3(64), 0, nullptr, st.tile, nb, ld, r0, dLab, dCnt, pass, dSum, dCss, dNnz);
      SMX_HIP(hipGetLastError());
      SMX_HIP(hipDeviceSynchronize());   // the next block's copy overwrites the tile
    }
  for (size_t k = 0; k < K; ++k) count[k] = cnt[k];
  const size_t dp = (size_t)ld * 8, hp = G * 8;
  SMX_HIP(hipMemcpy2D(sum, hp, dSum, dp, hp, K, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy2D(css, hp, dCss, dp, hp, K, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy2D(nnz, hp, dNnz, dp, hp, K, hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_group_ranksums(const float* cols, int32_t n_cols, int64_t n_cells, const int32_t* labels, int32_t n_groups, int32_t reference,
                       int64_t* rank2_sum, int64_t* tie_term) {
  SMX_REQUIRE(cols && rank2_sum && tie_term && n_cols > 0, "group_ranksums: bad arguments");
  SMX_REQUIRE(n_cells >= 1 && n_cells <= SMX_RG_MAX_CELLS, "group_ranksums: 1 <= n_cells <= 2^20");
  SMX_REQUIRE(n_groups >= 1 && n_groups <= SMX_RG_MAX_GROUPS, "group_ranksums: 1 <= n_groups <= 256");
  SMX_REQUIRE(reference >= -1 && reference < n_groups, "group_ranksums: reference is -1 (the rest) or a group");
  std::vector<long long> cnt;
  SMX_CHECK(check_labels("group_ranksums", labels, n_cells, n_groups, &cnt));
  const size_t N = (size_t)n_cells, K = (size_t)n_groups, Gt = (size_t)n_cols;
  const bool ref = reference >= 0;
  const size_t stride = N + 1, n_arr = ref ? 6 : 3, n_tie = ref ? K : 1;
  const size_t chunk = std::max<size_t>(1, std::min(Gt, SMX_RG_SORT_BYTES / (4 * N + 4 * n_arr * stride)));
  DeviceScratch buf;
  float* dCols; int32_t* dLab; unsigned* dSort; long long *dRank, *dTie, *dCnt;
  SMX_CHECK(buf.get(&dCols, chunk * N));
  SMX_CHECK(buf.put(&dLab, labels, N));
  SMX_CHECK(buf.put(&dCnt, (const long long*)cnt.data(), K));
  SMX_CHECK(buf.get(&dSort, n_arr * chunk * stride));
  SMX_CHECK(buf.get(&dRank, K * chunk));
  SMX_CHECK(buf.get(&dTie, n_tie * chunk));
  for (size_t g0 = 0; g0 < Gt; g0 += chunk) {
    const size_t n = std::min(chunk, Gt - g0);
    SMX_HIP(hipMemcpy(dCols, cols + g0 * N, n * N * sizeof(float), hipMemcpyHostToDevice));
    SMX_HIP(hipMemset(dRank, 0, K * n * 8));
    SMX_HIP(hipMemset(dTie, 0, n_tie * n * 8));
    RankSumArgs a;
    a.cols = dCols; a.labels = dLab; a.count = dCnt; a.N = (int)N; a.K = n_groups; a.ref = reference; a.n = (int)n; a.stride = (long)stride;
    a.A = dSort; a.B = dSort + chunk * stride; a.C = dSort + 2 * chunk * stride;
    a.D = dSort + 3 * chunk * stride; a.E = dSort + 4 * chunk * stride; a.F = dSort + 5 * chunk * stride;   // (allocated with a reference only)
    a.rank2_sum = dRank; a.tie = dTie;
    if (ref) hipLaunchKernelGGL(group_ranksum_ref_kernel, dim3((unsigned)n), dim3(256), 0, nullptr, a);
    else hipLaunchKernelGGL(group_ranksum_kernel, dim3((unsigned)n), dim3(256), 0, nullptr, a);
    SMX_HIP(hipGetLastError());
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy2D(rank2_sum + g0, Gt * 8, dRank, n * 8, n * 8, K, hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy2D(tie_term + g0, Gt * 8, dTie, n * 8, n * 8, n_tie, hipMemcpyDeviceToHost));
  }
  return SMX_OK;
}

}  // extern "C"
