// smx_knn.hip -- the neighbour graph of the reference's SingleCellOMIC.neighbors (sisua/data/_single_cell_analysis.py:546-630, a proxy to
// scanpy.pp.neighbors there) on host cells Z [N][D] float32: the exact k nearest neighbours of every cell, and the per-row part of UMAP's
// fuzzy connectivities.  Model-free entries: they upload, compute, download and free their own buffers.  The assembly of the sparse
// graphs is host SciPy (sisua_amd/neighbors.py).
//   k nearest     d2(i, j) = sum_d (z_i[d] - z_j[d])^2 in float64, the direct form of smx_dist.h.  The candidates of a cell are ordered
//                 by (d2, j) ascending, a total order: the answer does not depend on how the work is cut, and duplicates are ordinary
//                 neighbours at distance 0.  One workgroup per (tile of 256 cells i, slice of the j range) in the shape of
//                 silhouette_part_kernel: z_i in registers, tiles of z_j through LDS as float64 broadcasts.  A thread keeps the d2 of its
//                 current k-th best in a register; its sorted list lives in device memory as [slice][k][N] (a wave's accesses to one
//                 rank are contiguous).  A slice walks j upwards, so a candidate enters only when d2 < the k-th best (an equal d2 has the
//                 larger j) and is inserted behind its equals; after the first tiles insertions are rare and the loop is the distance
//                 plus one compare.  The number of slices is a function of N alone (developer knob: smx_set_tuning("knn_slices", s)).
//                 A second launch merges the slices' lists, one thread per cell, by the same order.
//   UMAP rows     smooth_knn_dist and compute_membership_strengths of umap-learn with local_connectivity = 1, bandwidth = 1, as the
//                 header states them: one thread per row, at most 64 rounds of bisection, every sum in column order.  The mean of the
//                 whole table is one launch of one workgroup: smx_block.h's fixed-order column sum.
// No float atomics; no workgroup waits on another; every loop is bounded by N, k, D or 64.
#include "smx_model.h"
#include "smx_dist.h"
#include "smx_block.h"   // the fixed-order column sum

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace smx {

#define SMX_KNN_MAX_SLICES 32
#define SMX_KNN_UMAP_ROUNDS 64

// list_d [slices][k][N], list_j [slices][k][N]: slice blockIdx.y's k best (d2, j) of every cell over j in [j0, j1), j != i, ascending;
// the ranks a slice cannot fill hold (+inf, INT_MAX)
template <int DP>
__global__ __launch_bounds__(SMX_CL_TILE) void knn_part_kernel(const float* Z, long N, int D, int k, long slice_len, double* list_d,
                                                               int32_t* list_j) {
  constexpr int TJ = SMX_CL_LDS_DOUBLES / DP;
  __shared__ double sh[SMX_CL_LDS_DOUBLES];
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  const bool live = i < N;
  const long j0 = (long)blockIdx.y * slice_len, j1 = min(N, j0 + slice_len);
  double* ld_ = list_d + (long)blockIdx.y * k * N + i;   // rank p at ld_[p * N]
  int32_t* lj_ = list_j + (long)blockIdx.y * k * N + i;
  if (live)
    for (int p = 0; p < k; ++p) { ld_[(long)p * N] = INFINITY; lj_[(long)p * N] = INT_MAX; }
  if (j0 >= j1) return;   // (block-uniform)
  float zi[DP];
  load_cell<DP>(zi, Z, i, N, D);
  double kth = INFINITY;   // the d2 at rank k - 1
  for (long jt = j0; jt < j1; jt += TJ) {
    const int nj = (int)min((long)TJ, j1 - jt);
    __syncthreads();
    stage_rows<DP>(sh, Z, jt, nj, D);
    __syncthreads();
    for (int jj = 0; jj < nj; ++jj) {
      const double d2 = sqdist<DP>(zi, sh + jj * DP);
      if (d2 < kth && live && jt + jj != i) {   // rare: the sorted insertion, behind every entry with d2' <= d2 (their j is smaller)
        int p = k - 1;
        while (p > 0) {
          const double dp = ld_[(long)(p - 1) * N];
          if (dp <= d2) break;
          ld_[(long)p * N] = dp;
          lj_[(long)p * N] = lj_[(long)(p - 1) * N];
          --p;
        }
        ld_[(long)p * N] = d2;
        lj_[(long)p * N] = (int32_t)(jt + jj);
        kth = ld_[(long)(k - 1) * N];
      }
    }
  }
}

// idx [N][k], dist [N][k] = the k smallest (d2, j) over the slices' lists, dist = sqrt(d2); one thread per cell
__global__ __launch_bounds__(SMX_CL_TILE) void knn_merge_kernel(const double* list_d, const int32_t* list_j, int n_slices, long N, int k,
                                                                int32_t* idx, double* dist) {
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  if (i >= N) return;
  int pos[SMX_KNN_MAX_SLICES];
#pragma unroll
  for (int s = 0; s < SMX_KNN_MAX_SLICES; ++s) pos[s] = 0;
  for (int t = 0; t < k; ++t) {
    double bd = INFINITY;
    int bj = INT_MAX, bs = 0;
#pragma unroll
    for (int s = 0; s < SMX_KNN_MAX_SLICES; ++s) {
      if (s < n_slices && pos[s] < k) {
        const long o = ((long)s * k + pos[s]) * N + i;
        const double d = list_d[o];
        const int j = list_j[o];
        if (d < bd || (d == bd && j < bj)) { bd = d; bj = j; bs = s; }
      }
    }
#pragma unroll
    for (int s = 0; s < SMX_KNN_MAX_SLICES; ++s) pos[s] += s == bs ? 1 : 0;
    idx[i * k + t] = bj;
    dist[i * k + t] = sqrt(bd);
  }
}

// *out = the sum of x [n] in the fixed order of smx_block.h's column sum
__global__ __launch_bounds__(SMX_CL_TILE) void knn_table_sum_kernel(const double* x, long n, double* out) {
  __shared__ double sh4[4];
  const double total = halving_column_sum(x, n, sh4);
  if (threadIdx.x == 0) *out = total;
}

// one thread per row of the table idx / dist [N][K] (column 0: the cell itself): rho, sigma, weight [K]
__global__ __launch_bounds__(SMX_CL_TILE) void knn_umap_kernel(const int32_t* idx, const double* dist, long N, int K, const double* table_sum,
                                                               double* rho_out, double* sigma_out, double* weight) {
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  if (i >= N) return;
  const double* d = dist + i * K;
  const double target = log2((double)K);
  double rho = 0.0, row_sum = 0.0;
  bool found = false;
  for (int c = 0; c < K; ++c) {
    const double v = d[c];
    row_sum += v;
    if (!found && v > 0.0) { rho = v; found = true; }
  }
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int round = 0; round < SMX_KNN_UMAP_ROUNDS; ++round) {
    double psum = 0.0;
    for (int c = 1; c < K; ++c) {
      const double t = d[c] - rho;
      psum += t > 0.0 ? exp(-(t / mid)) : 1.0;
    }
    if (fabs(psum - target) < 1e-5) break;
    if (psum > target) { hi = mid; mid = (lo + hi) / 2.0; }
    else {
      lo = mid;
      mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
    }
  }
  double sigma = mid;
  const double floor_ = rho > 0.0 ? 1e-3 * (row_sum / (double)K) : 1e-3 * (*table_sum / ((double)N * (double)K));
  if (sigma < floor_) sigma = floor_;
  rho_out[i] = rho;
  sigma_out[i] = sigma;
  for (int c = 0; c < K; ++c) {
    const double t = d[c] - rho;
    double w;
    if ((long)idx[i * K + c] == i) w = 0.0;
    else if (t <= 0.0 || sigma == 0.0) w = 1.0;
    else w = exp(-(t / sigma));
    weight[i * K + c] = w;
  }
}

// slices of the j range: enough workgroups for the machine at small N, one slice once the tiles of i alone fill it -- a function of N alone
static int knn_slices(long N) {
  const long tiles = (N + SMX_CL_TILE - 1) / SMX_CL_TILE;
  int s = (int)std::max<long>(1, std::min<long>(SMX_KNN_MAX_SLICES, 1024 / tiles));
  const int forced = (int)tuning("knn_slices", 0.0);   // (read per call: a test sets it between calls)
  if (forced > 0) s = std::min(forced, SMX_KNN_MAX_SLICES);
  return s;
}

}  // namespace smx

using namespace smx;

extern "C" {

int smx_knn(const float* Z, int64_t n_cells, int32_t D, int32_t k, int32_t* idx, double* dist) {
  SMX_REQUIRE(Z && idx && dist, "knn: null argument");
  SMX_REQUIRE(D >= 1 && D <= SMX_CL_MAX_D, "knn: 1 <= D <= 128");
  SMX_REQUIRE(k >= 1 && k <= SMX_CL_MAX_K, "knn: 1 <= k <= 256");
  SMX_REQUIRE(n_cells > k && n_cells < ((int64_t)1 << 31), "knn: k < n_cells < 2^31");
  const long N = (long)n_cells;
  for (size_t e = 0; e < (size_t)N * D; ++e) SMX_REQUIRE(std::isfinite(Z[e]), "knn: an entry of Z that is not finite");
  const int S = knn_slices(N), DP = padded_width(D);
  const long tiles = (N + SMX_CL_TILE - 1) / SMX_CL_TILE;
  const int TJ = SMX_CL_LDS_DOUBLES / DP;
  const long slice_len = ((N + S - 1) / S + TJ - 1) / TJ * TJ;   // whole tiles of j
  DeviceScratch buf;
  float* dZ; double *dLd, *dDist; int32_t *dLj, *dIdx;
  SMX_CHECK(buf.get(&dZ, (size_t)N * D));
  SMX_CHECK(buf.get(&dLd, (size_t)S * k * N)); SMX_CHECK(buf.get(&dLj, (size_t)S * k * N));
  SMX_CHECK(buf.get(&dIdx, (size_t)N * k)); SMX_CHECK(buf.get(&dDist, (size_t)N * k));
  SMX_HIP(hipMemcpy(dZ, Z, (size_t)N * D * sizeof(float), hipMemcpyHostToDevice));
  const dim3 grid((unsigned)tiles, (unsigned)S), block(SMX_CL_TILE);
  switch (DP) {
    case 16: hipLaunchKernelGGL(knn_part_kernel<16>, grid, block, 0, nullptr, dZ, N, D, k, slice_len, dLd, dLj); break;
    case 32: hipLaunchKernelGGL(knn_part_kernel<32>, grid, block, 0, nullptr, dZ, N, D, k, slice_len, dLd, dLj); break;
    case 64: hipLaunchKernelGGL(knn_part_kernel<64>, grid, block, 0, nullptr, dZ, N, D, k, slice_len, dLd, dLj); break;
    default: hipLaunchKernelGGL(knn_part_kernel<128>, grid, block, 0, nullptr, dZ, N, D, k, slice_len, dLd, dLj); break;
  }
  SMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)tiles), block, 0, nullptr, dLd, dLj, S, N, k, dIdx, dDist);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(idx, dIdx, (size_t)N * k * sizeof(int32_t), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(dist, dDist, (size_t)N * k * sizeof(double), hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_knn_umap(const int32_t* idx, const double* dist, int64_t n_cells, int32_t K, double* rho, double* sigma, double* weight) {
  SMX_REQUIRE(idx && dist && rho && sigma && weight, "knn_umap: null argument");
  SMX_REQUIRE(K >= 2 && K <= SMX_CL_MAX_K + 1, "knn_umap: 2 <= K <= 257");
  SMX_REQUIRE(n_cells >= 1 && n_cells < ((int64_t)1 << 31), "knn_umap: 1 <= n_cells < 2^31");
  const long N = (long)n_cells;
  for (size_t e = 0; e < (size_t)N * K; ++e) {
    SMX_REQUIRE(idx[e] >= 0 && (long)idx[e] < N, "knn_umap: an index outside 0 .. n_cells - 1");
    SMX_REQUIRE(std::isfinite(dist[e]) && dist[e] >= 0.0, "knn_umap: a distance that is negative or not finite");
  }
  DeviceScratch buf;
  int32_t* dIdx; double *dDist, *dSum, *dRho, *dSigma, *dW;
  SMX_CHECK(buf.put(&dIdx, idx, (size_t)N * K)); SMX_CHECK(buf.put(&dDist, dist, (size_t)N * K));
  SMX_CHECK(buf.get(&dSum, (size_t)1)); SMX_CHECK(buf.get(&dRho, (size_t)N)); SMX_CHECK(buf.get(&dSigma, (size_t)N));
  SMX_CHECK(buf.get(&dW, (size_t)N * K));
  hipLaunchKernelGGL(knn_table_sum_kernel, dim3(1), dim3(SMX_CL_TILE), 0, nullptr, dDist, N * K, dSum);
  SMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(knn_umap_kernel, dim3((unsigned)((N + SMX_CL_TILE - 1) / SMX_CL_TILE)), dim3(SMX_CL_TILE), 0, nullptr, dIdx, dDist, N, K,
                     dSum, dRho, dSigma, dW);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(rho, dRho, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(sigma, dSigma, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(weight, dW, (size_t)N * K * sizeof(double), hipMemcpyDeviceToHost));
  return SMX_OK;
}

}  // extern "C"
