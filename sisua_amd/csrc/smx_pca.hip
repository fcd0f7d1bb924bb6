// smx_pca.hip -- the two dense parts of an exact PCA of a host matrix X [n_cells][G] float32, dense or CSR (the reference's
// dimension_reduce(algo='pca'), sisua/data/_single_cell_analysis.py:385-451, runs IncrementalPCA there; the eigen-decomposition of the
// G x G covariance is host NumPy: sisua_amd/neighbors.py).  Model-free entries on the block streamer of smx_prep.hip (smx_prep.h).  Both
// products run on the float64 matrix pipe, v_mfma_f64_16x16x4_f64: lane l gives A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15], one
// float64 each, and receives D[row = (l >> 4) + 4 reg][col = l & 15], reg 0 .. 3 -- NOT the row map of the other MFMAs in this tree.
//   covariance    two passes.  Pass 1: the column sums of smx_prep_stats (slices of 64 rows in row order, the slices in order), mean =
//                 sum / n on the host.  Pass 2: S = sum_r (x_r - mean)^T (x_r - mean), the operands (double)x - mean formed in registers.
//                 A workgroup of 4 waves owns a 64 x 64 macro-tile of the LOWER triangle of S (1998 genes: 528 workgroups), a wave a
//                 32 x 32 quarter as 2 x 2 accumulators; both operands of an instruction are 4 rows x 16 columns of the tile, read
//                 straight from global memory (the tile is shared through L2).  A wave walks the block's rows in order, 4 at a time, and
//                 holds its accumulators from load to store; between blocks they rest in a float64 buffer [Gp][Gp], so the chain of a
//                 sum is the same whatever the block size: blocks start on multiples of 64 global rows.  A last launch divides by n - 1
//                 and mirrors the lower triangle.
//   projection    out = (x - mean) . components^T, [n][C] float32.  One wave per 16 rows, NT = ceil(C / 16) accumulators; the genes
//                 are taken 16 at a time, lane group q = l >> 4 holding genes 16 t + 4 q + s at step s = 0 .. 3 (a 16-byte load per lane
//                 and chunk): the order over the genes is a function of G alone.
// A row at or beyond the block's rows, a column at or beyond G enters as exactly 0, never as 0 - mean.  No atomics, no workgroup waits on
// another, every loop is bounded by the block's rows, G or C.
#include "smx_model.h"
#include "smx_prep.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace smx {

#define SMX_PCA_MAX_GENES 8192
#define SMX_PCA_MAX_COMPONENTS 128
#define SMX_PCA_TILE 64   // the macro-tile of S

typedef double pca_d4 __attribute__((ext_vector_type(4)));

// acc [Gp][Gp] += the centred products of the tile's rows [0, nb); grid (Gp / 64, Gp / 64), the blocks above the diagonal leave at once
__global__ __launch_bounds__(256) void pca_cov_kernel(const float* __restrict__ tile, long nb, int G, long ld, const double* __restrict__ mean,
                                                      double* __restrict__ acc, long Gp) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;   // (block-uniform)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int i0 = bi * SMX_PCA_TILE + (wave >> 1) * 32, j0 = bj * SMX_PCA_TILE + (wave & 1) * 32;
  int ci[2], cj[2];       // this lane's operand columns (clamped into the matrix: the value is dropped where the column is past G)
  double mi[2], mj[2];
  bool vi[2], vj[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int a = i0 + 16 * t + fr, b = j0 + 16 * t + fr;
    vi[t] = a < G; vj[t] = b < G;
    ci[t] = vi[t] ? a : G - 1; cj[t] = vj[t] ? b : G - 1;
    mi[t] = mean[ci[t]]; mj[t] = mean[cj[t]];
  }
  pca_d4 c[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) c[s][t][r] = acc[(long)(i0 + 16 * s + fq + 4 * r) * Gp + j0 + 16 * t + fr];
  for (long r0 = 0; r0 < nb; r0 += 4) {
    const long row = r0 + fq;
    const bool rv = row < nb;
    const float* p = tile + (rv ? row : nb - 1) * ld;
    double a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const double xa = (double)p[ci[t]] - mi[t], xb = (double)p[cj[t]] - mj[t];
      a[t] = (rv && vi[t]) ? xa : 0.0;
      b[t] = (rv && vj[t]) ? xb : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t) c[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[t], c[s][t], 0, 0, 0);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[(long)(i0 + 16 * s + fq + 4 * r) * Gp + j0 + 16 * t + fr] = c[s][t][r];
}

// acc [Gp][Gp] in place: the lower triangle (diagonal included) / (n - 1), mirrored above the diagonal
__global__ __launch_bounds__(256) void pca_cov_finish_kernel(double* __restrict__ acc, int G, long Gp, double denom) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)G * G) return;
  const long i = e / G, j = e - i * G;
  if (j > i) return;
  const double v = acc[i * Gp + j] / denom;
  acc[i * Gp + j] = v;
  acc[j * Gp + i] = v;
}

// out [nb][C] = (tile - mean) . comp^T; one wave (a workgroup of 64) per 16 rows, NT column tiles of 16 components
template <int NT>
__global__ __launch_bounds__(64) void pca_project_kernel(const float* __restrict__ tile, long nb, int G, long ld, const double* __restrict__ mean,
                                                         const double* __restrict__ comp, int C, float* __restrict__ out) {
  const int lane = threadIdx.x, fr = lane & 15, fq = lane >> 4;
  const long row0 = (long)blockIdx.x * 16, row = row0 + fr;
  const bool rv = row < nb;
  const float* p = tile + (rv ? row : nb - 1) * ld;
  const double* cp[NT];
  bool cv[NT];
  pca_d4 c[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int cc = 16 * t + fr;
    cv[t] = cc < C;
    cp[t] = comp + (long)(cv[t] ? cc : C - 1) * G;
    c[t] = pca_d4{0.0, 0.0, 0.0, 0.0};
  }
  for (int g0 = 0; g0 < G; g0 += 16) {
    const int g = g0 + 4 * fq;                                   // this lane's four genes of the chunk: g + s at step s
    const int gl = g + 4 <= (int)ld ? g : (int)ld - 4;           // (ld is a multiple of 4: an aligned 16-byte load inside the row)
    const float4 v = *reinterpret_cast<const float4*>(p + gl);
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bool gv = g + s < G;
      const int gc = gv ? g + s : G - 1;
      const double a = (rv && gv) ? (double)e[s] - mean[gc] : 0.0;   // (gl == g wherever gv holds)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const double w = cp[t][gc];
        c[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (gv && cv[t]) ? w : 0.0, c[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long orow = row0 + fq + 4 * r;
      const int ocol = 16 * t + fr;
      if (orow < nb && ocol < C) out[orow * C + ocol] = (float)c[t][r];
    }
}

namespace {

int pca_check(const char* who, const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
              int32_t block_rows, PrepInput* in) {
  SMX_CHECK(prep_check_input(who, x, indptr, cols, vals, n_cells, n_genes, block_rows, 0, nullptr, in));
  SMX_REQUIRE(n_genes <= SMX_PCA_MAX_GENES, (std::string(who) + ": n_genes <= 8192 (the covariance takes 8 n_genes^2 bytes)").c_str());
  return SMX_OK;
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_pca_cov(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                int32_t block_rows, double* mean, double* cov) {
  PrepInput in;
  SMX_CHECK(pca_check("pca_cov", x, indptr, cols, vals, n_cells, n_genes, block_rows, &in));
  SMX_REQUIRE(n_cells >= 2, "pca_cov: n_cells >= 2");
  SMX_REQUIRE(mean && cov, "pca_cov: null output");
  const long N = in.N, ld = in.ld;
  const int G = in.G;
  const long Gp = ((long)G + SMX_PCA_TILE - 1) / SMX_PCA_TILE * SMX_PCA_TILE;
  DeviceScratch buf;
  PrepStage st;
  SMX_CHECK(prep_stage_alloc(buf, in, &st, true));
  GenePart part; GeneAcc sums;
  SMX_CHECK(prep_gene_acc_alloc(buf, in, &part, &sums));
  double *dMean, *dAcc;
  SMX_CHECK(buf.get(&dMean, (size_t)G));
  SMX_CHECK(buf.get(&dAcc, (size_t)Gp * Gp));   // (zeros)
  const bool one_block = in.block >= N;
  // pass 1: the column sums, in the order of smx_prep_stats
  for (long r0 = 0; r0 < N; r0 += in.block) {
    const long nb = std::min(in.block, N - r0);
    SMX_CHECK(prep_load_block(in, st, r0, nb));
    SMX_CHECK(prep_launch_gene_sums(st.tile, nb, ld, r0, nullptr, part, sums));
    SMX_HIP(hipDeviceSynchronize());   // the next block's copy overwrites the tile
  }
  SMX_HIP(hipMemcpy(mean, sums.sum, (size_t)G * sizeof(double), hipMemcpyDeviceToHost));
  for (int g = 0; g < G; ++g) mean[g] /= (double)N;
  SMX_HIP(hipMemcpy(dMean, mean, (size_t)G * sizeof(double), hipMemcpyHostToDevice));
  // pass 2: the centred products, in global row order
  const unsigned T = (unsigned)(Gp / SMX_PCA_TILE);
  for (long r0 = 0; r0 < N; r0 += in.block) {
    const long nb = std::min(in.block, N - r0);
    if (!one_block) SMX_CHECK(prep_load_block(in, st, r0, nb));   // (a single block is still on the device)
    hipLaunchKernelGGL(pca_cov_kernel, dim3(T, T), dim3(256), 0, nullptr, st.tile, nb, G, ld, dMean, dAcc, Gp);
    SMX_HIP(hipGetLastError());
    SMX_HIP(hipDeviceSynchronize());
  }
  hipLaunchKernelGGL(pca_cov_finish_kernel, dim3((unsigned)(((long)G * G + 255) / 256)), dim3(256), 0, nullptr, dAcc, G, Gp, (double)(N - 1));
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipMemcpy2D(cov, (size_t)G * sizeof(double), dAcc, (size_t)Gp * sizeof(double), (size_t)G * sizeof(double), (size_t)G,
                      hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_pca_project(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                    int32_t block_rows, const double* mean, const double* components, int32_t n_components, float* out) {
  PrepInput in;
  SMX_CHECK(pca_check("pca_project", x, indptr, cols, vals, n_cells, n_genes, block_rows, &in));
  SMX_REQUIRE(mean && components && out, "pca_project: null argument");
  SMX_REQUIRE(n_components >= 1 && n_components <= SMX_PCA_MAX_COMPONENTS, "pca_project: 1 <= n_components <= 128");
  const long N = in.N, ld = in.ld;
  const int G = in.G, C = n_components;
  for (int g = 0; g < G; ++g) SMX_REQUIRE(std::isfinite(mean[g]), "pca_project: a mean that is not finite");
  for (size_t e = 0; e < (size_t)C * G; ++e) SMX_REQUIRE(std::isfinite(components[e]), "pca_project: a component that is not finite");
  DeviceScratch buf;
  PrepStage st;
  SMX_CHECK(prep_stage_alloc(buf, in, &st, true));
  double *dMean, *dComp; float* dOut;
  SMX_CHECK(buf.put(&dMean, mean, (size_t)G));
  SMX_CHECK(buf.put(&dComp, components, (size_t)C * G));
  SMX_CHECK(buf.get(&dOut, (size_t)in.block * C));
  const int NT = (C + 15) / 16;
  for (long r0 = 0; r0 < N; r0 += in.block) {
    const long nb = std::min(in.block, N - r0);
    SMX_CHECK(prep_load_block(in, st, r0, nb));
    const dim3 grid((unsigned)((nb + 15) / 16)), block(64);
#define SMX_PCA_PROJECT(NTV) hipLaunchKernelGGL(pca_project_kernel<NTV>, grid, block, 0, nullptr, st.tile, nb, G, ld, dMean, dComp, C, dOut)
    if (NT <= 1) SMX_PCA_PROJECT(1);
    else if (NT <= 2) SMX_PCA_PROJECT(2);
    else if (NT <= 4) SMX_PCA_PROJECT(4);
    else SMX_PCA_PROJECT(8);
#undef SMX_PCA_PROJECT
    SMX_HIP(hipGetLastError());
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(out + (size_t)r0 * C, dOut, (size_t)nb * C * sizeof(float), hipMemcpyDeviceToHost));
  }
  return SMX_OK;
}

}  // extern "C"
