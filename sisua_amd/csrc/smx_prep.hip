// smx_prep.hip -- what the reference's loaders do to a count matrix BEFORE training (sisua/data/_single_cell_analysis.py: filter_cells,
// filter_genes, normalize, expm1, filter_highly_variable_genes -- thin proxies to scanpy there), on a host matrix [n_cells][G] given dense
// or as CSR.  Model-free entries: they upload, compute, download and free their own buffers.  The device does the two things of size
// N x G -- the statistics of a VIEW of the matrix (smx_prep_stats) and the view written out (smx_prep_apply); everything of size N or G
// (medians, bins, cut-offs) is host NumPy (sisua_amd/preprocess.py).
//   view              v(r, g) = f(x(r, g) / c_r), c_r a float32 per-cell divisor or none, f the identity, log1pf or expm1f, in float32 with
//                     the IEEE division.  ONE kernel (prep_view_kernel; prep_csr_vals_kernel over stored entries) evaluates it, for both
//                     entry points: smx_prep_stats rewrites its device tile through it and then reads plain values, so the statistics of a
//                     view of X and those of the matrix smx_prep_apply made from X are sums of the same numbers.
//   blocks of rows    the matrix streams through one device tile [block_rows][ld], ld = G rounded up to 4, padding zero.  A dense block is
//                     a pitched copy; a CSR block crosses as CSR and is expanded by launch_csr_rows.  block_rows is a multiple of
//                     SMX_PREP_SLICE, so a block begins on a slice boundary of the GLOBAL row ids.
//   per-cell pass     one wave per row, lane l adds columns 4 l + 256 t + q in column order (float64), then the xor butterfly: the form of
//                     row_stats_kernel.  The order is a function of the column ids alone.
//   per-gene pass     one thread per 4 consecutive genes (a 16-byte load per row, a wave reads 1 KiB of a row), one workgroup per (256
//                     genes, slice of SMX_PREP_SLICE rows): a thread adds its slice's rows in row order and writes one partial per gene.  A
//                     second launch adds the block's slices in order onto accumulators that persist across blocks: the sum of a gene is
//                     ((slice 0 + slice 1) + slice 2) ... whatever the block size.
// No atomics, no workgroup waits on another, every loop is bounded by the block's rows, ld or a row's entries.  Both passes are
// memory-bound and small beside the PCIe copy of the block, which is why the view costs a pass of its own instead of being fused.
#include "smx_model.h"
#include "smx_prep.h"   // PrepInput, PrepStage and the per-gene sums: shared with smx_pca.hip
#include "smx_block.h"  // wave_sum_f64: the per-cell pass's butterfly, shared with row_stats_kernel

#include <algorithm>
#include <cmath>
#include <vector>

namespace smx {

#define SMX_PREP_TILE_BYTES ((size_t)64 << 20)   // the library's choice of block: about this much tile
#define SMX_PREP_MAX_TILE_BYTES ((size_t)1 << 30)
#define SMX_PREP_MAX_GENES (1 << 20)

struct PrepView {
  int func;               // 0 identity, 1 log1pf, 2 expm1f
  const float* row_div;   // [n_cells] (device) or NULL
  const float* mean;      // [G] (device) or NULL: then (v - mean[g]) / sd[g]
  const float* sd;
  int clip;
  float max_value;
};

__device__ __forceinline__ float prep_view(float x, int func, bool has_div, float c) {
  float v = has_div ? x / c : x;
  if (func == 1) v = log1pf(v);
  else if (func == 2) v = expm1f(v);
  return v;
}

// the tile [n][ld] in place: the view, then the centring and the clip where asked; columns >= G are written as zero
__global__ __launch_bounds__(256) void prep_view_kernel(float* __restrict__ tile, long n, int G, long ld, long row0, PrepView w) {
  const long q4 = ld >> 2, total = n * q4;
  const bool has_div = w.row_div != nullptr;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / q4;
    const int g = (int)(i - r * q4) * 4;
    float4* p = reinterpret_cast<float4*>(tile + r * ld + g);
    const float4 v = *p;
    const float c = has_div ? w.row_div[row0 + r] : 1.f;
    float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float t = 0.f;
      if (g + q < G) {
        t = prep_view(e[q], w.func, has_div, c);
        if (w.mean) t = (t - w.mean[g + q]) / w.sd[g + q];
        if (w.clip) t = t > w.max_value ? w.max_value : t;
      }
      e[q] = t;
    }
    *p = make_float4(e[0], e[1], e[2], e[3]);
  }
}

// the stored entries of n CSR rows in place, one wave per row.  indptr: the block's n + 1 absolute offsets; vals starts at entry indptr[0]
__global__ __launch_bounds__(256) void prep_csr_vals_kernel(const int64_t* __restrict__ indptr, float* __restrict__ vals, long n, long row0,
                                                            PrepView w) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const bool has_div = w.row_div != nullptr;
  const float c = has_div ? w.row_div[row0 + row] : 1.f;
  const int64_t base = indptr[0];
  for (int64_t i = indptr[row] - base + lane; i < indptr[row + 1] - base; i += 64) vals[i] = prep_view(vals[i], w.func, has_div, c);
}

// total[row] = the float64 sum of the row's values (of the genes the mask keeps), n_genes[row] = its entries > 0
__global__ __launch_bounds__(256) void prep_cell_kernel(const float* __restrict__ tile, long n, int G, long ld, long row0,
                                                        const uint8_t* __restrict__ mask, double* __restrict__ total,
                                                        int32_t* __restrict__ n_genes) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const float* r = tile + row * ld;
  double tot = 0.0;
  int cnt = 0;
  for (int g = lane * 4; g < G; g += 256) {
    const float4 v = *reinterpret_cast<const float4*>(r + g);   // (ld is a multiple of 4)
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (g + q < G) {
        if (!mask || mask[g + q]) tot += (double)e[q];
        cnt += e[q] > 0.f ? 1 : 0;
      }
  }
  tot = wave_sum_f64(tot);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (lane == 0) {
    total[row0 + row] = tot;
    n_genes[row0 + row] = cnt;
  }
}

// slice blockIdx.y of the tile's rows, genes 4 t .. 4 t + 3 of thread t: the rows in order
__global__ __launch_bounds__(64) void prep_gene_part_kernel(const float* __restrict__ tile, long n, long ld, long row0,
                                                            const float* __restrict__ thresh, GenePart p) {
  const long g = ((long)blockIdx.x * 64 + threadIdx.x) * 4;
  if (g >= ld) return;
  const long s = blockIdx.y, r0 = s * SMX_PREP_SLICE, r1 = r0 + SMX_PREP_SLICE < n ? r0 + SMX_PREP_SLICE : n;
  double sum[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
  int pos[4] = {0, 0, 0, 0}, above[4] = {0, 0, 0, 0};
#pragma unroll 4
  for (long r = r0; r < r1; ++r) {
    const float4 v = *reinterpret_cast<const float4*>(tile + r * ld + g);
    const float e[4] = {v.x, v.y, v.z, v.w};
    const float t = thresh ? thresh[row0 + r] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double d = (double)e[q];
      sum[q] += d;
      sq[q] += d * d;   // (the product of two float32 values is exact in float64)
      pos[q] += e[q] > 0.f ? 1 : 0;
      above[q] += (thresh && e[q] > t) ? 1 : 0;
    }
  }
  const long o = s * ld + g;   // (ld is a multiple of 4: the four partials of a thread are inside the row)
#pragma unroll
  for (int q = 0; q < 4; ++q) { p.sum[o + q] = sum[q]; p.sq[o + q] = sq[q]; p.pos[o + q] = pos[q]; p.above[o + q] = above[q]; }
}

// the block's slices onto the running accumulators, in slice order
__global__ __launch_bounds__(256) void prep_gene_combine_kernel(GenePart p, int slices, long ld, GeneAcc a) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= ld) return;
  double sum = a.sum[g], sq = a.sq[g];
  int64_t pos = a.pos[g], above = a.above[g];
  for (int s = 0; s < slices; ++s) {
    const long o = (long)s * ld + g;
    sum += p.sum[o]; sq += p.sq[o]; pos += p.pos[o]; above += p.above[o];
  }
  a.sum[g] = sum; a.sq[g] = sq; a.pos[g] = pos; a.above[g] = above;
}

// every refusal of the shared arguments, before any device work
int prep_check_input(const char* who, const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells,
                     int32_t n_genes, int32_t block_rows, int32_t func, const float* row_div, PrepInput* in) {
  const std::string w(who);
  SMX_REQUIRE((x != nullptr) != (indptr != nullptr), (w + ": exactly one of the dense matrix and the CSR arrays").c_str());
  SMX_REQUIRE(n_cells >= 1 && n_cells < ((int64_t)1 << 31), (w + ": 1 <= n_cells < 2^31").c_str());
  SMX_REQUIRE(n_genes >= 1 && n_genes <= SMX_PREP_MAX_GENES, (w + ": 1 <= n_genes <= 2^20").c_str());
  SMX_REQUIRE(block_rows >= 0, (w + ": block_rows >= 0 (0: the library's choice)").c_str());
  SMX_REQUIRE(func >= 0 && func <= 2, (w + ": func is 0 (identity), 1 (log1p) or 2 (expm1)").c_str());
  in->x = x; in->csr = CsrRows{indptr, cols, vals}; in->N = (long)n_cells; in->G = n_genes; in->ld = ((long)n_genes + 3) & ~3L;
  if (row_div)
    for (long i = 0; i < in->N; ++i)
      SMX_REQUIRE(std::isfinite(row_div[i]) && row_div[i] != 0.f, (w + ": a row divisor that is zero or not finite").c_str());
  const size_t row_bytes = (size_t)in->ld * sizeof(float);
  long br = block_rows > 0 ? (long)block_rows : (long)(SMX_PREP_TILE_BYTES / row_bytes);
  br = std::min<long>(br, (long)(SMX_PREP_MAX_TILE_BYTES / row_bytes));
  br = std::min<long>(br, 32768L * SMX_PREP_SLICE);   // (the slices are the per-gene launch's grid.y)
  br = std::min<long>(br, in->N);
  br = std::max<long>(SMX_PREP_SLICE, (br + SMX_PREP_SLICE - 1) / SMX_PREP_SLICE * SMX_PREP_SLICE);   // whole slices of the global row ids
  in->block = br;
  in->max_nnz = 0;
  if (!x) {
    SMX_CHECK(check_csr_rows(in->csr, (size_t)in->N, in->G));
    for (int64_t e = indptr[0]; e < indptr[in->N]; ++e)
      SMX_REQUIRE(cols[e] >= 0 && cols[e] < n_genes, (w + ": a CSR column outside 0 .. n_genes - 1").c_str());
    for (long r0 = 0; r0 < in->N; r0 += br)
      in->max_nnz = std::max(in->max_nnz, (size_t)(indptr[std::min(in->N, r0 + br)] - indptr[r0]));
  }
  return SMX_OK;
}

int prep_stage_alloc(DeviceScratch& buf, const PrepInput& in, PrepStage* st, bool want_tile) {
  if (want_tile) SMX_CHECK(buf.get(&st->tile, (size_t)in.block * in.ld));
  if (!in.x) {
    SMX_CHECK(buf.get(&st->ptr, (size_t)in.block + 1));
    if (want_tile) SMX_CHECK(buf.get(&st->cols, in.max_nnz));
    SMX_CHECK(buf.get(&st->vals, in.max_nnz));
  }
  return SMX_OK;
}

// rows [r0, r0 + nb) -> the tile
int prep_load_block(const PrepInput& in, const PrepStage& st, long r0, long nb) {
  if (in.x) {
    SMX_HIP(hipMemcpy2D(st.tile, (size_t)in.ld * sizeof(float), in.x + (size_t)r0 * in.G, (size_t)in.G * sizeof(float),
                        (size_t)in.G * sizeof(float), (size_t)nb, hipMemcpyHostToDevice));
    return SMX_OK;
  }
  const int64_t e0 = in.csr.indptr[r0];
  const size_t nnz = (size_t)(in.csr.indptr[r0 + nb] - e0);
  SMX_HIP(hipMemcpy(st.ptr, in.csr.indptr + r0, (size_t)(nb + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (nnz) {
    SMX_HIP(hipMemcpy(st.cols, in.csr.cols + e0, nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(st.vals, in.csr.vals + e0, nnz * sizeof(float), hipMemcpyHostToDevice));
  }
  return launch_csr_rows(nullptr, st.ptr, st.cols, st.vals, nb, in.G, in.ld, st.tile, nullptr);
}

int prep_gene_acc_alloc(DeviceScratch& buf, const PrepInput& in, GenePart* part, GeneAcc* acc) {   // (dmalloc zeroes: the accumulators start at 0)
  const size_t ld = (size_t)in.ld, max_slices = (size_t)(in.block / SMX_PREP_SLICE);
  SMX_CHECK(buf.get(&part->sum, max_slices * ld)); SMX_CHECK(buf.get(&part->sq, max_slices * ld));
  SMX_CHECK(buf.get(&part->pos, max_slices * ld)); SMX_CHECK(buf.get(&part->above, max_slices * ld));
  SMX_CHECK(buf.get(&acc->sum, ld)); SMX_CHECK(buf.get(&acc->sq, ld));
  SMX_CHECK(buf.get(&acc->pos, ld)); SMX_CHECK(buf.get(&acc->above, ld));
  return SMX_OK;
}

int prep_launch_gene_sums(const float* tile, long nb, long ld, long r0, const float* thresh, const GenePart& part, const GeneAcc& acc) {
  const int slices = (int)((nb + SMX_PREP_SLICE - 1) / SMX_PREP_SLICE);
  hipLaunchKernelGGL(prep_gene_part_kernel, dim3((unsigned)((ld / 4 + 63) / 64), (unsigned)slices), dim3(64), 0, nullptr, tile, nb, ld, r0,
                     thresh, part);
  SMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(prep_gene_combine_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, nullptr, part, slices, ld, acc);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

namespace {

int prep_launch_view(float* tile, long nb, int G, long ld, long r0, const PrepView& w) {
  const long quads = nb * (ld >> 2);
  const unsigned grid = (unsigned)std::min<long>(2048, (quads + 255) / 256);
  hipLaunchKernelGGL(prep_view_kernel, dim3(grid), dim3(256), 0, nullptr, tile, nb, G, ld, r0, w);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_prep_stats(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                   int32_t block_rows, int32_t func, const float* row_div, const uint8_t* col_mask, const float* row_thresh,
                   double* cell_total, int32_t* cell_n_genes, double* gene_sum, double* gene_sumsq, int64_t* gene_n_cells,
                   int64_t* gene_n_above) {
  PrepInput in;
  SMX_CHECK(prep_check_input("prep_stats", x, indptr, cols, vals, n_cells, n_genes, block_rows, func, row_div, &in));
  SMX_REQUIRE(cell_total && cell_n_genes && gene_sum && gene_sumsq && gene_n_cells, "prep_stats: null output");
  SMX_REQUIRE((row_thresh != nullptr) == (gene_n_above != nullptr), "prep_stats: row_thresh and gene_n_above go together");
  if (row_thresh)
    for (long i = 0; i < in.N; ++i) SMX_REQUIRE(row_thresh[i] == row_thresh[i], "prep_stats: a NaN row threshold");
  const long N = in.N, ld = in.ld;
  const int G = in.G;
  DeviceScratch buf;
  PrepStage st;
  SMX_CHECK(prep_stage_alloc(buf, in, &st, true));
  float *dDiv, *dThr; uint8_t* dMask;
  SMX_CHECK(buf.put(&dDiv, row_div, (size_t)N));
  SMX_CHECK(buf.put(&dThr, row_thresh, (size_t)N));
  SMX_CHECK(buf.put(&dMask, col_mask, (size_t)G));
  double* dTotal; int32_t* dNg;
  SMX_CHECK(buf.get(&dTotal, (size_t)N)); SMX_CHECK(buf.get(&dNg, (size_t)N));
  GenePart part; GeneAcc acc;
  SMX_CHECK(prep_gene_acc_alloc(buf, in, &part, &acc));
  const PrepView w{func, dDiv, nullptr, nullptr, 0, 0.f};
  const bool identity = func == 0 && !row_div;
  for (long r0 = 0; r0 < N; r0 += in.block) {
    const long nb = std::min(in.block, N - r0);
    SMX_CHECK(prep_load_block(in, st, r0, nb));
    if (!identity) SMX_CHECK(prep_launch_view(st.tile, nb, G, ld, r0, w));
    hipLaunchKernelGGL(prep_cell_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, nullptr, st.tile, nb, G, ld, r0, dMask, dTotal, dNg);
    SMX_HIP(hipGetLastError());
    SMX_CHECK(prep_launch_gene_sums(st.tile, nb, ld, r0, dThr, part, acc));
    SMX_HIP(hipDeviceSynchronize());   // the next block's copy overwrites the tile
  }
  SMX_HIP(hipMemcpy(cell_total, dTotal, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(cell_n_genes, dNg, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(gene_sum, acc.sum, (size_t)G * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(gene_sumsq, acc.sq, (size_t)G * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(gene_n_cells, acc.pos, (size_t)G * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (gene_n_above) SMX_HIP(hipMemcpy(gene_n_above, acc.above, (size_t)G * sizeof(int64_t), hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_prep_apply(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                   int32_t block_rows, int32_t func, const float* row_div, const float* mean, const float* sd, int32_t clip,
                   float max_value, float* out_dense, float* out_vals) {
  PrepInput in;
  SMX_CHECK(prep_check_input("prep_apply", x, indptr, cols, vals, n_cells, n_genes, block_rows, func, row_div, &in));
  SMX_REQUIRE((out_dense != nullptr) != (out_vals != nullptr), "prep_apply: exactly one of out_dense and out_vals");
  SMX_REQUIRE((mean != nullptr) == (sd != nullptr), "prep_apply: mean and std go together");
  SMX_REQUIRE(!out_vals || (!x && !mean && !clip), "prep_apply: out_vals is for CSR input without centring or clip");
  SMX_REQUIRE(!clip || max_value == max_value, "prep_apply: a NaN max_value");
  const long N = in.N, ld = in.ld;
  const int G = in.G;
  DeviceScratch buf;
  PrepStage st;
  SMX_CHECK(prep_stage_alloc(buf, in, &st, out_dense != nullptr));
  float *dDiv, *dMean, *dStd;
  SMX_CHECK(buf.put(&dDiv, row_div, (size_t)N));
  SMX_CHECK(buf.put(&dMean, mean, (size_t)G));
  SMX_CHECK(buf.put(&dStd, sd, (size_t)G));
  const PrepView w{func, dDiv, dMean, dStd, clip != 0, max_value};
  for (long r0 = 0; r0 < N; r0 += in.block) {
    const long nb = std::min(in.block, N - r0);
    if (out_dense) {
      SMX_CHECK(prep_load_block(in, st, r0, nb));
      SMX_CHECK(prep_launch_view(st.tile, nb, G, ld, r0, w));
      SMX_HIP(hipDeviceSynchronize());
      SMX_HIP(hipMemcpy2D(out_dense + (size_t)r0 * G, (size_t)G * sizeof(float), st.tile, (size_t)ld * sizeof(float),
                          (size_t)G * sizeof(float), (size_t)nb, hipMemcpyDeviceToHost));
    } else {   // the structure is unchanged: only the stored values cross, there and back
      const int64_t e0 = indptr[r0];
      const size_t nnz = (size_t)(indptr[r0 + nb] - e0);
      if (!nnz) continue;
      SMX_HIP(hipMemcpy(st.ptr, indptr + r0, (size_t)(nb + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
      SMX_HIP(hipMemcpy(st.vals, vals + e0, nnz * sizeof(float), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(prep_csr_vals_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, nullptr, st.ptr, st.vals, nb, r0, w);
      SMX_HIP(hipGetLastError());
      SMX_HIP(hipDeviceSynchronize());
      SMX_HIP(hipMemcpy(out_vals + e0, st.vals, nnz * sizeof(float), hipMemcpyDeviceToHost));
    }
  }
  return SMX_OK;
}

}  // extern "C"
