// smx_umap.hip -- the layout optimisation of UMAP (the reference scatters umap-learn's / cuML's 2-D embedding of the latent means or of an
// omic: sisua/data/_single_cell_analysis.py dimension_reduce(algo='umap')), in its PER-EPOCH form: every force of an epoch is taken from
// the positions at the epoch's start and then applied (cuML's reproducible mode), all in float64; the definitions are in
// include/sisua_hip.h.  Model-free entry: it uploads, computes, downloads and frees its own buffers.  The graph (kNN, connectivities,
// the cut at max / n_epochs, epochs_per_sample, a and b, the start) is prepared on the host (sisua_amd/neighbors.py).
//   epoch launch   sixteen lanes per cell, as tsne_row_kernel (a row of more than 64 entries: the 256 lanes of a workgroup of its own, the
//                  same code with chunks of 256): the row is walked in chunks of 16 entries.  Lane l owns entry 16 c + l of the
//                  row: it alone reads and writes the entry's two schedule doubles, decides whether the entry is active, adds its
//                  attraction and leaves its number of negatives m in LDS.  The per-epoch form makes the negatives of an entry
//                  independent of one another, so the chunk's negatives are numbered q = 0, 1, .. through its entries and lane l takes
//                  q = l, l + 16, ...: a weak entry that draws hundreds of negatives in its one active epoch is spread over the lanes
//                  instead of being one lane's serial tail.  The lanes are added by halving and lane 0 writes y_j + alpha x sum to
//                  the OTHER copy of Y.  A cell's epoch is a chain of dependent gathers, so the schedule words of the chunk ahead
//                  are loaded while the chunk in hand is worked on, and a lane's negatives are taken four at a time: four draws,
//                  four gathers in flight together, four terms, added in the order of q.
// The chunk loop runs to the longest row of the WAVE (a lane past its row holds m = 0), so every LDS hand-over and every shuffle is in
// wave-uniform control flow: no thread leaves before them.  No float atomics; no workgroup waits on another; every loop is bounded by
// the row, by 16 x negative_sample_rate x n_epochs or by n_epochs.
#include "smx_model.h"
#include "smx_dist.h"    // SMX_CL_TILE
#include "smx_block.h"   // wave_lds_sync

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace smx {

#define SMX_UMAP_LANES 16        // lanes that share one cell
#define SMX_UMAP_LONG 64         // a row of more entries is taken by a whole workgroup
#define SMX_UMAP_UNROLL 4        // negatives of a lane whose gathers are in flight together
#define SMX_UMAP_MAX_EPOCHS 10000
#define SMX_UMAP_MAX_NEG 64      // negative_sample_rate
enum { ST_UMAP_NEG = 100 };      // Philox stream of the negative samples (counter: entry, epoch, p >> 2, stream)

struct UmapEpoch {
  int n;                 // the epoch
  int S;                 // negative_sample_rate
  double m_max;          // S x n_epochs
  double alpha;          // initial_alpha x (1 - n / n_epochs)
  double a, b;
  double c_att, c_rep;   // (-2 a) b and (2 gamma) b
  uint32_t k0, k1;       // seed lo / hi
};

__device__ inline double umap_clip(double x) { return x > 4.0 ? 4.0 : (x < -4.0 ? -4.0 : x); }

// d = yj - yk and d2 = |d|^2, the components added in order; every operation rounded
template <int C>
__device__ inline double umap_d2(const double (&yj)[C], const double* yk, double (&d)[C]) {   // (yk: global memory or registers)
#pragma clang fp contract(off)
  d[0] = yj[0] - yk[0];
  double s = d[0] * d[0];
#pragma unroll
  for (int c = 1; c < C; ++c) {
    d[c] = yj[c] - yk[c];
    s = s + d[c] * d[c];
  }
  return s;
}

// one cell by LANES lanes (16: sixteen cells per workgroup, the cell's lanes in one wave; 256: the whole workgroup for one long row).
// j < 0: no cell (the lanes still take part in every hand-over)
template <int C, int LANES>
__device__ inline void umap_cell(const int64_t* indptr, const int32_t* cols, const double* eps, long N, const double* Yin, double* Yout,
                                 double* next, double* next_neg, const UmapEpoch& ep, long j, int* sh_m, double* sh4) {
#pragma clang fp contract(off)   // (the schedule is umap-learn's, decided on rounded float64 operations: bit-equal to the restatement)
  const int lane = threadIdx.x % LANES;
  const int gb = threadIdx.x - lane;   // the cell's LANES words of sh_m
  const bool live = j >= 0;            // (no thread leaves before the shuffles)
  const int64_t e0 = live ? indptr[j] : 0, e1 = live ? indptr[j + 1] : 0;
  double yj[C], acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { yj[c] = live ? Yin[j * C + c] : 0.0; acc[c] = 0.0; }
  int chunks = (int)((e1 - e0 + LANES - 1) / LANES);   // (a row holds fewer than n_cells < 2^31 entries)
  if (LANES < 64)
    for (int o = 32; o > 0; o >>= 1) chunks = max(chunks, __shfl_xor(chunks, o, 64));   // the wave's longest row
  const double dn = (double)ep.n;
  // the lane's entry of the chunk ahead: its four words are in flight while the chunk in hand is worked on (a dependent gather costs
  // microseconds at one wave per SIMD, and a cell's epoch is a chain of them)
  double nx_a = 0.0, es_a = 0.0, nn_a = 0.0;
  int col_a = 0;
  if (e0 + lane < e1) { nx_a = next[e0 + lane]; es_a = eps[e0 + lane]; nn_a = next_neg[e0 + lane]; col_a = cols[e0 + lane]; }
  for (int ch = 0; ch < chunks; ++ch) {
    const int64_t cb = e0 + (int64_t)ch * LANES;   // the chunk's first entry
    const int64_t e = cb + lane;
    const double nx = nx_a, es = es_a, nn = nn_a;
    const int col = col_a;
    if (e + LANES < e1) {
      const int64_t ea = e + LANES;
      nx_a = next[ea]; es_a = eps[ea]; nn_a = next_neg[ea]; col_a = cols[ea];
    }
    int m = 0;
    if (e < e1 && nx <= dn) {   // active
      double d[C];
      const double d2 = umap_d2<C>(yj, Yin + (long)col * C, d);
      if (d2 > 0.0) {
        const double pb = pow(d2, ep.b);
        const double g = (ep.c_att * (pb / d2)) / (ep.a * pb + 1.0);
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = acc[c] + 2.0 * umap_clip(g * d[c]);
      }
      if (ep.S > 0) {
        const double en = es / (double)ep.S;
        double md = trunc((dn - nn) / en);
        md = md > 0.0 ? md : 0.0;            // (also a NaN)
        md = md < ep.m_max ? md : ep.m_max;
        m = (int)md;
        next_neg[e] = nn + md * en;
      }
      next[e] = nx + es;
    }
    sh_m[threadIdx.x] = m;
    if (LANES < 64) wave_lds_sync(); else __syncthreads();
    int M = 0;   // the chunk's negatives: at most 256 x 64 x 10000
#pragma unroll 16
    for (int t = 0; t < LANES; ++t) M += sh_m[gb + t];
    int t = 0, cum = 0, mt = sh_m[gb];   // negatives [cum, cum + mt) are entry t's
    // four of the lane's negatives at a time: the four draws, then the four gathers in flight together, then the four terms -- added in
    // the order q = l, l + LANES, l + 2 LANES, ... all the same
    for (int q0 = lane; q0 < M; q0 += SMX_UMAP_UNROLL * LANES) {
      double yk[SMX_UMAP_UNROLL][C];
      bool on[SMX_UMAP_UNROLL];
#pragma unroll
      for (int u = 0; u < SMX_UMAP_UNROLL; ++u) {
        const int q = q0 + u * LANES;
        on[u] = q < M;
        long k = 0;
        if (on[u]) {
          while (q >= cum + mt) { cum += mt; ++t; mt = sh_m[gb + t]; }   // (q < M: t stays below LANES)
          const uint32_t p = (uint32_t)(q - cum);
          const U4 w = philox4x32_10((uint32_t)(cb + t), (uint32_t)ep.n, p >> 2, (uint32_t)ST_UMAP_NEG, ep.k0, ep.k1);
          const uint32_t sel = p & 3u;
          const uint32_t r = sel == 0u ? w.x : (sel == 1u ? w.y : (sel == 2u ? w.z : w.w));
          k = (long)(r % (uint32_t)N);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) yk[u][c] = on[u] ? Yin[k * C + c] : yj[c];
      }
#pragma unroll
      for (int u = 0; u < SMX_UMAP_UNROLL; ++u) {
        double d[C];
        const double d2 = umap_d2<C>(yj, yk[u], d);
        if (on[u] && d2 > 0.0) {
          const double pb = pow(d2, ep.b);
          const double g = ep.c_rep / ((0.001 + d2) * (ep.a * pb + 1.0));
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = acc[c] + umap_clip(g * d[c]);
        }
      }
    }
    if (LANES < 64) wave_lds_sync(); else __syncthreads();   // (every read of sh_m is done before the next chunk writes it)
  }
  if (LANES < 64) {
    for (int o = LANES / 2; o > 0; o >>= 1) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += __shfl_down(acc[c], o, LANES);
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = halving_block_sum(acc[c], sh4);   // the lanes of a wave by halving, then (0 + 1) + (2 + 3)
  }
  if (!live || lane != 0) return;
#pragma unroll
  for (int c = 0; c < C; ++c) Yout[j * C + c] = yj[c] + ep.alpha * acc[c];
}

// workgroups 0 .. tiles16 - 1: sixteen cells each, sixteen lanes per cell, the rows of at most SMX_UMAP_LONG entries; then one workgroup
// per longer row (long_ids, ascending): a hub of a kNN graph holds hundreds of entries, and walked sixteen at a time it was the tail
// that every epoch waited for
template <int C>
__global__ __launch_bounds__(SMX_CL_TILE) void umap_epoch_kernel(const int64_t* indptr, const int32_t* cols, const double* eps, long N,
                                                                 const double* Yin, double* Yout, double* next, double* next_neg,
                                                                 const int32_t* long_ids, unsigned tiles16, UmapEpoch ep) {
  __shared__ int sh_m[SMX_CL_TILE];
  __shared__ double sh4[4];
  if (blockIdx.x < tiles16) {
    long j = ((long)blockIdx.x * SMX_CL_TILE + threadIdx.x) / SMX_UMAP_LANES;
    if (j >= N || indptr[j + 1] - indptr[j] > SMX_UMAP_LONG) j = -1;
    umap_cell<C, SMX_UMAP_LANES>(indptr, cols, eps, N, Yin, Yout, next, next_neg, ep, j, sh_m, sh4);
  } else {
    umap_cell<C, SMX_CL_TILE>(indptr, cols, eps, N, Yin, Yout, next, next_neg, ep, (long)long_ids[blockIdx.x - tiles16], sh_m, sh4);
  }
}

__global__ __launch_bounds__(SMX_CL_TILE) void umap_pow_kernel(const double* x, double b, long n, double* out) {
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  if (i < n) out[i] = pow(x[i], b);
}

}  // namespace smx

using namespace smx;

extern "C" {

int smx_umap_layout(const int64_t* indptr, const int32_t* cols, const double* epochs_per_sample, int64_t n_cells, int32_t n_components,
                    const double* Y0, int32_t n_epochs, int32_t epoch_begin, int32_t epoch_end, double a, double b, double gamma,
                    double initial_alpha, int32_t negative_sample_rate, uint64_t seed, double* next_sample, double* next_negative, double* Y) {
  SMX_REQUIRE(indptr && Y0 && next_sample && next_negative && Y, "umap_layout: null argument");
  SMX_REQUIRE(n_cells >= 2 && n_cells < ((int64_t)1 << 31), "umap_layout: 2 <= n_cells < 2^31");
  SMX_REQUIRE(n_components >= 1 && n_components <= 3, "umap_layout: 1 <= n_components <= 3");
  SMX_REQUIRE(n_epochs >= 1 && n_epochs <= SMX_UMAP_MAX_EPOCHS, "umap_layout: 1 <= n_epochs <= 10000");
  SMX_REQUIRE(epoch_begin >= 0 && epoch_begin <= epoch_end && epoch_end <= n_epochs, "umap_layout: 0 <= epoch_begin <= epoch_end <= n_epochs");
  SMX_REQUIRE(negative_sample_rate >= 0 && negative_sample_rate <= SMX_UMAP_MAX_NEG, "umap_layout: 0 <= negative_sample_rate <= 64");
  SMX_REQUIRE(std::isfinite(a) && a >= 0.0 && std::isfinite(b) && b >= 0.0 && std::isfinite(gamma) && gamma >= 0.0,
              "umap_layout: a, b and gamma must be finite and >= 0");
  SMX_REQUIRE(std::isfinite(initial_alpha), "umap_layout: initial_alpha must be finite");
  SMX_REQUIRE(indptr[0] == 0, "umap_layout: indptr[0] must be 0");
  const long N = (long)n_cells;
  const int C = n_components;
  for (int64_t i = 0; i < n_cells; ++i)
    SMX_REQUIRE(indptr[i + 1] >= indptr[i] && indptr[i + 1] - indptr[i] < n_cells && indptr[i + 1] < ((int64_t)1 << 31),
                "umap_layout: indptr must not decrease, a row holds fewer than n_cells entries, and there are at most 2^31 - 1 entries");
  const size_t nnz = (size_t)indptr[N];
  SMX_REQUIRE(nnz == 0 || (cols && epochs_per_sample), "umap_layout: null argument");
  for (int64_t i = 0; i < n_cells; ++i) {
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
      SMX_REQUIRE(cols[e] >= 0 && (int64_t)cols[e] < n_cells, "umap_layout: a column outside 0 .. n_cells - 1");
      SMX_REQUIRE(cols[e] != i, "umap_layout: an entry on the diagonal");
      SMX_REQUIRE(e == indptr[i] || cols[e] > cols[e - 1], "umap_layout: the columns of a row must increase strictly");
      SMX_REQUIRE(std::isfinite(epochs_per_sample[e]) && epochs_per_sample[e] > 0.0, "umap_layout: an epochs_per_sample that is not finite and positive");
      SMX_REQUIRE(std::isfinite(next_sample[e]) && std::isfinite(next_negative[e]), "umap_layout: a schedule entry that is not finite");
    }
  }
  const size_t NC = (size_t)N * C;
  for (size_t e = 0; e < NC; ++e) SMX_REQUIRE(std::isfinite(Y0[e]), "umap_layout: an entry of Y0 that is not finite");

  DeviceScratch buf;
  int64_t* dIndptr;
  int32_t* dCols;
  double *dEps, *dNext, *dNeg, *dYa, *dYb;
  SMX_CHECK(buf.put(&dIndptr, indptr, (size_t)N + 1));
  if (nnz) {
    SMX_CHECK(buf.put(&dCols, cols, nnz)); SMX_CHECK(buf.put(&dEps, epochs_per_sample, nnz));
    SMX_CHECK(buf.put(&dNext, (const double*)next_sample, nnz)); SMX_CHECK(buf.put(&dNeg, (const double*)next_negative, nnz));
  } else {   // (an empty graph: nothing moves)
    SMX_CHECK(buf.get(&dCols, (size_t)1)); SMX_CHECK(buf.get(&dEps, (size_t)1));
    SMX_CHECK(buf.get(&dNext, (size_t)1)); SMX_CHECK(buf.get(&dNeg, (size_t)1));
  }
  SMX_CHECK(buf.put(&dYa, Y0, NC)); SMX_CHECK(buf.get(&dYb, NC));
  std::vector<int32_t> long_ids;   // the rows a whole workgroup takes
  for (int64_t i = 0; i < n_cells; ++i)
    if (indptr[i + 1] - indptr[i] > SMX_UMAP_LONG) long_ids.push_back((int32_t)i);
  int32_t* dLong;
  if (long_ids.empty()) SMX_CHECK(buf.get(&dLong, (size_t)1));
  else SMX_CHECK(buf.put(&dLong, (const int32_t*)long_ids.data(), long_ids.size()));
  UmapEpoch ep;
  ep.S = negative_sample_rate;
  ep.m_max = (double)negative_sample_rate * (double)n_epochs;
  ep.a = a; ep.b = b;
  ep.c_att = (-2.0 * a) * b;
  ep.c_rep = (2.0 * gamma) * b;
  ep.k0 = (uint32_t)(seed & 0xFFFFFFFFull); ep.k1 = (uint32_t)(seed >> 32);
  const unsigned tiles = (unsigned)(((size_t)N * SMX_UMAP_LANES + SMX_CL_TILE - 1) / SMX_CL_TILE);
  const dim3 grid(tiles + (unsigned)long_ids.size()), block(SMX_CL_TILE);
  for (int n = epoch_begin; n < epoch_end; ++n) {
    const double frac = (double)n / (double)n_epochs;
    const double rest = 1.0 - frac;
    ep.n = n;
    ep.alpha = initial_alpha * rest;
    switch (C) {
      case 1: hipLaunchKernelGGL(umap_epoch_kernel<1>, grid, block, 0, nullptr, dIndptr, dCols, dEps, N, dYa, dYb, dNext, dNeg, dLong, tiles, ep); break;
      case 2: hipLaunchKernelGGL(umap_epoch_kernel<2>, grid, block, 0, nullptr, dIndptr, dCols, dEps, N, dYa, dYb, dNext, dNeg, dLong, tiles, ep); break;
      default: hipLaunchKernelGGL(umap_epoch_kernel<3>, grid, block, 0, nullptr, dIndptr, dCols, dEps, N, dYa, dYb, dNext, dNeg, dLong, tiles, ep); break;
    }
    SMX_HIP(hipGetLastError());
    std::swap(dYa, dYb);   // dYa: the current embedding
  }
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(Y, dYa, NC * sizeof(double), hipMemcpyDeviceToHost));
  if (nnz) {
    SMX_HIP(hipMemcpy(next_sample, dNext, nnz * sizeof(double), hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy(next_negative, dNeg, nnz * sizeof(double), hipMemcpyDeviceToHost));
  }
  return SMX_OK;
}

int smx_umap_pow(const double* x, double b, int64_t n, double* out) {
  SMX_REQUIRE(x && out && n >= 1 && n < ((int64_t)1 << 31), "umap_pow: null argument or n outside 1 .. 2^31 - 1");
  SMX_REQUIRE(std::isfinite(b), "umap_pow: b must be finite");
  for (int64_t i = 0; i < n; ++i) SMX_REQUIRE(std::isfinite(x[i]) && x[i] > 0.0, "umap_pow: x must be finite and positive");
  DeviceScratch buf;
  double *dX, *dOut;
  SMX_CHECK(buf.put(&dX, x, (size_t)n)); SMX_CHECK(buf.get(&dOut, (size_t)n));
  hipLaunchKernelGGL(umap_pow_kernel, dim3((unsigned)((n + SMX_CL_TILE - 1) / SMX_CL_TILE)), dim3(SMX_CL_TILE), 0, nullptr, dX, b, (long)n, dOut);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(out, dOut, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return SMX_OK;
}

}  // extern "C"
