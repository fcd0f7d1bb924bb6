// smx_mbkmeans.hip -- the matrix work of scikit-learn's MiniBatchKMeans as the reference's SingleCellOMIC.clustering drives it
// (_single_cell_analysis.py:632-730: one partial_fit per batch of rows, then predict): the k-means++ seeding of the first batch, one
// mini-batch step, and the assignment of every row.  Model-free entries: they upload, compute, download and free their own buffers.  The
// random draws, the reassignment of starved centres and the bookkeeping are the host's (sisua_amd/minibatch_kmeans.py).
//   the distance sweep   ONE routine for the three entries (sweep_rows): squared distances of the rows of smx_prep.h's tile [rows][ld]
//                     float32 to centres [K][ld] float64, ld = n_genes rounded up to 4, both padded with zeros, in the direct form
//                     sum_j ((double)x_j - c_j)^2.  A wave takes MBK_ROWS = 4 consecutive rows, a workgroup of four waves 16; the lanes go
//                     over the columns, lane l the columns 256 i + 4 l .. 4 l + 3 for i = 0, 1, .. (one 16-byte load per row, two per
//                     centre), against MBK_CENTRES = 4 centres at a time: 16 float64 accumulators per lane, 16 FMAs for every 8 values
//                     loaded.  A lane adds its columns in rising order onto one accumulator per (row, centre), then the 64 lanes are summed
//                     by halving (smx_block.h): the order is a function of n_genes alone, and a zero of a CSR row is a tile entry like any
//                     other, so dense and CSR input give the same bits.  The centres are read from global memory: the four waves of a
//                     workgroup and its neighbours read the same lines at about the same time, and K x ld x 8 bytes (192 KB at the 12 x 1998
//                     of the benchmark matrix; 64 MB at the limits) sit in L2 / the Infinity Cache, not in 160 KB of LDS.
//   assignment        lane 0 of the wave keeps the smallest distance of each of its rows with `<`: ties go to the lowest centre, a NaN is
//                     never the smallest; a row whose every distance is NaN or +inf gets centre 0 and the distance +inf.
//   the centre update one wave per (256 columns, centre), as smx_group_moments: a ballot over 64 labels names the centre's rows, which are
//                     added IN ROW ORDER; then centre = (centre x count + sum) / (count + m), each operation rounded once (no FMA).
//   the seeding       per centre three launches and no host round trip: the candidates' rows as float64 centres (the first centre is the
//                     one candidate of round 0), the sweep that writes min(closest, distance) per candidate and row, and ONE workgroup
//                     that sums every candidate's potential in fixed order, keeps the lowest (ties to the lowest trial), makes its minima
//                     the new closest distances, scans them (waves scanned by shuffles, the carries added in wave order) and finds per
//                     trial the first position whose scan value is >= u x potential -- ballots in position order, no atomics.
// Every loop is bounded by the rows of a block, by ld or by K.
#include "smx_model.h"
#include "smx_prep.h"    // the block streamer of the count matrix
#include "smx_block.h"   // the fixed-order sums and the scans

#include <algorithm>
#include <cmath>
#include <vector>

namespace smx {

#define SMX_MBK_MAX_CLUSTERS 256
#define SMX_MBK_MAX_GENES 32768
#define SMX_MBK_MAX_SEED_ROWS 65536
#define SMX_MBK_MAX_TRIALS 16
#define SMX_MBK_MAX_RESIDENT ((size_t)1 << 31)   // seed and step hold their whole block in the tile: rows x ld floats (8 GB)
#define MBK_ROWS 4                               // rows of a wave
#define MBK_CENTRES 4                            // centres a wave holds at once
#define MBK_CHUNK 256                            // columns of one trip of a wave: 64 lanes x 4
#define MBK_NONE 0xFFFFFFFFu

// emit(q, row, k, d): in lane 0 of the wave, for every row r0 + q < nb of the wave and every centre k < K, k rising
template <class Emit>
__device__ __forceinline__ void sweep_rows(const float* __restrict__ tile, long nb, long ld, const double* __restrict__ C, int K, Emit emit) {
  const int lane = threadIdx.x & 63;
  const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * MBK_ROWS;
  if (r0 >= nb) return;   // (wave-uniform)
  const float* xr[MBK_ROWS];
#pragma unroll
  for (int q = 0; q < MBK_ROWS; ++q) xr[q] = tile + (r0 + q < nb ? r0 + q : nb - 1) * ld;   // (a ragged tile: the last row again, not emitted)
  for (int k0 = 0; k0 < K; k0 += MBK_CENTRES) {
    const double* cr[MBK_CENTRES];
#pragma unroll
    for (int p = 0; p < MBK_CENTRES; ++p) cr[p] = C + (long)(k0 + p < K ? k0 + p : K - 1) * ld;
    double acc[MBK_ROWS][MBK_CENTRES];
#pragma unroll
    for (int q = 0; q < MBK_ROWS; ++q)
#pragma unroll
      for (int p = 0; p < MBK_CENTRES; ++p) acc[q][p] = 0.0;
    for (long j = (long)lane * 4; j < ld; j += MBK_CHUNK) {   // (ld is a multiple of 4; the padding is zero on both sides)
      float x[MBK_ROWS][4];
#pragma unroll
      for (int q = 0; q < MBK_ROWS; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(xr[q] + j);
        x[q][0] = v.x; x[q][1] = v.y; x[q][2] = v.z; x[q][3] = v.w;
      }
#pragma unroll
      for (int p = 0; p < MBK_CENTRES; ++p) {
        const double2 c01 = *reinterpret_cast<const double2*>(cr[p] + j), c23 = *reinterpret_cast<const double2*>(cr[p] + j + 2);
        const double c[4] = {c01.x, c01.y, c23.x, c23.y};
#pragma unroll
        for (int q = 0; q < MBK_ROWS; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double d = (double)x[q][e] - c[e];
            acc[q][p] = fma(d, d, acc[q][p]);
          }
      }
    }
#pragma unroll
    for (int p = 0; p < MBK_CENTRES; ++p)
#pragma unroll
      for (int q = 0; q < MBK_ROWS; ++q) {
        const double s = halving_wave_sum(acc[q][p]);
        if (lane == 0 && r0 + q < nb && k0 + p < K) emit(q, r0 + q, k0 + p, s);
      }
  }
}

// labels (and the smallest distances, where asked) of the tile's rows; row0: the tile's first row in the output arrays
__global__ __launch_bounds__(256) void mbk_assign_kernel(const float* __restrict__ tile, long nb, long ld, const double* __restrict__ C, int K,
                                                         long row0, int32_t* __restrict__ labels, double* __restrict__ mind) {
  double best[MBK_ROWS];
  int lab[MBK_ROWS];
#pragma unroll
  for (int q = 0; q < MBK_ROWS; ++q) { best[q] = INFINITY; lab[q] = 0; }
  sweep_rows(tile, nb, ld, C, K, [&](int q, long, int k, double d) {
    if (d < best[q]) { best[q] = d; lab[q] = k; }
  });
  const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * MBK_ROWS;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int q = 0; q < MBK_ROWS; ++q)
      if (r0 + q < nb) {
        labels[row0 + r0 + q] = lab[q];
        if (mind) mind[row0 + r0 + q] = best[q];
      }
}

// the seeding: cdist [t][row] = min(closest[row], distance of the row to candidate t)
__global__ __launch_bounds__(256) void mbk_candidate_kernel(const float* __restrict__ tile, long nb, long ld, const double* __restrict__ CC, int T,
                                                            const double* __restrict__ closest, double* __restrict__ cdist) {
  sweep_rows(tile, nb, ld, CC, T, [&](int, long row, int t, double d) {
    const double c = closest[row];
    cdist[(long)t * nb + row] = d < c ? d : c;
  });
}

// the candidates' rows as float64 centres: CC [blockIdx.y][ld]
__global__ __launch_bounds__(256) void mbk_gather_kernel(const float* __restrict__ tile, long ld, const int32_t* __restrict__ cand,
                                                         double* __restrict__ CC) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j < ld) CC[(long)blockIdx.y * ld + j] = (double)tile[(long)cand[blockIdx.y] * ld + j];
}

struct SeedPick {
  int c, nc, T, n;          // the centre this round settles, its candidates, the trials of the next round, the rows
  long ld;
  const double* cdist;      // [nc][n]
  const double* CC;         // [nc][ld]
  const double* u;          // [T] of the next centre, or NULL after the last
  double* closest;          // [n]
  int32_t* cand;            // [max(nc, T)]: this round's candidates in, the next round's out
  double* centres;          // [K][ld]
  int32_t* indices;         // [K]
  double* potential;        // [K]
};

// ONE workgroup: the candidates' potentials, the best, the new closest distances; then the scan and the next candidates
__global__ __launch_bounds__(256) void mbk_pick_kernel(SeedPick a) {
  __shared__ double s4[4], pots[SMX_MBK_MAX_TRIALS], wtot[4];
  __shared__ unsigned hit[4][SMX_MBK_MAX_TRIALS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = a.n;
  for (int t = 0; t < a.nc; ++t) {
    const double p = halving_column_sum(a.cdist + (long)t * n, (long)n, s4);
    if (tid == 0) pots[t] = p;
  }
  __syncthreads();
  int best = 0;
  for (int t = 1; t < a.nc; ++t)
    if (pots[t] < pots[best]) best = t;   // (ties to the lowest trial)
  const double pot = pots[best];
  const int32_t chosen = a.cand[best];
  for (int i = tid; i < n; i += 256) a.closest[i] = a.cdist[(long)best * n + i];
  for (long j = tid; j < a.ld; j += 256) a.centres[(long)a.c * a.ld + j] = a.CC[(long)best * a.ld + j];
  if (tid == 0) { a.indices[a.c] = chosen; a.potential[a.c] = pot; }
  if (!a.u) return;
  __syncthreads();   // (every thread has read cand[best]; thread i wrote the closest[i + 256 m] it reads below)
  double tgt[SMX_MBK_MAX_TRIALS];
#pragma unroll
  for (int t = 0; t < SMX_MBK_MAX_TRIALS; ++t) tgt[t] = t < a.T ? a.u[t] * pot : 0.0;
  unsigned mine = MBK_NONE;
  double carry = 0.0;
  for (int t0 = 0; t0 < n; t0 += 256) {
    const int j = t0 + tid;
    const bool on = j < n;
    const double inc = wave_scan_add(on ? a.closest[j] : 0.0);
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    double base = carry;
    for (int q = 0; q < w; ++q) base += wtot[q];
    const double s = base + inc;
#pragma unroll
    for (int t = 0; t < SMX_MBK_MAX_TRIALS; ++t) {
      if (t < a.T) {   // (uniform)
        const unsigned long long b = __ballot(on && s >= tgt[t]);
        if (lane == 0) hit[w][t] = b ? (unsigned)(t0 + w * 64 + __ffsll(b) - 1) : MBK_NONE;
      }
    }
    carry = (((carry + wtot[0]) + wtot[1]) + wtot[2]) + wtot[3];
    __syncthreads();
    if (tid < a.T && mine == MBK_NONE)
      for (int q = 3; q >= 0; --q)
        if (hit[q][tid] != MBK_NONE) mine = hit[q][tid];   // (the first wave with a hit)
    __syncthreads();
  }
  if (tid < a.T) a.cand[tid] = mine == MBK_NONE ? n - 1 : (int32_t)mine;
}

// centre blockIdx.y, columns 4 t .. 4 t + 3 of thread t: the sum of the centre's rows in row order, then the incremental mean
__global__ __launch_bounds__(64) void mbk_update_kernel(const float* __restrict__ tile, long nb, long ld, const int32_t* __restrict__ labels,
                                                        double* __restrict__ C, const double* __restrict__ cnt_in, double* __restrict__ cnt_out) {
  const int lane = threadIdx.x, k = blockIdx.y;
  const long g = ((long)blockIdx.x * 64 + lane) * 4;
  const bool live = g < ld;   // (a dead lane still reads labels and votes)
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  long m = 0;
  for (long t0 = 0; t0 < nb; t0 += 64) {
    const long r = t0 + lane;
    unsigned long long mask = __ballot(r < nb && labels[r] == k);
    m += __popcll(mask);
    while (mask) {   // (wave-uniform) the next four rows of the centre: loads first, then the sums in row order
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
          s[0] += (double)v[u].x; s[1] += (double)v[u].y; s[2] += (double)v[u].z; s[3] += (double)v[u].w;
        }
    }
  }
  const double cnt = cnt_in[k];
  if (live && m > 0) {
    double* c = C + (long)k * ld + g;
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = __ddiv_rn(__dadd_rn(__dmul_rn(c[q], cnt), s[q]), cnt + (double)m);
  }
  if (blockIdx.x == 0 && lane == 0) cnt_out[k] = cnt + (double)m;
}

__global__ __launch_bounds__(256) void mbk_sum_kernel(const double* __restrict__ v, long n, double* __restrict__ out) {
  __shared__ double s4[4];
  const double s = halving_column_sum(v, n, s4);
  if (threadIdx.x == 0) *out = s;
}

namespace {

// the checks the three entries share; the centres' shape
int mbk_check(const char* who, const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
              int32_t block_rows, int32_t n_clusters, PrepInput* in) {
  const std::string w(who);
  SMX_CHECK(prep_check_input(who, x, indptr, cols, vals, n_rows, n_genes, block_rows, 0, nullptr, in));
  SMX_REQUIRE(n_genes <= SMX_MBK_MAX_GENES, (w + ": 1 <= n_genes <= 32768").c_str());
  SMX_REQUIRE(n_clusters >= 2 && n_clusters <= SMX_MBK_MAX_CLUSTERS, (w + ": 2 <= n_clusters <= 256").c_str());
  return SMX_OK;
}

// seed and step hold all their rows in the tile at once
int mbk_resident(const char* who, PrepInput* in) {
  const std::string w(who);
  in->block = (in->N + SMX_PREP_SLICE - 1) / SMX_PREP_SLICE * SMX_PREP_SLICE;
  SMX_REQUIRE((size_t)in->block * (size_t)in->ld <= SMX_MBK_MAX_RESIDENT, (w + ": rows x n_genes <= 2^31 (the block is held whole)").c_str());
  if (!in->x) in->max_nnz = (size_t)(in->csr.indptr[in->N] - in->csr.indptr[0]);
  return SMX_OK;
}

int mbk_put_centres(DeviceScratch& buf, const double* centres, int K, const PrepInput& in, double** d) {
  SMX_CHECK(buf.get(d, (size_t)K * in.ld));   // (dmalloc zeroes: the padding)
  if (centres)
    SMX_HIP(hipMemcpy2D(*d, (size_t)in.ld * 8, centres, (size_t)in.G * 8, (size_t)in.G * 8, (size_t)K, hipMemcpyHostToDevice));
  return SMX_OK;
}

unsigned mbk_grid(long nb) { return (unsigned)((nb + 4 * MBK_ROWS - 1) / (4 * MBK_ROWS)); }

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_mbkmeans_seed(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                      int32_t n_clusters, int32_t n_trials, int64_t first, const double* u, int32_t* indices, double* centres,
                      double* potential) {
  PrepInput in;
  SMX_CHECK(mbk_check("mbkmeans_seed", x, indptr, cols, vals, n_rows, n_genes, 0, n_clusters, &in));
  SMX_REQUIRE(u && indices && centres && potential, "mbkmeans_seed: null u or output");
  SMX_REQUIRE(n_rows >= n_clusters && n_rows <= SMX_MBK_MAX_SEED_ROWS, "mbkmeans_seed: n_clusters <= n_rows <= 65536");
  SMX_REQUIRE(n_trials >= 1 && n_trials <= SMX_MBK_MAX_TRIALS, "mbkmeans_seed: 1 <= n_trials <= 16");
  SMX_REQUIRE(first >= 0 && first < n_rows, "mbkmeans_seed: first is a row of the block");
  const int K = n_clusters, T = n_trials;
  for (long i = 0; i < (long)(K - 1) * T; ++i) SMX_REQUIRE(u[i] >= 0.0 && u[i] < 1.0, "mbkmeans_seed: u outside [0, 1)");
  SMX_CHECK(mbk_resident("mbkmeans_seed", &in));
  const long n = in.N, ld = in.ld;
  DeviceScratch buf;
  PrepStage st;
  SMX_CHECK(prep_stage_alloc(buf, in, &st, true));
  double *dCC, *dCent, *dCdist, *dClosest, *dPot, *dU;
  int32_t *dCand, *dIdx;
  SMX_CHECK(buf.get(&dCC, (size_t)T * ld));
  SMX_CHECK(mbk_put_centres(buf, nullptr, K, in, &dCent));
  SMX_CHECK(buf.get(&dCdist, (size_t)T * n));
  SMX_CHECK(buf.get(&dPot, (size_t)K));
  SMX_CHECK(buf.get(&dIdx, (size_t)K));
  SMX_CHECK(buf.put(&dU, u, (size_t)(K - 1) * T));
  std::vector<double> inf((size_t)n, INFINITY);
  std::vector<int32_t> cand0((size_t)SMX_MBK_MAX_TRIALS, (int32_t)first);
  SMX_CHECK(buf.put(&dClosest, (const double*)inf.data(), (size_t)n));
  SMX_CHECK(buf.put(&dCand, (const int32_t*)cand0.data(), cand0.size()));
  SMX_CHECK(prep_load_block(in, st, 0, n));
  for (int c = 0; c < K; ++c) {   // (stream order; no host round trip)
    const int nc = c == 0 ? 1 : T;
    hipLaunchKernelGGL(mbk_gather_kernel, dim3((unsigned)((ld + 255) / 256), (unsigned)nc), dim3(256), 0, nullptr, st.tile, ld, dCand, dCC);
    hipLaunchKernelGGL(mbk_candidate_kernel, dim3(mbk_grid(n)), dim3(256), 0, nullptr, st.tile, n, ld, dCC, nc, dClosest, dCdist);
    SeedPick a;
    a.c = c; a.nc = nc; a.T = T; a.n = (int)n; a.ld = ld; a.cdist = dCdist; a.CC = dCC; a.u = c + 1 < K ? dU + (size_t)c * T : nullptr;
    a.closest = dClosest; a.cand = dCand; a.centres = dCent; a.indices = dIdx; a.potential = dPot;
    hipLaunchKernelGGL(mbk_pick_kernel, dim3(1), dim3(256), 0, nullptr, a);
    SMX_HIP(hipGetLastError());
  }
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(indices, dIdx, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(potential, dPot, (size_t)K * 8, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy2D(centres, (size_t)in.G * 8, dCent, (size_t)ld * 8, (size_t)in.G * 8, (size_t)K, hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_mbkmeans_step(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                      int32_t n_clusters, double* centres, double* counts, int32_t* labels, double* inertia) {
  PrepInput in;
  SMX_CHECK(mbk_check("mbkmeans_step", x, indptr, cols, vals, n_rows, n_genes, 0, n_clusters, &in));
  SMX_REQUIRE(centres && counts && inertia, "mbkmeans_step: null centres, counts or inertia");
  const int K = n_clusters;
  for (int k = 0; k < K; ++k) SMX_REQUIRE(counts[k] >= 0.0 && std::isfinite(counts[k]), "mbkmeans_step: a count that is negative or not finite");
  SMX_CHECK(mbk_resident("mbkmeans_step", &in));
  const long n = in.N, ld = in.ld;
  DeviceScratch buf;
  PrepStage st;
  SMX_CHECK(prep_stage_alloc(buf, in, &st, true));
  double *dCent, *dCnt, *dCntNew, *dMind, *dInertia;
  int32_t* dLab;
  SMX_CHECK(mbk_put_centres(buf, centres, K, in, &dCent));
  SMX_CHECK(buf.put(&dCnt, (const double*)counts, (size_t)K));
  SMX_CHECK(buf.get(&dCntNew, (size_t)K));
  SMX_CHECK(buf.get(&dMind, (size_t)n));
  SMX_CHECK(buf.get(&dInertia, (size_t)1));
  SMX_CHECK(buf.get(&dLab, (size_t)n));
  SMX_CHECK(prep_load_block(in, st, 0, n));
  hipLaunchKernelGGL(mbk_assign_kernel, dim3(mbk_grid(n)), dim3(256), 0, nullptr, st.tile, n, ld, dCent, K, 0L, dLab, dMind);
  hipLaunchKernelGGL(mbk_sum_kernel, dim3(1), dim3(256), 0, nullptr, dMind, n, dInertia);
  hipLaunchKernelGGL(mbk_update_kernel, dim3((unsigned)((ld / 4 + 63) / 64), (unsigned)K), dim3(64), 0, nullptr, st.tile, n, ld, dLab, dCent, dCnt,
                     dCntNew);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy2D(centres, (size_t)in.G * 8, dCent, (size_t)ld * 8, (size_t)in.G * 8, (size_t)K, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(counts, dCntNew, (size_t)K * 8, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(inertia, dInertia, 8, hipMemcpyDeviceToHost));
  if (labels) SMX_HIP(hipMemcpy(labels, dLab, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_mbkmeans_predict(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                         int32_t block_rows, int32_t n_clusters, const double* centres, int32_t* labels, double* distance) {
  PrepInput in;
  SMX_CHECK(mbk_check("mbkmeans_predict", x, indptr, cols, vals, n_rows, n_genes, block_rows, n_clusters, &in));
  SMX_REQUIRE(centres && labels, "mbkmeans_predict: null centres or labels");
  const long N = in.N, ld = in.ld;
  const int K = n_clusters;
  DeviceScratch buf;
  PrepStage st;
  SMX_CHECK(prep_stage_alloc(buf, in, &st, true));
  double *dCent, *dMind = nullptr;
  int32_t* dLab;
  SMX_CHECK(mbk_put_centres(buf, centres, K, in, &dCent));
  SMX_CHECK(buf.get(&dLab, (size_t)N));
  if (distance) SMX_CHECK(buf.get(&dMind, (size_t)N));
  for (long r0 = 0; r0 < N; r0 += in.block) {
    const long nb = std::min(in.block, N - r0);
    SMX_CHECK(prep_load_block(in, st, r0, nb));
    hipLaunchKernelGGL(mbk_assign_kernel, dim3(mbk_grid(nb)), dim3(256), 0, nullptr, st.tile, nb, ld, dCent, K, r0, dLab, dMind);
    SMX_HIP(hipGetLastError());
    SMX_HIP(hipDeviceSynchronize());   // the next block's copy overwrites the tile
  }
  SMX_HIP(hipMemcpy(labels, dLab, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (distance) SMX_HIP(hipMemcpy(distance, dMind, (size_t)N * 8, hipMemcpyDeviceToHost));
  return SMX_OK;
}

}  // extern "C"
