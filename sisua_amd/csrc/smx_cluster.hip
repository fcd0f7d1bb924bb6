// smx_cluster.hip -- the two dense parts of the reference's clustering scores of a latent space (sisua/analysis/latent_benchmarks.py:69-117:
// silhouette_score on the true labels, KMeans(n_labels, n_init=200) for the predicted ones), on host arrays Z [N][D] float32.  Model-free
// entries: they upload, compute, download and free their own buffers.  Everything is float64 and in the DIRECT form sum_d (x[d] - y[d])^2:
// no Gram form, no MFMA (the cancellation of |x|^2 + |y|^2 - 2 x.y for near neighbours is what this file exists to avoid).
//   silhouette sums   the host orders the cells by class (stable), so a class is a contiguous range of j.  One workgroup per (tile of 256 cells
//                     i, slice of the j range): z_i sits in registers, tiles of z_j pass through LDS as float64 and every lane reads the same
//                     address (a broadcast); a thread walks j in order with ONE running sum that is closed at each class boundary into
//                     part [slice][class][i].  The number of slices is a function of N alone.  A second launch adds the slices in index order
//                     and forms a (own class, / (n_c - 1)) and b (the smallest mean over the other non-empty classes; NaN is kept).
//   k-means           all restarts together, the restart on the grid's y axis through a list of the restarts still running.  Assignment: one
//                     thread per cell, the restart's centres pass through LDS in chunks, strict < keeps the lowest index among ties; the
//                     changed labels are counted with one integer atomic per workgroup.  Update: one workgroup per (restart, cluster) scans the
//                     labels; lanes = dimensions, 256 / lanes contiguous segments of cells summed in order and then added in segment order.
//                     An empty cluster keeps its centre.  The host reads the changed counts between launches and drops converged restarts.
// No float atomics; every loop is bounded by N, K, D or max_iter; no workgroup waits on another.  The order of every sum is a function of
// (N, D, the labels) alone, so two calls give the same bits and a restart gives the same bits alone or in a batch.
// Non-finite input: an infinity is read as NaN, so the sums it touches are NaN (never inf - inf by accident of order); a NaN distance is
// never the smallest, so a NaN cell is assigned to centre 0.
#include "smx_model.h"
#include "smx_dist.h"   // sqdist, stage_rows, load_cell, nan_if_inf: shared with smx_knn.hip
#include "smx_block.h"  // the fixed-order column sum

#include <algorithm>
#include <cmath>
#include <numeric>

namespace smx {

// ---- silhouette ------------------------------------------------------------------------------------------------------------------
// Z: the cells in class order; off [K + 1]: where each class starts.  part [n_slices][K][N], zero on entry: a slice writes only the classes
// its j range meets.
template <int DP>
__global__ __launch_bounds__(SMX_CL_TILE) void silhouette_part_kernel(const float* Z, long N, int D, const int32_t* off, int K, long slice_len,
                                                                      double* part) {
  constexpr int TJ = SMX_CL_LDS_DOUBLES / DP;
  __shared__ double sh[SMX_CL_LDS_DOUBLES];
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  const long j0 = (long)blockIdx.y * slice_len, j1 = min(N, j0 + slice_len);
  if (j0 >= j1) return;   // (block-uniform)
  float zi[DP];
  load_cell<DP>(zi, Z, i, N, D);
  int c = 0;
  while (c < K - 1 && (long)off[c + 1] <= j0) ++c;   // the class of j0 (empty classes are passed over); bounded by K
  long c_end = off[c + 1];
  double acc = 0.0;
  double* out = part + (long)blockIdx.y * K * N + i;
  for (long jt = j0; jt < j1; jt += TJ) {
    const int nj = (int)min((long)TJ, j1 - jt);
    __syncthreads();
    stage_rows<DP>(sh, Z, jt, nj, D);
    __syncthreads();
    for (int jj = 0; jj < nj; ++jj) {
      if (jt + jj >= c_end) {   // (block-uniform) a class boundary: close the running sum
        if (i < N) out[(long)c * N] = acc;
        acc = 0.0;
        do { ++c; c_end = off[c + 1]; } while (c < K - 1 && c_end <= jt + jj);
      }
      acc += sqrt(sqdist<DP>(zi, sh + jj * DP));
    }
  }
  if (i < N) out[(long)c * N] = acc;
}

// a, b of the cell at sorted position i (class cls[i]); the slices are added in index order
__global__ __launch_bounds__(SMX_CL_TILE) void silhouette_finish_kernel(const double* part, int n_slices, long N, const int32_t* off, int K,
                                                                        const int32_t* cls, double* a, double* b) {
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  if (i >= N) return;
  const int own = cls[i];
  double av = 0.0, bv = INFINITY;
  for (int c = 0; c < K; ++c) {
    const int n_c = off[c + 1] - off[c];
    if (n_c == 0) continue;
    double tot = 0.0;
    for (int s = 0; s < n_slices; ++s) tot += part[((long)s * K + c) * N + i];
    if (c == own) av = n_c > 1 ? tot / (double)(n_c - 1) : 0.0;
    else {
      const double v = tot / (double)n_c;
      if (v < bv || v != v) bv = v;   // (a NaN stays: nothing compares below it and no later value replaces it)
    }
  }
  a[i] = av; b[i] = bv;
}

// ---- k-means ---------------------------------------------------------------------------------------------------------------------
struct AssignArgs {
  const float* Z; long N; int D, K;
  const int32_t* active;   // the restarts of this launch (grid y)
  const double* centres;   // [R][K][D]
  int32_t* labels;         // [R][N]
  double* mind2;           // [R][N]
  int32_t* changed;        // [R], zero on entry
};

template <int DP>
__global__ __launch_bounds__(SMX_CL_TILE) void kmeans_assign_kernel(AssignArgs a) {
  constexpr int KC = SMX_CL_LDS_DOUBLES / DP;
  __shared__ double sh[SMX_CL_LDS_DOUBLES];
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  const long r = a.active[blockIdx.y];
  float zi[DP];
  load_cell<DP>(zi, a.Z, i, a.N, a.D);
  int best = 0;
  double best_d = INFINITY;
  for (int k0 = 0; k0 < a.K; k0 += KC) {
    const int nk = min(KC, a.K - k0);
    __syncthreads();
    stage_rows<DP>(sh, a.centres + r * a.K * a.D, (long)k0, nk, a.D);
    __syncthreads();
    for (int kk = 0; kk < nk; ++kk) {
      const double d2 = sqdist<DP>(zi, sh + kk * DP);
      if (d2 < best_d) { best_d = d2; best = k0 + kk; }
    }
  }
  int moved = 0;
  if (i < a.N) {
    int32_t* lab = a.labels + r * a.N + i;
    moved = *lab != best;
    *lab = best;
    a.mind2[r * a.N + i] = best_d;
  }
  const int n_moved = __syncthreads_count(moved);
  if (threadIdx.x == 0 && n_moved) atomicAdd(a.changed + r, n_moved);
}

struct UpdateArgs {
  const float* Z; long N; int D, K;
  const int32_t* active;
  const int32_t* labels;
  double* centres;
};

// grid (K, active restarts).  DL lanes = dimensions (a power of two >= D), 256 / DL segments of cells
template <int DL>
__global__ __launch_bounds__(SMX_CL_TILE) void kmeans_update_kernel(UpdateArgs a) {
  constexpr int NSEG = SMX_CL_TILE / DL;
  __shared__ double ssum[SMX_CL_TILE];
  __shared__ int scnt[NSEG];
  const int d = threadIdx.x % DL, seg = threadIdx.x / DL, k = blockIdx.x;
  const long r = a.active[blockIdx.y];
  const long seg_len = (a.N + NSEG - 1) / NSEG;
  const long i0 = min(a.N, seg * seg_len), i1 = min(a.N, i0 + seg_len);
  const int32_t* lab = a.labels + r * a.N;
  double s = 0.0;
  int n = 0;
  for (long i = i0; i < i1; ++i)
    if (lab[i] == k) {
      ++n;
      if (d < a.D) s += (double)nan_if_inf(a.Z[i * a.D + d]);
    }
  ssum[threadIdx.x] = s;
  if (d == 0) scnt[seg] = n;
  __syncthreads();
  if (seg == 0 && d < a.D) {
    double tot = 0.0;
    long cnt = 0;
    for (int q = 0; q < NSEG; ++q) { tot += ssum[q * DL + d]; cnt += scnt[q]; }
    if (cnt > 0) a.centres[(r * a.K + k) * a.D + d] = tot / (double)cnt;   // (an empty cluster keeps its centre)
  }
}

// inertia[r] = the sum of mind2 [r][N] in the fixed order of smx_block.h's column sum
__global__ __launch_bounds__(SMX_CL_TILE) void kmeans_inertia_kernel(const double* mind2, long N, double* inertia) {
  __shared__ double sh4[4];
  const double total = halving_column_sum(mind2 + (long)blockIdx.x * N, N, sh4);
  if (threadIdx.x == 0) inertia[blockIdx.x] = total;
}

// slices of the j range: enough workgroups for the machine at small N, one slice once the tiles of i alone fill it -- a function of N alone
static int silhouette_slices(long N) {
  const long tiles = (N + SMX_CL_TILE - 1) / SMX_CL_TILE;
  return (int)std::max<long>(1, std::min<long>(32, 1024 / tiles));
}

}  // namespace smx

extern "C" {

int smx_cluster_silhouette(const float* Z, int64_t n_cells, int32_t D, const int32_t* labels, int32_t n_labels, double* a, double* b) {
  SMX_REQUIRE(Z && labels && a && b, "cluster_silhouette: null argument");
  SMX_REQUIRE(D >= 1 && D <= SMX_CL_MAX_D, "cluster_silhouette: 1 <= D <= 128");
  SMX_REQUIRE(n_labels >= 2 && n_labels <= SMX_CL_MAX_K, "cluster_silhouette: 2 <= n_labels <= 256");
  SMX_REQUIRE(n_cells >= 1 && n_cells < ((int64_t)1 << 31), "cluster_silhouette: 1 <= n_cells < 2^31");
  const long N = (long)n_cells;
  const int K = n_labels;
  std::vector<int32_t> off((size_t)K + 1, 0);
  for (long i = 0; i < N; ++i) {
    SMX_REQUIRE(labels[i] >= 0 && labels[i] < K, "cluster_silhouette: a label outside 0 .. n_labels - 1");
    ++off[(size_t)labels[i] + 1];
  }
  for (int c = 0; c < K; ++c) off[(size_t)c + 1] += off[(size_t)c];
  // the cells in class order, stable (a counting sort)
  std::vector<int32_t> order((size_t)N), cls((size_t)N), next(off.begin(), off.end() - 1);
  for (long i = 0; i < N; ++i) order[(size_t)next[(size_t)labels[i]]++] = (int32_t)i;
  std::vector<float> Zs((size_t)N * D);
  for (long p = 0; p < N; ++p) {
    std::copy(Z + (size_t)order[(size_t)p] * D, Z + ((size_t)order[(size_t)p] + 1) * D, Zs.begin() + (size_t)p * D);
    cls[(size_t)p] = labels[order[(size_t)p]];
  }
  const int S = silhouette_slices(N), DP = padded_width(D);
  const long tiles = (N + SMX_CL_TILE - 1) / SMX_CL_TILE;
  const int TJ = SMX_CL_LDS_DOUBLES / DP;
  const long slice_len = ((N + S - 1) / S + TJ - 1) / TJ * TJ;   // whole tiles of j
  DeviceScratch buf;
  float* dZ; int32_t *dOff, *dCls; double *dPart, *dA, *dB;
  SMX_CHECK(buf.get(&dZ, (size_t)N * D)); SMX_CHECK(buf.get(&dOff, (size_t)K + 1)); SMX_CHECK(buf.get(&dCls, (size_t)N));
  SMX_CHECK(buf.get(&dPart, (size_t)S * K * N)); SMX_CHECK(buf.get(&dA, (size_t)N)); SMX_CHECK(buf.get(&dB, (size_t)N));
  SMX_HIP(hipMemcpy(dZ, Zs.data(), Zs.size() * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dOff, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dCls, cls.data(), cls.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  const dim3 grid((unsigned)tiles, (unsigned)S), block(SMX_CL_TILE);
  switch (DP) {
    case 16: hipLaunchKernelGGL(silhouette_part_kernel<16>, grid, block, 0, nullptr, dZ, N, D, dOff, K, slice_len, dPart); break;
    case 32: hipLaunchKernelGGL(silhouette_part_kernel<32>, grid, block, 0, nullptr, dZ, N, D, dOff, K, slice_len, dPart); break;
    case 64: hipLaunchKernelGGL(silhouette_part_kernel<64>, grid, block, 0, nullptr, dZ, N, D, dOff, K, slice_len, dPart); break;
    default: hipLaunchKernelGGL(silhouette_part_kernel<128>, grid, block, 0, nullptr, dZ, N, D, dOff, K, slice_len, dPart); break;
  }
  SMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(silhouette_finish_kernel, dim3((unsigned)tiles), block, 0, nullptr, dPart, S, N, dOff, K, dCls, dA, dB);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  std::vector<double> ha((size_t)N), hb((size_t)N);
  SMX_HIP(hipMemcpy(ha.data(), dA, ha.size() * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(hb.data(), dB, hb.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (long p = 0; p < N; ++p) { a[order[(size_t)p]] = ha[(size_t)p]; b[order[(size_t)p]] = hb[(size_t)p]; }
  return SMX_OK;
}

int smx_cluster_kmeans(const float* Z, int64_t n_cells, int32_t D, int32_t K, const int32_t* init_idx, int32_t n_init, int32_t max_iter,
                       int32_t* labels_best, double* centres_best, double* inertia, int32_t* n_iter, int32_t* best, int32_t* labels_all) {
  SMX_REQUIRE(Z && init_idx && labels_best && centres_best && inertia && n_iter && best, "cluster_kmeans: null argument");
  SMX_REQUIRE(D >= 1 && D <= SMX_CL_MAX_D, "cluster_kmeans: 1 <= D <= 128");
  SMX_REQUIRE(K >= 2 && K <= SMX_CL_MAX_K, "cluster_kmeans: 2 <= K <= 256");
  SMX_REQUIRE(n_cells >= K && n_cells < ((int64_t)1 << 31), "cluster_kmeans: K <= n_cells < 2^31");
  SMX_REQUIRE(n_init >= 1 && n_init <= 4096, "cluster_kmeans: 1 <= n_init <= 4096");
  SMX_REQUIRE(max_iter >= 1, "cluster_kmeans: max_iter >= 1");
  const long N = (long)n_cells;
  const int R = n_init;
  const size_t KD = (size_t)K * D;
  std::vector<double> hC((size_t)R * KD);   // the initial centres: the named cells, as float64
  for (size_t e = 0; e < (size_t)R * K; ++e) {
    SMX_REQUIRE(init_idx[e] >= 0 && (long)init_idx[e] < N, "cluster_kmeans: an init_idx outside 0 .. n_cells - 1");
    for (int d = 0; d < D; ++d) {
      const float v = Z[(size_t)init_idx[e] * D + d];
      hC[e * D + d] = std::isinf(v) ? (double)NAN : (double)v;
    }
  }
  DeviceScratch buf;
  float* dZ; double *dC, *dMin, *dIn; int32_t *dLab, *dAct, *dActU, *dChg;   // (two lists: a copy into one never meets a launch that reads it)
  SMX_CHECK(buf.get(&dZ, (size_t)N * D)); SMX_CHECK(buf.get(&dC, hC.size())); SMX_CHECK(buf.get(&dMin, (size_t)R * N));
  SMX_CHECK(buf.get(&dIn, (size_t)R)); SMX_CHECK(buf.get(&dLab, (size_t)R * N)); SMX_CHECK(buf.get(&dAct, (size_t)R)); SMX_CHECK(buf.get(&dActU, (size_t)R));
  SMX_CHECK(buf.get(&dChg, (size_t)R));
  SMX_HIP(hipMemcpy(dZ, Z, (size_t)N * D * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dC, hC.data(), hC.size() * sizeof(double), hipMemcpyHostToDevice));
  SMX_HIP(hipMemset(dLab, 0xFF, (size_t)R * N * sizeof(int32_t)));   // label -1: the first assignment changes every cell
  std::vector<int32_t> active((size_t)R), chg((size_t)R);
  std::iota(active.begin(), active.end(), 0);
  std::fill(n_iter, n_iter + R, 0);
  const int DP = padded_width(D);
  const unsigned tiles = (unsigned)((N + SMX_CL_TILE - 1) / SMX_CL_TILE);
  const dim3 block(SMX_CL_TILE);
  for (int it = 1; it <= max_iter && !active.empty(); ++it) {
    const unsigned nA = (unsigned)active.size();
    SMX_HIP(hipMemcpy(dAct, active.data(), nA * sizeof(int32_t), hipMemcpyHostToDevice));
    SMX_HIP(hipMemset(dChg, 0, (size_t)R * sizeof(int32_t)));
    const AssignArgs aa{dZ, N, D, K, dAct, dC, dLab, dMin, dChg};
    const dim3 grid(tiles, nA);
    switch (DP) {
      case 16: hipLaunchKernelGGL(kmeans_assign_kernel<16>, grid, block, 0, nullptr, aa); break;
      case 32: hipLaunchKernelGGL(kmeans_assign_kernel<32>, grid, block, 0, nullptr, aa); break;
      case 64: hipLaunchKernelGGL(kmeans_assign_kernel<64>, grid, block, 0, nullptr, aa); break;
      default: hipLaunchKernelGGL(kmeans_assign_kernel<128>, grid, block, 0, nullptr, aa); break;
    }
    SMX_HIP(hipGetLastError());
    SMX_HIP(hipMemcpy(chg.data(), dChg, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost));   // (waits for the launch)
    std::vector<int32_t> still;
    for (int32_t r : active) {
      n_iter[r] = it;
      if (chg[(size_t)r] != 0) still.push_back(r);
    }
    active.swap(still);
    if (it == max_iter || active.empty()) break;   // the centres stay those of the last assignment
    SMX_HIP(hipMemcpy(dActU, active.data(), active.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    const UpdateArgs ua{dZ, N, D, K, dActU, dLab, dC};
    const dim3 ugrid((unsigned)K, (unsigned)active.size());
    switch (DP) {
      case 16: hipLaunchKernelGGL(kmeans_update_kernel<16>, ugrid, block, 0, nullptr, ua); break;
      case 32: hipLaunchKernelGGL(kmeans_update_kernel<32>, ugrid, block, 0, nullptr, ua); break;
      case 64: hipLaunchKernelGGL(kmeans_update_kernel<64>, ugrid, block, 0, nullptr, ua); break;
      default: hipLaunchKernelGGL(kmeans_update_kernel<128>, ugrid, block, 0, nullptr, ua); break;
    }
    SMX_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(kmeans_inertia_kernel, dim3((unsigned)R), block, 0, nullptr, dMin, N, dIn);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipMemcpy(inertia, dIn, (size_t)R * sizeof(double), hipMemcpyDeviceToHost));
  int bi = 0;
  for (int r = 1; r < R; ++r)
    if (inertia[r] < inertia[bi] || (inertia[bi] != inertia[bi] && inertia[r] == inertia[r])) bi = r;   // lowest; ties to the lowest r; NaN last
  *best = bi;
  SMX_HIP(hipMemcpy(labels_best, dLab + (size_t)bi * N, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(centres_best, dC + (size_t)bi * KD, KD * sizeof(double), hipMemcpyDeviceToHost));
  if (labels_all) SMX_HIP(hipMemcpy(labels_all, dLab, (size_t)R * N * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SMX_OK;
}

}  // extern "C"
