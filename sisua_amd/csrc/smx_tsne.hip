// smx_tsne.hip -- t-SNE embeddings of host cells (the reference scatters scikit-learn's / MulticoreTSNE's 2-D embedding of the latent
// means or of an omic: sisua/data/_single_cell_analysis.py dimension_reduce(algo='tsne'), fast_tsne in its plots).  The objective is
// scikit-learn's TSNE(method='barnes_hut') objective with the tree replaced by the EXACT sum over all pairs, all in float64; the
// definitions are in include/sisua_hip.h.  Model-free entries: they upload, compute, download and free their own buffers.  The joint P
// (the symmetrised CSR) is assembled on the host (sisua_amd/neighbors.py).
//   affinities    scikit-learn's _binary_search_perplexity, one thread per row of smx_knn's table, at most 100 rounds, every sum in
//                 column order; the row of cond_p is the round's scratch, as there.
//   repulsion     an n-body sweep in the shape of knn_part_kernel: one workgroup per (tile of 256 cells i, slice of the j range), y_i in
//                 registers, tiles of 128 y_j through LDS as broadcasts; a thread adds w and w^2 (y_i - y_j) over its slice in j order and
//                 leaves them as part [slice][1 + C][N].  The number of slices is a function of N alone (developer knob "tsne_slices").
//   Z             ONE launch of one workgroup: per cell the slices in slice order, the cells in 1024 strided partials, the lanes of a wave
//                 by halving, the sixteen waves by halving.
//   row launch    sixteen lanes per cell (a row of the symmetrised P holds a few hundred entries: one thread per row walked them as a
//                 serial chain of gathers, 1.3 ms per launch at 32768 cells against 0.9 ms of the sweep): lane l adds the
//                 row's entries l, l + 16, ... in column order, the lanes are added by halving; then lane 0 adds the slices of the
//                 repulsive sum in slice order, forms the gradient, and (in a descent) applies scikit-learn's gains / momentum /
//                 update, written to the OTHER copy of Y (the neighbours' y_j are read from the copy the iteration started with).
//                 Leaves the cell's squared gradient norm and KL term for the same fixed-order reduce, which runs on the iterations
//                 that report.
// smx_tsne_gradient and smx_tsne_fit launch the same three kernels through tsne_evaluate.  No float atomics; no workgroup waits on
// another; every loop is bounded by N, k, the row's entries, max_iter or 100; 1 / (1 + d2) is the IEEE float64 division.
#include "smx_model.h"
#include "smx_dist.h"
#include "smx_block.h"   // the fixed-order wave sum

#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>

namespace smx {

#define SMX_TSNE_MAX_SLICES 32
#define SMX_TSNE_TJ 128          // cells j per LDS tile
#define SMX_TSNE_ROUNDS 100
#define SMX_TSNE_ROW_LANES 16    // lanes that share one row of P in the row launch
#define SMX_TSNE_SUM_THREADS 1024
#define SMX_TSNE_EXPLORE 250     // scikit-learn's _EXPLORATION_MAX_ITER
#define SMX_TSNE_CHECK 50        // ... and _N_ITER_CHECK

// one thread per row of dist [N][k]: scikit-learn's binary search for the precision beta of the row; cond_p [N][k], beta [N]
__global__ __launch_bounds__(SMX_CL_TILE) void tsne_affinity_kernel(const double* dist, long N, int k, double target, double tol,
                                                                    double tiny, double* cond_p, double* beta_out) {
#pragma clang fp contract(off)   // (the host code it restates rounds every operation)
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  if (i >= N) return;
  const double* d = dist + i * k;
  double* P = cond_p + i * k;
  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, used = 1.0;
  for (int round = 0; round < SMX_TSNE_ROUNDS; ++round) {
    used = beta;
    double sum = 0.0;
    for (int c = 0; c < k; ++c) {
      const double d2 = d[c] * d[c];
      const double v = exp(-d2 * beta);
      P[c] = v;
      sum += v;
    }
    if (sum == 0.0) sum = tiny;
    double sdp = 0.0;
    for (int c = 0; c < k; ++c) {
      const double v = P[c] / sum;
      P[c] = v;
      sdp += (d[c] * d[c]) * v;
    }
    const double diff = (log(sum) + beta * sdp) - target;
    if (fabs(diff) <= tol) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
  beta_out[i] = used;
}

// w = 1 / (1 + |yi - yj|^2) and the difference d = yi - yj: the ONE form of the Student kernel, shared by both hot kernels
template <int C>
__device__ inline double student_w(const double (&yi)[C], const double* yj, double (&d)[C]) {
  d[0] = yi[0] - yj[0];
  double s = d[0] * d[0];
#pragma unroll
  for (int c = 1; c < C; ++c) {
    d[c] = yi[c] - yj[c];
    s = fma(d[c], d[c], s);
  }
  return 1.0 / (1.0 + s);
}

// part [slices][1 + C][N]: over the j of slice blockIdx.y, j != i, in j order: plane 0 the sum of w_ij, plane 1 + c of w_ij^2 (y_i - y_j)[c]
template <int C>
__global__ __launch_bounds__(SMX_CL_TILE) void tsne_rep_part_kernel(const double* Y, long N, long slice_len, double* part) {
  __shared__ double sh[SMX_TSNE_TJ * C];
  const long i = (long)blockIdx.x * SMX_CL_TILE + threadIdx.x;
  const bool live = i < N;
  const long j0 = (long)blockIdx.y * slice_len, j1 = min(N, j0 + slice_len);
  double yi[C], f[C], sw = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) { yi[c] = live ? Y[i * C + c] : 0.0; f[c] = 0.0; }
  for (long jt = j0; jt < j1; jt += SMX_TSNE_TJ) {
    const int nj = (int)min((long)SMX_TSNE_TJ, j1 - jt);
    __syncthreads();
    for (int e = threadIdx.x; e < nj * C; e += SMX_CL_TILE) sh[e] = Y[jt * C + e];
    __syncthreads();
    for (int jj = 0; jj < nj; ++jj) {
      double d[C];
      double w = student_w<C>(yi, sh + jj * C, d);
      w = jt + jj == i ? 0.0 : w;
      sw += w;
      const double w2 = w * w;
#pragma unroll
      for (int c = 0; c < C; ++c) f[c] = fma(w2, d[c], f[c]);
    }
  }
  if (live) {   // (a slice without cells writes its zeros: every plane is rewritten by every launch)
    double* o = part + (long)blockIdx.y * (1 + C) * N + i;
    o[0] = sw;
#pragma unroll
    for (int c = 0; c < C; ++c) o[(long)(1 + c) * N] = f[c];
  }
}

// out[blockIdx.x] = sum_i (sum_s x[s * stride + i], s ascending) in a fixed order: 1024 strided partials, the lanes of a wave by halving,
// the sixteen waves by halving.  Workgroup 0 sums xa (sa slices), workgroup 1 xb (sb slices).
__global__ __launch_bounds__(SMX_TSNE_SUM_THREADS) void tsne_sum_kernel(const double* xa, int sa, long stride_a, const double* xb, int sb,
                                                                       long stride_b, long n, double* out) {
  __shared__ double sh16[SMX_TSNE_SUM_THREADS / 64];
  const double* x = blockIdx.x == 0 ? xa : xb;
  const int S = blockIdx.x == 0 ? sa : sb;
  const long stride = blockIdx.x == 0 ? stride_a : stride_b;
  double v = 0.0;
  for (long i = threadIdx.x; i < n; i += SMX_TSNE_SUM_THREADS) {
    double r = x[i];
    for (int s = 1; s < S; ++s) r += x[(long)s * stride + i];
    v += r;
  }
  v = halving_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh16[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x < 64) {   // (the first wave: lanes 0 .. 15 hold the waves' sums)
    double t = threadIdx.x < SMX_TSNE_SUM_THREADS / 64 ? sh16[threadIdx.x] : 0.0;
    for (int o = 8; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
  }
}

struct TsneStep {      // what the row launch does besides the gradient
  int want_kl;         // leave the cell's KL term in row_kl
  int apply;           // 0: write grad_out; 1: the descent's update of Y, update, gains
  double exaggeration, momentum, lr;
};

// sixteen lanes per cell: grad_i = 4 [sum_{e in row} (exaggeration p_e) w (y_i - y_j) - (1 / Z) sum_s rep[s]], then either grad_out or the update.
// Lane l of a cell adds the row's entries l, l + 16, ... in this order; the lanes are added by halving (l + 8, l + 4, l + 2, l + 1) and lane 0
// finishes the cell.
template <int C>
__global__ __launch_bounds__(SMX_CL_TILE) void tsne_row_kernel(const int64_t* indptr, const int32_t* cols, const double* p, long N,
                                                               const double* Yin, const double* part, int S, const double* Zp, TsneStep st,
                                                               double* grad_out, double* Yout, double* update, double* gains,
                                                               double* row_sq, double* row_kl) {
#pragma clang fp contract(off)   // (scikit-learn's elementwise update rounds every operation; the sums spell their fma)
  const long i = ((long)blockIdx.x * SMX_CL_TILE + threadIdx.x) / SMX_TSNE_ROW_LANES;
  const int lane = threadIdx.x % SMX_TSNE_ROW_LANES;
  const bool live = i < N;   // (no thread leaves before the shuffles)
  const double Z = *Zp, invZ = 1.0 / Z;
  double yi[C], att[C], kl = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) { yi[c] = live ? Yin[i * C + c] : 0.0; att[c] = 0.0; }
  if (live) {
    const int64_t e1 = indptr[i + 1];
    for (int64_t e = indptr[i] + lane; e < e1; e += SMX_TSNE_ROW_LANES) {
      double d[C];
      const double pe = p[e];
      const double w = student_w<C>(yi, Yin + (long)cols[e] * C, d);
      const double a = (st.exaggeration * pe) * w;
#pragma unroll
      for (int c = 0; c < C; ++c) att[c] = fma(a, d[c], att[c]);
      if (st.want_kl) kl += pe * log((pe * Z) / w);
    }
  }
  for (int o = SMX_TSNE_ROW_LANES / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < C; ++c) att[c] += __shfl_down(att[c], o, SMX_TSNE_ROW_LANES);
    kl += __shfl_down(kl, o, SMX_TSNE_ROW_LANES);
  }
  if (!live || lane != 0) return;
  double sq = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double* r = part + (long)(1 + c) * N + i;
    double rep = r[0];
    for (int s = 1; s < S; ++s) rep += r[(long)s * (1 + C) * N];
    double g = 4.0 * (att[c] - invZ * rep);
    if (st.apply) {
      const long o = i * C + c;
      const double u = update[o];
      double gain = gains[o];
      gain = u * g < 0.0 ? gain + 0.2 : gain * 0.8;
      gain = gain < 0.01 ? 0.01 : gain;
      g = g * gain;
      const double un = st.momentum * u - st.lr * g;
      gains[o] = gain;
      update[o] = un;
      Yout[o] = yi[c] + un;
    } else {
      grad_out[i * C + c] = g;
    }
    sq = fma(g, g, sq);
  }
  row_sq[i] = sq;
  if (st.want_kl) row_kl[i] = kl;
}

// slices of the j range: knn_slices' rule -- a function of N alone
static int tsne_slices(long N) {
  const long tiles = (N + SMX_CL_TILE - 1) / SMX_CL_TILE;
  int s = (int)std::max<long>(1, std::min<long>(SMX_TSNE_MAX_SLICES, 1024 / tiles));
  const int forced = (int)tuning("tsne_slices", 0.0);   // (read per call: a test sets it between calls)
  if (forced > 0) s = std::min(forced, SMX_TSNE_MAX_SLICES);
  return s;
}

// the device side of one problem: P, the partial sums and the per-cell terms
struct TsneDevice {
  long N = 0;
  int C = 0, S = 1;
  long slice_len = 0;
  int64_t* indptr = nullptr;
  int32_t* cols = nullptr;
  double *p = nullptr, *part = nullptr, *Z = nullptr, *row_sq = nullptr, *row_kl = nullptr, *pair = nullptr;
};

static int tsne_upload(DeviceScratch& buf, TsneDevice* t, const int64_t* indptr, const int32_t* cols, const double* p, long N, int C) {
  t->N = N; t->C = C; t->S = tsne_slices(N);
  t->slice_len = ((N + t->S - 1) / t->S + SMX_TSNE_TJ - 1) / SMX_TSNE_TJ * SMX_TSNE_TJ;   // whole tiles of j
  const size_t nnz = (size_t)indptr[N];
  SMX_CHECK(buf.put(&t->indptr, indptr, (size_t)N + 1));
  if (nnz) { SMX_CHECK(buf.put(&t->cols, cols, nnz)); SMX_CHECK(buf.put(&t->p, p, nnz)); }
  else { SMX_CHECK(buf.get(&t->cols, (size_t)1)); SMX_CHECK(buf.get(&t->p, (size_t)1)); }   // (an empty P: nothing attracts)
  SMX_CHECK(buf.get(&t->part, (size_t)t->S * (1 + C) * N));
  SMX_CHECK(buf.get(&t->Z, (size_t)1));
  SMX_CHECK(buf.get(&t->row_sq, (size_t)N)); SMX_CHECK(buf.get(&t->row_kl, (size_t)N));
  SMX_CHECK(buf.get(&t->pair, (size_t)2));
  return SMX_OK;
}

// one evaluation of the objective's gradient at Yin, enqueued: the three launches every caller shares.  With st.want_kl a fourth leaves
// pair = (sum of the cells' squared gradients, KL).
static int tsne_evaluate(const TsneDevice& t, const double* Yin, const TsneStep& st, double* grad_out, double* Yout, double* update,
                         double* gains) {
  const long N = t.N;
  const unsigned tiles = (unsigned)((N + SMX_CL_TILE - 1) / SMX_CL_TILE);
  const unsigned row_tiles = (unsigned)((N * SMX_TSNE_ROW_LANES + SMX_CL_TILE - 1) / SMX_CL_TILE);
  const dim3 grid(tiles, (unsigned)t.S), block(SMX_CL_TILE);
  switch (t.C) {
    case 1: hipLaunchKernelGGL(tsne_rep_part_kernel<1>, grid, block, 0, nullptr, Yin, N, t.slice_len, t.part); break;
    case 2: hipLaunchKernelGGL(tsne_rep_part_kernel<2>, grid, block, 0, nullptr, Yin, N, t.slice_len, t.part); break;
    default: hipLaunchKernelGGL(tsne_rep_part_kernel<3>, grid, block, 0, nullptr, Yin, N, t.slice_len, t.part); break;
  }
  SMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(tsne_sum_kernel, dim3(1), dim3(SMX_TSNE_SUM_THREADS), 0, nullptr, t.part, t.S, (long)(1 + t.C) * N, t.part, 0, 0L, N, t.Z);
  SMX_HIP(hipGetLastError());
  switch (t.C) {
    case 1: hipLaunchKernelGGL(tsne_row_kernel<1>, dim3(row_tiles), block, 0, nullptr, t.indptr, t.cols, t.p, N, Yin, t.part, t.S, t.Z, st, grad_out,
                               Yout, update, gains, t.row_sq, t.row_kl); break;
    case 2: hipLaunchKernelGGL(tsne_row_kernel<2>, dim3(row_tiles), block, 0, nullptr, t.indptr, t.cols, t.p, N, Yin, t.part, t.S, t.Z, st, grad_out,
                               Yout, update, gains, t.row_sq, t.row_kl); break;
    default: hipLaunchKernelGGL(tsne_row_kernel<3>, dim3(row_tiles), block, 0, nullptr, t.indptr, t.cols, t.p, N, Yin, t.part, t.S, t.Z, st, grad_out,
                                Yout, update, gains, t.row_sq, t.row_kl); break;
  }
  SMX_HIP(hipGetLastError());
  if (st.want_kl) {
    hipLaunchKernelGGL(tsne_sum_kernel, dim3(2), dim3(SMX_TSNE_SUM_THREADS), 0, nullptr, t.row_sq, 1, 0L, t.row_kl, 1, 0L, N, t.pair);
    SMX_HIP(hipGetLastError());
  }
  return SMX_OK;
}

// the checks both entries share, on the host: the CSR of P and the embedding
static int tsne_check_problem(const int64_t* indptr, const int32_t* cols, const double* p, int64_t n_cells, int32_t C, const double* Y) {
  SMX_REQUIRE(indptr && cols && p && Y, "tsne: null argument");
  SMX_REQUIRE(n_cells >= 4 && n_cells < ((int64_t)1 << 31), "tsne: 4 <= n_cells < 2^31");
  SMX_REQUIRE(C >= 1 && C <= 3, "tsne: 1 <= n_components <= 3");
  SMX_REQUIRE(indptr[0] == 0, "tsne: indptr[0] must be 0");
  for (int64_t i = 0; i < n_cells; ++i) {
    SMX_REQUIRE(indptr[i + 1] >= indptr[i] && indptr[i + 1] - indptr[i] <= n_cells, "tsne: indptr must not decrease, and a row holds at most n_cells entries");
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
      SMX_REQUIRE(cols[e] >= 0 && (int64_t)cols[e] < n_cells, "tsne: a column outside 0 .. n_cells - 1");
      SMX_REQUIRE(e == indptr[i] || cols[e] > cols[e - 1], "tsne: the columns of a row must increase strictly");
      SMX_REQUIRE(std::isfinite(p[e]) && p[e] > 0.0, "tsne: an entry of P that is not finite and positive");
    }
  }
  for (size_t e = 0; e < (size_t)n_cells * C; ++e) SMX_REQUIRE(std::isfinite(Y[e]), "tsne: an entry of Y that is not finite");
  return SMX_OK;
}

}  // namespace smx

using namespace smx;

extern "C" {

int smx_tsne_affinities(const int32_t* idx, const double* dist, int64_t n_cells, int32_t k, double perplexity, double* cond_p, double* beta) {
  SMX_REQUIRE(idx && dist && cond_p && beta, "tsne_affinities: null argument");
  SMX_REQUIRE(k >= 1 && k <= SMX_CL_MAX_K, "tsne_affinities: 1 <= k <= 256");
  SMX_REQUIRE(n_cells >= 4 && n_cells > k && n_cells < ((int64_t)1 << 31), "tsne_affinities: 4 <= n_cells, k < n_cells < 2^31");
  SMX_REQUIRE(std::isfinite(perplexity) && perplexity >= 1.0 && perplexity < (double)n_cells, "tsne_affinities: 1 <= perplexity < n_cells");
  const long N = (long)n_cells;
  for (size_t e = 0; e < (size_t)N * k; ++e) {
    SMX_REQUIRE(idx[e] >= 0 && (long)idx[e] < N, "tsne_affinities: an index outside 0 .. n_cells - 1");
    SMX_REQUIRE(std::isfinite(dist[e]) && dist[e] >= 0.0, "tsne_affinities: a distance that is negative or not finite");
  }
  DeviceScratch buf;
  double *dDist, *dP, *dBeta;
  SMX_CHECK(buf.put(&dDist, dist, (size_t)N * k));
  SMX_CHECK(buf.get(&dP, (size_t)N * k)); SMX_CHECK(buf.get(&dBeta, (size_t)N));
  hipLaunchKernelGGL(tsne_affinity_kernel, dim3((unsigned)((N + SMX_CL_TILE - 1) / SMX_CL_TILE)), dim3(SMX_CL_TILE), 0, nullptr, dDist, N, k,
                     std::log((double)(float)perplexity), (double)1e-5f, (double)1e-8f, dP, dBeta);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(cond_p, dP, (size_t)N * k * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(beta, dBeta, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_tsne_gradient(const int64_t* indptr, const int32_t* cols, const double* p, int64_t n_cells, int32_t n_components, const double* Y,
                      double exaggeration, double* grad, double* kl, double* Z) {
  SMX_REQUIRE(grad && kl && Z, "tsne_gradient: null argument");
  SMX_CHECK(tsne_check_problem(indptr, cols, p, n_cells, n_components, Y));
  SMX_REQUIRE(std::isfinite(exaggeration) && exaggeration > 0.0, "tsne_gradient: exaggeration must be finite and positive");
  const long N = (long)n_cells;
  const int C = n_components;
  DeviceScratch buf;
  TsneDevice t;
  SMX_CHECK(tsne_upload(buf, &t, indptr, cols, p, N, C));
  double *dY, *dGrad;
  SMX_CHECK(buf.put(&dY, Y, (size_t)N * C)); SMX_CHECK(buf.get(&dGrad, (size_t)N * C));
  TsneStep st{1, 0, exaggeration, 0.0, 0.0};
  SMX_CHECK(tsne_evaluate(t, dY, st, dGrad, nullptr, nullptr, nullptr));
  SMX_HIP(hipDeviceSynchronize());
  double pair[2];
  SMX_HIP(hipMemcpy(grad, dGrad, (size_t)N * C * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(pair, t.pair, sizeof(pair), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(Z, t.Z, sizeof(double), hipMemcpyDeviceToHost));
  *kl = pair[1];
  return SMX_OK;
}

int smx_tsne_fit(const int64_t* indptr, const int32_t* cols, const double* p, int64_t n_cells, int32_t n_components, const double* Y0,
                 int32_t max_iter, double early_exaggeration, double learning_rate, double min_grad_norm, int32_t n_iter_without_progress,
                 double* Y, double* kl_trace, int32_t* n_iter, double* update_out, double* gains_out) {
  SMX_REQUIRE(Y && kl_trace && n_iter, "tsne_fit: null argument");
  SMX_CHECK(tsne_check_problem(indptr, cols, p, n_cells, n_components, Y0));
  SMX_REQUIRE(max_iter >= 1, "tsne_fit: max_iter >= 1");
  SMX_REQUIRE(std::isfinite(early_exaggeration) && early_exaggeration > 0.0, "tsne_fit: early_exaggeration must be finite and positive");
  SMX_REQUIRE(std::isfinite(learning_rate) && learning_rate > 0.0, "tsne_fit: learning_rate must be finite and positive");
  SMX_REQUIRE(min_grad_norm >= 0.0, "tsne_fit: min_grad_norm >= 0");
  SMX_REQUIRE(n_iter_without_progress >= 0, "tsne_fit: n_iter_without_progress >= 0");
  const long N = (long)n_cells;
  const int C = n_components;
  const size_t NC = (size_t)N * C;
  DeviceScratch buf;
  TsneDevice t;
  SMX_CHECK(tsne_upload(buf, &t, indptr, cols, p, N, C));
  double *dYa, *dYb, *dUpdate, *dGains;
  SMX_CHECK(buf.put(&dYa, Y0, NC)); SMX_CHECK(buf.get(&dYb, NC));
  SMX_CHECK(buf.get(&dUpdate, NC)); SMX_CHECK(buf.get(&dGains, NC));
  std::vector<double> ones(NC, 1.0);
  for (int32_t i = 0; i < max_iter; ++i) kl_trace[i] = std::numeric_limits<double>::quiet_NaN();
  int it = 0;   // iterations run so far
  // scikit-learn's two calls of _gradient_descent: each starts from update = 0 and gains = 1, and a stop ends the call it happens in
  for (int phase = 0; phase < 2 && it < max_iter; ++phase) {
    const int end = phase == 0 ? std::min<int>(SMX_TSNE_EXPLORE, max_iter) : max_iter;
    SMX_HIP(hipMemset(dUpdate, 0, NC * sizeof(double)));
    SMX_HIP(hipMemcpy(dGains, ones.data(), NC * sizeof(double), hipMemcpyHostToDevice));
    double best = std::numeric_limits<double>::max();
    int best_iter = it;
    for (int i = it; i < end; ++i) {
      const bool convergence = (i + 1) % SMX_TSNE_CHECK == 0, report = convergence || i == end - 1;
      TsneStep st{report ? 1 : 0, 1, phase == 0 ? early_exaggeration : 1.0, phase == 0 ? 0.5 : 0.8, learning_rate};
      SMX_CHECK(tsne_evaluate(t, dYa, st, nullptr, dYb, dUpdate, dGains));
      std::swap(dYa, dYb);   // dYa: the current embedding
      it = i + 1;
      if (!report) continue;
      double pair[2];   // (the copy waits for the launches in front of it)
      SMX_HIP(hipMemcpy(pair, t.pair, sizeof(pair), hipMemcpyDeviceToHost));
      kl_trace[i] = pair[1];
      if (!convergence) continue;
      if (pair[1] < best) { best = pair[1]; best_iter = i; }
      else if (phase == 1 && i - best_iter > n_iter_without_progress) break;
      if (std::sqrt(pair[0]) <= min_grad_norm) break;
    }
  }
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(Y, dYa, NC * sizeof(double), hipMemcpyDeviceToHost));
  if (update_out) SMX_HIP(hipMemcpy(update_out, dUpdate, NC * sizeof(double), hipMemcpyDeviceToHost));
  if (gains_out) SMX_HIP(hipMemcpy(gains_out, dGains, NC * sizeof(double), hipMemcpyDeviceToHost));
  *n_iter = it;
  return SMX_OK;
}

}  // extern "C"
