// smx_gmm_full.hip -- the full-covariance Gaussian mixture of the reference's clustering scores (sisua/analysis/latent_benchmarks.py:69-117:
// GaussianMixture(n_labels, random_state=5218)) on host arrays Z [N][D] float32: scikit-learn's EM loop run from R starting labelings, all
// restarts of a call together.  Model-free entries: they upload, compute, download and free their own buffers.  Everything is float64.
//   responsibilities  resp [R][K][N], so that every pass over the cells of one component reads it coalesced.
//   M-step            three launches.  (1) per (slice, component, restart): sum r and sum r z[d]; lanes = dimensions, 256 / lanes contiguous
//                     segments of the slice summed in cell order and then added in segment order.  (2) per (slice, component, restart): the
//                     scatter sums in the two-pass form.  The workgroup first adds the slices of (1) in index order (nk, mu: the same bits in
//                     every workgroup of the component), stages chunks of (z - mu) and r through LDS as float64, and every thread owns up to 9
//                     fixed entries (i, j) of the lower triangle with ONE running sum each over the slice's cells in order.  (3) per
//                     (component, restart): adds the partial triangles in slice order, / nk, + reg_covar on the diagonal, mirrors, writes the
//                     covariance, factors it in LDS (right-looking column Cholesky), inverts the factor in place (the inverse's strict lower
//                     triangle is kept transposed in the square's upper half, one thread per column), writes Linv, the E-step's constant and
//                     the weights and means.  A pivot that is not a positive finite number sets the restart's bad flag and the workgroup ends.
//                     The workgroup of component 0 also adds the E-step's lower-bound partials in index order and forms the stop flag.
//   E-step            one thread per cell, z in registers (D padded to 4, 8, 16, 32 or 64 with zeros); per component mu and the packed lower
//                     triangle of Linv pass through LDS (every lane reads the same address); diff = z - mu first, then y = Linv diff row by row
//                     (one chain per row, j ascending), q = sum y^2 (rows ascending).  l_nk is parked in resp, then the row maximum, the sum of
//                     exponentials in k order, and r = exp(l - lse) overwrite it.  The lower-bound partial of a workgroup: smx_block.h's
//                     fixed-order block sum.
//   host loop         after every iteration ONE copy of 2 R flags (stop, bad); finished restarts leave the list of the later launches.
// The number of slices is a function of N alone, and so is the order of every sum: two calls give the same bits and a restart gives the same
// bits alone or in a batch.  No float atomics; every loop is bounded by N, K, D, the slices or max_iter; no workgroup waits on another.
#include "smx_model.h"
#include "smx_block.h"   // the fixed-order block sum

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>

namespace smx {

#define SMX_GF_TILE 256
#define SMX_GF_MAX_D 64
#define SMX_GF_MAX_K 256
#define SMX_GF_MAX_R 8
#define SMX_GF_LDS_DOUBLES 4096     // 32 KB: the staged chunk of the scatter launch, the square of the closing launch
#define SMX_GF_SLICE_CELLS 1024     // a slice is at least this many cells ...
#define SMX_GF_MAX_SLICES 64        // ... until there are this many slices
#define SMX_GF_MAX_ENTRIES 9        // ceil(2080 / 256): the triangle entries of a thread at D = 64
#define SMX_GF_LOG_2PI 1.8378770664093454836

struct GfShape {
  long N, slice_len;
  int D, K, S, T;   // T = D (D + 1) / 2
};

// nk and mu[d] of (restart, component) from the partial sums pm [S][D + 1] (slot D: sum r), the slices in index order.  Threads d < D fill
// mu[d]; every thread returns nk (the same chain of additions, so the same bits)
__device__ inline double gf_mean_from_parts(const double* pm, int S, int D, double* mu) {
  double sr = 0.0;
  for (int s = 0; s < S; ++s) sr += pm[s * (D + 1) + D];
  const double nk = sr + 10.0 * DBL_EPSILON;
  if ((int)threadIdx.x < D) {
    double sz = 0.0;
    for (int s = 0; s < S; ++s) sz += pm[s * (D + 1) + threadIdx.x];
    mu[threadIdx.x] = sz / nk;
  }
  return nk;
}

// entry e of the row-major lower triangle -> (i, j), j <= i; bounded by D
__device__ inline void gf_entry(int e, int D, int* i, int* j) {
  int r = 0;
  while (r + 1 < D && (r + 1) * (r + 2) / 2 <= e) ++r;
  *i = r; *j = e - r * (r + 1) / 2;
}

// ---- the start: one-hot responsibilities ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SMX_GF_TILE) void gf_onehot_kernel(const int32_t* labels, long N, int K, double* resp) {
  const long i = (long)blockIdx.x * SMX_GF_TILE + threadIdx.x;
  if (i >= N) return;
  const long r = blockIdx.z, k = blockIdx.y;
  resp[(r * K + k) * N + i] = labels[r * N + i] == (int)k ? 1.0 : 0.0;
}

// ---- M-step (1): sum r, sum r z ------------------------------------------------------------------------------------------------------
struct GfMeanArgs {
  const float* Z; GfShape sh;
  const int32_t* active;
  const double* resp;   // [R][K][N]
  double* pm;           // [R][K][S][D + 1]
  int DL;               // lanes = dimensions: a power of two >= D
};

__global__ __launch_bounds__(SMX_GF_TILE) void gf_mean_part_kernel(GfMeanArgs a) {
  __shared__ double ssum[SMX_GF_TILE], srr[SMX_GF_TILE];
  const int D = a.sh.D, DL = a.DL, nseg = SMX_GF_TILE / DL;
  const int d = threadIdx.x % DL, seg = threadIdx.x / DL;
  const long r = a.active[blockIdx.z], k = blockIdx.y, s = blockIdx.x;
  const long i0 = min(a.sh.N, s * a.sh.slice_len), i1 = min(a.sh.N, i0 + a.sh.slice_len);
  const long seg_len = (i1 - i0 + nseg - 1) / nseg;
  const long b0 = min(i1, i0 + seg * seg_len), b1 = min(i1, b0 + seg_len);
  const double* rk = a.resp + (r * a.sh.K + k) * a.sh.N;
  double sz = 0.0, sr = 0.0;
  for (long i = b0; i < b1; ++i) {
    const double w = rk[i];
    sr += w;
    if (d < D) sz = fma(w, (double)a.Z[i * D + d], sz);
  }
  ssum[threadIdx.x] = sz; srr[threadIdx.x] = sr;
  __syncthreads();
  if (seg == 0 && d < D) {
    double tot = 0.0;
    for (int q = 0; q < nseg; ++q) tot += ssum[q * DL + d];
    a.pm[((r * a.sh.K + k) * a.sh.S + s) * (D + 1) + d] = tot;
  }
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int q = 0; q < nseg; ++q) tot += srr[q * DL];
    a.pm[((r * a.sh.K + k) * a.sh.S + s) * (D + 1) + D] = tot;
  }
}

// ---- M-step (2): the scatter sums of a slice ---------------------------------------------------------------------------------------
struct GfScatterArgs {
  const float* Z; GfShape sh;
  const int32_t* active;
  const double* resp;
  const double* pm;
  double* pt;           // [R][K][S][T]
};

template <int NE>
__global__ __launch_bounds__(SMX_GF_TILE) void gf_scatter_kernel(GfScatterArgs a) {
  __shared__ double sh[SMX_GF_LDS_DOUBLES];
  __shared__ double mu[SMX_GF_MAX_D];
  const int D = a.sh.D, T = a.sh.T;
  const long r = a.active[blockIdx.z], k = blockIdx.y, s = blockIdx.x;
  const long job = r * a.sh.K + k;
  gf_mean_from_parts(a.pm + job * a.sh.S * (D + 1), a.sh.S, D, mu);
  int ei[NE], ej[NE];
  double acc[NE];
#pragma unroll
  for (int q = 0; q < NE; ++q) {
    const int e = threadIdx.x + q * SMX_GF_TILE;
    ei[q] = 0; ej[q] = 0; acc[q] = 0.0;
    if (e < T) gf_entry(e, D, &ei[q], &ej[q]);
  }
  const int CH = SMX_GF_LDS_DOUBLES / (D + 1);   // cells of a chunk: CH D differences and CH responsibilities
  double* shr = sh + CH * D;
  const long i0 = min(a.sh.N, s * a.sh.slice_len), i1 = min(a.sh.N, i0 + a.sh.slice_len);
  const double* rk = a.resp + job * a.sh.N;
  for (long c0 = i0; c0 < i1; c0 += CH) {
    const int n = (int)min((long)CH, i1 - c0);
    __syncthreads();   // (the first pass: mu is complete; later ones: the previous chunk has been read)
    for (int e = threadIdx.x; e < n * D; e += SMX_GF_TILE) sh[e] = (double)a.Z[c0 * D + e] - mu[e % D];
    for (int c = threadIdx.x; c < n; c += SMX_GF_TILE) shr[c] = rk[c0 + c];
    __syncthreads();
    for (int c = 0; c < n; ++c) {
      const double w = shr[c];
      const double* row = sh + c * D;
#pragma unroll
      for (int q = 0; q < NE; ++q) acc[q] = fma(w * row[ei[q]], row[ej[q]], acc[q]);
    }
  }
  double* out = a.pt + (job * a.sh.S + s) * T;
#pragma unroll
  for (int q = 0; q < NE; ++q) {
    const int e = threadIdx.x + q * SMX_GF_TILE;
    if (e < T) out[e] = acc[q];
  }
}

// ---- M-step (3): close a component ---------------------------------------------------------------------------------------------------
struct GfCloseArgs {
  GfShape sh;
  const int32_t* active;
  const double* pm;
  const double* pt;
  double reg_covar, tol;
  int initial, n_tiles;
  const double* lb_part;   // [R][n_tiles]
  double* weights;         // [R][K]
  double* means;           // [R][K][D]
  double* cov;             // [R][K][D][D]
  double* linv;            // [R][K][D][D]
  double* logc;            // [R][K]: log w + logdet
  double* lb;              // [R]
  int32_t* flags;          // [2][R]: stop, bad
  int R;
};

__global__ __launch_bounds__(SMX_GF_TILE) void gf_close_kernel(GfCloseArgs a) {
  __shared__ double A[SMX_GF_LDS_DOUBLES];
  __shared__ double mu[SMX_GF_MAX_D], xd[SMX_GF_MAX_D];
  const int D = a.sh.D, T = a.sh.T, S = a.sh.S;
  const long r = a.active[blockIdx.y], k = blockIdx.x;
  const long job = r * a.sh.K + k;
  if (k == 0 && threadIdx.x == 0) {   // the restart's lower bound and stop flag
    if (a.initial) { a.lb[r] = -INFINITY; a.flags[r] = 0; }
    else {
      double ll = 0.0;
      for (int t = 0; t < a.n_tiles; ++t) ll += a.lb_part[r * a.n_tiles + t];
      const double lb = ll / (double)a.sh.N;
      a.flags[r] = fabs(lb - a.lb[r]) < a.tol ? 1 : 0;
      a.lb[r] = lb;
    }
  }
  const double nk = gf_mean_from_parts(a.pm + job * S * (D + 1), S, D, mu);
  const double w = nk / (double)a.sh.N;
  for (int e = threadIdx.x; e < T; e += SMX_GF_TILE) {
    int i, j;
    gf_entry(e, D, &i, &j);
    double tot = 0.0;
    for (int s = 0; s < S; ++s) tot += a.pt[(job * S + s) * T + e];
    double v = tot / nk;
    if (i == j) v += a.reg_covar;
    A[i * D + j] = v; A[j * D + i] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < D) a.means[job * D + threadIdx.x] = mu[threadIdx.x];
  if (threadIdx.x == 0) a.weights[job] = w;
  for (int e = threadIdx.x; e < D * D; e += SMX_GF_TILE) a.cov[job * D * D + e] = A[e];
  // the factor L (lower triangle of A, in place), column by column
  for (int j = 0; j < D; ++j) {
    __syncthreads();
    const double p = A[j * D + j];   // (every thread reads the same word: the exit below is block-uniform)
    if (!(p > 0.0 && p < INFINITY)) {
      if (threadIdx.x == 0) a.flags[a.R + r] = 1;
      return;
    }
    __syncthreads();
    const double ljj = sqrt(p);
    if (threadIdx.x == 0) A[j * D + j] = ljj;
    for (int i = j + 1 + threadIdx.x; i < D; i += SMX_GF_TILE) A[i * D + j] /= ljj;
    __syncthreads();
    const int m = D - 1 - j;
    for (int e = threadIdx.x; e < m * m; e += SMX_GF_TILE) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) A[i * D + c] = fma(-A[i * D + j], A[c * D + j], A[i * D + c]);
    }
  }
  __syncthreads();
  // X = L^-1: thread c owns column c; X[i][c] (i > c) is kept at A[c][i], the diagonal in xd
  if ((int)threadIdx.x < D) {
    const int c = threadIdx.x;
    const double xc = 1.0 / A[c * D + c];
    xd[c] = xc;
    for (int i = c + 1; i < D; ++i) {
      double s = A[i * D + c] * xc;
      for (int q = c + 1; q < i; ++q) s = fma(A[i * D + q], A[c * D + q], s);
      A[c * D + i] = -s / A[i * D + i];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < D * D; e += SMX_GF_TILE) {
    const int i = e / D, c = e % D;
    a.linv[job * D * D + e] = i > c ? A[c * D + i] : i == c ? xd[c] : 0.0;
  }
  if (threadIdx.x == 0) {
    double ld = 0.0;
    for (int d = 0; d < D; ++d) ld += log(A[d * D + d]);
    a.logc[job] = log(w) + (-ld);
  }
}

// ---- E-step --------------------------------------------------------------------------------------------------------------------------
struct GfEArgs {
  const float* Z; long N; int D, K;
  const int32_t* active;
  const double* means;     // [R][K][D]
  const double* linv;      // [R][K][D][D]
  const double* logc;      // [R][K]
  double* resp;            // [R][K][N]: l_nk, then r_nk
  double* lb_part;         // [R][n_tiles] or null
  int32_t* labels;         // [N] or null (the launch then has one restart)
  double* score;           // [N] or null
};

template <int DP>
__global__ __launch_bounds__(SMX_GF_TILE) void gf_estep_kernel(GfEArgs a) {
  __shared__ double shL[DP * (DP + 1) / 2];
  __shared__ double shmu[DP];
  __shared__ double sh4[4];
  const long i = (long)blockIdx.x * SMX_GF_TILE + threadIdx.x;
  const long r = a.active[blockIdx.y];
  const int D = a.D, K = a.K;
  const bool live = i < a.N;
  float z[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) z[d] = (live && d < D) ? a.Z[i * D + d] : 0.f;
  double* lrow = a.resp + r * K * a.N + i;
  const double d_log_2pi = (double)D * SMX_GF_LOG_2PI;
  double mx = -INFINITY;
  int best = 0;
  for (int k = 0; k < K; ++k) {
    const double* L = a.linv + (r * K + k) * D * D;
    __syncthreads();
    for (int e = threadIdx.x; e < D * D; e += SMX_GF_TILE) {
      const int ii = e / D, jj = e % D;
      if (jj <= ii) shL[ii * (ii + 1) / 2 + jj] = L[e];
    }
    if ((int)threadIdx.x < DP) shmu[threadIdx.x] = (int)threadIdx.x < D ? a.means[(r * K + k) * D + threadIdx.x] : 0.0;
    __syncthreads();
    double diff[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) diff[d] = (double)z[d] - shmu[d];
    double q = 0.0;
#pragma unroll
    for (int ii = 0; ii < DP; ++ii) {
      if (ii < D) {   // (block-uniform)
        double y = 0.0;
#pragma unroll
        for (int jj = 0; jj <= ii; ++jj) y = fma(shL[ii * (ii + 1) / 2 + jj], diff[jj], y);
        q = fma(y, y, q);
      }
    }
    const double l = a.logc[r * K + k] - (d_log_2pi + q) / 2.0;
    if (live) lrow[(long)k * a.N] = l;
    if (l > mx) { mx = l; best = k; }   // strict: ties to the lowest k
  }
  double lse = 0.0;
  if (live) {
    double se = 0.0;
    for (int k = 0; k < K; ++k) se += exp(lrow[(long)k * a.N] - mx);
    lse = mx + log(se);
    for (int k = 0; k < K; ++k) lrow[(long)k * a.N] = exp(lrow[(long)k * a.N] - lse);
    if (a.labels) a.labels[i] = best;
    if (a.score) a.score[i] = lse;
  }
  if (a.lb_part) {
    const double total = halving_block_sum(lse, sh4);
    if (threadIdx.x == 0) a.lb_part[r * gridDim.x + blockIdx.x] = total;
  }
}

static int gf_padded_width(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }

static int gf_slices(long N) {
  return (int)std::max<long>(1, std::min<long>(SMX_GF_MAX_SLICES, (N + SMX_GF_SLICE_CELLS - 1) / SMX_GF_SLICE_CELLS));
}

static void gf_launch_estep(int DP, dim3 grid, const GfEArgs& ea) {
  const dim3 block(SMX_GF_TILE);
  switch (DP) {
    case 4: hipLaunchKernelGGL(gf_estep_kernel<4>, grid, block, 0, nullptr, ea); break;
    case 8: hipLaunchKernelGGL(gf_estep_kernel<8>, grid, block, 0, nullptr, ea); break;
    case 16: hipLaunchKernelGGL(gf_estep_kernel<16>, grid, block, 0, nullptr, ea); break;
    case 32: hipLaunchKernelGGL(gf_estep_kernel<32>, grid, block, 0, nullptr, ea); break;
    default: hipLaunchKernelGGL(gf_estep_kernel<64>, grid, block, 0, nullptr, ea); break;
  }
}

static void gf_launch_scatter(int T, dim3 grid, const GfScatterArgs& sa) {
  const dim3 block(SMX_GF_TILE);
  const int ne = (T + SMX_GF_TILE - 1) / SMX_GF_TILE;
  if (ne <= 1) hipLaunchKernelGGL(gf_scatter_kernel<1>, grid, block, 0, nullptr, sa);
  else if (ne <= 3) hipLaunchKernelGGL(gf_scatter_kernel<3>, grid, block, 0, nullptr, sa);
  else if (ne <= 5) hipLaunchKernelGGL(gf_scatter_kernel<5>, grid, block, 0, nullptr, sa);
  else hipLaunchKernelGGL(gf_scatter_kernel<SMX_GF_MAX_ENTRIES>, grid, block, 0, nullptr, sa);
}

static int gf_check_shape(const char* who, const float* Z, int64_t n_cells, int32_t D, int32_t K) {
  const std::string w(who);
  if (!(D >= 1 && D <= SMX_GF_MAX_D)) { set_error(w + ": 1 <= D <= 64"); return SMX_ERR_INVALID; }
  if (!(K >= 2 && K <= SMX_GF_MAX_K)) { set_error(w + ": 2 <= K <= 256"); return SMX_ERR_INVALID; }
  if (!(n_cells >= K && n_cells < ((int64_t)1 << 31))) { set_error(w + ": K <= n_cells < 2^31"); return SMX_ERR_INVALID; }
  for (size_t e = 0; e < (size_t)n_cells * D; ++e)
    if (!std::isfinite(Z[e])) { set_error(w + ": Z holds a non-finite entry (cell " + std::to_string(e / D) + ")"); return SMX_ERR_INVALID; }
  return SMX_OK;
}

}  // namespace smx

extern "C" {

int smx_gmm_full_fit(const float* Z, int64_t n_cells, int32_t D, int32_t K, const int32_t* init_labels, int32_t R, int32_t max_iter, double tol,
                     double reg_covar, double* lower_bound, int32_t* n_iter, int32_t* converged, int32_t* status, int32_t* best,
                     double* weights, double* means, double* covariances, double* chol_inv, int32_t* labels, double* params_all) {
  using namespace smx;
  SMX_REQUIRE(Z && init_labels && lower_bound && n_iter && converged && status && best && weights && means && covariances && chol_inv && labels,
              "gmm_full_fit: null argument");
  SMX_REQUIRE(R >= 1 && R <= SMX_GF_MAX_R, "gmm_full_fit: 1 <= R <= 8");
  SMX_REQUIRE(max_iter >= 1, "gmm_full_fit: max_iter >= 1");
  SMX_REQUIRE(tol > 0.0 && std::isfinite(tol), "gmm_full_fit: tol > 0");
  SMX_REQUIRE(reg_covar >= 0.0 && std::isfinite(reg_covar), "gmm_full_fit: reg_covar >= 0");
  SMX_CHECK(gf_check_shape("gmm_full_fit", Z, n_cells, D, K));
  const long N = (long)n_cells;
  for (size_t e = 0; e < (size_t)R * N; ++e)
    SMX_REQUIRE(init_labels[e] >= 0 && init_labels[e] < K, "gmm_full_fit: an init_labels entry outside 0 .. K - 1");
  const int S = gf_slices(N), T = D * (D + 1) / 2, DP = gf_padded_width(D);
  const GfShape shp{N, (N + S - 1) / S, D, K, S, T};
  const unsigned tiles = (unsigned)((N + SMX_GF_TILE - 1) / SMX_GF_TILE);
  const size_t RK = (size_t)R * K, DD = (size_t)D * D;
  int DL = 1;
  while (DL < D) DL *= 2;
  DeviceScratch buf;
  float* dZ; double *dResp, *dPm, *dPt, *dW, *dMu, *dCov, *dLinv, *dLogc, *dLb, *dLbPart; int32_t *dLab, *dAct, *dFlags, *dOut;
  SMX_CHECK(buf.get(&dZ, (size_t)N * D)); SMX_CHECK(buf.get(&dResp, RK * N)); SMX_CHECK(buf.get(&dPm, RK * S * (D + 1)));
  SMX_CHECK(buf.get(&dPt, RK * S * T)); SMX_CHECK(buf.get(&dW, RK)); SMX_CHECK(buf.get(&dMu, RK * D)); SMX_CHECK(buf.get(&dCov, RK * DD));
  SMX_CHECK(buf.get(&dLinv, RK * DD)); SMX_CHECK(buf.get(&dLogc, RK)); SMX_CHECK(buf.get(&dLb, (size_t)R));
  SMX_CHECK(buf.get(&dLbPart, (size_t)R * tiles)); SMX_CHECK(buf.get(&dLab, (size_t)R * N)); SMX_CHECK(buf.get(&dAct, (size_t)R));
  SMX_CHECK(buf.get(&dFlags, (size_t)2 * R)); SMX_CHECK(buf.get(&dOut, (size_t)N));
  SMX_HIP(hipMemcpy(dZ, Z, (size_t)N * D * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dLab, init_labels, (size_t)R * N * sizeof(int32_t), hipMemcpyHostToDevice));
  std::vector<int32_t> active((size_t)R), flags((size_t)2 * R);
  for (int r = 0; r < R; ++r) { active[(size_t)r] = r; n_iter[r] = 0; converged[r] = 0; status[r] = 0; }
  SMX_HIP(hipMemcpy(dAct, active.data(), (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice));
  const dim3 block(SMX_GF_TILE);
  hipLaunchKernelGGL(gf_onehot_kernel, dim3(tiles, (unsigned)K, (unsigned)R), block, 0, nullptr, dLab, N, (int)K, dResp);
  SMX_HIP(hipGetLastError());
  const GfMeanArgs ma{dZ, shp, dAct, dResp, dPm, DL};
  const GfScatterArgs sa{dZ, shp, dAct, dResp, dPm, dPt};
  GfCloseArgs ca{shp, dAct, dPm, dPt, reg_covar, tol, 1, (int)tiles, dLbPart, dW, dMu, dCov, dLinv, dLogc, dLb, dFlags, (int)R};
  GfEArgs ea{dZ, N, (int)D, (int)K, dAct, dMu, dLinv, dLogc, dResp, dLbPart, nullptr, nullptr};
  const auto m_step = [&](unsigned nA) -> int {
    hipLaunchKernelGGL(gf_mean_part_kernel, dim3((unsigned)S, (unsigned)K, nA), block, 0, nullptr, ma);
    SMX_HIP(hipGetLastError());
    gf_launch_scatter(T, dim3((unsigned)S, (unsigned)K, nA), sa);
    SMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(gf_close_kernel, dim3((unsigned)K, nA), block, 0, nullptr, ca);
    SMX_HIP(hipGetLastError());
    SMX_HIP(hipMemcpy(flags.data(), dFlags, flags.size() * sizeof(int32_t), hipMemcpyDeviceToHost));   // (waits for the launches)
    return SMX_OK;
  };
  // drops the restarts that failed or stopped; true when the list changed
  const auto sift = [&](int it) {
    std::vector<int32_t> still;
    for (int32_t r : active) {
      n_iter[r] = it;
      if (flags[(size_t)R + r]) status[r] = 1;
      else if (flags[(size_t)r]) converged[r] = 1;
      else still.push_back(r);
    }
    const bool changed = still.size() != active.size();
    active.swap(still);
    return changed;
  };
  SMX_CHECK(m_step((unsigned)R));
  bool list_changed = sift(0);
  ca.initial = 0;
  for (int it = 1; it <= max_iter && !active.empty(); ++it) {
    const unsigned nA = (unsigned)active.size();
    if (list_changed) SMX_HIP(hipMemcpy(dAct, active.data(), nA * sizeof(int32_t), hipMemcpyHostToDevice));   // (no launch is in flight)
    gf_launch_estep(DP, dim3(tiles, nA), ea);
    SMX_HIP(hipGetLastError());
    SMX_CHECK(m_step(nA));
    list_changed = sift(it);
  }
  SMX_HIP(hipMemcpy(lower_bound, dLb, (size_t)R * sizeof(double), hipMemcpyDeviceToHost));
  int bi = -1;
  for (int r = 0; r < R; ++r) {
    if (status[r]) { lower_bound[r] = (double)NAN; continue; }
    if (bi < 0 || lower_bound[r] > lower_bound[bi]) bi = r;   // highest; ties to the lowest r; failed restarts last
  }
  if (params_all) {
    const size_t per = (size_t)K + (size_t)K * D + (size_t)K * DD;
    for (int r = 0; r < R; ++r) {
      double* p = params_all + (size_t)r * per;
      SMX_HIP(hipMemcpy(p, dW + (size_t)r * K, (size_t)K * sizeof(double), hipMemcpyDeviceToHost));
      SMX_HIP(hipMemcpy(p + K, dMu + (size_t)r * K * D, (size_t)K * D * sizeof(double), hipMemcpyDeviceToHost));
      SMX_HIP(hipMemcpy(p + K + (size_t)K * D, dCov + (size_t)r * K * DD, (size_t)K * DD * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  *best = bi < 0 ? 0 : bi;
  if (bi < 0) {
    set_error("gmm_full_fit: every restart met a covariance pivot that is not a positive finite number (an ill-defined empirical covariance)");
    return SMX_ERR_INVALID;
  }
  // the final E-step under the best restart's parameters: its labels
  const int32_t one = bi;
  SMX_HIP(hipMemcpy(dAct, &one, sizeof(int32_t), hipMemcpyHostToDevice));
  ea.lb_part = nullptr; ea.labels = dOut;
  gf_launch_estep(DP, dim3(tiles, 1u), ea);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipMemcpy(labels, dOut, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(weights, dW + (size_t)bi * K, (size_t)K * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(means, dMu + (size_t)bi * K * D, (size_t)K * D * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(covariances, dCov + (size_t)bi * K * DD, (size_t)K * DD * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(chol_inv, dLinv + (size_t)bi * K * DD, (size_t)K * DD * sizeof(double), hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_gmm_full_predict(const float* Z, int64_t n_cells, int32_t D, int32_t K, const double* weights, const double* means, const double* chol_inv,
                         int32_t* labels, double* resp, double* score) {
  using namespace smx;
  SMX_REQUIRE(Z && weights && means && chol_inv && labels, "gmm_full_predict: null argument");
  SMX_CHECK(gf_check_shape("gmm_full_predict", Z, n_cells, D, K));
  const long N = (long)n_cells;
  const size_t DD = (size_t)D * D;
  std::vector<double> logc((size_t)K);
  for (int k = 0; k < K; ++k) {
    SMX_REQUIRE(weights[k] > 0.0 && std::isfinite(weights[k]), "gmm_full_predict: weights must be positive and finite");
    double ld = 0.0;
    for (int i = 0; i < D; ++i) {
      SMX_REQUIRE(std::isfinite(means[(size_t)k * D + i]), "gmm_full_predict: means must be finite");
      for (int j = 0; j < D; ++j) SMX_REQUIRE(std::isfinite(chol_inv[k * DD + (size_t)i * D + j]), "gmm_full_predict: chol_inv must be finite");
      SMX_REQUIRE(chol_inv[k * DD + (size_t)i * D + i] > 0.0, "gmm_full_predict: the diagonal of chol_inv must be positive");
      ld += std::log(chol_inv[k * DD + (size_t)i * D + i]);
    }
    logc[(size_t)k] = std::log(weights[k]) + ld;
  }
  const unsigned tiles = (unsigned)((N + SMX_GF_TILE - 1) / SMX_GF_TILE);
  DeviceScratch buf;
  float* dZ; double *dResp, *dMu, *dLinv, *dLogc, *dScore = nullptr; int32_t *dAct, *dOut;
  SMX_CHECK(buf.get(&dZ, (size_t)N * D)); SMX_CHECK(buf.get(&dResp, (size_t)K * N)); SMX_CHECK(buf.get(&dMu, (size_t)K * D));
  SMX_CHECK(buf.get(&dLinv, K * DD)); SMX_CHECK(buf.get(&dLogc, (size_t)K)); SMX_CHECK(buf.get(&dAct, (size_t)1)); SMX_CHECK(buf.get(&dOut, (size_t)N));
  if (score) SMX_CHECK(buf.get(&dScore, (size_t)N));
  SMX_HIP(hipMemcpy(dZ, Z, (size_t)N * D * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dMu, means, (size_t)K * D * sizeof(double), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dLinv, chol_inv, K * DD * sizeof(double), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dLogc, logc.data(), (size_t)K * sizeof(double), hipMemcpyHostToDevice));   // (dAct is zero: restart 0)
  const GfEArgs ea{dZ, N, (int)D, (int)K, dAct, dMu, dLinv, dLogc, dResp, nullptr, dOut, dScore};
  gf_launch_estep(gf_padded_width(D), dim3(tiles, 1u), ea);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipMemcpy(labels, dOut, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (score) SMX_HIP(hipMemcpy(score, dScore, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  if (resp) {
    std::vector<double> hr((size_t)K * N);
    SMX_HIP(hipMemcpy(hr.data(), dResp, hr.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k)
      for (long i = 0; i < N; ++i) resp[(size_t)i * K + k] = hr[(size_t)k * N + i];
  }
  return SMX_OK;
}

}  // extern "C"
