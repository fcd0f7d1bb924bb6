// smx_gmm.hip -- the Gaussian mixtures of the reference's ProbabilisticEmbedding (sisua/label_threshold.py): one 1-D mixture of K components
// per protein column of a host matrix X [N][C] float32, scikit-learn's GaussianMixture(covariance_type='diag') loop run from R starts per
// column, all C x R jobs of a call together.  Model-free entries: they upload, compute, download and free their own buffers.
//   layout       X is uploaded once, column-major; a launch normalises it into T [C][N] float64 (t = log1p(fl32(fl32(x / den) * 1e4)), den =
//                fl32(s + eps), s the float64 sum of the column in cell order, taken on the host beside the argument checks).  With
//                remove_zeros a zero cell holds -1 in T and is skipped in every pass; ONE synthetic sample t = 0 stands for all of them and is
//                added by thread 0 of slice 0.
//   an iteration one launch over (job, slice of the cells): a thread strides over its slice with 3 K + 1 running sums (sum r, sum r t,
//                sum r t^2 per component, and the log-likelihood); lanes by halving, the four waves as (0 + 1) + (2 + 3), one partial per
//                (job, slice).  A second, tiny launch (one thread per job) adds the slices in index order and closes the M-step: weights,
//                means, variances, the constants of the next E-step, the lower bound and the stop flag |lb - lb_prev| < tol.  The host reads
//                the flags and drops finished jobs from the list, as smx_cluster_kmeans does with its changed counts.
//   the start    the same two launches with one-hot responsibilities: every sample goes to the nearest normalised seed (strict <: ties to the
//                lowest index); the seeds are normalised on the device by the function that normalises the cells.
// The number of slices is a function of N alone, and so is the order of every sum: two calls give the same bits, a job gives the same bits
// alone or in a batch, a column the same bits alone or among others.  No float atomics; every loop is bounded by N, K, the slices or max_iter;
// no workgroup waits on another.
#include "smx_model.h"
#include "smx_block.h"   // the fixed-order wave sum

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <string>

namespace smx {

#define SMX_GM_TILE 256
#define SMX_GM_MAX_K 8
#define SMX_GM_MAX_C 4096
#define SMX_GM_MAX_R 64
#define SMX_GM_SLICE_CELLS 4096   // a slice is at least this many cells ...
#define SMX_GM_MAX_SLICES 64      // ... until there are this many slices

// the reference's _log_norm with its float32 roundings; den = fl32(column sum + eps)
__device__ inline double gm_norm(float x, float den, int log_norm) {
  if (!log_norm) return (double)x;
  const float a = __fmul_rn(__fdiv_rn(x, den), 1e4f);
  return log1p((double)a);
}

// the constants of a component's weighted log-density: lp(t) = A - B (t - mean)^2
__device__ inline void gm_consts(double w, double var, double* A, double* B) {
  *A = log(w) - 0.91893853320467274178 - 0.5 * log(var);   // (0.5 log(2 pi))
  *B = 0.5 / var;
}

// NV running sums of every thread -> out [NV]: smx_block.h's wave sum, then the four waves in its order, NV wide (thread v closes sum v)
template <int NV>
__device__ inline void gm_block_sum(double (&acc)[NV], double* sh, double* out) {
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = halving_wave_sum(acc[v]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) sh[(threadIdx.x >> 6) * NV + v] = acc[v];
  }
  __syncthreads();
  if (threadIdx.x < NV) out[threadIdx.x] = (sh[threadIdx.x] + sh[NV + threadIdx.x]) + (sh[2 * NV + threadIdx.x] + sh[3 * NV + threadIdx.x]);
}

__global__ __launch_bounds__(SMX_GM_TILE) void gm_normalize_kernel(const float* X, long N, const float* den, int log_norm, int remove_zeros,
                                                                   double* T) {
  const long i = (long)blockIdx.x * SMX_GM_TILE + threadIdx.x;
  const long c = blockIdx.y;
  if (i >= N) return;
  const float x = X[c * N + i];
  T[c * N + i] = (remove_zeros && !(x > 0.f)) ? -1.0 : gm_norm(x, den[c], log_norm);
}

struct GmArgs {
  const double* T;          // [C][N]; < 0: not a sample
  long N, slice_len;
  int S, R;
  const int32_t* active;    // the jobs of this launch (grid x); job = column * R + restart
  const float* init_raw;    // [C R][K]
  const float* den;         // [C]
  int log_norm;
  const int32_t* has_zero;  // [C]: the synthetic sample 0 is part of the column's training set
  const double* params;     // [C R][5 K]: weights, means, variances, A, B
  double* part;             // [C R][S][3 K + 1]
};

template <int K>
__global__ __launch_bounds__(SMX_GM_TILE) void gm_init_kernel(GmArgs a) {
  constexpr int NV = 3 * K + 1;
  __shared__ double sh[4 * NV];
  const long job = a.active[blockIdx.x];
  const long c = job / a.R;
  const int s = blockIdx.y;
  double seed[K], acc[NV];
#pragma unroll
  for (int k = 0; k < K; ++k) seed[k] = gm_norm(a.init_raw[job * K + k], a.den[c], a.log_norm);
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  auto add = [&](double t) {
    int best = 0;
    double bd = fabs(t - seed[0]);
#pragma unroll
    for (int k = 1; k < K; ++k) {
      const double d = fabs(t - seed[k]);
      if (d < bd) { bd = d; best = k; }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (k == best) { acc[3 * k] += 1.0; acc[3 * k + 1] += t; acc[3 * k + 2] = fma(t, t, acc[3 * k + 2]); }
  };
  if (s == 0 && threadIdx.x == 0 && a.has_zero[c]) add(0.0);
  const double* t = a.T + c * a.N;
  const long i0 = (long)s * a.slice_len, i1 = min(a.N, i0 + a.slice_len);
  for (long i = i0 + threadIdx.x; i < i1; i += SMX_GM_TILE) {
    const double v = t[i];
    if (v >= 0.0) add(v);
  }
  gm_block_sum<NV>(acc, sh, a.part + (job * a.S + s) * NV);
}

template <int K>
__global__ __launch_bounds__(SMX_GM_TILE) void gm_em_kernel(GmArgs a) {
  constexpr int NV = 3 * K + 1;
  __shared__ double sh[4 * NV];
  const long job = a.active[blockIdx.x];
  const long c = job / a.R;
  const int s = blockIdx.y;
  const double* p = a.params + job * 5 * K;
  double mean[K], A[K], B[K], acc[NV];
#pragma unroll
  for (int k = 0; k < K; ++k) { mean[k] = p[K + k]; A[k] = p[3 * K + k]; B[k] = p[4 * K + k]; }
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  auto add = [&](double t) {
    double e[K], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double d = t - mean[k];
      e[k] = A[k] - B[k] * (d * d);
      mx = fmax(mx, e[k]);
    }
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { e[k] = exp(e[k] - mx); se += e[k]; }
    acc[3 * K] += mx + log(se);
    const double tt = t * t;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double r = e[k] / se;
      acc[3 * k] += r; acc[3 * k + 1] = fma(r, t, acc[3 * k + 1]); acc[3 * k + 2] = fma(r, tt, acc[3 * k + 2]);
    }
  };
  if (s == 0 && threadIdx.x == 0 && a.has_zero[c]) add(0.0);
  const double* t = a.T + c * a.N;
  const long i0 = (long)s * a.slice_len, i1 = min(a.N, i0 + a.slice_len);
  for (long i = i0 + threadIdx.x; i < i1; i += SMX_GM_TILE) {
    const double v = t[i];
    if (v >= 0.0) add(v);
  }
  gm_block_sum<NV>(acc, sh, a.part + (job * a.S + s) * NV);
}

struct GmStepArgs {
  const int32_t* active; int n_active;
  int K, S, R, initial;
  const double* part;       // [C R][S][3 K + 1]
  const double* n_train;    // [C]
  double reg_covar, tol;
  double* params;           // [C R][5 K]
  double* lb;               // [C R]
  int32_t* stop;            // [C R]
};

// one thread per job: the slices in index order, then scikit-learn's M-step and stop rule
__global__ __launch_bounds__(SMX_GM_TILE) void gm_mstep_kernel(GmStepArgs a) {
  const int q = blockIdx.x * SMX_GM_TILE + threadIdx.x;
  if (q >= a.n_active) return;
  const long job = a.active[q];
  const int K = a.K, NV = 3 * a.K + 1;
  const double n = a.n_train[job / a.R];
  const double* p = a.part + job * a.S * NV;
  double* out = a.params + job * 5 * K;
  for (int k = 0; k < K; ++k) {
    double sr = 0.0, srt = 0.0, srt2 = 0.0;
    for (int s = 0; s < a.S; ++s) { sr += p[s * NV + 3 * k]; srt += p[s * NV + 3 * k + 1]; srt2 += p[s * NV + 3 * k + 2]; }
    const double nk = sr + 10.0 * DBL_EPSILON;
    const double mean = srt / nk;
    const double var = fma(-mean, mean, srt2 / nk) + a.reg_covar;
    const double w = nk / n;
    double A, B;
    gm_consts(w, var, &A, &B);
    out[k] = w; out[K + k] = mean; out[2 * K + k] = var; out[3 * K + k] = A; out[4 * K + k] = B;
  }
  if (a.initial) { a.lb[job] = -INFINITY; a.stop[job] = 0; return; }
  double ll = 0.0;
  for (int s = 0; s < a.S; ++s) ll += p[s * NV + 3 * K];
  const double lb = ll / n;
  a.stop[job] = fabs(lb - a.lb[job]) < a.tol ? 1 : 0;
  a.lb[job] = lb;
}

struct GmPredictArgs {
  const float* X;           // [C][N]
  long N;
  const float* den;
  int log_norm, pos;
  const double* par;        // [C][3][K]: weights, means, variances
  const int32_t* order;     // [C][K]: components by increasing mean
  const double* thr;        // [C]
  double* prob;             // [C][N]
  float* bin;               // [C][N]
  double* score;            // [C][N] or null
};

template <int K>
__global__ __launch_bounds__(SMX_GM_TILE) void gm_predict_kernel(GmPredictArgs a) {
  __shared__ double shM[K], shA[K], shB[K], shSel[K];
  const long c = blockIdx.y;
  if (threadIdx.x < K) {
    const double* p = a.par + c * 3 * K;
    shM[threadIdx.x] = p[K + threadIdx.x];
    gm_consts(p[threadIdx.x], p[2 * K + threadIdx.x], &shA[threadIdx.x], &shB[threadIdx.x]);
    shSel[a.order[c * K + threadIdx.x]] = (int)threadIdx.x >= a.pos ? 1.0 : 0.0;   // (order is a permutation: checked by the host)
  }
  __syncthreads();
  const long i = (long)blockIdx.x * SMX_GM_TILE + threadIdx.x;
  if (i >= a.N) return;
  const double t = gm_norm(a.X[c * a.N + i], a.den[c], a.log_norm);
  double e[K], mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double d = t - shM[k];
    e[k] = shA[k] - shB[k] * (d * d);
    mx = fmax(mx, e[k]);
  }
  double se = 0.0, sel = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) { e[k] = exp(e[k] - mx); se += e[k]; }
#pragma unroll
  for (int k = 0; k < K; ++k) sel += shSel[k] * (e[k] / se);
  a.prob[c * a.N + i] = sel / (double)(K - a.pos);
  a.bin[c * a.N + i] = t >= a.thr[c] ? 1.f : 0.f;
  if (a.score) a.score[c * a.N + i] = mx + log(se);
}

static int gm_slices(long N) {
  return (int)std::max<long>(1, std::min<long>(SMX_GM_MAX_SLICES, (N + SMX_GM_SLICE_CELLS - 1) / SMX_GM_SLICE_CELLS));
}

#define SMX_GM_DISPATCH(kernel, K, grid, args)                                                                     \
  switch (K) {                                                                                                     \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(SMX_GM_TILE), 0, nullptr, args); break;                       \
    case 3: hipLaunchKernelGGL(kernel<3>, grid, dim3(SMX_GM_TILE), 0, nullptr, args); break;                       \
    case 4: hipLaunchKernelGGL(kernel<4>, grid, dim3(SMX_GM_TILE), 0, nullptr, args); break;                       \
    case 5: hipLaunchKernelGGL(kernel<5>, grid, dim3(SMX_GM_TILE), 0, nullptr, args); break;                       \
    case 6: hipLaunchKernelGGL(kernel<6>, grid, dim3(SMX_GM_TILE), 0, nullptr, args); break;                       \
    case 7: hipLaunchKernelGGL(kernel<7>, grid, dim3(SMX_GM_TILE), 0, nullptr, args); break;                       \
    default: hipLaunchKernelGGL(kernel<8>, grid, dim3(SMX_GM_TILE), 0, nullptr, args); break;                      \
  }

// X [N][C] -> Xc [C][N]; per column: the float64 sum in cell order, the number of positive cells.  Refuses a negative or non-finite entry.
static int gm_columns(const char* who, const float* X, long N, int C, std::vector<float>& Xc, std::vector<double>& sum, std::vector<long>& n_pos) {
  Xc.resize((size_t)N * C);
  sum.assign((size_t)C, 0.0);
  n_pos.assign((size_t)C, 0);
  for (long i = 0; i < N; ++i)
    for (int c = 0; c < C; ++c) {
      const float v = X[(size_t)i * C + c];
      if (!(v >= 0.f) || std::isinf(v)) {
        set_error(std::string(who) + ": X holds a negative or non-finite entry (column " + std::to_string(c) + ", cell " + std::to_string(i) + ")");
        return SMX_ERR_INVALID;
      }
      Xc[(size_t)c * N + i] = v;
      sum[(size_t)c] += (double)v;
      n_pos[(size_t)c] += v > 0.f;
    }
  return SMX_OK;
}

static float gm_den(double sum, int log_norm) { return log_norm ? (float)(sum + (double)FLT_EPSILON) : 1.f; }

}  // namespace smx

extern "C" {

int smx_gmm1d_fit(const float* X, int64_t n_cells, int32_t C, int32_t K, const float* init_raw, int32_t R, int32_t max_iter, double tol,
                  double reg_covar, int32_t remove_zeros, int32_t log_norm, double* lower_bound, int32_t* n_iter, int32_t* converged,
                  int32_t* best, double* weights, double* means, double* variances, int64_t* n_train, double* col_sum, double* params_all,
                  double* stats) {
  using namespace smx;
  SMX_REQUIRE(X && init_raw && lower_bound && n_iter && converged && best && weights && means && variances && n_train && col_sum,
              "gmm1d_fit: null argument");
  SMX_REQUIRE(C >= 1 && C <= SMX_GM_MAX_C, "gmm1d_fit: 1 <= C <= 4096");
  SMX_REQUIRE(K >= 2 && K <= SMX_GM_MAX_K, "gmm1d_fit: 2 <= K <= 8");
  SMX_REQUIRE(R >= 1 && R <= SMX_GM_MAX_R, "gmm1d_fit: 1 <= R <= 64");
  SMX_REQUIRE(n_cells >= 1 && n_cells < ((int64_t)1 << 31), "gmm1d_fit: 1 <= n_cells < 2^31");
  SMX_REQUIRE(max_iter >= 1, "gmm1d_fit: max_iter >= 1");
  SMX_REQUIRE(tol > 0.0 && std::isfinite(tol), "gmm1d_fit: tol > 0");
  SMX_REQUIRE(reg_covar >= 0.0 && std::isfinite(reg_covar), "gmm1d_fit: reg_covar >= 0");
  const auto t_begin = std::chrono::steady_clock::now();
  const long N = (long)n_cells;
  const size_t CR = (size_t)C * R;
  std::vector<float> Xc, den((size_t)C);
  std::vector<double> sum, ntr((size_t)C);
  std::vector<long> n_pos;
  std::vector<int32_t> has_zero((size_t)C);
  SMX_CHECK(gm_columns("gmm1d_fit", X, N, C, Xc, sum, n_pos));
  for (int c = 0; c < C; ++c) {
    has_zero[(size_t)c] = remove_zeros && n_pos[(size_t)c] < N;
    const long nt = remove_zeros ? n_pos[(size_t)c] + has_zero[(size_t)c] : N;
    if (nt < K) {
      set_error("gmm1d_fit: column " + std::to_string(c) + " has " + std::to_string(nt) + " training samples, fewer than K = " + std::to_string(K));
      return SMX_ERR_INVALID;
    }
    n_train[c] = nt; ntr[(size_t)c] = (double)nt; col_sum[c] = sum[(size_t)c]; den[(size_t)c] = gm_den(sum[(size_t)c], log_norm);
  }
  for (size_t e = 0; e < CR * K; ++e) SMX_REQUIRE(init_raw[e] >= 0.f && !std::isinf(init_raw[e]), "gmm1d_fit: a negative or non-finite init_raw");
  const int S = gm_slices(N), NV = 3 * K + 1;
  const long slice_len = ((N + S - 1) / S + SMX_GM_TILE - 1) / SMX_GM_TILE * SMX_GM_TILE;
  DeviceScratch buf;
  float *dX, *dDen, *dInit; double *dT, *dNtr, *dPart, *dPar, *dLb; int32_t *dZero, *dAct, *dStop;
  SMX_CHECK(buf.get(&dX, (size_t)N * C)); SMX_CHECK(buf.get(&dT, (size_t)N * C)); SMX_CHECK(buf.get(&dDen, (size_t)C));
  SMX_CHECK(buf.get(&dInit, CR * K)); SMX_CHECK(buf.get(&dNtr, (size_t)C)); SMX_CHECK(buf.get(&dPart, CR * S * NV));
  SMX_CHECK(buf.get(&dPar, CR * 5 * K)); SMX_CHECK(buf.get(&dLb, CR)); SMX_CHECK(buf.get(&dZero, (size_t)C)); SMX_CHECK(buf.get(&dAct, CR));
  SMX_CHECK(buf.get(&dStop, CR));
  SMX_HIP(hipMemcpy(dX, Xc.data(), Xc.size() * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dDen, den.data(), den.size() * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dInit, init_raw, CR * K * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dNtr, ntr.data(), ntr.size() * sizeof(double), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dZero, has_zero.data(), has_zero.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  std::vector<int32_t> active(CR), stop(CR);
  for (size_t j = 0; j < CR; ++j) { active[j] = (int32_t)j; n_iter[j] = 0; converged[j] = 0; }
  SMX_HIP(hipMemcpy(dAct, active.data(), CR * sizeof(int32_t), hipMemcpyHostToDevice));
  const unsigned tiles = (unsigned)((N + SMX_GM_TILE - 1) / SMX_GM_TILE);
  hipLaunchKernelGGL(gm_normalize_kernel, dim3(tiles, (unsigned)C), dim3(SMX_GM_TILE), 0, nullptr, dX, N, dDen, (int)log_norm, (int)remove_zeros, dT);
  SMX_HIP(hipGetLastError());
  const GmArgs ga{dT, N, slice_len, S, R, dAct, dInit, dDen, (int)log_norm, dZero, dPar, dPart};
  GmStepArgs sa{dAct, (int)CR, K, S, R, 1, dPart, dNtr, reg_covar, tol, dPar, dLb, dStop};
  const auto step_grid = [](size_t n) { return dim3((unsigned)((n + SMX_GM_TILE - 1) / SMX_GM_TILE)); };
  SMX_GM_DISPATCH(gm_init_kernel, K, dim3((unsigned)CR, (unsigned)S), ga);
  SMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(gm_mstep_kernel, step_grid(CR), dim3(SMX_GM_TILE), 0, nullptr, sa);
  SMX_HIP(hipGetLastError());
  sa.initial = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double kernel_ms = 0.0;
  long launches = 3, trips = 0;
  if (stats) { SMX_HIP(hipEventCreate(&ev0)); SMX_HIP(hipEventCreate(&ev1)); }
  struct EventGuard { hipEvent_t &a, &b; ~EventGuard() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); } } guard{ev0, ev1};
  SMX_HIP(hipDeviceSynchronize());
  const auto t_loop = std::chrono::steady_clock::now();
  bool list_changed = false;
  for (int it = 1; it <= max_iter && !active.empty(); ++it) {
    const size_t nA = active.size();
    if (list_changed) SMX_HIP(hipMemcpy(dAct, active.data(), nA * sizeof(int32_t), hipMemcpyHostToDevice));   // (no launch is in flight)
    if (stats) SMX_HIP(hipEventRecord(ev0, nullptr));
    SMX_GM_DISPATCH(gm_em_kernel, K, dim3((unsigned)nA, (unsigned)S), ga);
    SMX_HIP(hipGetLastError());
    sa.n_active = (int)nA;
    hipLaunchKernelGGL(gm_mstep_kernel, step_grid(nA), dim3(SMX_GM_TILE), 0, nullptr, sa);
    SMX_HIP(hipGetLastError());
    if (stats) SMX_HIP(hipEventRecord(ev1, nullptr));
    SMX_HIP(hipMemcpy(stop.data(), dStop, CR * sizeof(int32_t), hipMemcpyDeviceToHost));   // (waits for the launches)
    launches += 2; ++trips;
    if (stats) { float ms = 0.f; SMX_HIP(hipEventElapsedTime(&ms, ev0, ev1)); kernel_ms += ms; }
    std::vector<int32_t> still;
    for (int32_t j : active) {
      n_iter[j] = it;
      if (stop[(size_t)j]) converged[j] = 1; else still.push_back(j);
    }
    list_changed = still.size() != nA;
    active.swap(still);
  }
  const auto t_end_loop = std::chrono::steady_clock::now();
  std::vector<double> par(CR * 5 * K);
  SMX_HIP(hipMemcpy(par.data(), dPar, par.size() * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(lower_bound, dLb, CR * sizeof(double), hipMemcpyDeviceToHost));
  for (int c = 0; c < C; ++c) {
    const double* lb = lower_bound + (size_t)c * R;
    int bi = 0;
    for (int r = 1; r < R; ++r)
      if (lb[r] > lb[bi] || (lb[bi] != lb[bi] && lb[r] == lb[r])) bi = r;   // highest; ties to the lowest r; NaN last
    best[c] = bi;
    const double* p = par.data() + ((size_t)c * R + bi) * 5 * K;
    for (int k = 0; k < K; ++k) { weights[(size_t)c * K + k] = p[k]; means[(size_t)c * K + k] = p[K + k]; variances[(size_t)c * K + k] = p[2 * K + k]; }
  }
  if (params_all)
    for (size_t j = 0; j < CR; ++j) std::copy(par.begin() + j * 5 * K, par.begin() + j * 5 * K + 3 * K, params_all + j * 3 * K);
  if (stats) {
    const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    stats[0] = (double)launches; stats[1] = (double)trips; stats[2] = kernel_ms; stats[3] = ms(t_loop, t_end_loop);
    stats[4] = ms(t_begin, std::chrono::steady_clock::now());
  }
  return SMX_OK;
}

int smx_gmm1d_predict(const float* X, int64_t n_cells, int32_t C, int32_t K, const double* weights, const double* means, const double* variances,
                      const int32_t* order, int32_t positive_component, const double* threshold, int32_t log_norm, double* prob, float* bin,
                      double* score) {
  using namespace smx;
  SMX_REQUIRE(X && weights && means && variances && order && threshold && prob && bin, "gmm1d_predict: null argument");
  SMX_REQUIRE(C >= 1 && C <= SMX_GM_MAX_C, "gmm1d_predict: 1 <= C <= 4096");
  SMX_REQUIRE(K >= 2 && K <= SMX_GM_MAX_K, "gmm1d_predict: 2 <= K <= 8");
  SMX_REQUIRE(positive_component >= 1 && positive_component < K, "gmm1d_predict: 1 <= positive_component < K");
  SMX_REQUIRE(n_cells >= 1 && n_cells < ((int64_t)1 << 31), "gmm1d_predict: 1 <= n_cells < 2^31");
  const long N = (long)n_cells;
  const size_t CK = (size_t)C * K;
  std::vector<double> par(CK * 3);
  for (int c = 0; c < C; ++c) {
    unsigned seen = 0;
    for (int k = 0; k < K; ++k) {
      const size_t e = (size_t)c * K + k;
      SMX_REQUIRE(order[e] >= 0 && order[e] < K && !(seen >> order[e] & 1u), "gmm1d_predict: order is not a permutation of 0 .. K - 1");
      seen |= 1u << order[e];
      SMX_REQUIRE(weights[e] > 0.0 && std::isfinite(weights[e]) && std::isfinite(means[e]) && variances[e] > 0.0 && std::isfinite(variances[e]),
                  "gmm1d_predict: weights and variances must be positive and finite, means finite");
      par[(size_t)c * 3 * K + k] = weights[e]; par[(size_t)c * 3 * K + K + k] = means[e]; par[(size_t)c * 3 * K + 2 * K + k] = variances[e];
    }
    SMX_REQUIRE(threshold[c] == threshold[c], "gmm1d_predict: a NaN threshold");
  }
  std::vector<float> Xc, den((size_t)C);
  std::vector<double> sum;
  std::vector<long> n_pos;
  SMX_CHECK(gm_columns("gmm1d_predict", X, N, C, Xc, sum, n_pos));
  for (int c = 0; c < C; ++c) den[(size_t)c] = gm_den(sum[(size_t)c], log_norm);
  DeviceScratch buf;
  float *dX, *dDen, *dBin; double *dPar, *dThr, *dProb, *dScore = nullptr; int32_t* dOrd;
  SMX_CHECK(buf.get(&dX, (size_t)N * C)); SMX_CHECK(buf.get(&dDen, (size_t)C)); SMX_CHECK(buf.get(&dBin, (size_t)N * C));
  SMX_CHECK(buf.get(&dPar, par.size())); SMX_CHECK(buf.get(&dThr, (size_t)C)); SMX_CHECK(buf.get(&dProb, (size_t)N * C));
  SMX_CHECK(buf.get(&dOrd, CK));
  if (score) SMX_CHECK(buf.get(&dScore, (size_t)N * C));
  SMX_HIP(hipMemcpy(dX, Xc.data(), Xc.size() * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dDen, den.data(), den.size() * sizeof(float), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dPar, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dThr, threshold, (size_t)C * sizeof(double), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(dOrd, order, CK * sizeof(int32_t), hipMemcpyHostToDevice));
  const GmPredictArgs pa{dX, N, dDen, (int)log_norm, (int)positive_component, dPar, dOrd, dThr, dProb, dBin, dScore};
  const dim3 grid((unsigned)((N + SMX_GM_TILE - 1) / SMX_GM_TILE), (unsigned)C);
  SMX_GM_DISPATCH(gm_predict_kernel, K, grid, pa);
  SMX_HIP(hipGetLastError());
  std::vector<double> hp((size_t)N * C);
  std::vector<float> hb((size_t)N * C);
  SMX_HIP(hipMemcpy(hp.data(), dProb, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(hb.data(), dBin, hb.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int c = 0; c < C; ++c)
    for (long i = 0; i < N; ++i) { prob[(size_t)i * C + c] = hp[(size_t)c * N + i]; bin[(size_t)i * C + c] = hb[(size_t)c * N + i]; }
  if (score) {
    SMX_HIP(hipMemcpy(hp.data(), dScore, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int c = 0; c < C; ++c)
      for (long i = 0; i < N; ++i) score[(size_t)i * C + c] = hp[(size_t)c * N + i];
  }
  return SMX_OK;
}

}  // extern "C"
