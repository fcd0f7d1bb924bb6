// smx_logreg.hip -- L2-penalised logistic regression on the count matrix: what the reference's SingleCellOMIC.rank_vars_groups(method=
// 'logreg') asks of scikit-learn's LogisticRegression through scanpy (_single_cell_analysis.py:862-918), as a deterministic full-batch
// solve.  Model-free entries: they upload, compute, download and free their own buffers.
//   the objective     scikit-learn's in its mean form, F(W, b) = (1/N) sum_i loss_i + ||W||^2 / (2 C N), the intercept unpenalised.
//                     multinomial (K >= 3): K logit rows, loss_i = logsumexp(z_i) - z_{i, y_i}.  binary (2 classes): ONE stored logit row
//                     (class 1) beside an implicit zero logit, loss_i = softplus(z_i) - y_i z_i -- the same kernels with the zero logit
//                     joining the max and the sum.  Everything is float64 from the float32 tile on.
//   the parameters    one device vector theta [Kz x ld + Kp]: W [Kz][ld] (Kz logit rows, ld = n_genes rounded up to 4, padding zero and
//                     with a zero gradient) and behind it b [Kp], Kp = Kz rounded up to 4.  The gradient has the same layout.
//   the row sweep     the structure of smx_mbkmeans.hip's sweep_rows with a dot product in the place of the squared distance: a wave takes
//                     4 rows, a lane 4 columns of every 256, 4 classes at a time, 16 float64 accumulators fma((double)x, w, acc) from 0,
//                     each lane its columns in rising order, the 64 lanes by halving; the intercept is added last.  The wave keeps its rows'
//                     logits in LDS; then lane l takes the classes l, l + 64, ..: the max, sum exp(z - max) (a lane in rising order, the
//                     lanes by halving, the implicit zero logit last in lane 0), the loss in lane 0 and the residuals r_ik = p_ik -
//                     [y_i = k] -> R [N][Kp].  A workgroup's 16 losses: the rows of a wave in order, the waves as (0 + 1) + (2 + 3).
//   the gradient      one wave per (slice of SMX_PREP_SLICE rows, 256 columns, 4 classes): the slice's residuals go to LDS once and are
//                     read back as broadcasts, the rows are added in row order onto 16 accumulators per lane -> partials [slices][Kz][ld];
//                     the combine launch adds them in slice order, scales by 1/N, adds w / (C N), and also leaves the intercept's
//                     gradient (thread t the rows t, t + 256, .., then the workgroup by halving) and per-workgroup partials of ||W||^2 and
//                     max|g|.  One workgroup closes F and max|g| from the partials.  Four launches per evaluation, no atomics.
//   the solver        L-BFGS, memory 10, on the device vectors: the host keeps the Gram matrix of the basis {s_j, y_j, g} (one launch per
//                     iteration for the new rows: a workgroup per dot product, fixed order), runs the two-loop recursion on coefficients
//                     over that basis, and one launch forms the direction.  Armijo backtracking (c1 = 1e-4): first trial 1, or 1 / max|g|
//                     on the first iteration, halved at each failure, at most 30 trials; a trial with |F_new - F| <= 2^-43 |F| (the
//                     rounding of two evaluations) is accepted if it lowers max|g|.  A pair with s.y <= 0 is skipped.
// Every loop is bounded by N, ld, K, max_iter, the memory or the 30 trials.
#include "smx_model.h"
#include "smx_prep.h"    // the block streamer of the count matrix
#include "smx_block.h"   // the fixed-order sums

#include <algorithm>
#include <cmath>
#include <vector>

namespace smx {

#define SMX_LR_MAX_CLASSES 256
#define SMX_LR_MAX_GENES 32768
#define SMX_LR_MAX_RESIDENT ((size_t)1 << 31)   // the whole matrix is held in the tile: rows x ld floats (8 GB)
#define LR_ROWS 4                               // rows of a wave
#define LR_CLASSES 4                            // logit rows a wave holds at once
#define LR_CHUNK 256                            // columns of one trip of a wave: 64 lanes x 4
#define LR_MEMORY 10                            // pairs of the L-BFGS history
#define LR_SLOTS (LR_MEMORY + 1)                // ... and one more to write the next pair into before it is accepted
#define LR_NV (2 * LR_SLOTS + 1)                // the basis: s slots, y slots, the gradient
#define LR_TRIALS 30
#define LR_ARMIJO 1e-4
#define LR_FLAT 0x1p-43                         // two evaluations of F differ by their rounding alone below this share of |F|

__device__ __forceinline__ double wave_max_f64(double v) {   // in every lane
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// the tile's rows [0, nb) against W [Kz][ld], b [Kz].  logits != NULL: logits [row0 + row][Kz] and nothing else.  Otherwise R [row][Kp]
// and the workgroup's loss partial.
__global__ __launch_bounds__(256) void lr_rows_kernel(const float* __restrict__ tile, long nb, long ld, const double* __restrict__ W,
                                                      const double* __restrict__ b, int Kz, int binary, const int32_t* __restrict__ y,
                                                      int Kp, double* __restrict__ R, double* __restrict__ losspart, long row0,
                                                      double* __restrict__ logits) {
  __shared__ double zs[4][LR_ROWS][SMX_LR_MAX_CLASSES];
  __shared__ double l4[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long r0 = ((long)blockIdx.x * 4 + w) * LR_ROWS;
  double lsum = 0.0;
  if (r0 < nb) {   // (wave-uniform)
    const float* xr[LR_ROWS];
#pragma unroll
    for (int q = 0; q < LR_ROWS; ++q) xr[q] = tile + (r0 + q < nb ? r0 + q : nb - 1) * ld;   // (a ragged tile: the last row again, not used)
    for (int k0 = 0; k0 < Kz; k0 += LR_CLASSES) {
      const double* wr[LR_CLASSES];
#pragma unroll
      for (int p = 0; p < LR_CLASSES; ++p) wr[p] = W + (long)(k0 + p < Kz ? k0 + p : Kz - 1) * ld;
      double acc[LR_ROWS][LR_CLASSES];
#pragma unroll
      for (int q = 0; q < LR_ROWS; ++q)
#pragma unroll
        for (int p = 0; p < LR_CLASSES; ++p) acc[q][p] = 0.0;
      for (long j = (long)lane * 4; j < ld; j += LR_CHUNK) {   // (ld is a multiple of 4; the padding is zero on both sides)
        double x[LR_ROWS][4];
#pragma unroll
        for (int q = 0; q < LR_ROWS; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(xr[q] + j);
          x[q][0] = (double)v.x; x[q][1] = (double)v.y; x[q][2] = (double)v.z; x[q][3] = (double)v.w;
        }
#pragma unroll
        for (int p = 0; p < LR_CLASSES; ++p) {
          const double2 c01 = *reinterpret_cast<const double2*>(wr[p] + j), c23 = *reinterpret_cast<const double2*>(wr[p] + j + 2);
          const double c[4] = {c01.x, c01.y, c23.x, c23.y};
#pragma unroll
          for (int q = 0; q < LR_ROWS; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[q][p] = fma(x[q][e], c[e], acc[q][p]);
        }
      }
#pragma unroll
      for (int p = 0; p < LR_CLASSES; ++p)
#pragma unroll
        for (int q = 0; q < LR_ROWS; ++q) {
          const double s = halving_wave_sum(acc[q][p]);
          if (lane == 0 && k0 + p < Kz) zs[w][q][k0 + p] = s + b[k0 + p];   // (the intercept last)
        }
    }
    wave_lds_sync();
    for (int q = 0; q < LR_ROWS && r0 + q < nb; ++q) {   // (wave-uniform)
      const long row = r0 + q;
      if (logits) {
        for (int k = lane; k < Kz; k += 64) logits[(row0 + row) * Kz + k] = zs[w][q][k];
        continue;
      }
      double m = binary ? 0.0 : -INFINITY;   // (binary: the implicit zero logit)
      for (int k = lane; k < Kz; k += 64) m = fmax(m, zs[w][q][k]);
      m = wave_max_f64(m);
      double e = 0.0;
      for (int k = lane; k < Kz; k += 64) e += exp(zs[w][q][k] - m);
      if (binary && lane == 0) e += exp(0.0 - m);
      const double s = __shfl(halving_wave_sum(e), 0, 64);
      const int yi = y[row];
      for (int k = lane; k < Kz; k += 64) {
        const double hit = (binary ? yi == 1 : yi == k) ? 1.0 : 0.0;
        R[row * Kp + k] = __dsub_rn(__ddiv_rn(exp(zs[w][q][k] - m), s), hit);
      }
      if (lane == 0) {
        const double zy = binary ? (yi == 1 ? zs[w][q][0] : 0.0) : zs[w][q][yi];
        lsum += __dsub_rn(__dadd_rn(m, log(s)), zy);
      }
    }
  }
  if (logits) return;   // (uniform over the launch)
  if (lane == 0) l4[w] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) losspart[blockIdx.x] = (l4[0] + l4[1]) + (l4[2] + l4[3]);
}

// slice blockIdx.x (SMX_PREP_SLICE rows), columns 256 blockIdx.y + 4 lane .. + 3, classes 4 blockIdx.z .. + 3: sum_i r_ik x_ij in row order
__global__ __launch_bounds__(64) void lr_grad_kernel(const float* __restrict__ tile, long N, long ld, const double* __restrict__ R, int Kp,
                                                     int Kz, double* __restrict__ part) {
  __shared__ double rs[SMX_PREP_SLICE][LR_CLASSES];
  const int lane = threadIdx.x, k0 = (int)blockIdx.z * LR_CLASSES;
  const long i0 = (long)blockIdx.x * SMX_PREP_SLICE, j = ((long)blockIdx.y * 64 + lane) * 4;
  const int n = (int)(N - i0 < SMX_PREP_SLICE ? N - i0 : SMX_PREP_SLICE);
  const bool live = j < ld;
  if (lane < n) {
    const double* r = R + (i0 + lane) * Kp + k0;   // (Kp and k0 are multiples of 4: 32-byte aligned)
    const double2 a = *reinterpret_cast<const double2*>(r), c = *reinterpret_cast<const double2*>(r + 2);
    rs[lane][0] = a.x; rs[lane][1] = a.y; rs[lane][2] = c.x; rs[lane][3] = c.y;
  }
  wave_lds_sync();
  double acc[LR_CLASSES][4];
#pragma unroll
  for (int p = 0; p < LR_CLASSES; ++p)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[p][e] = 0.0;
  for (int t = 0; t < n; ++t) {
    const float4 v = live ? *reinterpret_cast<const float4*>(tile + (i0 + t) * ld + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    const double x[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
    for (int p = 0; p < LR_CLASSES; ++p) {
      const double r = rs[t][p];   // (wave-uniform: a broadcast read)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[p][e] = fma(r, x[e], acc[p][e]);
    }
  }
  if (live)
#pragma unroll
    for (int p = 0; p < LR_CLASSES; ++p)
      if (k0 + p < Kz) {
        double* o = part + ((long)blockIdx.x * Kz + k0 + p) * ld + j;
        *reinterpret_cast<double2*>(o) = make_double2(acc[p][0], acc[p][1]);
        *reinterpret_cast<double2*>(o + 2) = make_double2(acc[p][2], acc[p][3]);
      }
}

__device__ __forceinline__ double block_max_f64(double v, double* sh4) {   // in every thread; sh4 as halving_block_sum's
  v = wave_max_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(sh4[0], sh4[1]), fmax(sh4[2], sh4[3]));
}

// blockIdx.y < Kz: columns 256 blockIdx.x .. of class blockIdx.y: g = (the partials in slice order) / N + w / (C N), and the workgroup's
// sum of w^2 and max |g|.  blockIdx.y == Kz: the intercept's gradient of the classes blockIdx.x, blockIdx.x + gridDim.x, ..
__global__ __launch_bounds__(256) void lr_combine_kernel(const double* __restrict__ part, long slices, long ld, int Kz, int Kp, long N,
                                                         const double* __restrict__ R, const double* __restrict__ theta, double invN,
                                                         double lam, int fit_intercept, double* __restrict__ g, double* __restrict__ wsqpart,
                                                         double* __restrict__ gmaxpart) {
  __shared__ double s4[4];
  const int k = blockIdx.y;
  const long slot = (long)k * gridDim.x + blockIdx.x;
  if (k < Kz) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    double gv = 0.0, wv = 0.0;
    if (j < ld) {
      double acc = 0.0;
      for (long s = 0; s < slices; ++s) acc += part[(s * Kz + k) * ld + j];
      wv = theta[(long)k * ld + j];
      gv = __dadd_rn(__dmul_rn(acc, invN), __dmul_rn(wv, lam));
      g[(long)k * ld + j] = gv;
    }
    const double wsq = halving_block_sum(__dmul_rn(wv, wv), s4);
    const double gm = block_max_f64(fabs(gv), s4);
    if (threadIdx.x == 0) { wsqpart[slot] = wsq; gmaxpart[slot] = gm; }
    return;
  }
  double gm = 0.0;
  for (int c = blockIdx.x; c < Kz; c += gridDim.x) {   // (uniform)
    double v = 0.0;
    if (fit_intercept)
      for (long i = threadIdx.x; i < N; i += 256) v += R[i * Kp + c];
    v = __dmul_rn(halving_block_sum(v, s4), invN);
    if (threadIdx.x == 0) g[(long)Kz * ld + c] = v;
    gm = fmax(gm, fabs(v));
  }
  if (threadIdx.x == 0) { wsqpart[slot] = 0.0; gmaxpart[slot] = gm; }
}

// ONE workgroup: out[0] = F, out[1] = max|g|, out[2] = the sum of the losses
__global__ __launch_bounds__(256) void lr_close_kernel(const double* __restrict__ losspart, long n_loss, const double* __restrict__ wsqpart,
                                                       const double* __restrict__ gmaxpart, long n_part, double invN, double lam,
                                                       double* __restrict__ out) {
  __shared__ double s4[4];
  const double loss = halving_column_sum(losspart, n_loss, s4);
  const double wsq = halving_column_sum(wsqpart, n_part, s4);
  double gm = 0.0;
  for (long i = threadIdx.x; i < n_part; i += 256) gm = fmax(gm, gmaxpart[i]);   // (a NaN is never the larger: F carries it)
  gm = block_max_f64(gm, s4);
  if (threadIdx.x == 0) {
    out[0] = __dadd_rn(__dmul_rn(loss, invN), __dmul_rn(__dmul_rn(0.5, lam), wsq));
    out[1] = gm;
    out[2] = loss;
  }
}

struct LrBasis { const double* v[LR_NV]; double coef[LR_NV]; int rows[3]; };

__global__ __launch_bounds__(256) void lr_axpy_kernel(const double* __restrict__ theta, const double* __restrict__ d, double t, long P,
                                                      double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < P) out[i] = fma(t, d[i], theta[i]);
}

__global__ __launch_bounds__(256) void lr_pair_kernel(const double* __restrict__ tn, const double* __restrict__ to, const double* __restrict__ gn,
                                                      const double* __restrict__ go, long P, double* __restrict__ s, double* __restrict__ yv) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < P) { s[i] = __dsub_rn(tn[i], to[i]); yv[i] = __dsub_rn(gn[i], go[i]); }
}

// out [blockIdx.y][blockIdx.x] = v[rows[blockIdx.y]] . v[blockIdx.x]: thread t the elements t, t + 256, .., then the workgroup by halving
__global__ __launch_bounds__(256) void lr_dots_kernel(LrBasis a, long P, double* __restrict__ out) {
  __shared__ double s4[4];
  const double *u = a.v[a.rows[blockIdx.y]], *v = a.v[blockIdx.x];
  double acc = 0.0;
  for (long i = threadIdx.x; i < P; i += 256) acc = fma(u[i], v[i], acc);
  acc = halving_block_sum(acc, s4);
  if (threadIdx.x == 0) out[(long)blockIdx.y * LR_NV + blockIdx.x] = acc;
}

// d = -(sum_j coef_j v_j), j rising over the coefficients that are not zero
__global__ __launch_bounds__(256) void lr_direction_kernel(LrBasis a, long P, double* __restrict__ d) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  double acc = 0.0;
  for (int j = 0; j < LR_NV; ++j)
    if (a.coef[j] != 0.0) acc = fma(a.coef[j], a.v[j][i], acc);   // (uniform)
  d[i] = -acc;
}

namespace {

struct LrProblem {
  PrepInput in;
  int K = 0, Kz = 0, Kp = 0, binary = 0, fit_intercept = 1;
  long P = 0, slices = 0, n_loss = 0, n_part = 0;
  unsigned chunks256 = 0;
  double invN = 0.0, lam = 0.0;
  PrepStage st;
  int32_t* dY = nullptr;
  double *dR = nullptr, *dPart = nullptr, *dLossPart = nullptr, *dWsqPart = nullptr, *dGmaxPart = nullptr, *dOut = nullptr;
};

// the checks the three entries share.  want_labels 0: none (smx_logreg_decision); 1: in range (an evaluation is defined without a row of
// every class); 2: and every class with a row (a fit is not)
int lr_check(const char* who, const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
             int32_t block_rows, const int32_t* labels, int want_labels, int32_t n_classes, int32_t form, LrProblem* pb) {
  const std::string w(who);
  SMX_CHECK(prep_check_input(who, x, indptr, cols, vals, n_rows, n_genes, block_rows, 0, nullptr, &pb->in));
  SMX_REQUIRE(n_genes <= SMX_LR_MAX_GENES, (w + ": 1 <= n_genes <= 32768").c_str());
  SMX_REQUIRE(form == 0 || form == 1, (w + ": form is 0 (multinomial) or 1 (binary)").c_str());
  SMX_REQUIRE(form == 1 ? n_classes == 2 : (n_classes >= 3 && n_classes <= SMX_LR_MAX_CLASSES),
              (w + ": the binary form has 2 classes, the multinomial form 3 .. 256").c_str());
  const long N = pb->in.N;
  const size_t n_val = x ? (size_t)N * (size_t)n_genes : (size_t)(indptr[N] - indptr[0]);
  const float* v = x ? x : vals + indptr[0];
  for (size_t i = 0; i < n_val; ++i) SMX_REQUIRE(std::isfinite(v[i]), (w + ": a matrix value that is not finite").c_str());
  if (want_labels) {
    SMX_REQUIRE(labels, (w + ": null labels").c_str());
    std::vector<long> count((size_t)n_classes, 0);
    for (long i = 0; i < N; ++i) {
      SMX_REQUIRE(labels[i] >= 0 && labels[i] < n_classes, (w + ": a label outside 0 .. n_classes - 1").c_str());
      ++count[(size_t)labels[i]];
    }
    for (int k = 0; k < n_classes && want_labels > 1; ++k) SMX_REQUIRE(count[(size_t)k] > 0, (w + ": a class without a row").c_str());
  }
  pb->K = n_classes; pb->binary = form; pb->Kz = form ? 1 : n_classes; pb->Kp = (pb->Kz + 3) & ~3;
  pb->P = (long)pb->Kz * pb->in.ld + pb->Kp;
  return SMX_OK;
}

int lr_check_penalty(const char* who, double C, LrProblem* pb) {
  SMX_REQUIRE(std::isfinite(C) && C > 0.0, (std::string(who) + ": C must be finite and > 0").c_str());
  pb->invN = 1.0 / (double)pb->in.N;
  pb->lam = 1.0 / (C * (double)pb->in.N);
  return SMX_OK;
}

int lr_check_params(const char* who, const double* W, const double* b, const LrProblem& pb) {
  for (long i = 0; i < (long)pb.Kz * pb.in.G; ++i) SMX_REQUIRE(std::isfinite(W[i]), (std::string(who) + ": a weight that is not finite").c_str());
  for (int k = 0; k < pb.Kz; ++k) SMX_REQUIRE(std::isfinite(b[k]), (std::string(who) + ": an intercept that is not finite").c_str());
  return SMX_OK;
}

// the whole matrix in the tile, the labels, and the buffers of an evaluation
int lr_resident(const char* who, DeviceScratch& buf, const int32_t* labels, LrProblem* pb) {
  PrepInput& in = pb->in;
  in.block = (in.N + SMX_PREP_SLICE - 1) / SMX_PREP_SLICE * SMX_PREP_SLICE;
  SMX_REQUIRE((size_t)in.block * (size_t)in.ld <= SMX_LR_MAX_RESIDENT,
              (std::string(who) + ": rows x n_genes <= 2^31 (the matrix is held whole)").c_str());
  if (!in.x) in.max_nnz = (size_t)(in.csr.indptr[in.N] - in.csr.indptr[0]);
  pb->slices = in.block / SMX_PREP_SLICE;
  pb->n_loss = (in.N + 4 * LR_ROWS - 1) / (4 * LR_ROWS);
  pb->chunks256 = (unsigned)((in.ld + 255) / 256);
  pb->n_part = (long)(pb->Kz + 1) * pb->chunks256;
  SMX_CHECK(prep_stage_alloc(buf, in, &pb->st, true));
  SMX_CHECK(buf.put(&pb->dY, labels, (size_t)in.N));
  SMX_CHECK(buf.get(&pb->dR, (size_t)in.N * pb->Kp));   // (dmalloc zeroes: the columns Kz .. Kp - 1 stay zero)
  SMX_CHECK(buf.get(&pb->dPart, (size_t)pb->slices * pb->Kz * in.ld));
  SMX_CHECK(buf.get(&pb->dLossPart, (size_t)pb->n_loss));
  SMX_CHECK(buf.get(&pb->dWsqPart, (size_t)pb->n_part));
  SMX_CHECK(buf.get(&pb->dGmaxPart, (size_t)pb->n_part));
  SMX_CHECK(buf.get(&pb->dOut, (size_t)4));
  SMX_CHECK(prep_load_block(in, pb->st, 0, in.N));
  return SMX_OK;
}

// host W [Kz][G], b [Kz] -> theta (zeroed by its allocation)
int lr_put_params(double* theta, const double* W, const double* b, const LrProblem& pb) {
  const PrepInput& in = pb.in;
  if (W)
    SMX_HIP(hipMemcpy2D(theta, (size_t)in.ld * 8, W, (size_t)in.G * 8, (size_t)in.G * 8, (size_t)pb.Kz, hipMemcpyHostToDevice));
  if (b && pb.fit_intercept) SMX_HIP(hipMemcpy(theta + (long)pb.Kz * in.ld, b, (size_t)pb.Kz * 8, hipMemcpyHostToDevice));
  return SMX_OK;
}

int lr_get_params(const double* theta, double* W, double* b, const LrProblem& pb) {
  const PrepInput& in = pb.in;
  SMX_HIP(hipMemcpy2D(W, (size_t)in.G * 8, theta, (size_t)in.ld * 8, (size_t)in.G * 8, (size_t)pb.Kz, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(b, theta + (long)pb.Kz * in.ld, (size_t)pb.Kz * 8, hipMemcpyDeviceToHost));
  return SMX_OK;
}

unsigned lr_row_grid(long nb) { return (unsigned)((nb + 4 * LR_ROWS - 1) / (4 * LR_ROWS)); }

// F and max|g| at theta, the gradient into g: four launches, then one read of two scalars
int lr_evaluate(const LrProblem& pb, const double* theta, double* g, double* F, double* gmax) {
  const long N = pb.in.N, ld = pb.in.ld;
  hipLaunchKernelGGL(lr_rows_kernel, dim3(lr_row_grid(N)), dim3(256), 0, nullptr, pb.st.tile, N, ld, theta, theta + (long)pb.Kz * ld, pb.Kz,
                     pb.binary, pb.dY, pb.Kp, pb.dR, pb.dLossPart, 0L, (double*)nullptr);
  hipLaunchKernelGGL(lr_grad_kernel, dim3((unsigned)pb.slices, (unsigned)((ld / 4 + 63) / 64), (unsigned)(pb.Kp / LR_CLASSES)), dim3(64), 0,
                     nullptr, pb.st.tile, N, ld, pb.dR, pb.Kp, pb.Kz, pb.dPart);
  hipLaunchKernelGGL(lr_combine_kernel, dim3(pb.chunks256, (unsigned)(pb.Kz + 1)), dim3(256), 0, nullptr, pb.dPart, pb.slices, ld, pb.Kz, pb.Kp,
                     N, pb.dR, theta, pb.invN, pb.lam, pb.fit_intercept, g, pb.dWsqPart, pb.dGmaxPart);
  hipLaunchKernelGGL(lr_close_kernel, dim3(1), dim3(256), 0, nullptr, pb.dLossPart, pb.n_loss, pb.dWsqPart, pb.dGmaxPart, pb.n_part, pb.invN,
                     pb.lam, pb.dOut);
  SMX_HIP(hipGetLastError());
  double out[2];
  SMX_HIP(hipMemcpy(out, pb.dOut, sizeof(out), hipMemcpyDeviceToHost));
  *F = out[0]; *gmax = out[1];
  return SMX_OK;
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_logreg_eval(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                    const int32_t* labels, int32_t n_classes, int32_t form, double C, int32_t fit_intercept, const double* W, const double* b,
                    double* F, double* gW, double* gb) {
  LrProblem pb;
  SMX_CHECK(lr_check("logreg_eval", x, indptr, cols, vals, n_rows, n_genes, 0, labels, 1, n_classes, form, &pb));
  SMX_CHECK(lr_check_penalty("logreg_eval", C, &pb));
  SMX_REQUIRE(W && b && F && gW && gb, "logreg_eval: null W, b or output");
  SMX_CHECK(lr_check_params("logreg_eval", W, b, pb));
  pb.fit_intercept = fit_intercept != 0;
  DeviceScratch buf;
  SMX_CHECK(lr_resident("logreg_eval", buf, labels, &pb));
  double *dTheta, *dG, gmax = 0.0;
  SMX_CHECK(buf.get(&dTheta, (size_t)pb.P));
  SMX_CHECK(buf.get(&dG, (size_t)pb.P));
  SMX_CHECK(lr_put_params(dTheta, W, b, pb));
  SMX_CHECK(lr_evaluate(pb, dTheta, dG, F, &gmax));
  SMX_CHECK(lr_get_params(dG, gW, gb, pb));
  return SMX_OK;
}

int smx_logreg_fit(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                   const int32_t* labels, int32_t n_classes, int32_t form, double C, int32_t fit_intercept, double tol, int32_t max_iter,
                   const double* W0, const double* b0, double* W, double* b, double* F, double* gmax, int32_t* n_iter, int32_t* n_eval,
                   int32_t* converged) {
  LrProblem pb;
  SMX_CHECK(lr_check("logreg_fit", x, indptr, cols, vals, n_rows, n_genes, 0, labels, 2, n_classes, form, &pb));
  SMX_CHECK(lr_check_penalty("logreg_fit", C, &pb));
  SMX_REQUIRE(tol > 0.0 && std::isfinite(tol), "logreg_fit: tol must be finite and > 0");
  SMX_REQUIRE(max_iter >= 1, "logreg_fit: max_iter >= 1");
  SMX_REQUIRE(W && b && F && gmax && n_iter && n_eval && converged, "logreg_fit: null output");
  SMX_REQUIRE((W0 != nullptr) == (b0 != nullptr), "logreg_fit: the warm start is W0 and b0, or neither");
  if (W0) SMX_CHECK(lr_check_params("logreg_fit", W0, b0, pb));
  pb.fit_intercept = fit_intercept != 0;
  DeviceScratch buf;
  SMX_CHECK(lr_resident("logreg_fit", buf, labels, &pb));
  const long P = pb.P;
  const unsigned pgrid = (unsigned)((P + 255) / 256);
  double *dTheta, *dThetaNew, *dG, *dGNew, *dD, *dHist, *dDots;
  SMX_CHECK(buf.get(&dTheta, (size_t)P));
  SMX_CHECK(buf.get(&dThetaNew, (size_t)P));
  SMX_CHECK(buf.get(&dG, (size_t)P));
  SMX_CHECK(buf.get(&dGNew, (size_t)P));
  SMX_CHECK(buf.get(&dD, (size_t)P));
  SMX_CHECK(buf.get(&dHist, (size_t)(2 * LR_SLOTS) * P));   // s slots, then y slots (zeros until written)
  SMX_CHECK(buf.get(&dDots, (size_t)3 * LR_NV));
  SMX_CHECK(lr_put_params(dTheta, W0, b0, pb));

  const int GI = 2 * LR_SLOTS;   // the gradient's place in the basis
  LrBasis basis;
  auto set_basis = [&]() {
    for (int j = 0; j < 2 * LR_SLOTS; ++j) basis.v[j] = dHist + (long)j * P;
    basis.v[GI] = dG;
  };
  std::vector<double> B((size_t)LR_NV * LR_NV, 0.0);   // the Gram matrix of the basis
  auto dots = [&](int n_rows_, const int* rows) -> int {
    set_basis();
    for (int a = 0; a < 3; ++a) basis.rows[a] = rows[a < n_rows_ ? a : 0];
    hipLaunchKernelGGL(lr_dots_kernel, dim3(LR_NV, (unsigned)n_rows_), dim3(256), 0, nullptr, basis, P, dDots);
    SMX_HIP(hipGetLastError());
    double h[3 * LR_NV];
    SMX_HIP(hipMemcpy(h, dDots, sizeof(double) * (size_t)n_rows_ * LR_NV, hipMemcpyDeviceToHost));
    for (int a = 0; a < n_rows_; ++a)
      for (int j = 0; j < LR_NV; ++j) B[(size_t)rows[a] * LR_NV + j] = B[(size_t)j * LR_NV + rows[a]] = h[a * LR_NV + j];
    return SMX_OK;
  };

  double Fc = 0.0, gm = 0.0;
  SMX_CHECK(lr_evaluate(pb, dTheta, dG, &Fc, &gm));
  int evals = 1, it = 0;
  if (!std::isfinite(Fc) || !std::isfinite(gm)) { set_error("logreg_fit: the objective is not finite at the start point"); return SMX_ERR_NAN; }
  { const int rows[1] = {GI}; SMX_CHECK(dots(1, rows)); }
  std::vector<int> pairs;   // the slots of the history, oldest first
  while (gm > tol && it < max_iter) {
    // the two-loop recursion on coefficients over the basis: q = sum_j coef_j v_j, from q = g
    double coef[LR_NV] = {0.0}, alpha[LR_SLOTS] = {0.0};
    coef[GI] = 1.0;
    auto dot_with = [&](int row) { double s = 0.0; for (int j = 0; j < LR_NV; ++j) s += coef[j] * B[(size_t)row * LR_NV + j]; return s; };
    for (int i = (int)pairs.size() - 1; i >= 0; --i) {
      const int c = pairs[(size_t)i];
      alpha[c] = dot_with(c) / B[(size_t)c * LR_NV + LR_SLOTS + c];
      coef[LR_SLOTS + c] -= alpha[c];
    }
    if (!pairs.empty()) {
      const int c = pairs.back(), yc = LR_SLOTS + c;
      const double gamma = B[(size_t)c * LR_NV + yc] / B[(size_t)yc * LR_NV + yc];
      for (int j = 0; j < LR_NV; ++j) coef[j] *= gamma;
    }
    for (size_t i = 0; i < pairs.size(); ++i) {
      const int c = pairs[i];
      const double beta = dot_with(LR_SLOTS + c) / B[(size_t)c * LR_NV + LR_SLOTS + c];
      coef[c] += alpha[c] - beta;
    }
    double gd = -dot_with(GI);
    if (!(gd < 0.0)) {   // (not a descent direction: steepest descent, the history dropped)
      pairs.clear();
      for (int j = 0; j < LR_NV; ++j) coef[j] = 0.0;
      coef[GI] = 1.0;
      gd = -B[(size_t)GI * LR_NV + GI];
      if (!(gd < 0.0)) break;
    }
    set_basis();
    for (int j = 0; j < LR_NV; ++j) basis.coef[j] = coef[j];
    hipLaunchKernelGGL(lr_direction_kernel, dim3(pgrid), dim3(256), 0, nullptr, basis, P, dD);
    double t = it == 0 ? 1.0 / gm : 1.0, Fn = 0.0, gmn = 0.0;
    bool ok = false;
    for (int trial = 0; trial < LR_TRIALS; ++trial, t *= 0.5) {
      hipLaunchKernelGGL(lr_axpy_kernel, dim3(pgrid), dim3(256), 0, nullptr, dTheta, dD, t, P, dThetaNew);
      SMX_CHECK(lr_evaluate(pb, dThetaNew, dGNew, &Fn, &gmn));
      ++evals;
      // (close to the optimum a step changes F by less than F's own rounding: such a trial is accepted if it lowers max|g|)
      if (std::isfinite(Fn) && std::isfinite(gmn) && (Fn <= Fc + LR_ARMIJO * t * gd || (std::fabs(Fn - Fc) <= LR_FLAT * std::fabs(Fc) && gmn < gm))) {
        ok = true;
        break;
      }
    }
    if (!ok) break;   // (the line search found no decrease: what there is is returned, unconverged)
    int c = 0;        // a slot that holds no pair of the history
    while (std::find(pairs.begin(), pairs.end(), c) != pairs.end()) ++c;
    hipLaunchKernelGGL(lr_pair_kernel, dim3(pgrid), dim3(256), 0, nullptr, dThetaNew, dTheta, dGNew, dG, P, dHist + (long)c * P,
                       dHist + (long)(LR_SLOTS + c) * P);
    std::swap(dTheta, dThetaNew);
    std::swap(dG, dGNew);
    Fc = Fn; gm = gmn;
    { const int rows[3] = {c, LR_SLOTS + c, GI}; SMX_CHECK(dots(3, rows)); }
    if (B[(size_t)c * LR_NV + LR_SLOTS + c] > 0.0) {   // s.y > 0, or the pair is skipped
      pairs.push_back(c);
      if ((int)pairs.size() > LR_MEMORY) pairs.erase(pairs.begin());
    }
    ++it;
  }
  SMX_HIP(hipDeviceSynchronize());
  SMX_CHECK(lr_get_params(dTheta, W, b, pb));
  *F = Fc; *gmax = gm; *n_iter = it; *n_eval = evals; *converged = gm <= tol ? 1 : 0;
  return SMX_OK;
}

int smx_logreg_decision(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                        int32_t block_rows, int32_t n_classes, int32_t form, const double* W, const double* b, double* logits) {
  LrProblem pb;
  SMX_CHECK(lr_check("logreg_decision", x, indptr, cols, vals, n_rows, n_genes, block_rows, nullptr, 0, n_classes, form, &pb));
  SMX_REQUIRE(W && b && logits, "logreg_decision: null W, b or logits");
  SMX_CHECK(lr_check_params("logreg_decision", W, b, pb));
  const PrepInput& in = pb.in;
  const long N = in.N, ld = in.ld;
  DeviceScratch buf;
  SMX_CHECK(prep_stage_alloc(buf, in, &pb.st, true));
  double *dTheta, *dZ;
  SMX_CHECK(buf.get(&dTheta, (size_t)pb.P));
  SMX_CHECK(buf.get(&dZ, (size_t)N * pb.Kz));
  SMX_CHECK(lr_put_params(dTheta, W, b, pb));
  for (long r0 = 0; r0 < N; r0 += in.block) {
    const long nb = std::min(in.block, N - r0);
    SMX_CHECK(prep_load_block(in, pb.st, r0, nb));
    hipLaunchKernelGGL(lr_rows_kernel, dim3(lr_row_grid(nb)), dim3(256), 0, nullptr, pb.st.tile, nb, ld, dTheta, dTheta + (long)pb.Kz * ld,
                       pb.Kz, pb.binary, (const int32_t*)nullptr, pb.Kp, (double*)nullptr, (double*)nullptr, r0, dZ);
    SMX_HIP(hipGetLastError());
    SMX_HIP(hipDeviceSynchronize());   // the next block's copy overwrites the tile
  }
  SMX_HIP(hipMemcpy(logits, dZ, (size_t)N * pb.Kz * 8, hipMemcpyDeviceToHost));
  return SMX_OK;
}

}  // extern "C"
