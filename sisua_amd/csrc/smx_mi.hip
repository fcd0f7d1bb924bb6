// smx_mi.hip -- gene x protein mutual-information matrices (SingleCellOMIC.get_mutual_information, _single_cell_analysis.py:1148-1196;
// Posterior.get_correlation_matrix(corr_type='mi')): scikit-learn's three kNN estimators per pair of columns, all float64, every distance
// the exact |a - b|.  The definitions are in include/sisua_hip.h and tests/mutual_info_ref.py.  Model-free entries: they upload,
// compute, download and free their own buffers.  The columns arrive prepared by the host (scaled, noised); the device never evaluates
// digamma or log: it adds entries of the host's two tables.
//   column sort   one workgroup per column: the cell indices through smx_block.h's stable radix sort on the 64-bit order-preserving pattern
//                 of the double (-0 as +0), eight 8-bit passes, then its tie-run pass (col_rank2_kernel runs the same two on float32).
//                 Leaves, per column: the order, the sorted values, every cell's position, and every cell's run of equal values
//                 (start, length) -- the label groups of a discrete column.
//   cc            Kraskov: threads = 256 consecutive cells of the gene's SORTED order, four continuous proteins per workgroup.  The k-th
//                 smallest Chebyshev distance is a set function, so the sweep over the other cells may take them in any order: it takes
//                 tiles of 128 outward from the workgroup's own cells in the gene's order, (x_j, y_j) through LDS as broadcasts, the 8 best
//                 per protein sorted in registers, and stops when every thread's k-th best is no larger than its distance in x to the
//                 nearest cell not yet visited (a cell further out in x cannot be nearer).  nx and ny are binary searches in the two
//                 sorted columns with the subtraction itself as the predicate (rounding is monotone).
//   cd / dd       one workgroup per pair.  A second stable radix sort (1 .. 3 passes on the run start, < N) of one column's order by the
//                 other column's label gives, for cd, every label group as a contiguous run ordered by the continuous value -- a cell's k
//                 nearest in its group are among the k cells either side of it -- and for dd the (gene label, protein label) runs.
//                 m_i of cd: two binary searches in the continuous column's order and a prefix count of the kept cells.
//   closing       one workgroup per pair: the sums of table entries over the cells in ONE order, a function of N alone (256 strided
//                 partials, then smx_block.h's fixed-order block sum), then the estimator's expression and the clip at 0.
// No float atomics; every loop is bounded by N, P or k; nothing depends on the gene chunk.
#include "smx_model.h"
#include "smx_block.h"   // the radix sort, the tie-run pass, the keys, the scans and the fixed-order sums

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace smx {

#define SMX_MI_MAX_CELLS (1l << 20)
#define SMX_MI_MAX_K 8     // the register list of the cc sweep
#define SMX_MI_PT 4        // continuous proteins per workgroup of the cc sweep
#define SMX_MI_TJ 128      // cells j per LDS tile

// what the column sort leaves per column, each [n_cols][N]
struct MiCols {
  const double* v;      // the columns
  unsigned* ord;        // the cells in sorted order (stable)
  unsigned* tmp;        // the sort's other array
  double* sv;           // the sorted values
  int32_t* pos;         // every cell's position in ord
  int32_t* start;       // every cell's run of equal values: the position of its first member ...
  int32_t* count;       // ... and its length
  int32_t* nonfinite;   // [n_cols]
};

__global__ __launch_bounds__(256) void mi_col_sort_kernel(MiCols c, int N) {
  __shared__ SortShared sh;
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * N;
  const double* x = c.v + base;
  int bad = 0;
  for (int i = tid; i < N; i += 256) bad |= is_nonfinite(x[i]);
  unsigned* A = c.tmp + base;
  const auto key = [x](unsigned i) { return order_key(x[i]); };
  const unsigned* S = block_radix_sort(key, N, 8, nullptr, A, c.ord + base, sh);   // (eight passes: the result is in ord)
  double* sv = c.sv + base;
  int32_t *pos = c.pos + base, *start = c.start + base, *count = c.count + base;
  block_tie_runs(key, [=](int j, unsigned ci, unsigned st) { sv[j] = x[ci]; pos[ci] = j; start[ci] = (int32_t)st; }, N, S, A, sh);
  for (int j = tid; j < N; j += 256) {
    const unsigned ci = S[j];
    const unsigned st = (unsigned)start[ci];
    count[ci] = (int32_t)(A[st] - st + 1u);
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) c.nonfinite[blockIdx.x] = bad ? 1 : 0;
}

// one launch's view of the problem: a chunk of genes against all proteins
struct MiArgs {
  MiCols x, y;               // the chunk's genes, the proteins
  const uint8_t* xdisc;      // [Gc] of the chunk
  const uint8_t* ydisc;      // [P]
  const int32_t* ycont;      // the continuous proteins' indices [Pc]
  int N, Gc, P, Pc, k;
  const double* psi;         // digamma(n), n = 0 .. N (entry 0 is never read)
  const double* logn;        // log(n), n = 0 .. N (entry 0 is never read)
  int32_t* cells;            // [Gc][P][4][N]: the per-cell integers of every pair (see the closing kernel)
  double* radius;            // [Gc][P][N] or NULL: the per-cell radius
  unsigned* pairA;           // [Gc][P][N] x 2: the pair sort's arrays
  unsigned* pairB;
  int32_t* prefix;           // [Gc][P][N + 1]: cd's prefix count of the kept cells
  double* mi;                // [Gc][P]
};

__device__ inline double mi_just_below(double r) {   // nextafter(r, 0) of a finite r >= 0
  return r > 0.0 ? __longlong_as_double(__double_as_longlong(r) - 1ll) : 0.0;
}

// the positions [lo, hi] of the sorted values sv [N] whose distance to v = sv[at] is <= r, by the subtraction itself (monotone in the position)
__device__ inline void mi_within(const double* sv, int N, int at, double v, double r, int* lo_out, int* hi_out) {
  int a = 0, b = at;   // the first position in [0, at] with v - sv[.] <= r
  while (a < b) {
    const int m = (a + b) >> 1;
    if (v - sv[m] <= r) b = m; else a = m + 1;
  }
  *lo_out = a;
  a = at; b = N - 1;   // the last position in [at, N - 1] with sv[.] - v <= r
  while (a < b) {
    const int m = (a + b + 1) >> 1;
    if (sv[m] - v <= r) a = m; else b = m - 1;
  }
  *hi_out = a;
}

__global__ __launch_bounds__(256) void mi_cc_kernel(MiArgs a) {
  __shared__ double shx[SMX_MI_TJ];
  __shared__ double shy[SMX_MI_PT][SMX_MI_TJ];
  const int g = blockIdx.z;
  if (a.xdisc[g]) return;   // (block-uniform)
  const int N = a.N, tid = threadIdx.x;
  const int q0 = (int)blockIdx.y * SMX_MI_PT, np = min(SMX_MI_PT, a.Pc - q0);
  int pl[SMX_MI_PT];
#pragma unroll
  for (int q = 0; q < SMX_MI_PT; ++q) pl[q] = a.ycont[q0 + min(q, np - 1)];
  const unsigned* ordx = a.x.ord + (long)g * N;
  const double* xs = a.x.sv + (long)g * N;
  const int t0 = (int)blockIdx.x * 256, s = t0 + tid;
  const bool live = s < N;
  const unsigned ci = live ? ordx[s] : 0u;
  const double xi = live ? xs[s] : 0.0;
  double yi[SMX_MI_PT], best[SMX_MI_PT][SMX_MI_MAX_K];
#pragma unroll
  for (int q = 0; q < SMX_MI_PT; ++q) {
    yi[q] = a.y.v[(long)pl[q] * N + ci];
#pragma unroll
    for (int u = 0; u < SMX_MI_MAX_K; ++u) best[q][u] = INFINITY;
  }
  // The visited positions are [lo, hi): step 0 takes the workgroup's own cells, then tiles of 128 alternately below and above.  Before every
  // step below: no cell outside [lo, hi) is nearer than gap in x alone, so when every thread's k-th best is <= its gap the lists are final.
  int lo = t0, hi = t0;
  for (int step = 0; step < 2 * (N / SMX_MI_TJ + 2); ++step) {   // (ends at the latest when [lo, hi) is everything)
    int j0, j1;
    if (step == 0) { j0 = t0; j1 = min(N, t0 + 256); hi = j1; }
    else if (step & 1) {
      const double gl = lo > 0 ? xi - xs[lo - 1] : INFINITY, gr = hi < N ? xs[hi] - xi : INFINITY;
      const double gap = fmin(gl, gr);
      bool done = true;
      if (live) {
#pragma unroll
        for (int q = 0; q < SMX_MI_PT; ++q) {
          double r = best[q][0];
#pragma unroll
          for (int u = 1; u < SMX_MI_MAX_K; ++u) r = u == a.k - 1 ? best[q][u] : r;
          done = done && (q >= np || r <= gap);
        }
      }
      if (__syncthreads_and(done)) break;
      j0 = max(0, lo - SMX_MI_TJ); j1 = lo; lo = j0;
    } else { j0 = hi; j1 = min(N, hi + SMX_MI_TJ); hi = j1; }
    for (int jt = j0; jt < j1; jt += SMX_MI_TJ) {
      const int nj = min(SMX_MI_TJ, j1 - jt);
      __syncthreads();
      if (tid < nj) shx[tid] = xs[jt + tid];
#pragma unroll
      for (int q = 0; q < SMX_MI_PT; ++q) {
        const int jj = tid & (SMX_MI_TJ - 1);
        if ((tid >> 7) == (q & 1) && jj < nj) shy[q][jj] = a.y.v[(long)pl[q] * N + ordx[jt + jj]];   // (two proteins per half of the workgroup)
      }
      __syncthreads();
      for (int jj = 0; jj < nj; ++jj) {
        const double dx = jt + jj == s ? INFINITY : fabs(xi - shx[jj]);   // (the cell itself is no neighbour)
#pragma unroll
        for (int q = 0; q < SMX_MI_PT; ++q) {
          const double d = fmax(dx, fabs(yi[q] - shy[q][jj]));
          if (d < best[q][SMX_MI_MAX_K - 1]) {
            best[q][SMX_MI_MAX_K - 1] = d;
#pragma unroll
            for (int u = SMX_MI_MAX_K - 1; u > 0; --u) {
              const double l = fmin(best[q][u - 1], best[q][u]), h = fmax(best[q][u - 1], best[q][u]);
              best[q][u - 1] = l; best[q][u] = h;
            }
          }
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int q = 0; q < SMX_MI_PT; ++q) {
    if (q >= np) continue;
    const int p = pl[q];
    double kd = best[q][0];
#pragma unroll
    for (int u = 1; u < SMX_MI_MAX_K; ++u) kd = u == a.k - 1 ? best[q][u] : kd;
    const double r = mi_just_below(kd);
    int l0, h0, l1, h1;
    mi_within(xs, N, s, xi, r, &l0, &h0);
    mi_within(a.y.sv + (long)p * N, N, a.y.pos[(long)p * N + ci], yi[q], r, &l1, &h1);
    int32_t* out = a.cells + ((long)g * a.P + p) * 4 * N;
    out[ci] = h0 - l0 + 1;           // nx + 1: the cells within r along x, the cell itself among them
    out[(long)N + ci] = h1 - l1 + 1; // ny + 1
    if (a.radius) a.radius[((long)g * a.P + p) * N + ci] = r;
  }
}

// one workgroup per pair of which at least one column is discrete
__global__ __launch_bounds__(256) void mi_pair_kernel(MiArgs a) {
#pragma clang fp contract(off)
  __shared__ SortShared sh;
  const int g = blockIdx.y, p = blockIdx.x, N = a.N, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool xd = a.xdisc[g], yd = a.ydisc[p];
  if (!xd && !yd) return;   // (block-uniform)
  const long pair = (long)g * a.P + p, xo = (long)g * N, yo = (long)p * N;
  int32_t* out = a.cells + pair * 4 * N;
  unsigned* A = a.pairA + pair * N;
  unsigned* B = a.pairB + pair * N;
  const int passes = N <= 256 ? 1 : N <= 65536 ? 2 : 3;   // the key is a position < N
  if (xd && yd) {
    // ---- dd: the proteins' order sorted by the gene's label: runs of (gene label, protein label) ----
    const int32_t *sa = a.x.start + xo, *sb = a.y.start + yo;
    const unsigned* S = block_radix_sort([sa](unsigned i) { return (unsigned long long)sa[i]; }, N, passes, a.y.ord + yo, A, B, sh);
    double* term = reinterpret_cast<double*>(out);   // [N] over the first two planes: a run's term at its head, 0 elsewhere
    const double dN = (double)N, logN = a.logn[N];
    for (int j = tid; j < N; j += 256) {
      const unsigned i = S[j];
      const long long key = ((long long)sa[i] << 32) | (long long)sb[i];
      bool head = j == 0;
      if (!head) {
        const unsigned h = S[j - 1];
        head = (((long long)sa[h] << 32) | (long long)sb[h]) != key;
      }
      double t = 0.0;
      int nab = 0;
      if (head) {
        int lo = j, hi = N - 1;   // the last position of the run: the keys do not decrease along S
        while (lo < hi) {
          const int m = (lo + hi + 1) >> 1;
          const unsigned c = S[m];
          if ((((long long)sa[c] << 32) | (long long)sb[c]) == key) lo = m; else hi = m - 1;
        }
        nab = lo - j + 1;
        t = ((double)nab / dN) * (((a.logn[nab] - a.logn[a.x.count[xo + i]]) - a.logn[a.y.count[yo + i]]) + logN);
      }
      term[j] = t;
      out[2l * N + j] = nab;
      out[3l * N + j] = (int32_t)i;
    }
    return;
  }
  // ---- cd: the continuous column's order sorted by the discrete column's label: every label group a run ordered by the value ----
  const MiCols& cc = xd ? a.y : a.x;
  const MiCols& dc = xd ? a.x : a.y;
  const long co = xd ? yo : xo, dof = xd ? xo : yo;
  const double* cv = cc.v + co;
  const double* csv = cc.sv + co;
  const unsigned* cord = cc.ord + co;
  const int32_t *dstart = dc.start + dof, *dcount = dc.count + dof;
  const unsigned* S = block_radix_sort([dstart](unsigned i) { return (unsigned long long)dstart[i]; }, N, passes, cord, A, B, sh);
  // prefix[m] = the kept cells (label group of more than one) among the first m of the continuous column's order
  int32_t* prefix = a.prefix + pair * (N + 1);
  unsigned carry = 0;
  for (int t0 = 0; t0 < N; t0 += 256) {
    const int j = t0 + tid;
    const unsigned one = j < N && dcount[cord[j]] > 1 ? 1u : 0u;
    const unsigned inc = wave_scan_add(one);
    if (lane == 63) sh.wtot[w] = inc;
    __syncthreads();
    unsigned before = carry + inc - one;
    for (int q = 0; q < w; ++q) before += sh.wtot[q];
    carry += sh.wtot[0] + sh.wtot[1] + sh.wtot[2] + sh.wtot[3];
    if (j < N) prefix[j] = (int32_t)before;
    __syncthreads();
  }
  if (tid == 0) prefix[N] = (int32_t)carry;
  __syncthreads();   // (the workgroup's own stores: read back below through the CU's cache)
  for (int j = tid; j < N; j += 256) {
    const unsigned i = S[j];
    const int st = dstart[i], cnt = dcount[i];
    int ki = 0, m = 0;
    double r = 0.0;
    if (cnt > 1) {
      ki = min(a.k, cnt - 1);
      const double ci = cv[i];
      int l = j - 1, rr = j + 1;   // the group's cells either side, nearest first: the ki-th smallest of the two ascending lists
      double kd = 0.0;
      for (int t = 0; t < ki; ++t) {
        const double dl = l >= st ? ci - cv[S[l]] : INFINITY, dr = rr < st + cnt ? cv[S[rr]] - ci : INFINITY;
        if (dl <= dr) { kd = dl; --l; } else { kd = dr; ++rr; }
      }
      r = mi_just_below(kd);
      int lo, hi;
      mi_within(csv, N, cc.pos[co + i], ci, r, &lo, &hi);
      m = prefix[hi + 1] - prefix[lo];
    }
    out[i] = ki;
    out[(long)N + i] = cnt > 1 ? cnt : 0;
    out[2l * N + i] = m;
    out[3l * N + i] = cnt;
    if (a.radius) a.radius[pair * N + i] = r;
  }
}

// one workgroup per pair: the sums over the cells in the fixed order, the estimator's expression, the clip
__global__ __launch_bounds__(256) void mi_close_kernel(MiArgs a) {
#pragma clang fp contract(off)
  __shared__ double sd[4];
  __shared__ int si[4];
  const int g = blockIdx.y, p = blockIdx.x, N = a.N, tid = threadIdx.x;
  const bool xd = a.xdisc[g], yd = a.ydisc[p];
  const long pair = (long)g * a.P + p;
  const int32_t* in = a.cells + pair * 4 * N;
  double v;
  if (xd && yd) {
    const double* term = reinterpret_cast<const double*>(in);
    double s = 0.0;
    for (int j = tid; j < N; j += 256) s += term[j];
    v = halving_block_sum(s, sd);
  } else if (!xd && !yd) {
    double sx = 0.0, sy = 0.0;
    for (int i = tid; i < N; i += 256) { sx += a.psi[in[i]]; sy += a.psi[in[(long)N + i]]; }
    sx = halving_block_sum(sx, sd);
    sy = halving_block_sum(sy, sd);
    v = a.psi[N] + a.psi[a.k] - sx / (double)N - sy / (double)N;
  } else {
    double sk = 0.0, sc = 0.0, sm = 0.0;
    int kept = 0;
    for (int i = tid; i < N; i += 256) {
      const int c = in[(long)N + i];
      if (c) { sk += a.psi[in[i]]; sc += a.psi[c]; sm += a.psi[in[2l * N + i]]; ++kept; }
    }
    sk = halving_block_sum(sk, sd);
    sc = halving_block_sum(sc, sd);
    sm = halving_block_sum(sm, sd);
    kept = halving_block_sum(kept, si);
    const double n = (double)kept;
    v = kept ? a.psi[kept] + sk / n - sc / n - sm / n : 0.0;   // (no cell kept: 0, where scikit-learn raises)
  }
  if (tid == 0) a.mi[pair] = v > 0.0 ? v : 0.0;
}

// the device side of one set of columns
static int mi_cols_alloc(DeviceScratch& buf, MiCols* c, size_t n_cols, size_t N) {
  const size_t n = n_cols * N;
  double* v;
  SMX_CHECK(buf.get(&v, n));
  c->v = v;
  SMX_CHECK(buf.get(&c->ord, n)); SMX_CHECK(buf.get(&c->tmp, n)); SMX_CHECK(buf.get(&c->sv, n));
  SMX_CHECK(buf.get(&c->pos, n)); SMX_CHECK(buf.get(&c->start, n)); SMX_CHECK(buf.get(&c->count, n));
  SMX_CHECK(buf.get(&c->nonfinite, n_cols));
  return SMX_OK;
}

// upload n_cols columns, sort them, and refuse a column that is not finite: `what` and `index0` name it
static int mi_cols_sort(const MiCols& c, const double* host, int n_cols, long N, const char* what, long index0) {
  SMX_HIP(hipMemcpy(const_cast<double*>(c.v), host, (size_t)n_cols * N * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mi_col_sort_kernel, dim3((unsigned)n_cols), dim3(256), 0, nullptr, c, (int)N);
  SMX_HIP(hipGetLastError());
  std::vector<int32_t> nf((size_t)n_cols);
  SMX_HIP(hipMemcpy(nf.data(), c.nonfinite, nf.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int i = 0; i < n_cols; ++i)
    if (nf[i]) {
      set_error(std::string("mutual_info: ") + what + " column " + std::to_string(index0 + i) + " holds a value that is not finite");
      return SMX_ERR_INVALID;
    }
  return SMX_OK;
}

static int mi_check(const void* x, const uint8_t* xd, const void* y, const uint8_t* yd, int64_t N, int64_t G, int64_t P, int32_t k,
                    const double* psi, const double* logn) {
  SMX_REQUIRE(x && xd && y && yd && psi && logn, "mutual_info: null argument");
  SMX_REQUIRE(G >= 1 && P >= 1 && G * P < ((int64_t)1 << 31), "mutual_info: 1 <= n_genes, 1 <= n_proteins, n_genes x n_proteins < 2^31");
  SMX_REQUIRE(N >= 2 && N <= SMX_MI_MAX_CELLS, "mutual_info: 2 <= n_cells <= 2^20");
  SMX_REQUIRE(k >= 1, "mutual_info: n_neighbors >= 1");
  SMX_REQUIRE(k <= SMX_MI_MAX_K, "mutual_info: n_neighbors above 8 is not built (SMX_MI_MAX_K: the register list of the sweep)");
  SMX_REQUIRE(k < N, "mutual_info: n_neighbors must be below n_cells");
  return SMX_OK;
}

// The launches of one chunk of sorted genes against the sorted proteins, enqueued.
static int mi_launch(const MiArgs& a) {
  if (a.Pc > 0) {
    hipLaunchKernelGGL(mi_cc_kernel, dim3((unsigned)((a.N + 255) / 256), (unsigned)((a.Pc + SMX_MI_PT - 1) / SMX_MI_PT), (unsigned)a.Gc), dim3(256),
                       0, nullptr, a);
    SMX_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(mi_pair_kernel, dim3((unsigned)a.P, (unsigned)a.Gc), dim3(256), 0, nullptr, a);
  SMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(mi_close_kernel, dim3((unsigned)a.P, (unsigned)a.Gc), dim3(256), 0, nullptr, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

}  // namespace smx

using namespace smx;

extern "C" {

int smx_mutual_info(const double* xcols, const uint8_t* x_discrete, const double* ycols, const uint8_t* y_discrete, int64_t n_cells,
                    int32_t n_genes, int32_t n_proteins, int32_t n_neighbors, int32_t gene_chunk, const double* psi, const double* logn,
                    double* mi) {
  SMX_CHECK(mi_check(xcols, x_discrete, ycols, y_discrete, n_cells, n_genes, n_proteins, n_neighbors, psi, logn));
  SMX_REQUIRE(mi && gene_chunk >= 0, "mutual_info: null result or a negative gene_chunk");
  const long N = (long)n_cells;
  const int G = n_genes, P = n_proteins;
  // the genes of a chunk: 36 N bytes of sorted columns and 28 N P of pair work each; 256 MB by default, and a grid's third extent at most
  const size_t per_gene = (size_t)N * (36 + 28 * (size_t)P) + 64;
  int Gc = gene_chunk > 0 ? gene_chunk : (int)std::max<size_t>(1, ((size_t)256 << 20) / per_gene);
  Gc = std::min(std::min(Gc, G), 32768);
  std::vector<int32_t> ycont;
  for (int p = 0; p < P; ++p)
    if (!y_discrete[p]) ycont.push_back(p);
  DeviceScratch buf;
  MiArgs a{};
  a.N = (int)N; a.P = P; a.Pc = (int)ycont.size(); a.k = n_neighbors;
  SMX_CHECK(mi_cols_alloc(buf, &a.y, (size_t)P, (size_t)N));
  SMX_CHECK(mi_cols_alloc(buf, &a.x, (size_t)Gc, (size_t)N));
  uint8_t *dxd, *dyd;
  int32_t* dyc;
  double *dpsi, *dlog;
  SMX_CHECK(buf.get(&dxd, (size_t)Gc));
  SMX_CHECK(buf.put(&dyd, y_discrete, (size_t)P));
  SMX_CHECK(buf.get(&dyc, std::max<size_t>(1, ycont.size())));
  if (!ycont.empty()) SMX_HIP(hipMemcpy(dyc, ycont.data(), ycont.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  SMX_CHECK(buf.put(&dpsi, psi, (size_t)N + 1));
  SMX_CHECK(buf.put(&dlog, logn, (size_t)N + 1));
  const size_t pairs = (size_t)Gc * P;
  SMX_CHECK(buf.get(&a.cells, pairs * 4 * N));
  SMX_CHECK(buf.get(&a.pairA, pairs * N)); SMX_CHECK(buf.get(&a.pairB, pairs * N));
  SMX_CHECK(buf.get(&a.prefix, pairs * (N + 1)));
  SMX_CHECK(buf.get(&a.mi, pairs));
  a.xdisc = dxd; a.ydisc = dyd; a.ycont = dyc; a.psi = dpsi; a.logn = dlog; a.radius = nullptr;
  SMX_CHECK(mi_cols_sort(a.y, ycols, P, N, "protein", 0));
  for (int g0 = 0; g0 < G; g0 += Gc) {
    const int n = std::min(Gc, G - g0);
    a.Gc = n;
    SMX_HIP(hipMemcpy(dxd, x_discrete + g0, (size_t)n, hipMemcpyHostToDevice));
    SMX_CHECK(mi_cols_sort(a.x, xcols + (size_t)g0 * N, n, N, "gene", g0));
    SMX_CHECK(mi_launch(a));
    SMX_HIP(hipMemcpy(mi + (size_t)g0 * P, a.mi, (size_t)n * P * sizeof(double), hipMemcpyDeviceToHost));   // (waits for the launches)
  }
  return SMX_OK;
}

int smx_k_mi_cells(const double* x, int32_t x_discrete, const double* y, int32_t y_discrete, int64_t n_cells, int32_t n_neighbors,
                   const double* psi, const double* logn, int32_t* cells, double* radius, double* mi) {
  const uint8_t xd = x_discrete ? 1 : 0, yd = y_discrete ? 1 : 0;
  SMX_CHECK(mi_check(x, &xd, y, &yd, n_cells, 1, 1, n_neighbors, psi, logn));
  SMX_REQUIRE(cells && radius && mi, "mi_cells: null result");
  const long N = (long)n_cells;
  const int32_t yc0 = 0;
  DeviceScratch buf;
  MiArgs a{};
  a.N = (int)N; a.Gc = 1; a.P = 1; a.Pc = yd ? 0 : 1; a.k = n_neighbors;
  SMX_CHECK(mi_cols_alloc(buf, &a.y, 1, (size_t)N));
  SMX_CHECK(mi_cols_alloc(buf, &a.x, 1, (size_t)N));
  uint8_t *dxd, *dyd;
  int32_t* dyc;
  double *dpsi, *dlog;
  SMX_CHECK(buf.put(&dxd, &xd, (size_t)1)); SMX_CHECK(buf.put(&dyd, &yd, (size_t)1)); SMX_CHECK(buf.put(&dyc, &yc0, (size_t)1));
  SMX_CHECK(buf.put(&dpsi, psi, (size_t)N + 1)); SMX_CHECK(buf.put(&dlog, logn, (size_t)N + 1));
  SMX_CHECK(buf.get(&a.cells, (size_t)4 * N)); SMX_CHECK(buf.get(&a.radius, (size_t)N));
  SMX_CHECK(buf.get(&a.pairA, (size_t)N)); SMX_CHECK(buf.get(&a.pairB, (size_t)N));
  SMX_CHECK(buf.get(&a.prefix, (size_t)N + 1));
  SMX_CHECK(buf.get(&a.mi, (size_t)1));
  a.xdisc = dxd; a.ydisc = dyd; a.ycont = dyc; a.psi = dpsi; a.logn = dlog;
  SMX_CHECK(mi_cols_sort(a.y, y, 1, N, "protein", 0));
  SMX_CHECK(mi_cols_sort(a.x, x, 1, N, "gene", 0));
  SMX_CHECK(mi_launch(a));
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(cells, a.cells, (size_t)4 * N * sizeof(int32_t), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(radius, a.radius, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(mi, a.mi, sizeof(double), hipMemcpyDeviceToHost));
  return SMX_OK;
}

}  // extern "C"
