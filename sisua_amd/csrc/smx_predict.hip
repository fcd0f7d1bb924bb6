// smx_predict.hip -- evaluation-mode forward passes handed back to the host: smx_forward, smx_forward_samples, smx_predict, smx_decode.
#include "smx_model.h"
#include "smx_loss.h"

namespace smx {

// The k parameter planes of a batch, device [B][k * Gp] -> caller's [k][B][G]: ONE contiguous copy into a pinned
// staging buffer (a pitched copy into pageable memory runs at ~1.6 GB/s here), then row copies on the host.
static int fetch_planes(smx_model* m, int B, float* x_params) {
  if (!x_params) return SMX_OK;
  const size_t n = (size_t)B * m->k * m->Gp;
  SMX_CHECK(hgrow(m, &m->pinned, &m->pinned_floats, n, (size_t)m->Bmax * m->k * m->Gp));
  SMX_HIP(hipMemcpyAsync(m->pinned, m->P, n * sizeof(float), hipMemcpyDeviceToHost, m->st));
  SMX_HIP(hipStreamSynchronize(m->st));
  const size_t G = (size_t)m->G, ldp = (size_t)m->k * m->Gp;
  for (int ch = 0; ch < m->k; ++ch)
    for (int b = 0; b < B; ++b)
      memcpy(x_params + ((size_t)ch * B + b) * G, m->pinned + (size_t)b * ldp + (size_t)ch * m->Gp, G * sizeof(float));
  return SMX_OK;
}

// The label heads' outputs of a batch, device [B][ld] per head -> caller's [B][ky * P] at y_params[j] + y_draw * B * ky * P (a NULL
// y_params or y_params[j]: not asked for)
static int fetch_labels(smx_model* m, int B, float* const* y_params, size_t y_draw) {
  if (!y_params) return SMX_OK;
  std::vector<float> tmp;
  for (int j = 0; j < m->n_heads; ++j) {
    if (!y_params[j]) continue;
    const int P = m->cfg.label_dim[j], Pp = m->lab_Pp[j], ld = m->tensors[m->t_labW[j]].ld;
    float* dst = y_params[j] + y_draw * (size_t)B * m->lab_ky[j] * P;
    tmp.resize((size_t)B * ld);
    SMX_HIP(hipMemcpy(tmp.data(), m->laby_raw[j], tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
      for (int c = 0; c < m->lab_ky[j]; ++c)
        memcpy(dst + ((size_t)b * m->lab_ky[j] + c) * P, &tmp[(size_t)b * ld + (size_t)c * Pp], sizeof(float) * P);
  }
  return SMX_OK;
}

// copy the results of the forward pass in flight back to the caller's arrays (any pointer may be NULL);
// y_draw: draw index of the label outputs (fetch_labels)
static int fetch_forward(smx_model* m, int B, float* z_mean, float* z_scale, float* z_sample, float* l_mean, float* l_scale,
                         float* l_sample, float* x_params, float* const* y_params, size_t y_draw) {
  SMX_HIP(hipStreamSynchronize(m->st));
  const int D = m->D, Dp = m->Dp;
  const int lat_ld = m->lat_planes * Dp;
  auto fetch2d = [&](float* dst, const float* src, int ld, int w) -> int {
    if (!dst) return SMX_OK;
    SMX_HIP(hipMemcpy2D(dst, (size_t)w * sizeof(float), src, (size_t)ld * sizeof(float), (size_t)w * sizeof(float), (size_t)B,
                        hipMemcpyDeviceToHost));
    return SMX_OK;
  };
  SMX_CHECK(fetch2d(z_mean, m->mixpost ? m->zmean : m->latbuf, m->mixpost ? Dp : lat_ld, D));   // (mixture-density posterior: the mixture's mean)
  if (m->stochastic) SMX_CHECK(m->latent_tril ? fetch2d(z_scale, m->ltril, D * D, D * D) : fetch2d(z_scale, m->sig, Dp, D));   // (tril: the factor L [D][D])
  SMX_CHECK(fetch2d(z_sample, m->z, Dp, D));
  if (m->scvi) {
    SMX_CHECK(fetch2d(l_mean, m->latlbuf, 32, 1));
    SMX_CHECK(fetch2d(l_scale, m->lsig, 1, 1));
    SMX_CHECK(fetch2d(l_sample, m->lsmp, 1, 1));
  }
  SMX_CHECK(fetch_planes(m, B, x_params));
  return fetch_labels(m, B, y_params, y_draw);
}

// SingleCellModel.predict over a whole host matrix in ONE call.  The batch loop runs here; after every forward pass one
// small launch packs what the caller asked for (parameter planes, latent moments, draws, label outputs) into device
// staging laid out like the caller's arrays for a CHUNK of cells (up to 128 MB), and each chunk leaves the device as a
// few large contiguous copies straight into its final place (48 GB/s into pageable memory as into pinned,
// tools/pcie_probe.hip).  No per-batch result arrays, no host re-packing, no concatenation afterwards -- and no swarm
// of small pitched copies (each a synchronous call: at batch 8 x 10 draws they cost 4x the whole old path).
// (n_rep repetitions of a job, e.g. the draws of a stacked pass: repetition q reads src + q src_rep, writes dst + q dst_rep)
struct PackJob { float* dst; long dpitch; const float* src; long spitch; int width; int height; int n_rep; long dst_rep; long src_rep; };
// A job list travels as a kernel argument (2 KB); a pass that needs more jobs than fit (MISA with four components: 3 latent +
// 3 planes + 12 label planes) launches the full list and starts the next one -- jobs are independent of each other.
#define SMX_PACK_MAX 32
struct PackJobs { int n; PackJob j[SMX_PACK_MAX]; };
__global__ __launch_bounds__(256) void pack_kernel(PackJobs jobs_by_value) {
  const PackJobs& J = *(const PackJobs*)__builtin_amdgcn_kernarg_segment_ptr();   // (run-time job index: no scratch copy)
  const PackJob& j = J.j[blockIdx.y];
  if ((int)blockIdx.z >= j.n_rep) return;
  const long total = (long)j.width * j.height;
  float* dst = j.dst + (long)blockIdx.z * j.dst_rep;
  const float* src = j.src + (long)blockIdx.z * j.src_rep;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / j.width, c = i % j.width;
    dst[r * j.dpitch + c] = src[r * j.spitch + c];
  }
}
// One site's job list: add() launches the list when it is full and starts the next one, flush() launches what is left.  Every launch runs
// gx workgroups per job and gz repetitions (each job's n_rep); every job copies `height` rows.
struct PackList {
  hipStream_t st; unsigned gx, gz; int height;
  PackJobs J;
  PackList(hipStream_t st_, unsigned gx_, unsigned gz_, int height_) : st(st_), gx(gx_), gz(gz_), height(height_) { J.n = 0; }
  // rows of `width` floats, src (pitch spitch) -> dst (pitch dpitch); repetition q reads src + q src_rep, writes dst + q dst_rep (no dst: no job)
  int add(float* dst, size_t dpitch, const float* src, size_t spitch, size_t width, size_t dst_rep = 0, size_t src_rep = 0) {
    if (!dst) return SMX_OK;
    if (J.n == SMX_PACK_MAX) SMX_CHECK(flush());
    J.j[J.n++] = PackJob{dst, (long)dpitch, src, (long)spitch, (int)width, height, (int)gz, (long)dst_rep, (long)src_rep};
    return SMX_OK;
  }
  int flush() {
    if (!J.n) return SMX_OK;
    hipLaunchKernelGGL(pack_kernel, dim3(gx, (unsigned)J.n, gz), dim3(256), 0, st, J);
    J.n = 0;
    SMX_HIP(hipGetLastError());
    return SMX_OK;
  }
};

// ---- statistics of the gene output on the device (smx_predict_stat): what the reference's callers ask of predict()'s result --
// y.mean() / .variance() / .log_prob(x), posterior.py:187-255 -- computed from the parameter planes of a pass WITHOUT the planes leaving
// the device (24 KB per cell and draw at C2: predict's D2H traffic).  Formulas = sisua_amd/distributions.py (float32 here); held to
// float64 at saturated planes by tests/test_gpu_plane_stats.py (bounds: tests/plane_stat_ref.py).
struct StatArgs {
  const float* P; long ldp; long plane_stride;   // planes of `rows` = Sn * B stacked rows (row s * B + b = draw s of cell b)
  int B, Sn, G, lk, direct, count_only, stat;    // stat: 0 mean, 1 variance (per draw), 2 mean averaged over the draws, 3 log_prob
  float inv_S; int accumulate;                   // stat 2: this pass adds (sum over its draws) * inv_S to what earlier passes left
  float* dst; long dst_draw;                     // stat 0 / 1: dst[s * dst_draw + b * G + g]; stat 2: dst[b * G + g]; stat 3: dst[s * dst_draw + b]
  const float* T; long ldt; const int32_t* trows; int t_u16;   // stat 3: targets [B][ldt] (or the resident rows trows[b])
};
__device__ inline void plane_moments(int lk, int direct, int count_only, float p0, float p1, float p2, float& mean, float& var) {
  float mc, vc;
  if (lk == SMX_LLK_MSE) { mean = p0; var = 0.f; return; }
  if (lk == SMX_LLK_NB || lk == SMX_LLK_ZINB) { const float el = expf(p1); mc = expf(p0) * el; vc = mc * (1.f + el); }
  else {
    const float mu = direct ? p0 : softplus_sigmoid(p0).sp, th = direct ? p1 : softplus_sigmoid(p1 + SMX_SOFTPLUS_INV_1).sp;
    // mu (1 + mu / th), not mu + mu mu / th: mu mu underflows where the variance is still a normal number (mu ~ th ~ 1e-26: 37 % off);
    // mu == 0 (both underflowed: 0 / 0) has variance 0
    mc = mu; vc = mu > 0.f ? mu * (1.f + mu / th) : 0.f;
  }
  if ((lk == SMX_LLK_ZINB || lk == SMX_LLK_ZINBD) && !count_only) {
    // 1 - pi as sigmoid(-p2): the difference 1 - pi cancels from a gate logit of a few units on and is exactly 0 from 17
    const float pi = 1.f / (1.f + expf(-p2)), q = sigmoidf(-p2);
    mean = q * mc; var = q * (vc + pi * mc * mc);
  } else { mean = mc; var = vc; }
}
__global__ __launch_bounds__(256) void plane_stat_kernel(StatArgs a) {
  const int g = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (g >= a.G) return;
  const bool zi = a.lk == SMX_LLK_ZINB || a.lk == SMX_LLK_ZINBD;
  float acc = 0.f;
  for (int s = 0; s < a.Sn; ++s) {   // (draw order: the average over the draws is deterministic)
    const float* p = a.P + ((long)s * a.B + b) * a.ldp + g;
    float mean, var;
    plane_moments(a.lk, a.direct, a.count_only, p[0], a.lk == SMX_LLK_MSE ? 0.f : p[a.plane_stride], zi ? p[2 * a.plane_stride] : 0.f, mean, var);
    if (a.stat == 2) acc += mean;
    else a.dst[(long)s * a.dst_draw + (long)b * a.G + g] = a.stat == 0 ? mean : var;
  }
  if (a.stat == 2) { float* d = a.dst + (long)b * a.G + g; *d = (a.accumulate ? *d : 0.f) + acc * a.inv_S; }
}
template <int LK, int DIRECT>
__device__ inline float row_llk_elem(float x, float p0, float p1, float p2) {
  float llk, d0, d1, d2;
  count_elem<LK, DIRECT>(x, p0, p1, p2, llk, d0, d1, d2);
  return llk - lgammaf(x + 1.f);
}
// stat 3: one workgroup per stacked row: log p(target row | the row's planes), summed over the genes (Independent(..., 1).log_prob)
__global__ __launch_bounds__(256) void plane_logprob_kernel(StatArgs a) {
  __shared__ float sh[4];
  const int row = blockIdx.x, b = row % a.B, s = row / a.B;
  const float* p = a.P + (long)row * a.ldp;
  const long trow = a.trows ? a.trows[b] : b;
  int lk = a.lk;
  if (a.count_only && lk == SMX_LLK_ZINB) lk = SMX_LLK_NB;
  if (a.count_only && lk == SMX_LLK_ZINBD) lk = SMX_LLK_NBD;
  float acc = 0.f;
  for (int g = threadIdx.x; g < a.G; g += 256) {
    const float x = a.t_u16 ? (float)reinterpret_cast<const uint16_t*>(a.T)[trow * a.ldt + g] : a.T[trow * a.ldt + g];
    const float p0 = p[g], p1 = a.lk == SMX_LLK_MSE ? 0.f : p[a.plane_stride + g], p2 = (a.lk == SMX_LLK_ZINB || a.lk == SMX_LLK_ZINBD) ? p[2 * a.plane_stride + g] : 0.f;
    float v;
    switch (lk) {
      case SMX_LLK_NB: v = row_llk_elem<SMX_LLK_NB, 0>(x, p0, p1, p2); break;
      case SMX_LLK_ZINB: v = row_llk_elem<SMX_LLK_ZINB, 0>(x, p0, p1, p2); break;
      case SMX_LLK_NBD: v = a.direct ? row_llk_elem<SMX_LLK_NBD, 1>(x, p0, p1, p2) : row_llk_elem<SMX_LLK_NBD, 0>(x, p0, p1, p2); break;
      case SMX_LLK_ZINBD: v = a.direct ? row_llk_elem<SMX_LLK_ZINBD, 1>(x, p0, p1, p2) : row_llk_elem<SMX_LLK_ZINBD, 0>(x, p0, p1, p2); break;
      default: { const float df = x - p0; v = -(df * df) / (float)a.G; }   // 'mse': -log_prob == tf.losses.mse
    }
    acc += v;
  }
  acc = wave_sum(acc);   // the four waves' sums meet in LDS, added in wave order
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.dst[(long)s * a.dst_draw + b] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// The same statistics of the 'bernoulli' (logits) and 'normal' (loc | raw scale) outputs, as kernels of their own (the count kernels above
// stay as they are): Bernoulli mean p = sigmoid(l), variance sigmoid(l) sigmoid(-l); normal mean m, variance sigma^2, sigma = softplus(s + softplus^-1(1));
// log_prob = the sum over the genes of smx_loss.h's bernoulli_elem / normal_elem (no count constant).  count_only changes nothing here.
__device__ inline void rv_moments(int lk, float p0, float p1, float& mean, float& var) {
  if (lk == SMX_LLK_BERNOULLI) { const float p = 1.f / (1.f + expf(-p0)); mean = p; var = sigmoidf(p0) * sigmoidf(-p0); }   // (not p (1 - p): see plane_moments)
  else { const float sd = softplus_sigmoid(p1 + SMX_SOFTPLUS_INV_1).sp; mean = p0; var = sd * sd; }
}
__global__ __launch_bounds__(256) void plane_stat_rv_kernel(StatArgs a) {
  const int g = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (g >= a.G) return;
  const bool two = a.lk == SMX_LLK_NORMAL;
  float acc = 0.f;
  for (int s = 0; s < a.Sn; ++s) {   // (draw order: the average over the draws is deterministic)
    const float* p = a.P + ((long)s * a.B + b) * a.ldp + g;
    float mean, var;
    rv_moments(a.lk, p[0], two ? p[a.plane_stride] : 0.f, mean, var);
    if (a.stat == 2) acc += mean;
    else a.dst[(long)s * a.dst_draw + (long)b * a.G + g] = a.stat == 0 ? mean : var;
  }
  if (a.stat == 2) { float* d = a.dst + (long)b * a.G + g; *d = (a.accumulate ? *d : 0.f) + acc * a.inv_S; }
}
__global__ __launch_bounds__(256) void plane_logprob_rv_kernel(StatArgs a) {
  __shared__ float sh[4];
  const int row = blockIdx.x, b = row % a.B, s = row / a.B;
  const float* p = a.P + (long)row * a.ldp;
  const long trow = a.trows ? a.trows[b] : b;
  const bool two = a.lk == SMX_LLK_NORMAL;
  float acc = 0.f;
  for (int g = threadIdx.x; g < a.G; g += 256) {
    const float x = a.t_u16 ? (float)reinterpret_cast<const uint16_t*>(a.T)[trow * a.ldt + g] : a.T[trow * a.ldt + g];
    float v, d0, d1;
    if (two) normal_elem(x, p[g], p[a.plane_stride + g], v, d0, d1);
    else bernoulli_elem(x, p[g], v, d0);
    acc += v;
  }
  acc = wave_sum(acc);   // the four waves' sums meet in LDS, added in wave order
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.dst[(long)s * a.dst_draw + b] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
static int launch_plane_stat(hipStream_t st, const StatArgs& a) {
  const bool rv = a.lk == SMX_LLK_BERNOULLI || a.lk == SMX_LLK_NORMAL;
  if (a.stat == 3) hipLaunchKernelGGL(rv ? plane_logprob_rv_kernel : plane_logprob_kernel, dim3((unsigned)(a.Sn * a.B)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(rv ? plane_stat_rv_kernel : plane_stat_kernel, dim3((unsigned)((a.G + 255) / 256), (unsigned)a.B), dim3(256), 0, st, a);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
// what smx_predict_stat asks of the batch loop below in place of the parameter planes
// (stat 4: n_k predictive samples per draw under `seed`, smx_sample.hip)
struct StatReq {
  int stat = 0, count_only = 0; HostRows target{}; float* out = nullptr;   // target: neither form = the input rows themselves
  uint64_t seed = 0; int n_k = 1;
  // stat 2 only.  sel: n_sel gene indices (device) -- out is [n_cells][n_sel].  impute: nothing of the mean leaves the device; the scores
  // of |target - mean| do (smx_impute.hip), `target` being the original rows
  const int32_t* sel = nullptr; int n_sel = 0;
  int impute = 0; float* imp_median = nullptr; int32_t* imp_changed = nullptr; float* imp_lohi = nullptr;
  // keep_cols (with sel): nothing leaves the device; the selected columns are kept gene-major [n_sel][n_cells] there (smx_correlate.hip)
  float* keep_cols = nullptr;
};
// what a call wants of predict_core's walk: the statistic `sr` (NULL: none) and / or smx_predict's arrays (NULL: not asked for)
struct PredWant {
  const StatReq* sr = nullptr;
  float *z_mean = nullptr, *z_scale = nullptr, *z_samples = nullptr, *l_mean = nullptr, *l_scale = nullptr, *l_samples = nullptr, *x_params = nullptr;
  float* const* y_params = nullptr;
};

// ---- host rows given as CSR (the rows convention of sisua_hip.h): (indptr int64 [n + 1], cols int32, vals float32), indptr absolute ----
// what the C entry points check before any device work: offsets that never go back, at most G entries per row (so a batch of rows
// holds at most batch x G of them: the bound every staging buffer is sized by)
int check_csr_rows(const CsrRows& c, size_t n, int G) {
  SMX_REQUIRE(c.indptr, "CSR rows need indptr");
  SMX_REQUIRE(c.indptr[0] >= 0, "CSR indptr[0] must be >= 0");
  for (size_t i = 0; i < n; ++i)
    SMX_REQUIRE(c.indptr[i + 1] >= c.indptr[i] && c.indptr[i + 1] - c.indptr[i] <= (int64_t)G,
                "CSR indptr must be non-decreasing with at most n_genes entries per row");
  SMX_REQUIRE((c.cols && c.vals) || c.indptr[n] == c.indptr[0], "CSR rows need cols and vals");
  return SMX_OK;
}
// ... and of a matrix given in either form: every entry that takes (x, indptr, cols, vals) calls this once per matrix
int host_rows(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n, int G, HostRows* out) {
  SMX_REQUIRE((x != nullptr) != (indptr != nullptr), "host rows: exactly one of the dense matrix and the CSR arrays");
  SMX_REQUIRE(n >= 1, "host rows: at least one row");
  *out = HostRows{x, CsrRows{indptr, cols, vals}};
  return x ? SMX_OK : check_csr_rows(out->csr, (size_t)n, G);
}

// bytes of a block of n CSR rows with nnz entries as staged on the device: indptr | cols | vals, each 16-byte aligned
static size_t csr_stage_bytes(size_t n, size_t nnz) {
  auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
  return al((n + 1) * 8) + 2 * al(nnz * 4);
}
// rows [r0, r0 + n) of host CSR arrays -> device staging at `dst` (csr_stage_bytes of room) -> the dense tile out [n][Gp] and their
// lgx1 (may be NULL), in ONE launch (launch_csr_rows).  Three contiguous host-to-device copies: the indptr slice, the cols and vals.
static int stage_csr_rows(smx_model* m, const CsrRows& c, size_t r0, size_t n, char* dst, void* out, float* lgx1, int u16 = 0) {
  auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const int64_t e0 = c.indptr[r0];
  const size_t nnz = (size_t)(c.indptr[r0 + n] - e0);
  int64_t* d_ptr = reinterpret_cast<int64_t*>(dst);
  int32_t* d_cols = reinterpret_cast<int32_t*>(dst + al((n + 1) * 8));
  float* d_vals = reinterpret_cast<float*>(dst + al((n + 1) * 8) + al(nnz * 4));
  SMX_HIP(hipMemcpyAsync(d_ptr, c.indptr + r0, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, m->st));
  if (nnz) {
    SMX_HIP(hipMemcpyAsync(d_cols, c.cols + e0, nnz * sizeof(int32_t), hipMemcpyHostToDevice, m->st));
    SMX_HIP(hipMemcpyAsync(d_vals, c.vals + e0, nnz * sizeof(float), hipMemcpyHostToDevice, m->st));
  }
  return launch_csr_rows(m->st, d_ptr, d_cols, d_vals, (long)n, m->G, (long)m->Gp, out, lgx1, u16);
}
// the same through the model's growable buffer m->csr_host (one batch of rows: setup_pass, a batch of CSR targets; a block of
// a dense store uploaded from CSR, u16: the uint16 store)
int csr_host_rows(smx_model* m, const CsrRows& c, size_t r0, size_t n, void* out, float* lgx1, int u16) {
  SMX_CHECK(dgrow(m, &m->csr_host, &m->csr_host_bytes, csr_stage_bytes(n, (size_t)(c.indptr[r0 + n] - c.indptr[r0]))));
  return stage_csr_rows(m, c, r0, n, m->csr_host, out, lgx1, u16);
}

// Decoder layers over `rows` stacked rows (evaluation mode: moving statistics, no dropout; smx_score.hip).  The last
// layer's output: last_form 0 row-major f32 in place, 1 k-major f32 in ht [Hp][rows], 2 its three-way bf16 split in ht.
int stacked_decoder(smx_model* m, const float* z, long rows, float* const* hb, int last_form, float* ht, const float** out, int* out_ld) {
  const float* in = z;
  int ld = m->Dp;
  for (size_t i = 0; i < m->dec.size(); ++i) {
    MlpLayer& L = m->dec[i];
    GemmArgs g;
    g.A = in; g.lda = ld; g.B = P_(m, L.tW); g.ldb = m->tensors[L.tW].ld;
    g.M = (int)rows; g.N = L.out_p; g.K = L.in_p; g.C = hb[i & 1]; g.ldc = L.out_p; g.split_k = 1;
    const bool gen = L.act != SMX_ACT_RELU;   // (not ReLU: the product adds the bias only, score_bn_act's GEN_ACT kernels apply the activation)
    if (L.bn < 0) { g.bias = P_(m, L.tBias); g.act = gen ? 0 : 1; g.leak = L.leak; }
    SMX_CHECK(launch_gemm(m->st, g));
    const bool last = (i + 1 == m->dec.size());
    if (L.bn >= 0 || (last && last_form != 0) || gen) {
      ScoreBnArgs b;
      b.h = hb[i & 1]; b.R = rows; b.H = L.out; b.Hp = L.out_p; b.eps = m->cfg.bn_eps; b.leak = L.leak; b.act = L.act;
      if (L.bn >= 0) {
        b.gamma = P_(m, L.tGamma); b.beta = P_(m, L.tBeta);
        b.moving_mean = m->bn_moving + m->bn_off[L.bn]; b.moving_var = b.moving_mean + L.out_p;
      }
      if (last && last_form == 1) { b.out_t = ht; b.ldt = rows; }
      else if (last && last_form == 2) b.out3 = reinterpret_cast<__bf16*>(ht);
      SMX_CHECK(launch_score_bn_act(m->st, b));
    }
    in = hb[i & 1]; ld = L.out_p;
  }
  *out = in; *out_ld = ld;
  return SMX_OK;
}

// Stacked form (smx_score.hip): the encoder runs once, then the S draws of the B cells go through the decoder and the
// output head as S * B rows at a time (scvi: its library latent drawn per row as well, the raw planes materialised and a
// row-local softmax + likelihood launch, since its rate is normalised over all genes of a row; SCALE: its mixture prior
// in the latent part of log w).
bool stacked_scoring_ok(const smx_model* m) {
  if (!m->flags.stacked_scoring || !m->stochastic || m->use_injected || m->dec.empty()) return false;
  if (m->mixpost) return false;   // (mixture-density posterior: every draw picks its component -- the draw-by-draw form)
  if (m->latent_tril) return false;   // (full-covariance posterior: the draw-by-draw form, whose draws are latent_tril_fwd's)
  if (m->scale && (m->Dp > 64 || m->cfg.n_components > 32 || m->scale_tril)) return false;   // (full-covariance components: the draw-by-draw form, whose prior term is scale_prior_fwd's)
  if (m->scvi && !scvi_score_supported(m->Gp)) return false;
  if (!head_loss_supported(1, m->dec.back().out_p, m->Gp) || (m->dec.back().out_p % 4)) return false;
  for (const MlpLayer& L : m->dec)
    if ((L.in_p % 4) || (L.out_p % 32)) return false;
  return m->dec[0].in_p == m->Dp;
}

// ---- smx_predict's batch loop (predict_core below) -------------------------------------------------------------------------------------
// The device staging of one chunk of cells: its input rows and every requested output, each output segment laid out like the caller's
// array for the chunk's Cn cells (NULL: not asked for)
struct PredChunk {
  size_t Cn = 0, S = 0;   // cells of the chunk, draws per cell
  size_t c0 = 0;          // the chunk's first cell: its row of the call's input
  const StatReq* sr = nullptr;
  char* csr = nullptr;    // CSR input: the chunk's indptr slice | cols | vals (csr_stage_bytes)
  float *in_raw = nullptr, *in_x = nullptr, *in_lib = nullptr, *in_lgx1 = nullptr;   // input: raw rows [Cn][G] (dense), the tile [Cn][Gp], library prior, constants
  float *zm = nullptr, *zs = nullptr, *lm = nullptr, *ls = nullptr;   // latent moments [Cn][D] / [Cn]
  float *zd = nullptr, *ld = nullptr, *xp = nullptr, *st = nullptr;   // draws [S][Cn][D] / [S][Cn], planes [S][k][Cn][G], the statistic
  float *sel = nullptr, *imed = nullptr, *ichg = nullptr;   // the statistic's selected columns [Cn][n_sel]; imputation: median, changed flag (int32) [Cn]
  float* y[SMX_MAX_LABELS] = {};    // label outputs [S][Cn][wy]
  size_t wy[SMX_MAX_LABELS] = {};   // ... their widths per cell and draw
};

// the chunk's input rows from c0 on -> in_x [Cn][Gp], in_lib, in_lgx1 as ONE contiguous copy each: a host-to-device copy per minibatch from
// the caller's pageable array is staged synchronously by the runtime -- ~60 us per batch, at batch 8 (Posterior's default) most of the call.
// Dense rows: raw [Cn][G] -> a device re-pitch to [Cn][Gp] and the rows' likelihood constants from row_stats.  CSR rows: whole batches while
// their non-zeros fit nnz_cap (the first batch always does; Cn shrinks to them), the tile and the constants from one launch.
static int load_chunk(smx_model* m, PredChunk& c, const HostRows& rows, const float* host_library, size_t c0, size_t batch, size_t nnz_cap) {
  const size_t G = (size_t)m->G, Gp = (size_t)m->Gp;
  if (const CsrRows* cx = rows.x ? nullptr : &rows.csr) {
    size_t end = c0;
    while (end < c0 + c.Cn) {
      const size_t nxt = std::min(end + batch, c0 + c.Cn);
      if (end > c0 && (size_t)(cx->indptr[nxt] - cx->indptr[c0]) > nnz_cap) break;
      end = nxt;
    }
    c.Cn = end - c0;
    SMX_REQUIRE((size_t)(cx->indptr[c0 + c.Cn] - cx->indptr[c0]) <= nnz_cap, "CSR chunk exceeds its staging");
    SMX_CHECK(stage_csr_rows(m, *cx, c0, c.Cn, c.csr, c.in_x, c.in_lgx1));
  } else {
    SMX_HIP(hipMemcpyAsync(c.in_raw, rows.x + c0 * G, c.Cn * G * sizeof(float), hipMemcpyHostToDevice, m->st));
    if (Gp != G) SMX_HIP(hipMemsetAsync(c.in_x, 0, c.Cn * Gp * sizeof(float), m->st));
    PackList pl(m->st, (unsigned)std::min<size_t>(1024, (c.Cn * G + 255) / 256), 1, (int)c.Cn);
    SMX_CHECK(pl.add(c.in_x, Gp, c.in_raw, G, G));
    SMX_CHECK(pl.flush());
    SMX_CHECK(launch_row_stats(m->st, c.in_x, 0, (long)Gp, (long)c.Cn, m->G, c.in_lgx1, nullptr));
  }
  if (host_library) SMX_HIP(hipMemcpyAsync(c.in_lib, host_library + c0 * 2, c.Cn * 2 * sizeof(float), hipMemcpyHostToDevice, m->st));
  return SMX_OK;
}

// the statistic of the planes P of Sn draws (stacked rows) of the batch at b0 into the chunk's staging
static int stat_of(smx_model* m, const PredChunk& c, const Pass& ps, const float* P, long ldp, int Sn, size_t s0, size_t b0) {
  const StatReq& sr = *c.sr;
  const size_t G = (size_t)m->G, Cn = c.Cn;
  if (sr.stat == 4) {   // predictive samples: the chunk's staging is [n_k][S][Cn][G]
    SampleArgs q;
    q.P = P; q.ldp = ldp; q.plane_stride = m->Gp; q.B = ps.B; q.Sn = Sn; q.G = m->G; q.lk = m->cfg.likelihood; q.direct = m->scvi ? 1 : 0;
    q.count_only = sr.count_only; q.n_k = sr.n_k; q.k0 = (uint32_t)(sr.seed & 0xFFFFFFFFu); q.k1 = (uint32_t)(sr.seed >> 32);
    q.row0 = (uint32_t)(c.c0 + b0); q.s0 = (uint32_t)s0;
    q.dst = c.st + (s0 * Cn + b0) * G; q.dst_k = (long)(c.S * Cn * G); q.dst_draw = (long)(Cn * G);
    return launch_plane_sample(m->st, q);
  }
  StatArgs a;
  a.P = P; a.ldp = ldp; a.plane_stride = m->Gp; a.B = ps.B; a.Sn = Sn; a.G = m->G; a.lk = m->cfg.likelihood; a.direct = m->scvi ? 1 : 0;
  a.count_only = sr.count_only; a.stat = sr.stat; a.inv_S = 1.f / (float)c.S; a.accumulate = s0 > 0 ? 1 : 0;
  a.T = nullptr; a.ldt = 0; a.trows = nullptr; a.t_u16 = 0;
  if (sr.stat == 2) { a.dst = c.st + b0 * G; a.dst_draw = 0; }
  else if (sr.stat == 3) {
    a.dst = c.st + s0 * Cn + b0; a.dst_draw = (long)Cn;
    if (sr.target.x || sr.target.csr.indptr) { a.T = m->pred_target; a.ldt = m->Gp; }
    else { a.T = ps.Xsrc; a.ldt = m->Gp; a.trows = ps.xrows; a.t_u16 = ps.x_u16; }   // the input rows themselves
  } else { a.dst = c.st + (s0 * Cn + b0) * G; a.dst_draw = (long)(Cn * G); }
  return launch_plane_stat(m->st, a);
}

// the latent moments of the batch at b0 (the encoders' outputs of the pass in flight) onto a pack list into the chunk's staging
static int add_latent_moments(smx_model* m, PackList& pl, const PredChunk& c, size_t b0) {
  const size_t D = (size_t)m->D, Dp = (size_t)m->Dp;
  SMX_CHECK(pl.add(c.zm ? c.zm + b0 * D : nullptr, D, m->mixpost ? m->zmean : m->latbuf, m->mixpost ? Dp : m->lat_planes * Dp, D));
  if (m->latent_tril) SMX_CHECK(pl.add(c.zs ? c.zs + b0 * D * D : nullptr, D * D, m->ltril, D * D, D * D));   // (the factor L [D][D] per cell)
  else SMX_CHECK(pl.add(c.zs ? c.zs + b0 * D : nullptr, D, m->sig, Dp, D));
  SMX_CHECK(pl.add(c.lm ? c.lm + b0 : nullptr, 1, m->latlbuf, 32, 1));
  return pl.add(c.ls ? c.ls + b0 : nullptr, 1, m->lsig, 1, 1);
}

// One batch in the stacked form: the encoder once, then the draws of the batch as rows of one decoder pass (as the scoring paths,
// smx_score.hip) -- at batch 8 x 10 draws (Posterior's defaults, posterior.py:114-115) the draw-by-draw form is 50 launches per 8 cells.
// ids: the draw kernel's noise ids of the pass's rows (NULL: the row index).  need_dec: run the decoder and the heads at all.
static int predict_batch_stacked(smx_model* m, const PredChunk& c, const Pass& ps, size_t b0, const int32_t* ids, bool need_dec) {
  const int B = ps.B, Dp = m->Dp;
  const size_t S = c.S, Cn = c.Cn, G = (size_t)m->G, D = (size_t)m->D, k = (size_t)m->k;
  SMX_CHECK(forward_pass(m, ps, Loss::None, Fwd::EncodeOnly));
  int Hmax = 0, lab_floats = 0;
  for (const MlpLayer& L : m->dec) Hmax = std::max(Hmax, L.out_p);
  for (int j = 0; j < m->n_heads; ++j) lab_floats += c.y[j] ? m->tensors[m->t_labW[j]].ld : 0;
  const size_t ldp = k * (size_t)m->Gp;
  const int Sc = (int)std::min<size_t>(S, std::max<size_t>(1, (size_t)4096 / (size_t)B));   // draws per pass
  const size_t R = (size_t)Sc * B;
  SMX_CHECK(dgrow(m, &m->score_buf, &m->score_floats, R * ((size_t)Dp + 1 + 2 * (size_t)Hmax + ldp + (size_t)lab_floats)));
  float* zst = m->score_buf;
  float* lwst = zst + R * Dp;
  float* hb[2] = {lwst + R, lwst + R + R * Hmax};
  float* Pst = hb[1] + R * Hmax;
  float* yst = Pst + R * ldp;
  {
    PackList pl(m->st, 8, 1, B);
    SMX_CHECK(add_latent_moments(m, pl, c, b0));
    SMX_CHECK(pl.flush());
  }
  for (size_t s0 = 0; s0 < S; s0 += (size_t)Sc) {
    const int Sn = (int)std::min<size_t>((size_t)Sc, S - s0);
    const long rows = (long)Sn * B;
    ScoreDrawArgs d;
    d.lat = m->latbuf; d.ld = 2 * Dp; d.B = B; d.D = m->D; d.Dp = Dp; d.S = Sn; d.s0 = (int)s0;
    d.nk = make_key(m, ST_EPS_Z, 0, false); d.rows = ids; d.cell_base = ps.cell_base; d.z = zst; d.lw = lwst;
    SMX_CHECK(launch_score_draws(m->st, d));
    const float* hl = nullptr; int hld = 0;
    if (need_dec) { SMX_CHECK(stacked_decoder(m, zst, rows, hb, 0, nullptr, &hl, &hld)); m->audit_stk = {(long)R, rows, 0}; }
    PackList pl(m->st, (unsigned)std::min<size_t>(64, ((size_t)B * std::max(G, D) + 255) / 256), (unsigned)Sn, B);
    SMX_CHECK(pl.add(c.zd ? c.zd + (s0 * Cn + b0) * D : nullptr, D, zst, (size_t)Dp, D, Cn * D, (size_t)B * Dp));
    if (c.xp || c.st) {
      GemmArgs g;
      g.A = hl; g.lda = hld; g.B = P_(m, m->t_outW[0]); g.ldb = m->tensors[m->t_outW[0]].ld;
      g.C = Pst; g.ldc = (int)ldp; g.M = (int)rows; g.N = (int)ldp; g.K = hld; g.bias = P_(m, m->t_outb[0]); g.split_k = 1;
      SMX_CHECK(launch_gemm(m->st, g));
      for (size_t q = 0; q < k && c.xp; ++q)
        SMX_CHECK(pl.add(c.xp + ((s0 * k + q) * Cn + b0) * G, G, Pst + q * (size_t)m->Gp, ldp, G, k * Cn * G, (size_t)B * ldp));
      if (c.st) SMX_CHECK(stat_of(m, c, ps, Pst, (long)ldp, Sn, s0, b0));
    }
    float* ycur = yst;
    for (int j = 0; j < m->n_heads; ++j) {
      if (!c.y[j]) continue;
      const TensorInfo& tw = m->tensors[m->t_labW[j]];
      GemmArgs g;
      g.A = hl; g.lda = hld; g.B = P_(m, m->t_labW[j]); g.ldb = tw.ld;
      g.C = ycur; g.ldc = tw.ld; g.M = (int)rows; g.N = tw.ld; g.K = hld; g.bias = P_(m, m->t_labb[j]); g.split_k = 1;
      SMX_CHECK(launch_gemm(m->st, g));
      const size_t P = (size_t)m->cfg.label_dim[j], Pp = (size_t)m->lab_Pp[j], ld = (size_t)tw.ld, wy = c.wy[j];
      for (size_t q = 0; q < (size_t)m->lab_ky[j]; ++q)
        SMX_CHECK(pl.add(c.y[j] + (s0 * Cn + b0) * wy + q * P, wy, ycur + q * Pp, ld, P, Cn * wy, (size_t)B * ld));
      ycur += R * ld;
    }
    SMX_CHECK(pl.flush());
  }
  return SMX_OK;
}

// One batch draw by draw (smx_forward's kernels: bit-identical with it batch by batch).  The encoders run once per batch (eval mode: no
// noise in them); later draws re-sample the latents and decode.
static int predict_batch_drawwise(smx_model* m, const PredChunk& c, Pass& ps, size_t b0, bool need_dec) {
  const int B = ps.B;
  const size_t S = c.S, Cn = c.Cn, G = (size_t)m->G, D = (size_t)m->D, k = (size_t)m->k;
  for (size_t s = 0; s < S; ++s) {
    ps.sample = (int)s;
    // the encoders run once; a single draw nobody decodes stops at the latent moments
    const Fwd first = (need_dec || S > 1) ? Fwd::Full : Fwd::EncodeOnly;
    SMX_CHECK(forward_pass(m, ps, Loss::None, s == 0 ? first : Fwd::Resample));
    PackList pl(m->st, (unsigned)std::min<size_t>(256, ((size_t)B * std::max(G, D) + 255) / 256), 1, B);
    if (s == 0) SMX_CHECK(add_latent_moments(m, pl, c, b0));
    SMX_CHECK(pl.add(c.zd ? c.zd + (s * Cn + b0) * D : nullptr, D, m->z, (size_t)m->Dp, D));
    SMX_CHECK(pl.add(c.ld ? c.ld + s * Cn + b0 : nullptr, 1, m->lsmp, 1, 1));
    for (size_t q = 0; q < k && c.xp; ++q) SMX_CHECK(pl.add(c.xp + ((s * k + q) * Cn + b0) * G, G, m->P + q * (size_t)m->Gp, k * (size_t)m->Gp, G));
    if (c.st) SMX_CHECK(stat_of(m, c, ps, m->P, (long)(k * (size_t)m->Gp), 1, s, b0));
    for (int j = 0; j < m->n_heads; ++j) {
      if (!c.y[j]) continue;
      const size_t P = (size_t)m->cfg.label_dim[j], Pp = (size_t)m->lab_Pp[j], ld = (size_t)m->tensors[m->t_labW[j]].ld, wy = c.wy[j];
      for (size_t q = 0; q < (size_t)m->lab_ky[j]; ++q) SMX_CHECK(pl.add(c.y[j] + (s * Cn + b0) * wy + q * P, wy, m->laby_raw[j] + q * Pp, ld, P));
    }
    SMX_CHECK(pl.flush());
  }
  return SMX_OK;
}

}  // namespace smx

extern "C" {

int smx_forward(smx_model* m, const int32_t* row_ids, const float* host_x, const float* host_library, int32_t batch,
                int32_t sample_index, int32_t training, float* z_mean, float* z_scale, float* z_sample, float* l_mean,
                float* l_scale, float* l_sample, float* x_params, float* const* y_params) {
  SMX_REQUIRE(m, "null model");
  Pass ps;
  SMX_CHECK(setup_pass(m, ps, {row_ids, {host_x}, host_library}, batch, training, sample_index));
  SMX_REQUIRE(!(training && !row_ids), "training-mode forward needs resident rows");
  SMX_CHECK(forward_pass(m, ps, Loss::None));
  return fetch_forward(m, batch, z_mean, z_scale, z_sample, l_mean, l_scale, l_sample, x_params, y_params, 0);
}

int smx_forward_samples(smx_model* m, const int32_t* row_ids, const float* host_x, const float* host_library, int32_t batch,
                        int32_t n_samples, float* z_mean, float* z_scale, float* z_samples, float* l_mean, float* l_scale,
                        float* l_samples, float* x_params, float* const* y_params) {
  SMX_REQUIRE(m && n_samples > 0, "bad arguments");
  // several draws of a host batch: smx_predict over this one batch (same cell ids, same draws, same output layouts) decodes
  // them as rows of one pass instead of one decoder pass per draw
  if (!row_ids && host_x && n_samples > 1 && batch > 0 && batch <= m->Bmax && stacked_scoring_ok(m) && !m->scvi)
    return smx_predict(m, host_x, nullptr, nullptr, nullptr, host_library, batch, batch, n_samples, z_mean, z_scale, z_samples, l_mean, l_scale, l_samples, x_params, y_params);
  Pass ps;
  SMX_CHECK(setup_pass(m, ps, {row_ids, {host_x}, host_library}, batch, 0, 0));
  const size_t B = (size_t)batch;
  for (int s = 0; s < n_samples; ++s) {
    ps.sample = s;
    // the encoders run once (eval mode: no noise in them); later draws re-sample the latents and decode
    SMX_CHECK(forward_pass(m, ps, Loss::None, s == 0 ? Fwd::Full : Fwd::Resample));
    SMX_CHECK(fetch_forward(m, batch, s == 0 ? z_mean : nullptr, s == 0 ? z_scale : nullptr,
                            z_samples ? z_samples + (size_t)s * B * m->D : nullptr, s == 0 ? l_mean : nullptr,
                            s == 0 ? l_scale : nullptr, l_samples ? l_samples + (size_t)s * B : nullptr,
                            x_params ? x_params + (size_t)s * m->k * B * m->G : nullptr, y_params, (size_t)s));
  }
  return SMX_OK;
}

// rows (and a statistic's target): n_cells rows each, as the entry's host_rows checked them
static int predict_core(smx_model* m, const HostRows& rows, const float* host_library, int64_t n_cells, int32_t batch, int32_t n_samples, PredWant o) {
  SMX_REQUIRE(n_samples > 0, "bad arguments");
  SMX_REQUIRE(batch > 0 && batch <= m->Bmax, "batch must be in 1..max_batch");
  const StatReq* const sr = o.sr;
  const bool cx = rows.x == nullptr;   // CSR rows
  const size_t N = (size_t)n_cells, G = (size_t)m->G, Gp = (size_t)m->Gp, D = (size_t)m->D, k = (size_t)m->k, S = (size_t)n_samples;
  const size_t DS = m->latent_tril ? D * D : D;   // z_scale per cell: the factor L [D][D] of a tril posterior, the standard deviations otherwise
  if (!m->stochastic) o.z_scale = nullptr;
  if (!m->scvi) o.l_mean = o.l_scale = o.l_samples = nullptr;
  PredChunk ch;
  ch.S = S; ch.sr = sr;
  for (int j = 0; j < m->n_heads; ++j)
    if (o.y_params && o.y_params[j]) ch.wy[j] = (size_t)m->lab_ky[j] * (size_t)m->cfg.label_dim[j];
  // the requested statistic of the gene output, per cell: S G (mean / variance per draw), G (mean over the draws), S (log_prob)
  // (predictive samples: n_k S G)
  const size_t w_stat = !sr ? 0 : sr->stat == 2 ? G : sr->stat == 3 ? S : sr->stat == 4 ? (size_t)sr->n_k * S * G : S * G;
  // ---- the staging of a chunk of C cells, segment by segment in this order: (where, floats per cell, asked for).  Input rows: see
  // load_chunk; CSR rows have no raw [C][G] segment, their tile comes right after the CSR region (16-byte aligned for launch_csr_rows'
  // float4 stores) ----
  struct Seg { float** at; size_t w; bool on; };
  static_assert(SMX_MAX_LABELS == 4, "one segment per label head");
  const Seg plan[] = {
      {&ch.in_x, Gp, cx},
      {&ch.zm, D, o.z_mean != nullptr}, {&ch.zs, DS, o.z_scale != nullptr}, {&ch.lm, 1, o.l_mean != nullptr}, {&ch.ls, 1, o.l_scale != nullptr},
      {&ch.zd, S * D, o.z_samples != nullptr}, {&ch.ld, S, o.l_samples != nullptr}, {&ch.xp, S * k * G, o.x_params != nullptr},
      {&ch.st, w_stat, w_stat > 0},
      {&ch.sel, sr ? (size_t)sr->n_sel : 0, sr && sr->n_sel > 0 && !sr->keep_cols}, {&ch.imed, 1, sr && sr->impute}, {&ch.ichg, 1, sr && sr->impute},
      {&ch.in_raw, G, !cx}, {&ch.in_x, Gp, !cx}, {&ch.in_lib, 2, true}, {&ch.in_lgx1, 1, true},
      {&ch.y[0], S * ch.wy[0], ch.wy[0] > 0}, {&ch.y[1], S * ch.wy[1], ch.wy[1] > 0}, {&ch.y[2], S * ch.wy[2], ch.wy[2] > 0},
      {&ch.y[3], S * ch.wy[3], ch.wy[3] > 0}};
  size_t per_cell = 0;
  for (const Seg& g : plan) per_cell += g.on ? g.w : 0;
  SMX_REQUIRE(per_cell > (cx ? 0 : G) + Gp + 3, "no output requested");
  const bool impute = sr && sr->impute;
  const bool t_dev = sr && (sr->stat == 3 || impute) && (sr->target.x || sr->target.csr.indptr);   // targets other than the input rows
  if (t_dev) SMX_CHECK(dgrow(m, &m->pred_target, &m->pred_target_floats, (size_t)batch * Gp, (size_t)m->Bmax * Gp));   // a batch of target rows
  // 128 MB of staging (knob predict_stage_floats: tests force several chunks on small problems)
  const size_t cap_floats = (size_t)std::max(1.0, tuning("predict_stage_floats", (double)((size_t)32 << 20)));
  size_t C = std::max<size_t>((size_t)batch, cap_floats / per_cell / (size_t)batch * (size_t)batch);   // whole batches per chunk
  C = std::min(C, (N + (size_t)batch - 1) / (size_t)batch * (size_t)batch);
  // CSR rows: a chunk is also cut, at a batch boundary, where its non-zeros would pass nnz_cap; a batch holds at most batch x G of them
  // (check_csr_rows), so one batch always fits and a dense region only makes the chunks shorter
  const size_t nnz_cap = cx ? std::max((size_t)batch * G, std::min(C * G, cap_floats / 2)) : 0;
  const size_t csr_floats = cx ? csr_stage_bytes(C, nnz_cap) / 4 : 0;   // (a multiple of 16 bytes)
  SMX_CHECK(dgrow(m, &m->pred_stage, &m->pred_floats, csr_floats + C * per_cell));
  ch.csr = reinterpret_cast<char*>(m->pred_stage);
  float* at = m->pred_stage + csr_floats;
  for (const Seg& g : plan)
    if (g.on) { *g.at = at; at += C * g.w; }
  // the stacked form: with several draws, and for a statistic request at any draw count (smx_predict itself keeps the draw-by-draw
  // kernels at one draw: bit-identical with smx_forward batch by batch)
  const bool stack = (S > 1 || sr != nullptr) && stacked_scoring_ok(m) && !m->scvi;
  // SUPER-BATCHES: in evaluation mode nothing couples the rows of a minibatch (moving statistics, no dropout) but the noise ids -- a
  // cell's id is its index within ITS minibatch -- so the stacked form takes k minibatches per pass (k batch <= max_batch) and hands the
  // draw kernel the ids (row % batch): same numbers, 1 / k of the launches (at Posterior's batch 8 a pass is ~12 launches per 8 cells)
  size_t step = (size_t)batch;
  if (stack && (size_t)m->Bmax >= 2 * (size_t)batch) {
    step = (size_t)batch * ((size_t)m->Bmax / (size_t)batch);
    if (m->pred_ids_batch != batch) {
      if (!m->pred_ids) SMX_HIP(hipMalloc((void**)&m->pred_ids, (size_t)m->Bmax * sizeof(int32_t)));
      std::vector<int32_t> ids((size_t)m->Bmax);
      for (int i = 0; i < m->Bmax; ++i) ids[(size_t)i] = i % batch;
      SMX_HIP(hipMemcpy(m->pred_ids, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      m->pred_ids_batch = batch;
    }
  }
  SMX_REQUIRE(!m->scvi || host_library, "scvi needs host_library with host rows");
  bool any_y = false;
  for (int j = 0; j < m->n_heads; ++j) any_y = any_y || ch.y[j] != nullptr;
  const bool need_dec = ch.xp || ch.st || any_y;   // (latents only: the decoder and the heads are not run at all)
  auto out = [&](float* dst, const float* src, size_t count) -> int {   // one contiguous device -> host copy
    SMX_HIP(hipMemcpyAsync(dst, src, count * sizeof(float), hipMemcpyDeviceToHost, m->st));
    return SMX_OK;
  };
  // ---- imputation (smx_impute.hip): the histograms of the global selection, and d = |original - mean| of all cells when N G floats fit the
  // budget (knob impute_keep_bytes; default: half of the free device memory) -- otherwise levels 2 and 3 REPEAT the walk (level > 0 below:
  // the same passes give the same bits, every draw being a function of counters), each pass's rows of d going through a small scratch ----
  bool keep_d = false;
  if (impute) {
    SMX_REQUIRE(t_dev && sr->imp_median && sr->imp_changed && sr->imp_lohi, "imputation needs the original rows and its three outputs");
    if (!m->imp_hist) SMX_CHECK(dmalloc(&m->imp_hist, (size_t)SMX_IMP_HIST_WORDS));
    SMX_HIP(hipMemsetAsync(m->imp_hist, 0, (size_t)SMX_IMP_HIST_WORDS * sizeof(unsigned long long), m->st));
    double budget = tuning("impute_keep_bytes", -1.0);
    if (budget < 0.0) {
      size_t fr = 0, tot = 0;
      SMX_HIP(hipMemGetInfo(&fr, &tot));
      budget = 0.5 * (double)(fr + m->imp_d_floats * sizeof(float));
    }
    keep_d = (double)N * (double)G * 4.0 <= budget;
    SMX_CHECK(dgrow(m, &m->imp_d, &m->imp_d_floats, keep_d ? N * G : (size_t)m->Bmax * G));
  }
  unsigned long long* const lv_hist = impute ? m->imp_hist + SMX_IMP_L1_BINS : nullptr;
  // level 0: the walk itself.  level 1 / 2 (imputation without the kept d): the passes again, nothing copied out, the pass's rows of d
  // into the histogram of bits `shift`.. under the prefixes
  auto walk = [&](int level, const unsigned* prefix, unsigned mask, int shift) -> int {
  for (size_t c0 = 0; c0 < N; c0 += ch.Cn) {
    ch.Cn = std::min(C, N - c0);   // cells of this chunk (CSR rows: load_chunk may take fewer)
    ch.c0 = c0;
    SMX_CHECK(load_chunk(m, ch, rows, host_library, c0, (size_t)batch, nnz_cap));
    const size_t Cn = ch.Cn;
    for (size_t b0 = 0; b0 < Cn; b0 += step) {
      const int B = (int)std::min<size_t>(step, Cn - b0);
      const size_t g0 = c0 + b0;
      Pass ps = host_rows_pass(B, ch.in_x + b0 * Gp, ch.in_lib + b0 * 2, ch.in_lgx1 + b0);   // (on the chunk's resident copy)
      if (t_dev && sr->target.csr.indptr) SMX_CHECK(csr_host_rows(m, sr->target.csr, g0, (size_t)B, m->pred_target, nullptr));
      else if (t_dev)
        SMX_HIP(hipMemcpy2DAsync(m->pred_target, Gp * sizeof(float), sr->target.x + g0 * G, G * sizeof(float), G * sizeof(float), (size_t)B,
                                 hipMemcpyHostToDevice, m->st));
      if (stack) SMX_CHECK(predict_batch_stacked(m, ch, ps, b0, step > (size_t)batch ? m->pred_ids : nullptr, need_dec));
      else SMX_CHECK(predict_batch_drawwise(m, ch, ps, b0, need_dec));
      if (impute) {   // the rows' means over the draws are complete: their medians, flags and share of the level-1 histogram; or their d alone
        ImputeRowArgs ia;
        ia.mean = ch.st + b0 * G; ia.ldm = (long)G; ia.orig = m->pred_target; ia.ldo = (long)Gp; ia.cor = ch.in_x + b0 * Gp; ia.ldc = (long)Gp;
        ia.G = m->G; ia.d_only = level > 0 ? 1 : 0; ia.d = keep_d ? m->imp_d + g0 * G : (level > 0 ? m->imp_d : nullptr);
        ia.median = ch.imed + b0; ia.changed = reinterpret_cast<int32_t*>(ch.ichg) + b0; ia.hist = m->imp_hist;
        SMX_CHECK(launch_impute_rows(m->st, ia, B));
        if (level > 0) SMX_CHECK(launch_impute_level(m->st, m->imp_d, (long)((size_t)B * G), prefix, mask, shift, lv_hist));
      }
    }
    if (level > 0) { SMX_HIP(hipStreamSynchronize(m->st)); continue; }
    // ---- the chunk leaves the device: every segment's rows are contiguous here and in the caller's arrays ----
    if (ch.zm) SMX_CHECK(out(o.z_mean + c0 * D, ch.zm, Cn * D));
    if (ch.zs) SMX_CHECK(out(o.z_scale + c0 * DS, ch.zs, Cn * DS));
    if (ch.lm) SMX_CHECK(out(o.l_mean + c0, ch.lm, Cn));
    if (ch.ls) SMX_CHECK(out(o.l_scale + c0, ch.ls, Cn));
    if (ch.st && sr->keep_cols) SMX_CHECK(launch_keep_cols(m->st, ch.st, (long)G, (long)Cn, sr->sel, sr->n_sel, sr->keep_cols, (long)N, (long)c0));
    else if (ch.st && sr->stat == 2 && !impute && !ch.sel) SMX_CHECK(out(sr->out + c0 * G, ch.st, Cn * G));
    if (ch.sel) {
      SMX_CHECK(launch_gather_cols(m->st, ch.st, (long)G, (long)Cn, sr->sel, sr->n_sel, ch.sel));
      SMX_CHECK(out(sr->out + c0 * (size_t)sr->n_sel, ch.sel, Cn * (size_t)sr->n_sel));
    }
    if (impute) {
      SMX_CHECK(out(sr->imp_median + c0, ch.imed, Cn));
      SMX_CHECK(out(reinterpret_cast<float*>(sr->imp_changed) + c0, ch.ichg, Cn));
    }
    for (size_t s = 0; s < S && ch.st && sr->stat == 4; ++s)
      for (size_t q = 0; q < (size_t)sr->n_k; ++q) SMX_CHECK(out(sr->out + ((q * S + s) * N + c0) * G, ch.st + (q * S + s) * Cn * G, Cn * G));
    for (size_t s = 0; s < S && ch.st && sr->stat != 2 && sr->stat != 4; ++s) {
      if (sr->stat == 3) SMX_CHECK(out(sr->out + s * N + c0, ch.st + s * Cn, Cn));
      else SMX_CHECK(out(sr->out + (s * N + c0) * G, ch.st + s * Cn * G, Cn * G));
    }
    for (size_t s = 0; s < S; ++s) {
      if (ch.zd) SMX_CHECK(out(o.z_samples + (s * N + c0) * D, ch.zd + s * Cn * D, Cn * D));
      if (ch.ld) SMX_CHECK(out(o.l_samples + s * N + c0, ch.ld + s * Cn, Cn));
      if (ch.xp)
        for (size_t c = 0; c < k; ++c) SMX_CHECK(out(o.x_params + ((s * k + c) * N + c0) * G, ch.xp + (s * k + c) * Cn * G, Cn * G));
      for (int j = 0; j < m->n_heads; ++j)
        if (ch.y[j]) SMX_CHECK(out(o.y_params[j] + (s * N + c0) * ch.wy[j], ch.y[j] + s * Cn * ch.wy[j], Cn * ch.wy[j]));
    }
    SMX_HIP(hipStreamSynchronize(m->st));
  }
  return SMX_OK;
  };
  SMX_CHECK(walk(0, nullptr, 0u, 0));
  if (!impute) return SMX_OK;
  // ---- the two middle order statistics of all N G entries of d: ranks (NG - 1) / 2 and NG / 2, 64-bit.  Level 1 (bits 30..20) came with
  // the walk; the host picks each rank's bin, levels 2 (bits 19..10) and 3 (bits 9..0) count inside the picked prefixes ----
  std::vector<unsigned long long> h((size_t)SMX_IMP_HIST_WORDS);
  SMX_HIP(hipMemcpy(h.data(), m->imp_hist, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const bool any_nan = h[(size_t)SMX_IMP_HIST_WORDS - 1] != 0;
  const unsigned long long NG = (unsigned long long)N * (unsigned long long)G;
  unsigned long long rank[2] = {(NG - 1) / 2, NG / 2};
  unsigned prefix[2] = {0u, 0u};
  auto pick = [&](const unsigned long long* bins, int n_bins, int t, int shift) -> int {
    unsigned long long cum = 0;
    for (int b = 0; b < n_bins; ++b) {
      if (rank[t] < cum + bins[b]) { prefix[t] |= (unsigned)b << shift; rank[t] -= cum; return SMX_OK; }
      cum += bins[b];
    }
    set_error("imputation: the selection histogram does not hold the rank");
    return SMX_ERR_HIP;
  };
  for (int t = 0; t < 2; ++t) SMX_CHECK(pick(h.data(), SMX_IMP_L1_BINS, t, 20));
  unsigned mask = 0xFFF00000u;
  for (int shift = 10; shift >= 0; shift -= 10) {
    SMX_HIP(hipMemsetAsync(lv_hist, 0, (size_t)2 * SMX_IMP_LN_BINS * sizeof(unsigned long long), m->st));
    if (keep_d) SMX_CHECK(launch_impute_level(m->st, m->imp_d, (long)(N * G), prefix, mask, shift, lv_hist));
    else SMX_CHECK(walk(shift == 10 ? 1 : 2, prefix, mask, shift));
    SMX_HIP(hipStreamSynchronize(m->st));
    SMX_HIP(hipMemcpy(h.data(), lv_hist, (size_t)2 * SMX_IMP_LN_BINS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int t = 0; t < 2; ++t) SMX_CHECK(pick(h.data() + (size_t)t * SMX_IMP_LN_BINS, SMX_IMP_LN_BINS, t, shift));
    mask |= (unsigned)(SMX_IMP_LN_BINS - 1) << shift;
  }
  for (int t = 0; t < 2; ++t) {   // (a NaN anywhere: np.median's answer)
    const unsigned v = any_nan ? 0x7FC00000u : prefix[t];
    memcpy(sr->imp_lohi + t, &v, sizeof(float));
  }
  return SMX_OK;
}

int smx_predict(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals, const float* host_library,
                int64_t n_cells, int32_t batch, int32_t n_samples, float* z_mean, float* z_scale, float* z_samples, float* l_mean,
                float* l_scale, float* l_samples, float* x_params, float* const* y_params) {
  SMX_REQUIRE(m, "null model");
  HostRows rows;
  SMX_CHECK(host_rows(host_x, indptr, cols, vals, n_cells, m->G, &rows));
  return predict_core(m, rows, host_library, n_cells, batch, n_samples,
                      {nullptr, z_mean, z_scale, z_samples, l_mean, l_scale, l_samples, x_params, y_params});
}

int smx_predict_stat(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals, const float* host_library,
                     int64_t n_cells, int32_t batch, int32_t n_samples, int32_t stat, int32_t count_only, const float* target,
                     const int64_t* t_indptr, const int32_t* t_cols, const float* t_vals, float* out) {
  SMX_REQUIRE(m && out && stat >= 0 && stat <= 3, "bad arguments (stat: 0 mean, 1 variance, 2 mean over the draws, 3 log_prob)");
  SMX_REQUIRE(!(count_only && m->cfg.likelihood == SMX_LLK_MSE), "the deterministic 'mse' output has no count distribution");
  HostRows rows;
  StatReq sr;
  SMX_CHECK(host_rows(host_x, indptr, cols, vals, n_cells, m->G, &rows));
  if (target || t_indptr) SMX_CHECK(host_rows(target, t_indptr, t_cols, t_vals, n_cells, m->G, &sr.target));
  sr.stat = stat; sr.count_only = count_only ? 1 : 0; sr.out = out;
  return predict_core(m, rows, host_library, n_cells, batch, n_samples, {&sr});
}

// stat 2 restricted to n_sel gene columns: the indices are checked here and go to the device once
int smx_predict_stat_cols(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals,
                          const float* host_library, int64_t n_cells, int32_t batch, int32_t n_samples, int32_t count_only, const int32_t* genes,
                          int32_t n_sel, float* out) {
  SMX_REQUIRE(m && out && genes && n_sel > 0, "bad arguments");
  SMX_REQUIRE(!(count_only && m->cfg.likelihood == SMX_LLK_MSE), "the deterministic 'mse' output has no count distribution");
  HostRows rows;
  SMX_CHECK(host_rows(host_x, indptr, cols, vals, n_cells, m->G, &rows));
  for (int i = 0; i < n_sel; ++i) SMX_REQUIRE(genes[i] >= 0 && genes[i] < m->G, "gene index out of range");
  SMX_CHECK(dgrow(m, &m->pred_sel, &m->pred_sel_n, (size_t)n_sel));
  SMX_HIP(hipMemcpy(m->pred_sel, genes, (size_t)n_sel * sizeof(int32_t), hipMemcpyHostToDevice));
  StatReq sr;
  sr.stat = 2; sr.count_only = count_only ? 1 : 0; sr.out = out; sr.sel = m->pred_sel; sr.n_sel = n_sel;
  return predict_core(m, rows, host_library, n_cells, batch, n_samples, {&sr});
}

// the correlation sums of the walk's stat 2 (smx_correlate.hip): the selected genes in chunks of Gc whose kept columns, ranks and sort arrays
// (16 N bytes per gene) fit the knob correlate_keep_bytes; every chunk repeats the walk -- the same passes, the same bits
int smx_predict_correlate(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals,
                          const float* host_library, int64_t n_cells, int32_t batch, int32_t n_samples, int32_t count_only, const int32_t* genes,
                          int32_t n_sel, const int32_t* prot_rank2, const double* prot_unit, int32_t P, int64_t* sp_Sa, int64_t* sp_Saa,
                          int64_t* sp_Sab, double* pe_mean, double* pe_Sxx, double* pe_Sxy, int32_t* nonfinite) {
  SMX_REQUIRE(m && prot_rank2 && prot_unit && P > 0 && sp_Sa && sp_Saa && sp_Sab && pe_mean && pe_Sxx && pe_Sxy && nonfinite, "bad arguments");
  SMX_REQUIRE(n_cells > 0 && n_cells <= SMX_COR_MAX_CELLS, "correlations take 1 .. 2^20 cells");
  SMX_REQUIRE(!(count_only && m->cfg.likelihood == SMX_LLK_MSE), "the deterministic 'mse' output has no count distribution");
  SMX_REQUIRE(genes ? n_sel > 0 : true, "an empty gene list");
  HostRows rows;
  SMX_CHECK(host_rows(host_x, indptr, cols, vals, n_cells, m->G, &rows));
  const size_t n = genes ? (size_t)n_sel : (size_t)m->G, N = (size_t)n_cells, pn = (size_t)P * N;
  std::vector<int32_t> idx(n);
  for (size_t i = 0; i < n; ++i) {
    idx[i] = genes ? genes[i] : (int32_t)i;
    SMX_REQUIRE(idx[i] >= 0 && idx[i] < m->G, "gene index out of range");
  }
  SMX_CHECK(dgrow(m, &m->pred_sel, &m->pred_sel_n, n));
  SMX_HIP(hipMemcpy(m->pred_sel, idx.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  double budget = tuning("correlate_keep_bytes", -1.0);
  if (budget < 0.0) {
    size_t fr = 0, tot = 0;
    SMX_HIP(hipMemGetInfo(&fr, &tot));
    budget = 0.5 * (double)(fr + m->cor_keep_bytes);
  }
  const size_t Gc = (size_t)std::min((double)n, std::max(1.0, floor(budget / (16.0 * (double)N))));
  SMX_CHECK(dgrow(m, &m->cor_keep, &m->cor_keep_bytes, Gc * N * 16));
  SMX_CHECK(dgrow(m, &m->cor_ops, &m->cor_ops_bytes, pn * 12 + correlate_sums_bytes(Gc, (size_t)P) + 16));
  CorrelateWork w;
  w.cols = reinterpret_cast<float*>(m->cor_keep); w.rank2 = reinterpret_cast<int32_t*>(w.cols + Gc * N);
  w.sortA = reinterpret_cast<unsigned*>(w.rank2 + Gc * N); w.sortB = w.sortA + Gc * N;
  double* d_unit = reinterpret_cast<double*>(m->cor_ops);
  int32_t* d_rank = reinterpret_cast<int32_t*>(d_unit + pn);
  w.prot_unit = d_unit; w.prot_rank2 = d_rank;
  w.sums = m->cor_ops + (pn * 12 + 15) / 16 * 16;
  SMX_HIP(hipMemcpy(d_unit, prot_unit, pn * sizeof(double), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(d_rank, prot_rank2, pn * sizeof(int32_t), hipMemcpyHostToDevice));
  for (size_t g0 = 0; g0 < n; g0 += Gc) {
    const int gc = (int)std::min(Gc, n - g0);
    StatReq sr;
    sr.stat = 2; sr.count_only = count_only ? 1 : 0; sr.sel = m->pred_sel + g0; sr.n_sel = gc; sr.keep_cols = w.cols;
    SMX_CHECK(predict_core(m, rows, host_library, n_cells, batch, n_samples, {&sr}));
    const CorrelateOut o{reinterpret_cast<long long*>(sp_Sa) + g0, reinterpret_cast<long long*>(sp_Saa) + g0, reinterpret_cast<long long*>(sp_Sab) + g0 * (size_t)P,
                         pe_mean + g0, pe_Sxx + g0, pe_Sxy + g0 * (size_t)P, nonfinite + g0};
    SMX_CHECK(correlate_kept(m->st, w, gc, (long)N, P, o));
  }
  return SMX_OK;
}

// the imputation scores of the walk's stat 2 (smx_impute.hip)
int smx_predict_impute(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals, const float* host_library,
                       int64_t n_cells, int32_t batch, int32_t n_samples, int32_t count_only, const float* original, const int64_t* o_indptr,
                       const int32_t* o_cols, const float* o_vals, float* cell_median, int32_t* cell_changed, float* global_lohi) {
  SMX_REQUIRE(m && cell_median && cell_changed && global_lohi, "bad arguments");
  SMX_REQUIRE(!(count_only && m->cfg.likelihood == SMX_LLK_MSE), "the deterministic 'mse' output has no count distribution");
  HostRows rows;
  StatReq sr;
  SMX_CHECK(host_rows(host_x, indptr, cols, vals, n_cells, m->G, &rows));
  SMX_CHECK(host_rows(original, o_indptr, o_cols, o_vals, n_cells, m->G, &sr.target));
  sr.stat = 2; sr.count_only = count_only ? 1 : 0;
  sr.impute = 1; sr.imp_median = cell_median; sr.imp_changed = cell_changed; sr.imp_lohi = global_lohi;
  return predict_core(m, rows, host_library, n_cells, batch, n_samples, {&sr});
}

// stat 4 of the walk: n_k samples of the gene output per draw and cell, out [n_k, n_samples, n_cells, n_genes]
int smx_predict_sample(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals, const float* host_library,
                       int64_t n_cells, int32_t batch, int32_t n_samples, int32_t count_only, uint64_t seed, int32_t n_k, float* out) {
  SMX_REQUIRE(m && out && n_k > 0, "bad arguments");
  SMX_REQUIRE(!(count_only && m->cfg.likelihood == SMX_LLK_MSE), "the deterministic 'mse' output has no count distribution");
  SMX_REQUIRE(n_cells <= (int64_t)0xFFFFFFFFll && n_samples <= 65536, "the sampler's counters hold 2^32 cells and 2^16 draws");
  HostRows rows;
  SMX_CHECK(host_rows(host_x, indptr, cols, vals, n_cells, m->G, &rows));
  StatReq sr;
  sr.stat = 4; sr.count_only = count_only ? 1 : 0; sr.out = out; sr.seed = seed; sr.n_k = n_k;
  return predict_core(m, rows, host_library, n_cells, batch, n_samples, {&sr});
}

int smx_decode(smx_model* m, const float* z, const float* l, int32_t batch, float* x_params, float* const* y_params) {
  SMX_REQUIRE(m && z, "null argument");
  SMX_REQUIRE(batch > 0 && batch <= m->Bmax, "batch must be in 1..max_batch");
  SMX_REQUIRE(!m->scvi || l, "scvi decode needs the library latent");
  const Pass ps = host_rows_pass(batch, m->hostX, m->hostLib, m->hostLgx1);
  SMX_HIP(hipMemsetAsync(m->z, 0, (size_t)batch * m->Dp * sizeof(float), m->st));
  SMX_HIP(hipMemcpy2DAsync(m->z, (size_t)m->Dp * sizeof(float), z, (size_t)m->D * sizeof(float), (size_t)m->D * sizeof(float),
                           (size_t)batch, hipMemcpyHostToDevice, m->st));
  if (m->scvi) SMX_HIP(hipMemcpyAsync(m->lsmp, l, (size_t)batch * sizeof(float), hipMemcpyHostToDevice, m->st));
  SMX_CHECK(forward_pass(m, ps, Loss::None, Fwd::DecodeOnly));
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_CHECK(fetch_planes(m, batch, x_params));
  return fetch_labels(m, batch, y_params, 0);
}

}  // extern "C"
