// smx_kapi.hip -- kernel-level entry points (parity tests of single kernels): smx_k_count_llk, smx_k_adam, smx_k_gemm, smx_k_head_fused, smx_k_noise,
// smx_k_bn_fwd / smx_k_bn_bwd, smx_k_opt_carrier (clip + update by every launch that carries the optimiser's chunk body),
// smx_k_scvi_head_train / _fwd / _bwd (the scVI gene head's three launch forms), smx_k_label_loss (the label heads' launch).
#include "smx_model.h"
#include "smx_adam.h"
#include <hiprand/hiprand_kernel.h>

namespace smx {
// The library's noise function against hiprand's own Philox generator (row N-1, "sampling from a hiprand state per wavefront"): thread i
// builds a hiprandStatePhilox4_32_10_t with hiprand_init(seed, subsequence = (c2, c3) = (step, stream | sample << 8), offset =
// 4 * (c0, c1) = 4 * (column block, cell id)) and draws ONE hiprand4 -- and evaluates philox4x32_10(c0, c1, c2, c3, seed) as the kernels do.
__global__ void hiprand_probe_kernel(uint64_t seed, int n, const uint32_t* c, uint32_t* ours, uint32_t* theirs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c0 = c[4 * i], c1 = c[4 * i + 1], c2 = c[4 * i + 2], c3 = c[4 * i + 3];
  const U4 w = philox4x32_10(c0, c1, c2, c3, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32));
  ours[4 * i] = w.x; ours[4 * i + 1] = w.y; ours[4 * i + 2] = w.z; ours[4 * i + 3] = w.w;
  hiprandStatePhilox4_32_10_t st;
  hiprand_init(seed, (unsigned long long)c2 | ((unsigned long long)c3 << 32), 4ull * ((unsigned long long)c0 | ((unsigned long long)c1 << 32)), &st);
  const uint4 r = hiprand4(&st);
  theirs[4 * i] = r.x; theirs[4 * i + 1] = r.y; theirs[4 * i + 2] = r.z; theirs[4 * i + 3] = r.w;
}
// words of a and b that differ, added to *n (the stress entry point below)
__global__ void count_diff_kernel(const uint32_t* a, const uint32_t* b, long n, unsigned* out) {
  unsigned mine = 0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) mine += a[i] != b[i];
  if (mine) atomicAdd(out, mine);
}

// ===========================================================================
// noise probe (tests): what the kernels draw for (cell, column)
// ===========================================================================
__global__ void noise_probe_kernel(NoiseKey nk, const int64_t* cell_ids, int B, int width, float p, float* mult,
                                   float* normal) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * width) return;
  const int b = idx / width, c = idx % width;
  const U4 w = philox_block(nk, (uint32_t)cell_ids[b], (uint32_t)(c >> 2));
  if (mult) mult[idx] = (p > 0.f) ? dropout_mult1(w, c & 3, p, 1.f / (1.f - p)) : 1.f;
  if (normal) {
    const float4 n = normal4(w);
    normal[idx] = (c & 3) == 0 ? n.x : (c & 3) == 1 ? n.y : (c & 3) == 2 ? n.z : n.w;
  }
}
int launch_noise_probe(hipStream_t st, NoiseKey nk, const int64_t* cell_ids, int B, int width, float p, float* mult,
                       float* normal) {
  hipLaunchKernelGGL(noise_probe_kernel, dim3((B * width + 255) / 256), dim3(256), 0, st, nk, cell_ids, B, width, p,
                     mult, normal);
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}
}  // namespace smx

// Every entry point below takes its device memory from a DeviceScratch declared before its first allocation: whichever way it returns,
// the memory is freed.
namespace {
// the key of a probe: what make_key gives a step's launches, from the caller's (seed, stream, sample, step)
NoiseKey probe_key(uint64_t seed, int stream, int sample, int step) {
  NoiseKey nk;
  nk.k0 = (uint32_t)(seed & 0xFFFFFFFFu); nk.k1 = (uint32_t)(seed >> 32); nk.step = (uint32_t)step;
  nk.stream = (uint32_t)((stream & 0xFF) | ((sample & 0xFFFFFF) << 8)); nk.step_ptr = nullptr; nk.draw_rows = 0;
  return nk;
}
// llk[b] = the row's likelihood partials part[b][n_chunks] summed in float64, less sum_g lgamma(x + 1) (not of the 'bernoulli' /
// 'normal' densities); x [B][G] on the host
void llk_rows(const std::vector<float>& part, int n_chunks, const float* x, int B, int G, int likelihood, float* llk) {
  for (int b = 0; b < B; ++b) {
    double s = 0.0;
    for (int c = 0; c < n_chunks; ++c) s += part[(size_t)b * n_chunks + c];
    if (likelihood != SMX_LLK_BERNOULLI && likelihood != SMX_LLK_NORMAL)
      for (int g = 0; g < G; ++g) { const float v = x[(size_t)b * G + g]; if (v > 0.f) s -= lgamma((double)v + 1.0); }
    llk[b] = (float)s;
  }
}
}  // namespace

extern "C" {

int smx_k_hiprand(uint64_t seed, int32_t n, const uint32_t* counters, uint32_t* ours, uint32_t* hiprand_words) {
  SMX_REQUIRE(n > 0 && counters && ours && hiprand_words, "bad arguments");
  DeviceScratch buf;
  uint32_t *dC, *dO, *dH;
  SMX_CHECK(buf.put(&dC, counters, (size_t)4 * n));
  SMX_CHECK(buf.get(&dO, (size_t)4 * n));
  SMX_CHECK(buf.get(&dH, (size_t)4 * n));
  hipLaunchKernelGGL(smx::hiprand_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, seed, (int)n, dC, dO, dH);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(ours, dO, (size_t)16 * n, hipMemcpyDeviceToHost));
  SMX_HIP(hipMemcpy(hiprand_words, dH, (size_t)16 * n, hipMemcpyDeviceToHost));
  return SMX_OK;
}

// ---- kernel-level entry points ------------------------------------------------
int smx_k_count_llk(int likelihood, int direct, const float* x, const float* planes, int32_t B, int32_t G, float* llk,
                    float* grads) {
  SMX_REQUIRE(x && planes && llk && B > 0 && G > 0, "bad arguments");
  const int k = llk_planes(likelihood);
  const int Gp = round_up(G, 32);
  const int nch = loss_chunks(Gp, B);
  DeviceScratch buf;
  float *dX, *dPl, *dG, *dPart;
  SMX_CHECK(buf.get(&dX, (size_t)B * Gp));
  SMX_CHECK(buf.get(&dPl, (size_t)B * k * Gp));
  SMX_CHECK(buf.get(&dG, (size_t)B * k * Gp));
  SMX_CHECK(buf.get(&dPart, (size_t)B * nch));
  SMX_HIP(hipMemcpy2D(dX, (size_t)Gp * 4, x, (size_t)G * 4, (size_t)G * 4, (size_t)B, hipMemcpyHostToDevice));
  for (int c = 0; c < k; ++c)
    SMX_HIP(hipMemcpy2D(dPl + (size_t)c * Gp, (size_t)k * Gp * 4, planes + (size_t)c * B * G, (size_t)G * 4, (size_t)G * 4,
                        (size_t)B, hipMemcpyHostToDevice));
  LossArgs lo;
  lo.likelihood = likelihood; lo.direct = direct; lo.backward = grads != nullptr;
  lo.X = dX; lo.ldx = Gp; lo.P = dPl; lo.ldp = (long)k * Gp; lo.plane_stride = Gp; lo.dP = dG; lo.llk_part = dPart;
  lo.B = B; lo.G = G; lo.Gp = Gp; lo.grad_scale = 1.f;
  SMX_CHECK(launch_count_loss(nullptr, lo));
  std::vector<float> part((size_t)B * nch);
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(part.data(), dPart, part.size() * 4, hipMemcpyDeviceToHost));
  llk_rows(part, nch, x, B, G, likelihood, llk);
  if (grads)
    for (int c = 0; c < k; ++c)
      SMX_HIP(hipMemcpy2D(grads + (size_t)c * B * G, (size_t)G * 4, dG + (size_t)c * Gp, (size_t)k * Gp * 4, (size_t)G * 4,
                          (size_t)B, hipMemcpyDeviceToHost));
  return SMX_OK;
}

// the optimiser launch over caller-given tensors under `rule` (resolved hyper-parameters hp[4]): smx_k_adam / smx_k_opt
static int k_opt_launch(int rule, const float* hp, int32_t n_tensors, const int32_t* sizes, float* params, const float* grads, float* mom,
                        float* vel, int32_t step, float lr, float clipnorm, float* norms) {
  SMX_REQUIRE(n_tensors > 0 && n_tensors <= SMX_MAX_TENSORS && sizes && params && grads && mom && vel && step >= 1, "bad arguments");
  // the model's own layout: every tensor padded to a multiple of 64 floats, 4096-float optimiser chunks
  std::vector<size_t> off((size_t)n_tensors), pad((size_t)n_tensors);
  std::vector<OptChunk> chunks;
  size_t total = 0;
  const int CH = 4096;
  for (int t = 0; t < n_tensors; ++t) {
    SMX_REQUIRE(sizes[t] > 0, "empty tensor");
    off[t] = total; pad[t] = ((size_t)sizes[t] + 63) / 64 * 64;
    const int first = (int)chunks.size(), n = (int)((pad[t] + CH - 1) / CH);
    for (int i = 0; i < n; ++i) {
      OptChunk c;
      memset(&c, 0, sizeof(c));
      c.tensor = t; c.offset = (int)(off[t] + (size_t)i * CH);
      c.count = (int)((size_t)(i + 1) * CH <= pad[t] ? CH : pad[t] - (size_t)i * CH);
      c.first_chunk = first; c.n_chunks = n; c.tensor_count = (int32_t)pad[t];
      chunks.push_back(c);
    }
    total += pad[t];
  }
  StepState st3[3];
  memset(st3, 0, sizeof(st3));
  st3[2].next = (uint32_t)(step - 1);   // optimiser steps completed so far
  const float2 sch = make_float2(0.f, lr);   // the one-step schedule table: (beta, lr)
  DeviceScratch buf;
  float *dP, *dG, *dM, *dV, *dPart, *dNorm;
  OptChunk* dCh; StepState* dSt; float2* dSch;
  SMX_CHECK(buf.get(&dP, total));
  SMX_CHECK(buf.get(&dG, total));
  SMX_CHECK(buf.get(&dM, total));
  SMX_CHECK(buf.get(&dV, total));
  SMX_CHECK(buf.get(&dPart, chunks.size()));
  SMX_CHECK(buf.get(&dNorm, (size_t)n_tensors));
  SMX_CHECK(buf.put(&dCh, chunks.data(), chunks.size()));
  SMX_CHECK(buf.put(&dSt, st3, (size_t)3));
  SMX_CHECK(buf.put(&dSch, &sch, (size_t)1));
  auto put = [&](float* dst, const float* src) -> int {
    size_t lo = 0;
    for (int t = 0; t < n_tensors; ++t) {
      SMX_HIP(hipMemcpy(dst + off[t], src + lo, (size_t)sizes[t] * sizeof(float), hipMemcpyHostToDevice));
      lo += (size_t)sizes[t];
    }
    return SMX_OK;
  };
  auto get = [&](float* dst, const float* src) -> int {
    size_t lo = 0;
    for (int t = 0; t < n_tensors; ++t) {
      SMX_HIP(hipMemcpy(dst + lo, src + off[t], (size_t)sizes[t] * sizeof(float), hipMemcpyDeviceToHost));
      lo += (size_t)sizes[t];
    }
    return SMX_OK;
  };
  SMX_CHECK(put(dP, params)); SMX_CHECK(put(dG, grads)); SMX_CHECK(put(dM, mom)); SMX_CHECK(put(dV, vel));
  // the step's scalars exactly as a training step prepares them (bias-corrected step size on the device)
  AdamArgs a;
  opt_scalars(rule, hp, a);   // (t0 = 0: the rule's count t is the step given)
  SMX_CHECK(launch_step_begin(nullptr, dSt + 2, dSt, nullptr, nullptr, 0, 0, 0u, dSch, a.b1, a.b2, a.form, 0u));
  a.params = dP; a.grads = dG; a.m = dM; a.v = dV; a.chunks = dCh; a.n_chunks = (int)chunks.size(); a.n_launch = a.n_chunks; a.gap_from = a.n_chunks; a.gap_len = 0;
  a.partial = dPart; a.tensor_norm = dNorm; a.use_sq = 0; a.state = dSt;
  a.clipnorm = clipnorm; a.grad_scale = 1.f; a.sched = dSch;
  SMX_CHECK(launch_adam(nullptr, a));
  SMX_HIP(hipDeviceSynchronize());
  SMX_CHECK(get(params, dP)); SMX_CHECK(get(mom, dM)); SMX_CHECK(get(vel, dV));
  if (norms) SMX_HIP(hipMemcpy(norms, dNorm, (size_t)n_tensors * sizeof(float), hipMemcpyDeviceToHost));
  return SMX_OK;
}

int smx_k_adam(int32_t n_tensors, const int32_t* sizes, float* params, const float* grads, float* mom, float* vel,
               int32_t step, float lr, float beta1, float beta2, float eps, float clipnorm, float* norms) {
  const float hp[4] = {beta1, beta2, eps, 0.f};
  return k_opt_launch(SMX_OPT_ADAM, hp, n_tensors, sizes, params, grads, mom, vel, step, lr, clipnorm, norms);
}

int smx_k_opt(int32_t rule, const float* hp, int32_t n_hp, int32_t n_tensors, const int32_t* sizes, float* params, const float* grads,
              float* m, float* v, int32_t step, float lr, float clipnorm, float* norms) {
  static const float adam_hp[3] = {0.9f, 0.999f, 1e-7f};
  float res[4];
  SMX_CHECK(opt_resolve(rule, hp, n_hp, adam_hp, res));
  return k_opt_launch(rule, res, n_tensors, sizes, params, grads, m, v, step, lr, clipnorm, norms);
}

int smx_k_gemm(int transA, int transB, const float* A, const float* B, int32_t M, int32_t N, int32_t K, int32_t split_k,
               int32_t tile_cfg, float* C) {
  SMX_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, "bad arguments");
  // tile_cfg 100 / 101 / 102: the bf16 x 3 forms outside the LDS-tiled kernel -- smx_dgemm.hip (A [M][K]; K padded to 32 with
  // zeros), the 32 x 32-tile weight-gradient kernel and the panel form of smx_panel.h (both: A [K][M], Bm [K][N], M padded to 32)
  // tile_cfg 103: the gene-axis contraction of smx_bigk.hip (A [M][K], B in either layout; K padded to 32 with zeros): slices from
  // bigk_slices, per-slice slabs and the reduce launch as the step builds them (dd_bigk), identity rows, float32 A, no log1p
  const bool direct = tile_cfg == 100, wg = tile_cfg == 101 || tile_cfg == 102, bigk = tile_cfg == 103;
  SMX_REQUIRE(!direct || !transA, "tile 100 (dgemm) takes A as [M][K]");
  SMX_REQUIRE(!bigk || !transA, "tile 103 (bigk) takes A as [M][K]");
  SMX_REQUIRE(!wg || (transA && !transB), "tiles 101 / 102 (weight-gradient forms) take A as [K][M] and B as [K][N]");
  SMX_REQUIRE(tile_cfg != 102 || N <= 128, "tile 102 (panel form): N <= 128");
  // pad to the library's internal conventions: feature axes to 32, batch axes free
  const int Np = round_up(N, 32);
  const int Kp = (direct || bigk) ? round_up(K, 32) : round_up(K, 4), Mp = wg ? round_up(M, 32) : round_up(M, 4);
  const int lda = transA ? Mp : Kp, a_rows = transA ? K : M, a_cols = transA ? M : K;
  const int ldb = transB ? Kp : Np, b_rows = transB ? N : K, b_cols = transB ? K : N;
  const int S = split_k < 1 ? 1 : split_k;
  const int rowsC = transA ? Mp : M;   // (rows of C beyond M, when M was padded for k-major A, are never stored)
  DeviceScratch buf;
  float *dA, *dB, *dC;
  SMX_CHECK(buf.get(&dA, (size_t)a_rows * lda));
  SMX_CHECK(buf.get(&dB, (size_t)round_up(b_rows, 32) * ldb));
  SMX_CHECK(buf.get(&dC, (size_t)S * rowsC * Np));
  SMX_HIP(hipMemcpy2D(dA, (size_t)lda * 4, A, (size_t)a_cols * 4, (size_t)a_cols * 4, (size_t)a_rows, hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy2D(dB, (size_t)ldb * 4, B, (size_t)b_cols * 4, (size_t)b_cols * 4, (size_t)b_rows, hipMemcpyHostToDevice));
  GemmArgs g;
  g.A = dA; g.lda = lda; g.a_kmajor = transA; g.B = dB; g.ldb = ldb; g.b_nmajor = transB;
  g.C = dC; g.ldc = Np; g.slab_stride = (long)rowsC * Np; g.M = rowsC; g.N = Np; g.K = (transA) ? K : Kp;
  g.split_k = S; g.tile = tile_cfg;
  int eff = 1, rc;
  if (direct) {
    g.K = Kp;   // (the padding of A and B is zero: dmalloc clears)
    SMX_REQUIRE(dgemm_supported(g), "tile 100 (dgemm): K >= 512 after padding to 32, split_k = 1");
    rc = launch_dgemm(nullptr, g);
  } else if (bigk) {
    BigKArgs bk;
    bk.A = dA; bk.lda = lda; bk.Bm = dB; bk.ldb = ldb; bk.b_kmajor = transB ? 0 : 1;
    bk.M = M; bk.N = Np; bk.K = Kp; bk.ldc = Np; bk.slab_stride = (long)M * Np; bk.out = dC;
    bk.n_slices = bigk_slices(bk.K, SMX_BIGK_MAX_SLICES, &bk.k_chunk);
    SMX_CHECK(buf.get(&bk.part, (size_t)bk.n_slices * (size_t)bk.slab_stride));
    SMX_REQUIRE(S == 1 && bigk_supported(bk), "tile 103 (bigk): K >= 4096 after padding to 32, split_k = 1");
    rc = launch_bigk(nullptr, bk);
  } else if (wg) {
    g.split_k = 1; g.panel_hint = tile_cfg == 102;
    SMX_REQUIRE(S == 1 && wgrad_supported(g, K), "tiles 101 / 102: split_k = 1");
    rc = launch_wgrad_group(nullptr, &g, 1, K, 1);
  } else
  rc = launch_gemm(nullptr, g, &eff);
  SMX_CHECK(rc);
  if (tuning("kgemm_reps", 0) > 0 && !direct && !wg && !bigk) {  // diagnostic: average launch time of this shape / tile
    const int reps = (int)tuning("kgemm_reps", 0);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 5; ++i) launch_gemm(nullptr, g, nullptr);
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < reps; ++i) launch_gemm(nullptr, g, nullptr);
    hipEventRecord(e1, nullptr);
    hipEventSynchronize(e1);
    float ms = 0.f; hipEventElapsedTime(&ms, e0, e1);
    fprintf(stderr, "k_gemm tA=%d tB=%d M=%d N=%d K=%d split=%d tile=%d: %.2f us\n", transA, transB, M, N, K, eff, tile_cfg,
            1e3f * ms / reps);
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  SMX_HIP(hipDeviceSynchronize());
  std::vector<float> h((size_t)eff * rowsC * Np);
  SMX_HIP(hipMemcpy(h.data(), dC, h.size() * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      float s = 0.f;
      for (int z = 0; z < eff; ++z) s += h[((size_t)z * rowsC + i) * Np + j];
      C[(size_t)i * N + j] = s;
    }
  return SMX_OK;
}

// The fused head's operands on the device and its HeadFusedArgs but for the output pointers (dW, db, part, llk_part, sq_part): x [B][G] as
// float32 and, u16 != 0, as the uint16 image the launch then reads; d [B][128]; W [128][k][G] plane by plane into [128][k * Gp]; bias
// [k][G] into [k * Gp]; the table
static int head_fused_stage(DeviceScratch& buf, int likelihood, int u16, const float* x, const float* d, const float* W, const float* bias,
                            int B, int G, float grad_scale, HeadFusedArgs* a) {
  const int k = llk_planes(likelihood), Gp = round_up(G, 32), H = 128;
  float *dX, *dD, *dWt, *dBias, *dTab;
  uint16_t* dX16;
  SMX_CHECK(buf.get(&dTab, (size_t)SMX_HEAD_FUSED_TAB_BYTES / 4));
  SMX_CHECK(buf.get(&dX, (size_t)B * Gp));
  SMX_CHECK(buf.get(&dX16, (size_t)B * Gp));
  SMX_CHECK(buf.put(&dD, d, (size_t)B * H));
  SMX_CHECK(buf.get(&dWt, (size_t)H * k * Gp));
  SMX_CHECK(buf.get(&dBias, (size_t)k * Gp));
  SMX_HIP(hipMemcpy2D(dX, (size_t)Gp * 4, x, (size_t)G * 4, (size_t)G * 4, (size_t)B, hipMemcpyHostToDevice));
  if (u16) {
    std::vector<uint16_t> h16((size_t)B * Gp, 0);
    for (int b = 0; b < B; ++b)
      for (int g = 0; g < G; ++g) h16[(size_t)b * Gp + g] = (uint16_t)x[(size_t)b * G + g];
    SMX_HIP(hipMemcpy(dX16, h16.data(), h16.size() * 2, hipMemcpyHostToDevice));
  }
  for (int c = 0; c < k; ++c) {
    SMX_HIP(hipMemcpy2D(dWt + (size_t)c * Gp, (size_t)k * Gp * 4, W + (size_t)c * G, (size_t)k * G * 4, (size_t)G * 4, (size_t)H, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(dBias + (size_t)c * Gp, bias + (size_t)c * G, (size_t)G * 4, hipMemcpyHostToDevice));
  }
  a->D = dD; a->ldd = H; a->W = dWt; a->ldw = (long)k * Gp; a->bias = dBias;
  a->X = u16 ? (const void*)dX16 : (const void*)dX; a->ldx = Gp; a->x_u16 = u16 ? 1 : 0;
  a->slab_stride = (long)B * H; a->dtab = dTab;
  a->B = B; a->G = G; a->Gp = Gp; a->likelihood = likelihood; a->grad_scale = grad_scale;
  return SMX_OK;
}

// The fused output head of smx_headfused.hip over host arrays (H = 128 decoder columns, B <= 128 cells, G >= 4096 genes): W [128][k][G]
// (plane-major columns, as the model's head), bias [k][G], x [B][G] (u16 != 0: the counts travel through the uint16 store).  Out: llk [B], dW [128][k][G], db [k][G], dd [B][128], sumsq (of dW; may be NULL); us (may be
// NULL): average device time of `reps` launches of the fused kernel (HIP events; without the reduce launch).
int smx_k_head_fused(int likelihood, int u16, const float* x, const float* d, const float* W, const float* bias, int32_t B, int32_t G,
                     float grad_scale, int32_t reps, float* llk, float* dW, float* db, float* dd, float* sumsq, float* us) {
  SMX_REQUIRE(x && d && W && bias && llk && dW && db && dd && B > 0 && G > 0, "bad arguments");
  const int k = llk_planes(likelihood);
  const int Gp = round_up(G, 32), H = 128;
  SMX_REQUIRE(head_fused_supported(B, H, Gp, k), "head_fused: unsupported shape (B <= 256, G >= 4096 after padding, 2 or 3 planes)");
  const int grid = head_fused_grid(Gp), n_gt = head_fused_chunks(Gp);
  DeviceScratch buf;
  HeadFusedArgs a;
  SMX_CHECK(head_fused_stage(buf, likelihood, u16, x, d, W, bias, B, G, grad_scale, &a));
  float* dDd;
  SMX_CHECK(buf.get(&a.dW, (size_t)H * k * Gp));
  SMX_CHECK(buf.get(&a.db, (size_t)k * Gp));
  SMX_CHECK(buf.get(&a.part, (size_t)grid * B * H));
  SMX_CHECK(buf.get(&a.llk_part, (size_t)B * n_gt));
  SMX_CHECK(buf.get(&a.sq_part, (size_t)grid * 8));
  SMX_CHECK(buf.get(&dDd, (size_t)B * H));
  if (tuning("hf_dbg", 0) > 0) SMX_CHECK(buf.get(&a.dbg, (size_t)128));
  int n_sq = 0, n_slabs = 0;
  SMX_CHECK(launch_head_fused(nullptr, a, &n_slabs, &n_sq));
  SMX_CHECK(launch_head_fused_reduce(nullptr, a, n_slabs, dDd));
  if (reps > 0 && us) {
    int rc = SMX_OK;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < reps && rc == SMX_OK; ++i) rc = launch_head_fused(nullptr, a, &n_slabs, &n_sq);
    hipEventRecord(e1, nullptr);
    hipEventSynchronize(e1);
    float ms = 0.f; hipEventElapsedTime(&ms, e0, e1);
    *us = 1e3f * ms / (float)reps;
    hipEventDestroy(e0); hipEventDestroy(e1);
    SMX_CHECK(rc);
  }
  SMX_HIP(hipDeviceSynchronize());
  if (a.dbg) {
    long long h[128];
    hipMemcpy(h, a.dbg, sizeof(h), hipMemcpyDeviceToHost);
    for (int b = 0; b < 2; ++b) {
      fprintf(stderr, "hf stamps block %d: (prologue %lld)", b ? 100 : 0, h[64 * b] - h[64 * b + 63]);
      for (int i = 1; i < 62 && h[64 * b + i]; ++i) fprintf(stderr, " %lld", h[64 * b + i] - h[64 * b + i - 1]);
      fprintf(stderr, "\n");
    }
  }
  std::vector<float> part((size_t)B * n_gt), sq((size_t)n_sq);
  SMX_HIP(hipMemcpy(part.data(), a.llk_part, part.size() * 4, hipMemcpyDeviceToHost));
  llk_rows(part, n_gt, x, B, G, likelihood, llk);
  for (int c = 0; c < k; ++c) {
    SMX_HIP(hipMemcpy2D(dW + (size_t)c * G, (size_t)k * G * 4, a.dW + (size_t)c * Gp, (size_t)k * Gp * 4, (size_t)G * 4, (size_t)H, hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy(db + (size_t)c * G, a.db + (size_t)c * Gp, (size_t)G * 4, hipMemcpyDeviceToHost));
  }
  SMX_HIP(hipMemcpy(dd, dDd, (size_t)B * H * 4, hipMemcpyDeviceToHost));
  if (sumsq) {
    SMX_HIP(hipMemcpy(sq.data(), a.sq_part, sq.size() * 4, hipMemcpyDeviceToHost));
    double s = 0.0;
    for (float v : sq) s += v;
    *sumsq = (float)s;
  }
  return SMX_OK;
}

// The fused head launched `launches` times on the same inputs; every launch after the first is compared on the device, bit for bit, with
// what the first one left (dW, db, the d d slabs, the likelihood partials).  *n_differ = launches that differed anywhere, *first_word = index
// of the first differing word of the first differing launch within [dW | db | slabs | partials] (-1 if none).  Two timing-dependent wrong
// results of this kernel were hardware behaviour that no single launch shows reliably (tools/isa_lint.py); this is their regression test.
int smx_k_head_fused_stress(int likelihood, int u16, const float* x, const float* d, const float* W, const float* bias, int32_t B, int32_t G,
                            float grad_scale, int32_t launches, int32_t* n_differ, int64_t* first_word) {
  SMX_REQUIRE(x && d && W && bias && n_differ && B > 0 && B <= 128 && G > 0 && launches >= 2, "bad arguments");
  const int k = llk_planes(likelihood);
  const int Gp = round_up(G, 32), H = 128;
  SMX_REQUIRE(head_fused_supported(B, H, Gp, k), "head_fused: unsupported shape");
  const int grid = head_fused_grid(Gp), n_gt = head_fused_chunks(Gp);
  const size_t nW = (size_t)H * k * Gp, nb = (size_t)k * Gp, nP = (size_t)grid * B * H, nL = (size_t)B * n_gt, nOut = nW + nb + nP + nL;
  DeviceScratch buf;
  HeadFusedArgs a;
  SMX_CHECK(head_fused_stage(buf, likelihood, u16, x, d, W, bias, B, G, grad_scale, &a));
  float *dOut, *dRef;
  unsigned* dN;
  SMX_CHECK(buf.get(&dOut, nOut));
  SMX_CHECK(buf.get(&dRef, nOut));
  SMX_CHECK(buf.get(&a.sq_part, (size_t)grid * 8));
  SMX_CHECK(buf.get(&dN, (size_t)1));
  a.dW = dOut; a.db = dOut + nW; a.part = dOut + nW + nb; a.llk_part = dOut + nW + nb + nP;
  int n_sq = 0, n_slabs = 0, differ = 0;
  long long first = -1;
  std::vector<uint32_t> ho, hr;
  for (int it = 0; it < launches; ++it) {
    SMX_HIP(hipMemsetAsync(dOut, 0xFF, nOut * 4, nullptr));
    SMX_CHECK(launch_head_fused(nullptr, a, &n_slabs, &n_sq));
    if (it == 0) { SMX_HIP(hipMemcpyAsync(dRef, dOut, nOut * 4, hipMemcpyDeviceToDevice, nullptr)); continue; }
    SMX_HIP(hipMemsetAsync(dN, 0, 4, nullptr));
    hipLaunchKernelGGL(smx::count_diff_kernel, dim3(1024), dim3(256), 0, nullptr, reinterpret_cast<const uint32_t*>(dOut), reinterpret_cast<const uint32_t*>(dRef), (long)nOut, dN);
    unsigned n = 0;
    SMX_HIP(hipMemcpy(&n, dN, 4, hipMemcpyDeviceToHost));
    if (n) {
      ++differ;
      if (first < 0) {
        ho.resize(nOut); hr.resize(nOut);
        SMX_HIP(hipMemcpy(ho.data(), dOut, nOut * 4, hipMemcpyDeviceToHost)); SMX_HIP(hipMemcpy(hr.data(), dRef, nOut * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nOut; ++i) if (ho[i] != hr[i]) { first = (long long)i; break; }
      }
    }
  }
  SMX_HIP(hipDeviceSynchronize());
  *n_differ = differ;
  if (first_word) *first_word = first;
  return SMX_OK;
}

int smx_k_noise(uint64_t seed, int32_t stream, int32_t step, int32_t sample, const int64_t* cell_ids, int32_t B, int32_t width,
                float dropout_p, float* dropout_mult, float* normal) {
  SMX_REQUIRE(cell_ids && B > 0 && width > 0, "bad arguments");
  DeviceScratch buf;
  int64_t* dIds; float *dM, *dN;
  SMX_CHECK(buf.put(&dIds, cell_ids, (size_t)B));
  SMX_CHECK(buf.get(&dM, (size_t)B * width));
  SMX_CHECK(buf.get(&dN, (size_t)B * width));
  SMX_CHECK(launch_noise_probe(nullptr, probe_key(seed, stream, sample, step), dIds, B, width, dropout_p, dM, dN));
  SMX_HIP(hipDeviceSynchronize());
  if (dropout_mult) SMX_HIP(hipMemcpy(dropout_mult, dM, (size_t)B * width * 4, hipMemcpyDeviceToHost));
  if (normal) SMX_HIP(hipMemcpy(normal, dN, (size_t)B * width * 4, hipMemcpyDeviceToHost));
  return SMX_OK;
}

}  // extern "C"

// ---- the BatchNorm launches by themselves (smx_bn.hip: launch_bn_act_fwd / launch_bn_act_bwd pick the form; no front, no riders) ----------
namespace {
// An output buffer between two guard bands.  Bands and interior start as 0xFF bytes (a NaN no kernel computes): an element the launch
// never wrote reads as NaN, and a store beside the buffer changes a band word.  The memory is the call's DeviceScratch's.
constexpr size_t KBN_GUARD = 256;   // floats on either side
struct KbnOut {
  float* base = nullptr; size_t n = 0;
  float* p() const { return base + KBN_GUARD; }
  int alloc(DeviceScratch& buf, size_t count) {
    n = count ? count : 1;
    SMX_CHECK(buf.get(&base, n + 2 * KBN_GUARD));
    SMX_HIP(hipMemset(base, 0xFF, (n + 2 * KBN_GUARD) * 4));
    return SMX_OK;
  }
  int upload(const float* src, size_t count) { SMX_HIP(hipMemcpy(p(), src, count * 4, hipMemcpyHostToDevice)); return SMX_OK; }
  int download(float* dst, size_t count) const { if (dst) SMX_HIP(hipMemcpy(dst, p(), count * 4, hipMemcpyDeviceToHost)); return SMX_OK; }
  int intact(bool* ok) const {
    std::vector<uint32_t> h(2 * KBN_GUARD);
    SMX_HIP(hipMemcpy(h.data(), base, KBN_GUARD * 4, hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy(h.data() + KBN_GUARD, base + KBN_GUARD + n, KBN_GUARD * 4, hipMemcpyDeviceToHost));
    for (uint32_t w : h) if (w != 0xFFFFFFFFu) *ok = false;
    return SMX_OK;
  }
};
// SyncBatchNorm on one device: the ranks' gather buffers [world][2][Hp] summed on the host (every other slot is a zero: the sum is exact) and
// handed back to every rank
int kbn_all_reduce(std::vector<KbnOut>& gather, size_t n) {
  std::vector<float> sum(n, 0.f), one(n);
  for (auto& g : gather) {
    SMX_HIP(hipMemcpy(one.data(), g.p(), n * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) sum[i] += one[i];
  }
  for (auto& g : gather) SMX_HIP(hipMemcpy(g.p(), sum.data(), n * 4, hipMemcpyHostToDevice));
  return SMX_OK;
}
}  // namespace

extern "C" {

// ip: S, B, H, Hp, ld, wide, batchnorm, training, update_moving, act, mask_ld, stream, step, cell_base, world; fp: momentum, eps, leak, drop_p
int smx_k_bn_fwd(const int32_t* ip, const float* fp, const float* pre, const float* gamma, const float* beta, const float* bias,
                 const float* moving_mean, const float* moving_var, const float* mask, const int32_t* rows, uint64_t seed, float* out,
                 float* xhat, float* inv_std, float* batch_mean, float* batch_var, float* moving_mean_out, float* moving_var_out,
                 int32_t* guards_ok) {
  SMX_REQUIRE(ip && fp && pre && out && xhat && guards_ok, "k_bn_fwd: bad arguments");
  const int S = ip[0], B = ip[1], H = ip[2], Hp = ip[3], ld = ip[4], wide = ip[5], batchnorm = ip[6], training = ip[7], update_moving = ip[8],
            act = ip[9], mask_ld = ip[10], stream = ip[11], step = ip[12], world = ip[14];
  const uint32_t cell_base = (uint32_t)ip[13];
  SMX_REQUIRE(S > 0 && B > 0 && H > 0 && H <= Hp && Hp % 8 == 0 && (wide || ld >= Hp) && world >= 0 && (!mask || mask_ld >= Hp), "k_bn_fwd: bad shapes");
  SMX_REQUIRE(!batchnorm || (gamma && beta && moving_mean && moving_var), "k_bn_fwd: BatchNorm needs gamma, beta and the moving statistics");
  SMX_REQUIRE(!world || (!wide && batchnorm && training && B % world == 0), "k_bn_fwd: SyncBatchNorm takes plain slabs, training mode and equal shards");
  const long slab = wide ? (long)Hp * 128 : (long)B * ld;
  DeviceScratch buf;
  float *dPre, *dGamma, *dBeta, *dBias, *dMask; int32_t* dRows;
  KbnOut oOut, oXhat, oInv, oMean, oVar, oMm, oMv;
  int rc;
  if ((rc = buf.put(&dPre, pre, (size_t)S * slab)) || (rc = buf.put(&dGamma, gamma, Hp)) || (rc = buf.put(&dBeta, beta, Hp)) || (rc = buf.put(&dBias, bias, Hp)) ||
      (rc = buf.put(&dMask, mask, (size_t)B * mask_ld)) || (rc = buf.put(&dRows, rows, B)) || (rc = oOut.alloc(buf, (size_t)B * Hp)) || (rc = oXhat.alloc(buf, (size_t)B * Hp)) ||
      (rc = oInv.alloc(buf, Hp)) || (rc = oMean.alloc(buf, Hp)) || (rc = oVar.alloc(buf, Hp)) || (rc = oMm.alloc(buf, Hp)) || (rc = oMv.alloc(buf, Hp)))
    return rc;
  if (moving_mean && ((rc = oMm.upload(moving_mean, Hp)) || (rc = oMv.upload(moving_var, Hp)))) return rc;
  BnFwdArgs a;
  a.pre = dPre; a.n_slabs = S; a.slab_stride = slab; a.ld = wide ? Hp : ld;
  a.B = B; a.H = H; a.Hp = Hp; a.batchnorm = batchnorm; a.training = training; a.update_moving = update_moving;
  a.gamma = dGamma; a.beta = dBeta; a.bias = dBias; a.moving_mean = oMm.p(); a.moving_var = oMv.p();
  a.batch_mean = oMean.p(); a.batch_var = oVar.p(); a.momentum = fp[0]; a.eps = fp[1]; a.leak = fp[2]; a.drop_p = fp[3];
  a.xhat = oXhat.p(); a.inv_std = oInv.p(); a.out = oOut.p();
  a.nk = probe_key(seed, stream, 0, step); a.rows = dRows; a.cell_base = cell_base; a.inj_mask = dMask; a.inj_ld = mask_ld;
  a.wide = wide; a.act = act;
  std::vector<KbnOut> gather((size_t)world);
  if (!world) SMX_CHECK(launch_bn_act_fwd(nullptr, a));
  else {
    const int Bs = B / world;
    for (auto& g : gather) if ((rc = g.alloc(buf, (size_t)world * 2 * Hp))) return rc;
    for (int phase = 0; phase < 2; ++phase) {
      for (int k = 0; k < world; ++k) {   // rank k: rows [k Bs, (k + 1) Bs) of every slab
        BnFwdArgs r = a;
        r.B = Bs; r.pre = a.pre + (long)k * Bs * ld; r.xhat = a.xhat + (long)k * Bs * Hp; r.out = a.out + (long)k * Bs * Hp;
        if (a.inj_mask) r.inj_mask = a.inj_mask + (long)k * Bs * mask_ld;
        if (a.rows) r.rows = a.rows + k * Bs; else r.cell_base = cell_base + (uint32_t)(k * Bs);
        BnSyncArgs y; y.gather = gather[k].p(); y.rank = k; y.world = world;
        SMX_CHECK(launch_bn_sync_fwd(nullptr, r, y, phase));
      }
      SMX_HIP(hipDeviceSynchronize());
      if (phase == 0) SMX_CHECK(kbn_all_reduce(gather, (size_t)world * 2 * Hp));
    }
  }
  SMX_HIP(hipDeviceSynchronize());
  bool ok = true;
  for (const KbnOut* o : {&oOut, &oXhat, &oInv, &oMean, &oVar, &oMm, &oMv}) if ((rc = o->intact(&ok))) return rc;
  for (const auto& g : gather) if ((rc = g.intact(&ok))) return rc;
  *guards_ok = ok ? 1 : 0;
  if ((rc = oOut.download(out, (size_t)B * Hp)) || (rc = oXhat.download(xhat, (size_t)B * Hp)) || (rc = oInv.download(inv_std, Hp)) ||
      (rc = oMean.download(batch_mean, Hp)) || (rc = oVar.download(batch_var, Hp)) || (rc = oMm.download(moving_mean_out, Hp)) ||
      (rc = oMv.download(moving_var_out, Hp)))
    return rc;
  return SMX_OK;
}

// ip: S, B, H, Hp, ld, wide, batchnorm, training, act, mask_ld, stream, step, cell_base, world; fp: leak, drop_p.  dgamma / dbeta:
// [max(world, 1)][Hp] (under SyncBatchNorm every rank's share; their sum is the gradient)
int smx_k_bn_bwd(const int32_t* ip, const float* fp, const float* dout, const float* out, const float* xhat, const float* inv_std,
                 const float* gamma, const float* beta, const float* mask, const int32_t* rows, uint64_t seed, float* dpre, float* dgamma,
                 float* dbeta, float* dbias, int32_t* guards_ok) {
  SMX_REQUIRE(ip && fp && dout && out && xhat && dpre && guards_ok, "k_bn_bwd: bad arguments");
  const int S = ip[0], B = ip[1], H = ip[2], Hp = ip[3], ld = ip[4], wide = ip[5], batchnorm = ip[6], training = ip[7], act = ip[8],
            mask_ld = ip[9], stream = ip[10], step = ip[11], world = ip[13];
  const uint32_t cell_base = (uint32_t)ip[12];
  SMX_REQUIRE(S > 0 && B > 0 && H > 0 && H <= Hp && Hp % 8 == 0 && (wide || ld >= Hp) && world >= 0 && (!mask || mask_ld >= Hp), "k_bn_bwd: bad shapes");
  SMX_REQUIRE(!batchnorm || (gamma && beta && inv_std), "k_bn_bwd: BatchNorm needs gamma, beta and inv_std");
  SMX_REQUIRE(!world || (!wide && batchnorm && training && B % world == 0), "k_bn_bwd: SyncBatchNorm takes plain slabs, training mode and equal shards");
  const long slab = wide ? (long)Hp * 128 : (long)B * ld;
  const int nw = world > 1 ? world : 1;
  DeviceScratch buf;
  float *dDout, *dOutF, *dXhat, *dInv, *dGamma, *dBeta, *dMask; int32_t* dRows;
  KbnOut oDpre, oDg, oDb, oDbias;
  int rc;
  if ((rc = buf.put(&dDout, dout, (size_t)S * slab)) || (rc = buf.put(&dOutF, out, (size_t)B * Hp)) || (rc = buf.put(&dXhat, xhat, (size_t)B * Hp)) || (rc = buf.put(&dInv, inv_std, Hp)) ||
      (rc = buf.put(&dGamma, gamma, Hp)) || (rc = buf.put(&dBeta, beta, Hp)) || (rc = buf.put(&dMask, mask, (size_t)B * mask_ld)) || (rc = buf.put(&dRows, rows, B)) ||
      (rc = oDpre.alloc(buf, (size_t)B * Hp)) || (rc = oDg.alloc(buf, (size_t)nw * Hp)) || (rc = oDb.alloc(buf, (size_t)nw * Hp)) || (rc = oDbias.alloc(buf, Hp)))
    return rc;
  BnBwdArgs a;
  a.dout = dDout; a.n_slabs = S; a.slab_stride = slab; a.ld = wide ? Hp : ld;
  a.out = dOutF; a.xhat = dXhat; a.inv_std = dInv; a.gamma = dGamma; a.beta = dBeta;
  a.B = B; a.H = H; a.Hp = Hp; a.batchnorm = batchnorm; a.training = training;
  a.leak = fp[0]; a.drop_p = (training && fp[1] > 0.f) ? fp[1] : 0.f;
  a.drop_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  a.dpre = oDpre.p(); a.dgamma = oDg.p(); a.dbeta = oDb.p(); a.dbias = oDbias.p();
  a.nk = probe_key(seed, stream, 0, step); a.rows = dRows; a.cell_base = cell_base; a.inj_mask = dMask; a.inj_ld = mask_ld;
  a.wide = wide; a.act = act;
  std::vector<KbnOut> gather((size_t)world);
  if (!world) SMX_CHECK(launch_bn_act_bwd(nullptr, a));
  else {
    const int Bs = B / world;
    for (auto& g : gather) if ((rc = g.alloc(buf, (size_t)world * 2 * Hp))) return rc;
    for (int phase = 0; phase < 2; ++phase) {
      for (int k = 0; k < world; ++k) {
        BnBwdArgs r = a;
        r.B = Bs; r.dout = a.dout + (long)k * Bs * ld; r.out = a.out + (long)k * Bs * Hp; r.xhat = a.xhat + (long)k * Bs * Hp;
        r.dpre = a.dpre + (long)k * Bs * Hp; r.dgamma = a.dgamma + (long)k * Hp; r.dbeta = a.dbeta + (long)k * Hp;
        if (a.inj_mask) r.inj_mask = a.inj_mask + (long)k * Bs * mask_ld;
        if (a.rows) r.rows = a.rows + k * Bs; else r.cell_base = cell_base + (uint32_t)(k * Bs);
        BnSyncArgs y; y.gather = gather[k].p(); y.rank = k; y.world = world;
        SMX_CHECK(launch_bn_sync_bwd(nullptr, r, y, phase));
      }
      SMX_HIP(hipDeviceSynchronize());
      if (phase == 0) SMX_CHECK(kbn_all_reduce(gather, (size_t)world * 2 * Hp));
    }
  }
  SMX_HIP(hipDeviceSynchronize());
  bool ok = true;
  for (const KbnOut* o : {&oDpre, &oDg, &oDb, &oDbias}) if ((rc = o->intact(&ok))) return rc;
  for (const auto& g : gather) if ((rc = g.intact(&ok))) return rc;
  *guards_ok = ok ? 1 : 0;
  if ((rc = oDpre.download(dpre, (size_t)B * Hp)) || (rc = oDg.download(dgamma, (size_t)nw * Hp)) || (rc = oDb.download(dbeta, (size_t)nw * Hp)) ||
      (rc = oDbias.download(dbias, Hp)))
    return rc;
  return SMX_OK;
}

}  // extern "C"

// ---- the optimiser's carriers by themselves (smx_adam.h / smx_adam.hip: every launch that runs adam_tensor_clip + opt_apply4) --------------
namespace smx {
// test only: the 512-thread chunk body (a rider of the 512-thread launches in a training step; it cannot be launched alone there)
__global__ __launch_bounds__(512) void k_opt_body512_kernel(AdamArgs a) { adam_chunk_body<512, true>(a, (int)blockIdx.x); }
}  // namespace smx

namespace {
// which of the slots 2 / 3 the rule `form` reads and writes (OptSlots<F> by value)
void opt_slots_used(int form, bool* um, bool* uv) {
  switch (form) {
#define SMX_SLOTS_CASE(F) case F: *um = OptSlots<F>::m; *uv = OptSlots<F>::v; break
    SMX_SLOTS_CASE(OPT_SGD); SMX_SLOTS_CASE(OPT_SGD_MOM); SMX_SLOTS_CASE(OPT_SGD_NESTEROV); SMX_SLOTS_CASE(OPT_RMSPROP); SMX_SLOTS_CASE(OPT_RMSPROP_MOM);
    SMX_SLOTS_CASE(OPT_ADAGRAD); SMX_SLOTS_CASE(OPT_ADAMAX);
#undef SMX_SLOTS_CASE
    default: *um = OptSlots<OPT_ADAM>::m; *uv = OptSlots<OPT_ADAM>::v; break;
  }
}
}  // namespace

extern "C" {

// ip: rule, n_tensors, carrier, wgs, world, use_sq, step, t0, tied_t0, tied_t1, n_slots; fp: lr, clipnorm, grad_scale, tied_inv
int smx_k_opt_carrier(const int32_t* ip, const float* fp, const float* hp, int32_t n_hp, const int32_t* sizes, const float* params,
                      const float* grads, const float* m, const float* v, const int32_t* sq_first, const int32_t* sq_count, const float* sq_slots,
                      float* params_out, float* m_out, float* v_out, float* norms, float* lr_t, int32_t* guards_ok, int32_t* unused_ok) {
  SMX_REQUIRE(ip && fp && sizes && params && grads && m && v && params_out && m_out && v_out && guards_ok && unused_ok, "k_opt_carrier: bad arguments");
  const int rule = ip[0], n_tensors = ip[1], carrier = ip[2], wgs = ip[3], world = ip[4], use_sq = ip[5], step = ip[6], t0 = ip[7], tied_t0 = ip[8],
            tied_t1 = ip[9], n_slots = ip[10];
  static const float adam_hp[3] = {0.9f, 0.999f, 1e-7f};
  float res[4];
  SMX_CHECK(opt_resolve(rule, hp, n_hp, adam_hp, res));
  SMX_REQUIRE(n_tensors > 0 && n_tensors <= SMX_MAX_TENSORS && step >= 1 && t0 >= 0, "k_opt_carrier: bad tensor count, step or t0");
  SMX_REQUIRE(carrier >= SMX_CARRIER_LAUNCH && carrier <= SMX_CARRIER_BODY512, "k_opt_carrier: unknown carrier");
  SMX_REQUIRE(carrier != SMX_CARRIER_SWEEP || wgs > 0, "k_opt_carrier: the sweep needs wgs > 0");
  SMX_REQUIRE(carrier != SMX_CARRIER_SHARD || (wgs > 0 && world >= 1 && world <= 64 && !use_sq), "k_opt_carrier: the sharded chain needs wgs > 0, a world of 1 .. 64 and the partials' norm");
  SMX_REQUIRE(tied_t0 < n_tensors && tied_t1 < n_tensors && std::isfinite(fp[0]) && std::isfinite(fp[1]) && std::isfinite(fp[2]) && std::isfinite(fp[3]),
              "k_opt_carrier: bad tied tensors or scalars");
  SMX_REQUIRE(!use_sq || (sq_first && sq_count && n_slots >= 0 && (n_slots == 0 || sq_slots)), "k_opt_carrier: use_sq needs the slot tables");
  // the model's own layout, as k_opt_launch: every tensor padded to a multiple of 64 floats, 4096-float optimiser chunks
  std::vector<size_t> off((size_t)n_tensors), pad((size_t)n_tensors);
  std::vector<OptChunk> chunks;
  size_t total = 0;
  const int CH = 4096;
  for (int t = 0; t < n_tensors; ++t) {
    SMX_REQUIRE(sizes[t] > 0, "k_opt_carrier: empty tensor");
    if (use_sq) SMX_REQUIRE(sq_count[t] >= 0 && (sq_count[t] == 0 || (sq_first[t] >= 0 && (long)sq_first[t] + sq_count[t] <= (long)n_slots)), "k_opt_carrier: a tensor's slots lie outside sq_slots");
    off[t] = total; pad[t] = ((size_t)sizes[t] + 63) / 64 * 64;
    const int first = (int)chunks.size(), n = (int)((pad[t] + CH - 1) / CH);
    for (int i = 0; i < n; ++i) {
      OptChunk c;
      memset(&c, 0, sizeof(c));
      c.tensor = t; c.offset = (int)(off[t] + (size_t)i * CH);
      c.count = (int)((size_t)(i + 1) * CH <= pad[t] ? CH : pad[t] - (size_t)i * CH);
      c.first_chunk = first; c.n_chunks = n; c.tensor_count = (int32_t)pad[t];
      chunks.push_back(c);
    }
    total += pad[t];
  }
  const int n_chunks = (int)chunks.size();
  AdamArgs a;
  opt_scalars(rule, res, a);
  a.t0 = (uint32_t)t0;
  bool um = true, uv = true;
  opt_slots_used(a.form, &um, &uv);
  StepState st3[3];
  memset(st3, 0, sizeof(st3));
  st3[2].next = (uint32_t)(step - 1);   // optimiser steps completed so far: the rule's count is t = step - t0 (1 while step <= t0)
  const float2 sch = make_float2(0.f, fp[0]);
  DeviceScratch buf;
  KbnOut oP, oG, oM, oV, oPart, oNorm;
  std::vector<KbnOut> rank_part((size_t)(carrier == SMX_CARRIER_SHARD ? world : 0));
  OptChunk* dCh; StepState* dSt; float2* dSch; float* dSlots;
  int rc;
  if ((rc = oP.alloc(buf, total)) || (rc = oG.alloc(buf, total)) || (rc = oM.alloc(buf, total)) || (rc = oV.alloc(buf, total)) || (rc = oPart.alloc(buf, (size_t)n_chunks)) ||
      (rc = oNorm.alloc(buf, (size_t)n_tensors)) || (rc = buf.put(&dCh, chunks.data(), chunks.size())) || (rc = buf.put(&dSt, st3, (size_t)3)) ||
      (rc = buf.put(&dSch, &sch, (size_t)1)) || (rc = buf.put(&dSlots, use_sq && n_slots > 0 ? sq_slots : nullptr, (size_t)std::max(n_slots, 1))))
    return rc;
  for (auto& r : rank_part) if ((rc = r.alloc(buf, (size_t)n_chunks))) return rc;
  // a buffer the rule uses: zero padding around the caller's elements; one it does not use stays 0xFF bytes throughout
  auto fill = [&](KbnOut& o, const float* src) -> int {
    SMX_HIP(hipMemset(o.p(), 0, total * 4));
    size_t lo = 0;
    for (int t = 0; t < n_tensors; ++t) {
      SMX_HIP(hipMemcpy(o.p() + off[t], src + lo, (size_t)sizes[t] * 4, hipMemcpyHostToDevice));
      lo += (size_t)sizes[t];
    }
    return SMX_OK;
  };
  SMX_CHECK(fill(oP, params)); SMX_CHECK(fill(oG, grads));
  if (um) SMX_CHECK(fill(oM, m));
  if (uv) SMX_CHECK(fill(oV, v));
  SMX_CHECK(launch_step_begin(nullptr, dSt + 2, dSt, nullptr, nullptr, 0, 0, 0u, dSch, a.b1, a.b2, a.form, a.t0));
  a.params = oP.p(); a.grads = oG.p(); a.m = oM.p(); a.v = oV.p(); a.chunks = dCh; a.n_chunks = n_chunks; a.n_launch = n_chunks; a.gap_from = n_chunks; a.gap_len = 0;
  a.partial = oPart.p(); a.tensor_norm = oNorm.p(); a.state = dSt; a.sched = dSch;
  a.clipnorm = fp[1]; a.grad_scale = fp[2]; a.tied_t0 = tied_t0 >= 0 ? tied_t0 : -1; a.tied_t1 = tied_t1 >= 0 ? tied_t1 : -1; a.tied_inv = fp[3];
  a.use_sq = use_sq ? 1 : 0; a.sq_slots = dSlots;
  for (int t = 0; t < SMX_MAX_TENSORS; ++t) { a.sq_first[t] = use_sq && t < n_tensors ? sq_first[t] : 0; a.sq_count[t] = use_sq && t < n_tensors ? sq_count[t] : 0; }
  switch (carrier) {
    case SMX_CARRIER_LAUNCH: SMX_CHECK(launch_adam(nullptr, a)); break;
    case SMX_CARRIER_SWEEP:
      if (!use_sq) SMX_CHECK(launch_grad_sqsum_range(nullptr, a, 0, n_chunks));
      SMX_CHECK(launch_adam_sweep(nullptr, a, 0, n_chunks, wgs));
      break;
    case SMX_CARRIER_BODY512:
      if (!use_sq) SMX_CHECK(launch_grad_sqsum_range(nullptr, a, 0, n_chunks));
      hipLaunchKernelGGL(smx::k_opt_body512_kernel, dim3((unsigned)n_chunks), dim3(512), 0, nullptr, a);
      SMX_HIP(hipGetLastError());
      break;
    default: {   // the sharded chain of smx_backward.hip on one device: `world` equal slices cut at a 64-float boundary, through chunks where they fall
      const size_t slice = ((total + world - 1) / world + 63) / 64 * 64;
      auto rank_args = [&](int r) { AdamArgs x = a; x.shard_lo = (long)std::min((size_t)r * slice, total); x.shard_hi = (long)std::min(((size_t)r + 1) * slice, total); return x; };
      for (int r = 0; r < world; ++r) { AdamArgs x = rank_args(r); x.partial = rank_part[r].p(); SMX_CHECK(launch_grad_sqsum_shard(nullptr, x, 0, n_chunks)); }
      SMX_HIP(hipDeviceSynchronize());
      // the all-reduce of the partials: float32 sums in rank order, 0 + rank 0 + rank 1 + ...
      std::vector<float> sum((size_t)n_chunks, 0.f), one((size_t)n_chunks);
      for (int r = 0; r < world; ++r) {
        if ((rc = rank_part[r].download(one.data(), (size_t)n_chunks))) return rc;
        for (int c = 0; c < n_chunks; ++c) sum[c] += one[c];
      }
      if ((rc = oPart.upload(sum.data(), (size_t)n_chunks))) return rc;
      SMX_CHECK(launch_head_norms(nullptr, a, 0, n_chunks));
      for (int r = 0; r < world; ++r) { const AdamArgs x = rank_args(r); if (x.shard_hi > x.shard_lo) SMX_CHECK(launch_adam_shard(nullptr, x, 0, n_chunks, wgs)); }
    }
  }
  SMX_HIP(hipDeviceSynchronize());
  bool ok = true;
  for (const KbnOut* o : {&oP, &oG, &oM, &oV, &oPart, &oNorm}) if ((rc = o->intact(&ok))) return rc;
  for (const auto& r : rank_part) if ((rc = r.intact(&ok))) return rc;
  *guards_ok = ok ? 1 : 0;
  if ((rc = oP.download(params_out, total)) || (rc = oM.download(m_out, total)) || (rc = oV.download(v_out, total)) || (rc = oNorm.download(norms, (size_t)n_tensors))) return rc;
  bool same = true;
  for (const float* q : {um ? nullptr : m_out, uv ? nullptr : v_out})
    if (q) for (size_t i = 0; i < total; ++i) { uint32_t w; memcpy(&w, q + i, 4); if (w != 0xFFFFFFFFu) same = false; }
  *unused_ok = same ? 1 : 0;
  if (lr_t) { StepState h; SMX_HIP(hipMemcpy(&h, dSt, sizeof(h), hipMemcpyDeviceToHost)); *lr_t = h.lr_t; }
  return SMX_OK;
}

}  // extern "C"

// ---- the scVI gene head's launches by themselves (smx_scvi.hip: launch_scvi_head_train / _fwd / _bwd pick the instance by Gp) ---------------
// Host arrays in the step's own layout (raw / planes [B][ld], plane c of a row at c * plane_stride, Gp live + padded columns); every output
// between guard bands and NaN before the launch (KbnOut).  The entries check what keeps the kernels' accesses inside the buffers; alignment,
// the width limit and null outputs are the launchers' to refuse.
extern "C" {

// ip: B, G, Gp, plane_stride, ld, likelihood, x_u16, n_x, ldx, Kl, ldh, ldwl, n_lib, x_identity, ldl, stream, step, cell_base;
// fp: clip_library, grad_scale, kl_weight
int smx_k_scvi_head_train(const int32_t* ip, const float* fp, const float* raw, const void* x, const float* hl, const float* Wl, const float* bl,
                          const float* library, const int32_t* rows, const float* eps_in, uint64_t seed, float* draw, float* llk_part, float* l,
                          float* sig, float* eps, float* kl, float* latl, float* dlatl, float* dl, int32_t* guards_ok) {
  SMX_REQUIRE(ip && fp && raw && x && hl && Wl && bl && library && guards_ok, "k_scvi_head_train: bad arguments");
  const int B = ip[0], G = ip[1], Gp = ip[2], ps = ip[3], ld = ip[4], likelihood = ip[5], x_u16 = ip[6], n_x = ip[7], ldx = ip[8], Kl = ip[9],
            ldh = ip[10], ldwl = ip[11], n_lib = ip[12], x_identity = ip[13], ldl = ip[14], stream = ip[15], step = ip[16];
  SMX_REQUIRE(likelihood == SMX_LLK_NBD || likelihood == SMX_LLK_ZINBD, "k_scvi_head_train: likelihood must be nbd or zinbd");
  const int k = llk_planes(likelihood);
  SMX_REQUIRE(B > 0 && G > 0 && G <= Gp && ps >= Gp && (long)ld >= (long)(k - 1) * ps + Gp && n_x > 0 && ldx >= Gp && Kl > 0 && ldh >= Kl && ldwl >= 2 &&
              n_lib > 0 && ldl >= 2 && ldl <= 256, "k_scvi_head_train: bad shapes");
  SMX_REQUIRE(rows ? true : (n_lib >= B), "k_scvi_head_train: library needs a row per cell");
  SMX_REQUIRE((x_identity || !rows) ? n_x >= B : true, "k_scvi_head_train: x needs a row per cell");
  if (rows)
    for (int b = 0; b < B; ++b) SMX_REQUIRE(rows[b] >= 0 && rows[b] < n_lib && (x_identity || rows[b] < n_x), "k_scvi_head_train: a row id lies outside x or library");
  DeviceScratch buf;
  float *dRaw, *dHl, *dWl, *dBl, *dLib, *dEps; int32_t* dRows; uint8_t* dX;
  KbnOut oDraw, oLlk, oL, oSig, oEps, oKl, oLatl, oDlatl, oDl;
  int rc;
  if ((rc = buf.put(&dRaw, raw, (size_t)B * ld)) || (rc = buf.put(&dX, static_cast<const uint8_t*>(x), (size_t)n_x * ldx * (x_u16 ? 2 : 4))) ||
      (rc = buf.put(&dHl, hl, (size_t)B * ldh)) || (rc = buf.put(&dWl, Wl, (size_t)Kl * ldwl)) || (rc = buf.put(&dBl, bl, (size_t)2)) ||
      (rc = buf.put(&dLib, library, (size_t)n_lib * 2)) || (rc = buf.put(&dRows, rows, (size_t)B)) || (rc = buf.put(&dEps, eps_in, (size_t)B)) ||
      (rc = oDraw.alloc(buf, (size_t)B * ld)) || (rc = oLlk.alloc(buf, B)) || (rc = oL.alloc(buf, B)) || (rc = oSig.alloc(buf, B)) || (rc = oEps.alloc(buf, B)) ||
      (rc = oKl.alloc(buf, B)) || (rc = oLatl.alloc(buf, (size_t)B * ldl)) || (rc = oDlatl.alloc(buf, (size_t)B * ldl)) || (rc = oDl.alloc(buf, B)))
    return rc;
  ScviTrainArgs a;
  a.raw = dRaw; a.ld = ld; a.plane_stride = ps; a.B = B; a.G = G; a.Gp = Gp; a.likelihood = likelihood;
  a.X = reinterpret_cast<const float*>(dX); a.ldx = ldx; a.x_u16 = x_u16 ? 1 : 0; a.rows = dRows; a.x_identity = x_identity ? 1 : 0;
  a.clip_library = fp[0]; a.grad_scale = fp[1]; a.klw = KlWeight{nullptr, fp[2], 1.f, 0};
  a.hl = dHl; a.ldh = ldh; a.Kl = Kl; a.Wl = dWl; a.ldwl = ldwl; a.bl = dBl; a.library = dLib; a.cell_base = (uint32_t)ip[17];
  a.nk = probe_key(seed, stream, 0, step); a.inj_eps = dEps; a.inj_ld = 1; a.ldl = ldl;
  // (an output the caller leaves out reaches the launcher as NULL: its refusal)
  a.draw = draw ? oDraw.p() : nullptr; a.llk_part = llk_part ? oLlk.p() : nullptr; a.l = l ? oL.p() : nullptr; a.sig = sig ? oSig.p() : nullptr;
  a.eps = eps ? oEps.p() : nullptr; a.kl = kl ? oKl.p() : nullptr; a.latl = latl ? oLatl.p() : nullptr; a.dlatl = dlatl ? oDlatl.p() : nullptr;
  a.dl = dl ? oDl.p() : nullptr;
  SMX_CHECK(launch_scvi_head_train(nullptr, a));
  SMX_HIP(hipDeviceSynchronize());
  bool ok = true;
  for (const KbnOut* o : {&oDraw, &oLlk, &oL, &oSig, &oEps, &oKl, &oLatl, &oDlatl, &oDl}) if ((rc = o->intact(&ok))) return rc;
  *guards_ok = ok ? 1 : 0;
  if ((rc = oDraw.download(draw, (size_t)B * ld)) || (rc = oLlk.download(llk_part, B)) || (rc = oL.download(l, B)) || (rc = oSig.download(sig, B)) ||
      (rc = oEps.download(eps, B)) || (rc = oKl.download(kl, B)) || (rc = oLatl.download(latl, (size_t)B * ldl)) ||
      (rc = oDlatl.download(dlatl, (size_t)B * ldl)) || (rc = oDl.download(dl, B)))
    return rc;
  return SMX_OK;
}

// ip: B, G, Gp, plane_stride, ld, k; fp: clip_library.  raw [B][ld], l [B] -> planes [B][ld] (rate, theta[, gate]), rho_raw [B][Gp]
int smx_k_scvi_head_fwd(const int32_t* ip, const float* fp, const float* raw, const float* l, float* planes, float* rho_raw, int32_t* guards_ok) {
  SMX_REQUIRE(ip && fp && raw && l && planes && rho_raw && guards_ok, "k_scvi_head_fwd: bad arguments (an input or an output is NULL)");
  const int B = ip[0], G = ip[1], Gp = ip[2], ps = ip[3], ld = ip[4], k = ip[5];
  SMX_REQUIRE(B > 0 && G > 0 && G <= Gp && (k == 2 || k == 3) && ps >= Gp && (long)ld >= (long)(k - 1) * ps + Gp, "k_scvi_head_fwd: bad shapes");
  DeviceScratch buf;
  float *dRaw, *dL;
  KbnOut oPl, oRho;
  int rc;
  if ((rc = buf.put(&dRaw, raw, (size_t)B * ld)) || (rc = buf.put(&dL, l, (size_t)B)) || (rc = oPl.alloc(buf, (size_t)B * ld)) ||
      (rc = oRho.alloc(buf, (size_t)B * Gp)))
    return rc;
  ScviHeadArgs a;
  a.raw = dRaw; a.planes = oPl.p(); a.ld = ld; a.plane_stride = ps; a.B = B; a.G = G; a.Gp = Gp; a.k = k; a.l = dL; a.clip_library = fp[0];
  a.rho_raw = oRho.p();
  SMX_CHECK(launch_scvi_head_fwd(nullptr, a));
  SMX_HIP(hipDeviceSynchronize());
  bool ok = true;
  if ((rc = oPl.intact(&ok)) || (rc = oRho.intact(&ok))) return rc;
  *guards_ok = ok ? 1 : 0;
  if ((rc = oPl.download(planes, (size_t)B * ld)) || (rc = oRho.download(rho_raw, (size_t)B * Gp))) return rc;
  return SMX_OK;
}

// ip, fp as the forward entry's.  planes, dplanes [B][ld], rho_raw [B][Gp], l [B] -> draw [B][ld], dl [B]
int smx_k_scvi_head_bwd(const int32_t* ip, const float* fp, const float* planes, const float* dplanes, const float* rho_raw, const float* l,
                        float* draw, float* dl, int32_t* guards_ok) {
  SMX_REQUIRE(ip && fp && planes && dplanes && rho_raw && l && draw && dl && guards_ok, "k_scvi_head_bwd: bad arguments (an input or an output is NULL)");
  const int B = ip[0], G = ip[1], Gp = ip[2], ps = ip[3], ld = ip[4], k = ip[5];
  SMX_REQUIRE(B > 0 && G > 0 && G <= Gp && (k == 2 || k == 3) && ps >= Gp && (long)ld >= (long)(k - 1) * ps + Gp, "k_scvi_head_bwd: bad shapes");
  DeviceScratch buf;
  float *dPl, *dDp, *dRho, *dL;
  KbnOut oDraw, oDl;
  int rc;
  if ((rc = buf.put(&dPl, planes, (size_t)B * ld)) || (rc = buf.put(&dDp, dplanes, (size_t)B * ld)) || (rc = buf.put(&dRho, rho_raw, (size_t)B * Gp)) ||
      (rc = buf.put(&dL, l, (size_t)B)) || (rc = oDraw.alloc(buf, (size_t)B * ld)) || (rc = oDl.alloc(buf, B)))
    return rc;
  ScviHeadArgs a;
  a.planes = dPl; a.dplanes = dDp; a.rho_raw = dRho; a.l = dL; a.ld = ld; a.plane_stride = ps; a.B = B; a.G = G; a.Gp = Gp; a.k = k;
  a.clip_library = fp[0]; a.draw = oDraw.p(); a.dl = oDl.p();
  SMX_CHECK(launch_scvi_head_bwd(nullptr, a));
  SMX_HIP(hipDeviceSynchronize());
  bool ok = true;
  if ((rc = oDraw.intact(&ok)) || (rc = oDl.intact(&ok))) return rc;
  *guards_ok = ok ? 1 : 0;
  if ((rc = oDraw.download(draw, (size_t)B * ld)) || (rc = oDl.download(dl, B))) return rc;
  return SMX_OK;
}

// ---- the label heads' launch by itself (smx_loss.hip: launch_label_loss picks label_loss_kernel or, for 'mixtril', label_tril_kernel) ------
// ip: kind, C, B, P, Pp, ld, ldy, n_rows, observed, add, backward; fp: grad_scale.  llk [B] and draw [B][ld] go in AND out: the device copies
// start as the caller's values (the incoming accumulator; a pattern that tells "not written" from "written 0") between guard bands.
int smx_k_label_loss(const int32_t* ip, const float* fp, const float* raw, const float* Y, const int32_t* rows, const uint8_t* mask, float* llk,
                     float* draw, int32_t* guards_ok) {
  SMX_REQUIRE(ip && fp && raw && Y && llk && draw && guards_ok, "k_label_loss: bad arguments (an input or an output is NULL)");
  const int kind = ip[0], C = ip[1], B = ip[2], P = ip[3], Pp = ip[4], ld = ip[5], ldy = ip[6], n_rows = ip[7];
  SMX_REQUIRE(kind >= SMX_LABEL_NB && kind <= SMX_LABEL_NORMAL, "unknown label likelihood");
  SMX_REQUIRE(P > 0, "label_dim must be > 0");
  const bool tril = kind == SMX_LABEL_MIXTRIL, mix = kind == SMX_LABEL_MIXNB || kind == SMX_LABEL_MIXGAUSS || kind == SMX_LABEL_MIXZINB;
  if (tril) SMX_REQUIRE(P <= 64 && C >= 2 && C <= 4, "label_loss: 'mixtril' heads take 1..64 label dimensions and 2..4 components");
  if (mix) SMX_REQUIRE(C >= 1 && C <= 4, "k_label_loss: mixture label heads have 1..4 components");
  SMX_REQUIRE(P <= (1 << 20) && Pp == round_up(P, 32), "k_label_loss: Pp is the label dimension rounded up to 32");
  const long planes = tril ? (long)C * (2 + P) : kind == SMX_LABEL_MIXZINB ? 4L * C : mix ? 3L * C :
                      (kind == SMX_LABEL_NB || kind == SMX_LABEL_NBD || kind == SMX_LABEL_NORMAL) ? 2 : (kind == SMX_LABEL_ZINB || kind == SMX_LABEL_ZINBD) ? 3 : 1;
  SMX_REQUIRE((long)ld >= planes * Pp, "k_label_loss: ld is below planes x Pp");
  SMX_REQUIRE(B > 0 && ldy >= P && n_rows > 0 && (rows || n_rows >= B), "k_label_loss: bad shapes");
  if (rows) for (int b = 0; b < B; ++b) SMX_REQUIRE(rows[b] >= 0 && rows[b] < n_rows, "k_label_loss: a row index lies outside Y");
  DeviceScratch buf;
  float *dRaw, *dY; int32_t* dRows; uint8_t* dMask;
  KbnOut oLlk, oDraw;
  int rc;
  if ((rc = buf.put(&dRaw, raw, (size_t)B * ld)) || (rc = buf.put(&dY, Y, (size_t)n_rows * ldy)) || (rc = buf.put(&dRows, rows, (size_t)B)) ||
      (rc = buf.put(&dMask, mask, (size_t)n_rows)) || (rc = oLlk.alloc(buf, (size_t)B)) || (rc = oDraw.alloc(buf, (size_t)B * ld)) ||
      (rc = oLlk.upload(llk, (size_t)B)) || (rc = oDraw.upload(draw, (size_t)B * ld)))
    return rc;
  LabelArgs a;
  a.kind = kind; a.C = C; a.raw = dRaw; a.ld = ld; a.Y = dY; a.ldy = ldy; a.rows = dRows; a.mask = dMask; a.observed = ip[8];
  a.B = B; a.P = P; a.Pp = Pp; a.grad_scale = fp[0]; a.draw = oDraw.p(); a.llk = oLlk.p(); a.add = ip[9]; a.backward = ip[10];
  SMX_CHECK(launch_label_loss(nullptr, a));
  SMX_HIP(hipDeviceSynchronize());
  bool ok = true;
  if ((rc = oLlk.intact(&ok)) || (rc = oDraw.intact(&ok))) return rc;
  *guards_ok = ok ? 1 : 0;
  if ((rc = oLlk.download(llk, (size_t)B)) || (rc = oDraw.download(draw, (size_t)B * ld))) return rc;
  return SMX_OK;
}

}  // extern "C"
