// fuse_probe.hip -- what a launch boundary between two dependent small kernels costs on MI355X, against the same two phases in ONE launch
// whose second phase's workgroups wait for a counter the first phase's workgroups raise (blocks are dispatched in index order: the waiting
// blocks start only after every producer block has started, so the wait cannot starve the producers).
//   hipcc --offload-arch=gfx950 -O2 tools/dev/fuse_probe.hip -o /tmp/fuse_probe && /tmp/fuse_probe
// `fuse_probe seam`: only the second part -- the publish / wait pair of sisua_amd/csrc/smx_handoff.h at the geometry of the training step's
// seam between the decoder's and the encoder's BatchNorm-backward launches (seam_probe below).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <vector>
#include "../../sisua_amd/csrc/smx_handoff.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__device__ inline void phase_a(float* buf, int n, int bid, int nb, float s) {   // writes n floats
  for (int i = bid * 256 + threadIdx.x; i < n; i += nb * 256) buf[i] = s + (float)i;
}
__device__ inline void phase_b(const float* buf, float* out, int n, int bid, int nb) {   // reads them all, one number per block
  float t = 0.f;
  for (int i = bid * 256 + threadIdx.x; i < n; i += nb * 256) t += buf[i];
  for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out + bid, t);
}
__global__ __launch_bounds__(256) void ka(float* buf, int n, float s) { phase_a(buf, n, blockIdx.x, gridDim.x, s); }
__global__ __launch_bounds__(256) void kb(const float* buf, float* out, int n) { phase_b(buf, out, n, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256) void kab(float* buf, float* out, int n, float s, int na, unsigned* ctr) {
  const int bid = blockIdx.x;
  if (bid < na) {
    phase_a(buf, n, bid, na, s);
    __threadfence();   // this block's writes are visible device-wide before its count
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    const int nb = gridDim.x - na;
    if (threadIdx.x == 0) {
      while (__hip_atomic_load(ctr, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)na) __builtin_amdgcn_s_sleep(2);
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    phase_b(buf, out, n, bid - na, nb);
    __syncthreads();
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nb - 1) {   // the last consumer re-arms both
      __hip_atomic_store(ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ctr, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ... the same with the exchanged data moved by device-scope accesses (write-through stores, loads that do not trust the XCD's L2) and
// no release / acquire fence: what a fence costs on a part with eight non-coherent L2s is the write-back / invalidate of a whole L2
__global__ __launch_bounds__(256) void kab_wt(float* buf, float* out, int n, float s, int na, unsigned* ctr) {
  const int bid = blockIdx.x;
  if (bid < na) {
    for (int i = bid * 256 + threadIdx.x; i < n; i += na * 256) __hip_atomic_store(buf + i, s + (float)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);   // (vmcnt(0): the stores have been acknowledged)
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    const int nb = gridDim.x - na;
    if (threadIdx.x == 0) {
      while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)na) __builtin_amdgcn_s_sleep(2);
    }
    __syncthreads();
    float t = 0.f;
    for (int i = (bid - na) * 256 + threadIdx.x; i < n; i += nb * 256) t += __hip_atomic_load(buf + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out + (bid - na), t);
    __syncthreads();
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nb - 1) {
      __hip_atomic_store(ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- the seam's own geometry (round 7) ------------------------------------------------------------------------------------------------
// What the round-6 numbers above rest on -- 1 MB through 4-byte agent-scope accesses, 256 adds and a re-arm on one counter, a whole-L2
// write-back per producer, a consumer with nothing to do before its wait, a producer launch with no rider tail -- does not hold between
// the decoder's and the encoder's BatchNorm-backward launches of the training step.  There:
//   N_PROD = 128 producer workgroups (512 threads), each with ~3 us of work of its own, then ONE column of a [128][128] f32 matrix:
//            row-major (thread r stores 4 bytes, 512 bytes apart: what wgrad_group_kernel reads behind the launch) or, `col16`, a
//            column-major copy (one 512-byte run as 16-byte stores);
//   N_CONS = 16 consumer workgroups, ~2 us of work that does not depend on the matrix (64 KB of loads, then the clock), then all 64 KB
//            of it as eight 16-byte loads per thread, every word checked against the value its epoch should have left;
//   n_by   = 0 or 300 bandwidth-bound bystanders (64 KB in, 16 KB out each), as the launches' riders are.
// Forms:  two launches (producers + half the bystanders | consumers + the other half; plain stores and loads);
//         one launch, smx_handoff.h with the acquire (sc1 stores, plain loads);
//         one launch, smx_handoff.h without it (sc1 stores, sc1 loads) -- valid at one workgroup per CU only: the `lds 84K` rows;
//         both with the seam's counter as ONE word and as 8 shards on lines of their own; the consumers behind / ahead of the producers.
// Behind every row: where the last repetition's time went (the device's 100 MHz wall clock, us from the first workgroup's entry).
// Every form is verified first, launch by launch with the consumers L1-WARM (they plain-load every line of the matrix before they
// wait), the seam's error word read after each; only then timed as 2000 dependent repetitions.  The counter is zeroed once per series
// and never re-armed: target = 128 x repetition.
constexpr int N_PROD = 128, N_CONS = 16, SEAM_T = 512;
struct SeamP {
  float* D; float* Dc; const float* W; const smx::handoff_f4* by_src; smx::handoff_f4* by_dst; unsigned* bad; float* sink;
  smx::HandoffSeam seam;
  long long* stamps;   // null, or [0, 128): producers {entry, stores drained}, [128, 144): consumers {entry, wait begins, wait over, words checked}; 4 per workgroup
  int epoch, n_prod, n_cons, n_by, by_first, cons_first, form, col16, preread, prod_ticks, cons_ticks;
};
__device__ inline float seam_val(int epoch, int r, int c) { return (float)((epoch * 7 + r * 3 + c * 5) % 251); }
__device__ inline void busy_until(long long t0, int ticks) { while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(1); }   // (bounded by the clock itself)
__global__ __launch_bounds__(SEAM_T) void seam_kernel(SeamP p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ int ok_s;
  const int tid = (int)threadIdx.x;
  int b = (int)blockIdx.x, role;   // 0 producer, 1 consumer, 2 bystander
  if (p.cons_first) { if (b < p.n_cons) role = 1; else if ((b -= p.n_cons) < p.n_prod) role = 0; else { b -= p.n_prod; role = 2; } }
  else { if (b < p.n_prod) role = 0; else if ((b -= p.n_prod) < p.n_cons) role = 1; else { b -= p.n_cons; role = 2; } }
  const long long t0 = wall_clock64();
  if (role == 2) {
    if (b >= p.n_by) return;
    const int bb = p.by_first + b;   // (< 300: 300 x 4096 + 4096 float4 of the 4 M in by_src, 301 x 1024 of the 1 M in by_dst)
    smx::handoff_f4 v[8], acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p.by_src[(long)bb * 4096 + u * SEAM_T + tid];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
    p.by_dst[(long)bb * 1024 + tid] = acc;
    p.by_dst[(long)bb * 1024 + SEAM_T + tid] = acc + v[0];
    return;
  }
  if (role == 0) {
    const int col = b;   // < N_PROD = 128 columns
    busy_until(t0, p.prod_ticks);
    if (p.col16) {
      if (tid < 32) {
        const smx::handoff_f4 v = {seam_val(p.epoch, 4 * tid, col), seam_val(p.epoch, 4 * tid + 1, col), seam_val(p.epoch, 4 * tid + 2, col), seam_val(p.epoch, 4 * tid + 3, col)};
        if (p.form == 0) reinterpret_cast<smx::handoff_f4*>(p.Dc)[col * 32 + tid] = v;
        else smx::handoff_store4(smx::handoff_rsrc(p.Dc, 128 * 128 * 4), (unsigned)(col * 32 + tid) * 16u, v);
      }
    } else if (tid < 128) {
      if (p.form == 0) p.D[tid * 128 + col] = seam_val(p.epoch, tid, col);
      else smx::handoff_store(p.D + tid * 128 + col, seam_val(p.epoch, tid, col));
    }
    if (p.stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); if (tid == 0) { p.stamps[4 * col] = t0; p.stamps[4 * col + 1] = wall_clock64(); } }
    if (p.form != 0) smx::handoff_publish(p.seam, col);
    return;
  }
  // consumer b of n_cons: the independent part first
  const float* M = p.col16 ? p.Dc : p.D;
  float s = 0.f;
  {
    smx::handoff_f4 w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u] = reinterpret_cast<const smx::handoff_f4*>(p.W)[u * SEAM_T + tid];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += w[u].x + w[u].w;
    dyn[tid] = s;
  }
  if (p.preread) {   // every line of the matrix into this CU's L1 before the wait: what a stale read needs
    smx::handoff_f4 w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u] = reinterpret_cast<const smx::handoff_f4*>(M)[u * SEAM_T + tid];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += w[u].y * 1e-30f;
  }
  busy_until(t0, p.cons_ticks);
  const long long t1 = wall_clock64();
  if (p.form == 1) { if (!smx::handoff_wait<true>(p.seam, &ok_s)) return; }
  else if (p.form == 2) { if (!smx::handoff_wait<false>(p.seam, &ok_s)) return; }
  const long long t2 = wall_clock64();
  smx::handoff_f4 v[8];
  if (p.form == 2) {
    const __amdgpu_buffer_rsrc_t rs = smx::handoff_rsrc(M, 128 * 128 * 4);
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = smx::handoff_load4(rs, (unsigned)(u * SEAM_T + tid) * 16u);
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = reinterpret_cast<const smx::handoff_f4*>(M)[u * SEAM_T + tid];
  }
  int wrong = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = 4 * (u * SEAM_T + tid) + j, hi = e >> 7, lo = e & 127;
      const float want = p.col16 ? seam_val(p.epoch, lo, hi) : seam_val(p.epoch, hi, lo);
      wrong += (v[u][j] != want) ? 1 : 0;
      s += v[u][j];
    }
  if (wrong) atomicAdd(p.bad, (unsigned)wrong);
  if (tid == 0) p.sink[b] = s + dyn[1];
  if (p.stamps && tid == 0) { long long* q = p.stamps + 4 * (N_PROD + b); q[0] = t0; q[1] = t1; q[2] = t2; q[3] = s == 12345.f ? 0 : wall_clock64(); }
}

static int seam_probe() {
  const int reps = 2000;
  float *D, *Dc, *W, *sink; smx::handoff_f4 *by_src, *by_dst; unsigned *ctr, *bad;
  CHECK(hipMalloc(&D, 128 * 128 * 4)); CHECK(hipMalloc(&Dc, 128 * 128 * 4)); CHECK(hipMalloc(&W, 64 << 10)); CHECK(hipMalloc(&sink, 4096));
  CHECK(hipMalloc(&by_src, 64 << 20)); CHECK(hipMalloc(&by_dst, 16 << 20)); CHECK(hipMalloc(&ctr, smx::HANDOFF_STATE_BYTES)); CHECK(hipMalloc(&bad, 16));
  long long* stamps; CHECK(hipMalloc(&stamps, 4 * (N_PROD + N_CONS) * 8));
  CHECK(hipMemset(D, 0, 128 * 128 * 4)); CHECK(hipMemset(Dc, 0, 128 * 128 * 4)); CHECK(hipMemset(W, 0, 64 << 10)); CHECK(hipMemset(by_src, 0, 64 << 20));
  CHECK(hipMemset(bad, 0, 16));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&seam_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
  hipStream_t st; CHECK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  SeamP base;
  memset(&base, 0, sizeof(base));
  base.D = D; base.Dc = Dc; base.W = W; base.by_src = by_src; base.by_dst = by_dst; base.bad = bad; base.sink = sink;
  base.seam.counter = ctr; base.seam.error = ctr + smx::HANDOFF_MAX_SHARDS * smx::HANDOFF_SHARD_STRIDE; base.seam.timeout_ticks = 2000000;   // 20 ms
  base.prod_ticks = 300; base.cons_ticks = 200;
  // one repetition of a form; rep counts from 1 within a series
  auto launch = [&](const SeamP& c, int rep, size_t lds) {
    SeamP p = c;
    p.epoch = rep;
    if (c.form == 0) {
      SeamP a = p, b2 = p;
      a.n_cons = 0; a.n_by = c.n_by / 2; a.by_first = 0;
      b2.n_prod = 0; b2.n_by = c.n_by - c.n_by / 2; b2.by_first = c.n_by / 2;
      hipLaunchKernelGGL(seam_kernel, dim3(a.n_prod + a.n_by), dim3(SEAM_T), lds, st, a);
      hipLaunchKernelGGL(seam_kernel, dim3(b2.n_cons + b2.n_by), dim3(SEAM_T), lds, st, b2);
    } else {
      p.seam.target = (unsigned)(c.n_prod * rep);
      hipLaunchKernelGGL(seam_kernel, dim3(p.n_prod + p.n_cons + p.n_by), dim3(SEAM_T), lds, st, p);
    }
  };
  auto state = [&](unsigned* err, unsigned* wrong) -> int {
    unsigned h[4];
    CHECK(hipStreamSynchronize(st));
    CHECK(hipMemcpy(h, base.seam.error, 16, hipMemcpyDeviceToHost)); *err = h[0];
    CHECK(hipMemcpy(h, bad, 16, hipMemcpyDeviceToHost)); *wrong = h[0];
    return 0;
  };
  const char* form_name[3] = {"two launches            ", "one launch, acquire     ", "one launch, sc1 loads   "};
  printf("seam probe: %d producers x 512 B, %d consumers x 64 KB; us per repetition (wrong words: verification + timed run)\n", N_PROD, N_CONS);
  for (int lds_big = 0; lds_big < 2; ++lds_big)
    for (int n_by = 0; n_by <= 300; n_by += 300)
      for (int col16 = 0; col16 < 2; ++col16)
        for (int form = 0; form < 3; ++form)
          for (int cons_first = 0; cons_first < (form ? 2 : 1); ++cons_first)
          for (int shards = 1; shards <= (form ? 8 : 1); shards *= 8) {
            const size_t lds = lds_big ? 84 * 1024 : 4096;
            SeamP c = base;
            c.seam.shards = shards;
            c.n_prod = N_PROD; c.n_cons = N_CONS; c.n_by = n_by; c.form = form; c.col16 = col16; c.cons_first = cons_first;
            unsigned err = 0, wrong = 0;
            CHECK(hipMemsetAsync(ctr, 0, smx::HANDOFF_STATE_BYTES, st)); CHECK(hipMemsetAsync(bad, 0, 16, st));
            c.preread = 1;
            for (int rep = 1; rep <= 4; ++rep) {   // launch by launch: a wait that gives up ends the probe here
              launch(c, rep, lds);
              CHECK(hipGetLastError());
              if (state(&err, &wrong)) return 1;
              if (err) { printf("%s lds %s by %3d col16 %d cons_first %d: the wait gave up in verification launch %d -- stopping\n", form_name[form], lds_big ? "84K" : " 4K", n_by, col16, cons_first, rep); return 1; }
            }
            const unsigned wrong_v = wrong;
            c.preread = 0;
            float ms = 0.f;
            for (int warm = 0; warm < 2; ++warm) {
              CHECK(hipMemsetAsync(ctr, 0, smx::HANDOFF_STATE_BYTES, st));
              CHECK(hipEventRecord(e0, st));
              for (int rep = 1; rep <= reps; ++rep) launch(c, rep, lds);
              CHECK(hipEventRecord(e1, st)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms, e0, e1));
              if (state(&err, &wrong)) return 1;
              if (err) { printf("%s lds %s by %3d col16 %d cons_first %d: a wait gave up in the timed run -- stopping\n", form_name[form], lds_big ? "84K" : " 4K", n_by, col16, cons_first); return 1; }
            }
            // where the time goes inside the last of 20 more repetitions (10 ns ticks of the device's wall clock, from the first workgroup's entry)
            c.stamps = stamps;
            CHECK(hipMemsetAsync(ctr, 0, smx::HANDOFF_STATE_BYTES, st));
            for (int rep = 1; rep <= 20; ++rep) launch(c, rep, lds);
            if (state(&err, &wrong)) return 1;
            if (err) { printf("a wait gave up in the stamped run -- stopping\n"); return 1; }
            std::vector<long long> hs(4 * (N_PROD + N_CONS));
            CHECK(hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost));
            long long first = hs[0], p_last = 0; double c_in = 0, c_w0 = 0, c_w1 = 0, c_done = 0;
            for (int i = 0; i < N_PROD; ++i) { first = std::min(first, hs[4 * i]); p_last = std::max(p_last, hs[4 * i + 1]); }
            const long long* q = hs.data() + 4 * N_PROD;
            for (int i = 0; i < N_CONS; ++i) { c_in += q[4 * i] / 16.0; c_w0 += q[4 * i + 1] / 16.0; c_w1 += q[4 * i + 2] / 16.0; c_done += q[4 * i + 3] / 16.0; }
            printf("%s lds %s  bystanders %3d  %s  consumers %s shards %d:  %6.2f us   (wrong %u + %u)   last producer drained %5.2f | consumers: entry %5.2f  wait begins %5.2f  over %5.2f  checked %5.2f\n",
                   form_name[form], lds_big ? "84K" : " 4K", n_by, col16 ? "col-major 16 B" : "row-major  4 B",
                   form ? (cons_first ? "first " : "behind") : "  --  ", shards, 1000.0 * ms / reps, wrong_v, wrong - wrong_v, (p_last - first) * 0.01,
                   (c_in - first) * 0.01, (c_w0 - first) * 0.01, (c_w1 - first) * 0.01, (c_done - first) * 0.01);
            fflush(stdout);
          }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "seam")) return seam_probe();
  const int reps = 2000;
  float *buf, *out; unsigned* ctr;
  CHECK(hipMalloc(&buf, 64 << 20)); CHECK(hipMalloc(&out, 4096 * 4)); CHECK(hipMalloc(&ctr, 64)); CHECK(hipMemset(ctr, 0, 64)); CHECK(hipMemset(out, 0, 4096 * 4));
  hipStream_t st; CHECK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  const int cases[][3] = {{256, 64, 64 << 10}, {256, 64, 256 << 10}, {256, 64, 2 << 20}, {608, 73, 256 << 10}, {64, 128, 256 << 10}, {1024, 256, 8 << 20}};
  for (auto& c : cases) {
    const int na = c[0], nb = c[1], n = c[2];
    float ms2 = 0.f, ms1 = 0.f, ms0 = 0.f;
    for (int warm = 0; warm < 2; ++warm) {
      CHECK(hipEventRecord(e0, st));
      for (int r = 0; r < reps; ++r) { hipLaunchKernelGGL(ka, dim3(na), dim3(256), 0, st, buf, n, (float)r); hipLaunchKernelGGL(kb, dim3(nb), dim3(256), 0, st, buf, out, n); }
      CHECK(hipEventRecord(e1, st)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms2, e0, e1));
      CHECK(hipEventRecord(e0, st));
      for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(kab, dim3(na + nb), dim3(256), 0, st, buf, out, n, (float)r, na, ctr);
      CHECK(hipEventRecord(e1, st)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms1, e0, e1));
      CHECK(hipEventRecord(e0, st));
      for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(kab_wt, dim3(na + nb), dim3(256), 0, st, buf, out, n, (float)r, na, ctr);
      CHECK(hipEventRecord(e1, st)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms0, e0, e1));
    }
    // correctness of the fused form: out[b] accumulated the same sums twice per repetition in both forms -> compare one fresh pass of each
    std::vector<float> h2(nb), h1(nb);
    CHECK(hipMemset(out, 0, 4096 * 4));
    hipLaunchKernelGGL(ka, dim3(na), dim3(256), 0, st, buf, n, 3.f); hipLaunchKernelGGL(kb, dim3(nb), dim3(256), 0, st, buf, out, n);
    CHECK(hipStreamSynchronize(st)); CHECK(hipMemcpy(h2.data(), out, nb * 4, hipMemcpyDeviceToHost));
    int bad = 0, bad0 = 0;
    for (int t = 0; t < 200; ++t) {
      CHECK(hipMemsetAsync(out, 0, 4096 * 4, st));
      hipLaunchKernelGGL(kab, dim3(na + nb), dim3(256), 0, st, buf, out, n, 3.f, na, ctr);
      CHECK(hipStreamSynchronize(st)); CHECK(hipMemcpy(h1.data(), out, nb * 4, hipMemcpyDeviceToHost));
      for (int b = 0; b < nb; ++b) bad += (fabsf(h1[b] - h2[b]) > 1e-3f * fabsf(h2[b])) ? 1 : 0;
      CHECK(hipMemsetAsync(out, 0, 4096 * 4, st));
      hipLaunchKernelGGL(kab_wt, dim3(na + nb), dim3(256), 0, st, buf, out, n, 3.f, na, ctr);
      CHECK(hipStreamSynchronize(st)); CHECK(hipMemcpy(h1.data(), out, nb * 4, hipMemcpyDeviceToHost));
      for (int b = 0; b < nb; ++b) bad0 += (fabsf(h1[b] - h2[b]) > 1e-3f * fabsf(h2[b])) ? 1 : 0;
    }
    printf("producers %4d  consumers %3d  %7.2f KB:  two launches %.2f us per pair,  one launch with a counter and fences %.2f us (wrong: %d),  with device-scope accesses and no fence %.2f us (wrong: %d)\n", na, nb, n * 4 / 1024.0,
           1000.0 * ms2 / reps, 1000.0 * ms1 / reps, bad, 1000.0 * ms0 / reps, bad0);
  }
  return seam_probe();
}
