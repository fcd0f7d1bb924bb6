// smx_handoff.h -- handing data from some workgroups of a launch to others of the SAME launch (gfx950: eight XCDs whose L2s are not
// coherent with each other, a vector L1 per CU that no other CU's store refreshes).  One seam = one monotonic counter + one error word.
//
//   publish   the payload is stored write-through (sc1: handoff_store / handoff_store4) -> EVERY storing wave drains its stores
//             (`s_waitcnt vmcnt(0)`) -> workgroup barrier -> ONE lane adds 1 to the seam's counter (agent scope, relaxed).  No release
//             fence: a write-through store that has been acknowledged is in memory, there is no dirty line to write back.
//   wait      ONE wave polls the counter (lane l its shard l, summed over the wave) with relaxed sc1 loads and s_sleep until it reaches
//             `target`, bounded on the device's 100 MHz wall clock.  On expiry it sets the seam's error word and every thread of the workgroup gets `false`: the caller returns
//             without storing anything.  Then
//               ACQUIRE = true:   one agent-scope acquire (invalidates this CU's L1) + `vmcnt(0)` by the polling lane, the barrier, and
//                                 the workgroup reads the payload with plain loads;
//               ACQUIRE = false:  the barrier only; EVERY load of the payload must then be an sc1 load to registers (handoff_load4 /
//                                 handoff_load: they bypass the L1), the launch must hold one workgroup per CU, the memory comes from
//                                 hipMalloc and every payload byte was stored sc1 -- the measured form "one lane of each storing workgroup
//                                 signals for all its stores / an sc1 poll / the other waves load behind a barrier the polling wave joins".
//                                 A single plain load of a handed-off line is a stale read waiting to happen: keep ACQUIRE = true wherever
//                                 one of those conditions is not the launch's own.
//
// The counter is `shards` words on 128-byte lines of their own: 128 adds on ONE word cost 3-4 us at this part's memory side, more than the
// launch boundary a hand-off replaces; over 8 words the wait ends ~1.5 us after the last producer's drain (tools/dev/fuse_probe.hip seam;
// docs/LAB_NOTES.md).  The counter is monotonic.  The first step of a library call zeroes it (a memset node ahead of the launch, with the error word, in a
// block of their own at the start of its allocation: HANDOFF_STATE_BYTES, a multiple of 16); epochs count within the call: target = producers x (steps of this call so far, this one included).  No
// memset per launch, nothing re-armed inside a launch.  The host does not take the form while a graph is being captured (the target is
// an argument: frozen under replay).
//
// Progress.  Producers never wait for anything: a producer that has been dispatched runs to its publish whatever else is resident.  Only
// consumers wait, and a launch has at most HANDOFF_MAX_WAITERS of them.  Waiting workgroups hold at most that many of the chip's
// workgroup slots (256 CUs, at least one slot each), so the dispatcher always has a free slot for the next workgroup in its queue and
// every producer is dispatched eventually -- in whatever order the workgroups are dealt, wherever the consumers sit in the grid, and
// whether or not the whole grid is resident at once.  The bound on the wall clock is for a device that is going down, not for scheduling.
#pragma once
#include <hip/hip_runtime.h>

namespace smx {

constexpr int HANDOFF_MAX_WAITERS = 16;
constexpr int HANDOFF_SHARD_STRIDE = 32;   // unsigned words between two shards of a counter: a 128-byte line each
constexpr int HANDOFF_MAX_SHARDS = 8;
constexpr size_t HANDOFF_STATE_BYTES = (size_t)HANDOFF_MAX_SHARDS * HANDOFF_SHARD_STRIDE * 4 + 16;   // [shards | error word, padded]: the block the call's first step zeroes

struct HandoffSeam {
  unsigned* counter = nullptr;     // hipMalloc memory, the start of a HANDOFF_STATE_BYTES block zeroed once per library call
  unsigned* error = nullptr;       // non-zero after a wait that gave up; sticky until the host clears it
  unsigned target = 0;             // what the consumers wait for: producers x epochs of this call
  int shards = 1;                  // 1, 2, 4 or 8: producing workgroup b adds to shard b % shards (a line of its own), the waiting wave sums them
  long long timeout_ticks = 0;     // bound of a wait on the 100 MHz wall clock
};

typedef float handoff_f4 __attribute__((ext_vector_type(4)));
typedef unsigned handoff_u4 __attribute__((ext_vector_type(4)));

// a buffer descriptor over [p, p + bytes): the sc1 forms of the 16-byte accesses go through raw buffer instructions, whose cache bits
// the compiler takes as an argument (aux 16 = sc1) and whose completion it counts like any other vector-memory access
__device__ inline __amdgpu_buffer_rsrc_t handoff_rsrc(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(bytes > 0x7FFFFFFFL ? 0x7FFFFFFFL : bytes), 0x00020000);
}
__device__ inline void handoff_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // global_store_dword sc1
__device__ inline void handoff_store4(__amdgpu_buffer_rsrc_t rs, unsigned byte_off, handoff_f4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(handoff_u4, v), rs, (int)byte_off, 0, 16);
}
__device__ inline float handoff_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // global_load_dword sc1
__device__ inline handoff_f4 handoff_load4(__amdgpu_buffer_rsrc_t rs, unsigned byte_off) {
  return __builtin_bit_cast(handoff_f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, 16));
}

// every thread of the producing workgroup, behind its last payload store (one barrier inside)
__device__ inline void handoff_publish(const HandoffSeam& s, int producer) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave: its write-through stores are acknowledged (inline asm: the compiler must not drop it)
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(s.counter + (producer & (s.shards - 1)) * HANDOFF_SHARD_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every thread of the consuming workgroup (barriers inside); `ok_lds`: one int of LDS.  false: the wait gave up, return without storing.
// Wave 0 polls: lane l < shards reads shard l, the wave sums them (every iteration wave-uniform).
template <bool ACQUIRE>
__device__ inline bool handoff_wait(const HandoffSeam& s, int* ok_lds) {
  if (threadIdx.x < 64) {
    int ok = 1;
    const int l = (int)threadIdx.x;
    const long long t0 = wall_clock64();   // 100 MHz on gfx9
    for (;;) {
      unsigned got = l < s.shards ? __hip_atomic_load(s.counter + l * HANDOFF_SHARD_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
      for (int o = 1; o < HANDOFF_MAX_SHARDS; o <<= 1) got += __shfl_xor(got, o, 64);   // (lanes 0 .. 7 hold every shard)
      got = __builtin_amdgcn_readfirstlane(got);
      if ((int)(got - s.target) >= 0) break;
      __builtin_amdgcn_s_sleep(2);
      if (wall_clock64() - t0 > s.timeout_ticks) {
        if (l == 0) __hip_atomic_store(s.error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    if (ACQUIRE && ok) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the invalidate has completed before this wave reaches the barrier
    } else {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (no instruction: the payload's loads stay below the poll)
    }
    if (l == 0) *ok_lds = ok;
  }
  __syncthreads();
  const bool ok = *ok_lds != 0;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return ok;
}

}  // namespace smx
