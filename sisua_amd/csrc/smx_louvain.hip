// smx_louvain.hip -- Louvain communities of a symmetric graph (the reference's SingleCellOMIC.louvain, a proxy to scanpy.tl.louvain:
// _single_cell_analysis.py:732-835), as a deterministic colour-synchronous method (tests/louvain_ref.py is its NumPy
// restatement).  Model-free entries: they upload, compute, download and free their own buffers.
//   weights     quantised once on the host, q = llrint(w / wmax * 2^30) (unit weights: 1), entries of q == 0 dropped.  Every degree, total
//               and internal weight is an int64 sum of such q -- exact and independent of the order of summation, so integer atomics and
//               hash tables are allowed and no result depends on the launch geometry, on the order of a row's columns or on the call.
//   colouring   Jones-Plassmann rounds on the priority (mix32(v), -v): a vertex whose every neighbour of higher priority is coloured takes
//               the lowest colour none of them has -- the greedy colouring in decreasing priority, whatever the rounds' interleaving.
//   move        THE HOT PATH.  The vertices of one colour decide from the state at the start of the colour's turn (no two are adjacent).
//               A row of up to SMX_LV_TABLE_DEGREE entries: one wave, the neighbours' communities hashed into the wave's own LDS table
//               (64 .. 256 slots, at most half full) with integer LDS atomics, then one slot per lane: gain(D) = kin_D - (gamma k_v
//               tot_D) / m2 in float64 from the integers, each operation rounded once (contraction is off in this file), the best by
//               (gain, lowest id).  A longer row (a hub; the rows of the coarse levels): one workgroup, the row's entries sorted by
//               community with smx_block.h's radix sort, the tie-run pass adds each run's weights at its head, a gain per head.
//   apply       the colour's moves, then tot by int64 global atomics.
//   Q           in_c by int64 atomics, the terms in_c / m2 - gamma (tot_c / m2)^2 per community id, summed in smx_block.h's halving order.
//   relabel     the communities numbered in order of their lowest member (atomicMin, a flag scan).
//   aggregate   per coarse row a hash table in global memory (its size from the row's entry count), count, scan, fill.
//   order       the final ids by decreasing size, ties to the lowest member: one radix sort of the communities.
// The host reads back a few scalars per colouring round pair, per sweep (the moved count and Q) and per level; no vector crosses inside
// the loop.  Every loop is bounded by a row's length, a table's size or n.
#include "smx_model.h"
#include "smx_block.h"   // the radix sort, the tie-run pass and the fixed-order sums

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)   // a gain and a modularity term are the written operations, each rounded once

namespace smx {

#define SMX_LV_MAX_N (1l << 24)            // community ids are sort keys of 24 bits
#define SMX_LV_MAX_NNZ 2147483647ll        // 2^31 - 1 entries of at most 2^30: every total stays below 2^61
#define SMX_LV_TABLE_DEGREE 128            // rows of up to this many entries take the wave's LDS table
#define SMX_LV_TABLE_SLOTS 256             // ... which is at most half full
#define SMX_LV_QUANT 1073741824.0          // 2^30
#define SMX_LV_GRID_CAP 2048               // workgroups of a grid-stride launch
#define SMX_LV_SELF_KEY 0x1000000u         // a self loop's sort key: behind every community id
#define SMX_LV_HASH 2654435761u

typedef long long ll;
typedef unsigned long long ull;

struct LvGraph { const ll* ip; const int32_t* col; const ll* val; int n; int tdeg; };   // tdeg: the longest row of the wave form

__device__ inline int lv_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline ll lv_load(const ll* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void lv_add(ll* p, ll v) { atomicAdd(reinterpret_cast<ull*>(p), (ull)v); }

__device__ inline uint32_t lv_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
__device__ inline ull lv_priority(int v) { return ((ull)lv_mix32((uint32_t)v) << 32) | (ull)(0xFFFFFFFFu - (uint32_t)v); }

__device__ inline ll lv_wave_scan(ll v) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const ll t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// ---- exclusive scan of in [n] into out [n + 1] (out[n]: the total); in may be out -------------------------------------------------------
__global__ __launch_bounds__(256) void lv_scan_block_kernel(const ll* in, ll* out, long n, ll* bsum) {
  __shared__ ll wt[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long i0 = ((long)blockIdx.x * 256 + tid) * 4;
  ll x[4], s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { x[q] = i0 + q < n ? in[i0 + q] : 0; s += x[q]; }
  const ll inc = lv_wave_scan(s);
  if (lane == 63) wt[w] = inc;
  __syncthreads();
  ll pre = inc - s;
  for (int q = 0; q < w; ++q) pre += wt[q];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (i0 + q < n) out[i0 + q] = pre;
    pre += x[q];
  }
  if (tid == 255) bsum[blockIdx.x] = pre;
}

__global__ __launch_bounds__(256) void lv_scan_top_kernel(ll* bsum, long nb, ll* total) {
  __shared__ ll wt[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  ll carry = 0;
  for (long t0 = 0; t0 < nb; t0 += 256) {
    const long i = t0 + tid;
    const ll v = i < nb ? bsum[i] : 0;
    const ll inc = lv_wave_scan(v);
    if (lane == 63) wt[w] = inc;
    __syncthreads();
    ll pre = carry + inc - v;
    for (int q = 0; q < w; ++q) pre += wt[q];
    if (i < nb) bsum[i] = pre;
    carry += (wt[0] + wt[1]) + (wt[2] + wt[3]);
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(256) void lv_scan_add_kernel(ll* out, long n, const ll* bsum) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] += bsum[i >> 10];
}

// ---- a level's start: k_v, every vertex its own community, the long rows counted ------------------------------------------------------
__global__ __launch_bounds__(256) void lv_degree_kernel(LvGraph g, ll* k, ll* tot, int* comm, int* n_big) {
  const int lane = threadIdx.x & 63;
  const long nw = (long)gridDim.x * 4;
  for (long v = (long)blockIdx.x * 4 + (threadIdx.x >> 6); v < g.n; v += nw) {
    const ll s = g.ip[v], e = g.ip[v + 1];
    ll sum = 0;
    for (ll i = s + lane; i < e; i += 64) sum += g.val[i];
    sum = halving_wave_sum(sum);
    if (lane == 0) {
      k[v] = sum;
      if (tot) tot[v] = sum;
      if (comm) comm[v] = (int)v;
      if (n_big && e - s > g.tdeg) atomicAdd(n_big, 1);
    }
  }
}

__global__ __launch_bounds__(256) void lv_iota_kernel(int* x, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = (int)i;
}

// ---- colouring: one Jones-Plassmann round; stat[0]: the vertices still waiting (when count), stat[1]: the highest colour ----------------
__global__ __launch_bounds__(256) void lv_colour_kernel(LvGraph g, int* colour, int* stat, int count) {
  const int lane = threadIdx.x & 63;
  const long nw = (long)gridDim.x * 4;
  for (long vl = (long)blockIdx.x * 4 + (threadIdx.x >> 6); vl < g.n; vl += nw) {
    const int v = (int)vl;
    if (lv_load(colour + v) >= 0) continue;   // (wave-uniform)
    const ull pv = lv_priority(v);
    const ll s = g.ip[v], e = g.ip[v + 1];
    bool ready = true;
    for (ll i = s + lane; i < e; i += 64) {
      const int u = g.col[i];
      if (u != v && lv_priority(u) > pv && lv_load(colour + u) < 0) ready = false;
    }
    if (!__all(ready)) {
      if (count && lane == 0) atomicAdd(stat, 1);
      continue;
    }
    int base = 0, c = -1;
    while (c < 0) {   // (the colours in use are at most the row's length: base stays below it + 64)
      ull m = 0;
      for (ll i = s + lane; i < e; i += 64) {
        const int u = g.col[i];
        if (u != v && lv_priority(u) > pv) {
          const int cu = lv_load(colour + u) - base;
          if (cu >= 0 && cu < 64) m |= 1ull << cu;
        }
      }
      for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o, 64);
      if (~m) c = base + __ffsll((ull)~m) - 1;
      else base += 64;
    }
    if (lane == 0) {
      __hip_atomic_store(colour + v, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicMax(stat + 1, c);
    }
  }
}

// ---- the colour classes: bucket 2 colour (short rows) and 2 colour + 1 (long rows) --------------------------------------------------
__device__ inline int lv_bucket(const LvGraph& g, const int* colour, long v) {
  return 2 * colour[v] + (g.ip[v + 1] - g.ip[v] > g.tdeg ? 1 : 0);
}

__global__ __launch_bounds__(256) void lv_class_count_kernel(LvGraph g, const int* colour, ll* cnt) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < g.n) lv_add(cnt + lv_bucket(g, colour, v), 1);
}

__global__ __launch_bounds__(256) void lv_class_fill_kernel(LvGraph g, const int* colour, ll* cursor, int* list) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < g.n) list[atomicAdd(reinterpret_cast<ull*>(cursor + lv_bucket(g, colour, v)), 1ull)] = (int)v;
}

// ---- the move ---------------------------------------------------------------------------------------------------------------------------
struct LvMove {
  LvGraph g;
  const ll *k, *tot, *off;    // off [2 C + 1]: where each bucket of `list` starts
  const int *comm, *list;
  int* next;
  int colour;
  double gamma, m2;
  unsigned *A, *B;            // [nnz]: the long rows' sort arrays (a row uses its own span)
  ll* acc;                    // [nnz]: ... and their run sums
};

__device__ inline bool lv_better(double g, int id, double best, int bid) { return g > best || (g == best && id < bid); }

// rows of up to SMX_LV_TABLE_DEGREE entries: a wave per vertex
__global__ __launch_bounds__(256) void lv_move_wave_kernel(LvMove a) {
  __shared__ int keys[4][SMX_LV_TABLE_SLOTS];
  __shared__ ull vals[4][SMX_LV_TABLE_SLOTS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int* K = keys[w];
  ull* V = vals[w];
  const long b0 = a.off[2 * a.colour], b1 = a.off[2 * a.colour + 1], nw = (long)gridDim.x * 4;
  for (long i = b0 + (long)blockIdx.x * 4 + w; i < b1; i += nw) {
    const int v = a.list[i], own = a.comm[v];
    const ll s = a.g.ip[v], e = a.g.ip[v + 1];
    const int deg = (int)(e - s);   // (<= SMX_LV_TABLE_DEGREE: the bucket)
    int T = 64;
    while (T < 2 * deg) T <<= 1;
    const int shift = __clz(T) + 1;   // 32 - log2 T
    for (int j = lane; j < T; j += 64) { K[j] = -1; V[j] = 0ull; }
    wave_lds_sync();
    for (ll p = s + lane; p < e; p += 64) {
      const int u = a.g.col[p];
      if (u == v) continue;
      const int D = a.comm[u];
      unsigned h = ((unsigned)D * SMX_LV_HASH) >> shift;
      for (;;) {   // (at most half the slots are taken: an empty one is met)
        const int prev = atomicCAS(&K[h], -1, D);
        if (prev == -1 || prev == D) break;
        h = (h + 1u) & (unsigned)(T - 1);
      }
      atomicAdd(&V[h], (ull)a.g.val[p]);
    }
    wave_lds_sync();
    const ll kv = a.k[v];
    const double gk = a.gamma * (double)kv;
    double best = -INFINITY;
    int bid = INT_MAX;
    ll kin_own = 0;
    for (int j = lane; j < T; j += 64) {
      const int D = K[j];
      if (D < 0) continue;
      const ll kin = (ll)V[j];
      if (D == own) { kin_own = kin; continue; }
      const double gain = (double)kin - (gk * (double)a.tot[D]) / a.m2;
      if (lv_better(gain, D, best, bid)) { best = gain; bid = D; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bid, o, 64);
      if (lv_better(ob, oi, best, bid)) { best = ob; bid = oi; }
    }
    kin_own = halving_wave_sum(kin_own);   // (one lane holds it)
    if (lane == 0) {
      const double g_own = (double)kin_own - (gk * (double)(a.tot[own] - kv)) / a.m2;
      a.next[v] = (bid != INT_MAX && best > g_own) ? bid : own;
    }
    wave_lds_sync();   // (the slots are read before the next vertex clears them)
  }
}

// longer rows: a workgroup per vertex
__global__ __launch_bounds__(256) void lv_move_block_kernel(LvMove a) {
  __shared__ SortShared sh;
  __shared__ double sbest[4];
  __shared__ int sbid[4];
  __shared__ ll s4[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long b0 = a.off[2 * a.colour + 1], b1 = a.off[2 * a.colour + 2];
  for (long i = b0 + blockIdx.x; i < b1; i += gridDim.x) {   // (workgroup-uniform)
    const int v = a.list[i], own = a.comm[v];
    const ll s = a.g.ip[v];
    const int N = (int)(a.g.ip[v + 1] - s);
    const int32_t* col = a.g.col + s;
    const ll* val = a.g.val + s;
    const int* comm = a.comm;
    unsigned *A = a.A + s, *B = a.B + s;
    ll* acc = a.acc + s;
    for (int j = tid; j < N; j += 256) __hip_atomic_store(acc + j, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (at the L2, where the adds
                                                                                                          // run; the sort's barriers come first)
    const auto key = [col, comm, v](unsigned j) { const int u = col[j]; return u == v ? SMX_LV_SELF_KEY : (uint32_t)comm[u]; };
    const unsigned* S = block_radix_sort(key, N, 4, nullptr, A, B, sh);   // (four passes: the result is in B)
    block_tie_runs(key, [acc, val](int, unsigned entry, unsigned start) { lv_add(acc + start, val[entry]); }, N, S, A, sh);
    const ll kv = a.k[v];
    const double gk = a.gamma * (double)kv;
    double best = -INFINITY;
    int bid = INT_MAX;
    ll kin_own = 0;
    for (int j = tid; j < N; j += 256) {
      const uint32_t kj = key(S[j]);
      if (kj == SMX_LV_SELF_KEY || (j > 0 && key(S[j - 1]) == kj)) continue;   // a run's head carries its sum
      const ll kin = lv_load(acc + j);
      const int D = (int)kj;
      if (D == own) { kin_own = kin; continue; }
      const double gain = (double)kin - (gk * (double)a.tot[D]) / a.m2;
      if (lv_better(gain, D, best, bid)) { best = gain; bid = D; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bid, o, 64);
      if (lv_better(ob, oi, best, bid)) { best = ob; bid = oi; }
    }
    kin_own = halving_block_sum(kin_own, s4);
    if (lane == 0) { sbest[w] = best; sbid[w] = bid; }
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < 4; ++q)
        if (lv_better(sbest[q], sbid[q], best, bid)) { best = sbest[q]; bid = sbid[q]; }
      const double g_own = (double)kin_own - (gk * (double)(a.tot[own] - kv)) / a.m2;
      a.next[v] = (bid != INT_MAX && best > g_own) ? bid : own;
    }
    __syncthreads();
  }
}

// the colour's moves, then tot
__global__ __launch_bounds__(256) void lv_apply_kernel(const int* list, const ll* off, int colour, int* comm, const int* next, const ll* k,
                                                       ll* tot, int* moved) {
  const long b1 = off[2 * colour + 2], stride = (long)gridDim.x * 256;
  for (long i = off[2 * colour] + (long)blockIdx.x * 256 + threadIdx.x; i < b1; i += stride) {
    const int v = list[i], nc = next[v], oc = comm[v];
    if (nc == oc) continue;
    comm[v] = nc;
    lv_add(tot + oc, -k[v]);
    lv_add(tot + nc, k[v]);
    atomicAdd(moved, 1);
  }
}

// ---- modularity -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lv_inner_kernel(LvGraph g, const int* comm, ll* inner) {
  const int lane = threadIdx.x & 63;
  const long nw = (long)gridDim.x * 4;
  for (long v = (long)blockIdx.x * 4 + (threadIdx.x >> 6); v < g.n; v += nw) {
    const int c = comm[v];
    const ll e = g.ip[v + 1];
    ll sum = 0;
    for (ll i = g.ip[v] + lane; i < e; i += 64)
      if (comm[g.col[i]] == c) sum += g.val[i];
    sum = halving_wave_sum(sum);
    if (lane == 0 && sum) lv_add(inner + c, sum);
  }
}

__global__ __launch_bounds__(256) void lv_total_kernel(const int* comm, const ll* k, long n, ll* tot) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) lv_add(tot + comm[v], k[v]);
}

__global__ __launch_bounds__(256) void lv_term_kernel(const ll* inner, const ll* tot, long n, double gamma, double m2, double* term) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const double a = (double)inner[c] / m2, b = (double)tot[c] / m2;
  term[c] = a - gamma * (b * b);
}

struct LvSweepResult { double q; ll moved; };

__global__ __launch_bounds__(256) void lv_q_kernel(const double* term, long n, const int* moved, LvSweepResult* out) {
  __shared__ double s4[4];
  const double s = halving_column_sum(term, n, s4);
  if (threadIdx.x == 0) { out->q = s; out->moved = *moved; }
}

// ---- relabel: ids in order of the lowest member -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lv_low_kernel(const int* comm, long n, int* low) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) atomicMin(low + comm[v], (int)v);
}

__global__ __launch_bounds__(256) void lv_head_kernel(const int* comm, const int* low, long n, ll* flag) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) flag[v] = low[comm[v]] == (int)v ? 1 : 0;
}

__global__ __launch_bounds__(256) void lv_newid_kernel(const int* comm, const int* low, const ll* pos, long n, int* comm2) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) comm2[v] = (int)pos[low[comm[v]]];
}

__global__ __launch_bounds__(256) void lv_compose_kernel(int* label, long n, const int* map) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) label[i] = map[label[i]];
}

// ---- aggregate ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lv_row_entries_kernel(LvGraph g, const int* comm2, ll* cnt) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < g.n) lv_add(cnt + comm2[v], g.ip[v + 1] - g.ip[v]);
}

// a coarse row's table: more slots than it can have distinct columns
__global__ __launch_bounds__(256) void lv_table_size_kernel(ll* cnt, long nc) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c < nc) cnt[c] = min(2 * cnt[c] + 1, 2 * (ll)nc + 1);
}

__device__ inline void lv_table_add(int* K, ull* V, ll size, int key, ll w) {
  ll h = (ll)(((ull)(unsigned)key * SMX_LV_HASH) % (ull)size);
  for (;;) {   // (size > the row's distinct columns: an empty slot is met)
    const int prev = atomicCAS(K + h, -1, key);
    if (prev == -1 || prev == key) break;
    if (++h == size) h = 0;
  }
  atomicAdd(V + h, (ull)w);
}

__global__ __launch_bounds__(256) void lv_table_insert_kernel(LvGraph g, const int* comm2, const ll* tbase, int* K, ull* V) {
  const int lane = threadIdx.x & 63;
  const long nw = (long)gridDim.x * 4;
  for (long v = (long)blockIdx.x * 4 + (threadIdx.x >> 6); v < g.n; v += nw) {
    const int c = comm2[v];
    const ll base = tbase[c], size = tbase[c + 1] - base, e = g.ip[v + 1];
    for (ll p0 = g.ip[v]; p0 < e; p0 += 64) {   // (wave-uniform)
      const bool on = p0 + lane < e;
      const int key = on ? comm2[g.col[p0 + lane]] : -1;
      const ll wgt = on ? g.val[p0 + lane] : 0;
      const int k0 = __shfl(key, 0, 64);
      if (__all(!on || key == k0)) {   // one column (the rule at the late levels): one add
        const ll sum = halving_wave_sum(wgt);
        if (lane == 0) lv_table_add(K + base, V + base, size, k0, sum);
      } else if (on) {
        lv_table_add(K + base, V + base, size, key, wgt);
      }
    }
  }
}

__global__ __launch_bounds__(256) void lv_table_count_kernel(const ll* tbase, const int* K, long nc, ll* rc) {
  __shared__ ll s4[4];
  for (long c = blockIdx.x; c < nc; c += gridDim.x) {   // (workgroup-uniform)
    const ll e = tbase[c + 1];
    ll m = 0;
    for (ll j = tbase[c] + threadIdx.x; j < e; j += 256) m += K[j] >= 0 ? 1 : 0;
    m = halving_block_sum(m, s4);
    if (threadIdx.x == 0) rc[c] = m;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void lv_table_fill_kernel(const ll* tbase, const int* K, const ull* V, long nc, const ll* ip2, int32_t* col2,
                                                            ll* val2) {
  __shared__ unsigned cursor;
  for (long c = blockIdx.x; c < nc; c += gridDim.x) {
    if (threadIdx.x == 0) cursor = 0u;
    __syncthreads();
    const ll e = tbase[c + 1], o = ip2[c];
    for (ll j = tbase[c] + threadIdx.x; j < e; j += 256)
      if (K[j] >= 0) {
        const unsigned p = atomicAdd(&cursor, 1u);   // (below ip2[c + 1] - ip2[c]: the count of the same slots)
        col2[o + p] = K[j];
        val2[o + p] = (ll)V[j];
      }
    __syncthreads();
  }
}

// ---- the final ids: by decreasing size, ties to the lowest member (the lower id) --------------------------------------------------
__global__ __launch_bounds__(256) void lv_size_kernel(const int* label, long n, int* size) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) atomicAdd(size + label[v], 1);
}

__global__ __launch_bounds__(256) void lv_order_kernel(const int* size, int K, unsigned* A, unsigned* B, int* rank) {
  __shared__ SortShared sh;
  const auto key = [size](unsigned c) { return ((uint64_t)(0x2000000u - (unsigned)size[c]) << 24) | (uint64_t)c; };
  const unsigned* S = block_radix_sort(key, K, 7, nullptr, A, B, sh);   // (25 + 24 bits)
  for (int r = threadIdx.x; r < K; r += 256) rank[S[r]] = r;
}

namespace {

// the longest row that takes the wave's LDS table; the developer knob louvain_table_degree lowers it (a test sends every row through the
// workgroup form and asks for the same labels)
int lv_table_degree() { return (int)std::min(std::max(tuning("louvain_table_degree", (double)SMX_LV_TABLE_DEGREE), 1.0), (double)SMX_LV_TABLE_DEGREE); }

unsigned lv_tgrid(long n) { return (unsigned)std::max<long>(1, (n + 255) / 256); }
unsigned lv_wgrid(long n) { return (unsigned)std::max<long>(1, std::min<long>(SMX_LV_GRID_CAP, (n + 3) / 4)); }
unsigned lv_bgrid(long n) { return (unsigned)std::max<long>(1, std::min<long>(SMX_LV_GRID_CAP, n)); }

#define LV_LAUNCH(kernel, grid, ...)                                            \
  do {                                                                          \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, nullptr, __VA_ARGS__); \
    SMX_HIP(hipGetLastError());                                                 \
  } while (0)

// the checked, quantised graph: entries of q == 0 dropped
struct LvHostGraph {
  std::vector<ll> ip, q;
  std::vector<int32_t> col;
  ll m2 = 0;
  long n = 0;
};

// (rows, cols, w) -> its transpose, the rows' columns ascending: a counting sort by column
void lv_transpose(long n, const std::vector<ll>& ip, const std::vector<int32_t>& col, const std::vector<double>& w, std::vector<ll>* tip,
                  std::vector<int32_t>* tcol, std::vector<double>* tw) {
  const size_t nnz = col.size();
  tip->assign((size_t)n + 1, 0);
  tcol->resize(nnz);
  tw->resize(w.size());
  for (size_t e = 0; e < nnz; ++e) ++(*tip)[(size_t)col[e] + 1];
  for (long i = 0; i < n; ++i) (*tip)[(size_t)i + 1] += (*tip)[(size_t)i];
  std::vector<ll> cur(tip->begin(), tip->end() - 1);
  for (long i = 0; i < n; ++i)
    for (ll e = ip[(size_t)i]; e < ip[(size_t)i + 1]; ++e) {
      const ll p = cur[(size_t)col[(size_t)e]]++;
      (*tcol)[(size_t)p] = (int32_t)i;
      if (!w.empty()) (*tw)[(size_t)p] = w[(size_t)e];
    }
}

int lv_check_graph(const char* who, const int64_t* indptr, const int32_t* cols, const double* weights, int64_t n, LvHostGraph* out) {
  const std::string w(who);
  SMX_REQUIRE(indptr != nullptr, (w + ": null indptr").c_str());
  SMX_REQUIRE(n >= 1 && n <= SMX_LV_MAX_N, (w + ": 1 <= n <= 2^24").c_str());
  SMX_REQUIRE(indptr[0] == 0, (w + ": indptr[0] must be 0").c_str());
  for (int64_t i = 0; i < n; ++i) SMX_REQUIRE(indptr[i + 1] >= indptr[i], (w + ": indptr decreases").c_str());
  const ll nnz = indptr[n];
  SMX_REQUIRE(nnz <= SMX_LV_MAX_NNZ, (w + ": at most 2^31 - 1 entries").c_str());
  SMX_REQUIRE(nnz == 0 || cols != nullptr, (w + ": null cols").c_str());
  double wmax = 0.0;
  for (ll e = 0; e < nnz; ++e) {
    SMX_REQUIRE(cols[e] >= 0 && cols[e] < n, (w + ": a column outside 0 .. n - 1").c_str());
    if (weights) {
      SMX_REQUIRE(std::isfinite(weights[e]) && weights[e] >= 0.0, (w + ": a weight that is negative or not finite").c_str());
      wmax = std::max(wmax, weights[e]);
    }
  }
  // symmetric support and values, no column twice in a row: the transpose equals the matrix with its rows sorted (the transpose's transpose)
  std::vector<ll> ip(indptr, indptr + n + 1), tip, sip;
  std::vector<int32_t> col(cols, cols + nnz), tcol, scol;
  std::vector<double> wv, tw, sw;
  if (weights) wv.assign(weights, weights + nnz);
  lv_transpose((long)n, ip, col, wv, &tip, &tcol, &tw);
  lv_transpose((long)n, tip, tcol, tw, &sip, &scol, &sw);
  for (int64_t i = 0; i < n; ++i)
    for (ll e = sip[(size_t)i] + 1; e < sip[(size_t)i + 1]; ++e)
      SMX_REQUIRE(scol[(size_t)e] != scol[(size_t)e - 1], (w + ": a column stored twice in one row").c_str());
  SMX_REQUIRE(tip == sip && tcol == scol, (w + ": the support is not symmetric").c_str());
  SMX_REQUIRE(tw == sw, (w + ": the weights are not symmetric").c_str());
  out->n = (long)n;
  out->ip.assign((size_t)n + 1, 0);
  out->col.clear(); out->q.clear();
  out->col.reserve((size_t)nnz); out->q.reserve((size_t)nnz);
  out->m2 = 0;
  for (int64_t i = 0; i < n; ++i) {
    for (ll e = indptr[i]; e < indptr[i + 1]; ++e) {
      const ll q = weights ? (wmax > 0.0 ? llrint(weights[e] / wmax * SMX_LV_QUANT) : 0) : 1;
      if (q == 0) continue;
      out->col.push_back(cols[e]);
      out->q.push_back(q);
      out->m2 += q;
    }
    out->ip[(size_t)i + 1] = (ll)out->col.size();
  }
  return SMX_OK;
}

struct LvScan { ll* bsum; ll* total; };   // bsum [n / 1024 + 1]

int lv_scan(const LvScan& sc, const ll* in, ll* out, long n) {
  const long nb = std::max<long>(1, (n + 1023) / 1024);
  LV_LAUNCH(lv_scan_block_kernel, (unsigned)nb, in, out, n, sc.bsum);
  LV_LAUNCH(lv_scan_top_kernel, 1u, sc.bsum, nb, out + n);
  LV_LAUNCH(lv_scan_add_kernel, lv_tgrid(n), out, n, sc.bsum);
  return SMX_OK;
}

// in_c and the modularity of `comm` with totals `tot` -> out (device); moved: a device int copied beside it
int lv_modularity(const LvGraph& g, const int* comm, const ll* tot, ll* inner, double* term, double gamma, double m2, const int* moved,
                  LvSweepResult* out) {
  SMX_HIP(hipMemsetAsync(inner, 0, (size_t)g.n * sizeof(ll), nullptr));
  LV_LAUNCH(lv_inner_kernel, lv_wgrid(g.n), g, comm, inner);
  LV_LAUNCH(lv_term_kernel, lv_tgrid(g.n), inner, tot, (long)g.n, gamma, m2, term);
  LV_LAUNCH(lv_q_kernel, 1u, term, (long)g.n, moved, out);
  return SMX_OK;
}

int lv_put_graph(DeviceScratch& buf, const LvHostGraph& h, ll** ip, int32_t** col, ll** val) {
  const size_t n = (size_t)h.n, nnz = h.col.size();
  SMX_CHECK(buf.get(ip, n + 1)); SMX_CHECK(buf.get(col, nnz)); SMX_CHECK(buf.get(val, nnz));
  SMX_HIP(hipMemcpy(*ip, h.ip.data(), (n + 1) * sizeof(ll), hipMemcpyHostToDevice));
  if (nnz) {
    SMX_HIP(hipMemcpy(*col, h.col.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(*val, h.q.data(), nnz * sizeof(ll), hipMemcpyHostToDevice));
  }
  return SMX_OK;
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int32_t smx_louvain_table_degree(void) { return lv_table_degree(); }

int smx_louvain(const int64_t* indptr, const int32_t* cols, const double* weights, int64_t n, double resolution, double tol,
                int32_t max_sweeps, int32_t max_levels, int32_t* labels, int32_t* n_communities, int32_t* n_levels, double* modularity,
                int64_t* level_size, int32_t* sweeps, int32_t* colours) {
  SMX_REQUIRE(labels && n_communities && n_levels && modularity && level_size && sweeps && colours, "louvain: null output");
  SMX_REQUIRE(std::isfinite(resolution) && resolution >= 0.0, "louvain: resolution must be finite and >= 0");
  SMX_REQUIRE(std::isfinite(tol) && tol >= 0.0, "louvain: tol must be finite and >= 0");
  SMX_REQUIRE(max_sweeps >= 1 && max_levels >= 1, "louvain: max_sweeps >= 1 and max_levels >= 1");
  LvHostGraph h;
  SMX_CHECK(lv_check_graph("louvain", indptr, cols, weights, n, &h));
  *n_levels = 0;
  if (h.m2 == 0) {   // no weight at all: every vertex is its own community and Q = 0
    for (int64_t i = 0; i < n; ++i) labels[i] = (int32_t)i;
    *n_communities = (int32_t)n;
    return SMX_OK;
  }
  const size_t N = (size_t)h.n, NNZ = h.col.size();
  const double m2 = (double)h.m2, gamma = resolution;
  const int tdeg = lv_table_degree();
  DeviceScratch buf;
  ll *gip[2], *gval[2];
  int32_t* gcol[2];
  SMX_CHECK(lv_put_graph(buf, h, &gip[0], &gcol[0], &gval[0]));
  SMX_CHECK(buf.get(&gip[1], N + 1)); SMX_CHECK(buf.get(&gcol[1], NNZ)); SMX_CHECK(buf.get(&gval[1], NNZ));
  ll *dK, *dTot, *dTotSave, *dInner, *dCnt, *dOff, *dCursor, *dPos, *dTbase, *dRc;
  int *dComm, *dCommSave, *dNext, *dColour, *dLow, *dList, *dComm2, *dLabel, *dStat, *dTabK, *dRank;
  ull* dTabV;
  double* dTerm;
  LvSweepResult* dRes;
  LvScan sc;
  unsigned *dA = nullptr, *dB = nullptr;
  ll* dAcc = nullptr;
  SMX_CHECK(buf.get(&dK, N)); SMX_CHECK(buf.get(&dTot, N)); SMX_CHECK(buf.get(&dTotSave, N)); SMX_CHECK(buf.get(&dInner, N));
  SMX_CHECK(buf.get(&dCnt, 2 * N + 2)); SMX_CHECK(buf.get(&dOff, 2 * N + 2)); SMX_CHECK(buf.get(&dCursor, 2 * N + 2));
  SMX_CHECK(buf.get(&dPos, N + 1)); SMX_CHECK(buf.get(&dTbase, N + 1)); SMX_CHECK(buf.get(&dRc, N + 1));
  SMX_CHECK(buf.get(&dComm, N)); SMX_CHECK(buf.get(&dCommSave, N)); SMX_CHECK(buf.get(&dNext, N)); SMX_CHECK(buf.get(&dColour, N));
  SMX_CHECK(buf.get(&dLow, N)); SMX_CHECK(buf.get(&dList, N)); SMX_CHECK(buf.get(&dComm2, N)); SMX_CHECK(buf.get(&dLabel, N));
  SMX_CHECK(buf.get(&dRank, N)); SMX_CHECK(buf.get(&dStat, (size_t)4)); SMX_CHECK(buf.get(&dTerm, N)); SMX_CHECK(buf.get(&dRes, (size_t)1));
  SMX_CHECK(buf.get(&dTabK, 2 * NNZ + N)); SMX_CHECK(buf.get(&dTabV, 2 * NNZ + N));
  SMX_CHECK(buf.get(&sc.bsum, (2 * N + 2) / 1024 + 2));
  LV_LAUNCH(lv_iota_kernel, lv_tgrid((long)N), dLabel, (long)N);

  int cur = 0, levels = 0;
  long nl = (long)N;
  ll nnz_l = (ll)NNZ;
  long n_comm = (long)N;
  for (; levels < max_levels;) {
    const LvGraph g{gip[cur], gcol[cur], gval[cur], (int)nl, tdeg};
    // the level's start
    SMX_HIP(hipMemsetAsync(dStat, 0, 4 * sizeof(int), nullptr));
    LV_LAUNCH(lv_degree_kernel, lv_wgrid(nl), g, dK, dTot, dComm, dStat + 3);
    // colouring: rounds in pairs, the waiting vertices counted in the second
    SMX_HIP(hipMemsetAsync(dColour, 0xFF, (size_t)nl * sizeof(int), nullptr));
    int stat[4];
    for (;;) {   // (every round colours the waiting vertex of highest priority: at most nl rounds)
      SMX_HIP(hipMemsetAsync(dStat, 0, sizeof(int), nullptr));
      LV_LAUNCH(lv_colour_kernel, lv_wgrid(nl), g, dColour, dStat, 0);
      LV_LAUNCH(lv_colour_kernel, lv_wgrid(nl), g, dColour, dStat, 1);
      SMX_HIP(hipMemcpy(stat, dStat, sizeof(stat), hipMemcpyDeviceToHost));
      if (stat[0] == 0) break;
    }
    const int C = stat[1] + 1, n_big = stat[3];
    // the colour classes
    const long nbk = 2 * (long)C;
    SMX_HIP(hipMemsetAsync(dCnt, 0, (size_t)(nbk + 1) * sizeof(ll), nullptr));
    LV_LAUNCH(lv_class_count_kernel, lv_tgrid(nl), g, dColour, dCnt);
    SMX_CHECK(lv_scan(sc, dCnt, dOff, nbk));
    SMX_HIP(hipMemcpyAsync(dCursor, dOff, (size_t)(nbk + 1) * sizeof(ll), hipMemcpyDeviceToDevice, nullptr));
    LV_LAUNCH(lv_class_fill_kernel, lv_tgrid(nl), g, dColour, dCursor, dList);
    if (n_big > 0 && !dA) {   // (a coarse graph has no more entries than the first)
      SMX_CHECK(buf.get(&dA, NNZ)); SMX_CHECK(buf.get(&dB, NNZ)); SMX_CHECK(buf.get(&dAcc, NNZ));
    }
    LvMove mv;
    mv.g = g; mv.k = dK; mv.tot = dTot; mv.off = dOff; mv.comm = dComm; mv.list = dList; mv.next = dNext; mv.colour = 0;
    mv.gamma = gamma; mv.m2 = m2; mv.A = dA; mv.B = dB; mv.acc = dAcc;
    LvSweepResult res;
    SMX_CHECK(lv_modularity(g, dComm, dTot, dInner, dTerm, gamma, m2, dStat + 2, dRes));
    SMX_HIP(hipMemcpy(&res, dRes, sizeof(res), hipMemcpyDeviceToHost));
    double q_old = res.q;
    int n_sweeps = 0;
    while (n_sweeps < max_sweeps) {
      SMX_HIP(hipMemcpyAsync(dCommSave, dComm, (size_t)nl * sizeof(int), hipMemcpyDeviceToDevice, nullptr));
      SMX_HIP(hipMemcpyAsync(dTotSave, dTot, (size_t)nl * sizeof(ll), hipMemcpyDeviceToDevice, nullptr));
      SMX_HIP(hipMemsetAsync(dStat + 2, 0, sizeof(int), nullptr));
      for (int c = 0; c < C; ++c) {
        mv.colour = c;
        LV_LAUNCH(lv_move_wave_kernel, lv_wgrid(nl), mv);
        if (n_big > 0) LV_LAUNCH(lv_move_block_kernel, lv_bgrid(n_big), mv);
        LV_LAUNCH(lv_apply_kernel, std::min(lv_tgrid(nl), (unsigned)SMX_LV_GRID_CAP), dList, dOff, c, dComm, dNext, dK, dTot, dStat + 2);
      }
      ++n_sweeps;
      SMX_CHECK(lv_modularity(g, dComm, dTot, dInner, dTerm, gamma, m2, dStat + 2, dRes));
      SMX_HIP(hipMemcpy(&res, dRes, sizeof(res), hipMemcpyDeviceToHost));
      if (res.q < q_old) {   // the sweep lowered Q: its labels are put back
        SMX_HIP(hipMemcpyAsync(dComm, dCommSave, (size_t)nl * sizeof(int), hipMemcpyDeviceToDevice, nullptr));
        SMX_HIP(hipMemcpyAsync(dTot, dTotSave, (size_t)nl * sizeof(ll), hipMemcpyDeviceToDevice, nullptr));
        break;
      }
      const double gained = res.q - q_old;
      q_old = res.q;
      if (res.moved == 0 || gained <= tol) break;
    }
    // relabel in order of the lowest member; the first level's vertices follow
    SMX_HIP(hipMemsetAsync(dLow, 0x7F, (size_t)nl * sizeof(int), nullptr));
    LV_LAUNCH(lv_low_kernel, lv_tgrid(nl), dComm, nl, dLow);
    LV_LAUNCH(lv_head_kernel, lv_tgrid(nl), dComm, dLow, nl, dPos);
    SMX_CHECK(lv_scan(sc, dPos, dPos, nl));
    LV_LAUNCH(lv_newid_kernel, lv_tgrid(nl), dComm, dLow, dPos, nl, dComm2);
    LV_LAUNCH(lv_compose_kernel, lv_tgrid((long)N), dLabel, (long)N, dComm2);
    ll nc_ll = 0;
    SMX_HIP(hipMemcpy(&nc_ll, dPos + nl, sizeof(ll), hipMemcpyDeviceToHost));
    const long nc = (long)nc_ll;
    modularity[levels] = q_old; level_size[levels] = nc; sweeps[levels] = n_sweeps; colours[levels] = C;
    ++levels;
    n_comm = nc;
    if (nc == nl || levels == max_levels) break;
    // aggregate: a table per coarse row, count, scan, fill
    const int nx = cur ^ 1;
    SMX_HIP(hipMemsetAsync(dCnt, 0, (size_t)(nc + 1) * sizeof(ll), nullptr));
    LV_LAUNCH(lv_row_entries_kernel, lv_tgrid(nl), g, dComm2, dCnt);
    LV_LAUNCH(lv_table_size_kernel, lv_tgrid(nc), dCnt, nc);
    SMX_CHECK(lv_scan(sc, dCnt, dTbase, nc));
    const size_t slots = (size_t)(2 * nnz_l + nc);   // (>= the tables' total)
    SMX_HIP(hipMemsetAsync(dTabK, 0xFF, slots * sizeof(int), nullptr));
    SMX_HIP(hipMemsetAsync(dTabV, 0, slots * sizeof(ull), nullptr));
    LV_LAUNCH(lv_table_insert_kernel, lv_wgrid(nl), g, dComm2, dTbase, dTabK, dTabV);
    LV_LAUNCH(lv_table_count_kernel, lv_bgrid(nc), dTbase, dTabK, nc, dRc);
    SMX_CHECK(lv_scan(sc, dRc, gip[nx], nc));
    LV_LAUNCH(lv_table_fill_kernel, lv_bgrid(nc), dTbase, dTabK, dTabV, nc, gip[nx], gcol[nx], gval[nx]);
    SMX_HIP(hipMemcpy(&nnz_l, gip[nx] + nc, sizeof(ll), hipMemcpyDeviceToHost));
    SMX_REQUIRE(nnz_l >= 0 && (size_t)nnz_l <= NNZ, "louvain: internal error: a coarse graph larger than the first");
    cur = nx;
    nl = nc;
  }
  // the final ids
  unsigned *dSa, *dSb;
  int* dSize;
  SMX_CHECK(buf.get(&dSa, (size_t)n_comm)); SMX_CHECK(buf.get(&dSb, (size_t)n_comm)); SMX_CHECK(buf.get(&dSize, (size_t)n_comm));
  LV_LAUNCH(lv_size_kernel, lv_tgrid((long)N), dLabel, (long)N, dSize);
  LV_LAUNCH(lv_order_kernel, 1u, dSize, (int)n_comm, dSa, dSb, dRank);
  LV_LAUNCH(lv_compose_kernel, lv_tgrid((long)N), dLabel, (long)N, dRank);
  SMX_HIP(hipDeviceSynchronize());
  SMX_HIP(hipMemcpy(labels, dLabel, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  *n_communities = (int32_t)n_comm;
  *n_levels = levels;
  return SMX_OK;
}

int smx_louvain_modularity(const int64_t* indptr, const int32_t* cols, const double* weights, int64_t n, const int32_t* labels,
                           double resolution, double* q) {
  SMX_REQUIRE(labels && q, "louvain_modularity: null labels or output");
  SMX_REQUIRE(std::isfinite(resolution) && resolution >= 0.0, "louvain_modularity: resolution must be finite and >= 0");
  LvHostGraph h;
  SMX_CHECK(lv_check_graph("louvain_modularity", indptr, cols, weights, n, &h));
  for (int64_t i = 0; i < n; ++i) SMX_REQUIRE(labels[i] >= 0 && labels[i] < n, "louvain_modularity: a label outside 0 .. n - 1");
  *q = 0.0;
  if (h.m2 == 0) return SMX_OK;
  const size_t N = (size_t)h.n;
  DeviceScratch buf;
  ll *dIp, *dVal, *dK, *dTot, *dInner;
  int32_t* dCol;
  int *dComm, *dStat;
  double* dTerm;
  LvSweepResult* dRes;
  SMX_CHECK(lv_put_graph(buf, h, &dIp, &dCol, &dVal));
  SMX_CHECK(buf.get(&dK, N)); SMX_CHECK(buf.get(&dTot, N)); SMX_CHECK(buf.get(&dInner, N)); SMX_CHECK(buf.get(&dTerm, N));
  SMX_CHECK(buf.put(&dComm, (const int*)labels, N)); SMX_CHECK(buf.get(&dStat, (size_t)1)); SMX_CHECK(buf.get(&dRes, (size_t)1));
  const LvGraph g{dIp, dCol, dVal, (int)N, SMX_LV_TABLE_DEGREE};
  LV_LAUNCH(lv_degree_kernel, lv_wgrid((long)N), g, dK, (ll*)nullptr, (int*)nullptr, (int*)nullptr);
  LV_LAUNCH(lv_total_kernel, lv_tgrid((long)N), dComm, dK, (long)N, dTot);
  SMX_CHECK(lv_modularity(g, dComm, dTot, dInner, dTerm, resolution, (double)h.m2, dStat, dRes));
  LvSweepResult res;
  SMX_HIP(hipMemcpy(&res, dRes, sizeof(res), hipMemcpyDeviceToHost));
  *q = res.q;
  return SMX_OK;
}

}  // extern "C"
