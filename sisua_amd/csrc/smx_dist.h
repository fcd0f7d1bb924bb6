// smx_dist.h -- float64 direct-form distances between cells Z [N][D] float32, shared by smx_cluster.hip (silhouette, k-means) and
// smx_knn.hip (exact nearest neighbours): one cell per thread in registers, the other operand staged in LDS as float64 and read as a
// broadcast.  Everything is sum_d (x[d] - y[d])^2 in float64: no Gram form (the cancellation of |x|^2 + |y|^2 - 2 x.y for near neighbours is
// what these files exist to avoid).
#pragma once
#include <hip/hip_runtime.h>

namespace smx {

#define SMX_CL_TILE 256        // cells per workgroup (one per thread)
#define SMX_CL_LDS_DOUBLES 4096   // 32 KB of staged float64 operands
#define SMX_CL_MAX_D 128
#define SMX_CL_MAX_K 256

__device__ inline float nan_if_inf(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) == 0x7F800000u ? __uint_as_float(0x7FC00000u) : v; }

// sum_d (zi[d] - y[d])^2 over the padded width: four chains by d mod 4, then (s0 + s1) + (s2 + s3).  y: LDS, the same address in every lane.
template <int DP>
__device__ inline double sqdist(const float (&zi)[DP], const double* y) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
  for (int d = 0; d < DP; d += 4) {
    const double t0 = (double)zi[d] - y[d], t1 = (double)zi[d + 1] - y[d + 1], t2 = (double)zi[d + 2] - y[d + 2], t3 = (double)zi[d + 3] - y[d + 3];
    s0 = fma(t0, t0, s0); s1 = fma(t1, t1, s1); s2 = fma(t2, t2, s2); s3 = fma(t3, t3, s3);
  }
  return (s0 + s1) + (s2 + s3);
}

// rows [r0, r0 + n_rows) of a row-major matrix src [..][D] -> LDS [n_rows][DP] float64, zero beyond D.  T: float (cells) or double (centres)
template <int DP, class T>
__device__ inline void stage_rows(double* sh, const T* src, long r0, int n_rows, int D) {
  for (int e = threadIdx.x; e < n_rows * DP; e += SMX_CL_TILE) {
    const int jj = e / DP, d = e % DP;
    double v = 0.0;
    if (d < D) {
      if constexpr (sizeof(T) == 4) v = (double)nan_if_inf((float)src[(r0 + jj) * D + d]);
      else v = (double)src[(r0 + jj) * D + d];
    }
    sh[e] = v;
  }
}

template <int DP>
__device__ inline void load_cell(float (&zi)[DP], const float* Z, long i, long N, int D) {
#pragma unroll
  for (int d = 0; d < DP; ++d) zi[d] = (i < N && d < D) ? nan_if_inf(Z[i * D + d]) : 0.f;
}

// the register width of a cell: D rounded up to 16, 32, 64 or 128
inline int padded_width(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : D <= 64 ? 64 : 128; }

}  // namespace smx
