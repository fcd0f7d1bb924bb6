// ulp_probe.hip -- accuracy of the single-instruction transcendental forms the kernels use (smx_device.h) against
// float64 on the device: max and mean relative error of v_log_f32 (as ln), v_exp_f32, v_rcp_f32, v_sqrt_f32 and of rsqrtf over the
// argument ranges that occur in the step; of powf(b, t) on the ladder of the optimiser's step size (adam_lr_t: smx_adam.hip); and what
// v_sqrt_f32 returns at denormal arguments.   hipcc --offload-arch=gfx950 -O3 tools/ulp_probe.hip -o tools/ulp_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <vector>

__global__ void probe(int kind, float lo, float hi, int n, double* max_rel, double* sum_rel, double* max_abs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // log-uniform sweep of [lo, hi]
  const float x = (float)((double)lo * pow((double)hi / (double)lo, (double)i / (double)(n - 1)));   // (hi / lo is beyond float32 for the widest ranges)
  float got; double ref;
  switch (kind) {
    case 0: got = __builtin_amdgcn_logf(x) * 0.6931471805599453f; ref = log((double)x); break;
    case 1: got = __expf(-x); ref = exp(-(double)x); break;
    case 2: got = __builtin_amdgcn_rcpf(x); ref = 1.0 / (double)x; break;
    case 3: got = __builtin_amdgcn_sqrtf(x); ref = sqrt((double)x); break;
    case 4: got = __builtin_amdgcn_logf(1.0f + x) * 0.6931471805599453f; ref = log1p((double)x); break;   // log(1 + e)
    case 6: got = rsqrtf(x); ref = 1.0 / sqrt((double)x); break;   // (BatchNorm's inv = rsqrtf(var + eps): smx_bn.hip)
    default: got = __logf(x); ref = log((double)x); break;
  }
  const double ab = fabs((double)got - ref), rel = ref != 0.0 ? ab / fabs(ref) : ab;
  atomicMax((unsigned long long*)max_rel, (unsigned long long)__double_as_longlong(rel));
  atomicMax((unsigned long long*)max_abs, (unsigned long long)__double_as_longlong(ab));
  atomicAdd(sum_rel, rel);
}

// powf(b, (float)t) as adam_lr_t forms it against pow in float64: relative error in units of u = 2^-24 (0 where b^t is below float32)
__global__ void powf_probe(const float* b, const unsigned* t, int nb, int nt, double* rel_u) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb * nt) return;
  const float got = powf(b[i / nt], (float)t[i % nt]);
  const double ref = pow((double)b[i / nt], (double)(float)t[i % nt]);
  rel_u[i] = ref >= 1.1754943508222875e-38 ? fabs((double)got - ref) / ref * 16777216.0 : (got == 0.f || ref > 0.0 ? 0.0 : 1e300);
}
__global__ void sqrt_denormal_probe(const float* x, float* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = __builtin_amdgcn_sqrtf(x[i]);
}

int main() {
  {
    const float b[4] = {0.5f, 0.9f, 0.999f, 0.99999f};
    const unsigned t[7] = {1u, 2u, 3u, 10u, 1000u, 100000u, 16777217u};
    float* db; unsigned* dt; double* dr; double h[28];
    hipMalloc(&db, sizeof(b)); hipMalloc(&dt, sizeof(t)); hipMalloc(&dr, sizeof(h));
    hipMemcpy(db, b, sizeof(b), hipMemcpyHostToDevice); hipMemcpy(dt, t, sizeof(t), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(powf_probe, dim3(1), dim3(64), 0, 0, db, dt, 4, 7, dr);
    hipMemcpy(h, dr, sizeof(h), hipMemcpyDeviceToHost);
    double worst = 0.0;
    for (int i = 0; i < 4; ++i) {
      printf("powf b^t   b = %-8g rel err / u at t = 1, 2, 3, 10, 1000, 1e5, 2^24 + 1:", b[i]);
      for (int j = 0; j < 7; ++j) { printf(" %.3f", h[i * 7 + j]); if (h[i * 7 + j] > worst) worst = h[i * 7 + j]; }
      printf("\n");
    }
    printf("%-58s max rel %.3f u\n", "powf b^t   over the ladder above", worst);
    const float x[6] = {1e-45f, 1e-42f, 1e-40f, 9.99e-39f, 1.17549421e-38f, 1.17549435e-38f};
    float *dx, *dy, y[6];
    hipMalloc(&dx, sizeof(x)); hipMalloc(&dy, sizeof(y));
    hipMemcpy(dx, x, sizeof(x), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(sqrt_denormal_probe, dim3(1), dim3(64), 0, 0, dx, dy, 6);
    hipMemcpy(y, dy, sizeof(y), hipMemcpyDeviceToHost);
    for (int i = 0; i < 6; ++i) printf("v_sqrt x   x = %.8e -> %.8e  (sqrt %.8e)\n", x[i], y[i], sqrt((double)x[i]));
  }
  double* d; hipMalloc(&d, 3 * sizeof(double));
  struct { int kind; float lo, hi; const char* name; } cases[] = {
      {0, 1e-30f, 1e30f, "ln x      = v_log * ln2, x in [1e-30, 1e30]"}, {0, 0.5f, 2.0f, "ln x      near 1, x in [0.5, 2]"},
      {0, 0.97f, 1.03f, "ln x      x in [0.97, 1.03]"},
      {4, 0.03125f, 1.0f, "ln(1 + e) e in [1/32, 1] (log1p_small above its series)"},
      {1, 1e-6f, 80.f, "exp(-x)   = v_exp(x log2e), x in [1e-6, 80]"}, {2, 1e-30f, 1e30f, "1 / x     = v_rcp"},
      {3, 1e-30f, 1e30f, "sqrt x    = v_sqrt"}, {5, 0.5f, 2.0f, "__logf    near 1 (the 14-instruction form)"},
      {6, 1e-18f, 1e18f, "rsqrtf x  x in [1e-18, 1e18]"}, {6, 1e-3f, 4e-3f, "rsqrtf x  x in [1e-3, 4e-3] (var + eps at small variances)"}};
  const int n = 1 << 22;
  for (auto& c : cases) {
    hipMemset(d, 0, 3 * sizeof(double));
    hipLaunchKernelGGL(probe, dim3(n / 256), dim3(256), 0, 0, c.kind, c.lo, c.hi, n, d, d + 1, d + 2);
    double h[3]; hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    printf("%-58s max rel %.3e  mean rel %.3e  max abs %.3e\n", c.name, h[0], h[1] / n, h[2]);
  }
  return 0;
}
