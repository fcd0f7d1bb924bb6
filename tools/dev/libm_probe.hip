// libm_probe.hip -- the accuracy of the device library's expf, logf and lgammaf as this project's flags compile them (-O3, no fast-math),
// on the arguments the label heads hand them (smx_loss.hip: label_loss_kernel, label_tril_kernel), against the host's double functions:
//   expf   differences x - max <= 0 down to the underflow                   [-104, 0], 2^22 points, and -2^-k
//   logf   sums of at most 70 terms expf(x - max), one of them 1            [1, 70], 2^22 points
//   lgammaf(y + 1)  counts; real targets                                    every integer y = 0 .. 20000; 2^20 points of [0, 20000], 2^18 of [0, 3]
// Prints the largest error in ulps of the float32 result (the float32 nearest the double value is 0.5 at most), and for lgammaf the error
// against the term the bound tables carry for it.  tests/label_heads_ref.py records what this printed on an MI355X beside its table.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/dev/libm_probe.hip -o tools/dev/libm_probe && tools/dev/libm_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void probe_kernel(int fn, const float* x, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = fn == 0 ? expf(x[i]) : fn == 1 ? logf(x[i]) : lgammaf(x[i] + 1.f);
}

static double ulp_of(double v) {
  int e;
  frexp(v, &e);                                    // |v| = f 2^e, f in [0.5, 1)
  if (e < -125) e = -125;                          // (subnormal results: the spacing of 2^-149)
  return ldexp(1.0, e - 24);
}

static int run(int fn, const char* name, const std::vector<float>& x) {
  const int n = (int)x.size();
  float *dx, *dout;
  if (hipMalloc(&dx, n * sizeof(float)) != hipSuccess || hipMalloc(&dout, n * sizeof(float)) != hipSuccess) return 1;
  if (hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 1;
  hipLaunchKernelGGL(probe_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, fn, dx, dout, n);
  std::vector<float> got(n);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(got.data(), dout, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  (void)hipFree(dx); (void)hipFree(dout);
  // `term`: the error in units of the bound table's lgammaf term max(12 |lgamma|, 1) u, u = 2^-24 (a relative measure fails at the zeros y = 0, 1)
  double worst = 0.0, worst_term = 0.0; float at = 0.f, at_term = 0.f; int nan = 0;
  for (int i = 0; i < n; ++i) {
    const double a = x[i], ref = fn == 0 ? exp(a) : fn == 1 ? log(a) : lgamma(a + 1.0);
    if (std::isnan(got[i])) { ++nan; continue; }
    const double err = fabs((double)got[i] - ref), t = err / (fmax(12.0 * fabs(ref), 1.0) * ldexp(1.0, -24));
    if (t > worst_term) { worst_term = t; at_term = x[i]; }
    if (ref == 0.0) continue;
    const double u = err / ulp_of(ref);
    if (u > worst) { worst = u; at = x[i]; }
  }
  printf("%-16s %8d arguments: worst error %.3f ulp at x = %.9g", name, n, worst, at);
  if (fn == 2) printf("; %.3f of max(12 |lgamma|, 1) u at y = %.9g", worst_term, at_term);
  printf("; %d NaN\n", nan);
  return 0;
}

int main() {
  std::vector<float> x;
  const int N = 1 << 22;
  for (int i = 0; i < N; ++i) x.push_back((float)(-104.0 * i / (N - 1)));
  for (int k = 1; k < 140; ++k) x.push_back(-ldexpf(1.f, -k));
  if (run(0, "expf", x)) return 1;
  x.clear();
  for (int i = 0; i < N; ++i) x.push_back((float)(1.0 + 69.0 * i / (N - 1)));
  if (run(1, "logf", x)) return 1;
  x.clear();
  for (int i = 0; i <= 20000; ++i) x.push_back((float)i);
  if (run(2, "lgammaf integer", x)) return 1;
  x.clear();
  for (int i = 0; i < (1 << 20); ++i) x.push_back((float)(20000.0 * i / ((1 << 20) - 1)));
  for (int i = 0; i < (1 << 18); ++i) x.push_back((float)(3.0 * i / ((1 << 18) - 1)));
  if (run(2, "lgammaf real", x)) return 1;
  return 0;
}
