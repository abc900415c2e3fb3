// Developer probe: the relative error of the activations gs_dng_reg.hip evaluates in its raw form (csrc/gs_dng_reg_act.h:
// s = exp(r), o = sigmoid(r), om = 1 - sigmoid(r)) against float64, over the ranges tests/test_gpu_dng_reg.py draws its raw
// inputs from (scaling [-7, 1.5], opacity [-7, 7]), N evenly spaced fp32 arguments each.  The device library's accuracy for
// expf is not documented in the installed tree, so the raw form's tolerance rests on this measurement.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I sparse-view-3dgs-pack_amd/csrc tests/tools/dng_reg_act_probe.hip -o probe
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "gs_dng_reg_act.h"

__global__ void probe_kernel(const float* r, int n, float* s, float* o, float* om) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  s[i] = dr_exp(r[i]);
  dr_sigmoid(r[i], o[i], om[i]);
}

#define CHECK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

static int run(const char* what, float lo, float hi, int n, bool sigmoid) {
  std::vector<float> r(n), s(n), o(n), om(n);
  for (int i = 0; i < n; i++) r[i] = (float)((double)lo + ((double)hi - (double)lo) * i / (n - 1));
  float *dr, *ds, *dout, *dom;
  CHECK(hipMalloc(&dr, 4 * (size_t)n)); CHECK(hipMalloc(&ds, 4 * (size_t)n));
  CHECK(hipMalloc(&dout, 4 * (size_t)n)); CHECK(hipMalloc(&dom, 4 * (size_t)n));
  CHECK(hipMemcpy(dr, r.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dr, n, ds, dout, dom);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(s.data(), ds, 4 * (size_t)n, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(o.data(), dout, 4 * (size_t)n, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(om.data(), dom, 4 * (size_t)n, hipMemcpyDeviceToHost));
  CHECK(hipFree(dr)); CHECK(hipFree(ds)); CHECK(hipFree(dout)); CHECK(hipFree(dom));
  double e[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < n; i++) {
    const double x = (double)r[i];
    const double w[3] = {std::exp(x), 1.0 / (1.0 + std::exp(-x)), 1.0 / (1.0 + std::exp(x))};
    const double g[3] = {(double)s[i], (double)o[i], (double)om[i]};
    for (int k = sigmoid ? 1 : 0; k < (sigmoid ? 3 : 1); k++) {
      const double rel = std::fabs(g[k] - w[k]) / w[k];
      if (rel > e[k]) e[k] = rel;
    }
  }
  const double u = std::ldexp(1.0, -24);
  if (sigmoid)
    std::printf("%s over [%g, %g], %d arguments: max relative error sigmoid %.4e (%.3f x 2^-24), 1 - sigmoid %.4e (%.3f x 2^-24)\n",
                what, lo, hi, n, e[1], e[1] / u, e[2], e[2] / u);
  else
    std::printf("%s over [%g, %g], %d arguments: max relative error %.4e (%.3f x 2^-24)\n", what, lo, hi, n, e[0], e[0] / u);
  return 0;
}

// exp over a range that leaves fp32's normal numbers at both ends (tests/model_ops_reference.py takes its E from this line):
// the relative error where the float64 result is a normal fp32 number, the absolute error (in units of FLT_MIN) where it is
// below them, and the arguments at which the fp32 result and the rounded float64 result disagree about being infinite.
static int run_exp_wide(float lo, float hi, int n) {
  std::vector<float> r(n), s(n);
  for (int i = 0; i < n; i++) r[i] = (float)((double)lo + ((double)hi - (double)lo) * i / (n - 1));
  float *dr, *ds, *dout, *dom;
  CHECK(hipMalloc(&dr, 4 * (size_t)n)); CHECK(hipMalloc(&ds, 4 * (size_t)n));
  CHECK(hipMalloc(&dout, 4 * (size_t)n)); CHECK(hipMalloc(&dom, 4 * (size_t)n));
  CHECK(hipMemcpy(dr, r.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dr, n, ds, dout, dom);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(s.data(), ds, 4 * (size_t)n, hipMemcpyDeviceToHost));
  CHECK(hipFree(dr)); CHECK(hipFree(ds)); CHECK(hipFree(dout)); CHECK(hipFree(dom));
  const double flt_min = std::ldexp(1.0, -126), u = std::ldexp(1.0, -24);
  double rel = 0.0, sub = 0.0;
  int inf_differs = 0;
  for (int i = 0; i < n; i++) {
    const double w = std::exp((double)r[i]), g = (double)s[i];
    if (std::isinf((float)w) || std::isinf(s[i])) {
      inf_differs += std::isinf((float)w) != std::isinf(s[i]);
    } else if (w >= flt_min) {
      rel = std::fmax(rel, std::fabs(g - w) / w);
    } else {
      sub = std::fmax(sub, std::fabs(g - w) / flt_min);
    }
  }
  std::printf("exp over [%g, %g], %d arguments: max relative error %.4e (%.3f x 2^-24) where the result is a normal number; "
              "below them max absolute error %.4e x 2^-126; infinite on one side only at %d arguments\n",
              lo, hi, n, rel, rel / u, sub, inf_differs);
  return 0;
}

int main() {
  const int n = 1 << 22;
  if (run("exp", -7.f, 1.5f, n, false)) return 1;
  if (run("sigmoid", -7.f, 7.f, n, true)) return 1;
  if (run_exp_wide(-104.f, 89.f, n)) return 1;
  return 0;
}
