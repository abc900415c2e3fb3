// gs_dng_reg_act.h - the activations gs_dng_reg.hip evaluates in its raw form.  They sit in a header of their own so that
// tests/tools/dng_reg_act_probe.hip measures these very functions against float64.
#pragma once
#include <hip/hip_runtime.h>

// s = exp(raw scaling)
__device__ __forceinline__ float dr_exp(float r) { return expf(r); }

// o = sigmoid(r) and om = 1 - sigmoid(r), each formed without a cancellation: e = exp(-|r|) <= 1, and 1 / (1 + e), e / (1 + e)
// are the larger and the smaller of the two.  (1.f - o would lose every bit of om as o approaches 1, and the gradient with
// respect to the raw opacity carries the factor o (1 - o).)
__device__ __forceinline__ void dr_sigmoid(float r, float& o, float& om) {
  const float e = expf(-fabsf(r));
  const float a = 1.f / (1.f + e), b = e / (1.f + e);
  o = r >= 0.f ? a : b;
  om = r >= 0.f ? b : a;
}
