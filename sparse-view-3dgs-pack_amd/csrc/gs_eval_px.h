// gs_eval_px.h - the pixel transform of the test-set evaluation, the one copy gs_eval.hip (PSNR / SSIM / L1) and
// gs_eval_files.hip (SSIM_sk) share: both see the same float32 pixel for the same flags.
#pragma once
#include "gs_common.h"

// torchvision save_image's byte: mul(255).add_(0.5).clamp_(0, 255).to(uint8) - two separately rounded fp32 operations
__device__ __forceinline__ uint8_t ev_byte(float x) {
  const float s = __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
  return (uint8_t)(int)fminf(fmaxf(s, 0.f), 255.f);
}
// the pixel as the metrics see it; m is read only with GS_EVAL_MASK_DTU
__device__ __forceinline__ float ev_transform(float x, float m, int flags) {
  if (flags & GS_EVAL_CLAMP) x = fminf(fmaxf(x, 0.f), 1.f);
  if (flags & GS_EVAL_QUANTISE) x = __fdiv_rn((float)ev_byte(x), 255.0f);  // to_tensor
  if (flags & GS_EVAL_MASK_DTU) x = __fadd_rn(__fmul_rn(x, m), __fsub_rn(1.0f, m));
  return x;
}
