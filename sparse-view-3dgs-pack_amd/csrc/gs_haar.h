// gs_haar.h - the Haar analysis butterfly and the bilinear upsample shared by gs_loss.hip and gs_wef.hip (device code).
//
//   haar_block   one 2 x 2 block of pytorch_wavelets.DWTForward('db1', 'symmetric'): two separable stages with
//                c = float32(0.70710678...), first along W then along H; LH = low along W / high along H.  Odd sizes repeat the
//                last sample: the caller reads min(2i + 1, n - 1)
//   bilin_tap /  F.interpolate(size=(H,W), mode='bilinear', align_corners=False): source index scale * (dst + 0.5) - 0.5 clamped
//   bilin_sample at 0, the neighbour clamped at the last sample, rows blended after columns
// Both files compile with -ffp-contract=off: every operation here rounds on its own.
#pragma once
#include <hip/hip_runtime.h>

#define HC 0.7071067811865476f

struct Bands {
  float ll, lh, hl, hh;
};
__device__ __forceinline__ Bands haar_block(float a, float b, float c, float d) {
  const float lo_t = HC * a + HC * b, hi_t = HC * a - HC * b;
  const float lo_b = HC * c + HC * d, hi_b = HC * c - HC * d;
  Bands r;
  r.ll = HC * lo_t + HC * lo_b;
  r.lh = HC * lo_t - HC * lo_b;
  r.hl = HC * hi_t + HC * hi_b;
  r.hh = HC * hi_t - HC * hi_b;
  return r;
}
__device__ __forceinline__ int cdiv2(int n) { return (n + 1) >> 1; }

struct BilinTap {
  int i0, i1;
  float l0, l1;
};
// output sample `o` of `n_out` along one axis of a plane with `n_in` samples.  EXACT_EDGE: where the neighbour is clamped onto
// the sample itself (the last sample, or a plane of one) the weights are (1, 0), so that l0 * v + l1 * v is v and not v
// rounded twice - a plane of ONE coefficient then upsamples to exactly that coefficient (gs_wef.hip normalises by max - min)
template <bool EXACT_EDGE = false>
__device__ __forceinline__ BilinTap bilin_tap(int o, int n_in, int n_out) {
  const float scale = (float)n_in / (float)n_out;
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0) src = 0;
  BilinTap t;
  t.i0 = min((int)src, n_in - 1);  // (src < n_in - 0.5 in exact arithmetic: the clamp only guards the address)
  t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  if (EXACT_EDGE && t.i1 == t.i0) { t.l0 = 1.f; t.l1 = 0.f; }
  return t;
}
__device__ __forceinline__ float bilin_sample(const float* __restrict__ low, int w, const BilinTap& ty, const BilinTap& tx) {
  return ty.l0 * (tx.l0 * low[(size_t)ty.i0 * w + tx.i0] + tx.l1 * low[(size_t)ty.i0 * w + tx.i1]) +
         ty.l1 * (tx.l0 * low[(size_t)ty.i1 * w + tx.i0] + tx.l1 * low[(size_t)ty.i1 * w + tx.i1]);
}
