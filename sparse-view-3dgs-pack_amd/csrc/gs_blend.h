// gs_blend.h - the per-(pixel, Gaussian) alpha evaluation shared by the forward and backward blend kernels, and the cross-lane
// sums of the backward ones (gs_render_bwd_wave.hip, gs_depth_pass.hip).
//
// Both kernels must take IDENTICAL skip decisions (alpha >= 1/255, power <= 0) for the same pair, so the
// expression is spelled with explicit fmaf in one place.  The conic is staged pre-multiplied into the log2
// domain (qa = -0.5 log2e cxx, qb = -log2e cxy, qc = -0.5 log2e cyy): power2 = qa dx^2 + qb dx dy + qc dy^2 feeds
// v_exp_f32 directly (5 VALU ops + 1 transcendental instead of 8 + 1); reference: forward.cu:343-356,
// backward.cu:549-560 (power = -0.5 (A dx^2 + C dy^2) - B dx dy, alpha = min(0.99, o exp(power))).
#pragma once
#include <hip/hip_runtime.h>

#define GS_LOG2E 1.4426950408889634f

__device__ __forceinline__ float4 blend_stage_conic(float4 conic_o) {
  return make_float4(-0.5f * GS_LOG2E * conic_o.x, -GS_LOG2E * conic_o.y, -0.5f * GS_LOG2E * conic_o.z, conic_o.w);
}
// returns power in the log2 domain (same sign as the reference's `power`)
__device__ __forceinline__ float blend_power2(float4 q, float dx, float dy) {
  const float t = fmaf(q.y, dy, q.x * dx);
  return fmaf(q.z * dy, dy, t * dx);
}
__device__ __forceinline__ float blend_exp2(float p2) { return __builtin_amdgcn_exp2f(p2); }

// ---- cross-lane sums of the backward blend: DPP row scans and permlane swaps ----
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ float dppw(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, BOUND));
}
typedef unsigned uint2v __attribute__((ext_vector_type(2)));
// v_permlane32_swap: lanes 32..63 of a <-> lanes 0..31 of b; the sum then holds a's lane-pair sums in lanes
// 0..31 and b's in lanes 32..63: TWO values halve their lane count for one swap + one add
__device__ __forceinline__ float swap32_add(float a, float b) {
  const uint2v r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
  // NB: element access as r[0]/r[1] + __uint_as_float; `bit_cast(float, r.x) + bit_cast(float, r.y)` is miscompiled
  // by hipcc 7.2 into x + x (checked in the ISA)
  const unsigned x = r[0], y = r[1];
  return __uint_as_float(x) + __uint_as_float(y);
}
// v_permlane16_swap: odd rows of a <-> even rows of b; with a = (u | w), b = (x | y) as produced by swap32_add the
// sum holds u, x, w, y in rows 0..3 (16 lanes each)
__device__ __forceinline__ float swap16_add(float a, float b) {
  const uint2v r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
  const unsigned x = r[0], y = r[1];  // (same note)
  return __uint_as_float(x) + __uint_as_float(y);
}
// inclusive scan inside each row of 16 lanes: lane 15 of every row ends with the row total
__device__ __forceinline__ float row_total_in_lane15(float v) {
  v += dppw<0x111, 0xf, true>(v);  // row_shr:1
  v += dppw<0x112, 0xf, true>(v);  // row_shr:2
  v += dppw<0x114, 0xf, true>(v);  // row_shr:4
  v += dppw<0x118, 0xf, true>(v);  // row_shr:8
  return v;
}
// the same scan in the other direction: lane 0 of every row ends with the row total
__device__ __forceinline__ float row_total_in_lane0(float v) {
  v += dppw<0x101, 0xf, true>(v);  // row_shl:1
  v += dppw<0x102, 0xf, true>(v);  // row_shl:2
  v += dppw<0x104, 0xf, true>(v);  // row_shl:4
  v += dppw<0x108, 0xf, true>(v);  // row_shl:8
  return v;
}
