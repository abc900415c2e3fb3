// gs_resize.h - the two pieces of Pillow's integer resize (Resample.c) that gs_eval_files.hip and gs_image_ingest.hip share:
// the accumulator's shift-and-clamp and the guarded read of one table row.  Included only by those two files.
#pragma once
#include <stdint.h>

constexpr int RS_PREC = 22;  // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ uint8_t rs_clip8(int32_t acc) {
  const int32_t v = acc >> RS_PREC;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
// a table row whose run leaves the source axis reads nothing (the byte is 0): a wrong table cannot make a load stray
__device__ __forceinline__ int rs_run(const int32_t* __restrict__ bounds, int o, int ksize, int n_in, int& lo) {
  lo = bounds[2 * o];
  const int n = bounds[2 * o + 1];
  return (lo >= 0 && n >= 0 && n <= ksize && lo <= n_in - n) ? n : 0;
}
