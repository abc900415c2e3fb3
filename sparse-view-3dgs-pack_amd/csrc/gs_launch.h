// gs_launch.h - what the small-kernel files' entries and four-per-lane kernels share: the 16-byte alignment test, the capped
// grid size, the guarded four-float access.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static inline bool gs_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ceil(n / chunk) workgroups, at most cap, and at most max_blocks where the caller caps it (0: no cap).  n == 0 gives 0.
static inline int gs_capped_blocks(size_t n, size_t chunk, size_t cap, int max_blocks = 0) {
  size_t b = (n + chunk - 1) / chunk;
  if (b > cap) b = cap;
  if (max_blocks > 0 && b > (size_t)max_blocks) b = (size_t)max_blocks;
  return (int)b;
}

__device__ __forceinline__ void gs_unpack4(const float4 q, float* v) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }

// elements [i, i + 4) of p (i a multiple of 4) -> v, one 16-byte load where vec (p is 16-byte aligned) and all four exist;
// the ones at or beyond n are left alone
__device__ __forceinline__ void gs_load4(const float* p, size_t i, size_t n, int vec, float (&v)[4]) {
  if (vec && i + 4 <= n) {
    gs_unpack4(*reinterpret_cast<const float4*>(p + i), v);
  } else {
    for (int k = 0; k < 4; k++)
      if (i + k < n) v[k] = p[i + k];
  }
}

__device__ __forceinline__ void gs_store4(float* p, size_t i, size_t n, int vec, const float (&v)[4]) {
  if (vec && i + 4 <= n) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4; k++)
      if (i + k < n) p[i + k] = v[k];
  }
}
