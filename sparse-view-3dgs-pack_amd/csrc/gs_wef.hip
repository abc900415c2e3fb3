// gs_wef.hip - LGDWT-GS's Wavelet Error Field, its heatmap grid and the Charbonnier loss (gfx950, wave64):
//   LGDWT-GS/utils/loss_utils.py:156-221,284-329   compute_wef_maps / compute_wef_all_subbands
//   LGDWT-GS/utils/loss_utils.py:223-282           make_heatmap_rgb / make_wef_grid_image(_titled)
//   LGDWT-GS/utils/loss_utils.py:98-101            charbonnier_loss
// The reference runs two DWTs of the residual, then multiply, mean, interpolate, amin, amax, subtract, add and divide per map:
// about a hundred small launches for the all-band form.  Here a call is six launches:
//
//   wef_energy_kernel   one thread per level-2 coefficient = one 4 x 4 pixel block of pred and gt: residual, level-1 Haar bands,
//                       level-2 bands of LL1 (haar_block and the repeat-last-sample rule of dwt_fwd_kernel, at both levels),
//                       e = mean_c(scale * b_c^2) in the reference's order (square, scale, channel sum c = 0..C-1, divide by C).
//                       Writes four quarter-resolution planes and (all bands) four half-resolution ones
//   wef_bounds_kernel   the bilinear upsample of every requested plane evaluated on the fly (bilin_sample, gs_haar.h, with exact
//                       weights where the neighbour is clamped onto the sample: a plane of one coefficient stays constant, and
//                       its map is 0 / (0 + 1e-8f) = 0); per-workgroup minimum and maximum per map, NaN-propagating as torch's
//                       amin / amax
//   wef_combine_kernel  one workgroup: the partials of each map -> (min, max)
//   wef_maps_kernel     the upsample again, n = (u - min) / (max - min + 1e-8f) per map -> out[k]; the combined field
//                       (n_LL2 + n_LH2 + n_HL2) / 3 or (the eight in band order) / 8 -> out[K], and its own min / max partials
//   wef_combine_kernel  the combined field's (min, max)
//   wef_norm_kernel     the combined field normalised in place
//
// Minimum and maximum are order-free, so the partials may be combined in any grouping: the same bits on every run.  No float is
// added atomically (nothing is added across threads at all), nothing synchronises with the host.
// Every operation rounds on its own (-ffp-contract=off; divisions and the square root are the correctly rounded ones).
#include "gs_common.h"
#include "gs_haar.h"
#include "gs_launch.h"

namespace {

constexpr int WEF_NB = 1024;        // most workgroups of the two image passes (they stride): bounds the partials
constexpr int WEF_MAXK = 8;
constexpr int CH_NB = 1024;         // most workgroups of the Charbonnier forward

struct WefView {
  float* quarter[4];  // LL2, LH2, HL2, HH2   [h2 * w2]
  float* half[4];     // LL1, LH1, HL1, HH1   [h1 * w1] (all bands)
  float* part;        // [WEF_MAXK][WEF_NB][2]
  float* part_c;      // [WEF_NB][2]
  float* bounds;      // [WEF_MAXK + 1][2]
};
struct WefDims {
  int H, W, h1, w1, h2, w2;
};
inline WefDims wef_dims(int H, int W) {
  WefDims d;
  d.H = H; d.W = W;
  d.h1 = (H + 1) >> 1; d.w1 = (W + 1) >> 1;
  d.h2 = (d.h1 + 1) >> 1; d.w2 = (d.w1 + 1) >> 1;
  return d;
}
inline size_t wef_bytes(const WefDims& d, int all) {
  size_t b = 4 * gs_align(4 * (size_t)d.h2 * d.w2);
  if (all) b += 4 * gs_align(4 * (size_t)d.h1 * d.w1);
  return b + gs_align(4 * 2 * WEF_MAXK * WEF_NB) + gs_align(4 * 2 * WEF_NB) + gs_align(4 * 2 * (WEF_MAXK + 1));
}
inline WefView wef_view(void* tmp, const WefDims& d, int all) {
  char* p = (char*)tmp;
  WefView v;
  for (int k = 0; k < 4; k++) { v.quarter[k] = (float*)p; p += gs_align(4 * (size_t)d.h2 * d.w2); }
  for (int k = 0; k < 4; k++) {
    v.half[k] = all ? (float*)p : nullptr;
    if (all) p += gs_align(4 * (size_t)d.h1 * d.w1);
  }
  v.part = (float*)p; p += gs_align(4 * 2 * WEF_MAXK * WEF_NB);
  v.part_c = (float*)p; p += gs_align(4 * 2 * WEF_NB);
  v.bounds = (float*)p;
  return v;
}
inline bool wef_shape_ok(int32_t C, int32_t H, int32_t W, int32_t bands) {
  return C >= 1 && C <= 4 && H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31) &&
         (bands == GS_WEF_LEVEL2 || bands == GS_WEF_ALL);
}

// torch's amin / amax return NaN as soon as one element is NaN; fminf / fmaxf return the other operand
__device__ __forceinline__ float wef_min(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
__device__ __forceinline__ float wef_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// the workgroup's minimum / maximum of N pairs -> out[k * stride2 + 2 * workgroup + (0, 1)]
template <int N>
__device__ __forceinline__ void wef_block_minmax(float (&lo)[N], float (&hi)[N], float* __restrict__ out, int64_t stride2) {
  __shared__ float red[GS_BLOCK / 64][N][2];
#pragma unroll
  for (int k = 0; k < N; k++) {
    float a = lo[k], b = hi[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a = wef_min(a, __shfl_xor(a, off, 64));
      b = wef_max(b, __shfl_xor(b, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][k][0] = a; red[threadIdx.x >> 6][k][1] = b; }
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    float a = red[0][k][0], b = red[0][k][1];
    for (int w = 1; w < GS_BLOCK / 64; w++) { a = wef_min(a, red[w][k][0]); b = wef_max(b, red[w][k][1]); }
    out[(int64_t)k * stride2 + 2 * blockIdx.x] = a;       // [k][workgroup][2]
    out[(int64_t)k * stride2 + 2 * blockIdx.x + 1] = b;
  }
}

// ------------------------------------------------------------------------------------------------ energies
struct WefPlanesOut {
  float* quarter[4];
  float* half[4];
};
__global__ void __launch_bounds__(GS_BLOCK) wef_energy_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int C,
                                                              WefDims d, int all, int vec, WefPlanesOut out) {
  const int64_t o = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (o >= (int64_t)d.h2 * d.w2) return;
  const int j2 = (int)(o % d.w2), i2 = (int)(o / d.w2);
  const size_t plane = (size_t)d.H * d.W;
  float s1[4][2][2], s2[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    s2[k] = 0.f;
#pragma unroll
    for (int r = 0; r < 2; r++) s1[k][r][0] = s1[k][r][1] = 0.f;
  }
  for (int c = 0; c < C; c++) {
    const float* p = pred + c * plane;
    const float* g = gt + c * plane;
    float ll[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int i1 = min(2 * i2 + r, d.h1 - 1);              // (level 2 repeats the last row of LL1)
      const int ys[2] = {2 * i1, min(2 * i1 + 1, d.H - 1)};  // (level 1 repeats the last pixel row)
      float res[2][4];
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const size_t row = (size_t)ys[t] * d.W;
        if (vec) {  // W % 4 == 0 and 16-byte aligned images: the block's four columns exist and are one load
          const float4 a = *reinterpret_cast<const float4*>(p + row + 4 * (size_t)j2);
          const float4 b = *reinterpret_cast<const float4*>(g + row + 4 * (size_t)j2);
          res[t][0] = a.x - b.x; res[t][1] = a.y - b.y; res[t][2] = a.z - b.z; res[t][3] = a.w - b.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int j1 = min(2 * j2 + (k >> 1), d.w1 - 1);
            const int x = (k & 1) ? min(2 * j1 + 1, d.W - 1) : 2 * j1;
            res[t][k] = p[row + x] - g[row + x];
          }
        }
      }
#pragma unroll
      for (int cc = 0; cc < 2; cc++) {
        const Bands b = haar_block(res[0][2 * cc], res[0][2 * cc + 1], res[1][2 * cc], res[1][2 * cc + 1]);
        ll[r][cc] = b.ll;
        s1[0][r][cc] += b.ll * b.ll * 1.0f;
        s1[1][r][cc] += b.lh * b.lh * 1.0f;
        s1[2][r][cc] += b.hl * b.hl * 1.0f;
        s1[3][r][cc] += b.hh * b.hh * 1.0f;
      }
    }
    const Bands b2 = haar_block(ll[0][0], ll[0][1], ll[1][0], ll[1][1]);
    s2[0] += b2.ll * b2.ll * 4.0f;
    s2[1] += b2.lh * b2.lh * 2.0f;
    s2[2] += b2.hl * b2.hl * 2.0f;
    s2[3] += b2.hh * b2.hh * 2.0f;
  }
  const float fc = (float)C;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (out.quarter[k]) out.quarter[k][o] = __fdiv_rn(s2[k], fc);
  if (!all) return;
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int cc = 0; cc < 2; cc++) {
      const int i1 = 2 * i2 + r, j1 = 2 * j2 + cc;
      if (i1 >= d.h1 || j1 >= d.w1) continue;  // a repeated sample of level 2: no coefficient of level 1
#pragma unroll
      for (int k = 0; k < 4; k++) out.half[k][(size_t)i1 * d.w1 + j1] = __fdiv_rn(s1[k][r][cc], fc);
    }
}

// ------------------------------------------------------------------------------------------------ bounds and maps
// the requested planes in output order: all bands = four half-resolution planes then four quarter-resolution ones
struct WefPlanes {
  const float* p[WEF_MAXK];
};
template <bool ALL>
struct WefTaps {
  BilinTap qy, qx, hy, hx;
  __device__ __forceinline__ WefTaps(int y, int x, const WefDims& d) {
    qy = bilin_tap<true>(y, d.h2, d.H);
    qx = bilin_tap<true>(x, d.w2, d.W);
    if (ALL) { hy = bilin_tap<true>(y, d.h1, d.H); hx = bilin_tap<true>(x, d.w1, d.W); }
  }
  __device__ __forceinline__ float sample(const WefPlanes& pl, int k, const WefDims& d) const {
    if (ALL && k < 4) return bilin_sample(pl.p[k], d.w1, hy, hx);
    return bilin_sample(pl.p[k], d.w2, qy, qx);
  }
};

template <bool ALL>
__global__ void __launch_bounds__(GS_BLOCK) wef_bounds_kernel(WefPlanes pl, WefDims d, float* __restrict__ part) {
  constexpr int K = ALL ? 8 : 3;
  float lo[K], hi[K];
#pragma unroll
  for (int k = 0; k < K; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
  const int64_t n = (int64_t)d.H * d.W;
  for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_BLOCK) {
    const WefTaps<ALL> t((int)(i / d.W), (int)(i % d.W), d);
#pragma unroll
    for (int k = 0; k < K; k++) {
      const float u = t.sample(pl, k, d);
      lo[k] = wef_min(lo[k], u);
      hi[k] = wef_max(hi[k], u);
    }
  }
  wef_block_minmax<K>(lo, hi, part, 2 * (int64_t)WEF_NB);
}

// one workgroup: bounds[k] = (min, max) over part[k][0 .. nb), k < K
__global__ void __launch_bounds__(GS_BLOCK) wef_combine_kernel(const float* __restrict__ part, int nb, int K,
                                                               float* __restrict__ bounds, float* __restrict__ out_bounds) {
  __shared__ float red[GS_BLOCK / 64][2];
  for (int k = 0; k < K; k++) {
    const float* q = part + (size_t)k * 2 * WEF_NB;
    float a = INFINITY, b = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += GS_BLOCK) { a = wef_min(a, q[2 * i]); b = wef_max(b, q[2 * i + 1]); }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a = wef_min(a, __shfl_xor(a, off, 64));
      b = wef_max(b, __shfl_xor(b, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < GS_BLOCK / 64; w++) { a = wef_min(a, red[w][0]); b = wef_max(b, red[w][1]); }
      bounds[2 * k] = a;
      bounds[2 * k + 1] = b;
      if (out_bounds) { out_bounds[2 * k] = a; out_bounds[2 * k + 1] = b; }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ float wef_normalise(float u, float mn, float mx) {
  return __fdiv_rn(u - mn, (mx - mn) + 1e-8f);
}

template <bool ALL>
__global__ void __launch_bounds__(GS_BLOCK) wef_maps_kernel(WefPlanes pl, WefDims d, const float* __restrict__ bounds,
                                                            float* __restrict__ out, float* __restrict__ part_c) {
  constexpr int K = ALL ? 8 : 3;
  float mn[K], mx[K];
#pragma unroll
  for (int k = 0; k < K; k++) { mn[k] = bounds[2 * k]; mx[k] = bounds[2 * k + 1]; }
  float lo[1] = {INFINITY}, hi[1] = {-INFINITY};
  const int64_t n = (int64_t)d.H * d.W;
  for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_BLOCK) {
    const WefTaps<ALL> t((int)(i / d.W), (int)(i % d.W), d);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const float v = wef_normalise(t.sample(pl, k, d), mn[k], mx[k]);
      out[(size_t)k * n + i] = v;
      acc = k == 0 ? v : acc + v;
    }
    const float comb = __fdiv_rn(acc, ALL ? 8.0f : 3.0f);
    out[(size_t)K * n + i] = comb;
    lo[0] = wef_min(lo[0], comb);
    hi[0] = wef_max(hi[0], comb);
  }
  wef_block_minmax<1>(lo, hi, part_c, 0);
}

__global__ void __launch_bounds__(GS_BLOCK) wef_norm_kernel(float* __restrict__ x, int64_t n, const float* __restrict__ b) {
  const float mn = b[0], mx = b[1];
  for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_BLOCK)
    x[i] = wef_normalise(x[i], mn, mx);
}

// ------------------------------------------------------------------------------------------------ heatmap grid
__device__ __forceinline__ uint8_t wef_byte(float c) { return (uint8_t)(int)(c * 255.0f); }  // c in [0, 1]: truncation

__global__ void __launch_bounds__(GS_BLOCK) wef_grid_kernel(const float* __restrict__ maps, int K_total, int H, int W,
                                                            const int32_t* __restrict__ order, int n_keys, int cols, int rows,
                                                            const uint8_t* __restrict__ labels, uint8_t* __restrict__ out) {
  const int64_t GW = (int64_t)cols * W, total = GW * rows * H;
  const int64_t o = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (o >= total) return;
  const int64_t X = o % GW, Y = o / GW;
  uint8_t r = 0, g = 0, b = 0;
  const int tc = (int)(X / W), tr = (int)(Y / H);
  const int64_t idx = (int64_t)tr * cols + tc;
  if (idx < n_keys) {
    const int m = order[idx];
    if (m >= 0 && m < K_total) {
      const float v = maps[((size_t)m * H + (size_t)(Y - (int64_t)tr * H)) * W + (size_t)(X - (int64_t)tc * W)];
      const float x = fminf(fmaxf(v, 0.f), 1.f);  // (NaN -> 0)
      r = wef_byte(x);
      g = wef_byte(fminf(fmaxf(1.0f - fabsf(x - 0.5f) * 2.0f, 0.f), 1.f));
      b = wef_byte(1.0f - x);
    }
  }
  if (labels) {
    // the boxes are drawn in key order, each over everything before it, and may reach into the neighbouring tiles of a small
    // image: the last key whose box holds the pixel owns it
    for (int k = n_keys - 1; k >= 0; k--) {
      const int64_t bx = X - (int64_t)(k % cols) * W, by = Y - (int64_t)(k / cols) * H;
      if (bx >= 0 && bx < GS_WEF_LABEL_W && by >= 0 && by < GS_WEF_LABEL_H) {
        r = g = b = labels[((size_t)k * GS_WEF_LABEL_H + (size_t)by) * GS_WEF_LABEL_W + (size_t)bx] ? 255 : 0;
        break;
      }
    }
  }
  out[3 * o] = r; out[3 * o + 1] = g; out[3 * o + 2] = b;
}

// ------------------------------------------------------------------------------------------------ Charbonnier
// the terms are the reference's fp32 statements; their sum is float64 in a fixed order: a thread's strided terms, the wave's
// shuffle tree, the waves in index order, the workgroups' partials by ch_combine_kernel
__global__ void __launch_bounds__(GS_BLOCK) ch_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          int64_t n, float eps2, double* __restrict__ part) {
  __shared__ double red[GS_BLOCK / 64];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_BLOCK) {
    const float dd = pred[i] - target[i];
    acc += (double)__fsqrt_rn(dd * dd + eps2);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < GS_BLOCK / 64; w++) t += red[w];
    part[blockIdx.x] = t;
  }
}
__global__ void __launch_bounds__(GS_BLOCK) ch_combine_kernel(const double* __restrict__ part, int nb, int64_t n,
                                                              float* __restrict__ out) {
  __shared__ double red[GS_BLOCK / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += GS_BLOCK) acc += part[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < GS_BLOCK / 64; w++) t += red[w];
    out[0] = (float)(t / (double)n);  // rounded once
  }
}
// d/dpred mean(sqrt(d^2 + eps^2)) = g d / s / n, evaluated in double from the fp32 inputs and rounded once
__global__ void __launch_bounds__(GS_BLOCK) ch_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          int64_t n, double eps2, const float* __restrict__ grad_out,
                                                          float* __restrict__ d_pred, float* __restrict__ d_target) {
  const double g = (double)grad_out[0], dn = (double)n;
  for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_BLOCK) {
    const double dd = (double)pred[i] - (double)target[i];
    const float v = (float)(g * dd / sqrt(dd * dd + eps2) / dn);
    if (d_pred) d_pred[i] = v;
    if (d_target) d_target[i] = -v;
  }
}

}  // namespace

extern "C" {

size_t gs_wef_tmp_bytes(int32_t C, int32_t H, int32_t W, int32_t bands) {
  if (!wef_shape_ok(C, H, W, bands)) return 0;
  return wef_bytes(wef_dims(H, W), bands == GS_WEF_ALL);
}

int gs_wef_maps(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W, int32_t bands, void* tmp, size_t tmp_bytes,
                float* out_maps, float* out_bounds, void* stream) {
  if (!wef_shape_ok(C, H, W, bands)) return GS_E_SHAPE;
  if (!pred || !gt || !tmp || !out_maps) return GS_E_NULL;
  const int all = bands == GS_WEF_ALL;
  const WefDims d = wef_dims(H, W);
  if (tmp_bytes < wef_bytes(d, all)) return GS_E_SHAPE;
  if (((uintptr_t)tmp & 255) || ((uintptr_t)pred & 3) || ((uintptr_t)gt & 3) || ((uintptr_t)out_maps & 3) ||
      ((uintptr_t)out_bounds & 3))
    return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const WefView v = wef_view(tmp, d, all);
  const int K = all ? 8 : 3;
  const int64_t n = (int64_t)H * W;

  WefPlanesOut po;
  for (int k = 0; k < 4; k++) { po.quarter[k] = (all || k < 3) ? v.quarter[k] : nullptr; po.half[k] = v.half[k]; }
  const int vec = (W % 4 == 0 && ((uintptr_t)pred & 15) == 0 && ((uintptr_t)gt & 15) == 0) ? 1 : 0;
  const int64_t n2 = (int64_t)d.h2 * d.w2;
  hipLaunchKernelGGL(wef_energy_kernel, dim3((unsigned)((n2 + GS_BLOCK - 1) / GS_BLOCK)), dim3(GS_BLOCK), 0, s, pred, gt, (int)C, d,
                     all, vec, po);
  GS_LAUNCH_CHECK(s, 0);

  WefPlanes pl;
  for (int k = 0; k < WEF_MAXK; k++) pl.p[k] = nullptr;
  if (all) {
    for (int k = 0; k < 4; k++) { pl.p[k] = v.half[k]; pl.p[4 + k] = v.quarter[k]; }
  } else {
    for (int k = 0; k < 3; k++) pl.p[k] = v.quarter[k];
  }
  const unsigned nb = (unsigned)gs_capped_blocks((size_t)n, GS_BLOCK, WEF_NB);
  if (all) hipLaunchKernelGGL(wef_bounds_kernel<true>, dim3(nb), dim3(GS_BLOCK), 0, s, pl, d, v.part);
  else hipLaunchKernelGGL(wef_bounds_kernel<false>, dim3(nb), dim3(GS_BLOCK), 0, s, pl, d, v.part);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(wef_combine_kernel, dim3(1), dim3(GS_BLOCK), 0, s, (const float*)v.part, (int)nb, K, v.bounds, out_bounds);
  GS_LAUNCH_CHECK(s, 0);
  if (all) hipLaunchKernelGGL(wef_maps_kernel<true>, dim3(nb), dim3(GS_BLOCK), 0, s, pl, d, (const float*)v.bounds, out_maps, v.part_c);
  else hipLaunchKernelGGL(wef_maps_kernel<false>, dim3(nb), dim3(GS_BLOCK), 0, s, pl, d, (const float*)v.bounds, out_maps, v.part_c);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(wef_combine_kernel, dim3(1), dim3(GS_BLOCK), 0, s, (const float*)v.part_c, (int)nb, 1, v.bounds + 2 * K,
                     out_bounds ? out_bounds + 2 * K : nullptr);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(wef_norm_kernel, dim3(nb), dim3(GS_BLOCK), 0, s, out_maps + (size_t)K * n, n, (const float*)(v.bounds + 2 * K));
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_wef_grid(const float* maps, int32_t K_total, int32_t H, int32_t W, const int32_t* order, int32_t n_keys, int32_t tile_cols,
                const uint8_t* labels, uint8_t* out_u8, void* stream) {
  if (K_total < 1 || H < 1 || W < 1 || n_keys < 1 || tile_cols < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return GS_E_SHAPE;
  if (!maps || !order || !out_u8) return GS_E_NULL;
  if (((uintptr_t)maps & 3) || ((uintptr_t)order & 3)) return GS_E_SHAPE;
  const int rows = (n_keys + tile_cols - 1) / tile_cols;
  const int64_t total = (int64_t)rows * H * tile_cols * W;
  const int64_t blocks = (total + GS_BLOCK - 1) / GS_BLOCK;
  if (blocks >= ((int64_t)1 << 31)) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(wef_grid_kernel, dim3((unsigned)blocks), dim3(GS_BLOCK), 0, s, maps, (int)K_total, (int)H, (int)W, order,
                     (int)n_keys, (int)tile_cols, rows, labels, out_u8);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

size_t gs_charbonnier_tmp_bytes(int64_t n) {
  if (n < 1) return 0;
  return gs_align(sizeof(double) * CH_NB);
}

int gs_charbonnier_fwd(const float* pred, const float* target, int64_t n, double epsilon, void* tmp, size_t tmp_bytes, float* out,
                       void* stream) {
  if (n < 1) return GS_E_SHAPE;
  if (!pred || !target || !tmp || !out) return GS_E_NULL;
  if (tmp_bytes < gs_align(sizeof(double) * CH_NB) || ((uintptr_t)tmp & 255) || ((uintptr_t)pred & 3) || ((uintptr_t)target & 3) ||
      ((uintptr_t)out & 3))
    return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (unsigned)gs_capped_blocks((size_t)n, GS_BLOCK, CH_NB);
  const float eps2 = (float)(epsilon * epsilon);  // the reference adds the Python float epsilon * epsilon to an fp32 tensor
  hipLaunchKernelGGL(ch_fwd_kernel, dim3(nb), dim3(GS_BLOCK), 0, s, pred, target, n, eps2, (double*)tmp);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(ch_combine_kernel, dim3(1), dim3(GS_BLOCK), 0, s, (const double*)tmp, (int)nb, n, out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_charbonnier_bwd(const float* pred, const float* target, int64_t n, double epsilon, const float* grad_out, float* d_pred,
                       float* d_target, void* stream) {
  if (n < 1) return GS_E_SHAPE;
  if (!pred || !target || !grad_out || (!d_pred && !d_target)) return GS_E_NULL;
  if (((uintptr_t)pred & 3) || ((uintptr_t)target & 3) || ((uintptr_t)grad_out & 3) || ((uintptr_t)d_pred & 3) ||
      ((uintptr_t)d_target & 3))
    return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ch_bwd_kernel, dim3((unsigned)gs_capped_blocks((size_t)n, GS_BLOCK, 4096)), dim3(GS_BLOCK), 0, s, pred, target, n, epsilon * epsilon, grad_out,
                     d_pred, d_target);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
