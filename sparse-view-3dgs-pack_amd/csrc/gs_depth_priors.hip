// gs_depth_priors.hip - depth priors from files, on the device (gfx950, wave64):
//   gaussian-splatting/utils/make_depth_scale.py:8-64   the per-image scale / offset of depth_params.json  (gs_depth_scales)
//   gaussian-splatting/scene/cameras.py:60-78           the camera's inverse-depth map and its mask plane   (gs_invdepth_prepare)
//
// depth_scales_kernel: one launch for every image, one workgroup per image's observation segment.
//   phase A  each lane walks the segment GS_BLOCK apart: the id test against the dense point table, view-space z and 1 / z in
//            double (one rounding per operation: the file is compiled with -ffp-contract=off and spells the operations out),
//            the map coordinate in fp32, the five validity tests, the bilinear sample of the mono map under the stated
//            sub-pixel rule.  inv, mono and the validity word go to scratch; the workgroup reduces the count of valid
//            observations and max / min of inv over the USED ones (NaN-propagating, as np.max / np.min)
//   gate     n_valid > 10 and max - min > 1e-3, else zeros
//   phase B  the medians by radix SELECT over the scratch: 8 bits per pass from the top, an LDS histogram [256] of integer
//            counts, a workgroup scan, the digit that holds the wanted rank becomes the next byte of the prefix.  Doubles go
//            through 64-bit monotone keys (8 passes), floats through 32-bit ones (4 passes).  An even count selects both
//            middle ranks (two selects) and takes (a + b) / 2 in the sequence's own precision, as np.median's mean of two does
//   phase C  sum |inv - t_colmap| and sum |mono - t_mono| (the difference rounded to fp32 first, as numpy's float32 array is) in
//            double: a lane's strided partial in index order, a shuffle tree over the wave, the four waves ((0 + 1) + (2 + 3))
// No float atomics, nothing depends on arrival order, nothing synchronises with the host: the same bits on every run.
// The select is a copy of gs_depth_vis.hip's idea specialised to one workgroup per segment (that one narrows four ranks over a
// whole image across launches).
#include "gs_common.h"

namespace {

constexpr int DP_MAX_DIM = 1 << 20;      // rows / columns of a mono map
constexpr int IP_MAX_DIM = 1 << 15;      // rows / columns either side of gs_invdepth_prepare
constexpr int DP_MAX_COORD_BITS = 10;
static_assert(GS_BLOCK == 256, "one thread per digit in the select's scan");

struct DpView {
  double* inv;      // [n_obs] 1 / z
  float* mono;      // [n_obs] the sampled map
  uint32_t* valid;  // [n_obs] 1 = the observation takes part in the fit
};
inline size_t dp_bytes(int64_t n_obs) {
  const size_t n = n_obs > 0 ? (size_t)n_obs : 1;
  return gs_align(8 * n) + gs_align(4 * n) + gs_align(4 * n);
}
inline __host__ __device__ DpView dp_view(void* tmp, int64_t n_obs) {
  const size_t n = n_obs > 0 ? (size_t)n_obs : 1;
  char* p = (char*)tmp;
  DpView v;
  v.inv = (double*)p; p += gs_align(8 * n);
  v.mono = (float*)p; p += gs_align(4 * n);
  v.valid = (uint32_t*)p;
  return v;
}

__device__ __forceinline__ uint64_t dp_key64(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dp_value64(uint64_t key) {
  return __longlong_as_double((long long)((key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key));
}
__device__ __forceinline__ uint32_t dp_key32(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dp_value32(uint32_t key) {
  return __uint_as_float((key >> 31) ? (key & 0x7FFFFFFFu) : ~key);
}

__device__ __forceinline__ float dp_texel(const void* map, int dtype, int w, int y, int x) {
  const int64_t i = (int64_t)y * w + x;
  const float v = dtype == GS_DEPTH_MAP_U16 ? (float)((const uint16_t*)map)[i] : ((const float*)map)[i];
  return __fmul_rn(v, 1.52587890625e-05f);  // / 65536: a power of two, the same rounding as the division
}

// one coordinate -> (cell, fraction) under the sub-pixel rule
__device__ __forceinline__ void dp_cell(float x, int bits, int64_t& cell, float& f) {
  if (bits >= 0) {
    const float q = (float)(1 << bits);
    const int64_t i = (int64_t)llrintf(__fmul_rn(x, q));  // half-to-even
    cell = i >> bits;
    f = __fdiv_rn((float)(i & (int64_t)((1 << bits) - 1)), q);
  } else {
    const float fl = floorf(x);
    cell = (int64_t)fl;
    f = __fsub_rn(x, fl);
  }
}

__device__ float dp_sample(const void* map, int dtype, int h, int w, float x, float y, int bits) {
  int64_t cx, cy;
  float fx, fy;
  dp_cell(x, bits, cx, fx);
  dp_cell(y, bits, cy, fy);
  const int x0 = (int)min(max(cx, (int64_t)0), (int64_t)(w - 1)), x1 = (int)min(max(cx + 1, (int64_t)0), (int64_t)(w - 1));
  const int y0 = (int)min(max(cy, (int64_t)0), (int64_t)(h - 1)), y1 = (int)min(max(cy + 1, (int64_t)0), (int64_t)(h - 1));
  const float gx = __fsub_rn(1.0f, fx), gy = __fsub_rn(1.0f, fy);
  const float w00 = __fmul_rn(gy, gx), w01 = __fmul_rn(gy, fx), w10 = __fmul_rn(fy, gx), w11 = __fmul_rn(fy, fx);
  float acc = __fmul_rn(w00, dp_texel(map, dtype, w, y0, x0));
  acc = __fadd_rn(acc, __fmul_rn(w01, dp_texel(map, dtype, w, y0, x1)));
  acc = __fadd_rn(acc, __fmul_rn(w10, dp_texel(map, dtype, w, y1, x0)));
  acc = __fadd_rn(acc, __fmul_rn(w11, dp_texel(map, dtype, w, y1, x1)));
  return acc;
}

struct DpShared {
  uint32_t hist[256];
  uint32_t wsum[GS_BLOCK / 64];
  uint64_t prefix;
  uint32_t rank;
  uint32_t cnt[GS_BLOCK / 64], bad[GS_BLOCK / 64];
  double hi[GS_BLOCK / 64], lo[GS_BLOCK / 64];
  double sum_c[GS_BLOCK / 64], sum_m[GS_BLOCK / 64];
};

// the key at 0-based sorted position `rank` among the segment's valid entries; every thread of the workgroup calls it
template <bool WIDE>
__device__ uint64_t dp_select(const DpView& v, int64_t beg, int64_t end, uint32_t rank, DpShared& sh) {
  constexpr int PASSES = WIDE ? 8 : 4;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint64_t prefix = 0;
  if (t == 0) { sh.prefix = 0; sh.rank = 0; }
  for (int pass = 0; pass < PASSES; pass++) {
    const int shift = 8 * (PASSES - 1 - pass);
    sh.hist[t] = 0u;
    __syncthreads();
    for (int64_t k = beg + t; k < end; k += GS_BLOCK) {
      if (!v.valid[k]) continue;
      const uint64_t key = WIDE ? dp_key64(v.inv[k]) : (uint64_t)dp_key32(v.mono[k]);
      const uint64_t high = pass == 0 ? 0ull : (key >> (shift + 8));
      if (high == prefix) atomicAdd(&sh.hist[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = sh.hist[t];
    uint32_t inc = c;  // inclusive scan over the wave, then over the four waves
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    if (lane == 63) sh.wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += sh.wsum[w];
    const uint32_t ex = before + inc - c;
    if (rank >= ex && rank < ex + c) {  // true for exactly one digit (rank < the count under the prefix)
      sh.prefix = (prefix << 8) | (uint64_t)t;
      sh.rank = rank - ex;
    }
    __syncthreads();
    prefix = sh.prefix;
    rank = sh.rank;
    __syncthreads();
  }
  return prefix;
}

__global__ void __launch_bounds__(GS_BLOCK) depth_scales_kernel(const double* __restrict__ points, int64_t n_table,
                                                                const int64_t* __restrict__ obs_ids,
                                                                const double* __restrict__ obs_xy, int64_t n_obs,
                                                                const int64_t* __restrict__ seg, const double* __restrict__ cams,
                                                                const void* const* __restrict__ maps,
                                                                const int32_t* __restrict__ map_hw, int dtype, int bits, DpView v,
                                                                double* __restrict__ out) {
  __shared__ DpShared sh;
  const int img = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int64_t beg = seg[img], end = seg[img + 1];
  beg = beg < 0 ? 0 : (beg > n_obs ? n_obs : beg);
  end = end < beg ? beg : (end > n_obs ? n_obs : end);
  const double* c = cams + 8 * (size_t)img;
  const double r20 = c[0], r21 = c[1], r22 = c[2], t2 = c[3], s = c[4];
  const float wlim = (float)c[5], hlim = (float)c[6];
  const int h = map_hw[2 * img], w = map_hw[2 * img + 1];
  const void* map = maps[img];
  double* o = out + 8 * (size_t)img;
  if (h < 1 || w < 1 || h > DP_MAX_DIM || w > DP_MAX_DIM || map == nullptr) {  // (uniform) nothing to sample: the zero answer
    if (t < 8) o[t] = 0.0;
    return;
  }

  // ---- phase A
  uint32_t cnt = 0, bad = 0;
  double hi = -INFINITY, lo = INFINITY;
  for (int64_t k = beg + t; k < end; k += GS_BLOCK) {
    const int64_t id = obs_ids[k];
    uint32_t ok = 0;
    double inv = 0.0;
    float mono = 0.0f;
    if (id >= 0 && id < n_table) {
      const double X = points[3 * id], Y = points[3 * id + 1], Z = points[3 * id + 2];
      const double z = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(X, r20), __dmul_rn(Y, r21)), __dmul_rn(Z, r22)), t2);
      inv = __ddiv_rn(1.0, z);
      if (inv != inv) bad = 1u;
      else { hi = fmax(hi, inv); lo = fmin(lo, inv); }
      const float mx = (float)__dmul_rn(obs_xy[2 * k], s), my = (float)__dmul_rn(obs_xy[2 * k + 1], s);
      if (mx >= 0.0f && my >= 0.0f && mx < wlim && my < hlim && inv > 0.0) {
        ok = 1u;
        mono = dp_sample(map, dtype, h, w, mx, my, bits);
      }
    }
    v.inv[k] = inv;
    v.mono[k] = mono;
    v.valid[k] = ok;
    cnt += ok;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    cnt += __shfl_down(cnt, off, 64);
    bad |= __shfl_down(bad, off, 64);
    hi = fmax(hi, __shfl_down(hi, off, 64));
    lo = fmin(lo, __shfl_down(lo, off, 64));
  }
  if (lane == 0) { sh.cnt[wave] = cnt; sh.bad[wave] = bad; sh.hi[wave] = hi; sh.lo[wave] = lo; }
  __syncthreads();  // (also orders the scratch stores before the select's loads: one workgroup, one CU)
  const uint32_t n = sh.cnt[0] + sh.cnt[1] + sh.cnt[2] + sh.cnt[3];
  hi = fmax(fmax(sh.hi[0], sh.hi[1]), fmax(sh.hi[2], sh.hi[3]));
  lo = fmin(fmin(sh.lo[0], sh.lo[1]), fmin(sh.lo[2], sh.lo[3]));
  const double range = (sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3]) ? (double)__uint_as_float(0x7FC00000u) : __dsub_rn(hi, lo);
  if (!(n > 10u && range > 1e-3)) {  // (uniform)
    if (t < 8) o[t] = t == 2 ? (double)n : (t == 7 ? range : 0.0);
    return;
  }

  // ---- phase B
  const uint32_t k0 = (n - 1u) >> 1, k1 = n >> 1;
  const uint64_t ca = dp_select<true>(v, beg, end, k0, sh);
  const uint64_t cb = k1 != k0 ? dp_select<true>(v, beg, end, k1, sh) : ca;
  const uint32_t ma = (uint32_t)dp_select<false>(v, beg, end, k0, sh);
  const uint32_t mb = k1 != k0 ? (uint32_t)dp_select<false>(v, beg, end, k1, sh) : ma;
  const double t_c = k1 != k0 ? __ddiv_rn(__dadd_rn(dp_value64(ca), dp_value64(cb)), 2.0) : dp_value64(ca);
  const float t_m = k1 != k0 ? __fdiv_rn(__fadd_rn(dp_value32(ma), dp_value32(mb)), 2.0f) : dp_value32(ma);

  // ---- phase C
  double pc = 0.0, pm = 0.0;
  for (int64_t k = beg + t; k < end; k += GS_BLOCK) {
    if (!v.valid[k]) continue;
    pc = __dadd_rn(pc, fabs(__dsub_rn(v.inv[k], t_c)));
    pm = __dadd_rn(pm, (double)fabsf(__fsub_rn(v.mono[k], t_m)));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    pc = __dadd_rn(pc, __shfl_down(pc, off, 64));
    pm = __dadd_rn(pm, __shfl_down(pm, off, 64));
  }
  if (lane == 0) { sh.sum_c[wave] = pc; sh.sum_m[wave] = pm; }
  __syncthreads();
  if (t != 0) return;
  const double s_c = __ddiv_rn(__dadd_rn(__dadd_rn(sh.sum_c[0], sh.sum_c[1]), __dadd_rn(sh.sum_c[2], sh.sum_c[3])), (double)n);
  const double s_m = __ddiv_rn(__dadd_rn(__dadd_rn(sh.sum_m[0], sh.sum_m[1]), __dadd_rn(sh.sum_m[2], sh.sum_m[3])), (double)n);
  const double scale = __ddiv_rn(s_c, s_m);
  o[0] = scale;
  o[1] = __dsub_rn(t_c, __dmul_rn((double)t_m, scale));
  o[2] = (double)n;
  o[3] = t_c;
  o[4] = s_c;
  o[5] = (double)t_m;
  o[6] = s_m;
  o[7] = range;
}

// ---------------------------------------------------------------------------------------------- the camera's map
__device__ __forceinline__ float ip_load(const void* src, int dtype, int64_t i, float divisor) {
  const float v = dtype == GS_DEPTH_MAP_U16 ? (float)((const uint16_t*)src)[i] : ((const float*)src)[i];
  return __fdiv_rn(v, divisor);
}

__device__ __forceinline__ void ip_axis(int d, int n_in, int n_out, int& s0, int& s1, float& a0, float& a1) {
  const double scale = __ddiv_rn((double)n_in, (double)n_out);
  float f = (float)__dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), 0.5);
  const float fl = floorf(f);
  int s = (int)fl;
  f = __fsub_rn(f, fl);
  if (s < 0) { s = 0; f = 0.0f; }
  if (s >= n_in - 1) { s = n_in - 1; f = 0.0f; }
  s0 = s;
  s1 = s + 1 < n_in ? s + 1 : n_in - 1;  // (weight 0 there)
  a0 = __fsub_rn(1.0f, f);
  a1 = f;
}

__global__ void __launch_bounds__(GS_BLOCK) invdepth_prepare_kernel(const void* __restrict__ src, int dtype, int H, int W, int H2,
                                                                    int W2, float divisor, int apply, float scale, float offset,
                                                                    float mask_value, float* __restrict__ out,
                                                                    float* __restrict__ out_mask) {
  const int64_t p = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (p >= (int64_t)H2 * W2) return;
  const int dy = (int)(p / W2), dx = (int)(p % W2);
  float x;
  if (H == H2 && W == W2) {
    x = ip_load(src, dtype, p, divisor);
  } else {
    int x0, x1, y0, y1;
    float a0, a1, b0, b1;
    ip_axis(dx, W, W2, x0, x1, a0, a1);
    ip_axis(dy, H, H2, y0, y1, b0, b1);
    const float top = __fadd_rn(__fmul_rn(a0, ip_load(src, dtype, (int64_t)y0 * W + x0, divisor)),
                                __fmul_rn(a1, ip_load(src, dtype, (int64_t)y0 * W + x1, divisor)));
    const float bot = __fadd_rn(__fmul_rn(a0, ip_load(src, dtype, (int64_t)y1 * W + x0, divisor)),
                                __fmul_rn(a1, ip_load(src, dtype, (int64_t)y1 * W + x1, divisor)));
    x = __fadd_rn(__fmul_rn(b0, top), __fmul_rn(b1, bot));
  }
  if (x < 0.0f) x = 0.0f;
  if (apply) x = __fadd_rn(__fmul_rn(x, scale), offset);
  out[p] = x;
  if (out_mask) out_mask[p] = mask_value;
}

inline bool ip_dim_ok(int32_t n) { return n >= 1 && n <= IP_MAX_DIM; }

}  // namespace

extern "C" {

size_t gs_depth_scales_tmp_bytes(int64_t n_obs) {
  if (n_obs < 0) return 0;
  return dp_bytes(n_obs);
}

int gs_depth_scales(const double* points, int64_t n_table, const int64_t* obs_ids, const double* obs_xy, int64_t n_obs,
                    const int64_t* seg, const double* cams, const void* const* maps, const int32_t* map_hw, int32_t map_dtype,
                    int32_t coord_bits, int32_t n_images, void* tmp, size_t tmp_bytes, double* out, void* stream) {
  if (n_images < 0 || n_obs < 0 || n_table < 0) return GS_E_SHAPE;
  if (map_dtype != GS_DEPTH_MAP_U16 && map_dtype != GS_DEPTH_MAP_F32) return GS_E_SHAPE;
  if (coord_bits > DP_MAX_COORD_BITS) return GS_E_SHAPE;
  if (n_images == 0) return GS_OK;
  if (!seg || !cams || !maps || !map_hw || !tmp || !out) return GS_E_NULL;
  if ((n_obs > 0 && (!obs_ids || !obs_xy)) || (n_table > 0 && !points)) return GS_E_NULL;
  if (tmp_bytes < dp_bytes(n_obs)) return GS_E_SHAPE;
  if (((uintptr_t)tmp & 255) || ((uintptr_t)points & 7) || ((uintptr_t)obs_ids & 7) || ((uintptr_t)obs_xy & 7) ||
      ((uintptr_t)seg & 7) || ((uintptr_t)cams & 7) || ((uintptr_t)maps & 7) || ((uintptr_t)map_hw & 3) || ((uintptr_t)out & 7))
    return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_scales_kernel, dim3((unsigned)n_images), dim3(GS_BLOCK), 0, s, points, n_table, obs_ids, obs_xy, n_obs,
                     seg, cams, maps, map_hw, (int)map_dtype, (int)(coord_bits < 0 ? -1 : coord_bits), dp_view(tmp, n_obs), out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_invdepth_prepare(const void* src, int32_t src_dtype, int32_t H, int32_t W, int32_t H2, int32_t W2, float divisor,
                        int32_t apply_scale, float scale, float offset, float mask_value, float* out_invdepth, float* out_mask,
                        void* stream) {
  if (!ip_dim_ok(H) || !ip_dim_ok(W) || !ip_dim_ok(H2) || !ip_dim_ok(W2)) return GS_E_SHAPE;
  if (src_dtype != GS_DEPTH_MAP_U16 && src_dtype != GS_DEPTH_MAP_F32) return GS_E_SHAPE;
  if (!src || !out_invdepth) return GS_E_NULL;
  if (((uintptr_t)src & (src_dtype == GS_DEPTH_MAP_U16 ? 1 : 3)) || ((uintptr_t)out_invdepth & 3) || ((uintptr_t)out_mask & 3))
    return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H2 * W2;
  hipLaunchKernelGGL(invdepth_prepare_kernel, dim3((unsigned)((n + GS_BLOCK - 1) / GS_BLOCK)), dim3(GS_BLOCK), 0, s, src,
                     (int)src_dtype, (int)H, (int)W, (int)H2, (int)W2, divisor, (int)(apply_scale != 0), scale, offset, mask_value,
                     out_invdepth, out_mask);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
