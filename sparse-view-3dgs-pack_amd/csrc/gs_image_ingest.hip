// gs_image_ingest.hip - one decoded image, u8 [H,W,C] interleaved, to what the reference's Camera.__init__ keeps
// (LGDWT-GS/utils/camera_utils.py:loadCam, scene/cameras.py:42-56), in at most two launches (gfx950, wave64):
//   optional composite onto black / white at the source size (NeRF-synthetic, scene/dataset_readers.py:353-359), in double with
//     no contraction: q = byte(trunc((c / 255 * (a / 255) + bg * (1 - a / 255)) * 255)); the image goes on as RGB
//   PIL.Image.resize((W2, H2)) with its default filter: RGB as gs_resize_bicubic_u8; LA / RGBA by Pillow's premultiplied rule -
//     premultiply t = c a + 128, c' = ((t >> 8) + t) >> 8 fused into the load of whichever pass runs first, both passes of the
//     integer bicubic on the premultiplied bytes (alpha included), un-premultiply a == 0 or 255 -> c', else
//     min(255, 255 c' / a) in integer division fused into the store of whichever pass runs last.  Same size: a copy, no round trip
//   outputs, each optional: the resized bytes [H2,W2,Ce]; original_image fp32 [3,H2,W2] = byte / 255 (one correctly rounded
//     division); alpha_mask fp32 [1,H2,W2] = alpha byte / 255 or ones, a half of its columns zeroed on request
//   ingest_h_kernel     [H,W,C] -> [H,W2,Ce], one thread per output PIXEL (its Ce accumulators: the un-premultiply needs them
//                       together; an RGBA source pixel is one word load per tap)
//   ingest_v_kernel     [H,W2,Cs] -> [H2,W2,Ce], one thread per 4 adjacent bytes of an output row, word loads when the rows are
//                       word-aligned (RGBA always, LA with even W2): the vertical pass of gs_eval_files.hip with the fused ends
//   ingest_copy_kernel  same size: one thread per pixel
// Integer sums have no order, the composite is a fixed sequence of double roundings: the same bits as the numpy path of
// gsplat_amd/imageio.py.  No atomics, no read-back, no host synchronisation.
#include "gs_common.h"
#include "gs_resize.h"

namespace {

enum { PRE_NONE = 0, PRE_MUL = 1, PRE_COMP = 2 };
constexpr int II_ALL_FLAGS = GS_INGEST_COMPOSITE | GS_INGEST_WHITE | GS_INGEST_ZERO_LEFT | GS_INGEST_ZERO_RIGHT;

struct IngestOut {
  uint8_t* u8;    // [H2,W2,Ce] or null
  float* image;   // [3,H2,W2] or null
  float* alpha;   // [1,H2,W2] or null
  int u8_word;    // u8 is word-aligned and its rows are whole words
  int unpre;      // the bytes are premultiplied: un-premultiply them on the way out
  int flags;
};

__device__ __forceinline__ uint32_t ii_premul(uint32_t c, uint32_t a) {
  const uint32_t t = c * a + 128u;
  return ((t >> 8) + t) >> 8;
}
__device__ __forceinline__ uint32_t ii_unpremul(uint32_t c, uint32_t a) {
  if (a == 0u || a == 255u) return c;
  const uint32_t q = (255u * c) / a;
  return q > 255u ? 255u : q;
}
__device__ __forceinline__ uint32_t ii_composite(uint32_t c, uint32_t a, double bg) {
  const double na = (double)a / 255.0;
  const double v = ((double)c / 255.0) * na + bg * (1.0 - na);
  return (uint32_t)((int64_t)(v * 255.0)) & 255u;  // np.array(arr * 255.0, dtype=np.byte): truncation, the byte's bits
}
__device__ __forceinline__ float ii_mask(const IngestOut& o, uint32_t a, bool has_alpha, int x, int W2) {
  float m = has_alpha ? __fdiv_rn((float)a, 255.0f) : 1.0f;
  const int half = W2 / 2;
  if ((o.flags & GS_INGEST_ZERO_LEFT) && x < half) m = 0.0f;
  if ((o.flags & GS_INGEST_ZERO_RIGHT) && x >= half) m = 0.0f;
  return m;
}

// the Ce effective bytes of the source pixel at p (C interleaved bytes)
template <int PRE>
__device__ __forceinline__ void ii_load_px(const uint8_t* __restrict__ p, int C, int word, double bg, uint32_t v[4]) {
  uint32_t b[4] = {0u, 0u, 0u, 0u};
  if (C == 4 && word) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int c = 0; c < 4; c++) b[c] = (w >> (8 * c)) & 255u;
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (c < C) b[c] = p[c];
  }
  if (PRE == PRE_NONE) {
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = b[c];
  } else if (PRE == PRE_MUL) {
    const uint32_t a = C == 4 ? b[3] : b[1];
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = (c < C - 1) ? ii_premul(b[c], a) : b[c];
  } else {
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = ii_composite(b[c], b[3], bg);
    v[3] = 0u;
  }
}

// one finished pixel: un-premultiply, then the three outputs
__device__ __forceinline__ void ii_emit_px(const IngestOut& o, int H2, int W2, int Ce, int y, int x, uint32_t q[4]) {
  const bool has_alpha = Ce == 4;
  if (o.unpre) {
    const uint32_t a = q[Ce - 1];
#pragma unroll
    for (int c = 0; c < 3; c++)
      if (c < Ce - 1) q[c] = ii_unpremul(q[c], a);
  }
  const size_t px = (size_t)y * W2 + x;
  if (o.u8) {
    if (Ce == 4 && o.u8_word) {
      *reinterpret_cast<uint32_t*>(o.u8 + px * 4) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (c < Ce) o.u8[px * Ce + c] = (uint8_t)q[c];
    }
  }
  if (o.image) {
#pragma unroll
    for (int c = 0; c < 3; c++) o.image[((size_t)c * H2 + y) * W2 + x] = __fdiv_rn((float)q[c], 255.0f);
  }
  if (o.alpha) o.alpha[px] = ii_mask(o, q[3], has_alpha, x, W2);
}

// in [H,W,C] -> [H,W2,Ce]: mid (premultiplied bytes, when the vertical pass follows) or the outputs
template <int PRE>
__global__ void __launch_bounds__(GS_BLOCK) ingest_h_kernel(const uint8_t* __restrict__ in, int H, int W, int C, int Ce, int W2,
                                                            const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef,
                                                            int ksize, int word, double bg, uint8_t* __restrict__ mid,
                                                            IngestOut o) {
  const int64_t t = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (t >= (int64_t)H * W2) return;
  const int y = (int)(t / W2), x2 = (int)(t - (int64_t)y * W2);
  int lo;
  const int n = rs_run(bounds, x2, ksize, W, lo);
  const uint8_t* p = in + ((size_t)y * W + lo) * C;
  const int32_t* k = coef + (size_t)x2 * ksize;
  int32_t acc[4];
#pragma unroll
  for (int c = 0; c < 4; c++) acc[c] = 1 << (RS_PREC - 1);
  for (int i = 0; i < n; i++) {
    uint32_t v[4];
    ii_load_px<PRE>(p + (size_t)i * C, C, word, bg, v);
    const int32_t kk = k[i];
#pragma unroll
    for (int c = 0; c < 4; c++) acc[c] += kk * (int32_t)v[c];
  }
  uint32_t q[4];
#pragma unroll
  for (int c = 0; c < 4; c++) q[c] = rs_clip8(acc[c]);
  if (mid) {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (c < Ce) mid[(size_t)t * Ce + c] = (uint8_t)q[c];
  } else {
    ii_emit_px(o, H, W2, Ce, y, x2, q);
  }
}

// src [H,W2,Cs] -> the outputs [H2,W2,Ce]; blockIdx.x = y2 * blocks_per_row + the block's place in the row.  Cs != Ce only
// with PRE_COMP (RGBA in, RGB out).  `word`: Cs == Ce, src word-aligned and its rows whole words
template <int PRE>
__global__ void __launch_bounds__(GS_BLOCK) ingest_v_kernel(const uint8_t* __restrict__ src, int H, int W2, int Cs, int Ce, int H2,
                                                            const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef,
                                                            int ksize, int blocks_per_row, int word, double bg, IngestOut o) {
  const int y2 = blockIdx.x / blocks_per_row;
  const int j0 = ((blockIdx.x - y2 * blocks_per_row) * GS_BLOCK + threadIdx.x) * 4;
  const int row = W2 * Ce;
  if (j0 >= row) return;
  int lo;
  const int n = rs_run(bounds, y2, ksize, H, lo);
  const int32_t* k = coef + (size_t)y2 * ksize;
  const size_t srow = (size_t)W2 * Cs;
  int32_t acc[4];
  int xs[4], ch[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    acc[e] = 1 << (RS_PREC - 1);
    const int j = min(j0 + e, row - 1);
    xs[e] = j / Ce;
    ch[e] = j - xs[e] * Ce;
  }
  if (PRE != PRE_COMP && word) {  // then j0 + 3 < row, and with alpha (Ce = 2 or 4) the word holds whole pixels
    for (int i = 0; i < n; i++) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(src + (size_t)(lo + i) * srow + j0);
      const int32_t kk = k[i];
      uint32_t b[4];
#pragma unroll
      for (int e = 0; e < 4; e++) b[e] = (w >> (8 * e)) & 255u;
      if (PRE == PRE_MUL) {
        if (Ce == 4) {
#pragma unroll
          for (int e = 0; e < 3; e++) b[e] = ii_premul(b[e], b[3]);
        } else {
          b[0] = ii_premul(b[0], b[1]);
          b[2] = ii_premul(b[2], b[3]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; e++) acc[e] += kk * (int32_t)b[e];
    }
  } else {
    for (int i = 0; i < n; i++) {
      const uint8_t* r = src + (size_t)(lo + i) * srow;
      const int32_t kk = k[i];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        if (j0 + e >= row) continue;
        const uint8_t* p = r + (size_t)xs[e] * Cs;
        uint32_t v = p[ch[e]];
        if (PRE == PRE_MUL && ch[e] != Ce - 1) v = ii_premul(v, p[Ce - 1]);
        if (PRE == PRE_COMP) v = ii_composite(v, p[3], bg);
        acc[e] += kk * (int32_t)v;
      }
    }
  }
  uint32_t q[4];
#pragma unroll
  for (int e = 0; e < 4; e++) q[e] = rs_clip8(acc[e]);
  if (o.unpre) {  // Ce = 2 or 4 divides j0, and the row is whole pixels: a thread's valid bytes are whole pixels
    if (Ce == 4) {
#pragma unroll
      for (int e = 0; e < 3; e++) q[e] = ii_unpremul(q[e], q[3]);
    } else {
      q[0] = ii_unpremul(q[0], q[1]);
      q[2] = ii_unpremul(q[2], q[3]);
    }
  }
  if (o.u8) {
    if (o.u8_word) {
      *reinterpret_cast<uint32_t*>(o.u8 + (size_t)y2 * row + j0) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (j0 + e < row) o.u8[(size_t)y2 * row + j0 + e] = (uint8_t)q[e];
    }
  }
  if (o.image || o.alpha) {
    const bool has_alpha = Ce == 4;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (j0 + e >= row) break;
      const size_t px = (size_t)y2 * W2 + xs[e];
      if (o.image && ch[e] < 3) o.image[(size_t)ch[e] * H2 * W2 + px] = __fdiv_rn((float)q[e], 255.0f);
      if (o.alpha && ch[e] == (has_alpha ? 3 : 0)) o.alpha[px] = ii_mask(o, q[e], has_alpha, xs[e], W2);
    }
  }
}

template <int PRE>
__global__ void __launch_bounds__(GS_BLOCK) ingest_copy_kernel(const uint8_t* __restrict__ in, int H, int W, int C, int Ce,
                                                               int word, double bg, IngestOut o) {
  const int64_t t = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (t >= (int64_t)H * W) return;
  const int y = (int)(t / W), x = (int)(t - (int64_t)y * W);
  uint32_t q[4];
  ii_load_px<PRE>(in + (size_t)t * C, C, word, bg, q);
  ii_emit_px(o, H, W, Ce, y, x, q);
}

inline bool ii_shape_ok(int C, int H, int W, int H2, int W2, int flags) {
  if ((C != 2 && C != 3 && C != 4) || H <= 0 || W <= 0 || H2 <= 0 || W2 <= 0 || (flags & ~II_ALL_FLAGS)) return false;
  if ((flags & GS_INGEST_COMPOSITE) && C != 4) return false;
  if ((flags & GS_INGEST_WHITE) && !(flags & GS_INGEST_COMPOSITE)) return false;
  const int64_t lim = (int64_t)1 << 30;  // bytes of any of the three images: thread and block counts stay in 32 bits
  return (int64_t)H * W * C <= lim && (int64_t)H * W2 * C <= lim && (int64_t)H2 * W2 * C <= lim;
}
inline bool ii_word(const void* p, int64_t row_bytes) { return (((uintptr_t)p) & 3) == 0 && (row_bytes & 3) == 0; }

}  // namespace

extern "C" {

size_t gs_image_ingest_tmp_bytes(int32_t H, int32_t W, int32_t C, int32_t H2, int32_t W2, int32_t flags) {
  if (!ii_shape_ok(C, H, W, H2, W2, flags)) return 0;
  const int Ce = (flags & GS_INGEST_COMPOSITE) ? 3 : C;
  return (H2 != H && W2 != W) ? gs_align((size_t)H * W2 * Ce) : 0;
}

int gs_image_ingest(const uint8_t* in, int32_t H, int32_t W, int32_t C, int32_t H2, int32_t W2, const int32_t* xbounds,
                    const int32_t* xcoef, int32_t kx, const int32_t* ybounds, const int32_t* ycoef, int32_t ky, int32_t flags,
                    void* tmp, size_t tmp_bytes, uint8_t* out_u8, float* out_image, float* out_alpha, void* stream) {
  if (!in || (!out_u8 && !out_image && !out_alpha)) return GS_E_NULL;
  if (!ii_shape_ok(C, H, W, H2, W2, flags)) return GS_E_SHAPE;
  if (C == 2 && (out_image || out_alpha)) return GS_E_SHAPE;  // LA: resize only
  const bool hpass = W2 != W, vpass = H2 != H;
  if ((hpass && (!xbounds || !xcoef)) || (vpass && (!ybounds || !ycoef)) || (hpass && vpass && !tmp)) return GS_E_NULL;
  if ((hpass && kx <= 0) || (vpass && ky <= 0)) return GS_E_SHAPE;
  if (hpass && vpass && tmp_bytes < gs_image_ingest_tmp_bytes(H, W, C, H2, W2, flags)) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const bool comp = (flags & GS_INGEST_COMPOSITE) != 0;
  const int Ce = comp ? 3 : C;
  const bool alpha = Ce == 2 || Ce == 4;
  const double bg = (flags & GS_INGEST_WHITE) ? 1.0 : 0.0;
  const int pre = comp ? PRE_COMP : (alpha ? PRE_MUL : PRE_NONE);
  const int in_word = C == 4 && ii_word(in, 4);
  IngestOut o;
  o.u8 = out_u8;
  o.image = out_image;
  o.alpha = out_alpha;
  o.u8_word = out_u8 && ii_word(out_u8, (int64_t)W2 * Ce);
  o.unpre = alpha && (hpass || vpass);
  o.flags = flags;
  if (!hpass && !vpass) {
    const unsigned blocks = (unsigned)(((int64_t)H * W + GS_BLOCK - 1) / GS_BLOCK);
    if (comp)
      hipLaunchKernelGGL(ingest_copy_kernel<PRE_COMP>, dim3(blocks), dim3(GS_BLOCK), 0, s, in, H, W, C, Ce, in_word, bg, o);
    else
      hipLaunchKernelGGL(ingest_copy_kernel<PRE_NONE>, dim3(blocks), dim3(GS_BLOCK), 0, s, in, H, W, C, Ce, in_word, bg, o);
    GS_LAUNCH_CHECK(s, 0);
    return GS_OK;
  }
  const uint8_t* vsrc = in;
  int vpre = pre, Cs = C;
  if (hpass) {
    uint8_t* mid = vpass ? (uint8_t*)tmp : nullptr;
    const unsigned blocks = (unsigned)(((int64_t)H * W2 + GS_BLOCK - 1) / GS_BLOCK);
    if (pre == PRE_COMP)
      hipLaunchKernelGGL(ingest_h_kernel<PRE_COMP>, dim3(blocks), dim3(GS_BLOCK), 0, s, in, H, W, C, Ce, W2, xbounds, xcoef, kx,
                         in_word, bg, mid, o);
    else if (pre == PRE_MUL)
      hipLaunchKernelGGL(ingest_h_kernel<PRE_MUL>, dim3(blocks), dim3(GS_BLOCK), 0, s, in, H, W, C, Ce, W2, xbounds, xcoef, kx,
                         in_word, bg, mid, o);
    else
      hipLaunchKernelGGL(ingest_h_kernel<PRE_NONE>, dim3(blocks), dim3(GS_BLOCK), 0, s, in, H, W, C, Ce, W2, xbounds, xcoef, kx,
                         in_word, bg, mid, o);
    GS_LAUNCH_CHECK(s, 0);
    vsrc = mid;
    vpre = PRE_NONE;  // the intermediate holds the effective bytes
    Cs = Ce;
  }
  if (vpass) {
    const int row2 = W2 * Ce;
    const int bpr = ((row2 + 3) / 4 + GS_BLOCK - 1) / GS_BLOCK;
    const unsigned blocks = (unsigned)((int64_t)H2 * bpr);
    const int word = Cs == Ce && ii_word(vsrc, row2);
    if (vpre == PRE_COMP)
      hipLaunchKernelGGL(ingest_v_kernel<PRE_COMP>, dim3(blocks), dim3(GS_BLOCK), 0, s, vsrc, H, W2, Cs, Ce, H2, ybounds, ycoef, ky,
                         bpr, word, bg, o);
    else if (vpre == PRE_MUL)
      hipLaunchKernelGGL(ingest_v_kernel<PRE_MUL>, dim3(blocks), dim3(GS_BLOCK), 0, s, vsrc, H, W2, Cs, Ce, H2, ybounds, ycoef, ky,
                         bpr, word, bg, o);
    else
      hipLaunchKernelGGL(ingest_v_kernel<PRE_NONE>, dim3(blocks), dim3(GS_BLOCK), 0, s, vsrc, H, W2, Cs, Ce, H2, ybounds, ycoef, ky,
                         bpr, word, bg, o);
    GS_LAUNCH_CHECK(s, 0);
  }
  return GS_OK;
}

}  // extern "C"
