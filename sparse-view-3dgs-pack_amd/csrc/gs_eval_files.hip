// gs_eval_files.hip - what the evaluation from FILES needs beside gs_eval.hip (gfx950, wave64):
//
// gs_resize_bicubic_u8: PIL.Image.resize's default filter on 8-bit images - the antialiased bicubic of Pillow's
// Resample.c - bit for bit (DNGaussian/metrics_dtu.py:37-39 scores DTU on a quarter-size resize).  Pillow works in
// integers: per output sample a run of int32 coefficients (the normalised double weights times 2^22, rounded half away
// from zero), an int32 accumulator that starts at 2^21, an arithmetic shift by 22 and a clamp to a byte.  The tables are
// formed on the host in double (gsplat_amd/imageio.py), so nothing here rounds: integer sums have no order.
//   resize_h_kernel   [H,W,C] -> [H,W2,C], one thread per output byte
//   resize_v_kernel   [H,W2,C] -> [H2,W2,C], one thread per 4 adjacent bytes of an output row: the rows a thread reads are
//                     rows of the source, so a wave's loads are 256 contiguous bytes of each of the up to ky rows
// A pass whose sizes agree is skipped, as Pillow skips it; with both skipped the image is copied.
//
// gs_eval_ssim_sk: skimage.metrics.structural_similarity(a, b, channel_axis=2, data_range=1.0) with its defaults (7 x 7
// uniform window, sample covariance, the mean over the map cropped by 3 pixels - i.e. over the windows that lie wholly
// inside the image), on the pixels gs_eval_metrics sees (gs_eval_px.h).  A workgroup takes 32 x 32 windows of one channel
// plane: the 38 x 38 transformed pixels of both images go to LDS, the five window sums are formed separably in float64
// (7 taps in ascending order, rows then columns), S in float64, one partial per workgroup; one workgroup adds the partials
// in index order.  No atomics, no host synchronisation, the same bits on every run.
#include "gs_common.h"
#include "gs_eval_px.h"
#include "gs_resize.h"  // rs_clip8, rs_run: shared with gs_image_ingest.hip

namespace {

__device__ __forceinline__ void rs_store_f32(float* __restrict__ outf, int C, int H2, int W2, int y, int j, uint8_t q) {
  const int x = j / C, c = j - x * C;
  outf[((size_t)c * H2 + y) * W2 + x] = __fdiv_rn((float)q, 255.0f);  // to_tensor
}

__global__ void __launch_bounds__(GS_BLOCK) resize_h_kernel(const uint8_t* __restrict__ in, int H, int W, int C, int W2,
                                                            const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef,
                                                            int ksize, uint8_t* __restrict__ out, float* __restrict__ outf) {
  const int64_t t = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  const int row = W2 * C;
  if (t >= (int64_t)H * row) return;
  const int y = (int)(t / row), j = (int)(t - (int64_t)y * row);
  const int x2 = j / C, c = j - x2 * C;
  int lo;
  const int n = rs_run(bounds, x2, ksize, W, lo);
  const uint8_t* p = in + ((size_t)y * W + lo) * C + c;
  const int32_t* k = coef + (size_t)x2 * ksize;
  int32_t acc = 1 << (RS_PREC - 1);
  for (int i = 0; i < n; i++) acc += k[i] * (int32_t)p[(size_t)i * C];
  const uint8_t q = rs_clip8(acc);
  out[t] = q;
  if (outf) rs_store_f32(outf, C, H, W2, y, j, q);
}

// src [H,row] bytes -> out [H2,row]; blockIdx.x = y2 * blocks_per_row + the block's place in the row
__global__ void __launch_bounds__(GS_BLOCK) resize_v_kernel(const uint8_t* __restrict__ src, int H, int row, int C, int H2,
                                                            const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef,
                                                            int ksize, int blocks_per_row, uint8_t* __restrict__ out,
                                                            float* __restrict__ outf) {
  const int y2 = blockIdx.x / blocks_per_row;
  const int j0 = ((blockIdx.x - y2 * blocks_per_row) * GS_BLOCK + threadIdx.x) * 4;
  if (j0 >= row) return;
  int lo;
  const int n = rs_run(bounds, y2, ksize, H, lo);
  const int32_t* k = coef + (size_t)y2 * ksize;
  int32_t acc[4];
#pragma unroll
  for (int e = 0; e < 4; e++) acc[e] = 1 << (RS_PREC - 1);
  const bool vec = (row & 3) == 0 && (((uintptr_t)src) & 3) == 0;  // then j0 + 3 < row and every row's word is aligned
  if (vec) {
    for (int i = 0; i < n; i++) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(src + (size_t)(lo + i) * row + j0);
      const int32_t kk = k[i];
#pragma unroll
      for (int e = 0; e < 4; e++) acc[e] += kk * (int32_t)((w >> (8 * e)) & 255u);
    }
  } else {
    for (int i = 0; i < n; i++) {
      const uint8_t* p = src + (size_t)(lo + i) * row + j0;
      const int32_t kk = k[i];
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (j0 + e < row) acc[e] += kk * (int32_t)p[e];
    }
  }
  const int W2 = row / C;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    if (j0 + e >= row) break;
    const uint8_t q = rs_clip8(acc[e]);
    out[(size_t)y2 * row + j0 + e] = q;
    if (outf) rs_store_f32(outf, C, H2, W2, y2, j0 + e, q);
  }
}

__global__ void __launch_bounds__(GS_BLOCK) resize_copy_kernel(const uint8_t* __restrict__ in, int H, int row, int C,
                                                               uint8_t* __restrict__ out, float* __restrict__ outf) {
  const int64_t t = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (t >= (int64_t)H * row) return;
  const int y = (int)(t / row), j = (int)(t - (int64_t)y * row);
  const uint8_t q = in[t];
  out[t] = q;
  if (outf) rs_store_f32(outf, C, H, row / C, y, j, q);
}

inline bool rs_shape_ok(int C, int H, int W, int H2, int W2) {
  if ((C != 1 && C != 3) || H <= 0 || W <= 0 || H2 <= 0 || W2 <= 0) return false;
  const int64_t lim = (int64_t)1 << 30;  // bytes of any of the three images: thread and block counts stay in 32 bits
  return (int64_t)H * W * C <= lim && (int64_t)H * W2 * C <= lim && (int64_t)H2 * W2 * C <= lim;
}

// ---------------------------------------------------------------------------------------------- SSIM_sk
constexpr int SK_T = 32;            // windows per tile edge
constexpr int SK_WIN = 7;           // skimage's default win_size
constexpr int SK_S = SK_T + SK_WIN - 1;  // pixels per tile edge
constexpr int SK_ALL_FLAGS = GS_EVAL_CLAMP | GS_EVAL_QUANTISE | GS_EVAL_MASK_DTU;
// both kernels are written for 4 waves: thread -> (column tid & 31, rows 4 * (tid >> 5) ..+3) covers the 32 x 32 windows, the
// workgroup total adds four wave sums in one fixed order, and the finish kernel gives each of up to 4 channels a wave
static_assert(GS_BLOCK == 256 && SK_T == 32, "ssim_sk kernels: 256 threads, 32 x 32 windows per workgroup");

inline int64_t sk_tiles(int C, int H, int W) {
  return (int64_t)((W - SK_WIN + 1 + SK_T - 1) / SK_T) * ((H - SK_WIN + 1 + SK_T - 1) / SK_T) * C;
}

__global__ void __launch_bounds__(GS_BLOCK) ssim_sk_tile_kernel(const float* __restrict__ render, const float* __restrict__ gt,
                                                                const float* __restrict__ mask, int H, int W, int flags, int gx,
                                                                int gy, double* __restrict__ partials) {
  __shared__ float tile[2][SK_S][SK_S + 1];
  __shared__ double hor[5][SK_S][SK_T + 1];
  __shared__ double red[GS_BLOCK / 64];
  const int t = blockIdx.x;
  const int z = t / (gx * gy), rem = t - z * gx * gy;
  const int by = (rem / gx) * SK_T, bx = (rem % gx) * SK_T;
  const size_t plane = (size_t)z * H * W;
  const bool masked = (flags & GS_EVAL_MASK_DTU) != 0;
  for (int k = threadIdx.x; k < SK_S * SK_S; k += GS_BLOCK) {
    const int r = k / SK_S, c = k - r * SK_S;
    const int y = by + r, x = bx + c;
    float a = 0.f, b = 0.f;
    if (y < H && x < W) {  // (beyond the image: read by no window that counts)
      const size_t at = (size_t)y * W + x;
      const float m = masked ? mask[at] : 0.f;
      a = ev_transform(render[plane + at], m, flags);
      b = ev_transform(gt[plane + at], m, flags);
    }
    tile[0][r][c] = a;
    tile[1][r][c] = b;
  }
  __syncthreads();
  for (int item = threadIdx.x; item < SK_S * SK_T; item += GS_BLOCK) {
    const int r = item / SK_T, c = item - r * SK_T;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < SK_WIN; e++) {
      const double a = (double)tile[0][r][c + e], b = (double)tile[1][r][c + e];
      s[0] += a;
      s[1] += b;
      s[2] += a * a;
      s[3] += b * b;
      s[4] += a * b;
    }
#pragma unroll
    for (int q = 0; q < 5; q++) hor[q][r][c] = s[q];
  }
  __syncthreads();
  const int lx = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
  const int nwx = W - SK_WIN + 1, nwy = H - SK_WIN + 1;
  const double C1 = (0.01 * 1.0) * (0.01 * 1.0), C2 = (0.03 * 1.0) * (0.03 * 1.0);  // (K R)^2 at data_range R = 1
  const double NP = (double)(SK_WIN * SK_WIN), cov_norm = NP / (NP - 1.0);          // use_sample_covariance
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (bx + lx >= nwx || by + r0 + j >= nwy) continue;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < SK_WIN; e++)
#pragma unroll
      for (int q = 0; q < 5; q++) s[q] += hor[q][r0 + j + e][lx];
    const double ux = s[0] / NP, uy = s[1] / NP, uxx = s[2] / NP, uyy = s[3] / NP, uxy = s[4] / NP;
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
    const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    sum += (A1 * A2) / (B1 * B2);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_down(sum, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partials[t] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup.  Wave c owns channel c: lane l adds the l-th contiguous chunk of the channel's partials in index order, lane
// 0 the 64 chunk sums in lane order; thread 0 takes the channels' means in channel order.
__global__ void __launch_bounds__(GS_BLOCK) ssim_sk_finish_kernel(const double* __restrict__ partials, int per_plane, int C,
                                                                  double windows, double* __restrict__ out) {
  __shared__ double chunk[4][64];
  __shared__ double total[4];
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (c < C) {
    const int per = (per_plane + 63) / 64;
    const int lo = min(lane * per, per_plane), hi = min(lo + per, per_plane);
    const double* p = partials + (size_t)c * per_plane;
    double s = 0.0;
    for (int i = lo; i < hi; i++) s += p[i];
    chunk[c][lane] = s;
  }
  __syncthreads();
  if (c < C && lane == 0) {
    double s = 0.0;
    for (int l = 0; l < 64; l++) s += chunk[c][l];
    total[c] = s / windows;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int q = 0; q < C; q++) s += total[q];
  out[0] = s / (double)C;
}

}  // namespace

extern "C" {

size_t gs_resize_tmp_bytes(int32_t H, int32_t W, int32_t C, int32_t H2, int32_t W2) {
  if (!rs_shape_ok(C, H, W, H2, W2)) return 0;
  return (H2 != H && W2 != W) ? gs_align((size_t)H * W2 * C) : 0;
}

int gs_resize_bicubic_u8(const uint8_t* in, int32_t H, int32_t W, int32_t C, int32_t H2, int32_t W2, const int32_t* xbounds,
                         const int32_t* xcoef, int32_t kx, const int32_t* ybounds, const int32_t* ycoef, int32_t ky, void* tmp,
                         size_t tmp_bytes, uint8_t* out, float* out_f32, void* stream) {
  if (!in || !out) return GS_E_NULL;
  if (!rs_shape_ok(C, H, W, H2, W2)) return GS_E_SHAPE;
  const bool hpass = W2 != W, vpass = H2 != H;
  if ((hpass && (!xbounds || !xcoef)) || (vpass && (!ybounds || !ycoef)) || (hpass && vpass && !tmp)) return GS_E_NULL;
  if ((hpass && kx <= 0) || (vpass && ky <= 0)) return GS_E_SHAPE;
  if (hpass && vpass && tmp_bytes < gs_resize_tmp_bytes(H, W, C, H2, W2)) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const int row2 = W2 * C;
  if (!hpass && !vpass) {
    const unsigned blocks = (unsigned)(((int64_t)H * row2 + GS_BLOCK - 1) / GS_BLOCK);
    hipLaunchKernelGGL(resize_copy_kernel, dim3(blocks), dim3(GS_BLOCK), 0, s, in, H, row2, C, out, out_f32);
    GS_LAUNCH_CHECK(s, 0);
    return GS_OK;
  }
  const uint8_t* vsrc = in;
  if (hpass) {
    uint8_t* hdst = vpass ? (uint8_t*)tmp : out;
    const unsigned blocks = (unsigned)(((int64_t)H * row2 + GS_BLOCK - 1) / GS_BLOCK);
    hipLaunchKernelGGL(resize_h_kernel, dim3(blocks), dim3(GS_BLOCK), 0, s, in, H, W, C, W2, xbounds, xcoef, kx, hdst,
                       vpass ? (float*)nullptr : out_f32);
    GS_LAUNCH_CHECK(s, 0);
    vsrc = hdst;
  }
  if (vpass) {
    const int bpr = ((row2 + 3) / 4 + GS_BLOCK - 1) / GS_BLOCK;
    hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)((int64_t)H2 * bpr)), dim3(GS_BLOCK), 0, s, vsrc, H, row2, C, H2, ybounds,
                       ycoef, ky, bpr, out, out_f32);
    GS_LAUNCH_CHECK(s, 0);
  }
  return GS_OK;
}

size_t gs_eval_ssim_sk_tmp_bytes(int32_t C, int32_t H, int32_t W) {
  if (C <= 0 || C > 4 || H < SK_WIN || W < SK_WIN) return 0;
  return gs_align((size_t)sk_tiles(C, H, W) * sizeof(double));
}

int gs_eval_ssim_sk(const float* render, const float* gt, const float* mask, int32_t C, int32_t H, int32_t W, int32_t flags,
                    void* tmp, size_t tmp_bytes, double* out, void* stream) {
  if (!render || !gt || !tmp || !out) return GS_E_NULL;
  if ((flags & GS_EVAL_MASK_DTU) && !mask) return GS_E_NULL;
  if (C <= 0 || C > 4 || H < SK_WIN || W < SK_WIN || (flags & ~SK_ALL_FLAGS)) return GS_E_SHAPE;
  const int64_t n = sk_tiles(C, H, W);
  if (n > (int64_t)1 << 30 || tmp_bytes < gs_eval_ssim_sk_tmp_bytes(C, H, W)) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const int gx = (W - SK_WIN + 1 + SK_T - 1) / SK_T, gy = (H - SK_WIN + 1 + SK_T - 1) / SK_T;
  hipLaunchKernelGGL(ssim_sk_tile_kernel, dim3((unsigned)n), dim3(GS_BLOCK), 0, s, render, gt, mask, H, W, flags, gx, gy,
                     (double*)tmp);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(ssim_sk_finish_kernel, dim3(1), dim3(GS_BLOCK), 0, s, (const double*)tmp, gx * gy, C,
                     (double)(W - SK_WIN + 1) * (double)(H - SK_WIN + 1), out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
