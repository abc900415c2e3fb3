// gs_eval.hip - test-set evaluation of one view on the device (gfx950, wave64): MSE / PSNR, SSIM and L1 of a render against
// its ground truth from ONE pass over the two images, in the forms the reference's evaluation scripts compute them
// (LGDWT-GS/render.py:45-46 -> metrics.py:31-32,70-83; training_report, e.g. DNGaussian/train_llff.py:298-302;
// DNGaussian/metrics_dtu.py:40-46,93-95).
//
// eval_tile_kernel: a workgroup of GS_BLOCK threads takes one 32 x 32 tile of one channel plane (the tiling, the XCD-banded
// tile order and the separable 11-tap convolution of ssim_fwd_kernel in gs_loss.hip, restated here so that the criterion's
// kernels keep their bits), stages the tile and its 5-pixel halo into LDS WITH the pixel transform applied
//     clamp to [0, 1]  ->  8-bit round trip  ->  blend to white under the mask
// and forms, over the tile's own pixels only, the SSIM-map sum (fp32, as ssim_fwd_kernel), sum (a-b)^2, sum |a-b|, the
// masked sum (a-b)^2 and its element count (float64).  One row of partials per workgroup, plain stores, no atomics.
// eval_finish_kernel: one workgroup adds the rows in index order in float64 and writes the view's GS_EVAL_WORDS doubles.
#include "gs_common.h"
#include "gs_eval_px.h"

namespace {

__constant__ float EV_GW[11] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f,
                                0.10936068743467331f,  0.21300552785396576f,  0.26601171493530273f,
                                0.21300552785396576f,  0.10936068743467331f,  0.036000773310661316f,
                                0.0075987582094967365f, 0.001028380123898387f};
constexpr int EV_ST = 32;          // tile edge
constexpr int EV_SH = EV_ST + 10;  // with the halo
constexpr int EV_HS = 33;          // row stride of the horizontal-pass buffer (odd, see gs_loss.hip)
constexpr int EV_Q = 5;            // partial words per workgroup: ssim sum, sum d^2, sum |d|, masked sum d^2, masked count
constexpr int EV_LDS_WORDS = (2 * EV_SH * (EV_SH + 1) > 5 * EV_SH * EV_HS) ? 2 * EV_SH * (EV_SH + 1) : 5 * EV_SH * EV_HS;
constexpr int EV_ALL_FLAGS = GS_EVAL_CLAMP | GS_EVAL_QUANTISE | GS_EVAL_MASK_DTU;

// launch slot -> tile, as ssim_tile_of_block (gs_loss.hip): slot b belongs to XCD b % 8, and XCD k works through the k-th
// contiguous eighth of the tiles in raster order, so that tiles which share halo lines meet in one L2
struct EvTile { int bx, by, z, linear; bool live; };
__device__ __forceinline__ EvTile ev_tile_of_block(int gx, int gy, int gz, unsigned b) {
  const int n = gx * gy * gz, per = (n + 7) / 8;
  const int t = (int)(b & 7) * per + (int)(b >> 3);
  EvTile r;
  r.live = (int)(b >> 3) < per && t < n;
  r.linear = t;
  r.z = t / (gx * gy);
  const int rem = t - r.z * gx * gy;
  r.by = (rem / gx) * EV_ST;
  r.bx = (rem % gx) * EV_ST;
  return r;
}
inline int64_t ev_tiles(int C, int H, int W) {
  return (int64_t)((W + EV_ST - 1) / EV_ST) * ((H + EV_ST - 1) / EV_ST) * C;
}

// (ev_byte and ev_transform, the pixel as the metrics see it: gs_eval_px.h, shared with gs_eval_files.hip)

// Halo tile of both images, transformed, into tile[0] (render) and tile[1] (gt).  Outside the image the tile holds 0: the
// convolution pads with zero AFTER the blend, as F.conv2d does.  With W a multiple of 4 and 16-byte aligned planes the
// aligned span [bx - 8, bx + 40) of a row is fetched as 12 float4 (a float4 lies entirely inside or outside the image).
__device__ __forceinline__ void ev_stage(const float* __restrict__ img1, const float* __restrict__ img2,
                                         const float* __restrict__ mask, size_t plane, int H, int W, int bx, int by, int flags,
                                         float (*tile)[EV_SH][EV_SH + 1]) {
  const bool masked = (flags & GS_EVAL_MASK_DTU) != 0;
  const bool vec = (W & 3) == 0 && ((((uintptr_t)img1) | ((uintptr_t)img2) | (masked ? (uintptr_t)mask : 0)) & 15) == 0;
  if (vec) {
    constexpr int VPR = 12, NV = EV_SH * VPR, NVI = (NV + GS_BLOCK - 1) / GS_BLOCK;
    float4 a[NVI], b[NVI], m[NVI];
    bool in[NVI];
#pragma unroll
    for (int it = 0; it < NVI; it++) {
      const int v = threadIdx.x + it * GS_BLOCK;
      const int r = v / VPR, q = v % VPR;
      const int y = by + r - 5, x4 = bx - 8 + 4 * q;
      a[it] = b[it] = m[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      in[it] = v < NV && y >= 0 && y < H && x4 >= 0 && x4 + 3 < W;
      if (in[it]) {
        a[it] = *reinterpret_cast<const float4*>(img1 + plane + (size_t)y * W + x4);
        b[it] = *reinterpret_cast<const float4*>(img2 + plane + (size_t)y * W + x4);
        if (masked) m[it] = *reinterpret_cast<const float4*>(mask + (size_t)y * W + x4);
      }
    }
#pragma unroll
    for (int it = 0; it < NVI; it++) {
      const int v = threadIdx.x + it * GS_BLOCK;
      if (v < NV) {
        const int r = v / VPR, c0 = 4 * (v % VPR) - 3;  // tile column of the vector's first element
        const float av[4] = {a[it].x, a[it].y, a[it].z, a[it].w}, bv[4] = {b[it].x, b[it].y, b[it].z, b[it].w};
        const float mv[4] = {m[it].x, m[it].y, m[it].z, m[it].w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int c = c0 + e;
          if (c >= 0 && c < EV_SH) {
            tile[0][r][c] = in[it] ? ev_transform(av[e], mv[e], flags) : 0.f;
            tile[1][r][c] = in[it] ? ev_transform(bv[e], mv[e], flags) : 0.f;
          }
        }
      }
    }
  } else {
    constexpr int NIT = (EV_SH * EV_SH + GS_BLOCK - 1) / GS_BLOCK;
    float a[NIT], b[NIT], m[NIT];
    bool in[NIT];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int k = threadIdx.x + it * GS_BLOCK;
      const int r = k / EV_SH, c = k % EV_SH;
      const int y = by + r - 5, x = bx + c - 5;
      a[it] = b[it] = m[it] = 0.f;
      in[it] = k < EV_SH * EV_SH && x >= 0 && x < W && y >= 0 && y < H;
      if (in[it]) {
        a[it] = img1[plane + (size_t)y * W + x];
        b[it] = img2[plane + (size_t)y * W + x];
        if (masked) m[it] = mask[(size_t)y * W + x];
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int k = threadIdx.x + it * GS_BLOCK;
      if (k < EV_SH * EV_SH) {
        tile[0][k / EV_SH][k % EV_SH] = in[it] ? ev_transform(a[it], m[it], flags) : 0.f;
        tile[1][k / EV_SH][k % EV_SH] = in[it] ? ev_transform(b[it], m[it], flags) : 0.f;
      }
    }
  }
}

// Separable 11-tap convolution of (a, a^2, b, b^2, ab) over the halo tile: ssim_conv_tile<5, true> of gs_loss.hip.  A thread
// produces 4 adjacent outputs along the pass direction from 14 inputs; every output is the sum over t = 0..10 in ascending
// order.  `tile` and `hor` share their LDS.  out[j] belongs to tile row 4 * (tid / 32) + j, column tid % 32.
__device__ __forceinline__ void ev_conv_tile(const float (*tile)[EV_SH][EV_SH + 1], float (*hor)[EV_SH][EV_HS],
                                             float (&out)[4][5]) {
#pragma clang fp contract(fast)  // as the criterion's SSIM (and the reference's nvcc build) contracts the taps
  constexpr int NITEM = EV_SH * (EV_ST / 4);
  constexpr int NR = (NITEM + GS_BLOCK - 1) / GS_BLOCK;
  float acc[NR][4][5];
#pragma unroll
  for (int rd = 0; rd < NR; rd++) {
    const int item = threadIdx.x + rd * GS_BLOCK;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int q = 0; q < 5; q++) acc[rd][j][q] = 0.f;
    if (item < NITEM) {
      const int r = item / (EV_ST / 4), c0 = (item % (EV_ST / 4)) * 4;
#pragma unroll
      for (int e = 0; e < 14; e++) {
        const float a = tile[0][r][c0 + e], b = tile[1][r][c0 + e];
        const float val[5] = {a, a * a, b, b * b, a * b};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int t = e - j;
          if (t >= 0 && t < 11) {
#pragma unroll
            for (int q = 0; q < 5; q++) acc[rd][j][q] += EV_GW[t] * val[q];
          }
        }
      }
    }
  }
  __syncthreads();  // every read of `tile` is done: `hor` may overwrite it
#pragma unroll
  for (int rd = 0; rd < NR; rd++) {
    const int item = threadIdx.x + rd * GS_BLOCK;
    if (item < NITEM) {
      const int r = item / (EV_ST / 4), c0 = (item % (EV_ST / 4)) * 4;
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int q = 0; q < 5; q++) hor[q][r][c0 + j] = acc[rd][j][q];
    }
  }
  __syncthreads();
  const int lx = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int q = 0; q < 5; q++) out[j][q] = 0.f;
#pragma unroll
  for (int e = 0; e < 14; e++) {
    float val[5];
#pragma unroll
    for (int q = 0; q < 5; q++) val[q] = hor[q][r0 + e][lx];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int t = e - j;
      if (t >= 0 && t < 11) {
#pragma unroll
        for (int q = 0; q < 5; q++) out[j][q] += EV_GW[t] * val[q];
      }
    }
  }
}

__device__ __forceinline__ double ev_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// partials: word-major [EV_Q][n_tiles] doubles (the finishing kernel reads one word's row contiguously)
__global__ void __launch_bounds__(GS_BLOCK) eval_tile_kernel(const float* __restrict__ render, const float* __restrict__ gt,
                                                             const float* __restrict__ mask, int H, int W, int planes, int flags,
                                                             float C1, float C2, double* __restrict__ partials, int n_tiles,
                                                             uint8_t* __restrict__ qout) {
  __shared__ float lds_buf[EV_LDS_WORDS];
  __shared__ double red[EV_Q][GS_BLOCK / 64];
  float (*tile)[EV_SH][EV_SH + 1] = reinterpret_cast<float (*)[EV_SH][EV_SH + 1]>(lds_buf);
  float (*hor)[EV_SH][EV_HS] = reinterpret_cast<float (*)[EV_SH][EV_HS]>(lds_buf);
  const EvTile tl = ev_tile_of_block((W + EV_ST - 1) / EV_ST, (H + EV_ST - 1) / EV_ST, planes, blockIdx.x);
  if (!tl.live) return;
  const size_t plane = (size_t)tl.z * H * W;
  const int bx = tl.bx, by = tl.by;
  const bool masked = (flags & GS_EVAL_MASK_DTU) != 0;
  ev_stage(render, gt, mask, plane, H, W, bx, by, flags, tile);
  __syncthreads();
  // the error sums of this thread's 4 own pixels, from the transformed tile (before the convolution overwrites it)
  const int lx = threadIdx.x & 31, ly0 = threadIdx.x >> 5;
  double se = 0.0, ae = 0.0, sem = 0.0, cnt = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = bx + lx, y = by + 4 * ly0 + j;
    if (x >= W || y >= H) continue;
    const double d = (double)tile[0][4 * ly0 + j + 5][lx + 5] - (double)tile[1][4 * ly0 + j + 5][lx + 5];
    se += d * d;
    ae += fabs(d);
    if (masked && mask[(size_t)y * W + x] == 1.0f) {
      sem += d * d;
      cnt += 1.0;
    }
    if (qout) qout[((size_t)y * W + x) * planes + tl.z] = ev_byte(render[plane + (size_t)y * W + x]);
  }
  float out[4][5];
  ev_conv_tile(tile, hor, out);
  float msum = 0.f;  // the SSIM map of the 4 pixels: ssim_fwd_pixels of gs_loss.hip (one division per pixel)
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = bx + lx, y = by + 4 * ly0 + j;
    if (x >= W || y >= H) continue;
    const float mu1 = out[j][0], mu2 = out[j][2];
    const float sigma1_sq = out[j][1] - mu1 * mu1;
    const float sigma2_sq = out[j][3] - mu2 * mu2;
    const float sigma12 = out[j][4] - mu1 * mu2;
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const float Cc = (2.0f * mu1_mu2 + C1);
    const float D = (2.0f * sigma12 + C2);
    const float A = (mu1_sq + mu2_sq + C1);
    const float B = (sigma1_sq + sigma2_sq + C2);
    msum += (Cc * D) * (1.0f / (A * B));
  }
  // workgroup totals: a fixed shuffle tree per wave, the four waves added in one fixed order
  float ms = msum;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ms += __shfl_down(ms, off, 64);
  const double v[EV_Q] = {(double)ms, ev_wave_sum(se), ev_wave_sum(ae), ev_wave_sum(sem), ev_wave_sum(cnt)};
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < EV_Q; q++) red[q][threadIdx.x >> 6] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < EV_Q) {
    const int q = threadIdx.x;
    double t;
    if (q == 0) {  // the SSIM sum accumulates in fp32, as ssim_store_partial does
      t = (double)(((float)red[0][0] + (float)red[0][1]) + ((float)red[0][2] + (float)red[0][3]));
    } else {
      t = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
    }
    partials[(size_t)q * n_tiles + tl.linear] = t;
  }
}

// One workgroup.  Wave q owns word q: lane l adds the l-th contiguous chunk of the word's partials in index order, then
// lane 0 adds the 64 chunk sums in lane order - index order throughout, one fixed association, float64.
__global__ void __launch_bounds__(GS_BLOCK * 2) eval_finish_kernel(const double* __restrict__ partials, int n_tiles, double n_elems,
                                                                   int masked, double* __restrict__ out_row) {
  __shared__ double chunk[EV_Q][64];
  __shared__ double total[EV_Q];
  const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (q < EV_Q) {
    const int per = (n_tiles + 63) / 64;
    const int lo = lane * per, hi = min(lo + per, n_tiles);
    const double* p = partials + (size_t)q * n_tiles;
    double t = 0.0;
#pragma unroll 8
    for (int i = lo; i < hi; i++) t += p[i];
    chunk[q][lane] = t;
  }
  __syncthreads();
  if (q < EV_Q && lane == 0) {
    double t = 0.0;
    for (int l = 0; l < 64; l++) t += chunk[q][l];
    total[q] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double count = masked ? total[4] : n_elems;
  const double mse = (masked ? total[3] : total[1]) / count;  // empty mask: 0 / 0 = NaN, as the reference's mean of nothing
  out_row[0] = mse;
  out_row[1] = 20.0 * log10(1.0 / sqrt(mse));  // identical images: 1 / 0 = +inf
  out_row[2] = total[0] / n_elems;
  out_row[3] = total[2] / n_elems;
  out_row[4] = count;
  out_row[5] = out_row[6] = out_row[7] = 0.0;
}

}  // namespace

extern "C" {

int64_t gs_eval_partials_count(int32_t C, int32_t H, int32_t W) {
  if (C <= 0 || H <= 0 || W <= 0 || C > 4) return 0;
  return ev_tiles(C, H, W);
}

size_t gs_eval_tmp_bytes(int32_t C, int32_t H, int32_t W) {
  const int64_t n = gs_eval_partials_count(C, H, W);
  return n <= 0 ? 0 : gs_align((size_t)n * EV_Q * sizeof(double));
}

int gs_eval_metrics(const float* render, const float* gt, const float* mask, int32_t C, int32_t H, int32_t W, int32_t flags,
                    float C1, float C2, void* tmp, size_t tmp_bytes, double* out_row, uint8_t* quantised_out, void* stream) {
  if (!render || !gt || !tmp || !out_row) return GS_E_NULL;
  if ((flags & GS_EVAL_MASK_DTU) && !mask) return GS_E_NULL;
  if (C <= 0 || H <= 0 || W <= 0 || C > 4 || (flags & ~EV_ALL_FLAGS)) return GS_E_SHAPE;
  const int64_t n = ev_tiles(C, H, W);
  if (n > (int64_t)1 << 30 || tmp_bytes < gs_eval_tmp_bytes(C, H, W)) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)(((n + 7) / 8) * 8);
  hipLaunchKernelGGL(eval_tile_kernel, dim3(blocks), dim3(GS_BLOCK), 0, s, render, gt, mask, H, W, C, flags, C1, C2,
                     (double*)tmp, (int)n, quantised_out);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(GS_BLOCK * 2), 0, s, (const double*)tmp, (int)n,
                     (double)C * (double)H * (double)W, (flags & GS_EVAL_MASK_DTU) ? 1 : 0, out_row);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
