// gs_lpips.hip - LPIPS (VGG16, version 0.1, forward only) of a render against its ground truth on the device (gfx950, wave64),
// as the reference's lpipsPyTorch computes it for net_type='vgg' (lpipsPyTorch/modules/lpips.py:30-36, networks.py:50-63,88-96,
// utils.py:6-8), from weights the caller supplies.
//
// Activation layout: planar NCHW fp32 with N = 2, image 0 = the render, image 1 = the ground truth: [2][C][h][w], one layer
// in one ping-pong buffer.  It is torch's layout, so the stage entries take and return torch tensors as they are, and in the
// convolution a wave's 32 pixel lanes read and write 128 contiguous bytes of one row.
//
// lp_input_kernel     the pixel transform of the evaluation (gs_eval_px.h: clamp, 8-bit round trip, blend to white) on the
//                     first three channels of both images, then z_score: one fp32 subtraction and one fp32 division.
// lp_conv_kernel      conv3x3 (padding 1, stride 1) + bias + ReLU as an implicit GEMM on v_mfma_f32_32x32x2_f32, computed
//                     transposed as gs_mlp.hip does: the weights are the A operand (output channel on the row), the pixels the
//                     B operand (32 adjacent pixels of one image row on the lanes).  A workgroup of 4 waves owns TR rows x 32
//                     columns of ONE image and BN output channels; a wave owns TR / 4 rows and all BN channels
//                     (TR / 4 x BN / 32 accumulator tiles).  K runs over chunks of KC = 16 input channels (the 3-channel
//                     layer: one chunk of 4, the fourth channel all zero - its products add exactly 0); a chunk's (TR + 2) x 34
//                     input patch and its [KC][9][BN] weights are staged in LDS, and the chunk is summed as ONE fmaf chain from
//                     zero in the order   tap 0..8 (dy major), channel pair 0..KC/2-1, (even channel, odd channel)
//                     The chunk sums are added in chunk order, the bias last.  No split-K, no atomics: the same bits on
//                     every call, and an image's tiles are computed alike in either slot of the pair.
//                     Two shapes: 8 x 32 pixels x 64 channels (4 tiles per wave, 57.3 KiB LDS: two workgroups per CU), and, when
//                     that grid has fewer workgroups than the part has CUs (256), 4 x 32 pixels x 32 channels (one tile per
//                     wave, whose dependent-accumulator latency equals the instruction's issue interval; 30.8 KiB LDS).
// lp_pool_kernel      maxpool 2 x 2, stride 2, floor.
// lp_dist_kernel      a tap's distance: per pixel x / (sqrt(sum x^2) + 1e-10) of both images, sum_c lin[c] (x_c - y_c)^2, in
//                     float64 from the fp32 features on; 64 pixels per workgroup, its 4 waves take a quarter of the channels
//                     each and are added as (w0 + w1) + (w2 + w3), the pixels by one shuffle tree; one partial per workgroup.
// lp_finish_kernel    one workgroup adds the partials in index order (as eval_finish_kernel) and divides by the pixel count.
#include "gs_common.h"
#include "gs_eval_px.h"

namespace {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LP_CW = 32;          // tile columns = the MFMA's 32 pixel lanes
constexpr int LP_PC = LP_CW + 2;   // patch columns
constexpr int LP_CUS = 256;        // below this many workgroups the small tile shape is used
constexpr int LP_DPX = 64;         // pixels per workgroup of the distance kernel
constexpr int LP_EV_FLAGS = GS_EVAL_CLAMP | GS_EVAL_QUANTISE | GS_EVAL_MASK_DTU;
constexpr int LP_NCONV = 13, LP_NTAP = 5;
// VGG16's features up to relu5_3: (Cin, Cout) per convolution, and the number of convolutions in front of each tap
const int LP_CIN[LP_NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int LP_COUT[LP_NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int LP_BLOCK_CONVS[LP_NTAP] = {2, 2, 3, 3, 3};

inline int lp_cin_pad(int cin) { return cin == 3 ? 4 : cin; }
inline bool lp_pair_ok(int cin, int cout) {
  for (int i = 0; i < LP_NCONV; i++)
    if (LP_CIN[i] == cin && LP_COUT[i] == cout) return true;
  return false;
}

__global__ void __launch_bounds__(GS_BLOCK) lp_input_kernel(const float* __restrict__ render, const float* __restrict__ gt,
                                                            const float* __restrict__ mask, size_t HW, int flags,
                                                            float* __restrict__ out) {
  const size_t p = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (p >= HW) return;
  // networks.py:41-44: torch.Tensor([...]) rounds the literals to fp32
  const float mean[3] = {-.030f, -.088f, -.188f}, sd[3] = {.458f, .448f, .450f};
  const float m = (flags & GS_EVAL_MASK_DTU) ? mask[p] : 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float a = ev_transform(render[(size_t)c * HW + p], m, flags);
    const float b = ev_transform(gt[(size_t)c * HW + p], m, flags);
    out[(size_t)c * HW + p] = __fdiv_rn(__fsub_rn(a, mean[c]), sd[c]);
    out[(size_t)(3 + c) * HW + p] = __fdiv_rn(__fsub_rn(b, mean[c]), sd[c]);
  }
}

// w [Cout][Cin][3][3] (torch) -> out [CinPad][9][Cout], zero for the padding channel
__global__ void __launch_bounds__(GS_BLOCK) lp_pack_kernel(const float* __restrict__ w, int Cin, int CinPad, int Cout,
                                                           float* __restrict__ out) {
  const int i = blockIdx.x * GS_BLOCK + threadIdx.x;
  if (i >= CinPad * 9 * Cout) return;
  const int o = i % Cout, k = i / Cout, t = k % 9, c = k / 9;
  out[i] = c < Cin ? w[((size_t)o * Cin + c) * 9 + t] : 0.f;
}

template <int KC, int TR, int BN>
__global__ void __launch_bounds__(GS_BLOCK) lp_conv_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                           const float* __restrict__ bias, int Cin, int Cout, int H, int W,
                                                           int tilesX, int tilesY, float* __restrict__ y) {
  constexpr int PR = TR + 2, CS = PR * LP_PC, RW = TR / 4, NT = BN / 32;
  __shared__ float in_lds[KC * CS];
  __shared__ __attribute__((aligned(16))) float w_lds[KC * 9 * BN];
  const int ncb = Cout / BN;
  unsigned b = blockIdx.x;
  const int cb = (int)(b % ncb);
  b /= ncb;
  const int tx = (int)(b % tilesX);
  b /= tilesX;
  const int ty = (int)(b % tilesY);
  const int n = (int)(b / tilesY);
  const int x0 = tx * LP_CW, y0 = ty * TR;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const int CinPad = (Cin + KC - 1) / KC * KC;
  const float* xn = x + (size_t)n * Cin * H * W;

  lp_f32x16 tot[RW][NT];
#pragma unroll
  for (int rw = 0; rw < RW; rw++)
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
      for (int r = 0; r < 16; r++) tot[rw][nt][r] = 0.f;

  for (int c0 = 0; c0 < CinPad; c0 += KC) {
    // the chunk's input patch, zero outside the image (the convolution's padding) and for the padding channel
    for (int i = threadIdx.x; i < KC * CS; i += GS_BLOCK) {
      const int c = i / CS, rem = i - c * CS, r = rem / LP_PC, col = rem - r * LP_PC;
      const int gy = y0 + r - 1, gx = x0 + col - 1, ch = c0 + c;
      float v = 0.f;
      if (ch < Cin && gy >= 0 && gy < H && gx >= 0 && gx < W) v = xn[((size_t)ch * H + gy) * W + gx];
      in_lds[i] = v;
    }
    // the chunk's weights for this workgroup's channels: rows (c, tap) of the packed [CinPad][9][Cout]
    for (int i = threadIdx.x; i < KC * 9 * BN / 4; i += GS_BLOCK) {
      const int k = i / (BN / 4), q = i - k * (BN / 4);
      *reinterpret_cast<float4*>(&w_lds[k * BN + 4 * q]) =
          *reinterpret_cast<const float4*>(&wp[((size_t)c0 * 9 + k) * Cout + cb * BN + 4 * q]);
    }
    __syncthreads();
    lp_f32x16 part[RW][NT];
#pragma unroll
    for (int rw = 0; rw < RW; rw++)
#pragma unroll
      for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int r = 0; r < 16; r++) part[rw][nt][r] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; t++) {
      const int dy = t / 3, dx = t - 3 * dy;
#pragma unroll
      for (int cp = 0; cp < KC / 2; cp++) {
        const int c = 2 * cp + h;
        float av[NT], bv[RW];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) av[nt] = w_lds[(c * 9 + t) * BN + nt * 32 + j];
#pragma unroll
        for (int rw = 0; rw < RW; rw++) bv[rw] = in_lds[c * CS + (wv * RW + rw + dy) * LP_PC + j + dx];
#pragma unroll
        for (int rw = 0; rw < RW; rw++)
#pragma unroll
          for (int nt = 0; nt < NT; nt++)
            part[rw][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[nt], bv[rw], part[rw][nt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int rw = 0; rw < RW; rw++)
#pragma unroll
      for (int nt = 0; nt < NT; nt++) tot[rw][nt] += part[rw][nt];
    __syncthreads();  // every read of the chunk is done: the next chunk may overwrite it
  }
  // register r of a tile: output channel (r & 3) + 8 (r >> 2) + 4 h of the tile, pixel column j
  const int gx = x0 + j;
#pragma unroll
  for (int rw = 0; rw < RW; rw++) {
    const int gy = y0 + wv * RW + rw;
    if (gx >= W || gy >= H) continue;
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int o = cb * BN + nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        y[(((size_t)n * Cout + o) * H + gy) * W + gx] = fmaxf(__fadd_rn(tot[rw][nt][r], bias[o]), 0.f);
      }
  }
}

__global__ void __launch_bounds__(GS_BLOCK) lp_pool_kernel(const float* __restrict__ x, size_t NC, int H, int W, int Ho, int Wo,
                                                           float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (i >= NC * Ho * Wo) return;
  const int ox = (int)(i % Wo);
  const size_t q = i / Wo;
  const int oy = (int)(q % Ho);
  const size_t nc = q / Ho;
  const float* p = x + (nc * H + 2 * (size_t)oy) * W + 2 * ox;
  y[i] = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[W], p[W + 1]));
}

__global__ void __launch_bounds__(GS_BLOCK) lp_dist_kernel(const float* __restrict__ fx, const float* __restrict__ fy,
                                                           const double* __restrict__ lin, int C, size_t HW,
                                                           double* __restrict__ partials) {
  __shared__ double red[2][4][LP_DPX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t p = (size_t)blockIdx.x * LP_DPX + lane;
  const bool live = p < HW;
  const int per = (C + 3) / 4, lo = wv * per, hi = min(C, lo + per);
  double sx = 0.0, sy = 0.0;
  if (live) {
#pragma unroll 8
    for (int c = lo; c < hi; c++) {
      const double a = (double)fx[(size_t)c * HW + p], b = (double)fy[(size_t)c * HW + p];
      sx += a * a;
      sy += b * b;
    }
  }
  red[0][wv][lane] = sx;
  red[1][wv][lane] = sy;
  __syncthreads();
  // utils.py:6-8: x / (sqrt(sum x^2) + eps); a pixel whose channels are all zero gives 0 / 1e-10 = 0
  const double nx = sqrt((red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane])) + 1e-10;
  const double ny = sqrt((red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane])) + 1e-10;
  double acc = 0.0;
  if (live) {
#pragma unroll 8
    for (int c = lo; c < hi; c++) {
      const double d = (double)fx[(size_t)c * HW + p] / nx - (double)fy[(size_t)c * HW + p] / ny;
      acc += lin[c] * (d * d);
    }
  }
  __syncthreads();
  red[0][wv][lane] = acc;
  __syncthreads();
  if (wv != 0) return;
  double v = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) partials[blockIdx.x] = v;
}

// One workgroup of 64: lane l adds the l-th contiguous chunk of the partials in index order, lane 0 the 64 chunk sums in
// lane order.  out[tap] = the mean over the pixels; with `last`, out[5] = the sum of the five taps in tap order.
__global__ void __launch_bounds__(64) lp_finish_kernel(const double* __restrict__ partials, int n, double HW, int tap, int last,
                                                       double* __restrict__ out) {
  __shared__ double chunk[64];
  const int lane = threadIdx.x;
  const int per = (n + 63) / 64, lo = lane * per, hi = min(lo + per, n);
  double t = 0.0;
  for (int i = lo; i < hi; i++) t += partials[i];
  chunk[lane] = t;
  __syncthreads();
  if (lane != 0) return;
  t = 0.0;
  for (int l = 0; l < 64; l++) t += chunk[l];
  out[tap] = t / HW;
  if (last) out[5] = (((out[0] + out[1]) + out[2]) + out[3]) + out[4];
}

template <int KC>
int lp_conv_launch_kc(const float* x, const float* wp, const float* bias, int N, int Cin, int Cout, int H, int W, float* y,
                      hipStream_t s) {
  const int64_t tilesX = (W + LP_CW - 1) / LP_CW;
  const int64_t big = (int64_t)N * tilesX * ((H + 7) / 8) * (Cout / 64);
  if (big >= LP_CUS) {
    if (big > 0x7fffffff) return GS_E_SHAPE;
    hipLaunchKernelGGL((lp_conv_kernel<KC, 8, 64>), dim3((unsigned)big), dim3(GS_BLOCK), 0, s, x, wp, bias, Cin, Cout, H, W,
                       (int)tilesX, (H + 7) / 8, y);
  } else {
    const int64_t small = (int64_t)N * tilesX * ((H + 3) / 4) * (Cout / 32);
    hipLaunchKernelGGL((lp_conv_kernel<KC, 4, 32>), dim3((unsigned)small), dim3(GS_BLOCK), 0, s, x, wp, bias, Cin, Cout, H, W,
                       (int)tilesX, (H + 3) / 4, y);
  }
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int lp_conv_launch(const float* x, const float* wp, const float* bias, int N, int Cin, int Cout, int H, int W, float* y,
                   hipStream_t s) {
  return Cin == 3 ? lp_conv_launch_kc<4>(x, wp, bias, N, Cin, Cout, H, W, y, s)
                  : lp_conv_launch_kc<16>(x, wp, bias, N, Cin, Cout, H, W, y, s);
}

int lp_pool_launch(const float* x, int64_t NC, int H, int W, float* y, hipStream_t s) {
  const int Ho = H / 2, Wo = W / 2;
  const int64_t n = NC * Ho * Wo, blocks = (n + GS_BLOCK - 1) / GS_BLOCK;
  if (blocks > 0x7fffffff) return GS_E_SHAPE;
  hipLaunchKernelGGL(lp_pool_kernel, dim3((unsigned)blocks), dim3(GS_BLOCK), 0, s, x, (size_t)NC, H, W, Ho, Wo, y);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

inline int64_t lp_dist_blocks(int64_t HW) { return (HW + LP_DPX - 1) / LP_DPX; }

int lp_dist_launch(const float* fx, const float* fy, const double* lin, int C, int64_t HW, double* partials, int tap, int last,
                   double* out, hipStream_t s) {
  const int64_t blocks = lp_dist_blocks(HW);
  hipLaunchKernelGGL(lp_dist_kernel, dim3((unsigned)blocks), dim3(GS_BLOCK), 0, s, fx, fy, lin, C, (size_t)HW, partials);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(lp_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)partials, (int)blocks, (double)HW, tap, last, out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int lp_input_launch(const float* render, const float* gt, const float* mask, int H, int W, int flags, float* out, hipStream_t s) {
  const size_t HW = (size_t)H * W;
  hipLaunchKernelGGL(lp_input_kernel, dim3((unsigned)((HW + GS_BLOCK - 1) / GS_BLOCK)), dim3(GS_BLOCK), 0, s, render, gt, mask, HW,
                     flags, out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

inline bool lp_size_ok(int H, int W) { return H >= 16 && W >= 16 && (int64_t)H * W <= ((int64_t)1 << 24); }
inline size_t lp_act_bytes(int H, int W) { return gs_align((size_t)2 * 64 * H * W * sizeof(float)); }

}  // namespace

extern "C" {

int64_t gs_lpips_packed_floats(int32_t Cin, int32_t Cout) {
  return lp_pair_ok(Cin, Cout) ? (int64_t)lp_cin_pad(Cin) * 9 * Cout : 0;
}

int gs_lpips_pack_weights(const float* w, int32_t Cin, int32_t Cout, float* packed, void* stream) {
  if (!w || !packed) return GS_E_NULL;
  if (!lp_pair_ok(Cin, Cout)) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const int n = lp_cin_pad(Cin) * 9 * Cout;
  hipLaunchKernelGGL(lp_pack_kernel, dim3((n + GS_BLOCK - 1) / GS_BLOCK), dim3(GS_BLOCK), 0, s, w, Cin, lp_cin_pad(Cin), Cout,
                     packed);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_lpips_conv3x3_relu(const float* x, const float* packed_w, const float* bias, int32_t N, int32_t Cin, int32_t Cout,
                          int32_t H, int32_t W, float* y, void* stream) {
  if (!x || !packed_w || !bias || !y) return GS_E_NULL;
  if (N < 1 || H < 1 || W < 1 || !lp_pair_ok(Cin, Cout) || (((uintptr_t)packed_w) & 15)) return GS_E_SHAPE;
  if ((int64_t)N * (Cin > Cout ? Cin : Cout) * H * W >= ((int64_t)1 << 31)) return GS_E_SHAPE;
  return lp_conv_launch(x, packed_w, bias, N, Cin, Cout, H, W, y, (hipStream_t)stream);
}

int gs_lpips_maxpool2(const float* x, int64_t NC, int32_t H, int32_t W, float* y, void* stream) {
  if (!x || !y) return GS_E_NULL;
  if (NC < 1 || H < 2 || W < 2 || NC * H * W >= ((int64_t)1 << 31)) return GS_E_SHAPE;
  return lp_pool_launch(x, NC, H, W, y, (hipStream_t)stream);
}

size_t gs_lpips_distance_tmp_bytes(int32_t H, int32_t W) {
  if (H < 1 || W < 1) return 0;
  return gs_align((size_t)lp_dist_blocks((int64_t)H * W) * sizeof(double));
}

int gs_lpips_distance(const float* fx, const float* fy, const double* lin, int32_t C, int32_t H, int32_t W, void* tmp,
                      size_t tmp_bytes, double* out, void* stream) {
  if (!fx || !fy || !lin || !tmp || !out) return GS_E_NULL;
  if (C < 1 || H < 1 || W < 1 || (int64_t)C * H * W >= ((int64_t)1 << 31)) return GS_E_SHAPE;
  if (tmp_bytes < gs_lpips_distance_tmp_bytes(H, W)) return GS_E_SCRATCH;
  // (tap 0, not last: out[0] is the one word written)
  return lp_dist_launch(fx, fy, lin, C, (int64_t)H * W, (double*)tmp, 0, 0, out, (hipStream_t)stream);
}

size_t gs_lpips_tmp_bytes(int32_t H, int32_t W) {
  if (!lp_size_ok(H, W)) return 0;
  return 2 * lp_act_bytes(H, W) + gs_lpips_distance_tmp_bytes(H, W);
}

int gs_lpips_vgg(const float* render, const float* gt, const float* mask, int32_t C, int32_t H, int32_t W, int32_t flags,
                 const float* const* packed_w, const float* const* bias, const double* const* lin, void* tmp, size_t tmp_bytes,
                 double* out, void* stream) {
  if (!render || !gt || !packed_w || !bias || !lin || !tmp || !out) return GS_E_NULL;
  if ((flags & GS_EVAL_MASK_DTU) && !mask) return GS_E_NULL;
  for (int i = 0; i < LP_NCONV; i++)
    if (!packed_w[i] || !bias[i]) return GS_E_NULL;
  for (int i = 0; i < LP_NTAP; i++)
    if (!lin[i]) return GS_E_NULL;
  if (C < 3 || C > 4 || !lp_size_ok(H, W) || (flags & ~LP_EV_FLAGS)) return GS_E_SHAPE;
  for (int i = 0; i < LP_NCONV; i++)
    if (((uintptr_t)packed_w[i]) & 15) return GS_E_SHAPE;
  if (tmp_bytes < gs_lpips_tmp_bytes(H, W)) return GS_E_SCRATCH;
  hipStream_t s = (hipStream_t)stream;
  float* cur = (float*)((char*)tmp + lp_act_bytes(H, W));
  float* other = (float*)tmp;
  double* partials = (double*)((char*)tmp + 2 * lp_act_bytes(H, W));
  int rc = lp_input_launch(render, gt, mask, H, W, flags, cur, s);
  if (rc) return rc;
  int h = H, w = W, layer = 0;
  for (int tap = 0; tap < LP_NTAP; tap++) {
    if (tap > 0) {
      rc = lp_pool_launch(cur, (int64_t)2 * LP_COUT[layer - 1], h, w, other, s);
      if (rc) return rc;
      float* t = cur; cur = other; other = t;
      h /= 2;
      w /= 2;
    }
    for (int i = 0; i < LP_BLOCK_CONVS[tap]; i++, layer++) {
      rc = lp_conv_launch(cur, packed_w[layer], bias[layer], 2, LP_CIN[layer], LP_COUT[layer], h, w, other, s);
      if (rc) return rc;
      float* t = cur; cur = other; other = t;
    }
    const int Ct = LP_COUT[layer - 1];
    rc = lp_dist_launch(cur, cur + (size_t)Ct * h * w, lin[tap], Ct, (int64_t)h * w, partials, tap, tap == LP_NTAP - 1, out, s);
    if (rc) return rc;
  }
  return GS_OK;
}

}  // extern "C"
