// gs_mlp.hip - DNGaussian's per-Gaussian neural heads (scene/neural_renderer.py, GridRenderer), gfx950, wave64, f32 MFMA.
//
//   sigma_net  32 -> 64 -> 64 -> 65   bias-free, ReLU between; output column 0 = sigma, columns 1..64 = geo_feat
//   color_net  [enc_d 16 | geo_feat 64] -> 64 -> 3, colour = sigmoid(.) * 1.002 - 0.001
//
// Every product runs on v_mfma_f32_32x32x2_f32 (D[i][j] += A[i][k0] B[k0][j] + A[i][k1] B[k1][j], a k-ordered fmaf chain) and is
// computed TRANSPOSED, H^T = W X^T: the weight is the A operand (output feature i on the lane), the activations are the B
// operand (batch row j on the lane).  A 32 x 32 result tile then holds, in lane (j, h = lane >> 5) and register r,
//   feature rho(r) + 4 h of batch row j,        rho(r) = (r & 3) + 8 (r >> 2)
// which is exactly the B operand of the next layer's k-step r (k pair = features rho(r), rho(r) + 4): a layer's result feeds the
// next layer from registers, with no LDS round trip; the weight operand is fetched in that same permuted k order (hd_mm).
// Inputs are loaded from HBM straight into this layout (four consecutive features = one 16-byte load), outputs leave it the
// same way.  The thin outputs (sigma: 1 row, colour: 3 rows) are zero-padded 32-row tiles.
//
// A workgroup is four waves; a wave owns 32 batch rows of the workgroup's GS_DNG_HEADS_TILE_ROWS-row tile; workgroups are
// persistent and stride over the tiles (the caller may cap the grid: max_blocks).  All five weights sit in LDS in torch's [out][in] layout with an odd row stride (in + 1),
// so that both the forward's fetch (lane = out) and the backward's (lane = in, A = W^T) are spread over the banks.
//
// forward  = 1 launch (hd_fwd_kernel): writes sigma [B] and colour [B,3], nothing else.
// backward = 1 launch (hd_bwd_kernel) + hd_reduce_kernel.  It recomputes the forward of its tile, back-propagates through the
//   transposed weights in the same register layout, and forms the weight gradients dW = dY^T X (K = batch rows) per matrix in a
//   ROUND: the four waves write dY and X of their rows to an LDS image [128 rows][HD_SW], and each wave then runs the 32 x 32
//   tiles of dW assigned to it over all 128 rows, accumulating in registers across the workgroup's tiles (five accumulators per
//   wave).  At the end every workgroup writes its partial [15616] to tmp; hd_reduce_kernel adds the partials in workgroup
//   order.  No atomics: the same inputs give the same bits.  ReLU'(0) = 0.
#include "gs_common.h"
#include "gs_launch.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define HD_X GS_DNG_ENC_X
#define HD_D GS_DNG_ENC_D
#define HD_H GS_DNG_HIDDEN
#define HD_G GS_DNG_GEO
#define HD_CIN (HD_D + HD_G)
static_assert(HD_X == 32 && HD_D == 16 && HD_H == 64 && HD_G == 64, "the tiling below is written for DNGaussian's widths");
static_assert(GS_DNG_HEADS_TILE_ROWS == 128 && GS_BLOCK == 256, "four waves of 32 rows");

// LDS rows of the weights: [out][in + 1]
#define S_S0 (HD_X + 1)
#define S_S1 (HD_H + 1)
#define S_S2 (HD_H + 1)
#define S_C0 (HD_CIN + 1)
#define S_C1 (HD_H + 1)
#define L_S0 0
#define L_S1 (L_S0 + HD_H * S_S0)
#define L_S2 (L_S1 + HD_H * S_S1)
#define L_C0 (L_S2 + (1 + HD_G) * S_S2)
#define L_C1 (L_C0 + HD_H * S_C0)
#define L_END (L_C1 + 3 * S_C1)
static_assert(L_END % 4 == 0, "the staging image behind the weights is 16-byte aligned");
// the concatenated weight gradient (one partial per workgroup): w_s0 | w_s1 | w_s2 | w_c0 | w_c1
#define G_S0 0
#define G_S1 (G_S0 + HD_H * HD_X)
#define G_S2 (G_S1 + HD_H * HD_H)
#define G_C0 (G_S2 + (1 + HD_G) * HD_H)
#define G_C1 (G_C0 + HD_H * HD_CIN)
#define G_END (G_C1 + 3 * HD_H)
static_assert(G_END == 15616, "15 616 weights");
// the backward's LDS image of one round: [128 rows][HD_SW], dY columns first, then X (largest round: 64 + 16 + 64)
#define HD_SW 180
static_assert((L_END + GS_DNG_HEADS_TILE_ROWS * HD_SW) * 4 <= 160 * 1024, "weights + one round fit the CU's 160 KB of LDS");

struct HdArgs {
  const float* enc_x;
  const float* enc_d;
  int64_t B;
  int64_t ntiles;
  const float* w[5];  // s0 s1 s2 c0 c1
  float* sigma;
  float* color;
  const float* g_sigma;
  const float* g_color;
  float* g_enc_x;
  float* g_enc_d;
  float* part;  // [gridDim.x][G_END] or NULL: no weight gradients
  int vec;      // every row pointer is 16-byte aligned
};

struct HdAct {
  float x[16], d[8], h0[32], h1[32], geo[32], hc[32];
  float sig, cp[3];  // sigma and the colour pre-activations: valid on the lanes with h = 0
};

__device__ __forceinline__ void hd_load_weights(float* W, const HdArgs& a, bool color) {
  const int t = threadIdx.x;
  for (int e = t; e < HD_H * HD_X; e += GS_BLOCK) W[L_S0 + (e / HD_X) * S_S0 + e % HD_X] = a.w[0][e];
  for (int e = t; e < HD_H * HD_H; e += GS_BLOCK) W[L_S1 + (e / HD_H) * S_S1 + e % HD_H] = a.w[1][e];
  for (int e = t; e < (1 + HD_G) * HD_H; e += GS_BLOCK) W[L_S2 + (e / HD_H) * S_S2 + e % HD_H] = a.w[2][e];
  if (color) {
    for (int e = t; e < HD_H * HD_CIN; e += GS_BLOCK) W[L_C0 + (e / HD_CIN) * S_C0 + e % HD_CIN] = a.w[3][e];
    for (int e = t; e < 3 * HD_H; e += GS_BLOCK) W[L_C1 + (e / HD_H) * S_C1 + e % HD_H] = a.w[4][e];
  }
}

// feature of register group r4 (registers 4 r4 .. 4 r4 + 3 of an activation in tile layout) in lane half h
__device__ __forceinline__ int hd_feat(int r4, int h) { return 32 * (r4 >> 2) + 8 * (r4 & 3) + 4 * h; }

// NR features of row `row` of p [B][ld] -> v in tile layout (zeros for a row beyond B)
template <int NR>
__device__ __forceinline__ void hd_load(const float* p, int ld, size_t row, bool ok, int h, int vec, float* v) {
#pragma unroll
  for (int r4 = 0; r4 < NR / 4; r4++) {
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
      const float* s = p + row * ld + hd_feat(r4, h);
      if (vec) q = *reinterpret_cast<const float4*>(s);
      else q = make_float4(s[0], s[1], s[2], s[3]);
    }
    v[4 * r4] = q.x; v[4 * r4 + 1] = q.y; v[4 * r4 + 2] = q.z; v[4 * r4 + 3] = q.w;
  }
}

template <int NR>
__device__ __forceinline__ void hd_store(float* p, int ld, size_t row, bool ok, int h, int vec, const float* v) {
  if (!ok) return;
#pragma unroll
  for (int r4 = 0; r4 < NR / 4; r4++) {
    float* s = p + row * ld + hd_feat(r4, h);
    if (vec) *reinterpret_cast<float4*>(s) = make_float4(v[4 * r4], v[4 * r4 + 1], v[4 * r4 + 2], v[4 * r4 + 3]);
    else { s[0] = v[4 * r4]; s[1] = v[4 * r4 + 1]; s[2] = v[4 * r4 + 2]; s[3] = v[4 * r4 + 3]; }
  }
}

// acc += A B over NS k-steps.  B = b[0 .. NS) in tile layout (step s: features k = 32 (s >> 4) + rho(s & 15) + 4 h of the
// lane's batch row); A[i][k] = w[i * si + k * sk] for i < ni, k < nk, else 0.  (si, sk) = (row stride, 1): A = W, the forward;
// (1, row stride): A = W^T, the backward.
template <int NS>
__device__ __forceinline__ f32x16 hd_mm(f32x16 acc, const float* w, int si, int sk, int i, int ni, int nk, int h, const float* b) {
#pragma unroll
  for (int s = 0; s < NS; s++) {
    const int k = 32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2) + 4 * h;
    const float av = (i < ni && k < nk) ? w[i * si + k * sk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[s], acc, 0, 0, 0);
  }
  return acc;
}

__device__ __forceinline__ f32x16 hd_zero() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; r++) z[r] = 0.f;
  return z;
}

__device__ __forceinline__ float hd_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// the heads of the lane's batch row: sigma_net always, geo_feat and the colour net with `color`
template <bool COLOR>
__device__ __forceinline__ void hd_forward(const float* W, const HdArgs& a, size_t row, bool ok, int l31, int h, HdAct& t) {
  hd_load<16>(a.enc_x, HD_X, row, ok, h, a.vec, t.x);
#pragma unroll
  for (int m = 0; m < 2; m++) {
    const f32x16 acc = hd_mm<16>(hd_zero(), W + L_S0 + 32 * m * S_S0, S_S0, 1, l31, 32, HD_X, h, t.x);
#pragma unroll
    for (int r = 0; r < 16; r++) t.h0[16 * m + r] = fmaxf(acc[r], 0.f);
  }
#pragma unroll
  for (int m = 0; m < 2; m++) {
    const f32x16 acc = hd_mm<32>(hd_zero(), W + L_S1 + 32 * m * S_S1, S_S1, 1, l31, 32, HD_H, h, t.h0);
#pragma unroll
    for (int r = 0; r < 16; r++) t.h1[16 * m + r] = fmaxf(acc[r], 0.f);
  }
  {  // sigma: row 0 of w_s2, a tile with one live row
    const f32x16 acc = hd_mm<32>(hd_zero(), W + L_S2, S_S2, 1, l31, 1, HD_H, h, t.h1);
    t.sig = acc[0];
  }
  if (COLOR) {
    hd_load<8>(a.enc_d, HD_D, row, ok, h, a.vec, t.d);
#pragma unroll
    for (int m = 0; m < 2; m++) {  // geo_feat: rows 1 .. 64 of w_s2
      const f32x16 acc = hd_mm<32>(hd_zero(), W + L_S2 + (1 + 32 * m) * S_S2, S_S2, 1, l31, 32, HD_H, h, t.h1);
#pragma unroll
      for (int r = 0; r < 16; r++) t.geo[16 * m + r] = acc[r];
    }
#pragma unroll
    for (int m = 0; m < 2; m++) {  // colour net, layer 0: input = [enc_d | geo_feat]
      f32x16 acc = hd_mm<8>(hd_zero(), W + L_C0 + 32 * m * S_C0, S_C0, 1, l31, 32, HD_D, h, t.d);
      acc = hd_mm<32>(acc, W + L_C0 + 32 * m * S_C0 + HD_D, S_C0, 1, l31, 32, HD_G, h, t.geo);
#pragma unroll
      for (int r = 0; r < 16; r++) t.hc[16 * m + r] = fmaxf(acc[r], 0.f);
    }
    const f32x16 acc = hd_mm<32>(hd_zero(), W + L_C1, S_C1, 1, l31, 3, HD_H, h, t.hc);
    t.cp[0] = acc[0]; t.cp[1] = acc[1]; t.cp[2] = acc[2];
  }
}

template <bool COLOR>
__global__ __launch_bounds__(GS_BLOCK) void hd_fwd_kernel(HdArgs a) {
  __shared__ __attribute__((aligned(16))) float W[L_END];
  hd_load_weights(W, a, COLOR);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row = tile * GS_DNG_HEADS_TILE_ROWS + wave * 32 + l31;
    const bool ok = row < a.B;
    HdAct t;
    hd_forward<COLOR>(W, a, (size_t)row, ok, l31, h, t);
    if (ok && h == 0) {
      a.sigma[row] = t.sig;
      if (COLOR) {
#pragma unroll
        for (int o = 0; o < 3; o++) a.color[row * 3 + o] = hd_sigmoid(t.cp[o]) * 1.002f - 0.001f;
      }
    }
  }
}

// ---- backward ----
// NR registers of an activation in tile layout -> columns col .. of the lane's row of the round's LDS image
template <int NR>
__device__ __forceinline__ void hd_stage(float* st, int srow, int col, int h, const float* v) {
#pragma unroll
  for (int r4 = 0; r4 < NR / 4; r4++)
    *reinterpret_cast<float4*>(st + srow * HD_SW + col + hd_feat(r4, h)) =
        make_float4(v[4 * r4], v[4 * r4 + 1], v[4 * r4 + 2], v[4 * r4 + 3]);
}

// one 32 x 32 tile of dW = dY^T X over the 128 staged rows: acc[out][in] += sum_row dY[row][ycol + out] X[row][xcol + in]
__device__ __forceinline__ f32x16 hd_dw(f32x16 acc, const float* st, int ycol, int ny, int xcol, int nx, int l31, int h) {
  const float* pa = st + h * HD_SW + ycol + l31;
  const float* pb = st + h * HD_SW + xcol + l31;
  const bool va = l31 < ny, vb = l31 < nx;
#pragma unroll 8
  for (int s = 0; s < GS_DNG_HEADS_TILE_ROWS / 2; s++) {
    const float av = va ? pa[2 * s * HD_SW] : 0.f;
    const float bv = vb ? pb[2 * s * HD_SW] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  }
  return acc;
}

// a finished tile of dW -> the workgroup's partial: rows orow .. of a [.][ld] matrix at woff, columns ocol ..
__device__ __forceinline__ void hd_put(float* part, const f32x16& acc, int woff, int ld, int orow, int ny, int ocol, int nx, int l31,
                                       int h) {
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (o < ny && l31 < nx) part[woff + (orow + o) * ld + ocol + l31] = acc[r];
  }
}

template <bool COLOR>
__global__ __launch_bounds__(GS_BLOCK) void hd_bwd_kernel(HdArgs a) {
  __shared__ __attribute__((aligned(16))) float W[L_END + GS_DNG_HEADS_TILE_ROWS * HD_SW];
  float* st = W + L_END;
  hd_load_weights(W, a, COLOR);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
  const int srow = wave * 32 + l31;
  const bool want_w = a.part != nullptr;
  // the wave's five tiles of the weight gradient (the rounds below say which):
  //   A  w_c0 tile `wave` of six (m = t & 1: rows 32 m ..; n = t >> 1: enc_d columns, geo columns 0 .. 31, 32 .. 63)
  //   B  waves 0, 1: w_c0 tiles 4, 5;  waves 2, 3: w_c1 columns 32 (wave - 2) ..
  //   C  w_s2 rows 1 + 32 m .., columns 32 n ..  (t = wave)
  //   D  waves 0, 1: w_s2 row 0 (sigma), columns 32 wave ..;  waves 2, 3: w_s0 rows 32 (wave - 2) ..
  //   E  w_s1 rows 32 m .., columns 32 n ..  (t = wave)
  f32x16 accA = hd_zero(), accB = hd_zero(), accC = hd_zero(), accD = hd_zero(), accE = hd_zero();
  const int tm = wave & 1, tn = wave >> 1;

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row = tile * GS_DNG_HEADS_TILE_ROWS + srow;
    const bool ok = row < a.B;
    HdAct t;
    hd_forward<COLOR>(W, a, (size_t)row, ok, l31, h, t);
    const float gs = (ok && h == 0 && a.g_sigma) ? a.g_sigma[row] : 0.f;
    float ggeo[32];
    if (COLOR) {
      float gc[4] = {0.f, 0.f, 0.f, 0.f};
      if (ok && h == 0) {
#pragma unroll
        for (int o = 0; o < 3; o++) {
          const float s = hd_sigmoid(t.cp[o]);
          gc[o] = a.g_color[row * 3 + o] * 1.002f * (s * (1.f - s));
        }
      }
      float ghc[32];
#pragma unroll
      for (int m = 0; m < 2; m++) {  // through w_c1^T: K = 3
        const f32x16 acc = hd_mm<3>(hd_zero(), W + L_C1 + 32 * m, 1, S_C1, l31, 32, 3, h, gc);
#pragma unroll
        for (int r = 0; r < 16; r++) ghc[16 * m + r] = t.hc[16 * m + r] > 0.f ? acc[r] : 0.f;
      }
      if (want_w) {
        // round w_c1: dY = the colour pre-activation gradients (3, padded to 4), X = hc
        if (h == 0) *reinterpret_cast<float4*>(st + srow * HD_SW) = make_float4(gc[0], gc[1], gc[2], 0.f);
        hd_stage<32>(st, srow, 4, h, t.hc);
        __syncthreads();
        if (wave >= 2) accB = hd_dw(accB, st, 0, 3, 4 + 32 * (wave - 2), 32, l31, h);
        __syncthreads();
        // round w_c0: dY = ghc, X = [enc_d | geo]
        hd_stage<32>(st, srow, 0, h, ghc);
        hd_stage<8>(st, srow, 64, h, t.d);
        hd_stage<32>(st, srow, 80, h, t.geo);
        __syncthreads();
        accA = hd_dw(accA, st, 32 * tm, 32, tn == 0 ? 64 : 80, tn == 0 ? HD_D : 32, l31, h);
        if (wave < 2) accB = hd_dw(accB, st, 32 * tm, 32, 80 + 32, 32, l31, h);
        __syncthreads();
      }
      if (a.g_enc_d) {
        const f32x16 acc = hd_mm<32>(hd_zero(), W + L_C0, 1, S_C0, l31, HD_D, HD_H, h, ghc);
        float gd[8];
#pragma unroll
        for (int r = 0; r < 8; r++) gd[r] = acc[r];
        hd_store<8>(a.g_enc_d, HD_D, (size_t)row, ok, h, a.vec, gd);
      }
#pragma unroll
      for (int m = 0; m < 2; m++) {
        const f32x16 acc = hd_mm<32>(hd_zero(), W + L_C0 + HD_D + 32 * m, 1, S_C0, l31, 32, HD_H, h, ghc);
#pragma unroll
        for (int r = 0; r < 16; r++) ggeo[16 * m + r] = acc[r];
      }
    }
    const float gsv[1] = {gs};
    if (want_w) {
      // round w_s2: dY = [g_geo | g_sigma (1, padded to 4)], X = h1
      if (COLOR) hd_stage<32>(st, srow, 0, h, ggeo);
      if (h == 0) *reinterpret_cast<float4*>(st + srow * HD_SW + 64) = make_float4(gs, 0.f, 0.f, 0.f);
      hd_stage<32>(st, srow, 68, h, t.h1);
      __syncthreads();
      if (COLOR) accC = hd_dw(accC, st, 32 * tm, 32, 68 + 32 * tn, 32, l31, h);
      if (wave < 2) accD = hd_dw(accD, st, 64, 1, 68 + 32 * wave, 32, l31, h);
      __syncthreads();
    }
    float gh1[32];
#pragma unroll
    for (int m = 0; m < 2; m++) {  // through w_s2^T: K = 64 geo rows + the sigma row
      f32x16 acc = hd_zero();
      if (COLOR) acc = hd_mm<32>(acc, W + L_S2 + S_S2 + 32 * m, 1, S_S2, l31, 32, HD_G, h, ggeo);
      acc = hd_mm<1>(acc, W + L_S2 + 32 * m, 1, S_S2, l31, 32, 1, h, gsv);
#pragma unroll
      for (int r = 0; r < 16; r++) gh1[16 * m + r] = t.h1[16 * m + r] > 0.f ? acc[r] : 0.f;
    }
    if (want_w) {
      // round w_s1: dY = gh1, X = h0
      hd_stage<32>(st, srow, 0, h, gh1);
      hd_stage<32>(st, srow, 64, h, t.h0);
      __syncthreads();
      accE = hd_dw(accE, st, 32 * tm, 32, 64 + 32 * tn, 32, l31, h);
      __syncthreads();
    }
    float gh0[32];
#pragma unroll
    for (int m = 0; m < 2; m++) {
      const f32x16 acc = hd_mm<32>(hd_zero(), W + L_S1 + 32 * m, 1, S_S1, l31, 32, HD_H, h, gh1);
#pragma unroll
      for (int r = 0; r < 16; r++) gh0[16 * m + r] = t.h0[16 * m + r] > 0.f ? acc[r] : 0.f;
    }
    if (want_w) {
      // round w_s0: dY = gh0, X = enc_x
      hd_stage<32>(st, srow, 0, h, gh0);
      hd_stage<16>(st, srow, 64, h, t.x);
      __syncthreads();
      if (wave >= 2) accD = hd_dw(accD, st, 32 * (wave - 2), 32, 64, 32, l31, h);
      __syncthreads();
    }
    if (a.g_enc_x) {
      const f32x16 acc = hd_mm<32>(hd_zero(), W + L_S0, 1, S_S0, l31, HD_X, HD_H, h, gh0);
      float gx[16];
#pragma unroll
      for (int r = 0; r < 16; r++) gx[r] = acc[r];
      hd_store<16>(a.g_enc_x, HD_X, (size_t)row, ok, h, a.vec, gx);
    }
  }

  if (want_w) {
    float* part = a.part + (size_t)blockIdx.x * G_END;
    if (COLOR) {
      hd_put(part, accA, G_C0, HD_CIN, 32 * tm, 32, tn == 0 ? 0 : HD_D, tn == 0 ? HD_D : 32, l31, h);
      if (wave < 2) hd_put(part, accB, G_C0, HD_CIN, 32 * tm, 32, HD_D + 32, 32, l31, h);
      else hd_put(part, accB, G_C1, HD_H, 0, 3, 32 * (wave - 2), 32, l31, h);
    }
    hd_put(part, accC, G_S2, HD_H, 1 + 32 * tm, 32, 32 * tn, 32, l31, h);
    if (wave < 2) hd_put(part, accD, G_S2, HD_H, 0, 1, 32 * wave, 32, l31, h);
    else hd_put(part, accD, G_S0, HD_X, 32 * (wave - 2), 32, 0, 32, l31, h);
    hd_put(part, accE, G_S1, HD_H, 32 * tm, 32, 32 * tn, 32, l31, h);
  }
}

struct HdOut {
  float* g[5];
};

// weight gradient = the workgroups' partials added in workgroup order; without colour partials w_c0 / w_c1 (if asked for) are zero
__global__ __launch_bounds__(GS_BLOCK) void hd_reduce_kernel(const float* part, int nparts, int color_parts, HdOut out) {
  const int e = blockIdx.x * GS_BLOCK + threadIdx.x;
  if (e >= G_END) return;
  float s = 0.f;
  if (e < G_C0 || color_parts)
    for (int b = 0; b < nparts; b++) s += part[(size_t)b * G_END + e];
  const int w = e < G_S1 ? 0 : e < G_S2 ? 1 : e < G_C0 ? 2 : e < G_C1 ? 3 : 4;
  const int base = w == 0 ? G_S0 : w == 1 ? G_S1 : w == 2 ? G_S2 : w == 3 ? G_C0 : G_C1;
  if (out.g[w]) out.g[w][e - base] = s;
}

// ---- host side ----
#define HD_MAX_ROWS ((int64_t)1 << 40)

static int64_t hd_tiles(int64_t B) { return (B + GS_DNG_HEADS_TILE_ROWS - 1) / GS_DNG_HEADS_TILE_ROWS; }

}  // namespace

extern "C" {

size_t gs_dng_heads_tmp_bytes(int64_t B) {
  if (B <= 0 || B > HD_MAX_ROWS) return 0;
  return gs_align((size_t)gs_capped_blocks((size_t)B, GS_DNG_HEADS_TILE_ROWS, GS_DNG_HEADS_MAX_BLOCKS) * G_END * sizeof(float));
}

int gs_dng_heads_fwd(const float* enc_x, const float* enc_d, int64_t B, const float* w_s0, const float* w_s1, const float* w_s2,
                     const float* w_c0, const float* w_c1, float* sigma, float* color, int32_t max_blocks, void* stream) {
  if (B < 0 || B > HD_MAX_ROWS || max_blocks < 0) return GS_E_SHAPE;
  if (B == 0) return GS_OK;
  const bool col = enc_d != nullptr || color != nullptr;
  if (!enc_x || !w_s0 || !w_s1 || !w_s2 || !sigma) return GS_E_NULL;
  if (col && (!enc_d || !color || !w_c0 || !w_c1)) return GS_E_NULL;
  HdArgs a = {};
  a.enc_x = enc_x; a.enc_d = enc_d; a.B = B; a.ntiles = hd_tiles(B);
  a.w[0] = w_s0; a.w[1] = w_s1; a.w[2] = w_s2; a.w[3] = w_c0; a.w[4] = w_c1;
  a.sigma = sigma; a.color = color;
  a.vec = gs_aligned16(enc_x) && gs_aligned16(enc_d);
  hipStream_t s = (hipStream_t)stream;
  // one workgroup per CU for the colour form (370 registers: one wave per SIMD, so a second workgroup would only reload the
  // weights); the sigma-only form runs two waves per SIMD and its 62 KB of LDS fit twice: two workgroups per CU
  const dim3 grid((unsigned)gs_capped_blocks((size_t)a.ntiles, 1, (col ? 1 : 2) * (size_t)GS_DNG_HEADS_MAX_BLOCKS, max_blocks));
  if (col) hipLaunchKernelGGL(hd_fwd_kernel<true>, grid, dim3(GS_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(hd_fwd_kernel<false>, grid, dim3(GS_BLOCK), 0, s, a);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_dng_heads_bwd(const float* enc_x, const float* enc_d, int64_t B, const float* w_s0, const float* w_s1, const float* w_s2,
                     const float* w_c0, const float* w_c1, const float* g_sigma, const float* g_color, float* g_enc_x,
                     float* g_enc_d, float* g_w_s0, float* g_w_s1, float* g_w_s2, float* g_w_c0, float* g_w_c1, void* tmp,
                     size_t tmp_bytes, int32_t max_blocks, void* stream) {
  if (B < 0 || B > HD_MAX_ROWS || max_blocks < 0) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  HdOut out = {{g_w_s0, g_w_s1, g_w_s2, g_w_c0, g_w_c1}};
  const size_t wn[5] = {HD_H * HD_X, HD_H * HD_H, (1 + HD_G) * HD_H, HD_H * HD_CIN, 3 * HD_H};
  if (B == 0) {  // no rows: the weight gradients are zero
    for (int i = 0; i < 5; i++)
      if (out.g[i]) GS_HIP_CHECK(hipMemsetAsync(out.g[i], 0, wn[i] * sizeof(float), s));
    return GS_OK;
  }
  if (!enc_x || !w_s0 || !w_s1 || !w_s2) return GS_E_NULL;
  if (enc_d && (!w_c0 || !w_c1)) return GS_E_NULL;
  if (!enc_d && (g_color || g_enc_d || g_w_c0 || g_w_c1)) return GS_E_NULL;
  const bool want_w = g_w_s0 || g_w_s1 || g_w_s2 || g_w_c0 || g_w_c1;
  if (want_w && (!g_w_s0 || !g_w_s1 || !g_w_s2 || (enc_d && (!g_w_c0 || !g_w_c1)))) return GS_E_NULL;  // all together
  if (!want_w && !g_enc_x && !g_enc_d) return GS_E_NULL;
  if (want_w && (!tmp || tmp_bytes < gs_dng_heads_tmp_bytes(B))) return tmp ? GS_E_SHAPE : GS_E_NULL;
  if (!g_sigma && !g_color) {  // nothing flows in: every requested gradient is zero
    for (int i = 0; i < 5; i++)
      if (out.g[i]) GS_HIP_CHECK(hipMemsetAsync(out.g[i], 0, wn[i] * sizeof(float), s));
    if (g_enc_x) GS_HIP_CHECK(hipMemsetAsync(g_enc_x, 0, (size_t)B * HD_X * sizeof(float), s));
    if (g_enc_d) GS_HIP_CHECK(hipMemsetAsync(g_enc_d, 0, (size_t)B * HD_D * sizeof(float), s));
    return GS_OK;
  }
  const bool col = enc_d != nullptr && g_color != nullptr;
  if (!col && g_enc_d) GS_HIP_CHECK(hipMemsetAsync(g_enc_d, 0, (size_t)B * HD_D * sizeof(float), s));
  HdArgs a = {};
  a.enc_x = enc_x; a.enc_d = col ? enc_d : nullptr; a.B = B; a.ntiles = hd_tiles(B);
  a.w[0] = w_s0; a.w[1] = w_s1; a.w[2] = w_s2; a.w[3] = w_c0; a.w[4] = w_c1;
  a.g_sigma = g_sigma; a.g_color = col ? g_color : nullptr;
  a.g_enc_x = g_enc_x; a.g_enc_d = col ? g_enc_d : nullptr;
  a.part = want_w ? (float*)tmp : nullptr;
  a.vec = gs_aligned16(enc_x) && gs_aligned16(enc_d) && gs_aligned16(g_enc_x) && gs_aligned16(g_enc_d);
  const int nb = gs_capped_blocks((size_t)a.ntiles, 1, GS_DNG_HEADS_MAX_BLOCKS, max_blocks);
  if (col) hipLaunchKernelGGL(hd_bwd_kernel<true>, dim3(nb), dim3(GS_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(hd_bwd_kernel<false>, dim3(nb), dim3(GS_BLOCK), 0, s, a);
  GS_LAUNCH_CHECK(s, 0);
  if (want_w) {
    hipLaunchKernelGGL(hd_reduce_kernel, dim3((G_END + GS_BLOCK - 1) / GS_BLOCK), dim3(GS_BLOCK), 0, s, (const float*)tmp, nb,
                       col ? 1 : 0, out);
    GS_LAUNCH_CHECK(s, 0);
  }
  return GS_OK;
}

}  // extern "C"
