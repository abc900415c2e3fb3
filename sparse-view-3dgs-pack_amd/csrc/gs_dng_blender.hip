// gs_dng_blender.hip - what DNGaussian's Blender loops (train_blender.py, `training` and `training_sh`) add for a white
// background, gfx950, wave64:
//   the background mask of a ground-truth image and the mono-depth target zeroed under it (:87, :96-97, :123-124, :286, :295-296),
//   the white rule around a densification (:207-211, :366-370), on a given per-Gaussian colour or on the colour of the SH rows.
// In the reference each is boolean-index arithmetic (the white rule's gathers through a boolean mask are a nonzero and a host
// stall each; `x[mask] = 0` is a masked fill and does not stall); here every count stays in device memory.  No floating-point
// atomics (the one atomic is an integer add per workgroup in the two rules), no read-back, no host synchronisation: two runs
// give the same bits.
//
// target (gt [3,H,W], mono [H,W] or null, thr), TWO launches: bt_mask_kernel, a grid of at most BL_MAX_BLOCKS workgroups, block b
//   sweeping the chunks b, b + G, ... of BL_BLOCK_ELEMS pixels; in each of a chunk's BL_ELEMS steps lane t takes pixel
//   t + k GS_BLOCK, so every load and store instruction of a wave covers 64 consecutive elements of its plane whatever the
//   planes' alignment.  mask = min over the channels > thr, strictly, in fp32; a NaN channel leaves the pixel unmasked (torch's
//   min hands the NaN on and the comparison is false).  target = +0.0 where masked, else 255.0f - mono: one fp32 subtraction.
//   The workgroup's masked count goes through an integer LDS tree into its partial; bt_count_kernel, one workgroup, adds the
//   partials (integers: any order gives the same value).
// white rule (colour [P,3], statistic [P], raw opacity [P]): a row fires iff min_c colour > thr, strictly, fp32, a NaN fires
//   nothing.  A firing row gets statistic = +0.0 and raw opacity = log(x / (1 - x)), x = factor * sigmoid(opacity), evaluated in
//   double from the fp32 input and rounded once (-inf in: x = 0 and -inf out; NaN in: NaN out).
// white rule, SH form: the colour is render_sh's (gaussian_renderer/__init__.py:351-355): dir = xyz - campos, normalised;
//   colour = max(eval_sh(active degree, rows, dir) + 0.5, 0), evaluated in double from the fp32 inputs and rounded once (the SH
//   encoder kernels do the same).  A Gaussian on the camera centre has 0 / 0 = NaN directions, NaN colours, and fires nothing -
//   from degree 1 on: degree 0 does not look at the direction, in eval_sh as here.  The rows come split (dc [P,1,3] +
//   rest [P,M-1,3]) or packed ([P,M,3]); only the coefficients of the active degree are fetched, a workgroup's block of them
//   through LDS so that neighbouring lanes read neighbouring addresses (a lane's own row is 12 M bytes away from its
//   neighbour's).
// Both rules count the same way, in ONE kernel launch behind a 4-byte hipMemsetAsync of counts[0] on the same stream: every
//   workgroup sums its rows' decisions through an integer LDS tree and adds the sum with one integer atomicAdd.  Integer adds
//   commute: the value does not depend on their order.  (A counting workgroup that walks all P rows alone needs no memset but
//   is the launch's long pole - with the SH colours to evaluate it is slower than torch's own statements.)
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_reduce.h"

namespace {

#define BL_ELEMS 4  // pixels per lane and chunk
#define BL_BLOCK_ELEMS (BL_ELEMS * GS_BLOCK)
#define BL_MAX_BLOCKS 256
#define BL_MAX_N ((int64_t)1 << 31)  // pixels of an image, rows of a model (the counts are int32)
#define BL_MAX_COEF 16
#define BL_LDS_STRIDE (3 * BL_MAX_COEF + 1)  // odd: a lane's row starts in its own bank

static_assert(BL_MAX_BLOCKS <= GS_BLOCK, "the partial counts fit one workgroup's LDS array");

__device__ __forceinline__ bool bl_white(float r, float g, float b, float thr) {
  // torch's min over the channels hands a NaN on; a NaN does not pass the comparison
  const bool nan = r != r || g != g || b != b;
  float mn = r;
  mn = g < mn ? g : mn;
  mn = b < mn ? b : mn;
  return !nan && mn > thr;
}

__global__ __launch_bounds__(GS_BLOCK) void bt_mask_kernel(const float* gt, const float* mono, size_t n, float thr, int nblocks,
                                                           uint8_t* mask, float* target, int32_t* part) {
  __shared__ int sh[GS_BLOCK];
  const int t = threadIdx.x;
  int masked = 0;
  for (size_t base = (size_t)blockIdx.x * BL_BLOCK_ELEMS; base < n; base += (size_t)nblocks * BL_BLOCK_ELEMS) {
    for (int k = 0; k < BL_ELEMS; k++) {
      const size_t i = base + (size_t)k * GS_BLOCK + (size_t)t;
      if (i >= n) break;
      const bool m = bl_white(gt[i], gt[n + i], gt[2 * n + i], thr);
      mask[i] = m ? (uint8_t)1 : (uint8_t)0;
      if (target) target[i] = m ? 0.f : 255.0f - mono[i];
      masked += m ? 1 : 0;
    }
  }
  sh[t] = masked;
  gs_block_tree<GS_BLOCK, 1>(sh, t);
  if (t == 0) part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(GS_BLOCK) void bt_count_kernel(const int32_t* part, int nblocks, int32_t* count) {
  __shared__ int sh[GS_BLOCK];
  const int t = threadIdx.x;
  sh[t] = t < nblocks ? part[t] : 0;
  gs_block_tree<GS_BLOCK, 1>(sh, t);
  if (t == 0) count[0] = sh[0];
}

// inverse_sigmoid(factor * sigmoid(o)), in double from the fp32 input, rounded once
__device__ __forceinline__ float wr_opacity(float o, float factor) {
  const double s = 1.0 / (1.0 + exp(-(double)o));
  const double x = (double)factor * s;
  return (float)log(x / (1.0 - x));
}

// the workgroup's count of firing rows, then ONE integer add into the count the entry has zeroed on the stream
__device__ __forceinline__ void wr_count(bool fires, int* sh, int t, int32_t* counts) {
  sh[t] = fires ? 1 : 0;
  gs_block_tree<GS_BLOCK, 1>(sh, t);
  if (t == 0 && sh[0] != 0) atomicAdd(counts, sh[0]);
}

__global__ __launch_bounds__(GS_BLOCK) void wr_kernel(const float* colour, float* stat, float* opacity, size_t P, float thr,
                                                      float factor, int32_t* counts) {
  __shared__ int sh[GS_BLOCK];
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * GS_BLOCK + t;
  const bool fires = i < P && bl_white(colour[3 * i], colour[3 * i + 1], colour[3 * i + 2], thr);
  if (fires) {
    stat[i] = 0.f;
    opacity[i] = wr_opacity(opacity[i], factor);
  }
  wr_count(fires, sh, t, counts);
}

// utils/sh_utils.py:23-56 as doubles
#define BL_C0 0.28209479177387814
#define BL_C1 0.4886025119029199
#define BL_C2_0 1.0925484305920792
#define BL_C2_1 -1.0925484305920792
#define BL_C2_2 0.31539156525252005
#define BL_C2_3 -1.0925484305920792
#define BL_C2_4 0.5462742152960396
#define BL_C3_0 -0.5900435899266435
#define BL_C3_1 2.890611442640554
#define BL_C3_2 -0.4570457994644658
#define BL_C3_3 0.3731763325901154
#define BL_C3_4 -0.4570457994644658
#define BL_C3_5 1.445305721320277
#define BL_C3_6 -0.5900435899266435

struct ShRows {
  const float* dc;    // split: [P,1,3]; packed: null
  const float* rows;  // split: rest [P,M-1,3] (null when M == 1); packed: [P,M,3]
  int M;              // coefficients of a row: 1, 4, 9, 16
  int na;             // coefficients of the active degree, <= M
};

// The active coefficients of rows [r0, r0 + nr) -> LDS, row t at lds + t * BL_LDS_STRIDE, coefficient j (of the whole row) at
// 3 j.  Coalesced: consecutive lanes take consecutive elements of the (row, active element) enumeration, and the active
// elements of a row are consecutive in memory.
__device__ __forceinline__ void sh_stage(const ShRows& s, size_t r0, int nr, float* lds, int t) {
  if (s.dc) {
    for (int e = t; e < 3 * nr; e += GS_BLOCK) lds[(e / 3) * BL_LDS_STRIDE + e % 3] = s.dc[3 * r0 + e];
    const int w = 3 * (s.na - 1), S = 3 * (s.M - 1);
    for (int e = t; e < w * nr; e += GS_BLOCK) {
      const int r = e / w, k = e - r * w;
      lds[r * BL_LDS_STRIDE + 3 + k] = s.rows[(r0 + r) * (size_t)S + k];
    }
  } else {
    const int w = 3 * s.na, S = 3 * s.M;
    for (int e = t; e < w * nr; e += GS_BLOCK) {
      const int r = e / w, k = e - r * w;
      lds[r * BL_LDS_STRIDE + k] = s.rows[(r0 + r) * (size_t)S + k];
    }
  }
}

// colour of one row from its staged coefficients: max(eval_sh + 0.5, 0), NaN kept
__device__ __forceinline__ void sh_colour(const float* c, int na, const float* xyz, size_t i, const float* campos, float out[3]) {
  double x = (double)xyz[3 * i] - (double)campos[0];
  double y = (double)xyz[3 * i + 1] - (double)campos[1];
  double z = (double)xyz[3 * i + 2] - (double)campos[2];
  const double len = sqrt(x * x + y * y + z * z);
  x /= len; y /= len; z /= len;  // a zero length: 0 / 0 = NaN
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  for (int k = 0; k < 3; k++) {
    double r = BL_C0 * (double)c[k];
    if (na > 1) r = r - BL_C1 * y * (double)c[3 + k] + BL_C1 * z * (double)c[6 + k] - BL_C1 * x * (double)c[9 + k];
    if (na > 4)
      r = r + BL_C2_0 * xy * (double)c[12 + k] + BL_C2_1 * yz * (double)c[15 + k] +
          BL_C2_2 * (2.0 * zz - xx - yy) * (double)c[18 + k] + BL_C2_3 * xz * (double)c[21 + k] +
          BL_C2_4 * (xx - yy) * (double)c[24 + k];
    if (na > 9)
      r = r + BL_C3_0 * y * (3.0 * xx - yy) * (double)c[27 + k] + BL_C3_1 * xy * z * (double)c[30 + k] +
          BL_C3_2 * y * (4.0 * zz - xx - yy) * (double)c[33 + k] + BL_C3_3 * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * (double)c[36 + k] +
          BL_C3_4 * x * (4.0 * zz - xx - yy) * (double)c[39 + k] + BL_C3_5 * z * (xx - yy) * (double)c[42 + k] +
          BL_C3_6 * x * (xx - 3.0 * yy) * (double)c[45 + k];
    r += 0.5;
    out[k] = (float)(r < 0.0 ? 0.0 : r);  // (a NaN is not < 0 and stays, as in clamp_min)
  }
}

__global__ __launch_bounds__(GS_BLOCK) void wr_sh_kernel(const float* xyz, ShRows s, const float* campos, float* stat, float* opacity,
                                                         size_t P, float thr, float factor, float* colour_out, int32_t* counts) {
  __shared__ float lds[GS_BLOCK * BL_LDS_STRIDE];
  __shared__ int sh[GS_BLOCK];
  const int t = threadIdx.x;
  const size_t r0 = (size_t)blockIdx.x * GS_BLOCK;
  const int nr = (int)(P - r0 < (size_t)GS_BLOCK ? P - r0 : (size_t)GS_BLOCK);
  sh_stage(s, r0, nr, lds, t);
  __syncthreads();
  bool fires = false;
  if (t < nr) {
    const size_t i = r0 + t;
    float c[3];
    sh_colour(lds + t * BL_LDS_STRIDE, s.na, xyz, i, campos, c);
    if (colour_out) {
      colour_out[3 * i] = c[0];
      colour_out[3 * i + 1] = c[1];
      colour_out[3 * i + 2] = c[2];
    }
    fires = bl_white(c[0], c[1], c[2], thr);
    if (fires) {
      stat[i] = 0.f;
      opacity[i] = wr_opacity(opacity[i], factor);
    }
  }
  wr_count(fires, sh, t, counts);
}

static bool bl_n_ok(int64_t n) { return n >= 1 && n < BL_MAX_N; }

}  // namespace

extern "C" {

size_t gs_blender_tmp_bytes(int64_t n) {
  if (!bl_n_ok(n)) return 0;
  return gs_align((size_t)gs_capped_blocks((size_t)n, BL_BLOCK_ELEMS, BL_MAX_BLOCKS) * sizeof(int32_t));
}

int gs_blender_target(const float* gt, const float* mono, int32_t H, int32_t W, float thr, void* tmp, uint8_t* mask, int32_t* count,
                      float* target, void* stream) {
  if (H < 1 || W < 1 || !bl_n_ok((int64_t)H * (int64_t)W)) return GS_E_SHAPE;
  if (!gt || !tmp || !mask || !count || (target && !mono)) return GS_E_NULL;
  const size_t n = (size_t)H * (size_t)W;
  const int nb = gs_capped_blocks(n, BL_BLOCK_ELEMS, BL_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bt_mask_kernel, dim3(nb), dim3(GS_BLOCK), 0, s, gt, mono, n, thr, nb, mask, target, (int32_t*)tmp);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(bt_count_kernel, dim3(1), dim3(GS_BLOCK), 0, s, (const int32_t*)tmp, nb, count);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_dng_white_rule(const float* colour, float* stat, float* opacity, int64_t P, float thr, float factor, int32_t* counts,
                      void* stream) {
  if (!bl_n_ok(P)) return GS_E_SHAPE;
  if (!colour || !stat || !opacity || !counts) return GS_E_NULL;
  const unsigned rows = (unsigned)(((size_t)P + GS_BLOCK - 1) / GS_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t zeroed = hipMemsetAsync(counts, 0, sizeof(int32_t), s);
  if (zeroed != hipSuccess) return (int)zeroed;
  hipLaunchKernelGGL(wr_kernel, dim3(rows), dim3(GS_BLOCK), 0, s, colour, stat, opacity, (size_t)P, thr, factor, counts);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_dng_white_rule_sh(const float* xyz, const float* dc, const float* rows, int32_t M, int32_t active_degree, const float* campos,
                         float* stat, float* opacity, int64_t P, float thr, float factor, float* colour_out, int32_t* counts,
                         void* stream) {
  if (!bl_n_ok(P)) return GS_E_SHAPE;
  if (!(M == 1 || M == 4 || M == 9 || M == 16) || active_degree < 0 || active_degree > 3 ||
      (active_degree + 1) * (active_degree + 1) > M)
    return GS_E_SHAPE;
  // split: dc and (for M > 1) rest; packed: dc null and the whole rows
  if (!xyz || !campos || !stat || !opacity || !counts || (!dc && !rows) || (dc && M > 1 && !rows)) return GS_E_NULL;
  ShRows sr = {dc, rows, (int)M, (int)((active_degree + 1) * (active_degree + 1))};
  const unsigned nb = (unsigned)(((size_t)P + GS_BLOCK - 1) / GS_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t zeroed = hipMemsetAsync(counts, 0, sizeof(int32_t), s);
  if (zeroed != hipSuccess) return (int)zeroed;
  hipLaunchKernelGGL(wr_sh_kernel, dim3(nb), dim3(GS_BLOCK), 0, s, xyz, sr, campos, stat, opacity, (size_t)P, thr, factor,
                     colour_out, counts);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
