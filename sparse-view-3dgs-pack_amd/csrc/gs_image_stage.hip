// gs_image_stage.hip - what LGDWT-GS/train.py does to the render between the rasterizer and the loss.
//
//   lin  = raw . E[:3,:3] + E[:3,3]          (trained per-camera exposure, gaussian_renderer/__init__.py:112-115)
//   pred = clamp(lin, 0, 1) * alpha          (clamp of :119, then `image *= alpha_mask` of train.py:121-124)
//
// raw / pred are [3,H,W] planes, E the camera's [3,4] row (12 floats, row-major: E[c][k] at 4 c + k), alpha [H,W].
// E NULL: lin = raw; alpha NULL: alpha = 1.  A lane owns whole pixels (all three channels), four along x per float4 when
// the planes allow it (H*W a multiple of 4, 16-byte aligned), else one.
//
// Backward (g_pred = the criterion's image gradient, taken WITHOUT its clamp fold):
//   g_lin[j] = g_pred[j] * alpha * [0 <= lin[j] <= 1]            (torch's clamp gradient, as gs_ssim_bwd_uniform folds it)
//   g_raw[c] = sum_j E[c][j] g_lin[j]
//   dE[c][j] = sum_pix raw[c] g_lin[j],  dE[j][3] = sum_pix g_lin[j]
// The 12 exposure sums leave as one row per workgroup; gs_exposure_adam adds the rows in a fixed order (one wave per
// word, lane-strided, then a fixed shuffle tree - the shape of gs_lgdwt_combine_pp) in double: the same bits every run.
//
// Bytes per pixel: forward reads 12 (raw) + 4 (alpha) and writes 12; backward reads 12 (raw) + 12 (g_pred) + 4 (alpha)
// and writes 12.  At 1920 x 1080: 33 MB read / 25 MB written forward, 58 MB read / 25 MB written backward (a model, not
// a measurement).
#include <math.h>

#include "gs_common.h"
#include "gs_prof.h"

namespace {

constexpr int STAGE_MAX_WG = 1024;  // partial rows per backward launch (a function of H * W only)

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

__device__ __forceinline__ void load_e(const float* __restrict__ E_dev, float (&E)[12]) {
#pragma unroll
  for (int k = 0; k < 12; k++) E[k] = E_dev ? E_dev[k] : 0.f;
}

// lin of one pixel
__device__ __forceinline__ void expose(bool has_e, const float (&E)[12], const float (&r)[3], float (&l)[3]) {
#pragma unroll
  for (int j = 0; j < 3; j++) l[j] = has_e ? r[0] * E[j] + r[1] * E[4 + j] + r[2] * E[8 + j] + E[4 * j + 3] : r[j];
}

template <bool VEC>
__global__ void __launch_bounds__(GS_BLOCK) stage_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ E_dev,
                                                             const float* __restrict__ alpha, int64_t hw,
                                                             float* __restrict__ pred) {
  float E[12];
  load_e(E_dev, E);
  const bool has_e = E_dev != nullptr;
  constexpr int V = VEC ? 4 : 1;
  const int64_t n = hw / V;
  for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_BLOCK) {
    float r[3][V], a[V], o[3][V];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if constexpr (VEC) {
        const float4 x = reinterpret_cast<const float4*>(raw + (size_t)c * hw)[i];
        r[c][0] = x.x; r[c][1] = x.y; r[c][2] = x.z; r[c][3] = x.w;
      } else {
        r[c][0] = raw[(size_t)c * hw + i];
      }
    }
    if (alpha) {
      if constexpr (VEC) {
        const float4 x = reinterpret_cast<const float4*>(alpha)[i];
        a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w;
      } else {
        a[0] = alpha[i];
      }
    }
#pragma unroll
    for (int k = 0; k < V; k++) {
      const float rp[3] = {r[0][k], r[1][k], r[2][k]};
      float l[3];
      expose(has_e, E, rp, l);
#pragma unroll
      for (int j = 0; j < 3; j++) o[j][k] = alpha ? clamp01(l[j]) * a[k] : clamp01(l[j]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if constexpr (VEC) {
        float4 x;
        x.x = o[c][0]; x.y = o[c][1]; x.z = o[c][2]; x.w = o[c][3];
        reinterpret_cast<float4*>(pred + (size_t)c * hw)[i] = x;
      } else {
        pred[(size_t)c * hw + i] = o[c][0];
      }
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(GS_BLOCK) stage_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ E_dev,
                                                             const float* __restrict__ alpha, const float* __restrict__ g_pred,
                                                             int64_t hw, float* __restrict__ g_raw, float* __restrict__ partials) {
  float E[12];
  load_e(E_dev, E);
  const bool has_e = E_dev != nullptr;
  constexpr int V = VEC ? 4 : 1;
  const int64_t n = hw / V;
  float acc[12];  // dE[c][j] at 4 c + j, dE[j][3] at 4 j + 3
#pragma unroll
  for (int k = 0; k < 12; k++) acc[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_BLOCK) {
    float r[3][V], g[3][V], a[V], o[3][V];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if constexpr (VEC) {
        const float4 x = reinterpret_cast<const float4*>(raw + (size_t)c * hw)[i];
        const float4 y = reinterpret_cast<const float4*>(g_pred + (size_t)c * hw)[i];
        r[c][0] = x.x; r[c][1] = x.y; r[c][2] = x.z; r[c][3] = x.w;
        g[c][0] = y.x; g[c][1] = y.y; g[c][2] = y.z; g[c][3] = y.w;
      } else {
        r[c][0] = raw[(size_t)c * hw + i];
        g[c][0] = g_pred[(size_t)c * hw + i];
      }
    }
    if (alpha) {
      if constexpr (VEC) {
        const float4 x = reinterpret_cast<const float4*>(alpha)[i];
        a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w;
      } else {
        a[0] = alpha[i];
      }
    }
#pragma unroll
    for (int k = 0; k < V; k++) {
      const float rp[3] = {r[0][k], r[1][k], r[2][k]};
      float l[3], gl[3];
      expose(has_e, E, rp, l);
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const float gj = alpha ? g[j][k] * a[k] : g[j][k];
        gl[j] = (l[j] < 0.f || l[j] > 1.f) ? 0.f : gj;
      }
#pragma unroll
      for (int c = 0; c < 3; c++) o[c][k] = has_e ? E[4 * c] * gl[0] + E[4 * c + 1] * gl[1] + E[4 * c + 2] * gl[2] : gl[c];
      if (partials) {
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
          for (int j = 0; j < 3; j++) acc[4 * c + j] += rp[c] * gl[j];
#pragma unroll
        for (int j = 0; j < 3; j++) acc[4 * j + 3] += gl[j];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if constexpr (VEC) {
        float4 x;
        x.x = o[c][0]; x.y = o[c][1]; x.z = o[c][2]; x.w = o[c][3];
        reinterpret_cast<float4*>(g_raw + (size_t)c * hw)[i] = x;
      } else {
        g_raw[(size_t)c * hw + i] = o[c][0];
      }
    }
  }
  if (!partials) return;
  // wave64 shuffle tree, then the four waves' sums in wave order: one row of 12 per workgroup, every row written
  __shared__ float red[GS_BLOCK / 64][12];
#pragma unroll
  for (int k = 0; k < 12; k++) {
    float x = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < GS_BLOCK / 64; w++) t += red[w][threadIdx.x];
    partials[(size_t)blockIdx.x * 12 + threadIdx.x] = t;
  }
}

// One workgroup of 12 waves.  partials given: wave k adds word k of the n_part rows (lanes strided, double, fixed shuffle tree)
// -> the gradient of camera ci's row, zero for every other row (written to grad when given).  partials NULL: the gradient is
// read from grad.  exposure given: torch.optim.Adam's step (foreach form) over all n elements with that gradient.
__global__ void __launch_bounds__(768) exposure_adam_kernel(const float* __restrict__ partials, int n_part, int ci,
                                                            float* __restrict__ grad, float* __restrict__ p,
                                                            float* __restrict__ m, float* __restrict__ v, int n,
                                                            float step_size, float bc2_sqrt, float b2, float w1, float w2,
                                                            float eps, const float* __restrict__ gate) {
  if (gate && *gate != 0.0f) return;  // as gs_adam_step_gated: the view was invalid, nothing changes
  __shared__ float s_g[12];
  if (partials) {
    const int slot = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (slot < 12) {
      double t = 0.0;
      for (int w = lane; w < n_part; w += 64) t += (double)partials[(size_t)w * 12 + slot];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) t += __shfl_down(t, off, 64);
      if (lane == 0) s_g[slot] = (float)t;
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float g;
    if (partials) {
      g = (i / 12 == ci) ? s_g[i % 12] : 0.f;
      if (grad) grad[i] = g;
    } else {
      g = grad[i];
    }
    if (!p) continue;
    const float mi = m[i] + w1 * (g - m[i]);      // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = v[i] * b2 + w2 * (g * g);    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] + (-step_size) * (mi / denom);
  }
}

int stage_blocks(int64_t hw) {
  const int64_t b = ((hw + 3) / 4 + GS_BLOCK - 1) / GS_BLOCK;
  return (int)(b < 1 ? 1 : (b > STAGE_MAX_WG ? STAGE_MAX_WG : b));
}

bool stage_vec(int64_t hw, std::initializer_list<const void*> ptrs) {
  if (hw % 4 != 0) return false;
  for (const void* q : ptrs)
    if (((uintptr_t)q & 15) != 0) return false;
  return true;
}

}  // namespace

extern "C" {

int64_t gs_image_stage_partials_count(int32_t H, int32_t W) {
  return (H <= 0 || W <= 0) ? 0 : (int64_t)stage_blocks((int64_t)H * W);
}

int gs_image_stage_fwd(const float* raw, const float* exposure, const float* alpha, int32_t H, int32_t W, float* pred,
                       void* stream) {
  if (!raw || !pred) return GS_E_NULL;
  if (H <= 0 || W <= 0) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_IMAGE_STAGE, s);
  const int64_t hw = (int64_t)H * W;
  if (stage_vec(hw, {raw, alpha, pred}))
    hipLaunchKernelGGL(stage_fwd_kernel<true>, dim3(stage_blocks(hw)), dim3(GS_BLOCK), 0, s, raw, exposure, alpha, hw, pred);
  else
    hipLaunchKernelGGL(stage_fwd_kernel<false>, dim3(stage_blocks(hw)), dim3(GS_BLOCK), 0, s, raw, exposure, alpha, hw, pred);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_image_stage_bwd(const float* raw, const float* exposure, const float* alpha, const float* g_pred, int32_t H, int32_t W,
                       float* g_raw, float* partials, void* stream) {
  if (!raw || !g_pred || !g_raw) return GS_E_NULL;
  if (H <= 0 || W <= 0) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_IMAGE_STAGE, s);
  const int64_t hw = (int64_t)H * W;
  if (stage_vec(hw, {raw, alpha, g_pred, g_raw}))
    hipLaunchKernelGGL(stage_bwd_kernel<true>, dim3(stage_blocks(hw)), dim3(GS_BLOCK), 0, s, raw, exposure, alpha, g_pred, hw,
                       g_raw, partials);
  else
    hipLaunchKernelGGL(stage_bwd_kernel<false>, dim3(stage_blocks(hw)), dim3(GS_BLOCK), 0, s, raw, exposure, alpha, g_pred, hw,
                       g_raw, partials);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_exposure_adam(const float* partials, int64_t n_partials, int32_t camera, float* grad, float* exposure, float* exp_avg,
                     float* exp_avg_sq, int32_t n_cameras, float lr, double beta1, double beta2, float eps, int32_t step,
                     const float* gate, void* stream) {
  if (!partials && !grad) return GS_E_NULL;
  if (!exposure && !grad) return GS_E_NULL;
  if (exposure && (!exp_avg || !exp_avg_sq)) return GS_E_NULL;
  if (n_cameras <= 0 || n_cameras > (1 << 24)) return GS_E_SHAPE;
  if (partials && (n_partials <= 0 || n_partials > (1 << 24) || camera < 0 || camera >= n_cameras)) return GS_E_SHAPE;
  if (exposure && step < 1) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_ADAM, s);
  float step_size = 0.f, bc2_sqrt = 1.f;
  if (exposure) {  // torch: bias corrections, step size and 1 - beta in double, the kernel's operands in float
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    step_size = (float)((double)lr / bc1);
    bc2_sqrt = (float)sqrt(bc2);
  }
  hipLaunchKernelGGL(exposure_adam_kernel, dim3(1), dim3(768), 0, s, partials, (int)n_partials, camera, grad, exposure, exp_avg,
                     exp_avg_sq, 12 * n_cameras, step_size, bc2_sqrt, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                     eps, gate);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
