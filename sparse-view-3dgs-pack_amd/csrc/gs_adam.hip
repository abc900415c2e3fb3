// gs_adam.hip - fused Adam over the flat parameter buffer (SURVEY.md 8f-1 "next" row).
//
// The reference steps six torch tensors with torch.optim.Adam(lr=0, eps=1e-15) and per-group learning rates
// (LGDWT-GS/scene/gaussian_model.py:183-193, train.py:279-288).  Here parameters, gradients and both moment
// buffers are each ONE flat fp32 array (59 floats per Gaussian); a launch updates all of it in one streaming
// pass (28 B/element: read p,g,m,v, write p,m,v), the learning rate being looked up from a small segment table.
// A segment may alternate between two rates with a period (the [P,16,3] SH block: 3 DC floats at feature_lr,
// 45 at feature_lr/20), which lets the model keep DC and rest coefficients interleaved as the rasterizer wants
// them - no torch.cat per step.
// Arithmetic = torch.optim.Adam (no amsgrad, no weight decay):
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
#include <math.h>

#include "gs_common.h"
#include "gs_prof.h"

#define ADAM_MAX_SEG 8
struct AdamSegs {
  int n;
  long long begin[ADAM_MAX_SEG], end[ADAM_MAX_SEG];
  float lr_a[ADAM_MAX_SEG], lr_b[ADAM_MAX_SEG];
  int period[ADAM_MAX_SEG], split[ADAM_MAX_SEG];
  float inv_bc1[ADAM_MAX_SEG], inv_sqrt_bc2[ADAM_MAX_SEG];  // bias corrections of the segment's own step count
  int row_width[ADAM_MAX_SEG];                              // gs_adam_step_masked: floats per Gaussian (0: not masked)
};
// gs_adam_step_masked ("sparse_adam", train.py:282-284): is element i one of a row that is stepped?
__device__ __forceinline__ bool adam_row_on(const AdamSegs& s, int k, long long i, const float* __restrict__ row_mask) {
  if (!row_mask || s.row_width[k] <= 0) return true;
  return row_mask[(i - s.begin[k]) / s.row_width[k]] > 0.f;
}

// step size lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) of element i; false = covered by no segment (left untouched)
__device__ __forceinline__ bool adam_coef(const AdamSegs& s, long long i, float& lr_bc1, float& inv_sqrt_bc2,
                                          const float* __restrict__ row_mask = nullptr) {
  bool hit = false;
#pragma unroll
  for (int k = 0; k < ADAM_MAX_SEG; k++)
    if (k < s.n && i >= s.begin[k] && i < s.end[k]) {
      const float lr = (s.period[k] > 0 && (int)((i - s.begin[k]) % s.period[k]) >= s.split[k]) ? s.lr_b[k] : s.lr_a[k];
      lr_bc1 = lr * s.inv_bc1[k];
      inv_sqrt_bc2 = s.inv_sqrt_bc2[k];
      hit = adam_row_on(s, k, i, row_mask);
    }
  return hit;
}

__global__ void __launch_bounds__(GS_BLOCK) adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long long n,
                                                        AdamSegs segs, float b1, float b2, float eps,
                                                        const float* __restrict__ gate, const float* __restrict__ row_mask) {
  if (gate && *gate != 0.0f) return;  // gs_adam_step_gated: some rank's view was invalid - nobody steps
  const long long n4 = n >> 2;
  for (long long i4 = (long long)blockIdx.x * GS_BLOCK + threadIdx.x; i4 < n4; i4 += (long long)gridDim.x * GS_BLOCK) {
    float4 pp = reinterpret_cast<float4*>(p)[i4];
    const float4 gg = reinterpret_cast<const float4*>(g)[i4];
    float4 mm = reinterpret_cast<float4*>(m)[i4];
    float4 vv = reinterpret_cast<float4*>(v)[i4];
    float* pe = reinterpret_cast<float*>(&pp);
    const float* ge = reinterpret_cast<const float*>(&gg);
    float* me = reinterpret_cast<float*>(&mm);
    float* ve = reinterpret_cast<float*>(&vv);
    // Fast path: the four elements lie in one segment (always, except where a segment boundary is not a multiple
    // of 4): one table walk and one 64-bit modulo per vector instead of four
    const long long i0 = i4 * 4;
    int seg = -1;
#pragma unroll
    for (int k = 0; k < ADAM_MAX_SEG; k++)
      if (k < segs.n && i0 >= segs.begin[k] && i0 + 3 < segs.end[k]) seg = k;
    if (seg >= 0) {
      const float inv_sqrt_bc2 = segs.inv_sqrt_bc2[seg];
      const float lra = segs.lr_a[seg] * segs.inv_bc1[seg], lrb = segs.lr_b[seg] * segs.inv_bc1[seg];
      const int period = segs.period[seg], split = segs.split[seg];
      int ph = period > 0 ? (int)((i0 - segs.begin[seg]) % period) : 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float lr_bc1 = (period > 0 && ph >= split) ? lrb : lra;
        ph = (ph + 1 == period) ? 0 : ph + 1;
        if (!adam_row_on(segs, seg, i0 + k, row_mask)) continue;
        me[k] = b1 * me[k] + (1.f - b1) * ge[k];
        ve[k] = b2 * ve[k] + (1.f - b2) * ge[k] * ge[k];
        const float denom = sqrtf(ve[k]) * inv_sqrt_bc2 + eps;
        pe[k] = pe[k] - lr_bc1 * (me[k] / denom);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        float lr_bc1, inv_sqrt_bc2;
        if (!adam_coef(segs, i0 + k, lr_bc1, inv_sqrt_bc2, row_mask)) continue;
        me[k] = b1 * me[k] + (1.f - b1) * ge[k];
        ve[k] = b2 * ve[k] + (1.f - b2) * ge[k] * ge[k];
        const float denom = sqrtf(ve[k]) * inv_sqrt_bc2 + eps;
        pe[k] = pe[k] - lr_bc1 * (me[k] / denom);
      }
    }
    reinterpret_cast<float4*>(p)[i4] = pp;
    reinterpret_cast<float4*>(m)[i4] = mm;
    reinterpret_cast<float4*>(v)[i4] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {
    const long long i = n4 * 4 + threadIdx.x;
    float lr_bc1, inv_sqrt_bc2;
    if (adam_coef(segs, i, lr_bc1, inv_sqrt_bc2, row_mask)) {
      const float gi = g[i];
      const float mi = b1 * m[i] + (1.f - b1) * gi;
      const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
      m[i] = mi;
      v[i] = vi;
      p[i] = p[i] - lr_bc1 * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
    }
  }
}

extern "C" int gs_adam_step_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                  const GsAdamSeg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                                  const float* gate, void* stream);
extern "C" int gs_adam_step_masked(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                   const GsAdamSeg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                                   const float* gate, const float* row_mask, void* stream);
extern "C" int gs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                            const GsAdamSeg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                            void* stream) {
  return gs_adam_step_gated(params, grads, exp_avg, exp_avg_sq, n, segs, nseg, beta1, beta2, eps, step, nullptr, stream);
}
extern "C" int gs_adam_step_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                  const GsAdamSeg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                                  const float* gate, void* stream) {
  return gs_adam_step_masked(params, grads, exp_avg, exp_avg_sq, n, segs, nseg, beta1, beta2, eps, step, gate, nullptr, stream);
}
extern "C" int gs_adam_step_masked(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                   const GsAdamSeg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                                   const float* gate, const float* row_mask, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || (nseg > 0 && !segs)) return GS_E_NULL;
  if (n < 0 || nseg < 0 || nseg > ADAM_MAX_SEG || step < 1) return GS_E_SHAPE;
  if (n == 0) return GS_OK;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0)
    return GS_E_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_ADAM, s);
  AdamSegs a;
  a.n = nseg;
  for (int k = 0; k < ADAM_MAX_SEG; k++) {
    const bool on = k < nseg;
    a.begin[k] = on ? segs[k].begin : 0;
    a.end[k] = on ? segs[k].end : 0;
    a.lr_a[k] = on ? segs[k].lr_a : 0.f;
    a.lr_b[k] = on ? segs[k].lr_b : 0.f;
    a.period[k] = on ? segs[k].period : 0;
    a.split[k] = on ? segs[k].split : 0;
    a.row_width[k] = on ? segs[k].row_width : 0;
    const int st = (on && segs[k].step > 0) ? segs[k].step : step;
    const double bc1 = 1.0 - pow((double)beta1, (double)st), bc2 = 1.0 - pow((double)beta2, (double)st);
    a.inv_bc1[k] = (float)(1.0 / bc1);
    a.inv_sqrt_bc2[k] = (float)(1.0 / sqrt(bc2));
  }
  const long long n4 = (n + 3) / 4;
  long long blocks = (n4 + GS_BLOCK - 1) / GS_BLOCK;
  // one float4 per thread up to 2^20 workgroups: 0.292 ms at 59 M elements against 0.315 with an 8192-workgroup
  // grid-stride loop (and 0.331 with 2048) - short-lived workgroups keep more requests in flight
  if (blocks > (1ll << 20)) blocks = 1ll << 20;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(GS_BLOCK), 0, s, params, grads, exp_avg, exp_avg_sq,
                     (long long)n, a, beta1, beta2, eps, gate, row_mask);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// gs_adam_step_tensors: the optimizer behind the reference's OWN API (six torch tensors, one param group each:
// gaussian_model.py:183-193) in ONE launch, and - with a row mask - with traffic that follows the rows the view saw
// (train.py:282-284: `optimizer.step(radii > 0, N)`).
// Work map: the table below travels in the kernel arguments; tensor k owns the workgroups [wg_end[k-1], wg_end[k]), found by
// wave-uniform compares.  Inside its tensor a workgroup is adam_kernel's: one float4 per thread (grid-stride beyond the
// workgroup cap), and the tensor's first workgroup steps the n & 3 elements behind the float4 body.
// Mask first: a lane derives the row of its float4's first element (ONE division per float4), walks a phase counter over the
// four elements and reads the mask bytes of the rows they belong to BEFORE anything else.  A lane without a stepped element
// issues no load and no store, so a wave without one issues none (nothing but its mask bytes is fetched); a float4 that
// straddles a stepped and an unstepped row writes back the loaded bits of the unstepped elements.
// Arithmetic: adam_kernel's, same order.  GS_ADAM_NO_BIAS_CORRECTION is that very expression with both bias-correction
// factors equal to 1 (x * 1.0f is exact: sqrtf(v) * 1 + eps == sqrtf(v) + eps, lr * 1 == lr), so there is one code path.
// ------------------------------------------------------------------------------------------------------------------
#define ADAM_MAX_TENSORS 8
static_assert(sizeof(GsAdamTensor) == 56, "GsAdamTensor: the layout gsplat_amd/capi.py mirrors");
struct AdamTensors {
  int n;  // tensors with elements (the host drops the empty ones)
  float* p[ADAM_MAX_TENSORS];
  const float* g[ADAM_MAX_TENSORS];
  float* m[ADAM_MAX_TENSORS];
  float* v[ADAM_MAX_TENSORS];
  long long len[ADAM_MAX_TENSORS];
  int row_width[ADAM_MAX_TENSORS];  // 0: not masked
  float lr[ADAM_MAX_TENSORS], inv_bc1[ADAM_MAX_TENSORS], inv_sqrt_bc2[ADAM_MAX_TENSORS];
  unsigned wg_end[ADAM_MAX_TENSORS];  // prefix sums of the tensors' workgroup counts
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float lr_bc1, float inv_sqrt_bc2, float b1,
                                             float b2, float eps) {
  m = b1 * m + (1.f - b1) * g;
  v = b2 * v + (1.f - b2) * g * g;
  const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
  p = p - lr_bc1 * (m / denom);
}

__global__ void __launch_bounds__(GS_BLOCK) adam_tensors_kernel(AdamTensors t, float b1, float b2, float eps,
                                                                const unsigned char* __restrict__ row_mask) {
  // this workgroup's tensor: constant indices into the argument table, selected by wave-uniform compares (scalar registers)
  float* p = t.p[0];
  const float* g = t.g[0];
  float* m = t.m[0];
  float* v = t.v[0];
  long long n = t.len[0];
  int rw = t.row_width[0];
  float lr_bc1 = t.lr[0] * t.inv_bc1[0], isb = t.inv_sqrt_bc2[0];
  unsigned wg_first = 0, wg_last = t.wg_end[0];
#pragma unroll
  for (int k = 1; k < ADAM_MAX_TENSORS; k++)
    if (k < t.n && blockIdx.x >= t.wg_end[k - 1]) {
      p = t.p[k]; g = t.g[k]; m = t.m[k]; v = t.v[k];
      n = t.len[k];
      rw = t.row_width[k];
      lr_bc1 = t.lr[k] * t.inv_bc1[k];
      isb = t.inv_sqrt_bc2[k];
      wg_first = t.wg_end[k - 1];
      wg_last = t.wg_end[k];
    }
  const bool masked = row_mask != nullptr && rw > 0;
  const long long n4 = n >> 2;
  const bool small = n <= 0x7fffffffll;  // (element indices fit 32 bits: the one division per float4 is a 32-bit one)
  const long long stride = (long long)(wg_last - wg_first) * GS_BLOCK;
  for (long long i4 = (long long)(blockIdx.x - wg_first) * GS_BLOCK + threadIdx.x; i4 < n4; i4 += stride) {
    bool on[4] = {true, true, true, true};
    if (masked) {
      const long long i0 = i4 * 4;
      long long row;
      int ph;
      if (small) {
        const unsigned r32 = (unsigned)i0 / (unsigned)rw;
        row = r32;
        ph = (int)((unsigned)i0 - r32 * (unsigned)rw);
      } else {
        row = i0 / rw;
        ph = (int)(i0 - row * rw);
      }
      // (n == P * row_width and i0 + 3 < n: every row read here is < P)
      unsigned char mk = row_mask[row];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        on[e] = mk != 0;
        if (++ph == rw) {
          ph = 0;
          row++;
          if (e < 3) mk = row_mask[row];
        }
      }
      if (!(on[0] | on[1] | on[2] | on[3])) continue;  // no load, no store: a wave of such lanes moves nothing but mask bytes
    }
    float4 pp = reinterpret_cast<float4*>(p)[i4];
    const float4 gg = reinterpret_cast<const float4*>(g)[i4];
    float4 mm = reinterpret_cast<float4*>(m)[i4];
    float4 vv = reinterpret_cast<float4*>(v)[i4];
    float* pe = reinterpret_cast<float*>(&pp);
    const float* ge = reinterpret_cast<const float*>(&gg);
    float* me = reinterpret_cast<float*>(&mm);
    float* ve = reinterpret_cast<float*>(&vv);
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (on[e]) adam_element(pe[e], ge[e], me[e], ve[e], lr_bc1, isb, b1, b2, eps);
    reinterpret_cast<float4*>(p)[i4] = pp;
    reinterpret_cast<float4*>(m)[i4] = mm;
    reinterpret_cast<float4*>(v)[i4] = vv;
  }
  // the tensor's own tail: the n & 3 elements behind its float4 body (tensor sizes are P * {3,3,45,1,3,4})
  if (blockIdx.x == wg_first && threadIdx.x < (unsigned)(n & 3)) {
    const long long i = n4 * 4 + threadIdx.x;
    if (masked && row_mask[i / rw] == 0) return;
    float pi = p[i], mi = m[i], vi = v[i];
    adam_element(pi, g[i], mi, vi, lr_bc1, isb, b1, b2, eps);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

extern "C" int gs_adam_step_tensors(const GsAdamTensor* t, int32_t nt, int64_t P, float beta1, float beta2, float eps,
                                    int32_t flags, const uint8_t* row_mask, void* stream) {
  if (nt < 0 || nt > ADAM_MAX_TENSORS) return GS_E_SHAPE;
  if (flags & ~GS_ADAM_NO_BIAS_CORRECTION) return GS_E_UNSUPPORTED;
  if (nt > 0 && !t) return GS_E_NULL;
  const bool bc = !(flags & GS_ADAM_NO_BIAS_CORRECTION);
  for (int k = 0; k < nt; k++) {
    if (t[k].n < 0 || (bc && t[k].step < 1) || t[k].row_width < 0) return GS_E_SHAPE;
    if (row_mask && t[k].row_width > 0 && (P < 0 || t[k].n != P * (int64_t)t[k].row_width)) return GS_E_SHAPE;
  }
  AdamTensors a = {};
  long long blocks[ADAM_MAX_TENSORS];
  long long total = 0;
  for (int k = 0; k < nt; k++) {
    if (t[k].n == 0) continue;
    if (!t[k].param || !t[k].grad || !t[k].exp_avg || !t[k].exp_avg_sq) return GS_E_NULL;
    if ((((uintptr_t)t[k].param | (uintptr_t)t[k].grad | (uintptr_t)t[k].exp_avg | (uintptr_t)t[k].exp_avg_sq) & 15) != 0)
      return GS_E_UNSUPPORTED;
    const int j = a.n++;
    a.p[j] = t[k].param;
    a.g[j] = t[k].grad;
    a.m[j] = t[k].exp_avg;
    a.v[j] = t[k].exp_avg_sq;
    a.len[j] = t[k].n;
    a.row_width[j] = t[k].row_width;
    a.lr[j] = t[k].lr;
    a.inv_bc1[j] = a.inv_sqrt_bc2[j] = 1.0f;
    if (bc) {  // (as gs_adam_step forms them)
      const double bc1 = 1.0 - pow((double)beta1, (double)t[k].step), bc2 = 1.0 - pow((double)beta2, (double)t[k].step);
      a.inv_bc1[j] = (float)(1.0 / bc1);
      a.inv_sqrt_bc2[j] = (float)(1.0 / sqrt(bc2));
    }
    const long long n4 = (t[k].n + 3) / 4;
    blocks[j] = (n4 + GS_BLOCK - 1) / GS_BLOCK;
    total += blocks[j];
  }
  if (a.n == 0) return GS_OK;
  // gs_adam_step's launch shape: one float4 per thread up to 2^20 workgroups in all, a grid-stride loop inside a tensor beyond
  if (total > (1ll << 20)) {
    const long long cap = (1ll << 20) / a.n;
    for (int j = 0; j < a.n; j++)
      if (blocks[j] > cap) blocks[j] = cap;
  }
  unsigned end = 0;
  for (int j = 0; j < ADAM_MAX_TENSORS; j++) {
    if (j < a.n) end += (unsigned)blocks[j];
    a.wg_end[j] = end;
  }
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_ADAM, s);
  hipLaunchKernelGGL(adam_tensors_kernel, dim3(end), dim3(GS_BLOCK), 0, s, a, beta1, beta2, eps,
                     (const unsigned char*)row_mask);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}
