// gs_pearson.hip - FSGS's depth-correlation term (FSGS/train.py:100-109,121-131): Pearson's r of two fp32 sequences and the
// loss 1 - r, for up to two FORMS of the target at once with the smaller loss picked on the device, gfx950, wave64.
//
//   r = Sxy / sqrt(Sxx Syy), clamped to [-1, 1];  Sxx = sum (x - mean x)^2, Syy = sum (y - mean y)^2, Sxy = sum (x - mean x)(y - mean y)
//   y = t (GS_PEARSON_ID), -t (GS_PEARSON_NEG) or 1 / (t + 200) evaluated in fp32 (GS_PEARSON_RECIP200)
//
// forward = 2 launches:
//   pr_stats_kernel    x and t are read ONCE, as 16-byte loads.  Each lane adds, in float64, the sums of the values shifted by the
//                      sequence's first element (dx = x - x[0], dy = y - y[0]; the differences are taken in float64, where they
//                      are exact): sum dx, sum dx^2 and per form sum dy, sum dy^2, sum dx dy.  Raw fp32 moments of a depth map
//                      around 1000 with a spread of 0.01 cancel to nothing; the shifted float64 ones do not.  Which elements a
//                      lane takes is a function of n alone (block b of a grid of G sweeps the chunks b, b + G, ... of
//                      GS_PEARSON_BLOCK_ELEMS elements), the workgroup's sums go through one fixed LDS tree into the partials.
//   pr_finish_kernel   one workgroup: the partials in index order -> the statistics record, r per form, the branch by the rule of
//                      Python's min(a, b) on the fp32 losses (b only if b < a: a tie or a NaN keeps a), loss, r and branch to
//                      device memory.  Sxx == 0 or Syy == 0: r = NaN.
// backward = 1 launch: pr_bwd_kernel, four elements per lane, reads the record and dL/dloss (or dL/dr) from device memory:
//   dr/dx_i = (y_i - mean y) / sqrt(Sxx Syy) - r (x_i - mean x) / Sxx          (r unclamped: the clamp does not gate it)
//   dr/dy_i the same with x and y exchanged, sent to t through the form's derivative (ID, NEG).
//   A NaN r (constant sequence) gives zero gradients.
// No atomics, no read-back, no host synchronisation: two runs give the same bits.
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_reduce.h"

namespace {

#define PR_ITEMS (GS_PEARSON_BLOCK_ELEMS / (4 * GS_BLOCK))  // 16-byte loads per lane and sequence in one chunk
#define PR_Q 8                                             // float64 per partial: sum dx, dx^2, then (dy, dy^2, dx dy) per form
static_assert(PR_ITEMS * 4 * GS_BLOCK == GS_PEARSON_BLOCK_ELEMS, "a chunk is a whole number of float4 per lane");

struct PrStats {
  double n, mdx, Sxx;             // mdx = mean of dx: mean x = x0 + mdx
  double mdy[2], Syy[2], Sxy[2];  // per form
  double r[2];                    // unclamped; NaN when Sxx or Syy is 0
  float x0, y0[2];
  float loss[2];                  // 1 - clamp(r)
  int32_t form[2];                // form[1] = -1: one form only
  int32_t branch;                 // the form the loss came from
};

struct PrArgs {
  const float* x;
  const float* t;
  size_t n;
  int form[2];
  int vec;        // x and t (and the gradients) are 16-byte aligned
  int nblocks;
  PrStats* st;
  double* part;   // [nblocks][PR_Q]
};

__device__ __forceinline__ float pr_form(float t, int form) {
  if (form == GS_PEARSON_NEG) return -t;
  if (form == GS_PEARSON_RECIP200) return 1.f / (t + 200.f);
  return t;
}

__global__ __launch_bounds__(GS_BLOCK) void pr_stats_kernel(PrArgs a) {
  __shared__ double sh[PR_Q * GS_BLOCK];
  const int t = threadIdx.x;
  const double x0 = (double)a.x[0];
  const float t0 = a.t[0];
  const int two = a.form[1] >= 0;
  const double ya0 = (double)pr_form(t0, a.form[0]), yb0 = two ? (double)pr_form(t0, a.form[1]) : 0.0;
  double v[PR_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (size_t base = (size_t)blockIdx.x * GS_PEARSON_BLOCK_ELEMS; base < a.n; base += (size_t)a.nblocks * GS_PEARSON_BLOCK_ELEMS) {
    float xv[PR_ITEMS][4], tv[PR_ITEMS][4];
    for (int j = 0; j < PR_ITEMS; j++) {
      const size_t i = base + 4 * ((size_t)j * GS_BLOCK + t);
      gs_load4(a.x, i, a.n, a.vec, xv[j]);
      gs_load4(a.t, i, a.n, a.vec, tv[j]);
    }
    for (int j = 0; j < PR_ITEMS; j++) {
      const size_t i = base + 4 * ((size_t)j * GS_BLOCK + t);
      for (int k = 0; k < 4; k++) {
        if (i + k >= a.n) break;
        const double dx = (double)xv[j][k] - x0;
        v[0] += dx; v[1] += dx * dx;
        const double da = (double)pr_form(tv[j][k], a.form[0]) - ya0;
        v[2] += da; v[3] += da * da; v[4] += dx * da;
        if (two) {
          const double db = (double)pr_form(tv[j][k], a.form[1]) - yb0;
          v[5] += db; v[6] += db * db; v[7] += dx * db;
        }
      }
    }
  }
  gs_block_tree_sum<GS_BLOCK>(v, sh, t);
  if (t < PR_Q) a.part[(size_t)blockIdx.x * PR_Q + t] = sh[t * GS_BLOCK];  // (lane t < PR_Q takes row t's result)
}

__global__ __launch_bounds__(GS_BLOCK) void pr_finish_kernel(PrArgs a, float* out, int32_t* branch_out) {
  __shared__ double sh[PR_Q * GS_BLOCK];
  const int t = threadIdx.x;
  double v[PR_Q];
  gs_partials_tree_sum<GS_BLOCK>(a.part, a.nblocks, v, sh, t);
  if (t != 0) return;
  PrStats s;
  const double n = (double)a.n;
  const float t0 = a.t[0];
  s.n = n;
  s.x0 = a.x[0];
  s.mdx = v[0] / n;
  s.Sxx = fmax(v[1] - v[0] * v[0] / n, 0.0);
  for (int f = 0; f < 2; f++) {
    s.form[f] = a.form[f];
    if (a.form[f] < 0) {
      s.y0[f] = 0.f; s.mdy[f] = 0.0; s.Syy[f] = 0.0; s.Sxy[f] = 0.0;
      s.r[f] = __longlong_as_double(0x7ff8000000000000ll);
      s.loss[f] = __int_as_float(0x7fc00000);
      continue;
    }
    const double* w = v + 2 + 3 * f;
    s.y0[f] = pr_form(t0, a.form[f]);
    s.mdy[f] = w[0] / n;
    s.Syy[f] = fmax(w[1] - w[0] * w[0] / n, 0.0);
    s.Sxy[f] = w[2] - v[0] * w[0] / n;
    if (s.Sxx > 0.0 && s.Syy[f] > 0.0) {
      s.r[f] = s.Sxy[f] / sqrt(s.Sxx * s.Syy[f]);
      s.loss[f] = (float)(1.0 - fmin(fmax(s.r[f], -1.0), 1.0));
    } else {
      s.r[f] = __longlong_as_double(0x7ff8000000000000ll);
      s.loss[f] = __int_as_float(0x7fc00000);
    }
  }
  s.branch = (a.form[1] >= 0 && s.loss[1] < s.loss[0]) ? 1 : 0;  // Python's min(a, b): b only if b < a
  *a.st = s;
  const int b = s.branch;
  out[0] = s.loss[b];
  out[1] = s.r[b] == s.r[b] ? (float)fmin(fmax(s.r[b], -1.0), 1.0) : s.loss[b];
  out[2] = s.loss[0];
  out[3] = s.loss[1];
  if (branch_out) *branch_out = b;
}

__global__ __launch_bounds__(GS_BLOCK) void pr_bwd_kernel(PrArgs a, const float* dout, int wrt_r, float* grad_x, float* grad_t) {
  const size_t i = 4 * ((size_t)blockIdx.x * GS_BLOCK + threadIdx.x);
  if (i >= a.n) return;
  const PrStats* s = a.st;
  const int b = s->branch;
  const int form = s->form[b];
  const double r = s->r[b], Sxx = s->Sxx, Syy = s->Syy[b];
  const bool ok = r == r;  // NaN: a constant sequence - the loss is NaN, the gradient zero
  const double up = wrt_r ? (double)dout[0] : -(double)dout[0];  // loss = 1 - r
  const double inv = ok ? 1.0 / sqrt(Sxx * Syy) : 0.0;
  const double mx = (double)s->x0 + s->mdx, my = (double)s->y0[b] + s->mdy[b];
  const double dy_dt = form == GS_PEARSON_NEG ? -1.0 : 1.0;
  float xv[4] = {0.f, 0.f, 0.f, 0.f}, tv[4] = {0.f, 0.f, 0.f, 0.f}, gx[4], gt[4];
  gs_load4(a.x, i, a.n, a.vec, xv);
  gs_load4(a.t, i, a.n, a.vec, tv);
  for (int k = 0; k < 4; k++) {
    const double xc = (double)xv[k] - mx, yc = (double)pr_form(tv[k], form) - my;
    gx[k] = ok ? (float)(up * (yc * inv - r * xc / Sxx)) : 0.f;
    gt[k] = ok ? (float)(up * dy_dt * (xc * inv - r * yc / Syy)) : 0.f;
  }
  if (a.vec && i + 4 <= a.n) {
    if (grad_x) *reinterpret_cast<float4*>(grad_x + i) = make_float4(gx[0], gx[1], gx[2], gx[3]);
    if (grad_t) *reinterpret_cast<float4*>(grad_t + i) = make_float4(gt[0], gt[1], gt[2], gt[3]);
  } else {
    for (int k = 0; k < 4 && i + k < a.n; k++) {
      if (grad_x) grad_x[i + k] = gx[k];
      if (grad_t) grad_t[i + k] = gt[k];
    }
  }
}

// ---- host side ----
static bool pr_form_ok(int f) { return f == GS_PEARSON_ID || f == GS_PEARSON_NEG || f == GS_PEARSON_RECIP200; }

static int pr_check(int64_t n, int form_a, int form_b) {
  if (n < 2 || n > ((int64_t)1 << 40) || !pr_form_ok(form_a) || !(form_b == -1 || pr_form_ok(form_b))) return GS_E_SHAPE;
  return GS_OK;
}

static PrArgs pr_args(const float* x, const float* t, int64_t n, int form_a, int form_b, void* tmp) {
  PrArgs a = {};
  a.x = x; a.t = t; a.n = (size_t)n;
  a.form[0] = form_a; a.form[1] = form_b;
  a.vec = gs_aligned16(x) && gs_aligned16(t);
  a.nblocks = gs_capped_blocks(a.n, GS_PEARSON_BLOCK_ELEMS, GS_PEARSON_MAX_BLOCKS);
  a.st = (PrStats*)tmp;
  a.part = (double*)((char*)tmp + gs_align(sizeof(PrStats)));
  return a;
}

}  // namespace

extern "C" {

size_t gs_pearson_tmp_bytes(int64_t n) {
  if (n < 2 || n > ((int64_t)1 << 40)) return 0;
  return gs_align(sizeof(PrStats)) + gs_align((size_t)gs_capped_blocks((size_t)n, GS_PEARSON_BLOCK_ELEMS, GS_PEARSON_MAX_BLOCKS) * PR_Q * sizeof(double));
}

int gs_pearson_fwd(const float* x, const float* t, int64_t n, int32_t form_a, int32_t form_b, void* tmp, float* out,
                   int32_t* branch_out, void* stream) {
  const int rc = pr_check(n, form_a, form_b);
  if (rc) return rc;
  if (!x || !t || !tmp || !out) return GS_E_NULL;
  const PrArgs a = pr_args(x, t, n, form_a, form_b, tmp);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pr_stats_kernel, dim3(a.nblocks), dim3(GS_BLOCK), 0, s, a);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(pr_finish_kernel, dim3(1), dim3(GS_BLOCK), 0, s, a, out, branch_out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_pearson_bwd(const float* x, const float* t, int64_t n, int32_t form_a, int32_t form_b, int32_t flags, const void* tmp,
                   const float* dout_dev, float* grad_x, float* grad_t, void* stream) {
  const int rc = pr_check(n, form_a, form_b);
  if (rc) return rc;
  if (flags & ~GS_PEARSON_WRT_R) return GS_E_SHAPE;
  if (!x || !t || !tmp || !dout_dev || (!grad_x && !grad_t)) return GS_E_NULL;
  if (grad_t && (form_a == GS_PEARSON_RECIP200 || form_b == GS_PEARSON_RECIP200)) return GS_E_UNSUPPORTED;
  PrArgs a = pr_args(x, t, n, form_a, form_b, (void*)tmp);
  a.vec = a.vec && gs_aligned16(grad_x) && gs_aligned16(grad_t);
  hipStream_t s = (hipStream_t)stream;
  const size_t lanes = (a.n + 3) / 4;
  hipLaunchKernelGGL(pr_bwd_kernel, dim3((unsigned)((lanes + GS_BLOCK - 1) / GS_BLOCK)), dim3(GS_BLOCK), 0, s, a, dout_dev,
                     (flags & GS_PEARSON_WRT_R) != 0, grad_x, grad_t);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
