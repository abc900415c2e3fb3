// gs_depth_norm.hip - DNGaussian's depth-normalisation regulariser (utils/loss_utils.py: normalize, margin_l{1,2}_loss,
// patchify, patch_norm_{mse,l1}_loss[_global], loss_depth_smoothness) on one [1,1,H,W] fp32 depth image, gfx950, wave64.
//
// A call carries up to two patch TERMS (slot 0, slot 1: each its own patch size p, margin, local / global form, mse / l1,
// weight) and an optional SMOOTHNESS term.  The single-loss entries use slot 0 alone, gs_dng_depth_reg_* uses all three.
//
// forward = 4 launches, whatever the terms:
//   dn_stats_kernel     per patch: mean, then the centred sum of squares (second pass over rows the first pass just brought
//                       into cache), both accumulated in float64, for input and target; per-workgroup float64 partials of
//                       (sum m, sum m^2, sum SS).  Its last blocks walk the whole image in 2048-pixel chunks: the shifted
//                       moments of the uncropped image (global form) and the smoothness numerator / denominator.
//   dn_globals_kernel   one workgroup: adds the partials in index order -> std_all of each term (Chan's combination of equal
//                       sized groups: SS = sum SS_l + n sum (m_l - M)^2), the whole-image std, the smoothness loss.
//   dn_apply_kernel     per patch: d = n(input) - n(target), mask = |d| > margin, masked count, sum f(d), sum g, sum g (x - m)
//                       (g = f'(d) on the mask); per-patch sums into the patch record, per-workgroup partials of
//                       (count, sum f, sum Q / D^2).
//   dn_finish_kernel    one workgroup: partials in index order -> loss = sum f / count (0 / 0 = NaN on an empty mask, as the
//                       reference), the weighted total, and the scalars the backward reads.
// backward = 1 launch: dn_bwd_kernel, one lane per pixel, recomputes d with the forward's arithmetic (same bits, same mask;
//   this file is compiled with -ffp-contract=off) and evaluates
//     dL/dx_j = k [ (g_j - G_l / n) / D_l  -  (local) Q_l / D_l^2 * c_j / ((n - 1) s_l)  -  0.01 (x_j - M) / ((N - 1) std_all) * T ]
//   with k = weight * dL/dloss / count read from device memory (0 on an empty mask), T = sum_l Q_l / D_l^2, plus the
//   smoothness term's four neighbours.
//
// Mapping: a workgroup takes G = max(1, 256 / p) consecutive patches of one patch row; lane t owns image column x0 + t (+ 256 k
// when p > 256) and walks the p rows, so consecutive lanes read consecutive pixels of a row and a lane never leaves its
// patch.  The p column sums of a patch meet in LDS and are added by the patch's first lane in column order.  No float
// atomics, no host synchronisation: every sum has one fixed order.
#include "gs_common.h"
#include "gs_reduce.h"

namespace {

#define DN_IMG_CHUNK 2048  // pixels one image-walk workgroup takes (8 per lane)
#define DN_REC 8           // floats per patch record: m_x, SS_x, m_t, SS_t, G, Q, -, -
#define DN_SP 6            // float64 per stats partial: sum m_x, sum m_x^2, sum SS_x, and the same for the target
#define DN_AP 3            // float64 per apply partial: masked count, sum f(d), sum Q / D^2
#define DN_IP 6            // float64 per image partial: sum (x - x0), sum (x - x0)^2, the same for the target, smooth num, den

struct DnTerm {
  int on, p, Lx, Ly, G, wgx, nwg, glob, l1;
  float margin, w;
  float* rec;      // [Lx * Ly][DN_REC]
  double* spart;   // [nwg][DN_SP]
  double* apart;   // [nwg][DN_AP]
  uint8_t* mask;   // [Lx * Ly * p * p] or NULL
};

// what the one-workgroup kernels leave for the others
struct DnGlobals {
  double M[2];       // mean of the cropped input, per term
  double cnt[2];     // masked elements
  double T[2];       // sum_l Q_l / D_l^2
  double den;        // smoothness denominator
  float sig_x[2], sig_t[2];  // std_all (unbiased, cropped area)
  float S_x, S_t;    // unbiased std of the whole image
  float loss[4];     // total, term 0, term 1, smoothness
};

struct DnArgs {
  const float* x;    // input depth [H, W]
  const float* t;    // target [H, W] (patch terms)
  const float* img;  // smoothness guide [C, H, W]
  int C, H, W, smooth, need_S, nimg;
  float w_smooth;
  DnTerm term[2];
  double* ipart;     // [nimg][DN_IP]
  DnGlobals* g;
};

struct DnLayout {
  size_t off_g, off_ip, off_rec[2], off_sp[2], off_ap[2], total;
};

static DnTerm dn_term(int H, int W, int p) {
  DnTerm t = {};
  if (p <= 0) return t;
  t.on = 1;
  t.p = p;
  t.Lx = W / p;
  t.Ly = H / p;
  t.G = p >= GS_BLOCK ? 1 : GS_BLOCK / p;
  t.wgx = (t.Lx + t.G - 1) / t.G;
  t.nwg = t.wgx * t.Ly;
  return t;
}

static DnLayout dn_layout(int H, int W, const DnTerm* tm) {
  DnLayout l;
  size_t o = 0;
  l.off_g = o; o += gs_align(sizeof(DnGlobals));
  const size_t nimg = ((size_t)H * W + DN_IMG_CHUNK - 1) / DN_IMG_CHUNK;
  l.off_ip = o; o += gs_align(nimg * DN_IP * sizeof(double));
  for (int k = 0; k < 2; k++) {
    const size_t L = tm[k].on ? (size_t)tm[k].Lx * tm[k].Ly : 0, nwg = tm[k].on ? (size_t)tm[k].nwg : 0;
    l.off_rec[k] = o; o += gs_align(L * DN_REC * sizeof(float));
    l.off_sp[k] = o; o += gs_align(nwg * DN_SP * sizeof(double));
    l.off_ap[k] = o; o += gs_align(nwg * DN_AP * sizeof(double));
  }
  l.total = o;
  return l;
}

// ---- the arithmetic forward and backward share (same expressions -> same bits -> same mask) ----
struct DnScale { float sx, Dx, Dt; };
__device__ __forceinline__ DnScale dn_scales(const float* rec, const DnTerm& tm, const DnGlobals* g, int k) {
  const float nm1 = (float)(tm.p * tm.p - 1);
  DnScale s;
  s.sx = sqrtf(rec[1] / nm1);
  const float st = sqrtf(rec[3] / nm1);
  s.Dx = (tm.glob ? g->S_x : s.sx) + 1e-2f * g->sig_x[k];
  s.Dt = (tm.glob ? g->S_t : st) + 1e-2f * g->sig_t[k];
  return s;
}
__device__ __forceinline__ float dn_diff(float x, float t, const float* rec, const DnScale& s) {
  return (x - rec[0]) / s.Dx - (t - rec[2]) / s.Dt;
}
__device__ __forceinline__ float dn_g(float d, float margin, int l1) {  // f'(d) on the mask, 0 off it
  if (!(fabsf(d) > margin)) return 0.f;
  return l1 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 2.f * d;
}
__device__ __forceinline__ float dn_edge_w(const float* img, int C, size_t plane, size_t a, size_t b) {
  float s = 0.f;
  for (int c = 0; c < C; c++) s += fabsf(img[c * plane + a] - img[c * plane + b]);
  return expf(-(s / (float)C));
}
__device__ __forceinline__ float dn_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// v[q] of the lanes [t0, t0 + span) -> their sum, in lane order, at the lane `lead` (t == t0); sh: [NQ][GS_BLOCK].  A patch's
// lanes are a segment of the workgroup, not the whole of it, and the patch record's bits are this serial order: it is NOT
// gs_reduce.h's tree and stays here on purpose.
template <int NQ>
__device__ __forceinline__ void dn_segment_sum(double (&v)[NQ], double* sh, int t, bool lead, int span) {
  for (int q = 0; q < NQ; q++) sh[q * GS_BLOCK + t] = v[q];
  __syncthreads();
  if (lead)
    for (int q = 0; q < NQ; q++) {
      double a = 0.0;
      for (int i = 0; i < span; i++) a += sh[q * GS_BLOCK + t + i];
      v[q] = a;
    }
  __syncthreads();
}

// which patches a patch workgroup owns and where lane t stands in them
struct DnPlace {
  int py, px0, npatch, ncols, x0, y0, lp, span;
  bool lead;
};
__device__ __forceinline__ DnPlace dn_place(const DnTerm& tm, int b, int t) {
  DnPlace c;
  c.py = b / tm.wgx;
  c.px0 = (b % tm.wgx) * tm.G;
  c.npatch = min(tm.G, tm.Lx - c.px0);
  c.ncols = c.npatch * tm.p;
  c.x0 = c.px0 * tm.p;
  c.y0 = c.py * tm.p;
  c.lp = tm.G == 1 ? 0 : t / tm.p;       // a lane's columns t, t + 256, ... all lie in this patch
  c.span = min(tm.p, GS_BLOCK);
  c.lead = t < c.ncols && (tm.G == 1 ? t == 0 : t % tm.p == 0);
  return c;
}

__global__ __launch_bounds__(GS_BLOCK) void dn_stats_kernel(DnArgs a) {
  __shared__ double sh[4 * GS_BLOCK];
  __shared__ float sh_mean[2 * GS_BLOCK];
  __shared__ double sh_p[DN_SP * GS_BLOCK];
  const int t = threadIdx.x;
  int b = blockIdx.x;
  for (int k = 0; k < 2; k++) {
    const DnTerm& tm = a.term[k];
    if (!tm.on) continue;
    if (b >= tm.nwg) { b -= tm.nwg; continue; }
    const DnPlace c = dn_place(tm, b, t);
    const int p = tm.p;
    const double n = (double)p * p;
    double v[2] = {0.0, 0.0};
    for (int col = t; col < c.ncols; col += GS_BLOCK)
      for (int r = 0; r < p; r++) {
        const size_t i = (size_t)(c.y0 + r) * a.W + c.x0 + col;
        v[0] += (double)a.x[i];
        v[1] += (double)a.t[i];
      }
    dn_segment_sum<2>(v, sh, t, c.lead, c.span);
    if (c.lead) {
      sh_mean[2 * c.lp] = (float)(v[0] / n);
      sh_mean[2 * c.lp + 1] = (float)(v[1] / n);
    }
    __syncthreads();
    const float mx = sh_mean[2 * c.lp], mt = sh_mean[2 * c.lp + 1];
    double q[2] = {0.0, 0.0};
    for (int col = t; col < c.ncols; col += GS_BLOCK)
      for (int r = 0; r < p; r++) {
        const size_t i = (size_t)(c.y0 + r) * a.W + c.x0 + col;
        const double cx = (double)(a.x[i] - mx), ct = (double)(a.t[i] - mt);
        q[0] += cx * cx;
        q[1] += ct * ct;
      }
    dn_segment_sum<2>(q, sh, t, c.lead, c.span);
    if (c.lead) {
      float* rec = tm.rec + (size_t)(c.py * tm.Lx + c.px0 + c.lp) * DN_REC;
      const float ssx = (float)q[0], sst = (float)q[1];
      rec[0] = mx; rec[1] = ssx; rec[2] = mt; rec[3] = sst;
      rec[4] = rec[5] = rec[6] = rec[7] = 0.f;
      // (what the other kernels read back is what enters the combination: the rounded fp32 values)
      sh_p[0 * GS_BLOCK + c.lp] = (double)mx;
      sh_p[1 * GS_BLOCK + c.lp] = (double)mx * (double)mx;
      sh_p[2 * GS_BLOCK + c.lp] = (double)ssx;
      sh_p[3 * GS_BLOCK + c.lp] = (double)mt;
      sh_p[4 * GS_BLOCK + c.lp] = (double)mt * (double)mt;
      sh_p[5 * GS_BLOCK + c.lp] = (double)sst;
    }
    __syncthreads();
    if (t < DN_SP) {
      double s = 0.0;
      for (int i = 0; i < c.npatch; i++) s += sh_p[t * GS_BLOCK + i];
      tm.spart[(size_t)b * DN_SP + t] = s;
    }
    return;
  }
  // ---- image walk: chunk b of the whole (uncropped) image ----
  if (b >= a.nimg) return;
  const size_t N = (size_t)a.H * a.W;
  const float x0 = a.x[0], t0 = a.need_S ? a.t[0] : 0.f;
  double v[DN_IP] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < DN_IMG_CHUNK / GS_BLOCK; j++) {
    const size_t i = (size_t)b * DN_IMG_CHUNK + (size_t)j * GS_BLOCK + t;
    if (i >= N) break;
    const float xv = a.x[i];
    if (a.need_S) {
      const double dx = (double)(xv - x0), dt = (double)(a.t[i] - t0);
      v[0] += dx; v[1] += dx * dx; v[2] += dt; v[3] += dt * dt;
    }
    if (a.smooth) {
      const int px = (int)(i % a.W), py = (int)(i / a.W);
      if (px + 1 < a.W) {
        const float w = dn_edge_w(a.img, a.C, N, i, i + 1);
        v[4] += (double)(fabsf(xv - a.x[i + 1]) * w);
        v[5] += (double)w;
      }
      if (py + 1 < a.H) {
        const float w = dn_edge_w(a.img, a.C, N, i, i + a.W);
        v[4] += (double)(fabsf(xv - a.x[i + a.W]) * w);
        v[5] += (double)w;
      }
    }
  }
  gs_block_tree_sum<GS_BLOCK>(v, sh_p, t);
  if (t < DN_IP) a.ipart[(size_t)b * DN_IP + t] = v[t];
}

__global__ __launch_bounds__(GS_BLOCK) void dn_globals_kernel(DnArgs a) {
  __shared__ double sh[DN_SP * GS_BLOCK];
  const int t = threadIdx.x;
  if (a.need_S || a.smooth) {
    double v[DN_IP];
    gs_partials_tree_sum<GS_BLOCK>(a.ipart, a.nimg, v, sh, t);
    __syncthreads();  // sh is written again below
    if (t == 0) {
      const double N = (double)a.H * a.W;
      a.g->S_x = (float)sqrt(fmax(v[1] - v[0] * v[0] / N, 0.0) / (N - 1.0));
      a.g->S_t = (float)sqrt(fmax(v[3] - v[2] * v[2] / N, 0.0) / (N - 1.0));
      a.g->den = v[5];
      a.g->loss[3] = a.smooth ? (float)(v[4] / v[5]) : 0.f;
    }
  } else if (t == 0) {
    a.g->den = 0.0;
    a.g->loss[3] = 0.f;
  }
  for (int k = 0; k < 2; k++) {
    const DnTerm& tm = a.term[k];
    if (!tm.on) continue;
    double v[DN_SP];
    gs_partials_tree_sum<GS_BLOCK>(tm.spart, tm.nwg, v, sh, t);
    __syncthreads();  // sh is written again by the next term
    if (t == 0) {
      const double L = (double)tm.Lx * tm.Ly, n = (double)tm.p * tm.p, N = L * n;
      const double ssx = v[2] + n * fmax(v[1] - v[0] * v[0] / L, 0.0);
      const double sst = v[5] + n * fmax(v[4] - v[3] * v[3] / L, 0.0);
      a.g->M[k] = v[0] / L;
      a.g->sig_x[k] = (float)sqrt(ssx / (N - 1.0));
      a.g->sig_t[k] = (float)sqrt(sst / (N - 1.0));
    }
  }
}

__global__ __launch_bounds__(GS_BLOCK) void dn_apply_kernel(DnArgs a) {
  __shared__ double sh[4 * GS_BLOCK];
  __shared__ double sh_p[DN_AP * GS_BLOCK];
  const int t = threadIdx.x;
  int b = blockIdx.x;
  for (int k = 0; k < 2; k++) {
    const DnTerm& tm = a.term[k];
    if (!tm.on) continue;
    if (b >= tm.nwg) { b -= tm.nwg; continue; }
    const DnPlace c = dn_place(tm, b, t);
    const int p = tm.p;
    const size_t l = (size_t)c.py * tm.Lx + c.px0 + c.lp;
    float* rec = tm.rec + l * DN_REC;
    double v[4] = {0.0, 0.0, 0.0, 0.0};  // count, sum f(d), sum g, sum g (x - m)
    DnScale s = {1.f, 1.f, 1.f};
    if (t < c.ncols) {
      s = dn_scales(rec, tm, a.g, k);
      const float mx = rec[0];
      uint8_t* mask = tm.mask ? tm.mask + l * (size_t)p * p : nullptr;
      for (int col = t; col < c.ncols; col += GS_BLOCK) {
        const int cc = col - c.lp * p;
        for (int r = 0; r < p; r++) {
          const size_t i = (size_t)(c.y0 + r) * a.W + c.x0 + col;
          const float xv = a.x[i];
          const float d = dn_diff(xv, a.t[i], rec, s);
          const bool m = fabsf(d) > tm.margin;
          if (mask) mask[(size_t)r * p + cc] = m ? 1 : 0;
          if (m) {
            const float g = dn_g(d, tm.margin, tm.l1);
            v[0] += 1.0;
            v[1] += tm.l1 ? (double)fabsf(d) : (double)d * (double)d;
            v[2] += (double)g;
            v[3] += (double)g * (double)(xv - mx);
          }
        }
      }
    }
    dn_segment_sum<4>(v, sh, t, c.lead, c.span);
    if (c.lead) {
      rec[4] = (float)v[2];
      rec[5] = (float)v[3];
      sh_p[0 * GS_BLOCK + c.lp] = v[0];
      sh_p[1 * GS_BLOCK + c.lp] = v[1];
      sh_p[2 * GS_BLOCK + c.lp] = (double)rec[5] / ((double)s.Dx * (double)s.Dx);
    }
    __syncthreads();
    if (t < DN_AP) {
      double sum = 0.0;
      for (int i = 0; i < c.npatch; i++) sum += sh_p[t * GS_BLOCK + i];
      tm.apart[(size_t)b * DN_AP + t] = sum;
    }
    return;
  }
}

// mode 0: loss_out[0] = term 0 (or the smoothness loss when no term is on); mode 1: loss_out[0..3] = total, term 0, term 1, smooth
__global__ __launch_bounds__(GS_BLOCK) void dn_finish_kernel(DnArgs a, int mode, float* loss_out) {
  __shared__ double sh[DN_AP * GS_BLOCK];
  const int t = threadIdx.x;
  float loss[2] = {0.f, 0.f};
  for (int k = 0; k < 2; k++) {
    const DnTerm& tm = a.term[k];
    if (!tm.on) {
      if (t == 0) { a.g->cnt[k] = 0.0; a.g->T[k] = 0.0; a.g->loss[1 + k] = 0.f; }
      continue;
    }
    double v[DN_AP];
    gs_partials_tree_sum<GS_BLOCK>(tm.apart, tm.nwg, v, sh, t);
    __syncthreads();  // sh is written again by the next term
    loss[k] = (float)(v[1] / v[0]);  // 0 / 0 = NaN on an empty mask: the reference's mean over no elements
    if (t == 0) {
      a.g->cnt[k] = v[0];
      a.g->T[k] = v[2];
      a.g->loss[1 + k] = loss[k];
    }
  }
  if (t == 0) {
    const float ls = a.g->loss[3];  // written by dn_globals_kernel, an earlier launch
    float total = 0.f;
    if (a.term[0].on) total += a.term[0].w * loss[0];
    if (a.smooth) total += a.w_smooth * ls;
    if (a.term[1].on) total += a.term[1].w * loss[1];
    a.g->loss[0] = total;
    if (mode == 0) {
      loss_out[0] = a.term[0].on ? loss[0] : ls;
    } else {
      loss_out[0] = total; loss_out[1] = loss[0]; loss_out[2] = loss[1]; loss_out[3] = ls;
    }
  }
}

__global__ __launch_bounds__(GS_BLOCK) void dn_bwd_kernel(DnArgs a, const float* dloss, float* grad) {
  const size_t N = (size_t)a.H * a.W;
  const size_t i = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int px = (int)(i % a.W), py = (int)(i / a.W);
  const float up = dloss[0];
  const float xv = a.x[i];
  float out = 0.f;
  for (int k = 0; k < 2; k++) {
    const DnTerm& tm = a.term[k];
    if (!tm.on) continue;
    const int p = tm.p;
    const int bx = px / p, by = py / p;
    if (bx >= tm.Lx || by >= tm.Ly) continue;
    const double cnt = a.g->cnt[k];
    if (!(cnt > 0.0)) continue;  // empty mask: NaN loss, zero gradient
    const float* rec = tm.rec + ((size_t)by * tm.Lx + bx) * DN_REC;
    const DnScale s = dn_scales(rec, tm, a.g, k);
    const float d = dn_diff(xv, a.t[i], rec, s);
    const double g = (double)dn_g(d, tm.margin, tm.l1);
    const double n = (double)p * p, Nc = n * (double)tm.Lx * tm.Ly;
    const double Dx = (double)s.Dx, c = (double)(xv - rec[0]);
    double v = (g - (double)rec[4] / n) / Dx;
    if (!tm.glob) v -= (double)rec[5] / (Dx * Dx) * (c / ((n - 1.0) * (double)s.sx));
    v -= 1e-2 * ((double)xv - a.g->M[k]) / ((Nc - 1.0) * (double)a.g->sig_x[k]) * a.g->T[k];
    out += (float)(v * ((double)tm.w * (double)up / cnt));
  }
  if (a.smooth) {
    float v = 0.f;
    if (px + 1 < a.W) v += dn_sign(xv - a.x[i + 1]) * dn_edge_w(a.img, a.C, N, i, i + 1);
    if (px > 0) v -= dn_sign(a.x[i - 1] - xv) * dn_edge_w(a.img, a.C, N, i - 1, i);
    if (py + 1 < a.H) v += dn_sign(xv - a.x[i + a.W]) * dn_edge_w(a.img, a.C, N, i, i + a.W);
    if (py > 0) v -= dn_sign(a.x[i - a.W] - xv) * dn_edge_w(a.img, a.C, N, i - a.W, i);
    out += (float)((double)v * ((double)a.w_smooth * (double)up / a.g->den));
  }
  grad[i] = out;
}

// ---- host side ----
static int dn_check(int H, int W, int p0, int p1) {
  if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) return GS_E_SHAPE;
  const int lim = H < W ? H : W;
  if (p0 < 0 || p1 < 0 || p0 == 1 || p1 == 1 || p0 > lim || p1 > lim) return GS_E_SHAPE;
  return GS_OK;
}

static DnArgs dn_args(const float* x, const float* t, const float* img, int C, int H, int W, int p0, int p1, void* tmp) {
  DnArgs a = {};
  a.x = x; a.t = t; a.img = img; a.C = C; a.H = H; a.W = W;
  a.term[0] = dn_term(H, W, p0);
  a.term[1] = dn_term(H, W, p1);
  a.nimg = (int)(((size_t)H * W + DN_IMG_CHUNK - 1) / DN_IMG_CHUNK);
  const DnLayout l = dn_layout(H, W, a.term);
  char* base = (char*)tmp;
  a.g = (DnGlobals*)(base + l.off_g);
  a.ipart = (double*)(base + l.off_ip);
  for (int k = 0; k < 2; k++) {
    a.term[k].rec = (float*)(base + l.off_rec[k]);
    a.term[k].spart = (double*)(base + l.off_sp[k]);
    a.term[k].apart = (double*)(base + l.off_ap[k]);
    a.term[k].w = 1.f;
  }
  return a;
}

static int dn_forward(DnArgs& a, int mode, float* loss_out, hipStream_t s) {
  a.need_S = (a.term[0].on && a.term[0].glob) || (a.term[1].on && a.term[1].glob);
  const int walk = (a.need_S || a.smooth) ? a.nimg : 0;
  const int npatch_wg = (a.term[0].on ? a.term[0].nwg : 0) + (a.term[1].on ? a.term[1].nwg : 0);
  if (!walk) a.nimg = 0;
  hipLaunchKernelGGL(dn_stats_kernel, dim3(npatch_wg + walk), dim3(GS_BLOCK), 0, s, a);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(dn_globals_kernel, dim3(1), dim3(GS_BLOCK), 0, s, a);
  GS_LAUNCH_CHECK(s, 0);
  if (npatch_wg) {
    hipLaunchKernelGGL(dn_apply_kernel, dim3(npatch_wg), dim3(GS_BLOCK), 0, s, a);
    GS_LAUNCH_CHECK(s, 0);
  }
  hipLaunchKernelGGL(dn_finish_kernel, dim3(1), dim3(GS_BLOCK), 0, s, a, mode, loss_out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

static int dn_backward(const DnArgs& a, const float* dloss, float* grad, hipStream_t s) {
  const size_t N = (size_t)a.H * a.W;
  hipLaunchKernelGGL(dn_bwd_kernel, dim3((unsigned)((N + GS_BLOCK - 1) / GS_BLOCK)), dim3(GS_BLOCK), 0, s, a, dloss, grad);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // namespace

extern "C" {

size_t gs_depth_norm_tmp_bytes(int32_t H, int32_t W, int32_t p_local, int32_t p_global) {
  if (dn_check(H, W, p_local, p_global)) return 0;
  DnTerm tm[2] = {dn_term(H, W, p_local), dn_term(H, W, p_global)};
  return dn_layout(H, W, tm).total;
}

int gs_depth_norm_fwd(const float* input, const float* target, int32_t H, int32_t W, int32_t p, float margin, int32_t flags,
                      void* tmp, float* loss_out, uint8_t* mask_out, void* stream) {
  const int rc = dn_check(H, W, p, 0);
  if (rc) return rc;
  if (p < 2 || (flags & ~(GS_DN_GLOBAL | GS_DN_L1))) return GS_E_SHAPE;
  if (!input || !target || !tmp || !loss_out) return GS_E_NULL;
  DnArgs a = dn_args(input, target, nullptr, 0, H, W, p, 0, tmp);
  a.term[0].margin = margin;
  a.term[0].glob = (flags & GS_DN_GLOBAL) != 0;
  a.term[0].l1 = (flags & GS_DN_L1) != 0;
  a.term[0].mask = mask_out;
  return dn_forward(a, 0, loss_out, (hipStream_t)stream);
}

int gs_depth_norm_bwd(const float* input, const float* target, int32_t H, int32_t W, int32_t p, float margin, int32_t flags,
                      const void* tmp, const float* dloss_dev, float* grad_input, void* stream) {
  const int rc = dn_check(H, W, p, 0);
  if (rc) return rc;
  if (p < 2 || (flags & ~(GS_DN_GLOBAL | GS_DN_L1))) return GS_E_SHAPE;
  if (!input || !target || !tmp || !dloss_dev || !grad_input) return GS_E_NULL;
  DnArgs a = dn_args(input, target, nullptr, 0, H, W, p, 0, (void*)tmp);
  a.term[0].margin = margin;
  a.term[0].glob = (flags & GS_DN_GLOBAL) != 0;
  a.term[0].l1 = (flags & GS_DN_L1) != 0;
  return dn_backward(a, dloss_dev, grad_input, (hipStream_t)stream);
}

int gs_depth_smooth_fwd(const float* depth, const float* img, int32_t C, int32_t H, int32_t W, void* tmp, float* loss_out,
                        void* stream) {
  const int rc = dn_check(H, W, 0, 0);
  if (rc) return rc;
  if (C < 1) return GS_E_SHAPE;
  if (!depth || !img || !tmp || !loss_out) return GS_E_NULL;
  DnArgs a = dn_args(depth, nullptr, img, C, H, W, 0, 0, tmp);
  a.smooth = 1;
  a.w_smooth = 1.f;
  return dn_forward(a, 0, loss_out, (hipStream_t)stream);
}

int gs_depth_smooth_bwd(const float* depth, const float* img, int32_t C, int32_t H, int32_t W, const void* tmp,
                        const float* dloss_dev, float* grad_depth, void* stream) {
  const int rc = dn_check(H, W, 0, 0);
  if (rc) return rc;
  if (C < 1) return GS_E_SHAPE;
  if (!depth || !img || !tmp || !dloss_dev || !grad_depth) return GS_E_NULL;
  DnArgs a = dn_args(depth, nullptr, img, C, H, W, 0, 0, (void*)tmp);
  a.smooth = 1;
  a.w_smooth = 1.f;
  return dn_backward(a, dloss_dev, grad_depth, (hipStream_t)stream);
}

static int dn_reg_args(DnArgs& a, const float* input, const float* target, int32_t H, int32_t W, int32_t p_local,
                       int32_t p_global, float margin, float w_local, float w_global, float w_smooth, void* tmp) {
  const int rc = dn_check(H, W, p_local, p_global);
  if (rc) return rc;
  if (p_local < 2 || p_global < 2) return GS_E_SHAPE;
  if (!input || !target || !tmp) return GS_E_NULL;
  a = dn_args(input, target, target, 1, H, W, p_local, p_global, tmp);
  a.term[0].margin = a.term[1].margin = margin;
  a.term[1].glob = 1;
  a.term[0].w = w_local;
  a.term[1].w = w_global;
  a.smooth = w_smooth != 0.f;
  a.w_smooth = w_smooth;
  return GS_OK;
}

int gs_dng_depth_reg_fwd(const float* input, const float* target, int32_t H, int32_t W, int32_t p_local, int32_t p_global,
                         float margin, float w_local, float w_global, float w_smooth, void* tmp, float* loss_out,
                         uint8_t* mask_local, uint8_t* mask_global, void* stream) {
  DnArgs a;
  const int rc = dn_reg_args(a, input, target, H, W, p_local, p_global, margin, w_local, w_global, w_smooth, tmp);
  if (rc) return rc;
  if (!loss_out) return GS_E_NULL;
  a.term[0].mask = mask_local;
  a.term[1].mask = mask_global;
  return dn_forward(a, 1, loss_out, (hipStream_t)stream);
}

int gs_dng_depth_reg_bwd(const float* input, const float* target, int32_t H, int32_t W, int32_t p_local, int32_t p_global,
                         float margin, float w_local, float w_global, float w_smooth, const void* tmp, const float* dloss_dev,
                         float* grad_input, void* stream) {
  DnArgs a;
  const int rc = dn_reg_args(a, input, target, H, W, p_local, p_global, margin, w_local, w_global, w_smooth, (void*)tmp);
  if (rc) return rc;
  if (!dloss_dev || !grad_input) return GS_E_NULL;
  a.need_S = 1;
  return dn_backward(a, dloss_dev, grad_input, (hipStream_t)stream);
}

}  // extern "C"
