// gs_dng_reg.hip - three per-Gaussian pieces of a DNGaussian training step, gfx950, wave64:
//   the shape / scale / opacity regulariser added to the photometric loss every iteration,
//   the view directions fed to the SH encoder,
//   the near-camera prune mask over all spiral cameras.
// Every lane takes FOUR consecutive rows: 48 bytes of a [P,3] array are three 16-byte loads, 16 bytes of a [P] array one; an
// array whose base is not 16-byte aligned, and the last rows, go element by element (the row-to-lane assignment is the same).
//
// regulariser (scaling s [P,3], opacity o [P]; H = {o > 0.2f}, L = {o < 0.2f}; a tie for the row max / min -> lowest column):
//   shape = mean mx / mn, scale = mean mx^2, opa = 1 - mean_H o^2 + mean_L (1 - o)^2, total = w . (shape, scale, opa)
//   forward = 2 launches:
//     dr_stats_kernel   s and o are read ONCE.  Each lane adds, in float64, mx / mn, mx^2, o^2 on H and (1 - o)^2 on L (each
//                       formed in fp32) and counts H and L.  Which rows a lane takes is a function of P and the grid alone (block
//                       b of a grid of G sweeps the chunks b, b + G, ... of GS_DNG_REG_BLOCK_ROWS rows); the workgroup's sums go
//                       through one fixed LDS tree into its partial.
//     dr_finish_kernel  one workgroup: the partials in index order -> out[4] = shape, scale, opa, total and the record
//                       (P, n_hi, n_lo, weights) the backward reads.  0 / 0 of an empty set is the NaN the reference gives.
//   backward = 1 launch, dr_bwd_kernel: recomputes argmax / argmin per row, float64 arithmetic rounded once,
//     d/ds[argmax] = c_shape / (P mn) + c_scale 2 mx / P,  d/ds[argmin] -= c_shape mx / (P mn^2),  the third column 0,
//     d/do = -2 c_opa o / n_hi on H, -2 c_opa (1 - o) / n_lo on L, 0 at o == 0.2f;  c = g_terms + g_total w, from device memory.
//   GS_DNG_REG_RAW: s = exp(.), o = sigmoid(.) inside the kernels (argmax / argmin on the raw values: exp is monotone), the
//     gradients times s and o (1 - o).
// view directions: n = (x - c) / |x - c| and its backward (g - n (n . g)) / |x - c| in float64, rounded once.
// near mask: the centres go through LDS once per workgroup, each lane tests its four rows in registers against one centre after
//   the other (fp32 norm, as the reference; the root is folded into the threshold, exactly) and leaves the loop once all four are
//   set; one byte per row.
// No atomics, no read-back, no host synchronisation: two runs give the same bits.
#include "gs_common.h"
#include "gs_dng_reg_act.h"
#include "gs_launch.h"
#include "gs_reduce.h"

namespace {

#define DR_ROWS 4  // rows per lane and chunk
#define DR_Q 4     // float64 sums per partial
static_assert(DR_ROWS * GS_BLOCK == GS_DNG_REG_BLOCK_ROWS, "a chunk is four rows per lane");
#define DR_MAX_P ((int64_t)1 << 40)
#define NM_TILE 256  // centres in LDS at a time

struct DrRecord {
  int64_t P, n_hi, n_lo;
  double w[3];
};

struct DrPartial {
  double s[DR_Q];
  unsigned long long n[2];
};

struct DrArgs {
  const float* scaling;
  const float* opacity;
  size_t P;
  int raw;
  int vec_s, vec_o;  // 16-byte aligned (with the gradients, in the backward)
  int nblocks;
  double w[3];
  DrRecord* rec;
  DrPartial* part;  // [nblocks]
};

// rows [i, i + 4) of a [P,3] array (i a multiple of 4) -> v[12]; rows at or beyond P are left alone
__device__ __forceinline__ void load_rows3(const float* p, size_t i, size_t P, int vec, float (&v)[12]) {
  if (vec && i + 4 <= P) {
    const float4* q = reinterpret_cast<const float4*>(p + 3 * i);
    const float4 a = q[0], b = q[1], c = q[2];
    gs_unpack4(a, v); gs_unpack4(b, v + 4); gs_unpack4(c, v + 8);
  } else {
    for (int k = 0; k < 4; k++)
      if (i + k < P)
        for (int c = 0; c < 3; c++) v[3 * k + c] = p[3 * (i + k) + c];
  }
}

__device__ __forceinline__ void store_rows3(float* p, size_t i, size_t P, int vec, const float (&v)[12]) {
  if (vec && i + 4 <= P) {
    float4* q = reinterpret_cast<float4*>(p + 3 * i);
    q[0] = make_float4(v[0], v[1], v[2], v[3]);
    q[1] = make_float4(v[4], v[5], v[6], v[7]);
    q[2] = make_float4(v[8], v[9], v[10], v[11]);
  } else {
    for (int k = 0; k < 4; k++)
      if (i + k < P)
        for (int c = 0; c < 3; c++) p[3 * (i + k) + c] = v[3 * k + c];
  }
}

// one row of scaling: the columns of its max and min (a tie: the lowest column) and the two activated values
struct DrRow {
  float mx, mn;
  int amax, amin;
};

__device__ __forceinline__ DrRow dr_row(const float* s, int raw) {
  DrRow r;
  r.amax = 0; r.amin = 0;
  float hi = s[0], lo = s[0];
  for (int c = 1; c < 3; c++) {
    if (s[c] > hi) { hi = s[c]; r.amax = c; }
    if (s[c] < lo) { lo = s[c]; r.amin = c; }
  }
  r.mx = raw ? dr_exp(hi) : hi;
  r.mn = raw ? dr_exp(lo) : lo;
  return r;
}

__device__ __forceinline__ void dr_opacity(float v, int raw, float& o, float& om) {
  if (raw) {
    dr_sigmoid(v, o, om);
  } else {
    o = v;
    om = 1.f - v;
  }
}

__global__ __launch_bounds__(GS_BLOCK) void dr_stats_kernel(DrArgs a) {
  __shared__ double sh[DR_Q * GS_BLOCK];
  __shared__ unsigned long long shn[2 * GS_BLOCK];
  const int t = threadIdx.x;
  double v[DR_Q] = {0.0, 0.0, 0.0, 0.0};
  unsigned long long n[2] = {0ull, 0ull};
  for (size_t base = (size_t)blockIdx.x * GS_DNG_REG_BLOCK_ROWS; base < a.P; base += (size_t)a.nblocks * GS_DNG_REG_BLOCK_ROWS) {
    const size_t i = base + DR_ROWS * (size_t)t;
    if (i >= a.P) continue;
    float s[12] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, ov[4] = {0.f, 0.f, 0.f, 0.f};
    load_rows3(a.scaling, i, a.P, a.vec_s, s);
    gs_load4(a.opacity, i, a.P, a.vec_o, ov);
    for (int k = 0; k < DR_ROWS; k++) {
      if (i + k >= a.P) break;
      const DrRow r = dr_row(s + 3 * k, a.raw);
      const float ratio = r.mx / r.mn, sq = r.mx * r.mx;
      v[0] += (double)ratio;
      v[1] += (double)sq;
      float o, om;
      dr_opacity(ov[k], a.raw, o, om);
      if (o > 0.2f) {
        const float o2 = o * o;
        v[2] += (double)o2; n[0]++;
      } else if (o < 0.2f) {
        const float m2 = om * om;
        v[3] += (double)m2; n[1]++;
      }
    }
  }
  gs_rows_put<GS_BLOCK>(v, sh, t);
  gs_rows_put<GS_BLOCK>(n, shn, t);
  gs_block_tree<GS_BLOCK, DR_Q, 2>(sh, t, shn);
  if (t == 0) {
    DrPartial p;
    for (int q = 0; q < DR_Q; q++) p.s[q] = sh[q * GS_BLOCK];
    p.n[0] = shn[0]; p.n[1] = shn[GS_BLOCK];
    a.part[blockIdx.x] = p;
  }
}

__global__ __launch_bounds__(GS_BLOCK) void dr_finish_kernel(DrArgs a, float* out) {
  __shared__ double sh[DR_Q * GS_BLOCK];
  __shared__ unsigned long long shn[2 * GS_BLOCK];
  const int t = threadIdx.x;
  double v[DR_Q] = {0.0, 0.0, 0.0, 0.0};
  unsigned long long n[2] = {0ull, 0ull};
  for (int i = t; i < a.nblocks; i += GS_BLOCK) {  // (a partial is a record of two types: not gs_partials_tree_sum's [count][N])
    for (int q = 0; q < DR_Q; q++) v[q] += a.part[i].s[q];
    n[0] += a.part[i].n[0]; n[1] += a.part[i].n[1];
  }
  gs_rows_put<GS_BLOCK>(v, sh, t);
  gs_rows_put<GS_BLOCK>(n, shn, t);
  gs_block_tree<GS_BLOCK, DR_Q, 2>(sh, t, shn);
  if (t != 0) return;
  const double P = (double)a.P, n_hi = (double)shn[0], n_lo = (double)shn[GS_BLOCK];
  const double shape = sh[0] / P, scale = sh[GS_BLOCK] / P;
  const double opa = 1.0 - sh[2 * GS_BLOCK] / n_hi + sh[3 * GS_BLOCK] / n_lo;  // 0 / 0 of an empty set: NaN
  DrRecord r;
  r.P = (int64_t)a.P; r.n_hi = (int64_t)shn[0]; r.n_lo = (int64_t)shn[GS_BLOCK];
  for (int k = 0; k < 3; k++) r.w[k] = a.w[k];
  *a.rec = r;
  out[0] = (float)shape;
  out[1] = (float)scale;
  out[2] = (float)opa;
  out[3] = (float)(a.w[0] * shape + a.w[1] * scale + a.w[2] * opa);
}

__global__ __launch_bounds__(GS_BLOCK) void dr_bwd_kernel(DrArgs a, const float* g_terms, const float* g_total, float* g_scaling,
                                                          float* g_opacity) {
  const size_t i = DR_ROWS * ((size_t)blockIdx.x * GS_BLOCK + threadIdx.x);
  if (i >= a.P) return;
  const DrRecord* rec = a.rec;
  const double gt = g_total ? (double)g_total[0] : 0.0;
  double c[3];
  for (int k = 0; k < 3; k++) c[k] = (g_terms ? (double)g_terms[k] : 0.0) + gt * rec->w[k];
  const double invP = 1.0 / (double)rec->P;
  if (g_scaling) {
    float s[12] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, gs[12];
    load_rows3(a.scaling, i, a.P, a.vec_s, s);
    for (int k = 0; k < DR_ROWS; k++) {
      const DrRow r = dr_row(s + 3 * k, a.raw);
      const double mx = (double)r.mx, mn = (double)r.mn, inv = 1.0 / mn;
      double gmax = (c[0] * inv + c[1] * 2.0 * mx) * invP;
      double gmin = -(c[0] * mx * inv * inv) * invP;
      if (a.raw) { gmax *= mx; gmin *= mn; }  // ds / draw = s
      for (int col = 0; col < 3; col++) {
        double g = 0.0;
        if (col == r.amax) g += gmax;
        if (col == r.amin) g += gmin;
        gs[3 * k + col] = (col == r.amax || col == r.amin) ? (float)g : 0.f;
      }
    }
    store_rows3(g_scaling, i, a.P, a.vec_s, gs);
  }
  if (g_opacity) {
    float ov[4] = {0.f, 0.f, 0.f, 0.f}, go[4];
    gs_load4(a.opacity, i, a.P, a.vec_o, ov);
    const double k_hi = -2.0 * c[2] / (double)rec->n_hi, k_lo = -2.0 * c[2] / (double)rec->n_lo;  // used by members only
    for (int k = 0; k < DR_ROWS; k++) {
      float o, om;
      dr_opacity(ov[k], a.raw, o, om);
      double g = 0.0;
      if (o > 0.2f) g = k_hi * (double)o;
      else if (o < 0.2f) g = k_lo * (double)om;
      else { go[k] = 0.f; continue; }
      if (a.raw) g *= (double)o * (double)om;  // do / draw = o (1 - o)
      go[k] = (float)g;
    }
    gs_store4(g_opacity, i, a.P, a.vec_o, go);
  }
}

// ---- view directions ----
__global__ __launch_bounds__(GS_BLOCK) void vd_fwd_kernel(const float* xyz, const float* campos, size_t P, int vec, float* out) {
  const size_t i = DR_ROWS * ((size_t)blockIdx.x * GS_BLOCK + threadIdx.x);
  if (i >= P) return;
  const double c[3] = {(double)campos[0], (double)campos[1], (double)campos[2]};
  float x[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, n[12];
  load_rows3(xyz, i, P, vec, x);
  for (int k = 0; k < DR_ROWS; k++) {
    const double dx = (double)x[3 * k] - c[0], dy = (double)x[3 * k + 1] - c[1], dz = (double)x[3 * k + 2] - c[2];
    const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);  // at the centre: 0 * inf = NaN, the reference's 0 / 0
    n[3 * k] = (float)(dx * inv); n[3 * k + 1] = (float)(dy * inv); n[3 * k + 2] = (float)(dz * inv);
  }
  store_rows3(out, i, P, vec, n);
}

__global__ __launch_bounds__(GS_BLOCK) void vd_bwd_kernel(const float* xyz, const float* campos, size_t P, int vec, const float* g,
                                                          float* g_xyz) {
  const size_t i = DR_ROWS * ((size_t)blockIdx.x * GS_BLOCK + threadIdx.x);
  if (i >= P) return;
  const double c[3] = {(double)campos[0], (double)campos[1], (double)campos[2]};
  float x[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float gv[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gx[12];
  load_rows3(xyz, i, P, vec, x);
  load_rows3(g, i, P, vec, gv);
  for (int k = 0; k < DR_ROWS; k++) {
    const double dx = (double)x[3 * k] - c[0], dy = (double)x[3 * k + 1] - c[1], dz = (double)x[3 * k + 2] - c[2];
    const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
    const double nx = dx * inv, ny = dy * inv, nz = dz * inv;
    const double ga = (double)gv[3 * k], gb = (double)gv[3 * k + 1], gc = (double)gv[3 * k + 2];
    const double dot = nx * ga + ny * gb + nz * gc;
    gx[3 * k] = (float)((ga - nx * dot) * inv);
    gx[3 * k + 1] = (float)((gb - ny * dot) * inv);
    gx[3 * k + 2] = (float)((gc - nz * dot) * inv);
  }
  store_rows3(g_xyz, i, P, vec, gx);
}

// ---- near-camera mask ----
// sqrtf is monotone, so sqrtf(d2) < near  <=>  d2 <= t2 with t2 the largest float whose root is below `near`: found once per lane
// (near * near is within an ulp or two of it), it takes the root out of the K tests per row without moving a single decision.
// near <= 0 or NaN: nothing is closer, t2 = -1.
__device__ __forceinline__ float nm_threshold(float near) {
  if (!(near > 0.f)) return -1.f;
  float t = near * near;
  if (!(t <= 3.402823466e38f)) t = 3.402823466e38f;
  for (int it = 0; it < 4 && t > 0.f && !(sqrtf(t) < near); it++) t = __uint_as_float(__float_as_uint(t) - 1u);
  for (int it = 0; it < 4; it++) {
    const float up = __uint_as_float(__float_as_uint(t) + 1u);
    if (!(sqrtf(up) < near)) break;
    t = up;
  }
  return t;
}

__global__ __launch_bounds__(GS_BLOCK) void nm_kernel(const float* xyz, size_t P, const float* centers, int K, float near, int vec_x,
                                                      int vec_m, uint8_t* mask) {
  __shared__ float sc[3 * NM_TILE];
  const int t = threadIdx.x;
  const size_t i = DR_ROWS * ((size_t)blockIdx.x * GS_BLOCK + t);
  float x[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  unsigned full = 0u, set = 0u;  // bit k: row i + k exists / is within `near` of a centre
  const float t2 = nm_threshold(near);
  if (i < P) {
    load_rows3(xyz, i, P, vec_x, x);
    for (int k = 0; k < DR_ROWS; k++)
      if (i + k < P) full |= 1u << k;
  }
  for (int k0 = 0; k0 < K; k0 += NM_TILE) {  // (every lane of the workgroup walks the tiles: the barriers are uniform)
    const int kn = K - k0 < NM_TILE ? K - k0 : NM_TILE;
    if (k0) __syncthreads();
    for (int j = t; j < 3 * kn; j += GS_BLOCK) sc[j] = centers[3 * (size_t)k0 + j];
    __syncthreads();
    for (int k = 0; k < kn && set != full; k++) {
      const float cx = sc[3 * k], cy = sc[3 * k + 1], cz = sc[3 * k + 2];
      for (int r = 0; r < DR_ROWS; r++) {
        const float dx = x[3 * r] - cx, dy = x[3 * r + 1] - cy, dz = x[3 * r + 2] - cz;
        if (dx * dx + dy * dy + dz * dz <= t2) set |= 1u << r;
      }
      set &= full;
    }
  }
  if (i >= P) return;
  if (vec_m && i + 4 <= P) {
    *reinterpret_cast<uint32_t*>(mask + i) = (set & 1u) | ((set >> 1 & 1u) << 8) | ((set >> 2 & 1u) << 16) | ((set >> 3 & 1u) << 24);
  } else {
    for (int k = 0; k < DR_ROWS; k++)
      if (i + k < P) mask[i + k] = (uint8_t)(set >> k & 1u);
  }
}

// ---- host side ----
static bool dr_p_ok(int64_t P) { return P >= 1 && P <= DR_MAX_P; }

static unsigned row_grid(size_t P) {  // one lane per four rows
  const size_t lanes = (P + DR_ROWS - 1) / DR_ROWS;
  return (unsigned)((lanes + GS_BLOCK - 1) / GS_BLOCK);
}

static DrArgs dr_args(const float* scaling, const float* opacity, int64_t P, int flags, void* tmp) {
  DrArgs a = {};
  a.scaling = scaling; a.opacity = opacity; a.P = (size_t)P;
  a.raw = (flags & GS_DNG_REG_RAW) != 0;
  a.vec_s = gs_aligned16(scaling); a.vec_o = gs_aligned16(opacity);
  a.rec = (DrRecord*)tmp;
  a.part = (DrPartial*)((char*)tmp + gs_align(sizeof(DrRecord)));
  return a;
}

}  // namespace

extern "C" {

size_t gs_dng_reg_tmp_bytes(int64_t P) {
  if (!dr_p_ok(P)) return 0;
  return gs_align(sizeof(DrRecord)) + gs_align((size_t)gs_capped_blocks((size_t)P, GS_DNG_REG_BLOCK_ROWS, GS_DNG_REG_MAX_BLOCKS) * sizeof(DrPartial));
}

int gs_dng_reg_fwd(const float* scaling, const float* opacity, int64_t P, double w_shape, double w_scale, double w_opa,
                   int32_t flags, int32_t max_blocks, void* tmp, float* out, void* stream) {
  if (!dr_p_ok(P) || max_blocks < 0 || (flags & ~GS_DNG_REG_RAW)) return GS_E_SHAPE;
  if (!scaling || !opacity || !tmp || !out) return GS_E_NULL;
  DrArgs a = dr_args(scaling, opacity, P, flags, tmp);
  a.nblocks = gs_capped_blocks(a.P, GS_DNG_REG_BLOCK_ROWS, GS_DNG_REG_MAX_BLOCKS, max_blocks);
  a.w[0] = w_shape; a.w[1] = w_scale; a.w[2] = w_opa;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dr_stats_kernel, dim3(a.nblocks), dim3(GS_BLOCK), 0, s, a);
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(dr_finish_kernel, dim3(1), dim3(GS_BLOCK), 0, s, a, out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_dng_reg_bwd(const float* scaling, const float* opacity, int64_t P, int32_t flags, const void* tmp, const float* g_terms,
                   const float* g_total, float* g_scaling, float* g_opacity, void* stream) {
  if (!dr_p_ok(P) || (flags & ~GS_DNG_REG_RAW)) return GS_E_SHAPE;
  if (!tmp || (!g_terms && !g_total) || (!g_scaling && !g_opacity) || (g_scaling && !scaling) || (g_opacity && !opacity))
    return GS_E_NULL;
  DrArgs a = dr_args(scaling, opacity, P, flags, (void*)tmp);
  a.vec_s = a.vec_s && gs_aligned16(g_scaling);
  a.vec_o = a.vec_o && gs_aligned16(g_opacity);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dr_bwd_kernel, dim3(row_grid(a.P)), dim3(GS_BLOCK), 0, s, a, g_terms, g_total, g_scaling, g_opacity);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_view_dirs_fwd(const float* xyz, const float* campos, int64_t P, float* out, void* stream) {
  if (!dr_p_ok(P)) return GS_E_SHAPE;
  if (!xyz || !campos || !out) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vd_fwd_kernel, dim3(row_grid((size_t)P)), dim3(GS_BLOCK), 0, s, xyz, campos, (size_t)P,
                     (int)(gs_aligned16(xyz) && gs_aligned16(out)), out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_view_dirs_bwd(const float* xyz, const float* campos, int64_t P, const float* g, float* g_xyz, void* stream) {
  if (!dr_p_ok(P)) return GS_E_SHAPE;
  if (!xyz || !campos || !g || !g_xyz) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vd_bwd_kernel, dim3(row_grid((size_t)P)), dim3(GS_BLOCK), 0, s, xyz, campos, (size_t)P,
                     (int)(gs_aligned16(xyz) && gs_aligned16(g) && gs_aligned16(g_xyz)), g, g_xyz);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_near_mask(const float* xyz, int64_t P, const float* centers, int32_t K, float near, uint8_t* mask, void* stream) {
  if (!dr_p_ok(P) || K < 1) return GS_E_SHAPE;
  if (!xyz || !centers || !mask) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nm_kernel, dim3(row_grid((size_t)P)), dim3(GS_BLOCK), 0, s, xyz, (size_t)P, centers, (int)K, near,
                     (int)gs_aligned16(xyz), (int)(((uintptr_t)mask & 3) == 0), mask);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
