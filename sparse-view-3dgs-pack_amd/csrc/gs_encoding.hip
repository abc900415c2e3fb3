// gs_encoding.hip - DNGaussian's input encoders (gridencoder/src/gridencoder.cu, shencoder/src/shencoder.cu):
// the multi-resolution hash / tiled grid and the Cartesian real spherical harmonics, forward and backward.
//
// Built with -ffp-contract=off: the grid's corner selection and hash are a pure function of the fp32 inputs (the test
// oracle picks the same slots from the same fp32 arithmetic).
//
// Grid backward to the embeddings (gs_grid_encode_bwd): the reference issues one float atomicAdd per (point, level,
// corner, channel), whose sum depends on arrival order.  Here the gradient is the same bits on every run:
//   1. emit   : one (global slot, entry id) pair per (point, level, corner); points outside [0,1]^D get slot = n_slots
//   2. sort   : launch_radix_sort (stable LSD) by slot - entries of one slot keep their emission order
//   3. gather : one thread per sorted entry recomputes its weight, writes w * grad[b, l, :] in sorted order, and each
//               256-entry chunk is reduced by a fixed LDS tree into chunk_sum[chunk]
//   4. mark   : the first / one-past-last sorted position of every slot that received entries
//   5. slots  : one thread per slot adds its head entries, the chunk sums of the chunks it fills entirely, and its tail
//               entries, in that order.  A skewed slot (half the points in one coarse cell) costs its thread at most
//               2 x 256 entries plus one chunk sum per 256 entries.  Every slot is written, zero where nothing landed.
// Grid backward to the inputs: one thread per (point, dim) sums dy_dx[b, l, d, c] * grad[b, l, c] over (l, c) in order.
#include "gs_common.h"
#include "gs_reduce.h"

#include <cmath>

#define ENC_MAX_LEVELS 64
#define ENC_CHUNK GS_BLOCK  // entries per chunk sum of the segmented reduction

namespace {

struct EncLevels {
  float scale[ENC_MAX_LEVELS];      // exp2f(l * S) * H - 1, in fp32
  uint32_t res[ENC_MAX_LEVELS];     // (uint32_t)ceil(scale) + 1
};

// The level geometry is computed once on the host: the fp32 product l * S, its exp2 correctly rounded to fp32 (through
// double), then * H - 1 in fp32.  The same numbers on every device, and the ones the test oracle computes.
static EncLevels enc_levels(int L, float S, int H) {
  EncLevels g;
  for (int l = 0; l < L; l++) {
    const float ls = (float)l * S;
    const float e = (float)std::exp2((double)ls);
    const float sc = e * (float)H - 1.0f;
    g.scale[l] = sc;
    g.res[l] = (uint32_t)std::ceil(sc) + 1u;
  }
  return g;
}

struct EncHeader {
  uint32_t n;  // entries of the sort
  uint32_t pad[63];
};

struct EncTmp {
  EncHeader* hdr;
  SortBufs sort;
  float* contrib;    // [N][C] sorted contributions
  float* chunk;      // [ceil(N / ENC_CHUNK)][C]
  uint32_t* seg_lo;  // [n_slots] first sorted position, ~0u = empty
  uint32_t* seg_hi;  // [n_slots] one past the last
};

static inline size_t enc_chunks(size_t N) { return (N + ENC_CHUNK - 1) / ENC_CHUNK; }

static size_t enc_bytes(size_t N, size_t C, size_t n_slots) {
  return sizeof(EncHeader) + gs_align(sort_bytes(N)) + gs_align(4 * N * C) + gs_align(4 * enc_chunks(N) * C) +
         2 * gs_align(4 * n_slots);
}

static EncTmp enc_view(void* buf, size_t N, size_t C, size_t n_slots) {
  char* p = (char*)buf;
  EncTmp t;
  t.hdr = (EncHeader*)p; p += sizeof(EncHeader);
  t.sort = sort_view(p, N); p += gs_align(sort_bytes(N));
  t.contrib = (float*)p; p += gs_align(4 * N * C);
  t.chunk = (float*)p; p += gs_align(4 * enc_chunks(N) * C);
  t.seg_lo = (uint32_t*)p; p += gs_align(4 * n_slots);
  t.seg_hi = (uint32_t*)p;
  return t;
}

// ---- grid geometry shared by the forward and the backward kernels ----
__device__ inline uint32_t grid_index(int D, uint32_t gridtype, bool align_corners, uint32_t hashmap_size, uint32_t res,
                                      const uint32_t* cell) {
  uint32_t stride = 1, index = 0;
  for (int d = 0; d < D && stride <= hashmap_size; d++) {
    index += cell[d] * stride;
    stride *= align_corners ? res : res + 1u;
  }
  if (gridtype == 0 && stride > hashmap_size) {
    const uint32_t primes[5] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u};
    index = 0;
    for (int d = 0; d < D; d++) index ^= cell[d] * primes[d];
  }
  return index % hashmap_size;
}

// Position of point x at one level: integer cell, (smoothstep'd) fraction, its complement and its derivative factor.
// The complement under smoothstep is s(1 - p) = 1 - s(p): next to a cell face 1 - s(p) cancels and the left corner's
// weight (and with it a slot's whole gradient, when that corner is its only entry) would lose its relative accuracy.
// Returns false when a coordinate lies outside [0, 1].
template <int D>
__device__ inline bool grid_locate(const float* x, float scale, bool align_corners, uint32_t interp, uint32_t* cell,
                                   float* frac, float* cfrac, float* dfrac) {
  bool in = true;
#pragma unroll
  for (int d = 0; d < D; d++) in = in && !(x[d] < 0.0f || x[d] > 1.0f);
  if (!in) return false;
#pragma unroll
  for (int d = 0; d < D; d++) {
    float p = x[d] * scale + (align_corners ? 0.0f : 0.5f);
    const float fl = floorf(p);
    cell[d] = (uint32_t)fl;
    p -= fl;
    const float q = 1.0f - p;
    if (interp == 1) {
      dfrac[d] = 6.0f * p * q;
      frac[d] = p * p * (3.0f - 2.0f * p);
      cfrac[d] = q * q * (3.0f - 2.0f * q);
    } else {
      dfrac[d] = 1.0f;
      frac[d] = p;
      cfrac[d] = q;
    }
  }
  return true;
}

template <int D>
__device__ inline float corner_weight(const float* frac, const float* cfrac, uint32_t corner) {
  float w = 1.0f;
#pragma unroll
  for (int d = 0; d < D; d++) w *= (corner >> d) & 1u ? frac[d] : cfrac[d];
  return w;
}

// one thread per (point, level), the level fastest: out[b][l * C + c], dy_dx[b][l][d][c]
template <int D, int C>
__global__ void __launch_bounds__(GS_BLOCK) grid_fwd_kernel(const float* __restrict__ inputs, const float* __restrict__ emb,
                                                             const int32_t* __restrict__ offsets, uint32_t B, uint32_t L,
                                                             EncLevels lv, uint32_t gridtype, bool align_corners,
                                                             uint32_t interp, float* __restrict__ out,
                                                             float* __restrict__ dy_dx) {
  const size_t t = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (t >= (size_t)B * L) return;
  const size_t b = t / L;
  const uint32_t l = (uint32_t)(t - b * L);
  float x[D];
#pragma unroll
  for (int d = 0; d < D; d++) x[d] = inputs[b * D + d];
  uint32_t cell[D];
  float frac[D], cfrac[D], dfrac[D];
  float* o = out + t * C;
  float* g = dy_dx ? dy_dx + t * (D * C) : nullptr;
  if (!grid_locate<D>(x, lv.scale[l], align_corners, interp, cell, frac, cfrac, dfrac)) {
#pragma unroll
    for (int c = 0; c < C; c++) o[c] = 0.0f;
    if (g)
#pragma unroll
      for (int k = 0; k < D * C; k++) g[k] = 0.0f;
    return;
  }
  const uint32_t base = (uint32_t)offsets[l];
  const uint32_t hsize = (uint32_t)offsets[l + 1] - base;
  const uint32_t res = lv.res[l];
  float val[1 << D][C];
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; c++) acc[c] = 0.0f;
#pragma unroll
  for (uint32_t k = 0; k < (1u << D); k++) {
    uint32_t cc[D];
#pragma unroll
    for (int d = 0; d < D; d++) cc[d] = cell[d] + ((k >> d) & 1u);
    const size_t row = base + grid_index(D, gridtype, align_corners, hsize, res, cc);
    const float w = corner_weight<D>(frac, cfrac, k);
#pragma unroll
    for (int c = 0; c < C; c++) {
      val[k][c] = emb[row * C + c];
      acc[c] += w * val[k][c];
    }
  }
#pragma unroll
  for (int c = 0; c < C; c++) o[c] = acc[c];
  if (!g) return;
  const float scale = lv.scale[l];
#pragma unroll
  for (int gd = 0; gd < D; gd++) {
    float r[C];
#pragma unroll
    for (int c = 0; c < C; c++) r[c] = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < (1u << D); k++) {
      if ((k >> gd) & 1u) continue;  // k = left corner along gd, k | bit = right corner
      float w = scale;
#pragma unroll
      for (int d = 0; d < D; d++)
        if (d != gd) w *= (k >> d) & 1u ? frac[d] : cfrac[d];
#pragma unroll
      for (int c = 0; c < C; c++) r[c] += w * (val[k | (1u << gd)][c] - val[k][c]) * dfrac[gd];
    }
#pragma unroll
    for (int c = 0; c < C; c++) g[gd * C + c] = r[c];
  }
}

// 1. one thread per (point, level): its 2^D (slot, entry) pairs, entry = (b * L + l) * 2^D + corner
template <int D>
__global__ void __launch_bounds__(GS_BLOCK) grid_emit_kernel(const float* __restrict__ inputs, const int32_t* __restrict__ offsets,
                                                              uint32_t B, uint32_t L, EncLevels lv, uint32_t gridtype,
                                                              bool align_corners, uint32_t n_slots, uint32_t* __restrict__ keys,
                                                              uint32_t* __restrict__ vals, EncHeader* hdr) {
  const size_t t = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (t == 0) hdr->n = (uint32_t)((size_t)B * L << D);
  if (t >= (size_t)B * L) return;
  const size_t b = t / L;
  const uint32_t l = (uint32_t)(t - b * L);
  float x[D];
#pragma unroll
  for (int d = 0; d < D; d++) x[d] = inputs[b * D + d];
  uint32_t cell[D];
  float frac[D], cfrac[D], dfrac[D];
  const bool in = grid_locate<D>(x, lv.scale[l], align_corners, 0, cell, frac, cfrac, dfrac);
  const uint32_t base = (uint32_t)offsets[l];
  const uint32_t hsize = (uint32_t)offsets[l + 1] - base;
#pragma unroll
  for (uint32_t k = 0; k < (1u << D); k++) {
    uint32_t key = n_slots;
    if (in) {
      uint32_t cc[D];
#pragma unroll
      for (int d = 0; d < D; d++) cc[d] = cell[d] + ((k >> d) & 1u);
      key = base + grid_index(D, gridtype, align_corners, hsize, lv.res[l], cc);
    }
    const uint32_t e = (uint32_t)(t << D) + k;
    keys[e] = key;
    vals[e] = e;
  }
}

// 3. one thread per sorted entry: its contribution, then the chunk's fixed-tree sum
template <int D, int C>
__global__ void __launch_bounds__(GS_BLOCK) grid_gather_kernel(const float* __restrict__ inputs, const float* __restrict__ grad,
                                                                uint32_t N, uint32_t L, EncLevels lv, bool align_corners,
                                                                uint32_t interp, uint32_t n_slots,
                                                                const uint32_t* __restrict__ keys,
                                                                const uint32_t* __restrict__ vals, float* __restrict__ contrib,
                                                                float* __restrict__ chunk) {
  __shared__ float s_sum[C][GS_BLOCK];
  const uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x;
  float v[C];
#pragma unroll
  for (int c = 0; c < C; c++) v[c] = 0.0f;
  if (i < N && keys[i] < n_slots) {
    const uint32_t e = vals[i];
    const uint32_t t = e >> D, k = e & ((1u << D) - 1u);
    const uint32_t b = t / L, l = t - b * L;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = inputs[(size_t)b * D + d];
    uint32_t cell[D];
    float frac[D], cfrac[D], dfrac[D];
    grid_locate<D>(x, lv.scale[l], align_corners, interp, cell, frac, cfrac, dfrac);
    const float w = corner_weight<D>(frac, cfrac, k);
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = w * grad[(size_t)t * C + c];
  }
  if (i < N)
#pragma unroll
    for (int c = 0; c < C; c++) contrib[(size_t)i * C + c] = v[c];
#pragma unroll
  for (int c = 0; c < C; c++) s_sum[c][threadIdx.x] = v[c];
  gs_block_tree<GS_BLOCK, C>(&s_sum[0][0], (int)threadIdx.x);
  if (threadIdx.x < C) chunk[(size_t)blockIdx.x * C + threadIdx.x] = s_sum[threadIdx.x][0];
}

// 4. the sorted range of every slot that received entries
__global__ void __launch_bounds__(GS_BLOCK) grid_mark_kernel(const uint32_t* __restrict__ keys, uint32_t N, uint32_t n_slots,
                                                              uint32_t* __restrict__ seg_lo, uint32_t* __restrict__ seg_hi) {
  const uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x;
  if (i >= N) return;
  const uint32_t k = keys[i];
  if (k >= n_slots) return;
  if (i == 0 || keys[i - 1] != k) seg_lo[k] = i;
  if (i == N - 1 || keys[i + 1] != k) seg_hi[k] = i + 1;
}

// 5. one thread per slot: head entries + whole-chunk sums + tail entries, in sorted order
template <int C>
__global__ void __launch_bounds__(GS_BLOCK) grid_slot_kernel(const uint32_t* __restrict__ seg_lo, const uint32_t* __restrict__ seg_hi,
                                                              const float* __restrict__ contrib, const float* __restrict__ chunk,
                                                              uint32_t n_slots, float* __restrict__ grad_emb) {
  const uint32_t s = blockIdx.x * GS_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; c++) acc[c] = 0.0f;
  const uint32_t lo = seg_lo[s];
  if (lo != 0xFFFFFFFFu) {
    const uint32_t hi = seg_hi[s];
    const uint32_t c_first = (lo + ENC_CHUNK - 1) / ENC_CHUNK;  // first chunk that starts inside the segment
    const uint32_t c_last = hi / ENC_CHUNK;                      // chunks [c_first, c_last) lie entirely inside it
    if (c_first >= c_last) {
      for (uint32_t i = lo; i < hi; i++)
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += contrib[(size_t)i * C + c];
    } else {
      for (uint32_t i = lo; i < c_first * ENC_CHUNK; i++)
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += contrib[(size_t)i * C + c];
      for (uint32_t j = c_first; j < c_last; j++)
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += chunk[(size_t)j * C + c];
      for (uint32_t i = c_last * ENC_CHUNK; i < hi; i++)
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += contrib[(size_t)i * C + c];
    }
  }
#pragma unroll
  for (int c = 0; c < C; c++) grad_emb[(size_t)s * C + c] = acc[c];
}

// grad_inputs[b][d] = sum over (l, c) of grad[b][l][c] * dy_dx[b][l][d][c], in that order
template <int D, int C>
__global__ void __launch_bounds__(GS_BLOCK) grid_input_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ dy_dx,
                                                                   uint32_t B, uint32_t L, float* __restrict__ grad_inputs) {
  const size_t t = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (t >= (size_t)B * D) return;
  const size_t b = t / D;
  const int d = (int)(t - b * D);
  const float* g = grad + b * L * C;
  const float* j = dy_dx + b * L * D * C + d * C;
  float r = 0.0f;
  for (uint32_t l = 0; l < L; l++)
#pragma unroll
    for (int c = 0; c < C; c++) r += g[l * C + c] * j[(size_t)l * D * C + c];
  grad_inputs[t] = r;
}

// ---- spherical harmonics: Y_l^m = (-1)^m K_lm Pbar_l^|m|(z) * {Re, Im}((x + i y)^|m|), the r^2 -> 1 polynomial forms ----
// Evaluated in double and rounded once: the recurrences below are three fp32 ulps off a band-7 value otherwise, and the
// kernels are bound by their 4 * deg^2 bytes per point either way.
#define SH_MAX_DEG 8
struct ShNorm {
  double k[SH_MAX_DEG * (SH_MAX_DEG + 1) / 2];  // [l (l + 1) / 2 + m]: sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!), x sqrt(2) for m > 0
};

static ShNorm sh_norm() {
  ShNorm n;
  for (int l = 0; l < SH_MAX_DEG; l++)
    for (int m = 0; m <= l; m++) {
      double r = 1.0;
      for (int i = l - m + 1; i <= l + m; i++) r /= (double)i;
      double k = std::sqrt((2.0 * l + 1.0) / (4.0 * M_PI) * r);
      if (m > 0) k *= std::sqrt(2.0);
      n.k[l * (l + 1) / 2 + m] = k;
    }
  return n;
}

// Pbar_l^m(z) for l < deg, and its z-derivative: Pbar_m^m = (-1)^m (2m-1)!!, Pbar_{m+1}^m = (2m+1) z Pbar_m^m,
// (l - m) Pbar_l^m = (2l - 1) z Pbar_{l-1}^m - (l + m - 1) Pbar_{l-2}^m.  A_m + i B_m = (x + i y)^m.
template <bool GRAD>
__device__ inline void sh_eval(double x, double y, double z, int deg, const ShNorm& nm, const float* gout, float* out,
                               float* gx, float* gy, float* gz) {
  double A[SH_MAX_DEG], Bm[SH_MAX_DEG];
  A[0] = 1.0;
  Bm[0] = 0.0;
  for (int m = 1; m < deg; m++) {
    A[m] = x * A[m - 1] - y * Bm[m - 1];
    Bm[m] = x * Bm[m - 1] + y * A[m - 1];
  }
  double sx = 0.0, sy = 0.0, sz = 0.0;
  double pmm = 1.0;  // Pbar_m^m
  for (int m = 0; m < deg; m++) {
    if (m > 0) pmm *= -(double)(2 * m - 1);
    double p2 = 0.0, d2 = 0.0, p1 = pmm, d1 = 0.0;  // Pbar_{l-2}, Pbar_{l-1} and their derivatives
    for (int l = m; l < deg; l++) {
      double p, dp;
      if (l == m) {
        p = pmm;
        dp = 0.0;
      } else {
        p = ((double)(2 * l - 1) * z * p1 - (double)(l + m - 1) * p2) / (double)(l - m);
        dp = ((double)(2 * l - 1) * (p1 + z * d1) - (double)(l + m - 1) * d2) / (double)(l - m);
        p2 = p1;
        d2 = d1;
      }
      p1 = p;
      d1 = dp;
      const double k = nm.k[l * (l + 1) / 2 + m];
      const int jp = l * l + l + m, jn = l * l + l - m;
      if (!GRAD) {
        out[jp] = (float)(k * p * A[m]);
        if (m > 0) out[jn] = (float)(k * p * Bm[m]);
      } else {
        const double dA_dx = m > 0 ? (double)m * A[m - 1] : 0.0, dA_dy = m > 0 ? -(double)m * Bm[m - 1] : 0.0;
        const double gp = (double)gout[jp];
        sx += gp * k * p * dA_dx;
        sy += gp * k * p * dA_dy;
        sz += gp * k * dp * A[m];
        if (m > 0) {
          const double dB_dx = (double)m * Bm[m - 1], dB_dy = (double)m * A[m - 1];
          const double gn = (double)gout[jn];
          sx += gn * k * p * dB_dx;
          sy += gn * k * p * dB_dy;
          sz += gn * k * dp * Bm[m];
        }
      }
    }
  }
  if (GRAD) {
    *gx = (float)sx;
    *gy = (float)sy;
    *gz = (float)sz;
  }
}

__global__ void __launch_bounds__(GS_BLOCK) sh_fwd_kernel(const float* __restrict__ inputs, uint32_t B, int deg, ShNorm nm,
                                                           float* __restrict__ out) {
  const size_t b = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (b >= B) return;
  sh_eval<false>(inputs[3 * b], inputs[3 * b + 1], inputs[3 * b + 2], deg, nm, nullptr, out + b * deg * deg, nullptr, nullptr,
                 nullptr);
}

__global__ void __launch_bounds__(GS_BLOCK) sh_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ inputs,
                                                           uint32_t B, int deg, ShNorm nm, float* __restrict__ grad_inputs) {
  const size_t b = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (b >= B) return;
  float gx, gy, gz;
  sh_eval<true>(inputs[3 * b], inputs[3 * b + 1], inputs[3 * b + 2], deg, nm, grad + b * deg * deg, nullptr, &gx, &gy, &gz);
  grad_inputs[3 * b] = gx;
  grad_inputs[3 * b + 1] = gy;
  grad_inputs[3 * b + 2] = gz;
}

static inline unsigned enc_blocks(size_t n) { return (unsigned)((n + GS_BLOCK - 1) / GS_BLOCK); }

static int grid_check(int64_t B, int32_t D, int64_t n_slots, int32_t C, int32_t L, int32_t gridtype, int32_t interp) {
  if (B < 0 || L < 1 || n_slots < 1) return GS_E_SHAPE;
  if (D < 2 || D > 5 || !(C == 1 || C == 2 || C == 4 || C == 8)) return GS_E_UNSUPPORTED;
  if (L > ENC_MAX_LEVELS || gridtype < 0 || gridtype > 1 || interp < 0 || interp > 1) return GS_E_UNSUPPORTED;
  // sort entries, entry ids and the slot sentinel are 32-bit
  if (((uint64_t)B * (uint64_t)L << D) >= 0xFFFFFFFFull || (uint64_t)n_slots >= 0xFFFFFFFFull) return GS_E_SHAPE;
  return GS_OK;
}

template <int D, int C>
static int grid_fwd_launch(const float* inputs, uint32_t B, const float* emb, const int32_t* offsets, uint32_t L,
                           const EncLevels& lv, int gridtype, bool ac, int interp, float* out, float* dy_dx, hipStream_t s) {
  hipLaunchKernelGGL((grid_fwd_kernel<D, C>), dim3(enc_blocks((size_t)B * L)), dim3(GS_BLOCK), 0, s, inputs, emb, offsets, B,
                     L, lv, (uint32_t)gridtype, ac, (uint32_t)interp, out, dy_dx);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

template <int D, int C>
static int grid_bwd_launch(const float* grad, const float* inputs, uint32_t B, uint32_t n_slots, const int32_t* offsets,
                           uint32_t L, const EncLevels& lv, int gridtype, bool ac, int interp, const float* dy_dx,
                           float* grad_emb, float* grad_inputs, void* tmp, hipStream_t s) {
  if (grad_emb) {
    const uint32_t N = (uint32_t)((size_t)B * L << D);
    EncTmp t = enc_view(tmp, N, C, n_slots);
    hipLaunchKernelGGL((grid_emit_kernel<D>), dim3(enc_blocks((size_t)B * L)), dim3(GS_BLOCK), 0, s, inputs, offsets, B, L,
                       lv, (uint32_t)gridtype, ac, n_slots, t.sort.keys[0], t.sort.vals[0], t.hdr);
    GS_LAUNCH_CHECK(s, 0);
    int end_bit = 1;
    while (end_bit < 32 && (n_slots >> end_bit) != 0) end_bit++;  // the sentinel n_slots sorts last
    const int passes = (end_bit + RS_BITS - 1) / RS_BITS;
    int rc = launch_radix_sort(t.sort, &t.hdr->n, N, end_bit, 0, nullptr, s, 0);
    if (rc) return rc;
    const uint32_t* keys = t.sort.keys[passes & 1];
    const uint32_t* vals = t.sort.vals[passes & 1];
    hipLaunchKernelGGL((grid_gather_kernel<D, C>), dim3(enc_blocks(N)), dim3(GS_BLOCK), 0, s, inputs, grad, N, L, lv, ac,
                       (uint32_t)interp, n_slots, keys, vals, t.contrib, t.chunk);
    GS_LAUNCH_CHECK(s, 0);
    hipError_t e = hipMemsetAsync(t.seg_lo, 0xFF, 4 * (size_t)n_slots, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(grid_mark_kernel, dim3(enc_blocks(N)), dim3(GS_BLOCK), 0, s, keys, N, n_slots, t.seg_lo, t.seg_hi);
    GS_LAUNCH_CHECK(s, 0);
    hipLaunchKernelGGL((grid_slot_kernel<C>), dim3(enc_blocks(n_slots)), dim3(GS_BLOCK), 0, s, t.seg_lo, t.seg_hi, t.contrib,
                       t.chunk, n_slots, grad_emb);
    GS_LAUNCH_CHECK(s, 0);
  }
  if (grad_inputs) {
    hipLaunchKernelGGL((grid_input_bwd_kernel<D, C>), dim3(enc_blocks((size_t)B * D)), dim3(GS_BLOCK), 0, s, grad, dy_dx, B, L,
                       grad_inputs);
    GS_LAUNCH_CHECK(s, 0);
  }
  return GS_OK;
}

#define ENC_DISPATCH(FN, ...)                             \
  switch (D * 16 + C) {                                   \
    case 2 * 16 + 1: return FN<2, 1>(__VA_ARGS__);        \
    case 2 * 16 + 2: return FN<2, 2>(__VA_ARGS__);        \
    case 2 * 16 + 4: return FN<2, 4>(__VA_ARGS__);        \
    case 2 * 16 + 8: return FN<2, 8>(__VA_ARGS__);        \
    case 3 * 16 + 1: return FN<3, 1>(__VA_ARGS__);        \
    case 3 * 16 + 2: return FN<3, 2>(__VA_ARGS__);        \
    case 3 * 16 + 4: return FN<3, 4>(__VA_ARGS__);        \
    case 3 * 16 + 8: return FN<3, 8>(__VA_ARGS__);        \
    case 4 * 16 + 1: return FN<4, 1>(__VA_ARGS__);        \
    case 4 * 16 + 2: return FN<4, 2>(__VA_ARGS__);        \
    case 4 * 16 + 4: return FN<4, 4>(__VA_ARGS__);        \
    case 4 * 16 + 8: return FN<4, 8>(__VA_ARGS__);        \
    case 5 * 16 + 1: return FN<5, 1>(__VA_ARGS__);        \
    case 5 * 16 + 2: return FN<5, 2>(__VA_ARGS__);        \
    case 5 * 16 + 4: return FN<5, 4>(__VA_ARGS__);        \
    case 5 * 16 + 8: return FN<5, 8>(__VA_ARGS__);        \
    default: return GS_E_UNSUPPORTED;                     \
  }

}  // namespace

extern "C" {

size_t gs_grid_encode_tmp_bytes(int64_t B, int32_t D, int32_t L, int32_t C, int64_t n_slots) {
  if (B < 0 || D < 2 || D > 5 || L < 1 || C < 1 || n_slots < 1) return 0;
  return enc_bytes((size_t)B * (size_t)L << D, (size_t)C, (size_t)n_slots);
}

int gs_grid_encode_fwd(const float* inputs, int64_t B, int32_t D, const float* embeddings, int64_t n_slots, int32_t C,
                       const int32_t* offsets, int32_t L, float S, int32_t H, int32_t gridtype, int32_t align_corners,
                       int32_t interp, float* outputs, float* dy_dx, void* stream) {
  int rc = grid_check(B, D, n_slots, C, L, gridtype, interp);
  if (rc) return rc;
  if (B == 0) return GS_OK;
  if (!inputs || !embeddings || !offsets || !outputs) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  const EncLevels lv = enc_levels(L, S, H);
  const bool ac = align_corners != 0;
  ENC_DISPATCH(grid_fwd_launch, inputs, (uint32_t)B, embeddings, offsets, (uint32_t)L, lv, gridtype, ac, interp, outputs,
               dy_dx, s);
}

int gs_grid_encode_bwd(const float* grad, const float* inputs, int64_t B, int32_t D, int64_t n_slots, int32_t C,
                       const int32_t* offsets, int32_t L, float S, int32_t H, int32_t gridtype, int32_t align_corners,
                       int32_t interp, const float* dy_dx, float* grad_embeddings, float* grad_inputs, void* tmp,
                       size_t tmp_bytes, void* stream) {
  int rc = grid_check(B, D, n_slots, C, L, gridtype, interp);
  if (rc) return rc;
  if (!grad_embeddings && !grad_inputs) return GS_OK;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    if (grad_embeddings) {
      hipError_t e = hipMemsetAsync(grad_embeddings, 0, 4 * (size_t)n_slots * C, s);
      if (e != hipSuccess) return (int)e;
    }
    return GS_OK;
  }
  if (!grad || !inputs || !offsets) return GS_E_NULL;
  if (grad_inputs && !dy_dx) return GS_E_NULL;
  if (grad_embeddings) {
    if (!tmp) return GS_E_NULL;
    if (tmp_bytes < gs_grid_encode_tmp_bytes(B, D, L, C, n_slots)) return GS_E_SCRATCH;
  }
  const EncLevels lv = enc_levels(L, S, H);
  const bool ac = align_corners != 0;
  ENC_DISPATCH(grid_bwd_launch, grad, inputs, (uint32_t)B, (uint32_t)n_slots, offsets, (uint32_t)L, lv, gridtype, ac, interp,
               dy_dx, grad_embeddings, grad_inputs, tmp, s);
}

int gs_sh_encode_fwd(const float* inputs, int64_t B, int32_t degree, float* outputs, void* stream) {
  if (B < 0 || B >= 0xFFFFFFFFll) return GS_E_SHAPE;
  if (degree < 1 || degree > SH_MAX_DEG) return GS_E_UNSUPPORTED;
  if (B == 0) return GS_OK;
  if (!inputs || !outputs) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sh_fwd_kernel, dim3(enc_blocks((size_t)B)), dim3(GS_BLOCK), 0, s, inputs, (uint32_t)B, (int)degree,
                     sh_norm(), outputs);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_sh_encode_bwd(const float* grad, const float* inputs, int64_t B, int32_t degree, float* grad_inputs, void* stream) {
  if (B < 0 || B >= 0xFFFFFFFFll) return GS_E_SHAPE;
  if (degree < 1 || degree > SH_MAX_DEG) return GS_E_UNSUPPORTED;
  if (B == 0) return GS_OK;
  if (!grad || !inputs || !grad_inputs) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sh_bwd_kernel, dim3(enc_blocks((size_t)B)), dim3(GS_BLOCK), 0, s, grad, inputs, (uint32_t)B, (int)degree,
                     sh_norm(), grad_inputs);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}
}
