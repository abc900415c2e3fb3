// gs_depth_vis.hip - the turbo-coloured depth map of the render stage, on the device (gfx950, wave64):
//   DNGaussian/render.py:121,127-130 and spiral.py:114-121   visualize_cmap(depth, ones, turbo, curve_fn = -log(x + eps))
//   FSGS/utils/general_utils.py:157-176                      vis_depth(depth), curve 1 / x + 1e-10
// The reference pulls the image to the host and argsorts every pixel for weighted_percentile(x, ones, [0.5, 99.5]).  With unit
// weights those are two order statistics each read at (at most) two neighbouring ranks, so the sort becomes a radix SELECT:
//
//   minmax_kernel     (alpha given) per-workgroup minimum / maximum of depth, NaN-propagating as torch.min / torch.max
//   composite_kernel  (alpha given) d = (depth - min) / (max - min) + 1 * (1 - alpha), each operation rounded on its own
//                     (render.py:121); optionally the grey bytes save_image writes for 1 - d
//   hist_kernel x 4   float32 -> monotone 32-bit key (NaN last, as np.argsort places it; -0 = +0), 8 bits per pass from the top.
//                     A pixel counts in pass p only if its higher bits equal one of the (at most four) prefixes the wanted ranks
//                     still live in: integer counts in LDS [4][256], integer adds into the pass's global table
//   narrow_kernel x 4 one workgroup: scans the table, moves each wanted rank into its digit's bucket, renumbers the prefixes.
//                     After the last pass a prefix IS the key of the rank's value; thread 0 then forms lo and hi in double with
//                     np.interp's statements and leaves min(lo', hi') and |hi' - lo'| of the curved bounds for the last stage
//   colour_kernel     curve, normalise in double, nan_to_num(clip(., 0, 1)), matplotlib's index trunc(v * 256) with 256 -> 255,
//                     the three bytes of the caller's table row, interleaved [H,W,3]
//
// Four passes of 8 bits, not three of 11 / 11 / 10: four slots of 256 counters are 4 KB of LDS and at most 1 024 integer adds
// per workgroup to flush, where 4 x 2 048 would be 32 KB and 8 192; the image (8 MB at 1920 x 1080) stays in L2 / MALL between
// the passes, so a fourth read costs less than the wider flush.  Depth images put most pixels into one or two digits of the
// leading passes (sign and exponent), so before the LDS add a wave peels its two most common bins with a ballot and adds their
// population counts once; what is left takes one ds_add each.  Counts are integers: no order, the same bits on every run.
// Everything runs on the caller's stream; nothing synchronises with the host, and no float is added atomically.
#include "gs_common.h"
#include "gs_eval_px.h"

namespace {

constexpr int DV_SLOTS = 4;        // wanted ranks: (j, j + 1) of the low query and of the high one
constexpr int DV_RADIX = 256;
constexpr int DV_PASSES = 4;
constexpr int DV_ITEMS = 16;       // dwords a lane reads in the select passes, GS_BLOCK apart: one dword per lane per load
constexpr int DV_TILE = GS_BLOCK * DV_ITEMS;
constexpr int DV_MM_BLOCKS = 256;  // minmax partials: one per thread of the composite kernel's re-reduction
constexpr int64_t DV_MAX_N = (int64_t)1 << 24;  // np.cumsum of float32 ones counts exactly up to 2^24
static_assert(GS_BLOCK == 256 && DV_RADIX == GS_BLOCK, "one thread per digit in narrow_kernel");

struct DvCtl {                 // 256 bytes at the head of tmp
  uint32_t prefix[DV_SLOTS];   // per slot: the key bits above the current pass's digit
  uint32_t rank[DV_SLOTS];     // per wanted rank: its position among the pixels of its slot
  uint32_t slot_of[DV_SLOTS];  // per wanted rank: its slot
  uint32_t nslot;
  uint32_t pad0[3];
  double lo, hi;               // lo_auto - eps, hi_auto + eps
  double vmin, vden;           // min(curve(lo), curve(hi)), |curve(hi) - curve(lo)|
  uint32_t pad1[40];
};
static_assert(sizeof(DvCtl) == 256, "control block is one 256-B block");

struct DvQuery {    // formed on the host from n alone (np.interp's branch and node for both queries)
  uint32_t rank[DV_SLOTS];  // 0-based sorted positions: (j, j + 1) per query, j + 1 repeated as j where it is not read
  double q[2];              // p * float32(n / 100) in double
  int interp[2];            // 1: slope * (q - xp[j]) + fp[j];  0: fp[j] itself (below the first node, on a node, last node)
  double eps;
};

struct DvView {
  DvCtl* ctl;
  uint32_t* hist;    // [DV_PASSES][DV_SLOTS][DV_RADIX], zeroed at the start of every call
  float* mm;         // [DV_MM_BLOCKS][2] + flags [DV_MM_BLOCKS]
  uint32_t* mm_nan;
  float* d;          // [n] the composite image
};
inline size_t dv_hist_bytes() { return gs_align(sizeof(uint32_t) * DV_PASSES * DV_SLOTS * DV_RADIX); }
inline size_t dv_bytes(int64_t n) {
  return sizeof(DvCtl) + dv_hist_bytes() + gs_align(8 * DV_MM_BLOCKS) + gs_align(4 * DV_MM_BLOCKS) + gs_align(4 * (size_t)n);
}
inline DvView dv_view(void* tmp) {
  char* p = (char*)tmp;
  DvView v;
  v.ctl = (DvCtl*)p; p += sizeof(DvCtl);
  v.hist = (uint32_t*)p; p += dv_hist_bytes();
  v.mm = (float*)p; p += gs_align(8 * DV_MM_BLOCKS);
  v.mm_nan = (uint32_t*)p; p += gs_align(4 * DV_MM_BLOCKS);
  v.d = (float*)p;
  return v;
}

__device__ __forceinline__ uint32_t dv_key(float x) {
  if (x != x) return 0xFFFFFFFFu;         // every NaN after +inf (0xFF800000)
  if (x == 0.0f) return 0x80000000u;      // -0 and +0 compare equal in a sort
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dv_value(uint32_t key) {
  if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// ---------------------------------------------------------------------------------------------- composite
__global__ void __launch_bounds__(GS_BLOCK) minmax_kernel(const float* __restrict__ depth, int n, float* __restrict__ mm,
                                                          uint32_t* __restrict__ mm_nan) {
  __shared__ float smin[GS_BLOCK / 64], smax[GS_BLOCK / 64];
  __shared__ uint32_t snan[GS_BLOCK / 64];
  float lo = INFINITY, hi = -INFINITY;
  uint32_t bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_BLOCK) {
    const float x = depth[i];
    if (x != x) bad = 1;
    else { lo = fminf(lo, x); hi = fmaxf(hi, x); }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = fminf(lo, __shfl_down(lo, off, 64));
    hi = fmaxf(hi, __shfl_down(hi, off, 64));
    bad |= __shfl_down(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; snan[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mm[2 * blockIdx.x] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    mm[2 * blockIdx.x + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    mm_nan[blockIdx.x] = snan[0] | snan[1] | snan[2] | snan[3];
  }
}

__global__ void __launch_bounds__(GS_BLOCK) composite_kernel(const float* __restrict__ depth, const float* __restrict__ alpha,
                                                             int n, const float* __restrict__ mm,
                                                             const uint32_t* __restrict__ mm_nan, int mm_blocks,
                                                             float* __restrict__ d_out, float* __restrict__ d_copy,
                                                             uint8_t* __restrict__ grey) {
  __shared__ float smin[GS_BLOCK / 64], smax[GS_BLOCK / 64];
  __shared__ uint32_t snan[GS_BLOCK / 64];
  float lo = INFINITY, hi = -INFINITY;
  uint32_t bad = 0;
  if ((int)threadIdx.x < mm_blocks) { lo = mm[2 * threadIdx.x]; hi = mm[2 * threadIdx.x + 1]; bad = mm_nan[threadIdx.x]; }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    bad |= __shfl_xor(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; snan[threadIdx.x >> 6] = bad; }
  __syncthreads();
  lo = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
  hi = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  if (snan[0] | snan[1] | snan[2] | snan[3]) lo = hi = __uint_as_float(0x7FC00000u);  // torch.min / max return NaN
  const int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float range = __fsub_rn(hi, lo);
  const float d = __fadd_rn(__fdiv_rn(__fsub_rn(depth[i], lo), range), __fmul_rn(1.0f, __fsub_rn(1.0f, alpha[i])));
  d_out[i] = d;
  if (d_copy) d_copy[i] = d;
  if (grey) {
    const uint8_t q = ev_byte(__fsub_rn(1.0f, d));
    grey[3 * i] = q; grey[3 * i + 1] = q; grey[3 * i + 2] = q;
  }
}

// ---------------------------------------------------------------------------------------------- select
__global__ void __launch_bounds__(GS_BLOCK) dv_init_kernel(DvCtl* __restrict__ ctl, uint32_t* __restrict__ hist, DvQuery qy) {
  for (int i = threadIdx.x; i < DV_PASSES * DV_SLOTS * DV_RADIX; i += GS_BLOCK) hist[i] = 0u;
  if (threadIdx.x < DV_SLOTS) {
    ctl->prefix[threadIdx.x] = 0u;
    ctl->rank[threadIdx.x] = qy.rank[threadIdx.x];
    ctl->slot_of[threadIdx.x] = 0u;
  }
  if (threadIdx.x == 0) ctl->nslot = 1u;
}

__global__ void __launch_bounds__(GS_BLOCK) hist_kernel(const float* __restrict__ x, int n, int pass,
                                                        const DvCtl* __restrict__ ctl, uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[DV_SLOTS * DV_RADIX];
  const int nslot = min((int)ctl->nslot, DV_SLOTS);  // 1..4
  uint32_t pre[DV_SLOTS];
#pragma unroll
  for (int s = 0; s < DV_SLOTS; s++) pre[s] = ctl->prefix[s];
  for (int i = threadIdx.x; i < DV_SLOTS * DV_RADIX; i += GS_BLOCK) lh[i] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const int lane = threadIdx.x & 63;
  const int64_t base = (int64_t)blockIdx.x * DV_TILE + threadIdx.x;
#pragma unroll 4
  for (int it = 0; it < DV_ITEMS; it++) {
    const int64_t i = base + (int64_t)it * GS_BLOCK;
    int bin = -1;
    if (i < n) {
      const uint32_t key = dv_key(x[i]);
      const uint32_t high = pass == 0 ? 0u : (key >> (shift + 8));  // (pass 0: one slot, prefix 0)
#pragma unroll
      for (int s = 0; s < DV_SLOTS; s++)
        if (s < nslot && high == pre[s]) bin = s * DV_RADIX + (int)((key >> shift) & 255u);  // (prefixes are distinct)
    }
    // peel the wave's two most common bins: one LDS add of a population count each
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const unsigned long long active = __ballot(bin >= 0);
      if (active == 0ull) break;
      const int leader = __ffsll((long long)active) - 1;
      const int lb = __shfl(bin, leader, 64);
      const unsigned long long same = __ballot(bin == lb);
      if (lane == leader) atomicAdd(&lh[lb], (uint32_t)__popcll(same));
      if (bin == lb) bin = -1;
    }
    if (bin >= 0) atomicAdd(&lh[bin], 1u);
  }
  __syncthreads();
  uint32_t* g = hist + (size_t)pass * DV_SLOTS * DV_RADIX;
  for (int i = threadIdx.x; i < nslot * DV_RADIX; i += GS_BLOCK) {
    const uint32_t c = lh[i];
    if (c) atomicAdd(&g[i], c);
  }
}

__device__ __forceinline__ double dv_curve(double x, int rule) {
  if (rule == GS_DEPTH_VIS_DNG) return -log(x + (double)1.1920928955078125e-07f);  // float32's eps, in double as numpy promotes it
  if (rule == GS_DEPTH_VIS_FSGS) return 1.0 / x + 1e-10;
  return x;
}

// np.interp at one query: fp[j], fp[j + 1] are the values at the two wanted ranks, xp[j] = j + 1, xp[j + 1] - xp[j] = 1
__device__ double dv_interp(float fj, float fj1, uint32_t j, double q, int interp) {
  const double a = (double)fj, b = (double)fj1;
  if (!interp) return a;
  const double xj = (double)j + 1.0, xj1 = (double)j + 2.0;
  const double slope = (b - a) / (xj1 - xj);
  double r = slope * (q - xj) + a;
  if (r != r) {               // "If we get nan in one direction, try the other"
    r = slope * (q - xj1) + b;
    if (r != r && a == b) r = a;
  }
  return r;
}

__global__ void __launch_bounds__(GS_BLOCK) narrow_kernel(DvCtl* __restrict__ ctl, const uint32_t* __restrict__ hist, int pass,
                                                          DvQuery qy, int rule, double* __restrict__ out_bounds) {
  __shared__ uint32_t excl[DV_SLOTS][DV_RADIX + 1];
  __shared__ uint32_t wsum[GS_BLOCK / 64];
  __shared__ uint32_t new_prefix[DV_SLOTS], new_rank[DV_SLOTS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nslot = min((int)ctl->nslot, DV_SLOTS);
  const uint32_t* g = hist + (size_t)pass * DV_SLOTS * DV_RADIX;
  for (int s = 0; s < nslot; s++) {
    const uint32_t c = g[s * DV_RADIX + t];
    uint32_t inc = c;  // inclusive scan over the wave, then over the four waves
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += wsum[w];
    excl[s][t] = before + inc - c;
    if (t == DV_RADIX - 1) excl[s][DV_RADIX] = before + inc;
    __syncthreads();
  }
  // each wanted rank: the digit d of its slot with excl[d] <= rank < excl[d + 1]
#pragma unroll
  for (int k = 0; k < DV_SLOTS; k++) {
    const int s = min((int)ctl->slot_of[k], DV_SLOTS - 1);
    const uint32_t r = ctl->rank[k];
    if (r >= excl[s][t] && r < excl[s][t + 1]) {  // true for exactly one t (a rank below the slot's count)
      new_prefix[k] = (ctl->prefix[s] << 8) | (uint32_t)t;
      new_rank[k] = r - excl[s][t];
    }
  }
  __syncthreads();
  if (t != 0) return;
  // ranks ascend, so their prefixes do not descend: equal neighbours share a slot
  uint32_t ns = 0;
  for (int k = 0; k < DV_SLOTS; k++) {
    if (k == 0 || new_prefix[k] != new_prefix[k - 1]) ctl->prefix[ns++] = new_prefix[k];
    ctl->slot_of[k] = ns - 1;
    ctl->rank[k] = new_rank[k];
  }
  ctl->nslot = ns;
  if (pass != DV_PASSES - 1) return;
  const double lo_auto = dv_interp(dv_value(new_prefix[0]), dv_value(new_prefix[1]), qy.rank[0], qy.q[0], qy.interp[0]);
  const double hi_auto = dv_interp(dv_value(new_prefix[2]), dv_value(new_prefix[3]), qy.rank[2], qy.q[1], qy.interp[1]);
  const double lo = lo_auto - qy.eps, hi = hi_auto + qy.eps;
  const double clo = dv_curve(lo, rule), chi = dv_curve(hi, rule);
  ctl->lo = lo;
  ctl->hi = hi;
  ctl->vmin = (clo != clo || chi != chi) ? (clo + chi) : (clo < chi ? clo : chi);  // np.minimum propagates NaN
  ctl->vden = fabs(chi - clo);
  if (out_bounds) { out_bounds[0] = lo; out_bounds[1] = hi; }
}

// ---------------------------------------------------------------------------------------------- colourise
__device__ __forceinline__ int dv_index(float x, int rule, double vmin, double vden) {
  float v;
  if (rule == GS_DEPTH_VIS_DNG) v = (float)(-log((double)__fadd_rn(x, 1.1920928955078125e-07f)));  // double, rounded once
  else if (rule == GS_DEPTH_VIS_FSGS) v = __fadd_rn(__fdiv_rn(1.0f, x), 1e-10f);
  else v = x;
  double tn = ((double)v - vmin) / vden;
  if (tn != tn) tn = 0.0;                        // nan_to_num (clip leaves NaN alone)
  else tn = tn < 0.0 ? 0.0 : (tn > 1.0 ? 1.0 : tn);
  const int idx = (int)(tn * 256.0);             // matplotlib: xa *= N; xa[xa == N] = N - 1; astype(int)
  return idx > 255 ? 255 : idx;
}

__global__ void __launch_bounds__(GS_BLOCK) colour_kernel(const float* __restrict__ x, int n, int rule,
                                                          const DvCtl* __restrict__ ctl, const uint8_t* __restrict__ lut,
                                                          uint8_t* __restrict__ out, int vec) {
  __shared__ uint8_t tab[DV_RADIX * 3];
  for (int i = threadIdx.x; i < DV_RADIX * 3; i += GS_BLOCK) tab[i] = lut[i];
  __syncthreads();
  const double vmin = ctl->vmin, vden = ctl->vden;
  const int64_t p0 = ((int64_t)blockIdx.x * GS_BLOCK + threadIdx.x) * 4;
  if (p0 >= n) return;
  if (vec && p0 + 4 <= n) {  // four pixels: one 16-byte load, twelve bytes as three dwords (x and out are then aligned)
    const float4 f = *reinterpret_cast<const float4*>(x + p0);
    const float in[4] = {f.x, f.y, f.z, f.w};
    uint32_t b[12];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int idx = dv_index(in[e], rule, vmin, vden);
#pragma unroll
      for (int c = 0; c < 3; c++) b[3 * e + c] = tab[3 * idx + c];
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(out + 3 * p0);
#pragma unroll
    for (int w = 0; w < 3; w++) o[w] = b[4 * w] | (b[4 * w + 1] << 8) | (b[4 * w + 2] << 16) | (b[4 * w + 3] << 24);
  } else {
    for (int e = 0; e < 4 && p0 + e < n; e++) {
      const int idx = dv_index(x[p0 + e], rule, vmin, vden);
#pragma unroll
      for (int c = 0; c < 3; c++) out[3 * (p0 + e) + c] = tab[3 * idx + c];
    }
  }
}

// the host's share of weighted_percentile(x, ones, [0.5, 99.5]): it depends on n alone
DvQuery dv_query(int64_t n, int rule) {
  DvQuery qy;
  const float step = (float)n / 100.0f;  // acc_w[-1] / 100, a float32 scalar
  const double ps[2] = {50.0 - 99.0 / 2, 50.0 + 99.0 / 2};
  for (int k = 0; k < 2; k++) {
    const double q = ps[k] * (double)step;
    qy.q[k] = q;
    int64_t j;
    int interp = 0;
    if (q < 1.0) j = 0;                     // left of xp[0] = 1 (and the single-node case n == 1)
    else if (q > (double)n) j = n - 1;      // right of xp[-1]
    else {
      j = (int64_t)q - 1;                   // xp[j] = j + 1 <= q < j + 2
      if (j >= n - 1) j = n - 1;
      else if ((double)(j + 1) != q) interp = 1;
    }
    qy.rank[2 * k] = (uint32_t)j;
    qy.rank[2 * k + 1] = (uint32_t)(interp ? j + 1 : j);
    qy.interp[k] = interp;
  }
  qy.eps = rule == GS_DEPTH_VIS_FSGS ? 1e-10 : (double)1.1920928955078125e-07f;
  return qy;
}

inline bool dv_shape_ok(int32_t H, int32_t W) { return H >= 0 && W >= 0 && (int64_t)H * W <= DV_MAX_N; }

}  // namespace

extern "C" {

size_t gs_depth_vis_tmp_bytes(int32_t H, int32_t W) {
  if (!dv_shape_ok(H, W) || (int64_t)H * W == 0) return 0;
  return dv_bytes((int64_t)H * W);
}

int gs_depth_vis(const float* depth, const float* alpha, int32_t H, int32_t W, int32_t rule, const uint8_t* lut_rgb_u8, void* tmp,
                 size_t tmp_bytes, uint8_t* out_rgb_u8, uint8_t* out_grey_u8, float* out_composite, double* out_bounds, void* stream) {
  if (!dv_shape_ok(H, W)) return GS_E_SHAPE;
  if (rule != GS_DEPTH_VIS_IDENTITY && rule != GS_DEPTH_VIS_DNG && rule != GS_DEPTH_VIS_FSGS) return GS_E_SHAPE;
  const int64_t n64 = (int64_t)H * W;
  if (n64 == 0) return GS_OK;  // nothing to colour, nothing written (numpy has no percentile of an empty image)
  if (!depth || !lut_rgb_u8 || !tmp || !out_rgb_u8) return GS_E_NULL;
  if ((out_grey_u8 || out_composite) && !alpha) return GS_E_NULL;  // both are the composite's
  if (tmp_bytes < dv_bytes(n64)) return GS_E_SHAPE;
  if (((uintptr_t)tmp & 255) || ((uintptr_t)depth & 3) || (alpha && ((uintptr_t)alpha & 3)) || ((uintptr_t)out_composite & 3) ||
      (out_bounds && ((uintptr_t)out_bounds & 7)))
    return GS_E_SHAPE;
  const int n = (int)n64;
  hipStream_t s = (hipStream_t)stream;
  const DvView v = dv_view(tmp);
  const DvQuery qy = dv_query(n64, rule);
  const unsigned px_blocks = (unsigned)((n64 + GS_BLOCK - 1) / GS_BLOCK);
  const float* x = depth;
  if (alpha) {
    const int mmb = (int)(px_blocks < (unsigned)DV_MM_BLOCKS ? px_blocks : (unsigned)DV_MM_BLOCKS);
    hipLaunchKernelGGL(minmax_kernel, dim3(mmb), dim3(GS_BLOCK), 0, s, depth, n, v.mm, v.mm_nan);
    GS_LAUNCH_CHECK(s, 0);
    hipLaunchKernelGGL(composite_kernel, dim3(px_blocks), dim3(GS_BLOCK), 0, s, depth, alpha, n, (const float*)v.mm,
                       (const uint32_t*)v.mm_nan, mmb, v.d, out_composite, out_grey_u8);
    GS_LAUNCH_CHECK(s, 0);
    x = v.d;
  }
  hipLaunchKernelGGL(dv_init_kernel, dim3(1), dim3(GS_BLOCK), 0, s, v.ctl, v.hist, qy);
  GS_LAUNCH_CHECK(s, 0);
  const unsigned tiles = (unsigned)((n64 + DV_TILE - 1) / DV_TILE);
  for (int pass = 0; pass < DV_PASSES; pass++) {
    hipLaunchKernelGGL(hist_kernel, dim3(tiles), dim3(GS_BLOCK), 0, s, x, n, pass, (const DvCtl*)v.ctl, v.hist);
    GS_LAUNCH_CHECK(s, 0);
    hipLaunchKernelGGL(narrow_kernel, dim3(1), dim3(GS_BLOCK), 0, s, v.ctl, (const uint32_t*)v.hist, pass, qy, rule, out_bounds);
    GS_LAUNCH_CHECK(s, 0);
  }
  const int vec = (((uintptr_t)x & 15) == 0 && ((uintptr_t)out_rgb_u8 & 3) == 0) ? 1 : 0;
  const unsigned cblocks = (unsigned)(((n64 + 3) / 4 + GS_BLOCK - 1) / GS_BLOCK);
  hipLaunchKernelGGL(colour_kernel, dim3(cblocks), dim3(GS_BLOCK), 0, s, x, n, rule, (const DvCtl*)v.ctl, lut_rgb_u8, out_rgb_u8, vec);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
