// gs_dng_dtu.hip - what DNGaussian's DTU loop (train_dtu.py) adds to the LLFF one, gfx950, wave64:
//   the object mask of a ground-truth image (:84-94),
//   the masked-mean fill in front of both depth legs (:103-105, :136-138),
//   the alpha penalty behind the mask (:155-159),
//   the colour-gated edits of the densification statistic and the raw opacity (:218-230).
// In the reference each is boolean-index arithmetic, a nonzero and a host stall per statement; here every count stays in
// device memory.  No atomics, no read-back, no host synchronisation: two runs give the same bits.
//
// mask (gt [3,H,W], thr, run): dark = every channel < thr (= max over the channels < thr; a NaN channel is not dark, as in
//   torch).  mask[y,x] = dark[y,x] and dark[y-1,x] and ... and dark[y-min(run-1,y),x]: the run of dark pixels that ends at (y,x)
//   going up the column is at least min(y + 1, run) long.  ONE launch of ONE workgroup of DT_MASK_THREADS lanes: lane t walks
//   the columns t, t + DT_MASK_THREADS, ... down the rows with a run counter (neighbouring lanes read neighbouring addresses),
//   writes the mask byte and the three output channels (0 where masked, else the input's bits), and the workgroup's LDS tree
//   leaves the masked count.  One workgroup because the count needs every column and may use neither an atomic nor a second
//   launch; the images are a few hundred columns wide and the mask is formed once per camera.  A lane reads a pixel before it
//   writes the same pixel and nobody else touches it: the output may alias the input.
// masked sums (fill and penalty share them): ms_stats_kernel, a grid of at most DT_MAX_BLOCKS workgroups.  Which elements a lane
//   takes is a function of n and the grid alone (block b sweeps the chunks b, b + G, ... of DT_BLOCK_ELEMS elements, lane t the
//   four consecutive elements at 4 t of a chunk); each lane adds in float64, the workgroup's sums go through one fixed LDS tree
//   into its partial (sum, count).
//   fill:    partial = sum of x over mask == 0.  mf_fill_kernel: every workgroup adds the partials IN INDEX ORDER (one lane, from
//            LDS), mean = (float)(sum / count) - rounded to fp32 once, 0 / 0 = NaN - and writes x's bits where unmasked, the mean
//            where masked.  Backward: g where unmasked, +0.0 where masked; nothing flows through the mean.
//   penalty: partial = sum of (double)a * (double)a over mask != 0.  ap_finish_kernel: one workgroup, the partials in index
//            order, loss = (float)(sum / count) (count 0: NaN) and the count for the backward.  Backward:
//            (g / float(count)) * (2 * a) in fp32 where masked, +0.0 elsewhere; count 0: +0.0 everywhere.
// colour rule (colour [P,3], statistic [P], raw opacity [P]), ONE launch: a rule fires on a row when max_c < thr (black) or
//   min_c > thr (white), strictly, against the fp32 threshold; the statistic is divided by the rule's fp32 divisor and, when the
//   rule resets, the raw opacity becomes `value`.  Black before white.  The colours are not written, so the LAST workgroup of the
//   grid edits nothing and counts the rows of both rules over all P instead (integer LDS tree) - counts[2] = black, white.
#include "gs_common.h"
#include "gs_launch.h"
#include "gs_reduce.h"

namespace {

#define DT_MASK_THREADS 1024
#define DT_ELEMS 4  // elements per lane and chunk
#define DT_BLOCK_ELEMS (DT_ELEMS * GS_BLOCK)
#define DT_MAX_BLOCKS 256
#define DT_MAX_N ((int64_t)1 << 31)  // elements of an image (the counts are int32)

struct MsPartial {
  double s;
  unsigned long long n;
};

struct MsRecord {  // the head of tmp: what a backward reads
  long long count;
  long long pad[3];
};

__global__ __launch_bounds__(DT_MASK_THREADS) void dtu_mask_kernel(const float* gt, int H, int W, float thr, int run, uint8_t* mask,
                                                                   int32_t* count, float* gt_out) {
  __shared__ int sh[DT_MASK_THREADS];
  const int t = threadIdx.x;
  const size_t plane = (size_t)H * (size_t)W;
  int masked = 0;
  for (int x = t; x < W; x += DT_MASK_THREADS) {
    int c = 0;  // length of the dark run that ends at the current row, capped at `run`
    for (int y = 0; y < H; y++) {
      const size_t i = (size_t)y * (size_t)W + (size_t)x;
      const float r = gt[i], g = gt[plane + i], b = gt[2 * plane + i];
      const bool dark = r < thr && g < thr && b < thr;
      c = dark ? (c < run ? c + 1 : run) : 0;
      const int need = y + 1 < run ? y + 1 : run;
      const bool m = c >= need;
      mask[i] = m ? (uint8_t)1 : (uint8_t)0;
      gt_out[i] = m ? 0.f : r;
      gt_out[plane + i] = m ? 0.f : g;
      gt_out[2 * plane + i] = m ? 0.f : b;
      masked += m ? 1 : 0;
    }
  }
  sh[t] = masked;
  gs_block_tree<DT_MASK_THREADS, 1>(sh, t);
  if (t == 0) count[0] = sh[0];
}

// mode 0: x over mask == 0;  mode 1: x^2 (in float64) over mask != 0
__global__ __launch_bounds__(GS_BLOCK) void ms_stats_kernel(const float* x, const uint8_t* mask, size_t n, int mode, int nblocks,
                                                            MsPartial* part) {
  __shared__ double sh[GS_BLOCK];
  __shared__ unsigned long long shn[GS_BLOCK];
  const int t = threadIdx.x;
  double v = 0.0;
  unsigned long long cnt = 0ull;
  for (size_t base = (size_t)blockIdx.x * DT_BLOCK_ELEMS; base < n; base += (size_t)nblocks * DT_BLOCK_ELEMS) {
    const size_t i = base + DT_ELEMS * (size_t)t;
    for (int k = 0; k < DT_ELEMS; k++) {
      if (i + k >= n) break;
      const bool m = mask[i + k] != 0;
      const double d = (double)x[i + k];
      if (mode == 0) {
        if (!m) { v += d; cnt++; }
      } else {
        if (m) { v += d * d; cnt++; }
      }
    }
  }
  sh[t] = v;
  shn[t] = cnt;
  gs_block_tree<GS_BLOCK, 1, 1>(sh, t, shn);
  if (t == 0) {
    MsPartial p;
    p.s = sh[0]; p.n = shn[0];
    part[blockIdx.x] = p;
  }
}

// the partials in index order, by lane 0, from LDS -> (sum, count) in sh_s[0], sh_n[0] for every lane of the workgroup.  EVERY
// workgroup of mf_fill_kernel forms the mean this way and all must get the same bits; the serial index order is what the fill's
// parity records hold, so it is NOT gs_reduce.h's tree and stays here on purpose.
__device__ __forceinline__ void ms_total(const MsPartial* part, int nblocks, double* sh_s, unsigned long long* sh_n, int t) {
  for (int i = t; i < nblocks; i += GS_BLOCK) {
    sh_s[i] = part[i].s;
    sh_n[i] = part[i].n;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    unsigned long long c = 0ull;
    for (int i = 0; i < nblocks; i++) { s += sh_s[i]; c += sh_n[i]; }
    sh_s[0] = s; sh_n[0] = c;
  }
  __syncthreads();
}
static_assert(DT_MAX_BLOCKS <= GS_BLOCK, "the partials of a forward fit one workgroup's LDS arrays");

__global__ __launch_bounds__(GS_BLOCK) void mf_fill_kernel(const float* x, const uint8_t* mask, size_t n, int nblocks,
                                                           const MsPartial* part, float* out, float* mean_out) {
  __shared__ double sh_s[GS_BLOCK];
  __shared__ unsigned long long sh_n[GS_BLOCK];
  const int t = threadIdx.x;
  ms_total(part, nblocks, sh_s, sh_n, t);
  const float mean = (float)(sh_s[0] / (double)sh_n[0]);  // no unmasked pixel: 0 / 0 = NaN
  if (mean_out && blockIdx.x == 0 && t == 0) mean_out[0] = mean;
  const size_t i = DT_ELEMS * ((size_t)blockIdx.x * GS_BLOCK + t);
  for (int k = 0; k < DT_ELEMS; k++)
    if (i + k < n) out[i + k] = mask[i + k] ? mean : x[i + k];
}

__global__ __launch_bounds__(GS_BLOCK) void mf_bwd_kernel(const float* g, const uint8_t* mask, size_t n, float* gx) {
  const size_t i = DT_ELEMS * ((size_t)blockIdx.x * GS_BLOCK + threadIdx.x);
  for (int k = 0; k < DT_ELEMS; k++)
    if (i + k < n) gx[i + k] = mask[i + k] ? 0.f : g[i + k];
}

__global__ __launch_bounds__(GS_BLOCK) void ap_finish_kernel(int nblocks, const MsPartial* part, MsRecord* rec, float* out) {
  __shared__ double sh_s[GS_BLOCK];
  __shared__ unsigned long long sh_n[GS_BLOCK];
  const int t = threadIdx.x;
  ms_total(part, nblocks, sh_s, sh_n, t);
  if (t != 0) return;
  rec->count = (long long)sh_n[0];
  out[0] = (float)(sh_s[0] / (double)sh_n[0]);  // an empty mask: 0 / 0 = NaN
}

__global__ __launch_bounds__(GS_BLOCK) void ap_bwd_kernel(const float* alpha, const uint8_t* mask, size_t n, const MsRecord* rec,
                                                          const float* g, float* ga) {
  const size_t i = DT_ELEMS * ((size_t)blockIdx.x * GS_BLOCK + threadIdx.x);
  if (i >= n) return;
  const long long count = rec->count;
  const float c = count > 0 ? g[0] / (float)count : 0.f;
  for (int k = 0; k < DT_ELEMS; k++) {
    if (i + k >= n) break;
    const float two_a = 2.f * alpha[i + k];
    ga[i + k] = (count > 0 && mask[i + k]) ? c * two_a : 0.f;
  }
}

struct CrRule {
  int on, reset;
  float thr, div;
};

__device__ __forceinline__ void cr_fires(const float* c, const CrRule& black, const CrRule& white, bool& fb, bool& fw) {
  // torch's max / min over the channels hand a NaN on; a NaN passes neither comparison
  const bool nan = c[0] != c[0] || c[1] != c[1] || c[2] != c[2];
  float mx = c[0], mn = c[0];
  for (int k = 1; k < 3; k++) {
    mx = c[k] > mx ? c[k] : mx;
    mn = c[k] < mn ? c[k] : mn;
  }
  fb = black.on && !nan && mx < black.thr;
  fw = white.on && !nan && mn > white.thr;
}

__global__ __launch_bounds__(GS_BLOCK) void cr_kernel(const float* colour, float* stat, float* opacity, size_t P, CrRule black,
                                                      CrRule white, float value, int32_t* counts) {
  const int t = threadIdx.x;
  if (blockIdx.x + 1 == gridDim.x) {  // the counting workgroup: every row's colour, nothing written but the counts
    __shared__ int sh[2 * GS_BLOCK];
    int nb = 0, nw = 0;
    for (size_t i = t; i < P; i += GS_BLOCK) {
      const float c[3] = {colour[3 * i], colour[3 * i + 1], colour[3 * i + 2]};
      bool fb, fw;
      cr_fires(c, black, white, fb, fw);
      nb += fb ? 1 : 0;
      nw += fw ? 1 : 0;
    }
    sh[t] = nb; sh[GS_BLOCK + t] = nw;
    gs_block_tree<GS_BLOCK, 2>(sh, t);
    if (t == 0) { counts[0] = sh[0]; counts[1] = sh[GS_BLOCK]; }
    return;
  }
  const size_t i = (size_t)blockIdx.x * GS_BLOCK + t;
  if (i >= P) return;
  const float c[3] = {colour[3 * i], colour[3 * i + 1], colour[3 * i + 2]};
  bool fb, fw;
  cr_fires(c, black, white, fb, fw);
  if (!fb && !fw) return;
  float s = stat[i];
  if (fb) s = s / black.div;
  if (fw) s = s / white.div;
  stat[i] = s;
  if ((fb && black.reset) || (fw && white.reset)) opacity[i] = value;
}

static bool dt_n_ok(int64_t n) { return n >= 1 && n < DT_MAX_N; }

static unsigned dt_grid(size_t n) { return (unsigned)((n + DT_BLOCK_ELEMS - 1) / DT_BLOCK_ELEMS); }

static MsPartial* dt_partials(void* tmp) { return (MsPartial*)((char*)tmp + gs_align(sizeof(MsRecord))); }

}  // namespace

extern "C" {

int gs_dtu_mask(const float* gt, int32_t H, int32_t W, float thr, int32_t run, uint8_t* mask, int32_t* count, float* gt_out,
                void* stream) {
  if (H < 1 || W < 1 || run < 1 || !dt_n_ok((int64_t)H * (int64_t)W)) return GS_E_SHAPE;
  if (!gt || !mask || !count || !gt_out) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dtu_mask_kernel, dim3(1), dim3(DT_MASK_THREADS), 0, s, gt, (int)H, (int)W, thr, (int)run, mask, count, gt_out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

size_t gs_masked_tmp_bytes(int64_t n) {
  if (!dt_n_ok(n)) return 0;
  return gs_align(sizeof(MsRecord)) + gs_align((size_t)gs_capped_blocks((size_t)n, DT_BLOCK_ELEMS, DT_MAX_BLOCKS) * sizeof(MsPartial));
}

int gs_masked_fill_fwd(const float* x, const uint8_t* mask, int64_t n, void* tmp, float* out, float* mean_out, void* stream) {
  if (!dt_n_ok(n)) return GS_E_SHAPE;
  if (!x || !mask || !tmp || !out) return GS_E_NULL;
  const int nb = gs_capped_blocks((size_t)n, DT_BLOCK_ELEMS, DT_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ms_stats_kernel, dim3(nb), dim3(GS_BLOCK), 0, s, x, mask, (size_t)n, 0, nb, dt_partials(tmp));
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(mf_fill_kernel, dim3(dt_grid((size_t)n)), dim3(GS_BLOCK), 0, s, x, mask, (size_t)n, nb,
                     (const MsPartial*)dt_partials(tmp), out, mean_out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_masked_fill_bwd(const float* g, const uint8_t* mask, int64_t n, float* g_x, void* stream) {
  if (!dt_n_ok(n)) return GS_E_SHAPE;
  if (!g || !mask || !g_x) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mf_bwd_kernel, dim3(dt_grid((size_t)n)), dim3(GS_BLOCK), 0, s, g, mask, (size_t)n, g_x);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_alpha_penalty_fwd(const float* alpha, const uint8_t* mask, int64_t n, void* tmp, float* out, void* stream) {
  if (!dt_n_ok(n)) return GS_E_SHAPE;
  if (!alpha || !mask || !tmp || !out) return GS_E_NULL;
  const int nb = gs_capped_blocks((size_t)n, DT_BLOCK_ELEMS, DT_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ms_stats_kernel, dim3(nb), dim3(GS_BLOCK), 0, s, alpha, mask, (size_t)n, 1, nb, dt_partials(tmp));
  GS_LAUNCH_CHECK(s, 0);
  hipLaunchKernelGGL(ap_finish_kernel, dim3(1), dim3(GS_BLOCK), 0, s, nb, (const MsPartial*)dt_partials(tmp), (MsRecord*)tmp, out);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_alpha_penalty_bwd(const float* alpha, const uint8_t* mask, int64_t n, const void* tmp, const float* g, float* g_alpha,
                         void* stream) {
  if (!dt_n_ok(n)) return GS_E_SHAPE;
  if (!alpha || !mask || !tmp || !g || !g_alpha) return GS_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ap_bwd_kernel, dim3(dt_grid((size_t)n)), dim3(GS_BLOCK), 0, s, alpha, mask, (size_t)n, (const MsRecord*)tmp, g,
                     g_alpha);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_dng_colour_rule(const float* colour, float* stat, float* opacity, int64_t P, int32_t black_on, float black_thr,
                       float black_div, int32_t black_reset, int32_t white_on, float white_thr, float white_div,
                       int32_t white_reset, float value, int32_t* counts, void* stream) {
  if (!dt_n_ok(P)) return GS_E_SHAPE;
  if (!colour || !stat || !opacity || !counts) return GS_E_NULL;
  CrRule black = {black_on != 0, black_reset != 0, black_thr, black_div};
  CrRule white = {white_on != 0, white_reset != 0, white_thr, white_div};
  const unsigned rows = (unsigned)(((size_t)P + GS_BLOCK - 1) / GS_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cr_kernel, dim3(rows + 1), dim3(GS_BLOCK), 0, s, colour, stat, opacity, (size_t)P, black, white, value, counts);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

}  // extern "C"
