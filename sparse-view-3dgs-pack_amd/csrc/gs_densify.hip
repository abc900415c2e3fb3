// gs_densify.hip - densify, split and prune (LGDWT-GS/scene/gaussian_model.py:395-467) as ONE re-layout on the device:
// the device form of GaussianModelLite.densify_and_prune (gsplat_amd/trainer.py), whose host path is the arbiter.
//
//   plan    per source row: the discrete decisions, one flag byte; per 256-row block the counts of what the block contributes
//   scan    (one workgroup) exclusive prefixes of those counts over the blocks, and the totals the host reads back
//   emit    per source row: where its survivor / clone / samples go in the reference order
//           [survivors | clones | sample block 0 | ... | sample block N-1], and their centres
//   codes   Morton codes of the new centres (gsplat_amd/synthetic.py: morton_order, float64), for the spatial order
//   gather  the HBM pass: every output row's parameters and both Adam moments, written once, in their final order
//
// The plan is a pure per-SOURCE-row decision although the host evaluates its prune on the new rows, because
//   (1) a clone carries its source's raw opacity and scaling and is never a split row (clone needs small, split needs !small),
//       so the prune decision of a clone is the one of its source's survivor;
//   (2) the N samples of a split row share the source's opacity and the same log(exp(s) / (0.8 N)) scaling, so they share one
//       decision.
// tests/test_densify_device_cpu.py proves both against the host path.
//
// No atomics anywhere: a row's position is its block's prefix plus a ballot / popcount rank, so the same inputs give the same bits
// on every run and on every data-parallel rank.  Compiled with -ffp-contract=off: the plan's comparisons and the float64 Morton
// arithmetic are single roundings that restate torch's.
#include <math.h>

#include "gs_common.h"
#include "gs_prof.h"

#define DN_BLOCK 256
#define DN_WAVES (DN_BLOCK / 64)
#define DN_NC GS_DENSIFY_COUNTS  // counts per block: survivors kept, clones kept, split rows, split rows kept, clones selected
#define DN_KIND_SHIFT 30
#define DN_ROW_MASK 0x3FFFFFFFu
#define DN_INVALID 0xFFFFFFFFu
static_assert(GS_BLOCK == DN_BLOCK, "the dormant flags and the plan share the 256-row block");

struct DensifyTmp {
  uint32_t* totals;  // [DN_NC] (the first 256 bytes of tmp: what the host reads)
  uint8_t* flags;    // [P]
  uint32_t* counts;  // [nb][DN_NC]
  uint32_t* prefix;  // [nb][DN_NC] exclusive over the blocks
};
static inline size_t dn_blocks(size_t P) { return (P + DN_BLOCK - 1) / DN_BLOCK; }
static inline size_t dn_tmp_bytes(size_t P) {
  return 256 + gs_align(P) + 2 * gs_align(4 * DN_NC * dn_blocks(P));
}
static inline DensifyTmp dn_tmp_view(void* buf, size_t P) {
  char* p = (char*)buf;
  DensifyTmp t;
  t.totals = (uint32_t*)p; p += 256;
  t.flags = (uint8_t*)p; p += gs_align(P);
  t.counts = (uint32_t*)p; p += gs_align(4 * DN_NC * dn_blocks(P));
  t.prefix = (uint32_t*)p;
  return t;
}

// what a source row contributes, from its flag byte: [0] a survivor, [1] a clone, [2] it is split, [3] its samples are kept
static __device__ __forceinline__ void dn_preds(unsigned f, bool in, bool* c) {
  const bool split = (f & GS_DENSIFY_SPLIT) != 0;
  const bool kept = in && !split && !(f & GS_DENSIFY_PRUNE_SELF);
  c[0] = kept;
  c[1] = kept && (f & GS_DENSIFY_CLONE);
  c[2] = in && split;
  c[3] = in && split && !(f & GS_DENSIFY_PRUNE_SAMPLE);
}

__global__ void __launch_bounds__(DN_BLOCK) densify_plan_kernel(const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                               const float* __restrict__ accum, const float* __restrict__ denom, int P,
                                                               float max_grad, float scale_bound, float min_opacity, float world_bound,
                                                               float sample_div, int size_test, uint8_t* __restrict__ flags,
                                                               uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;   // (size_t: 4 i passes 2^31 long before i does)
  const bool in = i < (size_t)P;
  unsigned f = 0;
  if (in) {
    float g = accum[i] / denom[i];   // (correctly rounded, as torch's)
    if (g != g) g = 0.0f;            // grads[grads.isnan()] = 0
    const float e0 = expf(scaling[3 * i]), e1 = expf(scaling[3 * i + 1]), e2 = expf(scaling[3 * i + 2]);
    const float max_scale = fmaxf(fmaxf(e0, e1), e2);
    const bool small = max_scale <= scale_bound;
    const float op = 1.0f / (1.0f + expf(-opacity[i]));
    const bool faint = op < min_opacity;
    // the chain the host evaluates on the new rows: exp(log(exp(s) / (0.8 N)))
    const float m0 = expf(logf(e0 / sample_div)), m1 = expf(logf(e1 / sample_div)), m2 = expf(logf(e2 / sample_div));
    const float max_sample = fmaxf(fmaxf(m0, m1), m2);
    if (fabsf(g) >= max_grad && small) f |= GS_DENSIFY_CLONE;
    if (g >= max_grad && !small) f |= GS_DENSIFY_SPLIT;
    if (faint || (size_test && max_scale > world_bound)) f |= GS_DENSIFY_PRUNE_SELF;
    if (faint || (size_test && max_sample > world_bound)) f |= GS_DENSIFY_PRUNE_SAMPLE;
    flags[i] = (uint8_t)f;
  }
  bool c[DN_NC];
  dn_preds(f, in, c);
  c[4] = in && (f & GS_DENSIFY_CLONE);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < DN_NC; k++) {
    const unsigned long long b = __ballot(c[k]);
    if (lane == 0) s_cnt[wave][k] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x < DN_NC) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < DN_WAVES; w++) s += s_cnt[w][threadIdx.x];
    counts[(size_t)blockIdx.x * DN_NC + threadIdx.x] = s;
  }
}

// one workgroup: thread t owns the blocks [t per, (t + 1) per); exclusive prefixes in block order, totals last
__global__ void __launch_bounds__(DN_BLOCK) densify_scan_kernel(const uint32_t* __restrict__ counts, int nb, uint32_t* __restrict__ prefix,
                                                               uint32_t* __restrict__ totals) {
  __shared__ uint32_t s_sum[DN_NC][DN_BLOCK];
  const int t = threadIdx.x;
  const int per = (nb + DN_BLOCK - 1) / DN_BLOCK;
  const int lo = min(t * per, nb), hi = min(lo + per, nb);
  uint32_t s[DN_NC];
#pragma unroll
  for (int k = 0; k < DN_NC; k++) s[k] = 0;
  for (int b = lo; b < hi; b++)
#pragma unroll
    for (int k = 0; k < DN_NC; k++) s[k] += counts[(size_t)b * DN_NC + k];
#pragma unroll
  for (int k = 0; k < DN_NC; k++) s_sum[k][t] = s[k];
  __syncthreads();
  uint32_t run[DN_NC];
#pragma unroll
  for (int k = 0; k < DN_NC; k++) {
    uint32_t a = 0;
    for (int u = 0; u < t; u++) a += s_sum[k][u];
    run[k] = a;
  }
  for (int b = lo; b < hi; b++)
#pragma unroll
    for (int k = 0; k < DN_NC; k++) {
      prefix[(size_t)b * DN_NC + k] = run[k];
      run[k] += counts[(size_t)b * DN_NC + k];
    }
  if (t == DN_BLOCK - 1)
#pragma unroll
    for (int k = 0; k < DN_NC; k++) totals[k] = run[k];
}

struct EmitCounts {
  uint32_t n_keep, n_clone_keep, n_split, n_split_keep;
};

__global__ void __launch_bounds__(DN_BLOCK) densify_emit_kernel(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ prefix,
                                                               const uint32_t* __restrict__ totals, const float* __restrict__ xyz,
                                                               const float* __restrict__ scaling, const float* __restrict__ rotation,
                                                               const float* __restrict__ noise, int P, int N, EmitCounts n, uint32_t P2,
                                                               uint32_t* __restrict__ table, float* __restrict__ new_xyz) {
  __shared__ uint32_t s_cnt[DN_WAVES][4];
  // the counts the host sized the outputs with must be the plan's: anything else would place rows out of range
  if (totals[0] != n.n_keep || totals[1] != n.n_clone_keep || totals[2] != n.n_split || totals[3] != n.n_split_keep) return;
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = i < (size_t)P;
  const unsigned f = in ? flags[i] : 0u;
  bool c[4];
  dn_preds(f, in, c);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t rank[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned long long b = __ballot(c[k]);
    rank[k] = (uint32_t)__popcll(b & below);
    if (lane == 0) s_cnt[wave][k] = (uint32_t)__popcll(b);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    for (int w = 0; w < wave; w++) rank[k] += s_cnt[w][k];
    rank[k] += prefix[(size_t)blockIdx.x * DN_NC + k];   // ascending source row inside every group
  }
  if (!in) return;
  const float x0 = xyz[3 * i], x1 = xyz[3 * i + 1], x2 = xyz[3 * i + 2];
  if (c[0]) {
    const uint32_t j = rank[0];
    if (j < P2) {
      table[j] = (uint32_t)i | ((uint32_t)GS_DENSIFY_SURVIVOR << DN_KIND_SHIFT);
      new_xyz[3 * (size_t)j] = x0; new_xyz[3 * (size_t)j + 1] = x1; new_xyz[3 * (size_t)j + 2] = x2;
    }
  }
  if (c[1]) {
    const uint32_t j = n.n_keep + rank[1];
    if (j < P2) {
      table[j] = (uint32_t)i | ((uint32_t)GS_DENSIFY_CLONED << DN_KIND_SHIFT);
      new_xyz[3 * (size_t)j] = x0; new_xyz[3 * (size_t)j + 1] = x1; new_xyz[3 * (size_t)j + 2] = x2;
    }
  }
  if (c[3]) {
    // build_rotation (general_utils.py:78-99) of the normalised quaternion; samples = noise * exp(scaling); R samples + xyz
    const float r0 = rotation[4 * i], r1 = rotation[4 * i + 1], r2 = rotation[4 * i + 2], r3 = rotation[4 * i + 3];
    const float nrm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const float w = r0 / nrm, x = r1 / nrm, y = r2 / nrm, z = r3 / nrm;
    const float R00 = 1.0f - 2.0f * (y * y + z * z), R01 = 2.0f * (x * y - w * z), R02 = 2.0f * (x * z + w * y);
    const float R10 = 2.0f * (x * y + w * z), R11 = 1.0f - 2.0f * (x * x + z * z), R12 = 2.0f * (y * z - w * x);
    const float R20 = 2.0f * (x * z - w * y), R21 = 2.0f * (y * z + w * x), R22 = 1.0f - 2.0f * (x * x + y * y);
    const float s0 = expf(scaling[3 * i]), s1 = expf(scaling[3 * i + 1]), s2 = expf(scaling[3 * i + 2]);
    const uint32_t r = rank[2];   // among ALL split rows: the row of the host's noise.repeat(N, 1) order
    for (int k = 0; k < N; k++) {
      const uint32_t j = n.n_keep + n.n_clone_keep + (uint32_t)k * n.n_split_keep + rank[3];
      if (r >= n.n_split || j >= P2) continue;
      const float* nz = noise + 3 * ((size_t)k * n.n_split + r);
      const float v0 = nz[0] * s0, v1 = nz[1] * s1, v2 = nz[2] * s2;
      table[j] = (uint32_t)i | ((uint32_t)GS_DENSIFY_SAMPLE << DN_KIND_SHIFT);
      new_xyz[3 * (size_t)j] = (R00 * v0 + R01 * v1 + R02 * v2) + x0;
      new_xyz[3 * (size_t)j + 1] = (R10 * v0 + R11 * v1 + R12 * v2) + x1;
      new_xyz[3 * (size_t)j + 2] = (R20 * v0 + R21 * v1 + R22 * v2) + x2;
    }
  }
}

// synthetic.morton_order's arithmetic in float64: q = clamp(rint((x - lo) / max(hi - lo, 1e-30) * 1023), 0, 1023), bits of
// x, y, z interleaved from bit 0 upward (torch.round is half-to-even: rint in the default rounding mode)
__global__ void __launch_bounds__(DN_BLOCK) morton_codes_kernel(const float* __restrict__ xyz, long long n, const float* __restrict__ lo,
                                                               const float* __restrict__ hi, int32_t* __restrict__ codes) {
  const long long i = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t q[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double l = (double)lo[a], h = (double)hi[a];
    const double v = rint(((double)xyz[3 * i + a] - l) / fmax(h - l, 1e-30) * 1023.0);
    q[a] = v >= 1023.0 ? 1023u : (v > 0.0 ? (uint32_t)v : 0u);
  }
  uint32_t code = 0;
#pragma unroll
  for (int b = 0; b < 10; b++)
#pragma unroll
    for (int a = 0; a < 3; a++) code |= ((q[a] >> b) & 1u) << (3 * b + a);
  codes[i] = (int32_t)code;
}

// ------------------------------------------------------------------------------------------------------------------
// The gather.  The flat buffers are field-major ([P, w_f] blocks back to back); workgroup (x, y) writes the 256 w_f floats of
// rows [256 x, 256 x + 256) of field y: consecutive lanes write consecutive floats (fully coalesced), and read runs of one row
// of the field.  The rows' table entries are fetched once per workgroup into LDS.
// ------------------------------------------------------------------------------------------------------------------
#define DN_MAX_FIELDS 8
#define DN_UNROLL 4
struct GatherFields {
  int n;
  int width[DN_MAX_FIELDS];
  long long old_off[DN_MAX_FIELDS];  // start of the field's [P, w] block in the old buffers
  long long new_off[DN_MAX_FIELDS];  // ... of its [P2, w] block in the new ones
  int xyz_field, scaling_field;
};

template <int WC>
static __device__ __forceinline__ void gather_rows(const uint32_t* s_ent, const uint32_t* s_e, int rows, int w_rt, bool is_xyz,
                                                   bool is_scaling, float sample_div, const float* __restrict__ new_xyz,
                                                   const float* __restrict__ op, const float* __restrict__ om,
                                                   const float* __restrict__ ov, float* __restrict__ np, float* __restrict__ nm,
                                                   float* __restrict__ nv) {
  const int w = WC ? WC : w_rt;
  const int total = rows * w;
  // DN_UNROLL independent elements per thread and trip: their loads are all in flight before the first store
  for (int base = threadIdx.x; base < total; base += DN_BLOCK * DN_UNROLL) {
    float p[DN_UNROLL], m[DN_UNROLL], v[DN_UNROLL];
    bool ok[DN_UNROLL];
#pragma unroll
    for (int u = 0; u < DN_UNROLL; u++) {
      const int idx = base + u * DN_BLOCK;
      p[u] = m[u] = v[u] = 0.0f;
      ok[u] = false;
      if (idx >= total) continue;
      const int jl = idx / w, c = idx - jl * w;
      const uint32_t ent = s_ent[jl];
      if (ent == DN_INVALID) continue;
      ok[u] = true;
      const uint32_t kind = ent >> DN_KIND_SHIFT;
      const size_t so = (size_t)(ent & DN_ROW_MASK) * w + c;
      if (is_xyz) {
        p[u] = new_xyz[3 * (size_t)s_e[jl] + c];   // (a copy of the source's for a survivor or a clone)
      } else {
        p[u] = op[so];
        if (is_scaling && kind == GS_DENSIFY_SAMPLE) p[u] = logf(expf(p[u]) / sample_div);
      }
      if (kind == GS_DENSIFY_SURVIVOR) {
        m[u] = om[so];
        v[u] = ov[so];
      }
    }
#pragma unroll
    for (int u = 0; u < DN_UNROLL; u++) {
      const int idx = base + u * DN_BLOCK;
      if (!ok[u]) continue;
      np[idx] = p[u];
      nm[idx] = m[u];
      nv[idx] = v[u];
    }
  }
}

__global__ void __launch_bounds__(DN_BLOCK) densify_gather_kernel(const long long* __restrict__ perm, const uint32_t* __restrict__ table,
                                                                 const float* __restrict__ new_xyz, uint32_t P2,
                                                                 const float* __restrict__ old_p, const float* __restrict__ old_m,
                                                                 const float* __restrict__ old_v, uint32_t P, float* __restrict__ new_p,
                                                                 float* __restrict__ new_m, float* __restrict__ new_v, GatherFields f,
                                                                 float sample_div) {
  __shared__ uint32_t s_ent[DN_BLOCK], s_e[DN_BLOCK];
  const int fi = blockIdx.y;
  const uint32_t j0 = blockIdx.x * DN_BLOCK;
  const int rows = (int)min((uint32_t)DN_BLOCK, P2 - j0);
  {
    uint32_t ent = DN_INVALID, e = 0;
    if ((int)threadIdx.x < rows) {
      const unsigned long long ee = perm ? (unsigned long long)perm[j0 + threadIdx.x] : (unsigned long long)(j0 + threadIdx.x);
      if (ee < P2) {
        e = (uint32_t)ee;
        ent = table[e];
        if ((ent >> DN_KIND_SHIFT) > GS_DENSIFY_SAMPLE || (ent & DN_ROW_MASK) >= P) ent = DN_INVALID;
      }
    }
    s_ent[threadIdx.x] = ent;
    s_e[threadIdx.x] = e;
  }
  __syncthreads();
  const int w = f.width[fi];
  const float* op = old_p + f.old_off[fi];
  const float* om = old_m + f.old_off[fi];
  const float* ov = old_v + f.old_off[fi];
  const size_t base = (size_t)f.new_off[fi] + (size_t)j0 * w;
  float* np = new_p + base;
  float* nm = new_m + base;
  float* nv = new_v + base;
  const bool is_xyz = fi == f.xyz_field, is_scaling = fi == f.scaling_field;
#define DN_GATHER(WC) gather_rows<WC>(s_ent, s_e, rows, w, is_xyz, is_scaling, sample_div, new_xyz, op, om, ov, np, nm, nv)
  switch (w) {   // (workgroup-uniform: the division by the row width is by a constant for the model's own widths)
    case 1: DN_GATHER(1); break;
    case 3: DN_GATHER(3); break;
    case 4: DN_GATHER(4); break;
    case 48: DN_GATHER(48); break;
    default: DN_GATHER(0); break;
  }
#undef DN_GATHER
}

extern "C" {

size_t gs_densify_tmp_bytes(int32_t P) { return P < 1 ? 0 : dn_tmp_bytes((size_t)P); }

int gs_densify_plan(const float* scaling, const float* opacity, const float* xyz_gradient_accum, const float* denom, int32_t P,
                    int32_t N, float max_grad, float scale_bound, float min_opacity, float world_bound, float sample_div,
                    int32_t size_test, void* tmp, size_t tmp_bytes, void* stream) {
  if (!scaling || !opacity || !xyz_gradient_accum || !denom || !tmp) return GS_E_NULL;
  if (P < 1 || P > (int32_t)DN_ROW_MASK || N < 1 || N > GS_DENSIFY_MAX_N) return GS_E_SHAPE;
  if (tmp_bytes < dn_tmp_bytes((size_t)P)) return GS_E_SCRATCH;
  const DensifyTmp t = dn_tmp_view(tmp, (size_t)P);
  const int nb = (int)dn_blocks((size_t)P);
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(densify_plan_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, scaling, opacity, xyz_gradient_accum, denom, P, max_grad,
                     scale_bound, min_opacity, world_bound, sample_div, size_test ? 1 : 0, t.flags, t.counts);
  hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(DN_BLOCK), 0, s, t.counts, nb, t.prefix, t.totals);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_densify_emit(const void* tmp, size_t tmp_bytes, const float* xyz, const float* scaling, const float* rotation,
                    const float* noise, int32_t P, int32_t N, int32_t n_keep, int32_t n_clone_keep, int32_t n_split,
                    int32_t n_split_keep, int32_t P2, uint32_t* table, float* new_xyz, void* stream) {
  if (!tmp || !xyz || !scaling || !rotation || !table || !new_xyz) return GS_E_NULL;
  if (P < 1 || P > (int32_t)DN_ROW_MASK || N < 1 || N > GS_DENSIFY_MAX_N) return GS_E_SHAPE;
  if (n_keep < 0 || n_clone_keep < 0 || n_split < 0 || n_split_keep < 0 || n_split_keep > n_split || n_clone_keep > n_keep ||
      (int64_t)n_keep + n_split > P || P2 < 1 || (int64_t)n_keep + n_clone_keep + (int64_t)N * n_split_keep != P2)
    return GS_E_SHAPE;
  if (n_split_keep > 0 && !noise) return GS_E_NULL;
  if (tmp_bytes < dn_tmp_bytes((size_t)P)) return GS_E_SCRATCH;
  const DensifyTmp t = dn_tmp_view(const_cast<void*>(tmp), (size_t)P);
  EmitCounts n;
  n.n_keep = (uint32_t)n_keep; n.n_clone_keep = (uint32_t)n_clone_keep;
  n.n_split = (uint32_t)n_split; n.n_split_keep = (uint32_t)n_split_keep;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(densify_emit_kernel, dim3((unsigned)dn_blocks((size_t)P)), dim3(DN_BLOCK), 0, s, t.flags, t.prefix, t.totals, xyz,
                     scaling, rotation, noise, P, N, n, (uint32_t)P2, table, new_xyz);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_morton_codes(const float* xyz, int64_t n, const float* lo, const float* hi, int32_t* codes, void* stream) {
  if (!xyz || !lo || !hi || !codes) return GS_E_NULL;
  if (n < 1 || n > (int64_t)DN_ROW_MASK) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(morton_codes_kernel, dim3((unsigned)((n + DN_BLOCK - 1) / DN_BLOCK)), dim3(DN_BLOCK), 0, s, xyz, (long long)n, lo,
                     hi, codes);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_densify_gather(const int64_t* perm, const uint32_t* table, const float* new_xyz, int32_t P2, const float* old_flat,
                      const float* old_exp_avg, const float* old_exp_avg_sq, int32_t P, float* new_flat, float* new_exp_avg,
                      float* new_exp_avg_sq, int32_t nfields, const int32_t* widths, int32_t xyz_field, int32_t scaling_field,
                      float sample_div, void* stream) {
  if (!table || !new_xyz || !old_flat || !old_exp_avg || !old_exp_avg_sq || !new_flat || !new_exp_avg || !new_exp_avg_sq || !widths)
    return GS_E_NULL;
  if (P < 1 || P > (int32_t)DN_ROW_MASK || P2 < 1 || P2 > (int32_t)DN_ROW_MASK || nfields < 1 || nfields > DN_MAX_FIELDS ||
      xyz_field < 0 || xyz_field >= nfields || scaling_field < 0 || scaling_field >= nfields || xyz_field == scaling_field)
    return GS_E_SHAPE;
  GatherFields f;
  f.n = nfields;
  f.xyz_field = xyz_field;
  f.scaling_field = scaling_field;
  long long co = 0;
  for (int q = 0; q < DN_MAX_FIELDS; q++) {
    const int w = q < nfields ? widths[q] : 0;
    if (q < nfields && (w < 1 || w > 4096)) return GS_E_SHAPE;
    f.width[q] = w;
    f.old_off[q] = co * P;
    f.new_off[q] = co * P2;
    co += w;
  }
  if (widths[xyz_field] != 3) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(densify_gather_kernel, dim3((unsigned)dn_blocks((size_t)P2), (unsigned)nfields), dim3(DN_BLOCK), 0, s,
                     (const long long*)perm, table, new_xyz, (uint32_t)P2, old_flat, old_exp_avg, old_exp_avg_sq, (uint32_t)P, new_flat,
                     new_exp_avg, new_exp_avg_sq, f, sample_div);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}
}
