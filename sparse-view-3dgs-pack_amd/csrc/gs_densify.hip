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
//
// DNGaussian's rule (DNGaussian/scene/gaussian_model.py:454-524, GaussianModelLite.densify_and_prune_dng) is the same plan with one
// more condition on clone and split, sigmoid(opacity) > opa_thresh (gs_densify_plan_gated): still a per-source-row decision, since
// the gate reads the source's own opacity.  Its mask prunes (prune_points: near-camera, unseen, opacity) are a plan / emit pair of
// their own in front of the same gather (gs_prune_plan / gs_prune_emit).
//
// The second half of the file is FSGS's densification (FSGS/scene/gaussian_model.py:424-491, the device form of
// GaussianModelLite.densify_and_prune_fsgs): its stages hang on two kNN searches (see there).
//
// What the rules share stands once, in front of the kernels: dn_block_ranks (every plan and emit kernel's ballot / popcount
// ranks), dn_row_measures (both plans' per-row measures; each rule sets its own flag bits from them), dn_rotation /
// dn_sample_centre / dn_put_row / dn_put_samples (both emits), and ONE gather body, gather_rows<WC, PROX> in gather_block<PROX>:
// densify_gather_kernel (PROX off: no proximity branch, no neighbour-kind array) and fsgs_gather_kernel are its two
// instantiations, and dn_gather builds and checks the field table of both entry points.
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

// In-block exclusive ranks of K predicates - ballot / popcount inside the wave, the waves' counts through LDS - and the block's
// counts.  Every thread of the workgroup calls it (it synchronises), or none: an early return in front of it must be uniform
// over the workgroup.
template <int K>
static __device__ __forceinline__ void dn_block_ranks(const bool* c, uint32_t (*s_cnt)[DN_NC], uint32_t* rank, uint32_t* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const unsigned long long b = __ballot(c[k]);
    rank[k] = (uint32_t)__popcll(b & below);
    if (lane == 0) s_cnt[wave][k] = (uint32_t)__popcll(b);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    total[k] = 0;
#pragma unroll
    for (int w = 0; w < DN_WAVES; w++) {
      if (w < wave) rank[k] += s_cnt[w][k];
      total[k] += s_cnt[w][k];
    }
  }
}

// What both rules' plans measure of a source row (the flag bits they derive from it differ): the statistic g, the largest
// activated scale of the row and of its split samples, the activated opacity.
struct RowMeasures {
  float g, max_scale, op, max_sample;
  bool small, faint;
};
static __device__ __forceinline__ RowMeasures dn_row_measures(const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                              const float* __restrict__ accum, const float* __restrict__ denom,
                                                              size_t i, float scale_bound, float min_opacity, float sample_div) {
  RowMeasures m;
  m.g = accum[i] / denom[i];   // (correctly rounded, as torch's)
  if (m.g != m.g) m.g = 0.0f;  // grads[grads.isnan()] = 0
  const float e0 = expf(scaling[3 * i]), e1 = expf(scaling[3 * i + 1]), e2 = expf(scaling[3 * i + 2]);
  m.max_scale = fmaxf(fmaxf(e0, e1), e2);
  m.small = m.max_scale <= scale_bound;
  m.op = 1.0f / (1.0f + expf(-opacity[i]));
  m.faint = m.op < min_opacity;
  // the chain the host evaluates on the new rows: exp(log(exp(s) / (0.8 N)))
  const float m0 = expf(logf(e0 / sample_div)), m1 = expf(logf(e1 / sample_div)), m2 = expf(logf(e2 / sample_div));
  m.max_sample = fmaxf(fmaxf(m0, m1), m2);
  return m;
}

// build_rotation (general_utils.py:78-99) of the normalised quaternion, row-major
static __device__ __forceinline__ void dn_rotation(const float* __restrict__ q, float* R) {
  const float r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3];
  const float nrm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
  const float w = r0 / nrm, x = r1 / nrm, y = r2 / nrm, z = r3 / nrm;
  R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - w * z); R[2] = 2.0f * (x * z + w * y);
  R[3] = 2.0f * (x * y + w * z); R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - w * x);
  R[6] = 2.0f * (x * z - w * y); R[7] = 2.0f * (y * z + w * x); R[8] = 1.0f - 2.0f * (x * x + y * y);
}
// samples = noise * exp(scaling); R samples + xyz
static __device__ __forceinline__ void dn_sample_centre(const float* R, const float* s, const float* __restrict__ nz, const float* x,
                                                        float* out) {
  const float v0 = nz[0] * s[0], v1 = nz[1] * s[1], v2 = nz[2] * s[2];
  out[0] = (R[0] * v0 + R[1] * v1 + R[2] * v2) + x[0];
  out[1] = (R[3] * v0 + R[4] * v1 + R[5] * v2) + x[1];
  out[2] = (R[6] * v0 + R[7] * v1 + R[8] * v2) + x[2];
}
// output row j (if it is one of the n_out rows): its table entry - source row and kind - and its centre
static __device__ __forceinline__ void dn_put_row(uint32_t* __restrict__ table, float* __restrict__ xyz_out, uint32_t j, uint32_t n_out,
                                                  size_t src, uint32_t kind, const float* x) {
  if (j >= n_out) return;
  table[j] = (uint32_t)src | (kind << DN_KIND_SHIFT);
  xyz_out[3 * (size_t)j] = x[0]; xyz_out[3 * (size_t)j + 1] = x[1]; xyz_out[3 * (size_t)j + 2] = x[2];
}
// the N samples of split row i, the r-th of n_split split rows (the row of the host's noise.repeat(N, 1) order): sample k is
// output row j0 + k stride
static __device__ __forceinline__ void dn_put_samples(const float* __restrict__ scaling, const float* __restrict__ rotation,
                                                      const float* __restrict__ noise, size_t i, const float* x, uint32_t r,
                                                      uint32_t n_split, int N, uint32_t j0, uint32_t stride, uint32_t n_out,
                                                      uint32_t* __restrict__ table, float* __restrict__ xyz_out) {
  if (r >= n_split) return;
  float R[9], c[3];
  dn_rotation(rotation + 4 * i, R);
  const float s[3] = {expf(scaling[3 * i]), expf(scaling[3 * i + 1]), expf(scaling[3 * i + 2])};
  for (int k = 0; k < N; k++) {
    dn_sample_centre(R, s, noise + 3 * ((size_t)k * n_split + r), x, c);
    dn_put_row(table, xyz_out, j0 + (uint32_t)k * stride, n_out, i, GS_DENSIFY_SAMPLE, c);
  }
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
                                                               float sample_div, int size_test, int gated, float gate_opacity,
                                                               uint8_t* __restrict__ flags, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;   // (size_t: 4 i passes 2^31 long before i does)
  const bool in = i < (size_t)P;
  unsigned f = 0;
  if (in) {
    const RowMeasures m = dn_row_measures(scaling, opacity, accum, denom, i, scale_bound, min_opacity, sample_div);
    // DNGaussian's rule (gs_densify_plan_gated): clone and split also need get_opacity > opa_thresh; a NaN opacity selects nothing
    const bool open = !gated || m.op > gate_opacity;
    if (fabsf(m.g) >= max_grad && m.small && open) f |= GS_DENSIFY_CLONE;
    if (m.g >= max_grad && !m.small && open) f |= GS_DENSIFY_SPLIT;
    if (m.faint || (size_test && m.max_scale > world_bound)) f |= GS_DENSIFY_PRUNE_SELF;
    if (m.faint || (size_test && m.max_sample > world_bound)) f |= GS_DENSIFY_PRUNE_SAMPLE;
    flags[i] = (uint8_t)f;
  }
  bool c[DN_NC];
  dn_preds(f, in, c);
  c[4] = in && (f & GS_DENSIFY_CLONE);
  uint32_t rank[DN_NC], total[DN_NC];
  dn_block_ranks<DN_NC>(c, s_cnt, rank, total);
  if (threadIdx.x < DN_NC) counts[(size_t)blockIdx.x * DN_NC + threadIdx.x] = total[threadIdx.x];
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
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  // the counts the host sized the outputs with must be the plan's: anything else would place rows out of range (uniform over
  // the grid: nobody reaches the barrier)
  if (totals[0] != n.n_keep || totals[1] != n.n_clone_keep || totals[2] != n.n_split || totals[3] != n.n_split_keep) return;
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = i < (size_t)P;
  const unsigned f = in ? flags[i] : 0u;
  bool c[4];
  dn_preds(f, in, c);
  uint32_t rank[4], total[4];
  dn_block_ranks<4>(c, s_cnt, rank, total);
  if (!in) return;
#pragma unroll
  for (int k = 0; k < 4; k++) rank[k] += prefix[(size_t)blockIdx.x * DN_NC + k];   // ascending source row inside every group
  const float x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  if (c[0]) dn_put_row(table, new_xyz, rank[0], P2, i, GS_DENSIFY_SURVIVOR, x);
  if (c[1]) dn_put_row(table, new_xyz, n.n_keep + rank[1], P2, i, GS_DENSIFY_CLONED, x);
  if (c[3])   // rank[2]: among ALL split rows, kept or not
    dn_put_samples(scaling, rotation, noise, i, x, rank[2], n.n_split, N, n.n_keep + n.n_clone_keep + rank[3], n.n_split_keep, P2,
                   table, new_xyz);
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
// The gather, of both rules.  The flat buffers are field-major ([P, w_f] blocks back to back); workgroup (x, y) writes the
// 256 w_f floats of rows [256 x, 256 x + 256) of field y: consecutive lanes write consecutive floats (fully coalesced), and read
// runs of one row of the field.  The rows' table entries are fetched once per workgroup into LDS.
// PROX (FSGS): the table may hold proximity rows - the neighbour's raw scaling (sample-transformed if the neighbour, whose kind
// is in nb_kind, is a sample) and raw opacity, rotation (1, 0, 0, 0), every other field 0, moments +0.  Without PROX such an
// entry is dropped, and there is no neighbour-kind array.
// ------------------------------------------------------------------------------------------------------------------
#define DN_MAX_FIELDS 8
#define DN_UNROLL 4
enum { DN_ROLE_COPY = 0, DN_ROLE_XYZ, DN_ROLE_SCALING, DN_ROLE_OPACITY, DN_ROLE_ROTATION };
struct GatherFields {
  int n;
  int width[DN_MAX_FIELDS];
  int role[DN_MAX_FIELDS];
  long long old_off[DN_MAX_FIELDS];  // start of the field's [P, w] block in the old buffers
  long long new_off[DN_MAX_FIELDS];  // ... of its [P2, w] block in the new ones
};

template <int WC, bool PROX>
static __device__ __forceinline__ void gather_rows(const uint32_t* s_ent, const uint32_t* s_e, const uint8_t* s_nk, int rows, int w_rt,
                                                   int role, float sample_div, const float* __restrict__ new_xyz,
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
      const bool prox = PROX && kind == GS_DENSIFY_PROXIMITY;
      if (role == DN_ROLE_XYZ) {
        p[u] = new_xyz[3 * (size_t)s_e[jl] + c];   // (a copy of the source's for a survivor or a clone)
      } else if (role == DN_ROLE_SCALING) {
        p[u] = op[so];
        if (kind == GS_DENSIFY_SAMPLE || (prox && s_nk[jl] == GS_DENSIFY_SAMPLE)) p[u] = logf(expf(p[u]) / sample_div);
      } else if (!prox || role == DN_ROLE_OPACITY) {   // a copy: every field of the other kinds, the opacity of a proximity row
        p[u] = op[so];
      } else if (role == DN_ROLE_ROTATION) {
        p[u] = c == 0 ? 1.0f : 0.0f;
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

// one workgroup of the gather; s_ent, s_e (and s_nk with PROX): DN_BLOCK entries of LDS each
template <bool PROX>
static __device__ __forceinline__ void gather_block(uint32_t* s_ent, uint32_t* s_e, uint8_t* s_nk, const long long* __restrict__ perm,
                                                    const uint32_t* __restrict__ table, const uint8_t* __restrict__ nb_kind,
                                                    const float* __restrict__ new_xyz, uint32_t P2, const float* __restrict__ old_p,
                                                    const float* __restrict__ old_m, const float* __restrict__ old_v, uint32_t P,
                                                    float* __restrict__ new_p, float* __restrict__ new_m, float* __restrict__ new_v,
                                                    const GatherFields& f, float sample_div) {
  const int fi = blockIdx.y;
  const uint32_t j0 = blockIdx.x * DN_BLOCK;
  const int rows = (int)min((uint32_t)DN_BLOCK, P2 - j0);
  {
    uint32_t ent = DN_INVALID, e = 0;
    uint8_t nk = 0;
    if ((int)threadIdx.x < rows) {
      const unsigned long long ee = perm ? (unsigned long long)perm[j0 + threadIdx.x] : (unsigned long long)(j0 + threadIdx.x);
      if (ee < P2) {
        e = (uint32_t)ee;
        ent = table[e];
        if (PROX) nk = nb_kind[e];
        if ((!PROX && (ent >> DN_KIND_SHIFT) > GS_DENSIFY_SAMPLE) || (ent & DN_ROW_MASK) >= P) ent = DN_INVALID;
      }
    }
    s_ent[threadIdx.x] = ent;
    s_e[threadIdx.x] = e;
    if (PROX) s_nk[threadIdx.x] = nk;
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
#define DN_GATHER(WC) gather_rows<WC, PROX>(s_ent, s_e, s_nk, rows, w, f.role[fi], sample_div, new_xyz, op, om, ov, np, nm, nv)
  switch (w) {   // (workgroup-uniform: the division by the row width is by a constant for the model's own widths)
    case 1: DN_GATHER(1); break;
    case 3: DN_GATHER(3); break;
    case 4: DN_GATHER(4); break;
    case 48: DN_GATHER(48); break;
    default: DN_GATHER(0); break;
  }
#undef DN_GATHER
}

__global__ void __launch_bounds__(DN_BLOCK) densify_gather_kernel(const long long* __restrict__ perm, const uint32_t* __restrict__ table,
                                                                 const float* __restrict__ new_xyz, uint32_t P2,
                                                                 const float* __restrict__ old_p, const float* __restrict__ old_m,
                                                                 const float* __restrict__ old_v, uint32_t P, float* __restrict__ new_p,
                                                                 float* __restrict__ new_m, float* __restrict__ new_v, GatherFields f,
                                                                 float sample_div) {
  __shared__ uint32_t s_ent[DN_BLOCK], s_e[DN_BLOCK];
  gather_block<false>(s_ent, s_e, nullptr, perm, table, nullptr, new_xyz, P2, old_p, old_m, old_v, P, new_p, new_m, new_v, f,
                      sample_div);
}

__global__ void __launch_bounds__(DN_BLOCK) fsgs_gather_kernel(const long long* __restrict__ perm, const uint32_t* __restrict__ table,
                                                              const uint8_t* __restrict__ nb_kind, const float* __restrict__ new_xyz,
                                                              uint32_t P2, const float* __restrict__ old_p, const float* __restrict__ old_m,
                                                              const float* __restrict__ old_v, uint32_t P, float* __restrict__ new_p,
                                                              float* __restrict__ new_m, float* __restrict__ new_v, GatherFields f,
                                                              float sample_div) {
  __shared__ uint32_t s_ent[DN_BLOCK], s_e[DN_BLOCK];
  __shared__ uint8_t s_nk[DN_BLOCK];
  gather_block<true>(s_ent, s_e, s_nk, perm, table, nb_kind, new_xyz, P2, old_p, old_m, old_v, P, new_p, new_m, new_v, f, sample_div);
}

// Both gather entry points behind their null checks: the field table from the widths and the special fields - special[0] the
// centres (width 3), [1] the scaling, with nb_kind also [2] the opacity and [3] the rotation; all distinct - and the launch.
static int dn_gather(const int64_t* perm, const uint32_t* table, const uint8_t* nb_kind, const float* new_xyz, int32_t P2,
                     const float* old_flat, const float* old_exp_avg, const float* old_exp_avg_sq, int32_t P, float* new_flat,
                     float* new_exp_avg, float* new_exp_avg_sq, int32_t nfields, const int32_t* widths, const int32_t* special,
                     float sample_div, void* stream) {
  if (P < 1 || P > (int32_t)DN_ROW_MASK || P2 < 1 || P2 > (int32_t)DN_ROW_MASK || nfields < 1 || nfields > DN_MAX_FIELDS)
    return GS_E_SHAPE;
  GatherFields f;
  f.n = nfields;
  long long co = 0;
  for (int q = 0; q < DN_MAX_FIELDS; q++) {
    const int w = q < nfields ? widths[q] : 0;
    if (q < nfields && (w < 1 || w > 4096)) return GS_E_SHAPE;
    f.width[q] = w;
    f.role[q] = DN_ROLE_COPY;
    f.old_off[q] = co * P;
    f.new_off[q] = co * P2;
    co += w;
  }
  for (int a = 0; a < (nb_kind ? 4 : 2); a++) {
    if (special[a] < 0 || special[a] >= nfields || f.role[special[a]] != DN_ROLE_COPY) return GS_E_SHAPE;
    f.role[special[a]] = DN_ROLE_XYZ + a;
  }
  if (widths[special[0]] != 3) return GS_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  const dim3 grid((unsigned)dn_blocks((size_t)P2), (unsigned)nfields);
  if (nb_kind)
    hipLaunchKernelGGL(fsgs_gather_kernel, grid, dim3(DN_BLOCK), 0, s, (const long long*)perm, table, nb_kind, new_xyz, (uint32_t)P2,
                       old_flat, old_exp_avg, old_exp_avg_sq, (uint32_t)P, new_flat, new_exp_avg, new_exp_avg_sq, f, sample_div);
  else
    hipLaunchKernelGGL(densify_gather_kernel, grid, dim3(DN_BLOCK), 0, s, (const long long*)perm, table, new_xyz, (uint32_t)P2, old_flat,
                       old_exp_avg, old_exp_avg_sq, (uint32_t)P, new_flat, new_exp_avg, new_exp_avg_sq, f, sample_div);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// The mask prune (DNGaussian/scene/gaussian_model.py:374-392, the device form of GaussianModelLite.prune_points): the rows whose
// mask byte is 0, in their old order.  plan: rows kept per 256-row block, in the DN_NC-strided count layout so that the one-workgroup
// scan above serves it unchanged (columns 1 .. 4 stay 0); emit: destination = block prefix + ballot / popcount rank, the table
// entry (a survivor), the centre, and the three densification statistics, which a prune indexes and does not zero.  The
// parameters and moments then go through densify_gather_kernel with that table.
// ------------------------------------------------------------------------------------------------------------------
struct PruneTmp {
  uint32_t* totals;  // [DN_NC] in the first 256 bytes: word 0 = rows kept
  uint32_t* counts;  // [nb][DN_NC]
  uint32_t* prefix;  // [nb][DN_NC]
};
static inline size_t pr_tmp_bytes(size_t P) { return 256 + 2 * gs_align(4 * DN_NC * dn_blocks(P)); }
static inline PruneTmp pr_tmp_view(void* buf, size_t P) {
  char* p = (char*)buf;
  PruneTmp t;
  t.totals = (uint32_t*)p; p += 256;
  t.counts = (uint32_t*)p; p += gs_align(4 * DN_NC * dn_blocks(P));
  t.prefix = (uint32_t*)p;
  return t;
}

__global__ void __launch_bounds__(DN_BLOCK) prune_plan_kernel(const uint8_t* __restrict__ mask, int P, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool c[1] = {i < (size_t)P && mask[i] == 0};
  uint32_t rank[1], total[1];
  dn_block_ranks<1>(c, s_cnt, rank, total);
  if (threadIdx.x < DN_NC) counts[(size_t)blockIdx.x * DN_NC + threadIdx.x] = threadIdx.x == 0 ? total[0] : 0u;
}

__global__ void __launch_bounds__(DN_BLOCK) prune_emit_kernel(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ prefix,
                                                             const uint32_t* __restrict__ totals, const float* __restrict__ xyz,
                                                             const float* __restrict__ accum, const float* __restrict__ denom,
                                                             const float* __restrict__ radii, int P, uint32_t P2,
                                                             uint32_t* __restrict__ table, float* __restrict__ new_xyz,
                                                             float* __restrict__ new_accum, float* __restrict__ new_denom,
                                                             float* __restrict__ new_radii) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  // the count the host sized the outputs with must be the plan's (uniform over the grid: nobody reaches the barrier)
  if (totals[0] != P2) return;
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool c[1] = {i < (size_t)P && mask[i] == 0};
  uint32_t rank[1], total[1];
  dn_block_ranks<1>(c, s_cnt, rank, total);
  if (!c[0]) return;
  const size_t j = (size_t)prefix[(size_t)blockIdx.x * DN_NC] + rank[0];   // ascending source row: the old relative order
  if (j >= (size_t)P2) return;
  const float x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  dn_put_row(table, new_xyz, (uint32_t)j, P2, i, GS_DENSIFY_SURVIVOR, x);
  new_accum[j] = accum[i];
  new_denom[j] = denom[i];
  new_radii[j] = radii[i];
}

extern "C" {

size_t gs_densify_tmp_bytes(int32_t P) { return P < 1 ? 0 : dn_tmp_bytes((size_t)P); }

static int dn_plan(const float* scaling, const float* opacity, const float* xyz_gradient_accum, const float* denom, int32_t P, int32_t N,
                   float max_grad, float scale_bound, float min_opacity, float world_bound, float sample_div, int32_t size_test,
                   int gated, float gate_opacity, void* tmp, size_t tmp_bytes, void* stream) {
  if (!scaling || !opacity || !xyz_gradient_accum || !denom || !tmp) return GS_E_NULL;
  if (P < 1 || P > (int32_t)DN_ROW_MASK || N < 1 || N > GS_DENSIFY_MAX_N) return GS_E_SHAPE;
  if (tmp_bytes < dn_tmp_bytes((size_t)P)) return GS_E_SCRATCH;
  const DensifyTmp t = dn_tmp_view(tmp, (size_t)P);
  const int nb = (int)dn_blocks((size_t)P);
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(densify_plan_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, scaling, opacity, xyz_gradient_accum, denom, P, max_grad,
                     scale_bound, min_opacity, world_bound, sample_div, size_test ? 1 : 0, gated, gate_opacity, t.flags, t.counts);
  hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(DN_BLOCK), 0, s, t.counts, nb, t.prefix, t.totals);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_densify_plan(const float* scaling, const float* opacity, const float* xyz_gradient_accum, const float* denom, int32_t P,
                    int32_t N, float max_grad, float scale_bound, float min_opacity, float world_bound, float sample_div,
                    int32_t size_test, void* tmp, size_t tmp_bytes, void* stream) {
  return dn_plan(scaling, opacity, xyz_gradient_accum, denom, P, N, max_grad, scale_bound, min_opacity, world_bound, sample_div,
                 size_test, 0, 0.0f, tmp, tmp_bytes, stream);
}

int gs_densify_plan_gated(const float* scaling, const float* opacity, const float* xyz_gradient_accum, const float* denom, int32_t P,
                          int32_t N, float max_grad, float scale_bound, float min_opacity, float world_bound, float sample_div,
                          int32_t size_test, float gate_opacity, void* tmp, size_t tmp_bytes, void* stream) {
  return dn_plan(scaling, opacity, xyz_gradient_accum, denom, P, N, max_grad, scale_bound, min_opacity, world_bound, sample_div,
                 size_test, 1, gate_opacity, tmp, tmp_bytes, stream);
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
  const int32_t special[2] = {xyz_field, scaling_field};
  return dn_gather(perm, table, nullptr, new_xyz, P2, old_flat, old_exp_avg, old_exp_avg_sq, P, new_flat, new_exp_avg, new_exp_avg_sq,
                   nfields, widths, special, sample_div, stream);
}

size_t gs_prune_tmp_bytes(int32_t P) { return P < 1 ? 0 : pr_tmp_bytes((size_t)P); }

int gs_prune_plan(const uint8_t* mask, int32_t P, void* tmp, size_t tmp_bytes, void* stream) {
  if (!mask || !tmp) return GS_E_NULL;
  if (P < 1 || P > (int32_t)DN_ROW_MASK) return GS_E_SHAPE;
  if (tmp_bytes < pr_tmp_bytes((size_t)P)) return GS_E_SCRATCH;
  const PruneTmp t = pr_tmp_view(tmp, (size_t)P);
  const int nb = (int)dn_blocks((size_t)P);
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(prune_plan_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, mask, P, t.counts);
  hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(DN_BLOCK), 0, s, t.counts, nb, t.prefix, t.totals);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_prune_emit(const void* tmp, size_t tmp_bytes, const uint8_t* mask, const float* xyz, int32_t P, int32_t P2, uint32_t* table,
                  float* new_xyz, const float* xyz_gradient_accum, const float* denom, const float* max_radii2D,
                  float* new_xyz_gradient_accum, float* new_denom, float* new_max_radii2D, void* stream) {
  if (!tmp || !mask || !xyz || !table || !new_xyz || !xyz_gradient_accum || !denom || !max_radii2D || !new_xyz_gradient_accum ||
      !new_denom || !new_max_radii2D)
    return GS_E_NULL;
  if (P < 1 || P > (int32_t)DN_ROW_MASK || P2 < 1 || P2 > P) return GS_E_SHAPE;
  if (tmp_bytes < pr_tmp_bytes((size_t)P)) return GS_E_SCRATCH;
  const PruneTmp t = pr_tmp_view(const_cast<void*>(tmp), (size_t)P);
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(prune_emit_kernel, dim3((unsigned)dn_blocks((size_t)P)), dim3(DN_BLOCK), 0, s, mask, t.prefix, t.totals, xyz,
                     xyz_gradient_accum, denom, max_radii2D, P, (uint32_t)P2, table, new_xyz, new_xyz_gradient_accum, new_denom,
                     new_max_radii2D);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}
}

// ==================================================================================================================
// FSGS's densification (FSGS/scene/gaussian_model.py:424-491; host form and arbiter: GaussianModelLite.densify_and_prune_fsgs).
// It cannot be planned in one pass over the source rows: the split selection ORs in a distance rule whose kNN runs over
// [rows | clones], and proximity's kNN runs over the set AFTER the split, samples included.  So:
//
//   plan       per source row: clone, grad-split, prune and "wider than the extent" flags (self and sample), the clones' ranks,
//              the centres of [P rows | clones]                                              -> read-back 1: n_clone
//   (kNN #1)   gs_knn_mean_dist2_idx on those centres
//   merge      ORs the distance rule into the split flag; counts of what the intermediate set holds and of what survives
//                                                                                           -> read-back 2: n_split, n_stay, keeps
//   emit       Q = [rows that stay | clones | sample block 0 .. N-1], NO prune applied: source table and centres
//   (kNN #2)   with indices, on Q's centres
//   prox plan  per Q row: kept by the final prune?  selected by proximity?  which of its three new rows are kept?
//                                                                                           -> read-back 3: S, kept new rows
//   final      the final table in the reference's order [kept Q rows | kept proximity rows]: source row and kind, the kind of a
//              proximity row's neighbour in a side array, the centres (midpoints with the TILED selected rows)
//   (codes)    morton_codes_kernel, for the spatial order
//   gather     the one HBM pass, as above, plus the proximity rows
//
// A clone is never split (it is small; both split rules need it large while percent_dense <= 1, which the host checks), so the
// P + n_clone rows of kNN #1 need no table: row i < P is source i.  Every decision of a Q row or a proximity row is one of its
// SOURCE's flags: a clone carries its source's raw scaling and opacity, the samples share exp(log(exp(s) / (0.8 N))), and a
// proximity row takes its neighbour's raw scaling and opacity.
// ==================================================================================================================
#define FS_TOTAL_WORDS 64   // uint32 words in front of the scratch: what the host reads
#define FS_MERGE_AT 8       // ... the merge's five totals start here, the plan's (or the proximity plan's) at 0
#define FS_KIND_MAX GS_DENSIFY_PROXIMITY
static_assert(GS_DENSIFY_FSGS_MERGE_AT == FS_MERGE_AT, "the header tells the host where the merge's totals are");

struct FsgsTmp {
  uint32_t* totals;                                     // [FS_TOTAL_WORDS]
  uint8_t* flags;                                       // [P]
  uint32_t *counts_a, *prefix_a, *counts_b, *prefix_b;  // [nb][DN_NC] each
};
static inline size_t fs_tmp_bytes(size_t P) { return 4 * FS_TOTAL_WORDS + gs_align(P) + 4 * gs_align(4 * DN_NC * dn_blocks(P)); }
static inline FsgsTmp fs_tmp_view(void* buf, size_t P) {
  char* p = (char*)buf;
  const size_t blk = gs_align(4 * DN_NC * dn_blocks(P));
  FsgsTmp t;
  t.totals = (uint32_t*)p; p += 4 * FS_TOTAL_WORDS;
  t.flags = (uint8_t*)p; p += gs_align(P);
  t.counts_a = (uint32_t*)p; p += blk;
  t.prefix_a = (uint32_t*)p; p += blk;
  t.counts_b = (uint32_t*)p; p += blk;
  t.prefix_b = (uint32_t*)p;
  return t;
}

static __device__ __forceinline__ bool fs_pruned(unsigned f, uint32_t kind, int prune_on) {
  return prune_on && (f & (kind == GS_DENSIFY_SAMPLE ? GS_DENSIFY_FSGS_PRUNE_SAMPLE : GS_DENSIFY_FSGS_PRUNE_SELF)) != 0;
}
static __device__ __forceinline__ bool fs_wide(unsigned f, uint32_t kind) {
  return (f & (kind == GS_DENSIFY_SAMPLE ? GS_DENSIFY_FSGS_WIDE_SAMPLE : GS_DENSIFY_FSGS_WIDE_SELF)) != 0;
}

__global__ void __launch_bounds__(DN_BLOCK) fsgs_plan_kernel(const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                            const float* __restrict__ accum, const float* __restrict__ denom, int P,
                                                            float max_grad, float scale_bound, float min_opacity, float world_bound,
                                                            float extent_bound, float sample_div, int size_test,
                                                            uint8_t* __restrict__ flags, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = i < (size_t)P;
  unsigned f = 0;
  if (in) {
    const RowMeasures m = dn_row_measures(scaling, opacity, accum, denom, i, scale_bound, min_opacity, sample_div);
    if (fabsf(m.g) >= max_grad && m.small) f |= GS_DENSIFY_FSGS_CLONE;
    if (m.g >= max_grad && m.max_scale > scale_bound) f |= GS_DENSIFY_FSGS_GRAD_SPLIT;
    if (m.faint || (size_test && m.max_scale > world_bound)) f |= GS_DENSIFY_FSGS_PRUNE_SELF;
    if (m.faint || (size_test && m.max_sample > world_bound)) f |= GS_DENSIFY_FSGS_PRUNE_SAMPLE;
    if (m.max_scale > extent_bound) f |= GS_DENSIFY_FSGS_WIDE_SELF;
    if (m.max_sample > extent_bound) f |= GS_DENSIFY_FSGS_WIDE_SAMPLE;
    flags[i] = (uint8_t)f;
  }
  const bool c[1] = {in && (f & GS_DENSIFY_FSGS_CLONE)};
  uint32_t rank[1], total[1];
  dn_block_ranks<1>(c, s_cnt, rank, total);
  if (threadIdx.x < DN_NC) counts[(size_t)blockIdx.x * DN_NC + threadIdx.x] = threadIdx.x == 0 ? total[0] : 0u;
}

// the point set of kNN #1: the P centres, then the clones' (copies of their sources') by ascending source row
__global__ void __launch_bounds__(DN_BLOCK) fsgs_centres_kernel(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ prefix_a,
                                                               const float* __restrict__ xyz, int P, float* __restrict__ xyz1) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = i < (size_t)P;
  const bool c[1] = {in && (flags[i] & GS_DENSIFY_FSGS_CLONE)};
  uint32_t rank[1], total[1];
  dn_block_ranks<1>(c, s_cnt, rank, total);
  if (!in) return;
  const float x0 = xyz[3 * i], x1 = xyz[3 * i + 1], x2 = xyz[3 * i + 2];
  xyz1[3 * i] = x0; xyz1[3 * i + 1] = x1; xyz1[3 * i + 2] = x2;
  if (c[0]) {
    const size_t j = (size_t)P + prefix_a[(size_t)blockIdx.x * DN_NC] + rank[0];
    if (j < 2 * (size_t)P) { xyz1[3 * j] = x0; xyz1[3 * j + 1] = x1; xyz1[3 * j + 2] = x2; }
  }
}

// what a source row contributes to the intermediate set Q and to the final prune, from its merged flag byte:
// [0] it is split, [1] it stays in Q, [2] ... and survives the final prune, [3] its clone survives, [4] its samples survive
static __device__ __forceinline__ void fs_merge_preds(unsigned f, bool in, int prune_on, bool* c) {
  const bool split = in && (f & GS_DENSIFY_FSGS_SPLIT);
  const bool stay = in && (!split || !prune_on);
  const bool self_ok = !(prune_on && (f & GS_DENSIFY_FSGS_PRUNE_SELF));
  c[0] = split;
  c[1] = stay;
  c[2] = stay && self_ok;
  c[3] = in && (f & GS_DENSIFY_FSGS_CLONE) && self_ok;
  c[4] = split && !(prune_on && (f & GS_DENSIFY_FSGS_PRUNE_SAMPLE));
}

__global__ void __launch_bounds__(DN_BLOCK) fsgs_merge_kernel(uint8_t* __restrict__ flags, const float* __restrict__ dist, int P,
                                                             float dist_bound, int prune_on, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = i < (size_t)P;
  unsigned f = 0;
  if (in) {
    f = flags[i] & ~(unsigned)GS_DENSIFY_FSGS_SPLIT;
    if ((f & GS_DENSIFY_FSGS_GRAD_SPLIT) || (dist[i] > dist_bound && (f & GS_DENSIFY_FSGS_WIDE_SELF))) f |= GS_DENSIFY_FSGS_SPLIT;
    flags[i] = (uint8_t)f;
  }
  bool c[DN_NC];
  fs_merge_preds(f, in, prune_on, c);
  uint32_t rank[DN_NC], total[DN_NC];
  dn_block_ranks<DN_NC>(c, s_cnt, rank, total);
  if (threadIdx.x < DN_NC) counts[(size_t)blockIdx.x * DN_NC + threadIdx.x] = total[threadIdx.x];
}

struct FsgsEmitCounts {
  uint32_t n_clone, n_split, n_stay;
};

__global__ void __launch_bounds__(DN_BLOCK) fsgs_emit_kernel(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ prefix_a,
                                                            const uint32_t* __restrict__ prefix_b, const uint32_t* __restrict__ totals,
                                                            const float* __restrict__ xyz, const float* __restrict__ scaling,
                                                            const float* __restrict__ rotation, const float* __restrict__ noise, int P,
                                                            int N, FsgsEmitCounts n, uint32_t nQ, int prune_on,
                                                            uint32_t* __restrict__ table, float* __restrict__ xyz_q) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  // the counts the host sized Q with must be the plan's and the merge's (uniform over the grid: nobody reaches the barrier)
  if (totals[0] != n.n_clone || totals[FS_MERGE_AT] != n.n_split || totals[FS_MERGE_AT + 1] != n.n_stay) return;
  const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = i < (size_t)P;
  const unsigned f = in ? flags[i] : 0u;
  bool m[DN_NC];
  fs_merge_preds(f, in, prune_on, m);
  const bool c[3] = {m[1], in && (f & GS_DENSIFY_FSGS_CLONE), m[0]};   // stays, cloned, split
  uint32_t rank[3], total[3];
  dn_block_ranks<3>(c, s_cnt, rank, total);
  if (!in) return;
  rank[0] += prefix_b[(size_t)blockIdx.x * DN_NC + 1];
  rank[1] += prefix_a[(size_t)blockIdx.x * DN_NC];
  rank[2] += prefix_b[(size_t)blockIdx.x * DN_NC];
  const float x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  if (c[0]) dn_put_row(table, xyz_q, rank[0], nQ, i, GS_DENSIFY_SURVIVOR, x);
  if (c[1]) dn_put_row(table, xyz_q, n.n_stay + rank[1], nQ, i, GS_DENSIFY_CLONED, x);
  if (c[2])
    dn_put_samples(scaling, rotation, noise, i, x, rank[2], n.n_split, N, n.n_stay + n.n_clone + rank[2], n.n_split, nQ, table, xyz_q);
}

#define FS_Q_KEEP 1u
#define FS_Q_SEL 2u
#define FS_Q_CHILD_SHIFT 2

// per row j of Q: is it kept by the final prune, is it selected by proximity, and which of its three new rows (one per
// neighbour; a new row carries the neighbour's raw scaling and opacity, so the neighbour's prune decision) are kept
__global__ void __launch_bounds__(DN_BLOCK) fsgs_prox_plan_kernel(const uint8_t* __restrict__ flags, uint32_t P,
                                                                 const uint32_t* __restrict__ table_q, uint32_t nQ,
                                                                 const float* __restrict__ dist, const int32_t* __restrict__ nearest,
                                                                 float prox_bound, int prune_on, uint8_t* __restrict__ qflags,
                                                                 uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  const size_t j = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = j < (size_t)nQ;
  bool c[DN_NC] = {false, false, false, false, false};
  if (in) {
    const uint32_t ent = table_q[j], src = ent & DN_ROW_MASK, kind = ent >> DN_KIND_SHIFT;
    if (src < P && kind <= GS_DENSIFY_SAMPLE) {
      const unsigned f = flags[src];
      c[0] = !fs_pruned(f, kind, prune_on);
      c[1] = dist != nullptr && dist[j] > prox_bound && fs_wide(f, kind);
      if (c[1]) {
#pragma unroll
        for (int t = 0; t < 3; t++) {
          const int32_t nb = nearest[3 * j + t];
          if (nb < 0 || (uint32_t)nb >= nQ) continue;
          const uint32_t e2 = table_q[nb], s2 = e2 & DN_ROW_MASK, k2 = e2 >> DN_KIND_SHIFT;
          if (s2 < P && k2 <= GS_DENSIFY_SAMPLE) c[2 + t] = !fs_pruned(flags[s2], k2, prune_on);
        }
      }
    }
    qflags[j] = (uint8_t)((c[0] ? FS_Q_KEEP : 0u) | (c[1] ? FS_Q_SEL : 0u) | ((unsigned)c[2] << FS_Q_CHILD_SHIFT) |
                          ((unsigned)c[3] << (FS_Q_CHILD_SHIFT + 1)) | ((unsigned)c[4] << (FS_Q_CHILD_SHIFT + 2)));
  }
  uint32_t rank[DN_NC], total[DN_NC];
  dn_block_ranks<DN_NC>(c, s_cnt, rank, total);
  if (threadIdx.x < DN_NC) counts[(size_t)blockIdx.x * DN_NC + threadIdx.x] = total[threadIdx.x];
}

struct FsgsFinalCounts {
  uint32_t n_keep_q, S, n_keep_prox;
};
static __device__ __forceinline__ bool fs_final_counts_ok(const uint32_t* totals, FsgsFinalCounts n) {
  return totals[0] == n.n_keep_q && totals[1] == n.S && totals[2] + totals[3] + totals[4] == n.n_keep_prox;
}

// the kept rows of Q into the final table, in Q's order; the selected rows compacted (sel_rows[r] = the r-th selected row of Q)
// with the position of their first kept new row among all kept new rows
__global__ void __launch_bounds__(DN_BLOCK) fsgs_final_rows_kernel(const uint8_t* __restrict__ qflags, const uint32_t* __restrict__ prefix,
                                                                  const uint32_t* __restrict__ totals,
                                                                  const uint32_t* __restrict__ table_q, const float* __restrict__ xyz_q,
                                                                  uint32_t nQ, FsgsFinalCounts n, uint32_t P2,
                                                                  uint32_t* __restrict__ table, uint8_t* __restrict__ nb_kind,
                                                                  float* __restrict__ new_xyz, uint32_t* __restrict__ sel_rows,
                                                                  uint32_t* __restrict__ prox_base) {
  __shared__ uint32_t s_cnt[DN_WAVES][DN_NC];
  if (!fs_final_counts_ok(totals, n)) return;
  const size_t j = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  const bool in = j < (size_t)nQ;
  const unsigned q = in ? qflags[j] : 0u;
  const bool c[DN_NC] = {(q & FS_Q_KEEP) != 0, (q & FS_Q_SEL) != 0, ((q >> FS_Q_CHILD_SHIFT) & 1u) != 0,
                         ((q >> (FS_Q_CHILD_SHIFT + 1)) & 1u) != 0, ((q >> (FS_Q_CHILD_SHIFT + 2)) & 1u) != 0};
  uint32_t rank[DN_NC], total[DN_NC];
  dn_block_ranks<DN_NC>(c, s_cnt, rank, total);
  if (!in) return;
#pragma unroll
  for (int k = 0; k < DN_NC; k++) rank[k] += prefix[(size_t)blockIdx.x * DN_NC + k];
  if (c[0] && rank[0] < P2) {
    const size_t o = rank[0];
    table[o] = table_q[j];
    nb_kind[o] = 0;
    new_xyz[3 * o] = xyz_q[3 * j]; new_xyz[3 * o + 1] = xyz_q[3 * j + 1]; new_xyz[3 * o + 2] = xyz_q[3 * j + 2];
  }
  if (c[1] && rank[1] < n.S) {
    sel_rows[rank[1]] = (uint32_t)j;
    prox_base[rank[1]] = rank[2] + rank[3] + rank[4];   // kept new rows of the selected rows in front of this one
  }
}

// new row m of the reference's flattened order: neighbour m of the flattened [S, 3] lists (selected row m / 3, neighbour m % 3),
// midway between that neighbour and selected row m % S - the reference TILES the selected rows
__global__ void __launch_bounds__(DN_BLOCK) fsgs_final_prox_kernel(const uint8_t* __restrict__ qflags, const uint32_t* __restrict__ totals,
                                                                  const uint32_t* __restrict__ table_q, const float* __restrict__ xyz_q,
                                                                  const int32_t* __restrict__ nearest, uint32_t nQ, FsgsFinalCounts n,
                                                                  uint32_t P2, const uint32_t* __restrict__ sel_rows,
                                                                  const uint32_t* __restrict__ prox_base, uint32_t* __restrict__ table,
                                                                  uint8_t* __restrict__ nb_kind, float* __restrict__ new_xyz) {
  if (!fs_final_counts_ok(totals, n)) return;
  const size_t m = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
  if (m >= 3 * (size_t)n.S) return;
  const uint32_t r = (uint32_t)(m / 3), t = (uint32_t)(m - 3 * (size_t)r);
  const uint32_t j = sel_rows[r], partner = sel_rows[m % n.S];
  if (j >= nQ || partner >= nQ) return;
  const unsigned kept = ((unsigned)qflags[j] >> FS_Q_CHILD_SHIFT) & 7u;
  if (!((kept >> t) & 1u)) return;
  const size_t o = (size_t)n.n_keep_q + prox_base[r] + (uint32_t)__popc(kept & ((1u << t) - 1u));
  const int32_t nb = nearest[3 * (size_t)j + t];
  if (o >= P2 || nb < 0 || (uint32_t)nb >= nQ) return;
  const uint32_t e2 = table_q[nb];
  table[o] = (e2 & DN_ROW_MASK) | ((uint32_t)GS_DENSIFY_PROXIMITY << DN_KIND_SHIFT);
  nb_kind[o] = (uint8_t)(e2 >> DN_KIND_SHIFT);
#pragma unroll
  for (int a = 0; a < 3; a++) new_xyz[3 * o + a] = (xyz_q[3 * (size_t)partner + a] + xyz_q[3 * (size_t)nb + a]) / 2.0f;
}

extern "C" {

size_t gs_densify_fsgs_tmp_bytes(int32_t P) { return P < 1 ? 0 : fs_tmp_bytes((size_t)P); }

int gs_densify_fsgs_plan(const float* scaling, const float* opacity, const float* xyz_gradient_accum, const float* denom,
                         const float* xyz, int32_t P, int32_t N, float max_grad, float scale_bound, float min_opacity,
                         float world_bound, float extent_bound, float sample_div, int32_t size_test, void* tmp, size_t tmp_bytes,
                         float* xyz1, void* stream) {
  if (!scaling || !opacity || !xyz_gradient_accum || !denom || !xyz || !tmp || !xyz1) return GS_E_NULL;
  if (P < 1 || P > (int32_t)(DN_ROW_MASK / 2) || N < 1 || N > GS_DENSIFY_MAX_N) return GS_E_SHAPE;
  if (tmp_bytes < fs_tmp_bytes((size_t)P)) return GS_E_SCRATCH;
  const FsgsTmp t = fs_tmp_view(tmp, (size_t)P);
  const int nb = (int)dn_blocks((size_t)P);
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(fsgs_plan_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, scaling, opacity, xyz_gradient_accum, denom, P, max_grad,
                     scale_bound, min_opacity, world_bound, extent_bound, sample_div, size_test ? 1 : 0, t.flags, t.counts_a);
  hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(DN_BLOCK), 0, s, t.counts_a, nb, t.prefix_a, t.totals);
  hipLaunchKernelGGL(fsgs_centres_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, t.flags, t.prefix_a, xyz, P, xyz1);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_densify_fsgs_merge(void* tmp, size_t tmp_bytes, const float* dist, int32_t P, float dist_bound, int32_t prune_on,
                          void* stream) {
  if (!tmp || !dist) return GS_E_NULL;
  if (P < 1 || P > (int32_t)(DN_ROW_MASK / 2)) return GS_E_SHAPE;
  if (tmp_bytes < fs_tmp_bytes((size_t)P)) return GS_E_SCRATCH;
  const FsgsTmp t = fs_tmp_view(tmp, (size_t)P);
  const int nb = (int)dn_blocks((size_t)P);
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(fsgs_merge_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, t.flags, dist, P, dist_bound, prune_on ? 1 : 0, t.counts_b);
  hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(DN_BLOCK), 0, s, t.counts_b, nb, t.prefix_b, t.totals + FS_MERGE_AT);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_densify_fsgs_emit(const void* tmp, size_t tmp_bytes, const float* xyz, const float* scaling, const float* rotation,
                         const float* noise, int32_t P, int32_t N, int32_t n_clone, int32_t n_split, int32_t n_stay, int32_t nQ,
                         int32_t prune_on, uint32_t* table_q, float* xyz_q, void* stream) {
  if (!tmp || !xyz || !scaling || !rotation || !table_q || !xyz_q) return GS_E_NULL;
  if (P < 1 || P > (int32_t)(DN_ROW_MASK / 2) || N < 1 || N > GS_DENSIFY_MAX_N) return GS_E_SHAPE;
  if (n_clone < 0 || n_split < 0 || n_stay < 0 || n_clone > P || n_split > P || n_stay > P ||
      n_stay != (prune_on ? P - n_split : P) || nQ < 1 || (int64_t)n_stay + n_clone + (int64_t)N * n_split != nQ)
    return GS_E_SHAPE;
  if (n_split > 0 && !noise) return GS_E_NULL;
  if (tmp_bytes < fs_tmp_bytes((size_t)P)) return GS_E_SCRATCH;
  const FsgsTmp t = fs_tmp_view(const_cast<void*>(tmp), (size_t)P);
  FsgsEmitCounts n;
  n.n_clone = (uint32_t)n_clone; n.n_split = (uint32_t)n_split; n.n_stay = (uint32_t)n_stay;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(fsgs_emit_kernel, dim3((unsigned)dn_blocks((size_t)P)), dim3(DN_BLOCK), 0, s, t.flags, t.prefix_a, t.prefix_b,
                     t.totals, xyz, scaling, rotation, noise, P, N, n, (uint32_t)nQ, prune_on ? 1 : 0, table_q, xyz_q);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_densify_fsgs_prox_plan(const void* tmp, size_t tmp_bytes, int32_t P, const uint32_t* table_q, int32_t nQ, const float* dist,
                              const int32_t* nearest, float prox_bound, int32_t prune_on, void* tmp_q, size_t tmp_q_bytes,
                              void* stream) {
  if (!tmp || !table_q || !tmp_q) return GS_E_NULL;
  if ((dist == nullptr) != (nearest == nullptr)) return GS_E_NULL;
  if (P < 1 || P > (int32_t)(DN_ROW_MASK / 2) || nQ < 1 || nQ > (int32_t)DN_ROW_MASK) return GS_E_SHAPE;
  if (tmp_bytes < fs_tmp_bytes((size_t)P) || tmp_q_bytes < fs_tmp_bytes((size_t)nQ)) return GS_E_SCRATCH;
  const FsgsTmp t = fs_tmp_view(const_cast<void*>(tmp), (size_t)P);
  const FsgsTmp q = fs_tmp_view(tmp_q, (size_t)nQ);
  const int nb = (int)dn_blocks((size_t)nQ);
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(fsgs_prox_plan_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, t.flags, (uint32_t)P, table_q, (uint32_t)nQ, dist, nearest,
                     prox_bound, prune_on ? 1 : 0, q.flags, q.counts_a);
  hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(DN_BLOCK), 0, s, q.counts_a, nb, q.prefix_a, q.totals);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_densify_fsgs_final(const void* tmp_q, size_t tmp_q_bytes, const uint32_t* table_q, const float* xyz_q, const int32_t* nearest,
                          int32_t nQ, int32_t n_keep_q, int32_t S, int32_t n_keep_prox, int32_t P2, uint32_t* table,
                          uint8_t* nb_kind, float* new_xyz, uint32_t* sel_rows, uint32_t* prox_base, void* stream) {
  if (!tmp_q || !table_q || !xyz_q || !table || !nb_kind || !new_xyz) return GS_E_NULL;
  if (nQ < 1 || nQ > (int32_t)DN_ROW_MASK || n_keep_q < 0 || n_keep_q > nQ || S < 0 || S > nQ || n_keep_prox < 0 ||
      (int64_t)n_keep_prox > 3 * (int64_t)S || P2 < 1 || (int64_t)n_keep_q + n_keep_prox != P2 || P2 > (int32_t)DN_ROW_MASK)
    return GS_E_SHAPE;
  if (S > 0 && (!nearest || !sel_rows || !prox_base)) return GS_E_NULL;
  if (tmp_q_bytes < fs_tmp_bytes((size_t)nQ)) return GS_E_SCRATCH;
  const FsgsTmp q = fs_tmp_view(const_cast<void*>(tmp_q), (size_t)nQ);
  FsgsFinalCounts n;
  n.n_keep_q = (uint32_t)n_keep_q; n.S = (uint32_t)S; n.n_keep_prox = (uint32_t)n_keep_prox;
  hipStream_t s = (hipStream_t)stream;
  GS_PROF(ST_MODEL, s);
  hipLaunchKernelGGL(fsgs_final_rows_kernel, dim3((unsigned)dn_blocks((size_t)nQ)), dim3(DN_BLOCK), 0, s, q.flags, q.prefix_a, q.totals,
                     table_q, xyz_q, (uint32_t)nQ, n, (uint32_t)P2, table, nb_kind, new_xyz, sel_rows, prox_base);
  if (S > 0)
    hipLaunchKernelGGL(fsgs_final_prox_kernel, dim3((unsigned)dn_blocks(3 * (size_t)S)), dim3(DN_BLOCK), 0, s, q.flags, q.totals, table_q,
                       xyz_q, nearest, (uint32_t)nQ, n, (uint32_t)P2, sel_rows, prox_base, table, nb_kind, new_xyz);
  GS_LAUNCH_CHECK(s, 0);
  return GS_OK;
}

int gs_densify_fsgs_gather(const int64_t* perm, const uint32_t* table, const uint8_t* nb_kind, const float* new_xyz, int32_t P2,
                           const float* old_flat, const float* old_exp_avg, const float* old_exp_avg_sq, int32_t P, float* new_flat,
                           float* new_exp_avg, float* new_exp_avg_sq, int32_t nfields, const int32_t* widths, int32_t xyz_field,
                           int32_t scaling_field, int32_t opacity_field, int32_t rotation_field, float sample_div, void* stream) {
  if (!table || !nb_kind || !new_xyz || !old_flat || !old_exp_avg || !old_exp_avg_sq || !new_flat || !new_exp_avg || !new_exp_avg_sq ||
      !widths)
    return GS_E_NULL;
  const int32_t special[4] = {xyz_field, scaling_field, opacity_field, rotation_field};
  return dn_gather(perm, table, nb_kind, new_xyz, P2, old_flat, old_exp_avg, old_exp_avg_sq, P, new_flat, new_exp_avg, new_exp_avg_sq,
                   nfields, widths, special, sample_div, stream);
}
}
