// gs_depth_pass.hip - the depth-only pass: depth = sum z_i alpha_i T_i and alpha = sum alpha_i T_i of a view, and the
// gradients of those two images with respect to the means and / or the opacities.  Nothing else.
//
// DNGaussian renders every training view three times; two of the three ("hard depth": opacity 0.95 everywhere, gradient to
// the means only; "soft depth": gradient to the opacities only) blend a constant colour 1 whose image nobody reads
// (DNGaussian/gaussian_renderer/__init__.py:128-269).  Served by the general FSGS-generation kernels they blend three channels
// of ones, keep twelve sums per (tile, Gaussian) in the backward and run the float64 covariance chain down to scales and
// quaternions for gradients that are thrown away.  The kernels here are those kernels with everything taken out that the two
// passes do not need:
//   depth_fwd_wave_kernel   = render_fwd_wave_kernel<false, FSGS, CULL> without colour, background, reached marking and depth
//                             limits.  The per-pixel arithmetic of D, X and T is the general kernel's, operation for operation:
//                             the two images are the general path's bit for bit (tests/test_gpu_depth_pass.py asserts it).
//   depth_bwd_wave_kernel   = render_bwd_wave_kernel<true, true, FSGS> with the colour cotangent identically zero: no colour
//                             sums, no background term; six sums per (tile, Gaussian) for the means, one for the opacities.
//   depth_point_bwd_kernel  = the per-Gaussian tail, one thread per Gaussian: cov2D backward (float64, mean part only),
//                             projection backward, the depth term; no cov3D backward, no SH, no colour.
//   depth_point_step_kernel = that tail with Adam on the ONE tensor a DNGaussian depth leg steps (the means, or the raw
//                             opacities through the sigmoid's backward) in place of the gradient stores
//                             (gs_depth_backward_step).
// Same tile mapping, lists, splat records, alpha rules and float64 gradient rows as the general path (gs_render_fwd_wave.hip,
// gs_render_bwd_wave.hip, gs_backward_math.h).
//
// The file is built without fp contraction (the per-Gaussian tail restates gs_preprocess_bwd.hip's fp32 roundings); the two
// blend kernels contract by pragma, as the general blend kernels do by flag.
#include "gs_blend.h"
#include "gs_common.h"
#include "gs_backward_math.h"

#define WB 64  // batch = one list entry per lane

// ------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------
template <bool CULL>
__global__ void __launch_bounds__(64) depth_fwd_wave_kernel(const uint2* __restrict__ ranges,
                                                            const uint32_t* __restrict__ point_list, int W, int H, int grid_x,
                                                            const Splat* __restrict__ splat, float* __restrict__ final_T,
                                                            uint32_t* __restrict__ n_contrib, uint32_t* __restrict__ tile_work,
                                                            float* __restrict__ stop_depth, float* __restrict__ out_depth,
                                                            float* __restrict__ out_alpha) {
#pragma clang fp contract(fast)
  __shared__ float4 s_a[WB];  // x, y, view depth, cull extent y (CULL) / view depth (!CULL)
  __shared__ float4 s_c[WB];  // conic, opacity
  __shared__ float s_ex[CULL ? WB : 1];  // cull extent x

  // the general kernel's XCD-aware mapping (consecutive workgroup ids go round-robin over the 8 XCDs)
  const int n_tiles = grid_x * ((H + TILE_Y - 1) / TILE_Y);
  const int per_xcd = (int)(gridDim.x >> 3);  // the grid is padded to a multiple of 8 workgroups
  const int tile = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if (tile >= n_tiles) return;
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const int lane = threadIdx.x;
  const int px0 = tile_x * TILE_X + (lane & 7), py0 = tile_y * TILE_Y + (lane >> 3);
  const float pixfx0 = (float)px0, pixfy0 = (float)py0;
  const float tile_fx0 = (float)(tile_x * TILE_X), tile_fy0 = (float)(tile_y * TILE_Y);

  const uint2 range = ranges[tile];
  const int n = (int)(range.y - range.x);
  const int rounds = (n + WB - 1) / WB;

  // T[s] > 0: alive; T[s] < 0: done, |T[s]| is the final transmittance ("done" in the sign bit, as the general kernel)
  float T[4], D[4], X[4];
  uint32_t last_contributor[4];
  bool inside[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int px = px0 + (s & 1) * 8, py = py0 + (s >> 1) * 8;
    inside[s] = px < W && py < H;
    T[s] = inside[s] ? 1.0f : -1.0f;
    D[s] = X[s] = 0.f;
    last_contributor[s] = 0;
  }

  float stop_z = __builtin_inff();  // view depth of the entry at which the tile's last pixel saturated
  float4 ra, rc;
  ra = rc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (lane < n) {
    const float4* rec = reinterpret_cast<const float4*>(&splat[point_list[range.x + lane]]);
    ra = rec[0]; rc = rec[1];
  }
  for (int i = 0; i < rounds; i++) {
    if (!__any(fmaxf(fmaxf(T[0], T[1]), fmaxf(T[2], T[3])) > 0.f)) break;  // the whole tile is done
    __syncthreads();  // single wave: previous batch fully consumed
    s_a[lane] = make_float4(ra.x, ra.y, ra.z, ra.z);
    s_c[lane] = blend_stage_conic(rc);  // (qa, qb, qc, opacity), see gs_blend.h
    if (CULL) {  // the general kernel's exact-safe tile cull, same expressions
      const float det = rc.x * rc.z - rc.y * rc.y;
      const float L2 = 2.0f * __logf(255.0f * 1.0001f * fmaxf(rc.w, 1e-20f));  // < 0: opacity below 1/255, never blends
      const bool ok = det > 0.f && L2 >= 0.f;
      const float ex = ok ? sqrtf(L2 * rc.z / det) * 1.02f + 1.0f : (L2 >= 0.f ? 3.0e38f : -1.0f);
      const float ey = ok ? sqrtf(L2 * rc.x / det) * 1.02f + 1.0f : (L2 >= 0.f ? 3.0e38f : -1.0f);
      s_ex[lane] = ex;
      s_a[lane].w = ey;
    }
    __syncthreads();
    {
      const int nxt = (i + 1) * WB + lane;
      if (nxt < n) {
        const float4* rec = reinterpret_cast<const float4*>(&splat[point_list[range.x + nxt]]);
        ra = rec[0]; rc = rec[1];
      }
    }
    const int cnt = min(WB, n - i * WB);
    bool running = true;  // (wave-uniform; the outer loop's own check ends the tile when the batch loop has been left)
    for (int j = 0; j < cnt && running; j++) {
      const uint32_t contributor = (uint32_t)(i * WB + j + 1);
      const float4 a = s_a[j];
      if (CULL) {  // wave-uniform: distance from the centre to the tile's pixel range, per axis
        const float ddx = fmaxf(fmaxf(tile_fx0 - a.x, a.x - (tile_fx0 + 15.0f)), 0.f);
        const float ddy = fmaxf(fmaxf(tile_fy0 - a.y, a.y - (tile_fy0 + 15.0f)), 0.f);
        if (ddx > s_ex[j] || ddy > a.w) continue;
      }
      const float4 co = s_c[j];
      float alpha[4];
      bool hit[4];
      unsigned long long hmask = 0ull;  // lane masks stay scalar
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const float dx = a.x - (pixfx0 + (float)((s & 1) * 8));
        const float dy = a.y - (pixfy0 + (float)((s >> 1) * 8));
        const float p2 = blend_power2(co, dx, dy);
        alpha[s] = fminf(0.99f, co.w * blend_exp2(p2));
        const bool c1 = p2 <= 0.0f, c2 = alpha[s] >= 1.0f / 255.0f;
        const bool alive = T[s] > 0.f;
        hit[s] = alive && c1 && c2;
        hmask |= __ballot(c1) & __ballot(c2) & __ballot(alive);
      }
      if (hmask == 0ull) continue;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        if (hit[s]) {
          const float test_T = T[s] * (1 - alpha[s]);
          const bool sat = test_T < 0.0001f;          // saturates here: this entry is NOT blended, the pixel is done
          const float w = sat ? 0.f : alpha[s] * T[s];
          D[s] += a.z * w;
          X[s] += w;
          T[s] = sat ? -T[s] : test_T;
          last_contributor[s] = sat ? last_contributor[s] : contributor;
        }
      }
      running = __any(fmaxf(fmaxf(T[0], T[1]), fmaxf(T[2], T[3])) > 0.f);
      if (!running && !CULL) stop_z = a.w;
    }
  }
  if (lane == 0) stop_depth[tile] = stop_z;
  {
    // what the backward blend of this tile will cost: it walks the list back from the tile's deepest last contributor
    uint32_t lmax = max(max(last_contributor[0], last_contributor[1]), max(last_contributor[2], last_contributor[3]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lmax = max(lmax, (uint32_t)__shfl_xor((int)lmax, off, 64));
    if (lane == 0) tile_work[tile] = lmax;
  }
#pragma unroll
  for (int s = 0; s < 4; s++) {
    if (inside[s]) {
      const int px = px0 + (s & 1) * 8, py = py0 + (s >> 1) * 8;
      const int pix_id = W * py + px;
      final_T[pix_id] = fabsf(T[s]);
      n_contrib[pix_id] = last_contributor[s];
      out_depth[pix_id] = D[s];
      out_alpha[pix_id] = X[s];
    }
  }
}

int launch_depth_fwd(const uint2* ranges, const uint32_t* point_list, int W, int H, int grid_x, int grid_y, const Splat* splat,
                     float* final_T, uint32_t* n_contrib, uint32_t* tile_work, float* stop_depth, float* out_depth,
                     float* out_alpha, int cull, hipStream_t s) {
  const dim3 grid(((grid_x * grid_y + 7) / 8) * 8);
  if (cull)
    hipLaunchKernelGGL((depth_fwd_wave_kernel<true>), grid, dim3(64), 0, s, ranges, point_list, W, H, grid_x, splat, final_T,
                       n_contrib, tile_work, stop_depth, out_depth, out_alpha);
  else
    hipLaunchKernelGGL((depth_fwd_wave_kernel<false>), grid, dim3(64), 0, s, ranges, point_list, W, H, grid_x, splat, final_T,
                       n_contrib, tile_work, stop_depth, out_depth, out_alpha);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// backward blend (the cross-lane sums are gs_blend.h's)
// ------------------------------------------------------------------------------------------------------------------
// GRAD_MEANS: the six sums the mean gradient needs (mean2D x, y; conic xx, xy, yy; depth) go to the Gaussian's float64 row in
// ONE atomic instruction of six lanes, seven with GRAD_OPACITY (the general kernel's has twelve).
// GRAD_OPACITY alone: one sum, a fixed reduction tree, one lane's atomic.
template <bool GRAD_MEANS, bool GRAD_OPACITY>
__global__ void __launch_bounds__(64, 4) depth_bwd_wave_kernel(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int grid_x,
    const Splat* __restrict__ splat, const float* __restrict__ final_Ts, const uint32_t* __restrict__ n_contrib,
    const uint32_t* __restrict__ tile_work, const uint32_t* __restrict__ tile_order, const float* __restrict__ dL_ddepth,
    const float* __restrict__ dL_dalpha_img, gs_row_t* __restrict__ grad_rows) {
#pragma clang fp contract(fast)
  __shared__ float4 s_a[WB];  // x, y, view depth, -
  __shared__ float4 s_c[WB];  // conic, opacity
  __shared__ uint32_t s_id[WB];

  // longest tile first, per XCD band (tile_order_kernel in gs_render_fwd_wave.hip)
  const uint32_t tile_u = tile_order[blockIdx.x];
  if (tile_u == 0xFFFFFFFFu) return;
  const int tile = (int)tile_u;
  const uint32_t lmax = tile_work[tile];  // deepest last contributor of the tile's pixels
  if (lmax == 0) return;
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const int lane = threadIdx.x;
  const uint2 range = ranges[tile];
  const int n = (int)(range.y - range.x);
  if (n == 0) return;

  const int px0 = tile_x * TILE_X + (lane & 7), py0 = tile_y * TILE_Y + (lane >> 3);
  const float pixfx0 = (float)px0, pixfy0 = (float)py0;

  // One scalar recurrence per pixel, as in the general kernel, with the colour cotangent zero:
  //   kd = z_i dL_ddepth + 1 dL_dalpha_img,  A = last_alpha (kd_prev - A) + A,  dL_dalpha = (kd - A) T
  // (no background term: the colour image, the only one with a background, has no cotangent)
  float T[4], dLd[4], dLa[4];
  float A[4], kd_prev[4], last_alpha[4];
  uint32_t lastc[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int px = px0 + (s & 1) * 8, py = py0 + (s >> 1) * 8;
    const bool inside = px < W && py < H;
    const int pix_id = W * py + px;
    T[s] = inside ? final_Ts[pix_id] : 0.f;
    lastc[s] = inside ? n_contrib[pix_id] : 0u;
    dLd[s] = (dL_ddepth && inside) ? dL_ddepth[pix_id] : 0.f;        // (a null cotangent is a zero image)
    dLa[s] = (dL_dalpha_img && inside) ? dL_dalpha_img[pix_id] : 0.f;
    A[s] = kd_prev[s] = last_alpha[s] = 0.f;
  }
  // After the reduction lane 15 of row q holds sum q (mean2D x, y, conic xx, xy) and lane 0 of rows 0, 1, 2 holds conic yy,
  // opacity, depth: per-lane slot and factor are fixed for the whole kernel (the general kernel's scheme with fewer lanes)
  const int rq = lane >> 4, lr = lane & 15;
  const float rowscale0 = rq == 0 ? (0.5f * W) / GS_LOG2E : (rq == 1 ? (0.5f * H) / GS_LOG2E : -0.5f);
  const float rowscale1 = rq == 0 ? -0.5f : 1.0f;
  const int lane_slot = lr == 15 ? rq : (rq == 0 ? GR_CYY : (rq == 1 ? GR_OP : GR_ID));
  const float lane_scale = lr == 15 ? rowscale0 : rowscale1;
  const bool lane_adds = lr == 15 || (lr == 0 && (rq == 0 || (rq == 1 && GRAD_OPACITY) || rq == 2));
  const int q0 = n - (int)lmax;  // entries q < q0 (counted from the back) are behind every pixel's last contributor
  const int rounds = (n + WB - 1) / WB;

  float4 ra, rc;
  uint32_t rid = 0;
  ra = rc = make_float4(0.f, 0.f, 0.f, 0.f);
  {
    const int q = (q0 / WB) * WB + lane;
    if (q < n) {
      rid = point_list[range.y - q - 1];
      const float4* rec = reinterpret_cast<const float4*>(&splat[rid]);
      ra = rec[0]; rc = rec[1];
    }
  }
  for (int i = q0 / WB; i < rounds; i++) {
    __syncthreads();  // (single wave) previous batch fully consumed
    s_id[lane] = rid;
    s_a[lane] = make_float4(ra.x, ra.y, ra.z, 0.f);
    s_c[lane] = blend_stage_conic(rc);
    __syncthreads();
    {
      const int q = (i + 1) * WB + lane;
      if (q < n) {
        rid = point_list[range.y - q - 1];
        const float4* rec = reinterpret_cast<const float4*>(&splat[rid]);
        ra = rec[0]; rc = rec[1];
      }
    }
    const int cnt = min(WB, n - i * WB);
    const int jbeg = max(0, q0 - i * WB);
    for (int j = jbeg; j < cnt; j++) {
      const uint32_t contributor = (uint32_t)(n - 1 - (i * WB + j));
      const float4 a = s_a[j];
      const float4 co = s_c[j];
      float G[4], alpha[4];
      bool valid[4];
      unsigned long long vmask[4];
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const float dx = a.x - (pixfx0 + (float)((s & 1) * 8));
        const float dy = a.y - (pixfy0 + (float)((s >> 1) * 8));
        const float p2 = blend_power2(co, dx, dy);
        G[s] = blend_exp2(p2);
        alpha[s] = fminf(0.99f, co.w * G[s]);
        const bool c0 = contributor < lastc[s], c1 = p2 <= 0.0f, c2 = alpha[s] >= 1.0f / 255.0f;
        valid[s] = c0 && c1 && c2;
        vmask[s] = __ballot(c0) & __ballot(c1) & __ballot(c2);
      }
      if ((vmask[0] | vmask[1] | vmask[2] | vmask[3]) == 0ull) continue;

      float v_mx = 0.f, v_my = 0.f, v_cxx = 0.f, v_cxy = 0.f, v_cyy = 0.f, v_op = 0.f, v_id = 0.f;
      const float q2a = co.x + co.x, q2c = co.z + co.z;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        if (valid[s]) {
          const float om = 1.f - alpha[s];
          float rinv = __builtin_amdgcn_rcpf(om);
          rinv = fmaf(rinv, fmaf(-om, rinv, 1.0f), rinv);
          T[s] = T[s] * rinv;
          A[s] = fmaf(last_alpha[s], kd_prev[s] - A[s], A[s]);
          const float kd = fmaf(a.z, dLd[s], dLa[s]);
          kd_prev[s] = kd;
          const float dL_dalpha = (kd - A[s]) * T[s];
          last_alpha[s] = alpha[s];
          if (GRAD_OPACITY) v_op = fmaf(G[s], dL_dalpha, v_op);
          if (GRAD_MEANS) {
            const float dx = a.x - (pixfx0 + (float)((s & 1) * 8));
            const float dy = a.y - (pixfy0 + (float)((s >> 1) * 8));
            const float w = alpha[s] * T[s];
            v_id = fmaf(w, dLd[s], v_id);
            const float h = co.w * G[s] * dL_dalpha;
            const float hx = h * dx, hy = h * dy;
            v_cxx = fmaf(hx, dx, v_cxx);
            v_cxy = fmaf(hx, dy, v_cxy);
            v_cyy = fmaf(hy, dy, v_cyy);
            v_mx = fmaf(q2a, hx, fmaf(co.y, hy, v_mx));
            v_my = fmaf(q2c, hy, fmaf(co.y, hx, v_my));
          }
        }
      }
      if (GRAD_MEANS) {
        const float s0 = swap32_add(v_mx, v_cxx), s1 = swap32_add(v_my, v_cxy);  // (mx|cxx) (my|cxy)
        const float s2 = swap32_add(v_cyy, v_id);                                   // (cyy|id)
        const float s3 = GRAD_OPACITY ? swap32_add(v_op, 0.f) : 0.f;                // (op|-)
        const float t0 = row_total_in_lane15(swap16_add(s0, s1));                // rows: mx my cxx cxy   (lane 15)
        const float t1 = row_total_in_lane0(swap16_add(s2, s3));                 // rows: cyy op id -     (lane 0)
        const float tot = (lr == 15 ? t0 : t1) * lane_scale;
        // one global_atomic_add_f64 instruction, seven (six) lanes, one 128-byte line
        if (lane_adds) atomicAdd(grad_rows + (size_t)s_id[j] * GR_STRIDE + lane_slot, (double)tot);
      } else {
        // the four row totals (lane 15 of each row), added in a fixed order; one lane's atomic
        const float t = row_total_in_lane15(v_op);
        const int ti = __builtin_bit_cast(int, t);
        const float r0 = __int_as_float(__builtin_amdgcn_readlane(ti, 15)), r1 = __int_as_float(__builtin_amdgcn_readlane(ti, 31));
        const float r2 = __int_as_float(__builtin_amdgcn_readlane(ti, 47)), r3 = __int_as_float(__builtin_amdgcn_readlane(ti, 63));
        const float tot = (r0 + r1) + (r2 + r3);
        if (lane == 0) atomicAdd(grad_rows + (size_t)s_id[j] * GR_STRIDE + GR_OP, (double)tot);
      }
    }
  }
}

int launch_depth_bwd(const uint2* ranges, const uint32_t* point_list, int W, int H, int grid_x, int grid_y, const Splat* splat,
                     const float* final_T, const uint32_t* n_contrib, const uint32_t* tile_work, const uint32_t* tile_order,
                     const float* dL_ddepth, const float* dL_dalpha, gs_row_t* grad_rows, int grad_flags, hipStream_t s) {
#define GS_DEPTH_BWD(GM, GO)                                                                                                \
  hipLaunchKernelGGL((depth_bwd_wave_kernel<GM, GO>), dim3(((grid_x * grid_y + 7) / 8) * 8), dim3(64), 0, s, ranges, point_list, W, \
                     H, grid_x, splat, final_T, n_contrib, tile_work, tile_order, dL_ddepth, dL_dalpha, grad_rows)
  if (grad_flags == 3) GS_DEPTH_BWD(true, true);
  else if (grad_flags == 1) GS_DEPTH_BWD(true, false);
  else GS_DEPTH_BWD(false, true);
#undef GS_DEPTH_BWD
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// per-Gaussian tail: one thread per Gaussian, every output row written (zeros for culled rows and rows without instances)
// ------------------------------------------------------------------------------------------------------------------
// The row's gradient from its float64 sums: dL/dmean (GRAD_MEANS; mx, my = dL/dmean2D) and dL/d(activated opacity)
// (GRAD_OPACITY).  One copy of the expressions for the kernel that writes the gradients and the one that steps with them: the
// file is built without contraction, so both round alike.
template <bool GRAD_MEANS, bool GRAD_OPACITY>
__device__ __forceinline__ void depth_point_grad(const DepthPointArgs& a, int idx, V3& dmean, float& mx, float& my, float& dop) {
  const bool active = a.radii[idx] > 0 && !(a.skip_uninstanced && a.tiles_touched[idx] == 0);
  dmean = {0.f, 0.f, 0.f};
  mx = my = dop = 0.f;
  if (active) {
    const double2* gr = reinterpret_cast<const double2*>(a.grad_rows + (size_t)idx * GR_STRIDE);
    if (GRAD_OPACITY) dop = (float)gr[2].y;  // [cyy op]
    if (GRAD_MEANS) {
      const double2 g0 = gr[0], g1 = gr[1], g2 = gr[2], g4 = gr[4];  // [mx my] [cxx cxy] [cyy op] . [b id]
      const V3 mean = {a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]};
      // Sigma in double: from the parameters when they are there, else the caller's covariance as given (chain_from_row)
      SymD Sg;
      if (a.scales) {
        const V3 scl = load_scales(a.scales, idx, 0);
        const V4 rq = load_rotation(a.rotations, idx, 0);
        const double mod = a.scale_modifier;
        const D3 s = {mod * scl.x, mod * scl.y, mod * scl.z};
        Sg = sigma_from_scale_rot(s, quat_to_Rd(rq));
      } else {
        const float2* cv = reinterpret_cast<const float2*>(a.cov3D + 6 * (size_t)idx);
        const float2 v0 = cv[0], v1 = cv[1], v2 = cv[2];
        Sg = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y};
      }
      // only the mean part of the result is used: the dL/dSigma half of cov2d_backward is dead code here
      const Cov2DBack cb = cov2d_backward(mean, Sg, a.viewmatrix, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, {g1.x, g1.y, g2.x},
                                          0.f, 0.f, false, 0.0);
      dmean = cb.dmean;
      {
        // the depth image's part, as chain_from_row writes it (-confidence fork, backward.cu:394-403)
        const float* vm = a.viewmatrix;
        const float zc = vm[2] * mean.x + vm[6] * mean.y + vm[10] * mean.z + vm[14];
        const float gd = (float)g4.y;
        dmean = dmean + V3{(vm[2] - vm[3] * zc) * gd, (vm[6] - vm[7] * zc) * gd, (vm[10] - vm[11] * zc) * gd};
      }
      mx = (float)g0.x;
      my = (float)g0.y;
      dmean = dmean + projection_backward(mean, a.projmatrix, mx, my);
    }
  }
}

template <bool GRAD_MEANS, bool GRAD_OPACITY>
__global__ void __launch_bounds__(GS_BLOCK) depth_point_bwd_kernel(DepthPointArgs a) {
  const int idx = blockIdx.x * GS_BLOCK + threadIdx.x;
  if (idx >= a.P) return;
  V3 dmean;
  float mx, my, dop;
  depth_point_grad<GRAD_MEANS, GRAD_OPACITY>(a, idx, dmean, mx, my, dop);
  if (GRAD_MEANS) {
    a.dL_dmeans3D[3 * idx] = dmean.x;
    a.dL_dmeans3D[3 * idx + 1] = dmean.y;
    a.dL_dmeans3D[3 * idx + 2] = dmean.z;
    a.dL_dmeans2D[3 * idx] = mx;
    a.dL_dmeans2D[3 * idx + 1] = my;
    a.dL_dmeans2D[3 * idx + 2] = 0.f;
  }
  if (GRAD_OPACITY) a.dL_dopacity[idx] = dop;
}

int launch_depth_point_bwd(const DepthPointArgs& a, int grad_flags, hipStream_t s) {
  const dim3 grid((a.P + GS_BLOCK - 1) / GS_BLOCK);
  if (grad_flags == 3) hipLaunchKernelGGL((depth_point_bwd_kernel<true, true>), grid, dim3(GS_BLOCK), 0, s, a);
  else if (grad_flags == 1) hipLaunchKernelGGL((depth_point_bwd_kernel<true, false>), grid, dim3(GS_BLOCK), 0, s, a);
  else hipLaunchKernelGGL((depth_point_bwd_kernel<false, true>), grid, dim3(GS_BLOCK), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// gs_depth_backward_step's tail: depth_point_bwd_kernel with Adam on the ONE tensor the depth leg steps in place of the gradient
// stores.  WHICH 1: param = the means [P,3]; 2: param = the raw opacities [P], the activated ones (g->opacities) give the
// sigmoid's backward in gs_activations_bwd's expression.  Every row is stepped (a zero gradient decays the moments).
// A workgroup owns GS_BLOCK consecutive Gaussians, so GS_BLOCK * 3 (or GS_BLOCK) floats of param / exp_avg / exp_avg_sq in one piece: each
// thread leaves its row's gradient in LDS and the workgroup then walks the piece one dword per lane, consecutive lanes on
// consecutive addresses - the [P,3] rows are 12 bytes apart and start on no vector boundary, so a per-thread row access would
// be three strided dword instructions per array.  Arithmetic: gs_adam.hip's adam_element, this file too is built without
// contraction.
// ------------------------------------------------------------------------------------------------------------------
template <int WHICH>
__global__ void __launch_bounds__(GS_BLOCK) depth_point_step_kernel(DepthPointArgs a, DepthStepArgs st) {
  constexpr int N = WHICH == 1 ? 3 : 1;
  __shared__ float s_g[GS_BLOCK * N];
  const int first = blockIdx.x * GS_BLOCK;
  const int idx = first + threadIdx.x;
  if (idx < a.P) {
    V3 dmean;
    float mx, my, dop;
    depth_point_grad<WHICH == 1, WHICH == 2>(a, idx, dmean, mx, my, dop);
    if (WHICH == 1) {
      s_g[3 * threadIdx.x] = dmean.x;
      s_g[3 * threadIdx.x + 1] = dmean.y;
      s_g[3 * threadIdx.x + 2] = dmean.z;
    } else {
      const float s = st.activated[idx];  // sigmoid backward: grad * (1 - s) * s
      s_g[threadIdx.x] = dop * (1.0f - s) * s;
    }
  }
  __syncthreads();  // (WHICH 1: every read of the means above precedes the stores below - param may BE a.means3D)
  const int cnt = min(GS_BLOCK, a.P - first) * N;
  float* __restrict__ p = st.param + (size_t)first * N;
  float* __restrict__ m = st.exp_avg + (size_t)first * N;
  float* __restrict__ v = st.exp_avg_sq + (size_t)first * N;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int j = k * GS_BLOCK + threadIdx.x;
    if (j < cnt) {
      float pe = p[j], me = m[j], ve = v[j];
      const float g = s_g[j];
      me = st.b1 * me + (1.f - st.b1) * g;
      ve = st.b2 * ve + (1.f - st.b2) * g * g;
      const float denom = sqrtf(ve) * st.inv_sqrt_bc2 + st.eps;
      pe = pe - st.lr_bc1 * (me / denom);
      p[j] = pe;
      m[j] = me;
      v[j] = ve;
    }
  }
}

int launch_depth_point_step(const DepthPointArgs& a, const DepthStepArgs& st, int which, hipStream_t s) {
  const dim3 grid((a.P + GS_BLOCK - 1) / GS_BLOCK);
  if (which == 1) hipLaunchKernelGGL((depth_point_step_kernel<1>), grid, dim3(GS_BLOCK), 0, s, a, st);
  else hipLaunchKernelGGL((depth_point_step_kernel<2>), grid, dim3(GS_BLOCK), 0, s, a, st);
  return 0;
}
