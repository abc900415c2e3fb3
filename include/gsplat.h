/*
 * gsplat.h — C ABI of libgsplat_hip.so, the MI355X (gfx950) differentiable 3D-Gaussian
 * rasterizer + distCUDA2 kNN + Haar-DWT / patch-ELF / SSIM loss kernels.
 *
 * This is the drop-in boundary for the hot path of sparse-view-3dgs-pack (LGDWT-GS).
 * Every entry point takes plain pointers + sizes + a hipStream_t passed as void*; no torch
 * types cross it.  All pointers are DEVICE pointers unless a parameter says "host".
 * Every function returns 0 on success, <0 for an invalid argument (GS_E_*), >0 = hipError_t.
 * Nothing throws across this ABI and nothing here allocates, frees or synchronises the
 * device except where stated (gs_forward_geometry's optional host read-back).
 *
 * Reference interfaces replaced (paths under
 * /root/reference/fs3dgs_benchmark/gaussian-splatting/submodules/):
 *   gs_forward_geometry + gs_forward_render
 *        = CudaRasterizer::Rasterizer::forward   diff-gaussian-rasterization/cuda_rasterizer/rasterizer_impl.cu:198-341
 *          as bound by RasterizeGaussiansCUDA     diff-gaussian-rasterization/rasterize_points.cu:35-124
 *          and pybind `rasterize_gaussians`       diff-gaussian-rasterization/ext.cpp:15-19
 *   gs_backward
 *        = CudaRasterizer::Rasterizer::backward   cuda_rasterizer/rasterizer_impl.cu:345-450
 *          as bound by RasterizeGaussiansBackwardCUDA  rasterize_points.cu:126-223
 *   gs_mark_visible
 *        = Rasterizer::markVisible                rasterizer_impl.cu:141-153, rasterize_points.cu:225-244
 *   gs_knn_mean_dist2
 *        = SimpleKNN::knn / distCUDA2             simple-knn/simple_knn.cu:186-222, simple-knn/spatial.cu:15-26
 *   gs_ssim_fwd / gs_ssim_bwd
 *        = fusedssim / fusedssim_backward         fused-ssim/ssim.cu:187-366
 *   gs_dwt_* / gs_elf_* / gs_patch_*
 *        = get_dwt_subbands / compute_elf_map / compute_patch_dwt_loss
 *          /root/reference/fs3dgs_benchmark/LGDWT-GS/utils/loss_utils.py:106-153,336-442
 *          (arithmetic of the un-vendored pytorch_wavelets DWTForward(J=1,'db1','symmetric'))
 */
#ifndef GSPLAT_H_INCLUDED
#define GSPLAT_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 7  /* round 5: gs_depth_l1, GsView.debug bit 1, binning buffer = sort arrays + region / chunk / tile tables;
                             GsGaussians.shs_rest / GsStepState.grad_out_rest (the model's split SH rows) */

/* error codes (negative = caller error) */
#define GS_OK 0
#define GS_E_NULL (-1)      /* required pointer is NULL */
#define GS_E_SHAPE (-2)     /* inconsistent sizes / exclusive-argument rule violated */
#define GS_E_SCRATCH (-3)   /* scratch buffer too small */
#define GS_E_OVERFLOW (-4)  /* num_rendered exceeded binning capacity (re-run gs_forward_render) */
#define GS_E_UNSUPPORTED (-5)

#define GS_TILE_X 16 /* cuda_rasterizer/config.h:16 */
#define GS_TILE_Y 16 /* cuda_rasterizer/config.h:17 */
#define GS_NUM_CHANNELS 3 /* cuda_rasterizer/config.h:15 */

/* Per-call camera / raster configuration.
 * Mirrors GaussianRasterizationSettings (dgr_3dgs/__init__.py:143-156).  Matrices are the
 * transposed (row-vector) forms the reference's Python hands over: viewmatrix = W2C^T,
 * projmatrix = (P*W2C)^T, each 16 contiguous floats. */
typedef struct GsView {
  int32_t image_height;
  int32_t image_width;
  float tanfovx;
  float tanfovy;
  float scale_modifier;
  int32_t sh_degree;   /* active degree D, 0..3 */
  int32_t prefiltered; /* bool */
  int32_t antialiasing; /* bool */
  int32_t debug;       /* non-zero: synchronise + check after every launch (auxiliary.h:178-185).  Bit 1 (value 2 or 3) is a
                          self-test of the list construction of tile_cull = 0 / 1 (csrc/gs_tilebin.hip): every third Gaussian
                          takes the row-wise entry enumeration that is normally reserved for Gaussians whose span hull holds
                          more regions than tiles; the lists must not change */
  int32_t tile_cull;   /* 0: instance lists = the reference's bounding-square rule (rasterizer_impl.cu:70-111), bit-identical
                          point_list / ranges / num_rendered; 1: additionally drop (tile, Gaussian) pairs on which alpha <
                          1/255 for every pixel (csrc/gs_tilecull.h) - same images and gradients, ~2.6x fewer instances;
                          2: the lists of 1 - every tile's list holds the same Gaussians in the same (depth, index) order -
                          built by REGION BINNING (csrc/gs_regionbin.hip: two launches instead of twenty-three; the lists of
                          different tiles lie in point_list in no particular order, ranges[] says where).  With 2 the
                          binning buffer must be given to gs_forward_geometry already (scratch->binning / binning_capacity) */
  const float* bg;         /* [3] */
  const float* viewmatrix; /* [16] */
  const float* projmatrix; /* [16] */
  const float* campos;     /* [3] */
} GsView;

/* Per-Gaussian inputs.  Exactly one of {shs, colors_precomp} and exactly one of
 * {scales+rotations, cov3D_precomp} is non-NULL (dgr_3dgs/__init__.py:178-182).
 * "Absent" is an explicit NULL (the reference passed data_ptr() of an empty tensor). */
typedef struct GsGaussians {
  int32_t P; /* number of Gaussians */
  int32_t M; /* SH coefficients stored per Gaussian (16 for degree 3); 0 when shs == NULL */
  const float* means3D;        /* [P,3] */
  const float* shs;            /* [P,M,3] or NULL */
  const float* colors_precomp; /* [P,3] or NULL */
  const float* opacities;      /* [P]   (the [P,1] tensor) */
  const float* scales;         /* [P,3] or NULL */
  const float* rotations;      /* [P,4] or NULL (r,x,y,z; NOT renormalised, forward.cu:123) */
  const float* cov3D_precomp;  /* [P,6] or NULL */
  const float* extra_channel;  /* [P] or NULL: a 4th per-Gaussian value blended with the same weights as the colour
                                  (gs_forward_render_x); replaces the reference's second rasterizer pass for the NIR
                                  albedo, mult-dwtgs/gaussian_renderer/__init__.py:151-258 */
  int32_t raw_activations;     /* 0: opacities / scales / rotations are the activated values, as the reference's rasterizer
                                  takes them.  1: they are the model's RAW rows (gaussian_model.py:60-78) and the kernels
                                  apply sigmoid / exp / F.normalize on the fly, with gs_activations_fwd's arithmetic bit for
                                  bit - so the activated copies are never written nor read.  Honoured by
                                  gs_forward_geometry (hence by every forward render behind it, gs_forward_render_fsgs
                                  included) and by gs_backward_step / _x / _fsgs only (the plain backwards return gradients
                                  with respect to the activated values: GS_E_UNSUPPORTED with this flag) */
  const float* extra_gain;     /* with raw_activations and extra_channel: device scalar; the blended 4th channel is then
                                  sigmoid(extra_channel[i]) * clamp(*extra_gain, 0.1, 10) - the multispectral model's raw NIR
                                  albedo and global gain (mult-dwtgs/gaussian_renderer/__init__.py:166-169), activated in
                                  the kernel like the other raw rows.  NULL: extra_channel holds the values to blend */
  const float* shs_rest;       /* NULL: `shs` holds all M coefficients of a Gaussian in one row.  Otherwise the SPLIT layout of the
                                  reference's GaussianModel (scene/gaussian_model.py:45-46,127-130): `shs` = _features_dc [P,1,3],
                                  `shs_rest` = _features_rest [P,M-1,3] - the kernels read the two rows where the model keeps
                                  them, so no torch.cat copy of 192 B per Gaussian runs per view (gaussian_model.py:get_features).
                                  Honoured by gs_forward_geometry and by gs_backward_step in its gradients-out form
                                  (GsStepState.grad_out_rest); the other entries return GS_E_UNSUPPORTED */
} GsGaussians;

/* Caller-owned scratch.  geom and img sizes depend on (P, W, H); binning on the capacity in
 * instances (Gaussian x tile pairs).  The three buffers are the private fwd<->bwd contract
 * (the reference's geomBuffer / binningBuffer / imgBuffer byte tensors): backward must get
 * back exactly the bytes forward wrote. */
typedef struct GsScratch {
  void* geom;
  size_t geom_bytes;
  void* img;
  size_t img_bytes;
  void* binning;
  size_t binning_bytes;
  int64_t binning_capacity; /* instances the binning buffer was sized for */
  const uint32_t* tile_order_hint; /* optional (NULL: image order): launch order of the forward blend's tiles, as
                                      gs_export_tile_order returned it for an earlier view of the SAME image size -
                                      typically the previous visit of this camera, or just the previous view.  Pure
                                      scheduling (longest tile first, see gs_export_tile_order): outputs do not depend on it.
                                      Must be an unmodified export - every tile exactly once. */
  const float* tile_depth_limit;   /* optional (NULL: none), only read when GsView.tile_cull is set; gs_tile_depth_limit_floats(W, H) floats: per tile, the view
                                      depth beyond which (plus a 5 % + 0.02 margin) no (tile, Gaussian) pair is emitted -
                                      gs_export_tile_stop_depth of an earlier forward of the SAME camera.  The forward checks
                                      that the cut lists were long enough (gs_forward_status.trunc_failed == 0); when they
                                      were, every output and gradient equals that of the uncut lists.  When the flag is set
                                      the outputs are NOT valid: repeat gs_forward_geometry + gs_forward_render without
                                      limits.  The same pointer and contents must be passed to both forward calls. */
  uint32_t* tile_order_out;        /* optional: gs_forward_render also writes what gs_export_tile_order would return here */
  float* tile_depth_limit_out;     /* optional: ... and what gs_export_tile_stop_depth would return here (one launch serves
                                      both; the buffers may be the ones passed as tile_order_hint / tile_depth_limit: they
                                      are read before they are written; a forward that overflowed its binning capacity
                                      writes neither, so that it can be repeated with the same hint and bounds) */
  int32_t binned;                  /* 1: gs_forward_bin has already built the instance lists of this view in these buffers;
                                      gs_forward_render* then only blends.  Written by the library: gs_forward_geometry
                                      clears it (a new geometry state invalidates any lists), gs_forward_bin sets it - a
                                      caller that re-uses one GsScratch across views need not touch it */
  int32_t defer_tile_order;        /* 1: gs_forward_render* stops after the blend; the caller runs gs_forward_tile_order (the forward's
                                      last kernel: launch order of the backward, the camera's next hints / depth bounds, status_host)
                                      itself - on another stream, beside whatever follows the forward, ordered before gs_backward* */
  const uint32_t* step_tag;        /* optional, device: gs_forward_status then copies TWELVE words out - the four status words,
                                      four reserved ones, *step_tag, three reserved - so that a caller that replays a
                                      captured graph of the step can tell, by polling its pinned block for the tag it
                                      uploaded before the replay, that the status of THAT replay has arrived (no stream
                                      synchronisation, no event inside the graph) */
  const float* tile_depth_limit_slack; /* optional, device, one float >= 1 (NULL: 1): the bounds written to tile_depth_limit_out
                                      are multiplied by it.  A caller whose model moves fast between two visits of a camera (early
                                      training) raises it for the cameras whose limits fail and lowers it again when they hold:
                                      longer lists, fewer repeated views.  Device memory so that a replayed graph sees changes. */
  uint32_t* status_host;           /* optional: 16 words of PINNED, device-mapped host memory (hipHostMalloc / torch pin_memory).
                                      gs_forward_render* then delivers what gs_forward_status would - words 0-3 = num_rendered,
                                      overflow, trunc_failed, largest region count; with step_tag also word 8 = *step_tag and word 9 =
                                      GS_STATUS_CHECK - from its LAST kernel, with system-scope stores: no copy command, no extra
                                      launch on the stream.  Complete when the call's work has completed; a host that polls for
                                      the tag accepts the block when the check word matches, as with gs_forward_status. */
  void* early_geometry_done;       /* optional (NULL: none), a hipEvent_t: gs_forward_geometry_early has run for EXACTLY this view,
                                      these Gaussian rows, these buffers, this tile_depth_limit and this radii array, and the event
                                      was recorded behind it.  gs_forward_geometry then waits for the event, resets the header and
                                      runs the geometry kernel only over the 256-row blocks that call left out; everything downstream
                                      is the single launch's, bit for bit.  Only with GsView.tile_cull = 2.  One-shot: the library
                                      clears the field, so a forward repeated with the same struct runs in full. */
} GsScratch;

/* Gradient outputs of gs_backward (rasterize_points.cu:163-178).  All are written in full by
 * the call (rows of culled Gaussians become 0) - the caller need not zero them.  Any pointer
 * may be NULL when that gradient is not wanted, except that dL_dsh / dL_dcolors follow the
 * colour mode and dL_dscales+dL_drotations / dL_dcov3D follow the covariance mode. */
typedef struct GsGrads {
  float* dL_dmeans3D;   /* [P,3] */
  float* dL_dmeans2D;   /* [P,3]  (z = 0) */
  float* dL_dsh;        /* [P,M,3] */
  float* dL_dcolors;    /* [P,3] */
  float* dL_dopacity;   /* [P] */
  float* dL_dscales;    /* [P,3] */
  float* dL_drotations; /* [P,4] */
  float* dL_dcov3D;     /* [P,6] */
  float* dL_dextra;     /* [P]  gradient of GsGaussians.extra_channel (gs_backward_x only), may be NULL */
} GsGrads;

int gs_abi_version(void);
/* Human readable build string: arch, compiler, kernel variants. */
const char* gs_build_info(void);
/* sizeof() of a public struct as this library was compiled: 0 GsView, 1 GsGaussians, 2 GsScratch, 3 GsGrads, 4 GsStepState,
 * 5 GsLgdwtParams, 6 GsAdamSeg; 0 for any other index.  A binding written in another language (the ctypes mirror of
 * gsplat_amd/capi.py, a cgo / JNI struct) checks its own layout against it at load time. */
size_t gs_struct_bytes(int32_t which);

/* out[0..2] = bytes needed for geom, img, binning given capacity R_capacity instances.
 * workspace_bytes (may be NULL) = bytes gs_backward needs as its workspace. */
int gs_scratch_bytes(int32_t P, int32_t W, int32_t H, int64_t R_capacity, size_t out[3],
                     size_t* backward_workspace_bytes);

/* Phase 1 of forward: per-Gaussian preprocess (cull, project, cov3D, EWA cov2D, conic,
 * radius, tile rect, SH->RGB) and the prefix sum of tiles_touched.  Writes radii[P].
 * num_rendered is left in the geom header on the device; if num_rendered_host != NULL it is
 * also copied there with hipMemcpyAsync on `stream` (pass pinned memory, then wait on the
 * stream/an event before reading it).  Does not block the host. */
int gs_forward_geometry(const GsView* view, const GsGaussians* g, GsScratch* scratch,
                        int32_t* radii, int32_t* num_rendered_host, void* stream);

/* Phase 2 of forward: duplicate (tile|depth) keys, stable radix sort on the low
 * 32+ceil_log2(T) key bits, tile ranges, front-to-back alpha blend.  Reads num_rendered from
 * the geom header on the device.  If it exceeds scratch->binning_capacity nothing is blended,
 * an overflow flag is left in the geom header and the image outputs are undefined: the caller
 * (who learns num_rendered from phase 1) re-runs this phase with a larger binning buffer.
 * out_color [3,H,W], out_invdepth [H,W] (may be NULL). */
int gs_forward_render(const GsView* view, const GsGaussians* g, GsScratch* scratch,
                      float* out_color, float* out_invdepth, void* stream);

/* The binning stage of gs_forward_render on its own (instance lists + tile ranges), followed by an asynchronous copy of
 * the four status words of gs_forward_status to status_host (pinned; may be NULL).  A caller that wants to know whether
 * the lists fitted the binning capacity without waiting for the blend calls this, records an event, calls
 * gs_forward_render* with scratch->binned = 1 and waits for the event while the blend runs. */
int gs_forward_bin(const GsView* view, const GsGaussians* g, GsScratch* scratch, uint32_t* status_host, void* stream);

/* gs_forward_render with a 4th blended channel: out_extra[H,W] = sum_i extra_i alpha_i T_i + T_final * bg[0], i.e.
 * channel 0 of a second rasterizer pass with colors_precomp = extra.repeat(1,3) - what the reference's render_nir
 * keeps (mult-dwtgs/gaussian_renderer/__init__.py:190-256) - sharing preprocess, binning and the alpha evaluation
 * with the colour pass.  out_extra == NULL is gs_forward_render. */
int gs_forward_render_x(const GsView* view, const GsGaussians* g, GsScratch* scratch,
                        float* out_color, float* out_invdepth, float* out_extra, void* stream);

/* Backward of the whole rasterizer.  num_rendered is the value forward produced.
 * dL_dinvdepth may be NULL (then no inverse-depth gradient path runs).
 * workspace: >= backward_workspace_bytes from gs_scratch_bytes (per Gaussian one 128-byte row of float64 blend sums -
 * stage 1 - and one 80-byte record of stage 2's float64 covariance chain).
 * Accuracy (fp32 outputs): every gradient tensor within 1e-4 of its largest entry of the reference algorithm evaluated
 * in exact arithmetic on the same blend sums.  For dL_dscales / dL_drotations that is a stronger statement than "1e-4 of
 * the reference's fp32 run": the chain conic -> cov2D -> cov3D -> (scale, quaternion) (backward.cu:248-275, 330-393)
 * cancels 3-4 digits for needle-shaped footprints, and the reference's own fp32 formula is 1.0e-3 / 2.0e-3 of the
 * tensor's max away from the float64 image of its inputs at 1 M Gaussians / 1080p.  Here the blend sums are accumulated
 * in float64 rows and that chain is evaluated in float64 (csrc/gs_backward_math.h), so these two tensors are the exact
 * image rounded once and repeat from run to run; tests/test_gpu_fullsize.py asserts it, DESIGN.md section 2 has the analysis. */
int gs_backward(const GsView* view, const GsGaussians* g, const int32_t* radii,
                const GsScratch* scratch, int64_t num_rendered, const float* dL_dcolor,
                const float* dL_dinvdepth, const GsGrads* grads, void* workspace,
                size_t workspace_bytes, void* stream);

/* gs_backward with the image gradient of the 4th channel (dL_dextra_img [H,W], NULL = gs_backward); geometry
 * gradients are those of the sum of both passes, grads->dL_dextra[P] receives the channel's own gradient. */
int gs_backward_x(const GsView* view, const GsGaussians* g, const int32_t* radii,
                  const GsScratch* scratch, int64_t num_rendered, const float* dL_dcolor,
                  const float* dL_dinvdepth, const float* dL_dextra_img, const GsGrads* grads,
                  void* workspace, size_t workspace_bytes, void* stream);

/* gs_backward for the model's SPLIT SH rows (GsGaussians.shs_rest != NULL, raw_activations == 0): what the reference's
 * `rasterizer(dc=pc.get_features_dc, shs=pc.get_features_rest, ...)` call needs (gaussian_renderer/__init__.py:82-100).
 * grads->dL_dsh is then the gradient of the DC rows, [P,1,3], and dL_dsh_rest that of g->shs_rest, [P,M-1,3]: one
 * contiguous gradient per model tensor, both FULLY written (zeros for culled Gaussians and for the coefficients above the
 * active degree: allocate them uninitialised), straight from the per-Gaussian kernel - no [P,M,3] intermediate, no copy.
 * Values are bit for bit the slices [:, :1] and [:, 1:] of the dL_dsh that gs_backward writes for the concatenated rows.
 * Everything else - the other gradients, anti-aliasing, dL_dinvdepth, the workspace - is gs_backward.
 * GS_E_UNSUPPORTED: g->shs_rest == NULL or raw_activations set; GS_E_NULL: dL_dsh_rest or grads->dL_dsh missing; no launch
 * in either case.  (gs_backward itself keeps answering GS_E_UNSUPPORTED for split rows.) */
int gs_backward_split(const GsView* view, const GsGaussians* g, const int32_t* radii,
                      const GsScratch* scratch, int64_t num_rendered, const float* dL_dcolor,
                      const float* dL_dinvdepth, const GsGrads* grads, float* dL_dsh_rest, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The older rasterizer generation used by FSGS / DNGaussian (SURVEY 8f-4;
 * FSGS/submodules/diff-gaussian-rasterization-confidence: `rasterize_gaussians` returns colour, depth, alpha -
 * rasterize_points.cu, forward.cu:262-380; backward takes their three image gradients, backward.cu:414-600).
 * Same geometry phase (gs_forward_geometry with antialiasing = 0: the 0.3 low-pass is unconditional there).
 * out_depth[H,W] = sum depth_i alpha_i T_i (view-space z), out_alpha[H,W] = sum alpha_i T_i; no inverse depth. */
int gs_forward_render_fsgs(const GsView* view, const GsGaussians* g, GsScratch* scratch,
                           float* out_color, float* out_depth, float* out_alpha, void* stream);
int gs_backward_fsgs(const GsView* view, const GsGaussians* g, const int32_t* radii,
                     const GsScratch* scratch, int64_t num_rendered, const float* dL_dcolor,
                     const float* dL_ddepth, const float* dL_dalpha, const GsGrads* grads,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The depth-only pass: the depth and alpha images of the generation above without its colour image, and their gradients
 * with respect to the means and / or the opacities only - what DNGaussian's two depth passes (render_for_depth, render_for_opa:
 * constant colour 1, scales and rotations detached) read.  Additive; device library only.
 * gs_depth_forward runs on scratch whose geometry phase has run (gs_forward_geometry with antialiasing = 0 and any [P,3] array
 * as colors_precomp: the colours are never read here), builds the lists unless scratch->binned, blends and leaves the
 * backward blend's launch order.  out_depth / out_alpha [H,W] are the images of gs_forward_render_fsgs, bit for bit.
 * Depth-limited lists, tile-order hints and exports are not served (tile_depth_limit set: GS_E_UNSUPPORTED).
 * gs_depth_backward: dL_ddepth / dL_dalpha [H,W], either may be NULL (= zero).  grad_flags: 1 = means (dL_dmeans3D [P,3] and
 * dL_dmeans2D [P,3], both required), 2 = opacities (dL_dopacity [P]), 3 = both; every row of a requested output is written.
 * workspace: >= P * 128 bytes rounded up to 256 (the float64 blend sums), device memory.
 * Status codes, no launch: anti-aliasing, raw_activations, shs_rest, extra_channel -> GS_E_UNSUPPORTED; NULL outputs or a NULL
 * gradient pointer of a requested family -> GS_E_NULL; grad_flags outside 1..3 -> GS_E_SHAPE.  P == 0: outputs zeroed, GS_OK. */
int gs_depth_forward(const GsView* view, const GsGaussians* g, GsScratch* scratch, float* out_depth,
                     float* out_alpha, void* stream);
int gs_depth_backward(const GsView* view, const GsGaussians* g, const int32_t* radii,
                      const GsScratch* scratch, int64_t num_rendered, const float* dL_ddepth,
                      const float* dL_dalpha, int grad_flags, float* dL_dmeans3D, float* dL_dmeans2D,
                      float* dL_dopacity, void* workspace, size_t workspace_bytes, void* stream);

/* gs_depth_backward with the optimizer step of a DNGaussian depth leg in its tail (train_llff.py:104-135: each leg's backward is
 * followed by an Adam step of ONE tensor).  Row zeroing and blend backward are gs_depth_backward's; the per-Gaussian launch then
 * steps the row it has just differentiated.  Additive; device library only.
 *   which 1: gradient to the means; param / exp_avg / exp_avg_sq [P,3] (param may be g->means3D itself).
 *   which 2: gradient to the opacities; param / moments [P] are the RAW opacity row, g->opacities its sigmoid: the gradient of
 *            the raw row is dL_dopacity * (1 - s) * s, gs_activations_bwd's expression.
 * The row's gradient has the bits gs_depth_backward writes (zero for culled rows and rows without instances); the update is
 * the rule at gs_adam_step_tensors with flags == 0, coefficients formed from (lr, step) as gs_adam_step forms them, so
 * parameters and moments equal gs_depth_backward [+ the sigmoid line] + gs_adam_step bit for bit.  EVERY row is stepped: a zero
 * gradient still decays the moments and moves the parameter.  No gradient array and no dL_dmeans2D is written.
 * flags: GS_DEPTH_STEP_ROWS_GIVEN - the float64 rows in `workspace` are taken as they are (as a gs_depth_backward of the same
 * scratch and cotangents left them): no zeroing, no blend; dL_ddepth / dL_dalpha may then be NULL.
 * workspace as gs_depth_backward.  Status codes, no launch: gs_depth_backward's, and NULL param / moments -> GS_E_NULL; which
 * outside 1..2 or step < 1 -> GS_E_SHAPE; an unknown flag bit -> GS_E_UNSUPPORTED.  P == 0: GS_OK, nothing launched. */
#define GS_DEPTH_STEP_ROWS_GIVEN 1
int gs_depth_backward_step(const GsView* view, const GsGaussians* g, const int32_t* radii,
                           const GsScratch* scratch, int64_t num_rendered, const float* dL_ddepth,
                           const float* dL_dalpha, int which, float* param, float* exp_avg, float* exp_avg_sq,
                           float lr, int32_t step, float beta1, float beta2, float eps, int32_t flags,
                           void* workspace, size_t workspace_bytes, void* stream);

/* present[i] = (view-space z of means3D[i]) > 0.2   (rasterizer_impl.cu:54-66) */
int gs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix,
                    const float* projmatrix, uint8_t* present, void* stream);

/* Region binning (GsView.tile_cull = 2), which form of the forward geometry kernel fills the region buckets: 1 = a wave shares
 * the regions of its large footprints among its lanes (csrc/gs_preprocess.hip), 0 = every lane walks its own.  Same lists,
 * same records, bit for bit; the second form is the control arm of a measurement.  form < 0 changes nothing.  Returns the
 * form the next launches take; until set it is the environment's GS_REGION_COOP (read once), else the built-in default.
 * Not synchronised with launches in flight on other threads. */
int gs_region_coop(int32_t form);

/* ---- debug / parity exports: copy internal state into plain arrays (any pointer may be
 * NULL).  Used by the parity tests to compare against the oracle; not on the hot path. ---- */
int gs_export_geom(const GsScratch* scratch, int32_t P, float* depths, float* means2D /*[P,2]*/,
                   float* cov3D /*[P,6]*/, float* conic_opacity /*[P,4]*/, float* rgb /*[P,3]*/,
                   uint8_t* clamped /*[P,3]*/, uint32_t* tiles_touched, uint32_t* point_offsets,
                   void* stream);
int gs_export_binning(const GsScratch* scratch, int64_t num_rendered, uint64_t* keys_sorted,
                      uint32_t* point_list, void* stream);
int gs_export_img(const GsScratch* scratch, int32_t W, int32_t H, float* final_T,
                  uint32_t* n_contrib, uint32_t* ranges /*[T,2]*/, void* stream);

/* The tail of a single-GPU train step fused into the backward (LGDWT-GS/train.py:262-288,
 * scene/gaussian_model.py:40-60,183-193,471-473): gs_backward, then IN THE SAME per-Gaussian kernel the backward of the
 * parameter activations (exp / F.normalize / sigmoid), the densification statistics of the view and the Adam update of
 * the Gaussian's 59 parameters - the 236 B/Gaussian of gradients are never written to memory nor read back, and three
 * launches (activation backward, statistics, Adam) disappear.  Valid when every gradient is final after this one view
 * (one camera per optimizer step on one GPU - the reference's own loop); the data-parallel step keeps gs_backward +
 * all-reduce + gs_adam_step.  Arithmetic per element is that of gs_activations_bwd, gs_densify_stats and gs_adam_step.
 *
 * The raw parameter rows live in the caller's buffers; g->means3D must BE st->xyz and g->shs must BE st->features (no
 * activation in between), g->scales / rotations / opacities are the activated tensors handed to the forward;
 * g->M == 16, no precomputed colours / covariances. */
typedef struct GsStepState {
  float* xyz;       /* [P,3]   raw parameters, updated in place */
  float* features;  /* [P,16,3] */
  float* opacity;   /* [P]   pre-sigmoid */
  float* scaling;   /* [P,3] pre-exp */
  float* rotation;  /* [P,4] un-normalised */
  float* m[5];      /* Adam exp_avg of the five rows above, same shapes */
  float* v[5];      /* Adam exp_avg_sq */
  float lr[6];      /* xyz, features DC (k = 0), features rest (k = 1..15), opacity, scaling, rotation */
  int32_t step[5];  /* the row's 1-based Adam step count (bias correction); 0 = row skipped: parameter and moments untouched */
  float beta1, beta2, eps;
  float* max_radii2D;        /* [P] densification statistics of train.py:266-268 (all three or none) */
  float* xyz_gradient_accum; /* [P] */
  float* denom;              /* [P] */
  const float* coef_dev;      /* optional, device, 11 floats (15 with st->extra: + the same two constants of the sixth row and
                                of the gain): lr[c] / (1 - beta1^t) for the six learning-rate classes, then
                                1 / sqrt(1 - beta2^t) for the five rows.  NULL: computed from lr[] / step[] on the host and
                                passed as kernel arguments.  A caller that REPLAYS a captured graph of the step must use
                                this form (kernel arguments are frozen at capture) and refresh the buffer before each
                                replay; step[] then only says which rows are skipped. */
  const double* rows_override; /* parity probe, normally NULL: [P,16] float64 blend sums to use INSTEAD of running stage 1 (layout:
                                gs_backward_from_rows) - lets a test hand the fused tail and the three-kernel tail the
                                very same sums and compare them bit for bit */
  /* ---- data-parallel form (N > 1): gradients OUT instead of the Adam step ----
   * grad_out[0] != NULL: the gradients with respect to the RAW rows (xyz [P,3], features [P,16,3], opacity [P], scaling [P,3],
   * rotation [P,4]: the five pointers, typically into one flat buffer that is then all-reduced) are WRITTEN there and no
   * parameter or moment is touched; m[] / v[] / lr[] / step[] are ignored.  The statistics are then this view's
   * INCREMENTS, assigned: xyz_gradient_accum[i] = |dL/dmean2D_i| (0 when culled), denom[i] = visible ? 1 : 0 (summed over
   * ranks by the caller); max_radii2D is updated in place as always.  fail_flag (device, may be NULL): set to 1.0f when
   * the forward had flagged overflow or trunc_failed - the call then writes ZERO statistic increments and no gradients -
   * else to 0.0f; reduced (sum) with the gradients it tells every rank whether any rank's view was invalid
   * (gs_adam_step_gated takes it as its gate).  The single-GPU form writes the same flag when fail_flag is given (the gate of
 * the trained exposures' step, gs_exposure_adam). */
  float* grad_out[5];
  float* fail_flag;
  /* ---- two-phase step (single GPU; any list mode) ----
   * 0: gs_backward_step handles every Gaussian.  2: only the Gaussians that emitted instances in this view - the caller has
   * already run gs_step_uninstanced on the same state for the others. */
  int32_t phase;
  /* The workspace rows between steps (single GPU, rows_override == NULL).  0: gs_backward_step clears the rows of the
   * Gaussians with instances before the blend accumulates into them and leaves the sums behind (a probe may read them).
   * 1: as 0, and the per-Gaussian kernel zeroes every row it has consumed - also when the step is a no-op on the device -
   * so the workspace is all zero again when the call has run.  2: the caller guarantees exactly that state on entry (same
   * workspace, last used by a call with rows_clean != 0, or zero-filled): no clear launch at all. */
  int32_t rows_clean;
  void* phase1_done; /* with phase = 2: a hipEvent_t recorded behind gs_step_uninstanced on its stream, or NULL.  gs_backward_step
                        makes its stream wait for it AFTER the backward blend has been launched - the two then run side by
                        side - and before the per-Gaussian kernel.  NULL: the caller has ordered the two calls itself. */
  /* ---- 4th blended channel (gs_backward_step_x; multispectral train step, mult-dwtgs/train_nir.py): g->extra_channel must
   * BE st->extra (the raw per-Gaussian parameter, e.g. the NIR albedo before its sigmoid) and g->extra_gain st->gain.  The
   * raw row is stepped like the five rows above (sixth row: lr_extra, step_extra, coef_dev[11..12]); the global gain - one
   * scalar, dL/dgain = sum_i dL/dextra_i sigmoid(raw_i) inside the clamp, 0 outside - by the first workgroup of the
   * per-Gaussian kernel, from one partial sum per 256 Gaussians that the float64 chain kernel left behind the records in
   * the workspace, added in index order (deterministic; lr_gain, step_gain, coef_dev[13..14]).  Data-parallel form:
   * grad_out_extra [P] / grad_out_gain [1] receive the gradients instead. */
  float* extra;    /* [P] or NULL (then none of the fields below is read) */
  float* extra_m;
  float* extra_v;
  float* gain;     /* device scalar */
  float* gain_m;
  float* gain_v;
  float lr_extra, lr_gain;
  int32_t step_extra, step_gain;
  float* grad_out_extra;
  float* grad_out_gain;
  /* data-parallel form, optional: [P] bytes, 1 where this view's gradients of the Gaussian may be non-zero (it emitted
   * instances), 0 where every one of its gradient floats was written as zero.  The union of the ranks' masks is what a
   * sparse exchange has to move (gsplat_amd.trainer: pack the union's rows, all-reduce, scatter back). */
  uint8_t* grad_mask;
  /* Adam-inside-the-backward form, optional: one byte per block of GS_STEP_BLOCK (256) consecutive Gaussians, 1 = "BOTH
   * Adam moments of EVERY row of every Gaussian of the block are +0" (the caller's claim; gsplat_amd.trainer derives it
   * from the moments themselves).  The zero-gradient update of such a block changes no bit of parameters or moments
   * (m' = v' = +0, p' = p - lr * (0 / eps) = p; needs eps > 0), so the kernels skip its parameter and moment traffic;
   * a block in which a Gaussian receives a gradient gets its byte cleared by the kernel that writes its moments.
   * View statistics are kept for every Gaussian as without it.  With the model's rows in spatial order (neighbours in
   * memory = neighbours in space) the Gaussians no camera reaches fill whole blocks. */
  uint8_t* dormant;
  /* "sparse_adam" (train.py:282-284): 1 = a Gaussian with radii <= 0 in this view is not stepped at all - its parameters and
   * both moments keep their bits (with the default optimizer it takes a zero-gradient step: the moments decay, the
   * parameter moves by the old momentum).  Visible Gaussians without instances (culled spans, depth limits) still take
   * their zero-gradient step.  Blocks of 256 rows without a visible Gaussian cost no parameter or moment traffic. */
  int32_t sparse;
  /* 1: "a Gaussian with instances" means, for this step's tail, one that owns a list entry the BACKWARD BLEND VISITS (in front of
   * its tile's deepest last contributor; the forward blend leaves one byte per Gaussian saying so in the geometry buffer) instead
   * of one that emitted instances at all.  The others - accepted by a tile but lying behind every pixel's saturation, a quarter
   * to a third of the accepted ones on a trained scene - have all-zero sums, hence exact-zero gradients: gs_step_uninstanced
   * steps them beside the blend, the chain and the per-Gaussian kernel of gs_backward_step never read their rows.  Same
   * parameters, moments and statistics as with 0 (a moment may differ in the sign of a zero).  Give the SAME value to
   * gs_step_uninstanced and to gs_backward_step.  Ignored - the split stays on tiles_touched - with rows_override, in the
   * data-parallel form, and when the forward blend did not write the flags (GS_REACHED_SPLIT=0 in the environment).
   * (The field lies in what was padding behind `sparse`: no offset and no size changed, a caller that zero-fills the struct
   * gets the old behaviour.) */
  int32_t reached_split;
  /* Gradients-out form with the split SH layout (GsGaussians.shs_rest != NULL): grad_out[1] receives the gradient of
   * _features_dc [P,1,3] and grad_out_rest that of _features_rest [P,M-1,3] - each a contiguous tensor as autograd's
   * AccumulateGrad wants it (a strided slice of one [P,16,3] buffer is copied again).  NULL with the one-row layout. */
  float* grad_out_rest;
} GsStepState;
#define GS_STEP_BLOCK 256
int gs_backward_step(const GsView* view, const GsGaussians* g, const int32_t* radii,
                     const GsScratch* scratch, int64_t num_rendered, const float* dL_dcolor,
                     const float* dL_dinvdepth, const GsStepState* st, void* workspace,
                     size_t workspace_bytes, void* stream);
/* gs_backward_step behind gs_forward_render_x: dL_dextra_img [H,W] is the image gradient of the 4th channel; st->extra et
 * al. describe its parameters (see GsStepState). */
int gs_backward_step_x(const GsView* view, const GsGaussians* g, const int32_t* radii,
                       const GsScratch* scratch, int64_t num_rendered, const float* dL_dcolor,
                       const float* dL_dinvdepth, const float* dL_dextra_img, const GsStepState* st,
                       void* workspace, size_t workspace_bytes, void* stream);
/* gs_backward_step behind gs_forward_render_fsgs (the FSGS / DNGaussian rasterizer generation; FSGS/train.py:133-176 is one
 * camera per optimizer step, so every gradient is final after this view): dL_ddepth / dL_dalpha [H,W] are the image
 * gradients of that generation's depth and alpha outputs, as gs_backward_fsgs takes them.  Same per-Gaussian kernel, same
 * element arithmetic: given the same blend sums the call leaves the bits that gs_backward_fsgs + gs_activations_bwd +
 * gs_densify_stats + gs_adam_step leave.  Both forms of GsStepState are served - Adam inside (m / v) and gradients out
 * (grad_out, with split SH rows through shs_rest / grad_out_rest as gs_backward_step serves them) - and so are
 * GsGaussians.raw_activations, rows_override, rows_clean, reached_split, dormant, sparse, coef_dev and fail_flag.
 * Status codes, no launch: GS_E_NULL for a NULL dL_ddepth, dL_dalpha or st; GS_E_UNSUPPORTED for view->antialiasing, for a
 * 4th channel (g->extra_channel or st->extra: this generation has none) and for st->phase != 0 (no two-phase form: do not
 * pair it with gs_step_uninstanced); everything gs_backward_step refuses (GsStepState's rules above). */
int gs_backward_step_fsgs(const GsView* view, const GsGaussians* g, const int32_t* radii,
                          const GsScratch* scratch, int64_t num_rendered, const float* dL_dcolor,
                          const float* dL_ddepth, const float* dL_dalpha, const GsStepState* st,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The part of gs_backward_step that does not wait for the loss: a Gaussian that emitted no instance in this view
 * (tiles_touched == 0: off screen, culled, or cut by the depth limits - four fifths of them on depth-limited lists) has
 * zero gradients whatever the image looks like, so its view statistics and its Adam step (zero gradient: the moments decay,
 * the parameter moves by the old momentum - torch.optim.Adam does the same) need nothing but the forward's geometry stage.
 * Call it on a second stream, ordered after gs_forward_render, right before gs_backward_step with st->phase = 2 on the
 * first: it then runs CONCURRENTLY with stage 1 of the backward, the blend - a pure HBM stream next to a kernel that is
 * bound by vector issue and leaves HBM idle (next to the criterion's kernels it gains nothing: they slow down by what it
 * takes, measured).  gs_backward_step steps the Gaussians with instances; its per-Gaussian kernel must be ordered after
 * this call (st->phase1_done; the two split the float4s of the parameter rows between them).  Like gs_backward_step a no-op on the device when the forward had flagged
 * overflow or trunc_failed, and with st->reached_split it reads the per-Gaussian flags the forward blend writes - so it must
 * not start before the forward BLEND has finished.  Same element arithmetic: the
 * two calls together leave the bits gs_backward_step (phase 0) leaves.  With tile_cull = 0 every visible Gaussian has
 * instances, and the Gaussians without are the ones outside the frustum (59 % of bench.py's scene: with the rows in spatial
 * order most of their blocks are dormant, see GsStepState.dormant).  GS_E_UNSUPPORTED in the data-parallel form.
 * Although `scratch` is const, the call WRITES one word of the geometry header it points at: the block cursor its
 * workgroups draw their work from (zeroed by gs_forward_geometry, re-armed by the call's last workgroup).  Every call is
 * therefore one full zero-gradient step of the uninstanced Gaussians - calling it twice behind one forward steps them
 * twice; two calls on the SAME scratch must not overlap in time (they would share the cursor). */
int gs_step_uninstanced(const GsView* view, const GsGaussians* g, const int32_t* radii,
                        const GsScratch* scratch, const GsStepState* st, void* stream);

/* Additive entry (GS_ABI_VERSION unchanged).  The early geometry pass of the NEXT view, in place: zeroes the region counters and
 * runs gs_forward_geometry's kernel for `view` over the 256-row blocks in which GeomView.reached - as the previous forward
 * blend on these buffers left it - flags no row.  Made to be issued on the stream that carries gs_step_uninstanced, right behind
 * it: the rows of those blocks are final then (phase 2 of gs_backward_step writes parameters only in blocks with a reached row,
 * and only whole float4s of a block's piece: every parameter array must start on 16 bytes), and the previous view's backward
 * blend, chain and phase-2 kernels, which may still be running, read nothing of such a block but its zero flags.  The header and
 * the list cursor are not touched.  `scratch`: the previous forward's geom / img / binning buffers and capacity, with the
 * tile_depth_limit of `view`; `radii`: the array the next gs_forward_geometry will be given (not the previous view's, which its
 * tail still reads).  Then record an event and hand it to that gs_forward_geometry as GsScratch.early_geometry_done - if, and only
 * if, it is called for this very view, rows, buffers, limit table and radii, and nothing wrote the rows in between; otherwise
 * call it as usual: it zeroes the counters again and overwrites every row, the early pass was wasted work.
 * GsView.tile_cull = 2 only, and only while the forward blend fills the flags (GS_REACHED_SPLIT): GS_E_UNSUPPORTED otherwise. */
int gs_forward_geometry_early(const GsView* view, const GsGaussians* g, const GsScratch* scratch, int32_t* radii,
                              void* stream);

/* Stage 2 of gs_backward on its own (parity export): the per-Gaussian chain rule from given sums of the blend
 * backward.  rows [P,16] FLOAT64 (device): mean2D.x, mean2D.y, conic.xx, conic.xy, conic.yy, opacity, r, g, b, depth slot,
 * 4th channel, 5 pad - what stage 1 leaves in the workspace (backward.cu:593-635 accumulates the same ten sums with
 * float atomics; here a tile's fp32 totals are added into float64 slots, so the sums do not depend on the order the
 * tiles arrive in).  depth_mode: 0 none, 1 the depth slot is dL/d(inverse depth) (dr_aa), 2 dL/d(depth) (FSGS generation).
 * Lets a test feed both implementations the SAME sums and so separate the (ill-conditioned)
 * conic -> scale / rotation chain from the accumulation that precedes it.  workspace: as gs_backward (stage 2 keeps its
 * per-Gaussian records there). */
int gs_backward_from_rows(const GsView* view, const GsGaussians* g, const int32_t* radii,
                          const GsScratch* scratch, const double* rows, int32_t depth_mode,
                          const GsGrads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* The order in which the backward blend of this view takes its tiles: 8 * ceil(T/8) entries, entry b = the tile of
 * workgroup b (0xFFFFFFFF: none), per XCD band of the image by decreasing number of list entries the tile visits.  One
 * wave owns a tile and runs at the pace of its dependent instruction chain, so handing out the longest tiles first
 * shortens the kernel's tail (csrc/gs_render_fwd_wave.hip).  The forward blend's cost per tile is nearly the same
 * quantity, unknown before it has run - but a good predictor is the previous view: pass the export back in as
 * GsScratch.tile_order_hint.  out: device, 8 * ceil(T/8) uint32. */
int gs_export_tile_order(const GsScratch* scratch, int32_t W, int32_t H, uint32_t* out, void* stream);

/* Depth-limited emission.  Most (tile, Gaussian) pairs of a trained scene lie behind the depth at which the tile's
 * pixels saturate (forward.cu:326-328 stops there); they are keyed, sorted and stored but never blended.
 * gs_export_tile_stop_depth returns, per tile, the view depth of the list entry at which the last forward on this
 * scratch stopped (+inf: some pixel of the tile never saturated - the whole list matters).  Handed back as
 * GsScratch.tile_depth_limit on the next forward of the same camera, pairs deeper than that (with margin) are not emitted.
 * out: device, gs_tile_depth_limit_floats(W, H) floats: per tile the largest stop depth of its 3 x 3 neighbourhood, then
 * the largest of those per aligned run of four tiles of a row (why: csrc/gs_tilecull.h).  "No limit" = all +inf. */
size_t gs_tile_depth_limit_floats(int32_t W, int32_t H);
int gs_export_tile_stop_depth(const GsScratch* scratch, int32_t W, int32_t H, float* out, void* stream);
/* Asynchronous read-back of the last forward's counters into host memory (pinned for a true async copy):
 * out[0] = instances emitted (num_rendered), out[1] = overflow (binning capacity exceeded: nothing was blended),
 * out[2] = trunc_failed (a depth-limited tile ran out of list entries: outputs invalid, see GsScratch.tile_depth_limit),
 * out[3] = 0, or with GsView.tile_cull = 2 the largest number of Gaussians any 4 x 4-tile region received (the region
 * buckets hold binning_capacity / regions entries each, at most 16 384: a larger value set `overflow` too).  Valid after
 * `stream` has been synchronised.
 * With GsScratch.step_tag set the copy is 12 words: out[8] = *step_tag as the device held it when this call ran, out[9] =
 * GS_STATUS_CHECK(out[8], out[0], out[1], out[2]).  A host that polls out[8] for its tag instead of synchronising must not
 * trust out[0..2] until out[9] matches them: nothing orders the bytes of a device-to-host copy for a concurrent reader. */
#define GS_STATUS_CHECK(tag, num_rendered, overflow, trunc_failed) \
  ((((uint32_t)(tag)) * 2654435761u) ^ (((uint32_t)(num_rendered)) * 40503u) ^ (((uint32_t)(overflow)) << 30) ^ \
   (((uint32_t)(trunc_failed)) << 31) ^ 0x5bd1e995u)
int gs_forward_status(const GsScratch* scratch, uint32_t* out /*[4] or [12] host*/, void* stream);
/* The last kernel of gs_forward_render* on its own (GsScratch.defer_tile_order = 1): same arguments, any stream that is ordered
 * after the render's. */
int gs_forward_tile_order(const GsView* view, const GsScratch* scratch, void* stream);
/* Developer statistics of the last forward on this scratch: what the backward blend's loop meets.  out (device, 8 x u64,
 * zeroed by the caller) += [entries visited, entries with a valid pixel, (entry, quadrant) pairs with a valid pixel,
 * valid (entry, pixel) pairs, tiles with work, list entries of those tiles, 0, 0].  tests/tools/blend_stats.py */
int gs_debug_blend_stats(const GsScratch* scratch, int32_t P, int32_t W, int32_t H, uint64_t* out, void* stream);
/* keys_sorted for the product's lists (the product keeps no tile-key array in any list mode: gs_export_binning returns
 * GS_E_UNSUPPORTED when asked for keys): keys_sorted[i] = (tile << 32 | depth bits) of list entry i, rebuilt from ranges[] and
 * the Gaussians' depths.  tile_cull = 0 / 1: point_list is the reference's, tile after tile.  tile_cull = 2 (region
 * binning): the lists of different tiles lie in point_list in no particular order, inside a tile the order is the reference's. */
int gs_export_binning_region(const GsScratch* scratch, int32_t W, int32_t H, int64_t num_rendered, uint64_t* keys_sorted,
                             uint32_t* point_list, void* stream);
/* Developer entries to the stable LSD radix sort of (u32 key, u32 value) pairs and to the one-workgroup scan behind the depth
 * order, the region partition, the grid encoder's slot sort and the kNN's Morton sort (csrc/gs_binning.hip), run exactly as
 * those callers run them.  tests/test_gpu_sort.py.  Every pointer is a device pointer.
 * tmp: >= gs_debug_sort_tmp_bytes(n_bound) bytes, laid out as the callers' sort buffers; its contents on entry do not matter.
 * The sort handles n = min(*n_dev, n_bound) pairs and orders them stably by the key's bits [0, end_bit) (8-bit passes, or with
 * digit_bits = 9 one 9-bit pass: end_bit <= 9, else GS_E_SHAPE).
 * depth_form = 0: keys / vals (n_bound words each) are copied into half `start_buf` of the ping-pong buffers and sorted.
 * depth_form = 1: vals = NULL; the first pass reads `keys` in place (left untouched), value = index, keys 0xFFFFFFFF are
 * dropped (n_bound > 16 384) or sorted to the tail (the one-workgroup form), *n_kept = number of the others.
 * keys_out / vals_out: n_bound words each of the half the sort ends in - start_buf ^ (passes & 1), start_buf ^ 1 for the 9-bit
 * form -; words at and beyond n are whatever `tmp` held.  digit_totals: NULL, or 512 words: after the 9-bit form the number of
 * keys of every digit.  Returns the sort's own status. */
size_t gs_debug_sort_tmp_bytes(int64_t n_bound);
int gs_debug_sort_pairs(const uint32_t* keys, const uint32_t* vals, const uint32_t* n_dev, int64_t n_bound, int32_t end_bit,
                        int32_t start_buf, int32_t digit_bits, int32_t depth_form, void* tmp, size_t tmp_bytes,
                        uint32_t* keys_out, uint32_t* vals_out, uint32_t* n_kept, uint32_t* digit_totals, void* stream);
/* In-place exclusive scan of sums[0, nb) by one workgroup; the total lands at sums[nb] (device, nb + 1 words). */
int gs_debug_scan_sums(uint32_t* sums, int32_t nb, void* stream);

/* ---- simple-knn ---- */
/* out[i] = mean of the 3 smallest squared distances from point i to the other points.
 * tmp: >= gs_knn_tmp_bytes(P) bytes of device scratch. */
size_t gs_knn_tmp_bytes(int32_t P);
int gs_knn_mean_dist2(const float* xyz /*[P,3]*/, int32_t P, float* out /*[P]*/, void* tmp,
                      size_t tmp_bytes, void* stream);
/* FSGS's fork of simple-knn (FSGS/submodules/simple-knn/simple_knn.cu:132-189, spatial.cu) also returns the three
 * neighbours themselves: nearest[3 i + j] = index of the j-th nearest point of point i (nearest first; ties and
 * the traversal order are the reference's).  nearest == NULL is gs_knn_mean_dist2. */
int gs_knn_mean_dist2_idx(const float* xyz /*[P,3]*/, int32_t P, float* out /*[P]*/,
                          int32_t* nearest /*[P,3]*/, void* tmp, size_t tmp_bytes, void* stream);

/* ---- DNGaussian's input encoders (gridencoder/src/gridencoder.cu, shencoder/src/shencoder.cu), fp32 ----
 * Grid: inputs [B,D] (D 2..5) in [0,1]; embeddings [n_slots,C] (C 1, 2, 4 or 8); offsets [L+1] device int32 (offsets[L] =
 * n_slots, L <= 64); S = log2(per_level_scale); H = base resolution; gridtype 0 = hash, 1 = tiled; interp 0 = linear,
 * 1 = smoothstep.  Level l: scale = exp2(l * S) * H - 1 (the fp32 product l * S, exp2 rounded once to fp32, then fp32
 * arithmetic), resolution = ceil(scale) + 1.  A point with a coordinate outside [0,1] gets zero output, zero dy_dx and no
 * embedding gradient.
 * gs_grid_encode_fwd: outputs [B, L*C]; dy_dx [B,L,D,C] or NULL (what the input gradient needs).
 * gs_grid_encode_bwd: grad [B, L*C]; grad_embeddings [n_slots,C] (every row written, zero where nothing landed; the same
 * bits on every run: a stable sort of the (slot, contribution) pairs and a fixed-order segmented sum) or NULL;
 * grad_inputs [B,D] from dy_dx, or NULL.  tmp: >= gs_grid_encode_tmp_bytes(B, D, L, C, n_slots) bytes of device scratch
 * when grad_embeddings is given.  B * L * 2^D must stay below 2^32.
 * SH: inputs [B,3]; degree 1..8; outputs [B, degree^2] = the Cartesian real SH polynomials (r^2 -> 1 forms, evaluated as
 * written for non-unit inputs); gs_sh_encode_bwd: grad_inputs [B,3] = their gradient against grad [B, degree^2]. */
size_t gs_grid_encode_tmp_bytes(int64_t B, int32_t D, int32_t L, int32_t C, int64_t n_slots);
int gs_grid_encode_fwd(const float* inputs, int64_t B, int32_t D, const float* embeddings, int64_t n_slots, int32_t C,
                       const int32_t* offsets, int32_t L, float S, int32_t H, int32_t gridtype, int32_t align_corners,
                       int32_t interp, float* outputs, float* dy_dx, void* stream);
int gs_grid_encode_bwd(const float* grad, const float* inputs, int64_t B, int32_t D, int64_t n_slots, int32_t C,
                       const int32_t* offsets, int32_t L, float S, int32_t H, int32_t gridtype, int32_t align_corners,
                       int32_t interp, const float* dy_dx, float* grad_embeddings, float* grad_inputs, void* tmp,
                       size_t tmp_bytes, void* stream);
int gs_sh_encode_fwd(const float* inputs, int64_t B, int32_t degree, float* outputs, void* stream);
int gs_sh_encode_bwd(const float* grad, const float* inputs, int64_t B, int32_t degree, float* grad_inputs, void* stream);

/* ---- DNGaussian's depth-normalisation regulariser (utils/loss_utils.py: patch_norm_{mse,l1}_loss[_global],
 * loss_depth_smoothness), fp32, one [1,1,H,W] image ----
 * Patches: non-overlapping p x p (2 <= p <= min(H, W)), stride p, rows / columns beyond floor(H/p) p, floor(W/p) p dropped;
 * L = floor(H/p) floor(W/p) patches in row-major patch order, elements row-major inside a patch (the order of mask_out).
 * n(x) = (x - patch mean) / (s + 1e-2 std_all): std_all = unbiased std of the L p^2 patchified elements (carries gradient);
 * s = the patch's unbiased std (carries gradient), or with GS_DN_GLOBAL the unbiased std of the whole uncropped image
 * (detached).  d = n(input) - n(target), mask = |d| > margin; loss = mean over the mask of d^2 (GS_DN_L1: |d|): NaN on an
 * empty mask, and then a zero gradient.  The gradient goes to input only.
 * tmp: >= gs_depth_norm_tmp_bytes(H, W, p_local, p_global) bytes of device scratch (0 = that term is absent); a single-loss
 * call sizes it with (p, 0) whatever its form, the smoothness pair with (0, 0).  The forward leaves in tmp what the backward
 * of the SAME arguments reads; the backward is one launch and reads dL/dloss from device memory (no host synchronisation
 * anywhere, every sum in one fixed order: the same bits on every run).
 * gs_depth_smooth_*: loss = (sum |dx depth| wx + sum |dy depth| wy) / (sum wx + sum wy), wx = exp(-mean_c |dx img|), img [C,H,W].
 * gs_dng_depth_reg_*: the reference's call in one pass structure: w_local * mse(p_local) + w_smooth * smoothness(input,
 * target) + w_global * mse_global(p_global), both with `margin`; loss_out[4] = total, local, global, smoothness (0 when
 * w_smooth == 0: the term is skipped); mask_local / mask_global nullable. */
#define GS_DN_GLOBAL 1
#define GS_DN_L1 2
size_t gs_depth_norm_tmp_bytes(int32_t H, int32_t W, int32_t p_local, int32_t p_global);
int gs_depth_norm_fwd(const float* input, const float* target, int32_t H, int32_t W, int32_t p, float margin, int32_t flags,
                      void* tmp, float* loss_out, uint8_t* mask_out /*[L p^2] or NULL*/, void* stream);
int gs_depth_norm_bwd(const float* input, const float* target, int32_t H, int32_t W, int32_t p, float margin, int32_t flags,
                      const void* tmp, const float* dloss_dev, float* grad_input /*[H,W]*/, void* stream);
int gs_depth_smooth_fwd(const float* depth, const float* img, int32_t C, int32_t H, int32_t W, void* tmp, float* loss_out,
                        void* stream);
int gs_depth_smooth_bwd(const float* depth, const float* img, int32_t C, int32_t H, int32_t W, const void* tmp,
                        const float* dloss_dev, float* grad_depth /*[H,W]*/, void* stream);
int gs_dng_depth_reg_fwd(const float* input, const float* target, int32_t H, int32_t W, int32_t p_local, int32_t p_global,
                         float margin, float w_local, float w_global, float w_smooth, void* tmp, float* loss_out /*[4]*/,
                         uint8_t* mask_local, uint8_t* mask_global, void* stream);
int gs_dng_depth_reg_bwd(const float* input, const float* target, int32_t H, int32_t W, int32_t p_local, int32_t p_global,
                         float margin, float w_local, float w_global, float w_smooth, const void* tmp, const float* dloss_dev,
                         float* grad_input /*[H,W]*/, void* stream);

/* ---- FSGS's depth-correlation term (FSGS/train.py:100-109,121-131; csrc/gs_pearson.hip) ----
 * Pearson's r of two fp32 sequences of n >= 2 elements, r = Sxy / sqrt(Sxx Syy) clamped to [-1, 1], and the loss 1 - r.  The
 * second sequence is derived from the target t inside the kernel by a FORM: y = t (ID), -t (NEG), 1 / (t + 200) in fp32
 * (RECIP200).  A forward serves form_a and, unless form_b is -1, form_b from one read of x and t, and picks the branch on the
 * device by the rule of Python's min(loss_a, loss_b): b only if loss_b < loss_a, so a tie or a NaN keeps a.
 * out[4] = loss of the chosen form, its r, loss_a, loss_b (NaN without form_b); branch_out (nullable) = 0 / 1.
 * A constant sequence (Sxx or Syy = 0) gives a NaN loss and zero gradients.
 * tmp: >= gs_pearson_tmp_bytes(n) bytes of device scratch (0: n out of range).  The forward (two launches) leaves in tmp what the
 * backward of the SAME arguments reads.  The backward is one launch: dout_dev is dL/dloss of the chosen form, or dL/dr with
 * GS_PEARSON_WRT_R, read from device memory; grad_x and grad_t are each nullable, not both; the gradient to t goes through
 * the form's derivative and exists for ID and NEG only (GS_E_UNSUPPORTED with RECIP200).  The clamp does not gate the gradient.
 * No host synchronisation anywhere and every sum in one fixed order: the same bits on every run.  The sums are float64 sums of
 * the values shifted by the sequences' first elements.  A workgroup sweeps GS_PEARSON_BLOCK_ELEMS elements at a time, the grid
 * is at most GS_PEARSON_MAX_BLOCKS workgroups and strides over what is left. */
#define GS_PEARSON_ID 0
#define GS_PEARSON_NEG 1
#define GS_PEARSON_RECIP200 2
#define GS_PEARSON_WRT_R 1
#define GS_PEARSON_BLOCK_ELEMS 4096
#define GS_PEARSON_MAX_BLOCKS 512
size_t gs_pearson_tmp_bytes(int64_t n);
int gs_pearson_fwd(const float* x, const float* t, int64_t n, int32_t form_a, int32_t form_b /* -1: none */, void* tmp,
                   float* out /*[4]*/, int32_t* branch_out, void* stream);
int gs_pearson_bwd(const float* x, const float* t, int64_t n, int32_t form_a, int32_t form_b, int32_t flags, const void* tmp,
                   const float* dout_dev, float* grad_x /*[n]*/, float* grad_t /*[n]*/, void* stream);

/* ---- DNGaussian's neural colour and opacity heads (scene/neural_renderer.py, GridRenderer; csrc/gs_mlp.hip) ----
 * Two bias-free ReLU MLPs on per-Gaussian encodings, each direction ONE fused launch on the f32 MFMA:
 *   sigma_net  enc_x [B,32] -> 64 -> 64 -> 65: column 0 = sigma [B], columns 1..64 = geo_feat
 *   color_net  [enc_d [B,16] | geo_feat] -> 64 -> 3, color [B,3] = sigmoid(.) * 1.002 - 0.001
 * Weights in torch.nn.Linear layout [out,in], contiguous fp32: w_s0 [64,32], w_s1 [64,64], w_s2 [65,64], w_c0 [64,80],
 * w_c1 [3,64].  No activation ever reaches device memory.
 * Forward: enc_d = color = NULL is the sigma-only form (w_c0 / w_c1 are then not read); otherwise both are required.
 * Backward: recomputes the forward.  g_sigma [B] and g_color [B,3] are each nullable (= zero); g_enc_x [B,32], g_enc_d [B,16]
 * and the weight gradients are nullable outputs and a NULL output is not computed; the weight gradients are requested all
 * together (three in the sigma-only form enc_d = NULL, else five).  They need tmp: >= gs_dng_heads_tmp_bytes(B) bytes of
 * device scratch, one partial per workgroup, added in workgroup order by a second small launch: no atomics, the same bits on
 * every run.  ReLU'(0) = 0.  A workgroup takes GS_DNG_HEADS_TILE_ROWS rows at a time; the backward's grid is at most
 * GS_DNG_HEADS_MAX_BLOCKS workgroups, which stride over what is left (the forward: as many for the colour form, twice as many
 * for the sigma-only form).  max_blocks > 0 caps either grid further (0: no cap; tests use it to make every workgroup take
 * several tiles of a small batch); it changes the order in which the weight gradients are summed, nothing else.
 * GS_E_NULL: a required pointer is missing; GS_E_SHAPE: B < 0, max_blocks < 0, or tmp_bytes smaller than B needs.  B = 0: returns 0, the forward
 * launches nothing, the backward zeroes the weight gradients.  Everything is enqueued on `stream`; no host synchronisation. */
#define GS_DNG_ENC_X 32
#define GS_DNG_ENC_D 16
#define GS_DNG_HIDDEN 64
#define GS_DNG_GEO 64
#define GS_DNG_HEADS_TILE_ROWS 128
#define GS_DNG_HEADS_MAX_BLOCKS 256
size_t gs_dng_heads_tmp_bytes(int64_t B);
int gs_dng_heads_fwd(const float* enc_x, const float* enc_d, int64_t B, const float* w_s0, const float* w_s1, const float* w_s2,
                     const float* w_c0, const float* w_c1, float* sigma /*[B]*/, float* color /*[B,3]*/, int32_t max_blocks,
                     void* stream);
int gs_dng_heads_bwd(const float* enc_x, const float* enc_d, int64_t B, const float* w_s0, const float* w_s1, const float* w_s2,
                     const float* w_c0, const float* w_c1, const float* g_sigma, const float* g_color, float* g_enc_x,
                     float* g_enc_d, float* g_w_s0, float* g_w_s1, float* g_w_s2, float* g_w_c0, float* g_w_c1, void* tmp,
                     size_t tmp_bytes, int32_t max_blocks, void* stream);

/* ---- DNGaussian's per-Gaussian regulariser, view directions and near-camera mask (csrc/gs_dng_reg.hip) ----
 * Regulariser over scaling [P,3] (positive) and opacity [P] (in (0,1)), P >= 1, fp32:
 *   mx_i / mn_i = row max / min of scaling (a tie goes to the lowest column), H = {o_i > 0.2f}, L = {o_i < 0.2f}
 *   shape = mean mx_i / mn_i, scale = mean mx_i^2, opa = 1 - mean_H o_i^2 + mean_L (1 - o_i)^2,
 *   total = w_shape shape + w_scale scale + w_opa opa;      out[4] = shape, scale, opa, total
 * Each ratio and square is taken in fp32, the sums are float64 in one fixed order (the same bits on every run).  o_i == 0.2f is
 * in neither set; an empty set makes opa and total NaN while every gradient element stays finite.
 * GS_DNG_REG_RAW: scaling and opacity are the model's raw rows, s = exp(.), o = sigmoid(.) are evaluated in the kernel and the
 * gradients are with respect to the raw values; no activated tensor is written.
 * Forward: two launches; a workgroup sweeps GS_DNG_REG_BLOCK_ROWS rows at a time, the grid is at most GS_DNG_REG_MAX_BLOCKS
 * workgroups (max_blocks > 0 caps it further, 0: no cap; tests use it to make a small P stride) and strides over what is left.
 * tmp: >= gs_dng_reg_tmp_bytes(P) bytes of device scratch (0: P out of range); the forward leaves in it what the backward of the
 * SAME arguments reads.  Backward: one launch.  g_terms [3] = dL/d(shape, scale, opa) and g_total [1] = dL/dtotal are read
 * from device memory, each nullable (= zero), not both; g_scaling [P,3] (every column written, nothing to zero beforehand) and
 * g_opacity [P] are each nullable (that half is skipped), not both.
 * gs_view_dirs_*: out_i = (x_i - c) / |x_i - c| for xyz [P,3] and campos [3] (device memory); the backward gives
 * g_xyz_i = (g_i - n_i (n_i . g_i)) / |x_i - c|, nothing to campos.  A row at the camera centre is NaN.
 * gs_near_mask: mask_i (one byte, 0 / 1) = OR_k (|x_i - c_k| < near) for centers [K,3] (device memory), K >= 1, norm in fp32.
 * One launch each.  GS_E_NULL: a required pointer is missing; GS_E_SHAPE: P < 1, K < 1, P out of range, max_blocks < 0 or an
 * unknown flag.  Everything is enqueued on `stream`; no host synchronisation, no atomics. */
#define GS_DNG_REG_RAW 1
#define GS_DNG_REG_BLOCK_ROWS 1024
#define GS_DNG_REG_MAX_BLOCKS 1024
size_t gs_dng_reg_tmp_bytes(int64_t P);
int gs_dng_reg_fwd(const float* scaling, const float* opacity, int64_t P, double w_shape, double w_scale, double w_opa,
                   int32_t flags, int32_t max_blocks, void* tmp, float* out /*[4]*/, void* stream);
int gs_dng_reg_bwd(const float* scaling, const float* opacity, int64_t P, int32_t flags, const void* tmp, const float* g_terms,
                   const float* g_total, float* g_scaling /*[P,3]*/, float* g_opacity /*[P]*/, void* stream);
int gs_view_dirs_fwd(const float* xyz, const float* campos, int64_t P, float* out /*[P,3]*/, void* stream);
int gs_view_dirs_bwd(const float* xyz, const float* campos, int64_t P, const float* g /*[P,3]*/, float* g_xyz /*[P,3]*/,
                     void* stream);
int gs_near_mask(const float* xyz, int64_t P, const float* centers, int32_t K, float near, uint8_t* mask /*[P]*/, void* stream);

/* ---- what DNGaussian's DTU loop adds: object mask, masked-mean fill, alpha penalty, colour rules (csrc/gs_dng_dtu.hip) ----
 * Additive entries (GS_ABI_VERSION unchanged).  fp32 images of n = H W elements, 1 <= n < 2^31; masks are one byte per element,
 * 0 / non-zero.  Every count stays in device memory; no atomics, no host synchronisation, the same bits on every run.
 * gs_dtu_mask: gt [3,H,W]; dark = every channel < thr (fp32, strictly); mask[y,x] = 1 iff the run of dark pixels ending at (y,x)
 *   going up its column is at least min(y + 1, run) long (run >= 1; train_dtu.py:84-94 has run = 50).  count[0] (int32) = masked
 *   pixels; gt_out [3,H,W] = gt with the masked pixels 0 in every channel, and may be gt itself.  One launch, one workgroup.
 * gs_masked_fill_fwd: out = x where mask == 0, else mean of x over mask == 0: the float64 sum of per-workgroup partials, added
 *   in index order, over the float64 count, rounded to fp32 once (no unmasked element: NaN).  mean_out [1], nullable, receives
 *   it too.  tmp: >= gs_masked_tmp_bytes(n) bytes of device scratch.  Two launches.  gs_masked_fill_bwd: g_x = g where
 *   mask == 0, +0.0 where masked (nothing flows through the mean).  One launch.
 * gs_alpha_penalty_fwd: out[0] = mean of alpha^2 over mask != 0, squares and sum in float64 in the same fixed order, rounded
 *   once; an empty mask gives NaN.  Two launches; tmp (gs_masked_tmp_bytes(n)) keeps the count for the backward of the SAME
 *   arguments.  gs_alpha_penalty_bwd: g [1] from device memory; g_alpha = (g / (float)count) * (2 * alpha) in fp32 where masked,
 *   +0.0 elsewhere; count 0: +0.0 everywhere.  One launch.
 * gs_dng_colour_rule (train_dtu.py:218-230): colour [P,3] read-only, stat [P] and opacity [P] (the raw row) edited in place.  The
 *   black rule fires on a row when max_c < black_thr, the white rule when min_c > white_thr (strict, fp32; a NaN colour fires
 *   neither); a rule that fires divides stat by its divisor in fp32 and, if its reset flag is set, stores `value` into opacity.
 *   Black is applied before white; *_on = 0 switches a rule off.  counts[2] (int32) = rows the black / the white rule fired on.
 *   One launch.
 * GS_E_NULL: a required pointer is missing; GS_E_SHAPE: H, W, run or P < 1, or n / P >= 2^31. */
int gs_dtu_mask(const float* gt, int32_t H, int32_t W, float thr, int32_t run, uint8_t* mask /*[H,W]*/, int32_t* count /*[1]*/,
                float* gt_out /*[3,H,W]*/, void* stream);
size_t gs_masked_tmp_bytes(int64_t n);
int gs_masked_fill_fwd(const float* x, const uint8_t* mask, int64_t n, void* tmp, float* out /*[n]*/, float* mean_out /*[1]*/,
                       void* stream);
int gs_masked_fill_bwd(const float* g, const uint8_t* mask, int64_t n, float* g_x /*[n]*/, void* stream);
int gs_alpha_penalty_fwd(const float* alpha, const uint8_t* mask, int64_t n, void* tmp, float* out /*[1]*/, void* stream);
int gs_alpha_penalty_bwd(const float* alpha, const uint8_t* mask, int64_t n, const void* tmp, const float* g /*[1]*/,
                         float* g_alpha /*[n]*/, void* stream);
int gs_dng_colour_rule(const float* colour, float* stat, float* opacity, int64_t P, int32_t black_on, float black_thr,
                       float black_div, int32_t black_reset, int32_t white_on, float white_thr, float white_div,
                       int32_t white_reset, float value, int32_t* counts /*[2]*/, void* stream);

/* ---- what DNGaussian's Blender loops add for a white background: target and white rules (csrc/gs_dng_blender.hip) ----
 * Additive entries (GS_ABI_VERSION unchanged).  Every count stays in device memory; no floating-point atomics, no host
 * synchronisation, the same bits on every run.  1 <= H W < 2^31, 1 <= P < 2^31.
 * gs_blender_target (train_blender.py:87, :96-97): gt [3,H,W]; mask[y,x] = 1 iff the minimum over the three channels > thr
 *   (fp32, strictly; a NaN channel leaves the pixel unmasked).  target [H,W], nullable, = +0.0 where masked, else
 *   255.0f - mono (one fp32 subtraction); mono [H,W] is required only with target.  count[0] (int32) = masked pixels, from
 *   per-workgroup partials in tmp (>= gs_blender_tmp_bytes(H W) bytes of device scratch).  Two launches.  The outputs alias no
 *   input.
 * gs_dng_white_rule (:207-211): colour [P,3] read-only, stat [P] and opacity [P] (the raw row) edited in place.  A row fires iff
 *   min_c colour > thr (strict, fp32; a NaN fires nothing); it gets stat = +0.0 and opacity = log(x / (1 - x)) with
 *   x = factor * sigmoid(opacity), evaluated in double from the fp32 input and rounded once (-inf gives -inf, NaN gives NaN).
 *   counts[0] (int32) = rows that fired.  One kernel launch behind a 4-byte hipMemsetAsync of counts on the same stream: every
 *   workgroup adds its count with one INTEGER atomic add (order-free); there is no floating-point atomic.
 * gs_dng_white_rule_sh (:366-370): the same rule on colour = max(eval_sh(active_degree, rows, dir) + 0.5, 0),
 *   dir = (xyz - campos) normalised, evaluated in double from the fp32 inputs and rounded once (a zero-length direction: NaN
 *   colours, nothing fires - from degree 1 on; degree 0 does not use the direction).  The rows of M = 1, 4, 9 or 16 coefficients come split - dc [P,1,3] and rows = rest [P,M-1,3]
 *   (ignored when M == 1) - or packed: dc null and rows [P,M,3].  Coefficients above the active degree are not read.
 *   colour_out [P,3], nullable, receives the colour.  Counted and launched as gs_dng_white_rule.
 * GS_E_NULL: a required pointer is missing; GS_E_SHAPE: H, W or P < 1, H W or P >= 2^31, M not 1 / 4 / 9 / 16, active_degree < 0 or > 3
 *   or (active_degree + 1)^2 > M.  Every check precedes the first launch.  A failed memset
 *   returns its hipError_t (> 0), as a failed launch does. */
size_t gs_blender_tmp_bytes(int64_t n);
int gs_blender_target(const float* gt, const float* mono, int32_t H, int32_t W, float thr, void* tmp, uint8_t* mask /*[H,W]*/,
                      int32_t* count /*[1]*/, float* target /*[H,W]*/, void* stream);
int gs_dng_white_rule(const float* colour, float* stat, float* opacity, int64_t P, float thr, float factor, int32_t* counts /*[1]*/,
                      void* stream);
int gs_dng_white_rule_sh(const float* xyz, const float* dc, const float* rows, int32_t M, int32_t active_degree, const float* campos,
                         float* stat, float* opacity, int64_t P, float thr, float factor, float* colour_out /*[P,3]*/,
                         int32_t* counts /*[1]*/, void* stream);

/* ---- losses (images are [C,H,W] or [N,C,H,W] contiguous fp32) ---- */

/* sums[0] = sum |a-b| over n elements (atomically added: zero it first).
 * grad (may be NULL) = coef * sign(a-b). */
int gs_l1_fwd(const float* a, const float* b, int64_t n, float* sum, void* stream);
int gs_l1_bwd(const float* a, const float* b, int64_t n, float coef, float* grad_a,
              int32_t accumulate, void* stream);

/* One level of the Haar analysis ('db1', mode 'symmetric': odd sizes repeat the last sample).
 * x [NC,H,W] -> ll, lh, hl, hh each [NC, ceil(H/2), ceil(W/2)].  lh = low along W, high along H. */
int gs_dwt_haar_fwd(const float* x, int32_t NC, int32_t H, int32_t W, float* ll, float* lh,
                    float* hl, float* hh, void* stream);
/* adjoint: dx [NC,H,W] (=, not +=) from the four band gradients (any may be NULL = zero). */
int gs_dwt_haar_bwd(const float* dll, const float* dlh, const float* dhl, const float* dhh,
                    int32_t NC, int32_t H, int32_t W, float* dx, void* stream);

/* Fused global 2-level DWT L1 loss (train.py:132-164).
 * band_sums[8] += sum |band(pred) - band(gt)| for LL1,LH1,HL1,HH1,LL2,LH2,HL2,HH2 (zero first).
 * counts: level-1 bands have C*ceil(H/2)*ceil(W/2) elements, level-2 C*ceil(h1/2)*ceil(w1/2). */
int gs_dwt2_l1_fwd(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W,
                   float* band_sums, void* stream);
/* grad_pred (+= if accumulate) = sum_b coef[b] * DWT_b^T sign(band_b(pred-gt)); coef is a
 * DEVICE array of 8 floats (w_b * upstream / N_b). */
int gs_dwt2_l1_bwd(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W,
                   const float* coef_dev, float* grad_pred, int32_t accumulate, void* stream);

/* ELF map (loss_utils.py:336-366): elf_low = LL/(LL+LH+HL+HH+1e-8) with per-pixel channel-L1
 * of the level-1 bands, then bilinear x2 upsample (align_corners=False) to [H,W]. */
int gs_elf_map(const float* img, int32_t C, int32_t H, int32_t W, float* elf_low /*[h1,w1] tmp*/,
               float* elf /*[H,W]*/, void* stream);
/* means[L] = mean of elf over each non-overlapping patch (row-major patch order, remainder
 * dropped: F.unfold semantics, loss_utils.py:391-400). */
int gs_patch_means(const float* elf, int32_t H, int32_t W, int32_t patch, float* means,
                   void* stream);
/* Patch DWT loss over the selected patches (mask[L] != 0): sums[3] += sum |band(pred-gt)| for
 * LH1, HL1, HH1 restricted to selected patches (zero first). */
int gs_patch_dwt_fwd(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W,
                     int32_t patch, const uint8_t* mask, float* sums, void* stream);
int gs_patch_dwt_bwd(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W,
                     int32_t patch, const uint8_t* mask, const float* coef_dev /*[3]*/,
                     float* grad_pred, int32_t accumulate, void* stream);

/* Fused SSIM, 11-tap sigma=1.5 separable window, zero padding ("same").
 * img1,img2 [B,C,H,W]; ssim_map and the three partial-derivative maps (may be NULL when no
 * backward is wanted) have the same shape. */
int gs_ssim_fwd(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H, int32_t W,
                float C1, float C2, float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq,
                float* dm_dsigma12, void* stream);
int gs_ssim_bwd(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H, int32_t W,
                float C1, float C2, const float* dL_dmap, const float* dm_dmu1,
                const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1,
                void* stream);

/* ---- fused form of the LGDWT-GS criterion (LGDWT-GS/train.py:128-202): the per-term kernels above with
 * device-resident coefficients, one shared image-gradient buffer, SSIM's mean and the clamp(0,1) backward folded
 * in, and the loss composition itself (running-mean DWT scale included) done by one tiny kernel instead of
 * host arithmetic on .item() values. ---- */
int gs_l1_bwd_dev(const float* a, const float* b, int64_t n, const float* coef_dev /*[1]*/, float* grad_a,
                  int32_t accumulate, void* stream);
/* gs_l1_fwd + gs_dwt2_l1_fwd from ONE read of the two images: l1_sum[0] += sum |pred - gt|, band_sums[8] as
 * gs_dwt2_l1_fwd; and their two backward kernels as one write of the gradient image:
 * grad_pred (+= if accumulate) = l1_coef_dev[0] * sign(pred - gt) + the gs_dwt2_l1_bwd term. */
int gs_l1_dwt2_fwd(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W, float* l1_sum,
                   float* band_sums, void* stream);
/* gs_l1_dwt2_fwd on clamp(raw, 0, 1), which is also written to clamped_out [C,H,W] (the clamp of
 * gaussian_renderer/__init__.py:119 without a pass of its own).  H and W multiples of 4 and 16-byte aligned planes, else
 * GS_E_UNSUPPORTED (clamp first and call gs_l1_dwt2_fwd). */
int gs_l1_dwt2_fwd_clamp(const float* raw, const float* gt, int32_t C, int32_t H, int32_t W, float* l1_sum,
                         float* band_sums, float* clamped_out, void* stream);
/* gs_l1_dwt2_fwd_clamp and gs_patch_dwt_fwd in one pass, gs_l1_dwt2_bwd and gs_patch_dwt_bwd in one: the patch term's sums
 * are the level-1 LH / HL / HH differences of the same 2 x 2 blocks, restricted to the selected patches (mask [H/ps * W/ps],
 * loss_utils.py:395-442), and its gradient rides on the same band signs.  patch_sums[3] +=; patch_coef_dev[3] as coef_dev of
 * gs_patch_dwt_bwd.  H, W and ps multiples of 4 and 16-byte aligned planes, else GS_E_UNSUPPORTED (use the separate calls). */
int gs_l1_dwt2_patch_fwd_clamp(const float* raw, const float* gt, int32_t C, int32_t H, int32_t W, int32_t ps,
                               const uint8_t* mask, float* l1_sum, float* band_sums, float* patch_sums,
                               float* clamped_out, void* stream);
int gs_l1_dwt2_patch_bwd(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W, int32_t ps,
                         const uint8_t* mask, const float* l1_coef_dev /*[1]*/, const float* coef_dev /*[8]*/,
                         const float* patch_coef_dev /*[3]*/, float* grad_pred, int32_t accumulate, void* stream);
int gs_l1_dwt2_bwd(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W,
                   const float* l1_coef_dev /*[1]*/, const float* coef_dev /*[8]*/, float* grad_pred,
                   int32_t accumulate, void* stream);
/* Order-independent sums (round 4).  The *_fwd kernels above add each workgroup's sums to their targets with float atomics:
 * the totals then depend, in the last bits, on the order in which the workgroups finish.  These forms store the
 * workgroups' sums instead - partials[12 w + k] for workgroup w of gs_l1_dwt2_patch_fwd_clamp_p (k: 0..7 the band sums,
 * 8 the L1 sum, 9..11 the patch sums; gs_dwt_partials_count(C, H, W) rows; ps = 0 / mask = NULL: no patch term),
 * partials[w] for gs_l1_fwd_p (gs_l1_partials_count(n) entries) - and gs_lgdwt_combine_pp adds them to sums[] in index
 * order before it composes the loss: two runs of a train step give the same bits (tests/test_gpu_fused_step.py).
 * H, W (and ps) multiples of 4, 16-byte aligned planes, else GS_E_UNSUPPORTED (use the atomic forms). */
int64_t gs_dwt_partials_count(int32_t C, int32_t H, int32_t W);
int gs_l1_dwt2_patch_fwd_clamp_p(const float* raw, const float* gt, int32_t C, int32_t H, int32_t W, int32_t ps,
                                 const uint8_t* mask, float* partials, float* clamped_out, void* stream);
int64_t gs_l1_partials_count(int64_t n);
int gs_l1_fwd_p(const float* a, const float* b, int64_t n, float* partials, void* stream);
/* Depth regularisation of the step (LGDWT-GS/train.py:204-216): Ll1depth_pure = mean |(invDepth - mono_invdepth) * depth_mask|
 * over the n pixels of the rasterizer's inverse-depth output.  One pass gives both halves (either pointer may be NULL, not
 * both): partials[w] = workgroup w's sum of |(d - m) k| (gs_depth_l1_partials_count(n) entries; the caller adds them in
 * index order and divides by n), and grad[i] = coef * (coef_dev ? coef_dev[0] : 1) * sign((d - m) k) * k - the gradient of
 * weight * mean with coef = weight / n (sign(0) = 0 as torch.abs has it).  mask NULL: all ones.  grad is what
 * gs_backward* takes as dL_dinvdepth. */
int64_t gs_depth_l1_partials_count(int64_t n);
int gs_depth_l1(const float* invdepth, const float* mono_invdepth, const float* mask, int64_t n, float* partials, float coef,
                const float* coef_dev, float* grad, void* stream);
/* like gs_ssim_fwd but returns sum(ssim_map) (+=, zero it first) instead of the map.  One atomic per workgroup on
 * sum_out: prefer gs_ssim_fwd_partials below for large images (the atomics serialise: 98 vs 59 us at 1080p). */
int gs_ssim_fwd_sum(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H, int32_t W, float C1,
                    float C2, float* sum_out, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
                    void* stream);
/* gs_ssim_fwd_sum without the atomic: workgroup w of the launch stores its share of sum(ssim_map) to partials[w]
 * (gs_ssim_partials_count() of them, all written); gs_lgdwt_combine_p adds them to sums[1] in a fixed order.
 * (One device-scope atomic per workgroup on ONE address is serialised at ~14 ns each on MI355X: 86 us at 1080p.) */
int64_t gs_ssim_partials_count(int32_t B, int32_t C, int32_t H, int32_t W);
int gs_ssim_fwd_partials(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H, int32_t W, float C1,
                         float C2, float* partials, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
                         void* stream);
/* like gs_ssim_bwd with dL_dmap == coef_dev[0] everywhere; optionally adds to dL_dimg1 and then zeroes the
 * result where clamp_src (the un-clamped render) lies outside [0,1].  With clamp_src given, img1 must be
 * clamp(clamp_src, 0, 1) - the kernel then forms it from clamp_src instead of reading img1. */
int gs_ssim_bwd_uniform(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H, int32_t W,
                        const float* coef_dev, const float* dm_dmu1, const float* dm_dsigma1_sq,
                        const float* dm_dsigma12, float* dL_dimg1, int32_t accumulate, const float* clamp_src,
                        void* stream);
typedef struct GsLgdwtParams {
  float lambda_dssim;        /* 0.2 */
  float n_pix;               /* C*H*W */
  float n_band1, n_band2;    /* elements per level-1 / level-2 band */
  float dwt_w[8];            /* LL1 LH1 HL1 HH1 LL2 LH2 HL2 HH2 */
  float patch_w[3];          /* w_lh, w_hl, (w_lh+w_hl)/2 */
  float patch_weight;        /* beta = 0.1 */
  float patch_elems_per_sel; /* C * (patch/2)^2 */
  int32_t dwt_enable, patch_enable;
  int32_t reset_sums;        /* 1: the call zeroes sums[0..12] after it has read them (the accumulators of the next view:
                                a caller that keeps ONE sums buffer per camera, word 13 preset, then needs no fill kernel) */
  int32_t custom_base;       /* 1: base = w_l1 * L1 + w_ssim * (1 - SSIM) instead of (1 - lambda) L1 + lambda (1 - SSIM): the NIR
                                term of mult-dwtgs/train_nir.py:96-104 (nir_weight * (L1 + 0.2 (1 - SSIM)),
                                mult-dwtgs/utils/loss_utils.py:93-144) through the same kernels */
  float w_l1, w_ssim;
} GsLgdwtParams;
/* sums[16]: 0 l1 | 1 ssim | 2..9 bands | 10..12 patch | 13 selected patches.  running_mean: device scalar,
 * updated in place (train.py:193-195).  out[24]: 0 loss 1 base 2 dwt 3 patch 4 dwt_scale 5 l1 6 ssim 7 the running mean
 * before the call;
 * 8 c_l1, 9 c_ssim, 10..17 c_band, 18..20 c_patch = dLoss/d(term sum). */
int gs_lgdwt_combine(const float* sums, float* running_mean, const GsLgdwtParams* params /*host*/, float* out,
                     void* stream);
/* the same with the SSIM sum given as sums[1] + sum(ssim_partials[0..n_partials)) */
int gs_lgdwt_combine_p(const float* sums, const float* ssim_partials, int64_t n_partials, float* running_mean,
                       const GsLgdwtParams* params /*host*/, float* out, void* stream);
/* ... and with the DWT / L1 / patch sums given as sums[] + the per-workgroup partials of gs_l1_dwt2_patch_fwd_clamp_p
 * (n_dwt rows of 12) and of gs_l1_fwd_p (n_l1 entries), added in index order */
int gs_lgdwt_combine_pp(const float* sums, const float* ssim_partials, int64_t n_partials, const float* dwt_partials,
                        int64_t n_dwt, const float* l1_partials, int64_t n_l1, float* running_mean,
                        const GsLgdwtParams* params /*host*/, float* out, void* stream);
/* The criterion with the clamped image never written, for [C,H,W] images.  gs_lgdwt_fused_fwd = gs_l1_dwt2_patch_fwd_clamp_p
 * (clamped_out not written; dwt_partials: gs_dwt_partials_count(C, H, W) rows of 12, the same bits) + gs_ssim_fwd_partials on
 * clamp(raw, 0, 1) (ssim_partials: gs_ssim_partials_count(1, C, H, W); the same maps and partials bit for bit); add them up
 * with gs_lgdwt_combine_pp.  gs_lgdwt_fused_bwd writes grad once, bit for bit what gs_l1_dwt2_patch_bwd (mask given; or
 * gs_l1_dwt2_bwd with flags & 2; or gs_l1_bwd_dev) followed by gs_ssim_bwd_uniform accumulating onto it write, with
 * img = flags & 1 ? clamp(raw, 0, 1) : raw; coef_dev = out[8..23] of the combine (c_l1, c_ssim, c_band x8, c_patch x3);
 * flags & 4 zeroes the result where raw lies outside [0, 1] (clamp_src of gs_ssim_bwd_uniform).
 * H, W (and ps) multiples of 4 and 16-byte aligned planes, else GS_E_UNSUPPORTED (use the separate calls). */
int gs_lgdwt_fused_fwd(const float* raw, const float* gt, int32_t C, int32_t H, int32_t W, float C1, float C2, int32_t ps,
                       const uint8_t* mask, float* dwt_partials, float* ssim_partials, float* dm_dmu1, float* dm_dsigma1_sq,
                       float* dm_dsigma12, void* stream);
int gs_lgdwt_fused_bwd(const float* raw, const float* gt, int32_t C, int32_t H, int32_t W, int32_t flags, int32_t ps,
                       const uint8_t* mask, const float* coef_dev, const float* dm_dmu1, const float* dm_dsigma1_sq,
                       const float* dm_dsigma12, float* grad, void* stream);

/* ---- optimiser (caller side of the path): fused Adam over ONE flat fp32 parameter buffer.
 * Replaces torch.optim.Adam(lr=0, eps=1e-15) with per-group learning rates,
 * LGDWT-GS/scene/gaussian_model.py:183-193 + train.py:279-288.  Segment k covers elements [begin, end);
 * element i uses lr_a, or lr_b when period > 0 and (i - begin) % period >= split (interleaved SH DC / rest).
 * step: the segment's own 1-based step count for the bias correction, 0 = the call's `step` (torch keeps the
 * counter per parameter: a group whose tensor was just replaced - reset_opacity, gaussian_model.py:258-261 - has
 * no gradient that iteration, is skipped by optimizer.step() and falls one step behind the others).
 * Elements covered by no segment are left untouched (parameter AND moments). */
typedef struct GsAdamSeg {
  int64_t begin, end;
  float lr_a, lr_b;
  int32_t period, split;
  int32_t step;
  int32_t row_width; /* gs_adam_step_masked: floats per Gaussian in this segment (element i belongs to row (i - begin) / row_width);
                        0: the segment is not masked */
} GsAdamSeg;
/* segs is a HOST array (<= 8 entries, copied into the launch); step = 1-based iteration for the bias correction. */
int gs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                 const GsAdamSeg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                 void* stream);
/* the same, but a no-op on the device when *gate != 0 (gate: device float, may be NULL = gs_adam_step): the data-parallel
 * step passes the all-reduced GsStepState.fail_flag - if any rank rendered from lists that proved too short, no replica
 * steps, and every rank repeats the step once its host has seen the flag */
int gs_adam_step_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                       const GsAdamSeg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                       const float* gate, void* stream);
/* "sparse_adam" (LGDWT-GS/train.py:282-284: `visible = radii > 0; optimizer.step(visible, N)`; the optimizer class itself,
 * SparseGaussianAdam, lives in a branch of the rasterizer that the reference does not vendor): the same update, but only for
 * the rows with row_mask[row] > 0 (device, float [P]; segments with row_width > 0) - the parameters AND both moments of
 * every other row keep their bits.  gate as gs_adam_step_gated (may be NULL). */
int gs_adam_step_masked(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                        const GsAdamSeg* segs, int32_t nseg, float beta1, float beta2, float eps, int32_t step,
                        const float* gate, const float* row_mask, void* stream);

/* The optimizer behind the reference's OWN API: the parameter tensors of up to 8 param groups (gaussian_model.py:183-193:
 * six groups, one tensor each, sizes P * {3,3,45,1,3,4}) stepped by ONE launch, each with its own learning rate and step
 * count.  `t` is a HOST array (copied into the launch).  Tensors with n == 0 are skipped; nt == 0 returns GS_OK without a
 * launch.
 * row_mask (device, [P] bytes - torch.bool's storage, 0 = not stepped - or NULL = every row): a tensor with row_width > 0 is
 * stepped only in the rows r with row_mask[r] != 0 (element i belongs to row i / row_width); every other row keeps every
 * bit of param, exp_avg and exp_avg_sq (NaNs included) and grad is only read.  The kernel reads the mask bytes of a float4's
 * rows first: a float4 without a stepped element is neither loaded nor stored, so the traffic is P mask bytes + 28 B times the
 * elements of the float4s that hold a stepped element.
 * Two rules, each ONE expression order (csrc/gs_adam.hip is compiled without contraction):
 *   flags == 0: the arithmetic of the gs_adam_step family to the letter,
 *       m = b1*m + (1-b1)*g;  v = b2*v + ((1-b2)*g)*g;  p = p - (lr * inv_bc1) * (m / (sqrtf(v) * inv_sqrt_bc2 + eps))
 *     with inv_bc1 = (float)(1 / (1 - b1^step)), inv_sqrt_bc2 = (float)(1 / sqrt(1 - b2^step)) formed in double: on one
 *     tensor with every row stepped the bits are gs_adam_step's, with a mask they are gs_adam_step_masked's.
 *   GS_ADAM_NO_BIAS_CORRECTION: the rule of the accelerated rasterizer's SparseGaussianAdam,
 *       m = b1*m + (1-b1)*g;  v = b2*v + ((1-b2)*g)*g;  p = p - lr * (m / (sqrtf(v) + eps))
 *     (`step` is not read).  That optimizer's source is NOT in the reference tree (train.py only probes for the class): the
 *     rule - Adam's moments, no bias correction - is known here only from this project's review notes, and the
 *     association lr * (m / denom) is this project's choice (the same as in the rule above), not a transcription.
 * GS_E_NULL: t missing, or a null pointer in a tensor with n > 0; GS_E_SHAPE: nt outside 0..8, n < 0, row_width < 0,
 * step < 1 with flags == 0, or a mask given while a tensor has row_width > 0 and n != P * row_width; GS_E_UNSUPPORTED: a
 * tensor base that is not 16-byte aligned (as gs_adam_step), or an unknown flag bit. */
typedef struct GsAdamTensor { /* one parameter tensor of a group */
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;         /* elements */
  int32_t row_width; /* floats per Gaussian (n == P * row_width) when row_mask is given; 0 = this tensor is never masked */
  int32_t step;      /* 1-based step count of THIS tensor for the bias correction */
  float lr;
  int32_t pad;
} GsAdamTensor;
#define GS_ADAM_NO_BIAS_CORRECTION 1
int gs_adam_step_tensors(const GsAdamTensor* t, int32_t nt, int64_t P, float beta1, float beta2, float eps, int32_t flags,
                         const uint8_t* row_mask, void* stream);

/* ---- per-Gaussian elementwise work of the train step outside the rasterizer ----
 * Parameter activations of GaussianModel (LGDWT-GS/scene/gaussian_model.py:40-60,102-117): scales = exp(scaling),
 * rotations = F.normalize(rotation) (eps 1e-12), opacities = sigmoid(opacity); all [P,k] contiguous fp32 (any
 * 4-byte alignment).  One kernel instead of ~5 torch kernels. */
int gs_activations_fwd(const float* scaling /*[P,3]*/, const float* rotation /*[P,4]*/,
                       const float* opacity /*[P]*/, int32_t P, float* scales_out, float* rotations_out,
                       float* opacities_out, void* stream);
/* Their backward (the autograd formulas of exp / normalize / sigmoid), written (=) into d_*; one kernel. */
int gs_activations_bwd(const float* scaling, const float* rotation, const float* opacity, int32_t P,
                       const float* dL_dscales, const float* dL_drotations, const float* dL_dopacities,
                       float* d_scaling, float* d_rotation, float* d_opacity, void* stream);
/* Densification statistics of one view (train.py:266-268, gaussian_model.py:471-473), for Gaussians with
 * radii > 0: max_radii2D = max(max_radii2D, radii); xyz_gradient_accum += |dL_dmeans2D.xy|; denom += 1. */
int gs_densify_stats(const int32_t* radii, const float* dL_dmeans2D /*[P,3]*/, int32_t P,
                     float* max_radii2D /*[P]*/, float* xyz_gradient_accum /*[P]*/, float* denom /*[P]*/,
                     void* stream);

/* ---- densify, split and prune as one re-layout on the device (gaussian_model.py:395-467; the host form and arbiter is
 * GaussianModelLite.densify_and_prune).  Four steps, the host in between only to size the new buffers and draw the noise:
 *
 * gs_densify_plan (two launches): per row i of the P, from the raw scaling [P,3] and opacity [P] and the statistics [P],
 *   g = xyz_gradient_accum / denom (NaN -> 0), max_scale = max_k exp(scaling_k), small = max_scale <= scale_bound, and one flag
 *   byte: GS_DENSIFY_CLONE = |g| >= max_grad && small; GS_DENSIFY_SPLIT = g >= max_grad && !small; GS_DENSIFY_PRUNE_SELF =
 *   sigmoid(opacity) < min_opacity || (size_test && max_scale > world_bound); GS_DENSIFY_PRUNE_SAMPLE = the same for the N
 *   samples of the row, with max_k exp(log(exp(scaling_k) / sample_div)) in place of max_scale (sample_div = 0.8 N).  All five
 *   thresholds are the fp32 values torch compares fp32 tensors with.  A row contributes: a survivor if it is neither split nor
 *   PRUNE_SELF, a clone if it is a survivor and CLONE, N samples if it is SPLIT and not PRUNE_SAMPLE.
 *   tmp (>= gs_densify_tmp_bytes(P) bytes, 256-byte aligned) receives, first, the GS_DENSIFY_COUNTS totals as uint32 -
 *   [survivors, clones kept, split rows, split rows whose samples are kept, rows with CLONE] - then, from byte 256, the P flag
 *   bytes; behind them the per-256-row-block counts and their exclusive prefixes over the blocks (private to gs_densify_emit).
 * gs_densify_emit (one launch): for the output order [survivors | clones | sample block 0 | ... | sample block N-1], each group by
 *   ascending source row, P2 = n_keep + n_clone_keep + N n_split_keep rows: table[j] = source row | kind << 30 (kind:
 *   GS_DENSIFY_SURVIVOR / CLONED / SAMPLE) and new_xyz[j] = the row's centre - a copy of xyz for a survivor or a clone; for sample k
 *   of the split row of rank r among ALL n_split split rows, R(q / |q|) (noise[k n_split + r] * exp(scaling)) + xyz with R of
 *   general_utils.py:78-99 and noise [N n_split, 3].  The four counts are the first four totals of the plan in the same tmp: the
 *   kernel compares them with what it finds there and writes nothing if they differ.
 * gs_morton_codes (one launch): codes[i] = the 30-bit Morton code of xyz[i] in the box lo[3] .. hi[3] (device memory, fp32), 10 bits
 *   per axis, q = clamp(rint((x - lo) / max(hi - lo, 1e-30) * 1023), 0, 1023) in float64, bits of x, y, z interleaved from bit 0.
 * gs_densify_gather (one launch): output row j of the new flat parameter / exp_avg / exp_avg_sq buffers (field-major, nfields
 *   blocks [P2, widths[f]]) from row e = perm ? perm[j] : j of the table: a survivor copies its source's parameters and both
 *   moments bit for bit; a clone copies the parameters, moments +0; a sample likewise, except field xyz_field (width 3), which is
 *   new_xyz[e] for every kind, and field scaling_field = log(exp(s) / sample_div).  A row whose perm or table entry is out of
 *   range is left unwritten.  1 416 B of compulsory traffic per output row of 59 floats.
 * GS_E_NULL: a required pointer is missing (noise only when n_split_keep > 0, perm never); GS_E_SHAPE: P < 1 or >= 2^30, N outside
 * 1 .. GS_DENSIFY_MAX_N, counts that are negative, exceed P or do not add up to P2, P2 < 1, a field count or width out of range;
 * GS_E_SCRATCH: tmp_bytes too small.  Everything is enqueued on `stream`; no host synchronisation, no atomics: the same inputs
 * give the same bits. */
#define GS_DENSIFY_CLONE 1
#define GS_DENSIFY_SPLIT 2
#define GS_DENSIFY_PRUNE_SELF 4
#define GS_DENSIFY_PRUNE_SAMPLE 8
#define GS_DENSIFY_SURVIVOR 0
#define GS_DENSIFY_CLONED 1
#define GS_DENSIFY_SAMPLE 2
#define GS_DENSIFY_COUNTS 5
#define GS_DENSIFY_MAX_N 8
size_t gs_densify_tmp_bytes(int32_t P);
int gs_densify_plan(const float* scaling, const float* opacity, const float* xyz_gradient_accum, const float* denom, int32_t P,
                    int32_t N, float max_grad, float scale_bound, float min_opacity, float world_bound, float sample_div,
                    int32_t size_test, void* tmp, size_t tmp_bytes, void* stream);
int gs_densify_emit(const void* tmp, size_t tmp_bytes, const float* xyz, const float* scaling, const float* rotation,
                    const float* noise, int32_t P, int32_t N, int32_t n_keep, int32_t n_clone_keep, int32_t n_split,
                    int32_t n_split_keep, int32_t P2, uint32_t* table, float* new_xyz, void* stream);
int gs_morton_codes(const float* xyz, int64_t n, const float* lo, const float* hi, int32_t* codes, void* stream);
int gs_densify_gather(const int64_t* perm, const uint32_t* table, const float* new_xyz, int32_t P2, const float* old_flat,
                      const float* old_exp_avg, const float* old_exp_avg_sq, int32_t P, float* new_flat, float* new_exp_avg,
                      float* new_exp_avg_sq, int32_t nfields, const int32_t* widths /*host*/, int32_t xyz_field,
                      int32_t scaling_field, float sample_div, void* stream);

/* ---- DNGaussian's densification rule and its mask prunes on the device (DNGaussian/scene/gaussian_model.py:374-392, 454-524; the
 * host forms and arbiters are GaussianModelLite.densify_and_prune_dng and GaussianModelLite.prune_points).
 *
 * gs_densify_plan_gated (two launches): gs_densify_plan with one more condition on GS_DENSIFY_CLONE and GS_DENSIFY_SPLIT -
 *   sigmoid(opacity) > gate_opacity (the reference's get_opacity > opa_thresh; the sigmoid is the value the min_opacity test is
 *   taken on, the threshold the fp32 value torch compares with; a NaN opacity selects nothing).  The prune flags, the layout of
 *   tmp (gs_densify_tmp_bytes) and the five totals are gs_densify_plan's, so gs_densify_emit, gs_morton_codes and
 *   gs_densify_gather follow unchanged.  With gate_opacity < 0 the bytes of tmp are gs_densify_plan's.
 * gs_prune_plan (two launches): mask [P] bytes, nonzero = the row goes.  tmp (>= gs_prune_tmp_bytes(P) bytes, 256-byte aligned)
 *   receives in word 0 (uint32) the number of rows kept - the one value the host reads -, behind byte 256 the rows kept per
 *   256-row block and their exclusive prefixes over the blocks (private to gs_prune_emit).
 * gs_prune_emit (one launch): the P2 kept rows in their old relative order: table[j] = source row | GS_DENSIFY_SURVIVOR << 30,
 *   new_xyz[j] = a copy of the row's centre, and new_xyz_gradient_accum / new_denom / new_max_radii2D [P2] = the source's
 *   statistics (a prune indexes them, it does not zero them).  P2 must be the total in tmp: the kernel compares and writes nothing
 *   if they differ.  The parameters and both moments then go through gs_densify_gather with that table (perm = NULL: a subsequence
 *   of spatially ordered rows is ordered); no row is a sample, so its sample_div is not read.
 * GS_E_NULL: a pointer is missing; GS_E_SHAPE: P < 1 or >= 2^30, N outside 1 .. GS_DENSIFY_MAX_N, P2 < 1 or > P; GS_E_SCRATCH:
 * tmp_bytes too small - all before any launch.  Enqueued on `stream`, no host synchronisation, no atomics: the same inputs give
 * the same bits. */
int gs_densify_plan_gated(const float* scaling, const float* opacity, const float* xyz_gradient_accum, const float* denom, int32_t P,
                          int32_t N, float max_grad, float scale_bound, float min_opacity, float world_bound, float sample_div,
                          int32_t size_test, float gate_opacity, void* tmp, size_t tmp_bytes, void* stream);
size_t gs_prune_tmp_bytes(int32_t P);
int gs_prune_plan(const uint8_t* mask, int32_t P, void* tmp, size_t tmp_bytes, void* stream);
int gs_prune_emit(const void* tmp, size_t tmp_bytes, const uint8_t* mask, const float* xyz, int32_t P, int32_t P2, uint32_t* table,
                  float* new_xyz, const float* xyz_gradient_accum, const float* denom, const float* max_radii2D,
                  float* new_xyz_gradient_accum, float* new_denom, float* new_max_radii2D, void* stream);

/* ---- FSGS's densification on the device (FSGS/scene/gaussian_model.py:424-491; the host form and arbiter is
 * GaussianModelLite.densify_and_prune_fsgs).  Its split ORs in a distance rule over [rows | clones] and its proximity unpooling
 * runs over the set after the split, so two gs_knn_mean_dist2_idx calls stand between the steps and the host reads counts back
 * three times (n_clone; the merge's totals; the proximity plan's totals) to size the next buffers.  prune_on = iteration >
 * prune_from_iter: with 0 nothing is removed, the split originals included.
 *
 * gs_densify_fsgs_plan (three launches): per row i of the P the flag byte GS_DENSIFY_FSGS_CLONE = |g| >= max_grad && max_scale <=
 *   scale_bound; GRAD_SPLIT = g >= max_grad && max_scale > scale_bound; PRUNE_SELF / PRUNE_SAMPLE as GS_DENSIFY_PRUNE_*; WIDE_SELF =
 *   max_scale > extent_bound, WIDE_SAMPLE = the same for max_k exp(log(exp(scaling_k) / sample_div)) (g, max_scale as in
 *   gs_densify_plan; every threshold the fp32 value torch compares with).  tmp (>= gs_densify_fsgs_tmp_bytes(P) bytes, 256-byte
 *   aligned) receives in uint32 word 0 the number of rows with CLONE; xyz1 [2 P, 3] receives the P centres and behind them the
 *   clones' (copies of their sources') by ascending source row: the point set of kNN #1.
 * gs_densify_fsgs_merge (two launches): dist [>= P] = kNN #1's mean squared distances; SPLIT = GRAD_SPLIT || (dist > dist_bound &&
 *   WIDE_SELF) is written into the flag byte (a clone is never split while percent_dense <= 1: the caller's duty).  tmp words
 *   GS_DENSIFY_FSGS_MERGE_AT .. + 4 receive [rows split, rows that stay (not split, or prune_on = 0), of those the rows the final
 *   prune keeps, clones it keeps, split rows whose samples it keeps].
 * gs_densify_fsgs_emit (one launch): the intermediate set Q = [rows that stay | clones | sample block 0 | ... | sample block N-1],
 *   nQ = n_stay + n_clone + N n_split rows, no prune applied: table_q[j] = source row | kind << 30 and xyz_q[j] = the centre, the
 *   samples' as in gs_densify_emit with noise [N n_split, 3].  The counts must be the ones in tmp, or nothing is written.
 * gs_densify_fsgs_prox_plan (two launches): per row j of Q, from its source's flags: kept by the final prune; selected = dist[j] >
 *   prox_bound && WIDE (of its kind), dist / nearest [nQ] / [nQ, 3] = kNN #2 on xyz_q (both NULL: no proximity); and for each of
 *   its three neighbours whether the new row taken from it is kept (the neighbour's own prune decision).  tmp_q (>=
 *   gs_densify_fsgs_tmp_bytes(nQ)) receives in words 0 .. 4 [kept rows of Q, selected rows S, kept new rows of neighbour 0, 1, 2].
 * gs_densify_fsgs_final (one or two launches): the final table, P2 = n_keep_q + n_keep_prox rows in the reference's order [kept
 *   rows of Q | kept new rows]: table[o] = source row | kind << 30 (a new row: the NEIGHBOUR's source row, kind
 *   GS_DENSIFY_PROXIMITY, and nb_kind[o] = the neighbour's kind; 0 otherwise), new_xyz[o] = the centre.  New row m of the 3 S takes
 *   neighbour m % 3 of selected row m / 3 and lies midway between it and selected row m % S (the reference tiles the selected
 *   rows).  sel_rows / prox_base: [S] uint32 scratch.  The three counts must be the ones in tmp_q, or nothing is written.
 * gs_densify_fsgs_gather (one launch): gs_densify_gather plus the proximity rows: xyz = new_xyz[e]; scaling_field = the source's,
 *   log(exp(s) / sample_div) if nb_kind[e] is GS_DENSIFY_SAMPLE; opacity_field copied; rotation_field (1, 0, 0, 0); every other
 *   field 0; moments +0.
 * Errors as above: GS_E_NULL (noise only when n_split > 0; sel_rows / prox_base / nearest only when S > 0; perm never), GS_E_SHAPE
 * (P < 1 or >= 2^29, nQ or P2 < 1 or >= 2^30, N outside 1 .. GS_DENSIFY_MAX_N, counts that are negative, too large or do not add
 * up, field indices that coincide), GS_E_SCRATCH - all before anything is enqueued.  No atomics, no host synchronisation. */
#define GS_DENSIFY_PROXIMITY 3
#define GS_DENSIFY_FSGS_CLONE 1
#define GS_DENSIFY_FSGS_GRAD_SPLIT 2
#define GS_DENSIFY_FSGS_SPLIT 4
#define GS_DENSIFY_FSGS_PRUNE_SELF 8
#define GS_DENSIFY_FSGS_PRUNE_SAMPLE 16
#define GS_DENSIFY_FSGS_WIDE_SELF 32
#define GS_DENSIFY_FSGS_WIDE_SAMPLE 64
#define GS_DENSIFY_FSGS_MERGE_AT 8
size_t gs_densify_fsgs_tmp_bytes(int32_t P);
int gs_densify_fsgs_plan(const float* scaling, const float* opacity, const float* xyz_gradient_accum, const float* denom,
                         const float* xyz, int32_t P, int32_t N, float max_grad, float scale_bound, float min_opacity,
                         float world_bound, float extent_bound, float sample_div, int32_t size_test, void* tmp, size_t tmp_bytes,
                         float* xyz1 /*[2 P, 3]*/, void* stream);
int gs_densify_fsgs_merge(void* tmp, size_t tmp_bytes, const float* dist, int32_t P, float dist_bound, int32_t prune_on,
                          void* stream);
int gs_densify_fsgs_emit(const void* tmp, size_t tmp_bytes, const float* xyz, const float* scaling, const float* rotation,
                         const float* noise, int32_t P, int32_t N, int32_t n_clone, int32_t n_split, int32_t n_stay, int32_t nQ,
                         int32_t prune_on, uint32_t* table_q, float* xyz_q, void* stream);
int gs_densify_fsgs_prox_plan(const void* tmp, size_t tmp_bytes, int32_t P, const uint32_t* table_q, int32_t nQ, const float* dist,
                              const int32_t* nearest, float prox_bound, int32_t prune_on, void* tmp_q, size_t tmp_q_bytes,
                              void* stream);
int gs_densify_fsgs_final(const void* tmp_q, size_t tmp_q_bytes, const uint32_t* table_q, const float* xyz_q, const int32_t* nearest,
                          int32_t nQ, int32_t n_keep_q, int32_t S, int32_t n_keep_prox, int32_t P2, uint32_t* table,
                          uint8_t* nb_kind, float* new_xyz, uint32_t* sel_rows, uint32_t* prox_base, void* stream);
int gs_densify_fsgs_gather(const int64_t* perm, const uint32_t* table, const uint8_t* nb_kind, const float* new_xyz, int32_t P2,
                           const float* old_flat, const float* old_exp_avg, const float* old_exp_avg_sq, int32_t P, float* new_flat,
                           float* new_exp_avg, float* new_exp_avg_sq, int32_t nfields, const int32_t* widths /*host*/,
                           int32_t xyz_field, int32_t scaling_field, int32_t opacity_field, int32_t rotation_field, float sample_div,
                           void* stream);

/* ---- the visibility-sparse gradient exchange of the data-parallel step (N > 1; no reference counterpart: the reference trains
 * on one GPU).  Only Gaussians that emitted instances in SOME rank's view have a non-zero gradient row, so the ranks exchange
 * the rows of the union only.  The flat gradient buffer is field-major: field f is a [P, widths[f]] row-major block, the blocks
 * back to back.  pos[i] = (number of j <= i with mask[j] != 0) - 1: the inclusive prefix of the union mask, minus one.
 * gs_rows_pack: packed = the K union rows of every field, field after field ([K, widths[f]] blocks): one launch instead of an
 * index_select per field.  gs_rows_unpack: the inverse, into the rows of the union (the others are not touched). */
int gs_rows_pack(const float* flat, int32_t P, int32_t nfields, const int32_t* widths /*host*/, const uint8_t* mask,
                 const int32_t* pos, int32_t K, float* packed, void* stream);
int gs_rows_unpack(float* flat, int32_t P, int32_t nfields, const int32_t* widths /*host*/, const uint8_t* mask,
                   const int32_t* pos, int32_t K, const float* packed, void* stream);
/* ---- image stage of the train step (LGDWT-GS/train.py:117-124 + gaussian_renderer/__init__.py:112-119): what happens to the
 * render between the rasterizer and the loss.  raw / pred / g_pred / g_raw: [3,H,W] planes; exposure: the camera's [3,4]
 * row (12 device floats, row-major), NULL = none; alpha: [H,W] device floats, NULL = all ones.  All buffers distinct.
 *   forward : lin[j] = sum_c raw[c] E[c][j] + E[j][3];  pred = clamp(lin, 0, 1) * alpha     (exposure, clamp, mask)
 *   backward: g_lin[j] = g_pred[j] * alpha * [0 <= lin[j] <= 1];  g_raw[c] = sum_j E[c][j] g_lin[j];
 *             partials (may be NULL) = one row of 12 per workgroup (gs_image_stage_partials_count(H, W) rows, all written):
 *             word 4 c + j = sum raw[c] g_lin[j], word 4 j + 3 = sum g_lin[j] - the workgroup's share of dL/dE.
 * g_pred is the criterion's gradient with respect to pred WITHOUT its clamp fold (gs_ssim_bwd_uniform: clamp_src = NULL).
 * float4 along x when H*W is a multiple of 4 and the planes 16-byte aligned; any size works. */
int64_t gs_image_stage_partials_count(int32_t H, int32_t W);
int gs_image_stage_fwd(const float* raw, const float* exposure, const float* alpha, int32_t H, int32_t W, float* pred,
                       void* stream);
int gs_image_stage_bwd(const float* raw, const float* exposure, const float* alpha, const float* g_pred, int32_t H, int32_t W,
                       float* g_raw, float* partials, void* stream);
/* The trained exposures' optimizer (torch.optim.Adam over the [n_cameras,3,4] tensor, LGDWT-GS/scene/gaussian_model.py:201)
 * in ONE launch of one workgroup.  partials != NULL: the n_partials rows of gs_image_stage_bwd are added in a fixed order
 * (double) into the gradient of camera `camera`'s row; every other row's gradient is 0; the whole gradient is written to
 * grad when grad != NULL.  partials == NULL: the gradient is read from grad.  exposure != NULL: one Adam step (1-based `step`,
 * bias-corrected, lr, betas, eps as torch; the betas in double, as torch has them for 1 - beta) over all 12 n_cameras elements with that gradient - rows with a zero gradient
 * move as torch moves them; exp_avg / exp_avg_sq required.  exposure == NULL: gradient only (grad required).
 * gate: as gs_adam_step_gated - device float, may be NULL; when *gate != 0 nothing is written at all. */
int gs_exposure_adam(const float* partials, int64_t n_partials, int32_t camera, float* grad, float* exposure, float* exp_avg,
                     float* exp_avg_sq, int32_t n_cameras, float lr, double beta1, double beta2, float eps, int32_t step,
                     const float* gate, void* stream);
/* mask[i] = 1 when Gaussian i emitted instances in the forward whose geometry state `scratch` holds (what gs_backward_step's
 * data-parallel form writes into GsStepState.grad_mask later - available as soon as the forward's geometry phase has run,
 * so the union of the ranks' masks can be exchanged while the loss and the backward are still running). */
int gs_export_row_mask(const GsScratch* scratch, int32_t P, uint8_t* mask, void* stream);

/* ---- test-set evaluation of one view (csrc/gs_eval.hip): MSE / PSNR, SSIM and L1 of render against gt, both [C,H,W] fp32,
 * in the forms of the reference's evaluation scripts, from one pass over the images and a one-workgroup combine ----
 * The pixel transform, applied to BOTH images while they are staged, in this order:
 *   GS_EVAL_CLAMP     x <- clamp(x, 0, 1)                                     (training_report, DNGaussian/train_llff.py:298,302)
 *   GS_EVAL_QUANTISE  q = (uint8) clamp(x * 255 + 0.5, 0, 255), x <- q / 255  (torchvision save_image -> to_tensor: the PNG
 *                     round trip of LGDWT-GS/render.py:45-46 -> metrics.py:31-32; the multiply and the add round separately)
 *   GS_EVAL_MASK_DTU  x <- x * m + (1 - m), mask [H,W] fp32 broadcast over the channels (DNGaussian/metrics_dtu.py:40-46;
 *                     the reference's mask is a 3-channel image, DTU's are grey).  SSIM and L1 run over all pixels of the
 *                     blended images (zero padding outside the image, as F.conv2d pads after the blend), MSE / PSNR over
 *                     the elements with m == 1 only (metrics_dtu.py:93-95).
 * out_row[GS_EVAL_WORDS] doubles in device memory: 0 mse | 1 psnr = 20 log10(1 / sqrt(mse)) | 2 ssim (mean of the map, 11-tap
 * Gaussian window, constants C1, C2) | 3 l1 (mean) | 4 count = the elements mse ran over | 5..7 reserved = 0.  Identical images:
 * psnr = +inf; an empty mask: mse = psnr = NaN, count = 0 - both as in the reference.
 * quantised_out (nullable): uint8 [H,W,C], the bytes save_image would write for render (before any mask; the same bytes
 * with or without GS_EVAL_CLAMP / GS_EVAL_QUANTISE).
 * tmp: >= gs_eval_tmp_bytes(C, H, W) bytes of device scratch, one row of gs_eval_partials_count(C, H, W) float64 partials per
 * sum; every partial is written before it is read.  The error sums and the count accumulate in float64, the SSIM-map sum of
 * a workgroup in fp32 as the criterion's kernels do; the partials are added in index order in float64: the same bits on
 * every run.  Two launches on `stream`, no atomics, no host synchronisation, no device-to-host copy.
 * GS_E_NULL: render, gt, tmp or out_row missing, or GS_EVAL_MASK_DTU without mask; GS_E_SHAPE: C, H or W <= 0, C > 4, unknown
 * flag bits, or tmp_bytes too small.  Both size queries return 0 for such a shape. */
#define GS_EVAL_CLAMP 1
#define GS_EVAL_QUANTISE 2
#define GS_EVAL_MASK_DTU 4
#define GS_EVAL_WORDS 8
int64_t gs_eval_partials_count(int32_t C, int32_t H, int32_t W);
size_t gs_eval_tmp_bytes(int32_t C, int32_t H, int32_t W);
int gs_eval_metrics(const float* render, const float* gt, const float* mask /*NULL unless GS_EVAL_MASK_DTU*/, int32_t C,
                    int32_t H, int32_t W, int32_t flags, float C1, float C2, void* tmp, size_t tmp_bytes,
                    double* out_row /*[GS_EVAL_WORDS], device*/, uint8_t* quantised_out /*NULL ok*/, void* stream);

/* ---- evaluation from files (csrc/gs_eval_files.hip): PIL.Image.resize on 8-bit images, and skimage's SSIM ----
 * gs_resize_bicubic_u8: in uint8 [H,W,C] interleaved, C = 1 or 3 -> out uint8 [H2,W2,C], the bytes Pillow's
 * Image.resize((W2, H2)) gives for modes L and RGB with its default filter (antialiased bicubic, Resample.c), and, when
 * out_f32 is given, the same image as fp32 planar [C,H2,W2] = byte / 255 (to_tensor; what gs_eval_metrics takes).
 * The per-axis tables are the caller's, in device memory (gsplat_amd/imageio.py forms them in double on the host):
 *   bounds int32 [n_out,2] = (first source sample, run length n <= ksize) per output sample;
 *   coef   int32 [n_out,ksize] = the normalised weights * 2^22, rounded half away from zero, zero beyond the run.
 * out = clamp((2^21 + sum coef * sample) >> 22, 0, 255) in int32, the horizontal pass first into an 8-bit intermediate
 * (tmp), then the vertical pass.  A pass whose sizes agree is skipped (its tables may be NULL); with both skipped the image
 * is copied.  A table row whose run leaves the source reads nothing and gives 0.  At most two launches on `stream`.
 * tmp: >= gs_resize_tmp_bytes(H, W, C, H2, W2) bytes of device scratch = the intermediate when both passes run, else 0
 * (tmp may then be NULL).  GS_E_NULL: in, out, a needed table or needed tmp missing; GS_E_SHAPE: C outside {1, 3}, a size
 * <= 0, an image above 2^30 bytes, ksize <= 0 for a pass that runs, or tmp_bytes too small.
 *
 * gs_eval_ssim_sk: out[0] (one double, device memory) = skimage.metrics.structural_similarity(a, b, channel_axis=2,
 * data_range=1.0) with its defaults, of render and gt [C,H,W] fp32 after gs_eval_metrics's pixel transform (same flags, same
 * order, the one implementation): per channel the 7 x 7 box means ux, uy, uxx, uyy, uxy, v_ab = 49/48 (u_ab - u_a u_b),
 * S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = 1e-4, C2 = 9e-4, the mean of S over the windows
 * that lie wholly inside the image (skimage's 3-pixel crop), then the mean over the channels.  Window sums and the map sum
 * are float64 in one fixed order: the same bits on every run.  Two launches, no atomics, no host synchronisation.
 * tmp: >= gs_eval_ssim_sk_tmp_bytes(C, H, W).  GS_E_NULL: render, gt, tmp or out missing, or GS_EVAL_MASK_DTU without mask;
 * GS_E_SHAPE: C outside 1..4, H < 7 or W < 7 (skimage raises there), unknown flag bits, or tmp_bytes too small. */
size_t gs_resize_tmp_bytes(int32_t H, int32_t W, int32_t C, int32_t H2, int32_t W2);
int gs_resize_bicubic_u8(const uint8_t* in, int32_t H, int32_t W, int32_t C, int32_t H2, int32_t W2,
                         const int32_t* xbounds, const int32_t* xcoef, int32_t kx, const int32_t* ybounds,
                         const int32_t* ycoef, int32_t ky, void* tmp, size_t tmp_bytes, uint8_t* out,
                         float* out_f32 /*NULL ok*/, void* stream);
size_t gs_eval_ssim_sk_tmp_bytes(int32_t C, int32_t H, int32_t W);
int gs_eval_ssim_sk(const float* render, const float* gt, const float* mask /*NULL unless GS_EVAL_MASK_DTU*/, int32_t C,
                    int32_t H, int32_t W, int32_t flags, void* tmp, size_t tmp_bytes, double* out /*device*/, void* stream);

/* ---- LPIPS, net_type='vgg', version 0.1, forward only (csrc/gs_lpips.hip) ----
 * Additive entries (GS_ABI_VERSION unchanged).  lpipsPyTorch/modules/lpips.py:30-36 of render against gt, both [C,H,W] fp32 of
 * which the first three channels are used, after gs_eval_metrics's pixel transform (same flags, same order, the one
 * implementation) and the reference's z_score on the image as it is in [0, 1].  The weights are the caller's:
 *   packed_w[13]  the thirteen 3 x 3 convolutions of torchvision's vgg16().features up to relu5_3, each repacked ONCE by
 *                 gs_lpips_pack_weights from torch's [Cout][Cin][3][3] into gs_lpips_packed_floats(Cin, Cout) floats
 *                 ([Cin, padded to 4 for Cin = 3][9][Cout]; 16-byte aligned);
 *   bias[13]      their biases, [Cout] fp32;
 *   lin[5]        the 1 x 1 "lin" weights of the five taps (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3), [C] FLOAT64
 *                 (the fp32 weights widened).
 * The three are HOST arrays of device pointers.  out[6] doubles in device memory: the five per-tap terms, then their sum in
 * tap order.  The convolutions run on the f32 MFMA in one fixed K order; everything from the fp32 features on is float64
 * summed in one fixed order: the same bits on every call, and an image's features do not depend on its slot of the pair.  No
 * atomics, no host synchronisation, no device-to-host copy; every word of tmp is written before it is read.
 * tmp: >= gs_lpips_tmp_bytes(H, W) bytes of device scratch (two activation buffers of 2 x 64 x H x W fp32 and the distance's
 * partials), 256-byte aligned.
 * GS_E_NULL: a required pointer is missing (mask only with GS_EVAL_MASK_DTU); GS_E_SHAPE: C outside 3..4, H or W below 16 (the
 * fifth tap would be empty; torch raises there too), H * W > 2^24, unknown flag bits or a packed weight off 16 bytes;
 * GS_E_SCRATCH: tmp_bytes too small.  gs_lpips_tmp_bytes returns 0 for such a size.
 *
 * The stages on their own, launched exactly as gs_lpips_vgg launches them (the tests' handle on each):
 *   gs_lpips_conv3x3_relu  y [N][Cout][H][W] = relu(conv3x3(x [N][Cin][H][W], padding 1) + bias), (Cin, Cout) one of VGG16's
 *                          eight pairs 3-64, 64-64, 64-128, 128-128, 128-256, 256-256, 256-512, 512-512 (else GS_E_SHAPE)
 *   gs_lpips_maxpool2      y [NC][H/2][W/2] = max over 2 x 2, stride 2, an odd last row or column dropped; H, W >= 2
 *   gs_lpips_distance      out[0] = mean over the pixels of sum_c lin[c] (x_c / (|x| + 1e-10) - y_c / (|y| + 1e-10))^2 of two
 *                          [C][H][W] fp32 feature maps; tmp >= gs_lpips_distance_tmp_bytes(H, W) */
int64_t gs_lpips_packed_floats(int32_t Cin, int32_t Cout);
int gs_lpips_pack_weights(const float* w /*[Cout][Cin][3][3]*/, int32_t Cin, int32_t Cout, float* packed, void* stream);
size_t gs_lpips_tmp_bytes(int32_t H, int32_t W);
int gs_lpips_vgg(const float* render, const float* gt, const float* mask /*NULL unless GS_EVAL_MASK_DTU*/, int32_t C, int32_t H,
                 int32_t W, int32_t flags, const float* const* packed_w /*host [13]*/, const float* const* bias /*host [13]*/,
                 const double* const* lin /*host [5]*/, void* tmp, size_t tmp_bytes, double* out /*[6], device*/, void* stream);
int gs_lpips_conv3x3_relu(const float* x, const float* packed_w, const float* bias, int32_t N, int32_t Cin, int32_t Cout,
                          int32_t H, int32_t W, float* y, void* stream);
int gs_lpips_maxpool2(const float* x, int64_t NC, int32_t H, int32_t W, float* y, void* stream);
size_t gs_lpips_distance_tmp_bytes(int32_t H, int32_t W);
int gs_lpips_distance(const float* fx, const float* fy, const double* lin, int32_t C, int32_t H, int32_t W, void* tmp,
                      size_t tmp_bytes, double* out /*device*/, void* stream);

/* ---- the turbo-coloured depth map of the render stage (csrc/gs_depth_vis.hip) ----
 * DNGaussian/render.py:121,127-130 (and spiral.py:114-121) and FSGS/utils/general_utils.py:157-176 on the device:
 *   alpha given: d = (depth - min) / (max - min) + 1 * (1 - alpha), every operation rounded to fp32 on its own, min / max
 *                NaN-propagating as torch's; out_grey_u8 (NULL ok) [H,W,3] = the bytes save_image writes for 1 - d,
 *                out_composite (NULL ok) fp32 [H,W] = d.
 *                Without alpha the depth image itself is coloured.
 *   lo_auto, hi_auto = weighted_percentile(x, ones, [0.5, 99.5]): np.argsort's order (NaN last), acc_w = 1..n, the queries
 *                p * float32(n / 100) in double, np.interp's statements in double.  A radix select, not a sort: exact.
 *   lo = lo_auto - eps, hi = hi_auto + eps; eps = float32's epsilon (rules IDENTITY, DNG) or 1e-10 (FSGS)
 *   curve:       IDENTITY x | DNG -log(x + eps32): the pixel in double, rounded to fp32 once; lo, hi in double |
 *                FSGS 1 / x + 1e-10: the pixel in fp32, lo and hi in double
 *   v = nan_to_num(clip((curve(x) - min(lo', hi')) / |hi' - lo'|, 0, 1)) in double, index = trunc(256 v) with 256 -> 255
 *   out_rgb_u8 [H,W,3] interleaved = row `index` of lut_rgb_u8 [256,3], the caller's table (the byte rule stays on the host)
 *   out_bounds (NULL ok, device): double[2] = lo, hi before the curve.
 * All launches go to `stream`; no host synchronisation, integer atomics only: the same bits on every run.
 * tmp: >= gs_depth_vis_tmp_bytes(H, W) bytes of device scratch, 256-byte aligned; it need not be cleared between calls.
 * GS_E_SHAPE: H or W < 0, H * W > 2^24 (where float32's cumulative sum of ones stops counting), an unknown rule, tmp_bytes
 * too small, tmp not 256-byte aligned or an image / out_bounds pointer not aligned to its element; the size query returns 0
 * for such a shape.  H * W == 0: GS_OK, nothing is launched or written.  GS_E_NULL: depth, lut_rgb_u8, tmp or out_rgb_u8
 * missing, or out_grey_u8 / out_composite without alpha. */
#define GS_DEPTH_VIS_IDENTITY 0
#define GS_DEPTH_VIS_DNG 1
#define GS_DEPTH_VIS_FSGS 2
size_t gs_depth_vis_tmp_bytes(int32_t H, int32_t W);
int gs_depth_vis(const float* depth, const float* alpha /*NULL ok*/, int32_t H, int32_t W, int32_t rule,
                 const uint8_t* lut_rgb_u8 /*[256,3]*/, void* tmp, size_t tmp_bytes, uint8_t* out_rgb_u8 /*[H,W,3]*/,
                 uint8_t* out_grey_u8 /*NULL ok*/, float* out_composite /*NULL ok*/, double* out_bounds /*NULL ok*/,
                 void* stream);

/* ---- LGDWT-GS's Wavelet Error Field, its heatmap grid and the Charbonnier loss (csrc/gs_wef.hip) ----
 * LGDWT-GS/utils/loss_utils.py:156-329 and 98-101 on the device, one image per call.
 * gs_wef_maps: pred, gt [C,H,W] fp32, C in 1..4.  The 2-level Haar bands of pred - gt (the butterfly and repeat-last-sample
 *   rule of gs_dwt_forward), e = mean_c(scale * b_c^2) (scale 1 at level 1, 4 for LL2, 2 for LH2 / HL2 / HH2), upsampled to
 *   [H,W] as F.interpolate(mode='bilinear', align_corners=False), n = (u - min) / (max - min + 1e-8f) per map, and the field
 *   of their mean normalised the same way.  Every operation rounds to fp32 on its own; min and max propagate NaN as torch's
 *   amin / amax do.
 *   bands = GS_WEF_LEVEL2: out_maps [4][H][W] = LL2, LH2, HL2, WEF = norm((n_LL2 + n_LH2 + n_HL2) / 3)
 *   bands = GS_WEF_ALL:    out_maps [9][H][W] = LL1, LH1, HL1, HH1, LL2, LH2, HL2, HH2, COMBINED = norm((their sum in that order) / 8)
 *   out_bounds (NULL ok, device): float [K + 1][2] = (min, max) of each upsampled map and of the combined field before its
 *   own normalisation, K = 3 or 8.
 *   tmp: >= gs_wef_tmp_bytes(C, H, W, bands) bytes of device scratch, 256-byte aligned, not cleared between calls.  After the
 *   call it starts with the energy planes, each padded to a multiple of 256 bytes: LL2, LH2, HL2, HH2 [ceil(ceil(H/2)/2)]
 *   [ceil(ceil(W/2)/2)] (HH2's plane is always there, written for GS_WEF_ALL only), then for GS_WEF_ALL LL1, LH1, HL1, HH1
 *   [ceil(H/2)][ceil(W/2)].
 *   Six launches on `stream`, no host synchronisation, no atomics: the same bits on every run.
 * gs_wef_grid: maps [K_total][H][W] -> out_u8 [rows * H][tile_cols * W][3], rows = ceil(n_keys / tile_cols).  Tile idx shows
 *   maps[order[idx]] at row idx / tile_cols, column idx % tile_cols: x = clamp(v, 0, 1) (NaN -> 0), r = x,
 *   g = clamp(1 - |x - 0.5| * 2, 0, 1), b = 1 - x, byte = (uint8)(c * 255) truncated.  Unused tiles, and tiles whose order entry
 *   lies outside [0, K_total), are 0.  order: device int32 [n_keys].
 *   labels (NULL ok, device): uint8 [n_keys][GS_WEF_LABEL_H][GS_WEF_LABEL_W]; the box of tile idx, GS_WEF_LABEL_W x
 *   GS_WEF_LABEL_H pixels from the tile's top-left corner and clipped at the image border (not at the tile's), is 255 where
 *   its label is non-zero and 0 elsewhere; where boxes overlap the highest idx wins (they are drawn in key order).
 * gs_charbonnier_fwd: out[0] = mean(sqrtf(d * d + eps2)), d = pred - target, eps2 = (float)(epsilon * epsilon); the terms are
 *   fp32, their sum float64 in a fixed order, divided by n and rounded once.  tmp: >= gs_charbonnier_tmp_bytes(n) bytes, 256-byte
 *   aligned.  Two launches.
 * gs_charbonnier_bwd: d_pred[i] = grad_out[0] * d / sqrt(d * d + epsilon^2) / n evaluated in double from the fp32 inputs and
 *   rounded once, d_target[i] its negative; either may be NULL (not both).  One launch.
 * GS_E_SHAPE: C outside 1..4, a size below 1, H * W >= 2^31, an unknown band set, tmp_bytes too small, tmp not 256-byte
 * aligned or another pointer not aligned to its element; the size queries return 0 for such a shape.  GS_E_NULL: a required
 * pointer missing. */
#define GS_WEF_LEVEL2 0
#define GS_WEF_ALL 1
#define GS_WEF_LABEL_W 121
#define GS_WEF_LABEL_H 27
size_t gs_wef_tmp_bytes(int32_t C, int32_t H, int32_t W, int32_t bands);
int gs_wef_maps(const float* pred, const float* gt, int32_t C, int32_t H, int32_t W, int32_t bands, void* tmp, size_t tmp_bytes,
                float* out_maps, float* out_bounds /*NULL ok*/, void* stream);
int gs_wef_grid(const float* maps, int32_t K_total, int32_t H, int32_t W, const int32_t* order /*[n_keys]*/, int32_t n_keys,
                int32_t tile_cols, const uint8_t* labels /*NULL ok*/, uint8_t* out_u8, void* stream);
size_t gs_charbonnier_tmp_bytes(int64_t n);
int gs_charbonnier_fwd(const float* pred, const float* target, int64_t n, double epsilon, void* tmp, size_t tmp_bytes,
                       float* out /*device [1]*/, void* stream);
int gs_charbonnier_bwd(const float* pred, const float* target, int64_t n, double epsilon, const float* grad_out /*device [1]*/,
                       float* d_pred /*NULL ok*/, float* d_target /*NULL ok*/, void* stream);

/* ---- depth priors from files: depth_params.json's fit and the camera's inverse-depth map (csrc/gs_depth_priors.hip) ----
 * gs_depth_scales: gaussian-splatting/utils/make_depth_scale.py:8-64 for n_images images in ONE launch, one workgroup per
 *   image.  Image i owns the observations [seg[i], seg[i + 1]) of obs_ids / obs_xy (seg: device int64 [n_images + 1], ascending,
 *   seg[n_images] <= n_obs).  Per observation, in double, one rounding per operation:
 *     used  = 0 <= id < n_table                       (a row of the dense table that no point fills is zeros and is used)
 *     z     = ((X r20 + Y r21) + Z r22) + t2,  inv = 1 / z          (X, Y, Z) = table[id]; the script reads no other row of R
 *     mx    = (float)(x s), my = (float)(y s)          s = map rows / camera height
 *     valid = used && mx >= 0 && my >= 0 && mx < wlim && my < hlim && inv > 0     the four map tests in fp32
 *     mono  = the map sampled at (mx, my): each coordinate rounded half-to-even to 2^-coord_bits of a pixel
 *             (i = rint(x 2^bits), cell = i >> bits, f = (i & (2^bits - 1)) / 2^bits; coord_bits < 0: cell = floor(x), f = x - cell),
 *             weights (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx and ((w00 v00 + w01 v01) + w10 v10) + w11 v11 with every
 *             multiply and add rounded to fp32, cell indices clamped to the map.  A map sample is value / 65536 (uint16 or fp32).
 *   cams: device double [n_images][8] = r20, r21, r22, t2, s, wlim, hlim, 0 (wlim / hlim hold fp32 values: (float)(width s), ...).
 *   maps: device array of n_images device pointers; map_hw: device int32 [n_images][2] = rows, columns (each 1 .. 2^20).
 *   map_dtype: GS_DEPTH_MAP_U16 or GS_DEPTH_MAP_F32, for every map of the call.
 *   n_valid > 10 and (max - min of inv over the USED observations) > 1e-3, else scale = offset = 0.  Otherwise the medians of
 *   inv (double) and mono (fp32) over the valid observations by radix select (both middle elements when the count is even:
 *   (a + b) / 2 in the sequence's own precision), the mean absolute deviations as float64 sums in a fixed order (per-lane
 *   strided partials, a fixed tree) divided by n_valid, scale = s_colmap / s_mono, offset = t_colmap - t_mono scale.
 *   out: device double [n_images][8] = scale, offset, n_valid, t_colmap, s_colmap, t_mono, s_mono, max - min (the four
 *   statistics are 0 where the gate fails).
 *   tmp: >= gs_depth_scales_tmp_bytes(n_obs) bytes of device scratch, 256-byte aligned, not cleared between calls.
 *   Integer atomics in LDS only, no host synchronisation: the same bits on every run.
 * gs_invdepth_prepare: gaussian-splatting/scene/cameras.py:60-78 for one map, one launch.  src [H][W] uint16 or fp32; per output
 *   pixel of [H2][W2]: value / divisor (fp32 division), bilinear resize (fx = (float)((dx + 0.5) * ((double)W / W2) - 0.5),
 *   sx = floor(fx), fx -= sx, sx < 0 -> (0, 0), sx >= W - 1 -> (W - 1, 0); horizontally a0 S0 + a1 S1 with a0 = 1 - fx, a1 = fx,
 *   then vertically the same, every operation rounded to fp32; equal sizes copy), negatives to 0, then with apply_scale != 0
 *   x * scale rounded, + offset rounded (never fused).  out_mask (NULL ok) [H2][W2] = mask_value.
 * GS_E_SHAPE: a count or size below its minimum or above its maximum (n_images, n_obs, n_table < 0; H, W, H2, W2 outside
 * 1 .. 2^15), an unknown dtype, coord_bits > 10, tmp_bytes too small, tmp not 256-byte aligned, a pointer not aligned to its
 * element.  n_images == 0: GS_OK, nothing launched.  GS_E_NULL: a required pointer missing (obs_* and points may be NULL when
 * n_obs == 0 / n_table == 0). */
#define GS_DEPTH_MAP_U16 0
#define GS_DEPTH_MAP_F32 1
size_t gs_depth_scales_tmp_bytes(int64_t n_obs);
int gs_depth_scales(const double* points /*[n_table,3]*/, int64_t n_table, const int64_t* obs_ids /*[n_obs]*/,
                    const double* obs_xy /*[n_obs,2]*/, int64_t n_obs, const int64_t* seg /*[n_images+1]*/,
                    const double* cams /*[n_images,8]*/, const void* const* maps /*[n_images]*/, const int32_t* map_hw /*[n_images,2]*/,
                    int32_t map_dtype, int32_t coord_bits, int32_t n_images, void* tmp, size_t tmp_bytes,
                    double* out /*[n_images,8]*/, void* stream);
int gs_invdepth_prepare(const void* src, int32_t src_dtype, int32_t H, int32_t W, int32_t H2, int32_t W2, float divisor,
                        int32_t apply_scale, float scale, float offset, float mask_value, float* out_invdepth /*[H2,W2]*/,
                        float* out_mask /*NULL ok*/, void* stream);

/* ---- image ingest (csrc/gs_image_ingest.hip): one decoded image to what the reference's Camera keeps ----
 * Additive entries (GS_ABI_VERSION unchanged).  in uint8 [H,W,C] interleaved, C = 3 (RGB), 4 (RGBA) or 2 (LA: out_u8 only).
 *   GS_INGEST_COMPOSITE (C = 4 only; with GS_INGEST_WHITE onto white, else black): first, at the source size,
 *     q = byte(trunc((c / 255 * (a / 255) + bg * (1 - a / 255)) * 255)) evaluated in double, every operation rounded on its own
 *     (scene/dataset_readers.py:353-359); the image goes on as RGB, Ce = 3 channels, no alpha.  Otherwise Ce = C.
 *   Resize to (W2, H2) by PIL.Image.resize's default filter, with the tables of gs_resize_bicubic_u8: RGB as there; LA / RGBA by
 *     Pillow's premultiplied rule - t = c a + 128, c' = ((t >> 8) + t) >> 8 on the way into the first pass that runs, both passes
 *     on the premultiplied bytes (alpha included), a == 0 or 255 -> c' else min(255, 255 c' / a) (integer division) on the way out
 *     of the last.  A pass whose sizes agree is skipped; with both skipped the bytes are copied, without that round trip.
 *   Outputs, each NULL ok but not all three: out_u8 [H2,W2,Ce]; out_image fp32 [3,H2,W2] = byte / 255, one correctly rounded
 *     division (Camera.original_image); out_alpha fp32 [1,H2,W2] = alpha byte / 255, or 1 where the image has no alpha
 *     (Camera.alpha_mask), with columns < W2 / 2 zeroed under GS_INGEST_ZERO_LEFT and columns >= W2 / 2 under
 *     GS_INGEST_ZERO_RIGHT (train_test_exp, scene/cameras.py:50-54).
 * At most two launches on `stream`; no atomics, no read-back, no host synchronisation; a table row whose run leaves the source
 * reads nothing.  tmp: >= gs_image_ingest_tmp_bytes(...) bytes = the intermediate [H,W2,Ce] when both passes run, else 0.
 * GS_E_NULL: in, all three outputs, a needed table or needed tmp missing; GS_E_SHAPE: C outside {2, 3, 4}, a size <= 0, an image
 * above 2^30 bytes, unknown flag bits, GS_INGEST_COMPOSITE with C != 4, GS_INGEST_WHITE without it, C = 2 with out_image or
 * out_alpha, ksize <= 0 for a pass that runs, or tmp_bytes too small. */
#define GS_INGEST_COMPOSITE 1
#define GS_INGEST_WHITE 2
#define GS_INGEST_ZERO_LEFT 4
#define GS_INGEST_ZERO_RIGHT 8
size_t gs_image_ingest_tmp_bytes(int32_t H, int32_t W, int32_t C, int32_t H2, int32_t W2, int32_t flags);
int gs_image_ingest(const uint8_t* in, int32_t H, int32_t W, int32_t C, int32_t H2, int32_t W2, const int32_t* xbounds,
                    const int32_t* xcoef, int32_t kx, const int32_t* ybounds, const int32_t* ycoef, int32_t ky, int32_t flags,
                    void* tmp, size_t tmp_bytes, uint8_t* out_u8 /*NULL ok*/, float* out_image /*NULL ok*/,
                    float* out_alpha /*NULL ok*/, void* stream);

/* ---- optional per-stage timing (HIP events recorded on the caller's stream around every kernel
 * group).  Off by default.  bench.py enables it over the timed region to get each kernel's average
 * launch duration on the stream it is launched on.  (No reference counterpart: the reference only
 * brackets whole iterations with a torch.cuda.Event pair, LGDWT-GS/train.py:65-66,97,220.) ---- */
int gs_profile_enable(int32_t on);
/* Restrict the timers to one stage (index as in gs_profile_stage_name; < 0 = all stages again).  Every recorded
 * event pair drains the pipeline for ~10 us, so a throughput measurement keeps only the kernel it reports on. */
int gs_profile_only(int32_t stage);
int gs_profile_reset(void);
int gs_profile_stage_count(void);
const char* gs_profile_stage_name(int32_t stage);
/* Waits for every recorded event, then ms[i] / counts[i] = accumulated milliseconds / launches of stage i. */
int gs_profile_read(double* ms, int64_t* counts, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_H_INCLUDED */
