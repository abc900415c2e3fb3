"""Host glue between torch tensors and the C ABI (include/gsplat.h).

``RasterBackend`` re-creates the three pybind entry points of the reference extension module
(`rasterize_gaussians`, `rasterize_gaussians_backward`, `mark_visible`:
diff-gaussian-rasterization/ext.cpp:15-19, rasterize_points.cu:35-244) with identical positional
arguments and return tuples, on top of the two-phase C ABI.  Tensors stay torch-owned; only raw
addresses and the current HIP stream cross the boundary.
"""
import ctypes as C
import os

import torch

from .capi import GsGaussians, GsGrads, GsScratch, GsView

NUM_CHANNELS = 3
_DEPTH_ONLY = 2   # _Forward.fsgs of a depth-only forward (RasterBackend.depth_forward): _render calls gs_depth_forward


def _ptr(t):
    """Explicit NULL for 'absent' (the reference relied on data_ptr() of an empty tensor)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _prep(t, device):
    """contiguous fp32 on `device`; empty stays empty (rasterize_points.cu:101-120)."""
    if t is None or t.numel() == 0:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    if t.device != device:
        t = t.to(device)
    return t.contiguous()


def _regions(W, H):
    """Regions of a W x H view: blocks of 4 x 4 tiles of 16 x 16 pixels (csrc/gs_common.h RG_TILES)."""
    return ((((W + 15) // 16) + 3) // 4) * ((((H + 15) // 16) + 3) // 4)


class _Forward:
    """What the steps of one forward (RasterBackend.rasterize_gaussians) share: its view, Gaussians, buffers, outputs and
    camera state; on the GPU also its stream and pinned status block."""
    __slots__ = ("device", "stream", "view", "g", "P", "W", "H", "geom", "img", "radii", "out_color", "out_invdepth",
                 "out_extra", "fsgs", "extra", "cache", "use_order", "use_limit", "static", "cur", "status", "early")

    def __init__(self, device, stream, view, g, P, W, H, geom, img, radii, out_color, out_invdepth, out_extra, fsgs, extra,
                 cache, use_order, use_limit, static):
        self.device, self.stream, self.view, self.g = device, stream, view, g
        self.P, self.W, self.H = P, W, H
        self.geom, self.img, self.radii = geom, img, radii
        self.out_color, self.out_invdepth, self.out_extra = out_color, out_invdepth, out_extra
        self.fsgs, self.extra = fsgs, extra
        self.cache, self.use_order, self.use_limit, self.static = cache, use_order, use_limit, static
        self.cur = self.status = self.early = None


class _Last:
    """The last non-empty forward, as its backward finds it - by its geometry buffer, the object itself: the structs it built
    (and the tensors they point into) and whether it read raw rows.  When it armed the early side launch of a two-phase
    train step (RasterBackend.launch_uninstanced_early): that `step`, the forward's radii and image buffer, and once the
    launch is issued its `done` event; a fused backward ends the arming.  `binning`, `cap`: the binning buffer of a deferred
    region-binned forward and its capacity (what an early geometry pass of the next view would fill its buckets in)."""
    __slots__ = ("geom", "P", "view", "g", "keep", "raw", "step", "radii", "img", "done", "binning", "cap")

    def __init__(self, geom, P, view, g, keep, raw):
        self.geom, self.P, self.view, self.g, self.keep, self.raw = geom, P, view, g, keep, raw
        self.step = self.radii = self.img = self.done = self.binning = self.cap = None


class _Early:
    """An early geometry pass (RasterBackend.request_early_geometry) that has been issued: the view it was computed for and the
    rows it read (as the bytes of their structs), the caller's token, the buffers it wrote - the previous forward's geom / img /
    binning and a radii array of its own -, the limit table it read, and the event recorded behind it."""
    __slots__ = ("view", "g", "token", "P", "geom", "img", "binning", "cap", "radii", "limit", "limit_version", "event", "keep")


class RasterBackend:
    """Binds one implementation of the C ABI (`api`) to one torch device type."""

    def __init__(self, api, device_type="cuda"):
        self.api = api
        self.device_type = device_type
        self._pinned = None
        # optimistic binning capacity (instances): skips the forward's host sync when the previous
        # call's num_rendered is a good predictor; see rasterize_gaussians().
        self._capacity_hint = 0
        self._capacity_hint_limited = 0
        self.optimistic = os.environ.get("GS_SYNC_FORWARD", "0") != "1"
        # instance lists: True = drop (tile, Gaussian) pairs no pixel of which can reach alpha >= 1/255
        # (csrc/gs_tilecull.h; same images / gradients, ~2.6x fewer instances); GS_TILE_CULL=0 = the
        # reference's bounding-square lists, bit-identical point_list / ranges / num_rendered
        self.tile_cull = os.environ.get("GS_TILE_CULL", "1") != "0"
        # how the culled lists are built: "region" = region binning (csrc/gs_regionbin.hip, GsView.tile_cull = 2: two launches),
        # "lsd" = depth sort + emission + partition by tile (csrc/gs_binning.hip, 23 launches).  Same lists tile by tile.
        # "auto" (default): region binning, except for forwards WITHOUT depth limits whose lists are known to be long (more
        # than REGION_AUTO_MAX instances per region at the capacity the previous views needed: ~5 000 Gaussians per region) -
        # a region's bitonic sort grows as n log^2 n and its bucket atomics as n, so beyond that the LSD path is as fast or
        # faster (C3 full culled lists, 9.55 M instances: preprocess + binning 0.44 ms with regions, 0.42 ms LSD; depth-limited,
        # 1.86 M: 0.20 vs 0.30)
        self.binning = os.environ.get("GS_BINNING", "auto")
        self.last_deferred_num_rendered = None  # instance count of the last deferred forward whose verdict was collected
        self._region_off = set()   # (P, W, H, limited lists?) whose regions hold more Gaussians than one workgroup sorts: LSD path
        self._cap_memo = {}
        self._scratch_memo = {}
        self._cap_by_buffer = {}
        self._cam_cache = {}
        # one-shot identity of the camera of the NEXT forward (GaussianRasterizer.camera_key); None = hash the view matrix
        self.camera_key = None
        # one-shot, set with camera_key by GaussianRasterizer: the caller named the camera and did not decline depth limits
        # (GaussianRasterizer.camera_limits) - the forward may use this camera's verified limits as with GS_DEPTH_LIMIT=1
        self.camera_key_limits = False
        self._vm_ids = {}
        self.camera_cache_stats = dict(hits=0, misses=0, hashed=0)
        self.order_hint_on = True   # (False: image order - outputs do not depend on it, see GsScratch.tile_order_hint)
        # depth-limited emission (GsScratch.tile_depth_limit): on the second and later visits of a camera, (tile, Gaussian)
        # pairs behind the depth at which that tile's blend stopped last time are not emitted.  Checked, not assumed: the
        # forward flags lists that were cut too short and the view is rendered again without limits - which the host
        # can only know once the blend has finished.  Waiting for that inside the forward costs more than the shorter sort
        # saves (C3: 1.43 -> 1.60 ms/step), so it is OFF unless asked for (GS_DEPTH_LIMIT=1), and the train step asks for
        # the deferred form instead: `depth_limit_request = "defer"` (one-shot, next forward) leaves the verdict in
        # `self.deferred` for the caller to collect later - gsplat_amd.trainer does, its step kernel being a no-op on the
        # device when the flag is set.  Only with tile_cull.
        self.depth_limit_on = os.environ.get("GS_DEPTH_LIMIT", "0") == "1"
        self.depth_limit_request = None
        self.deferred = None
        self._status_ring = {}
        self.depth_limit_stats = dict(used=0, failed=0)
        self._pinned_by_device = {}
        # one-shot output arena for the next backward: {"means3D": [P,3], "sh": [P,M,3]} fp32 tensors to write
        # dL_dmeans3D / dL_dsh INTO (e.g. views of a flat gradient buffer) instead of fresh allocations
        self.grad_arena = None
        # capture-safe forward (hipGraph): a fixed binning capacity (instances) instead of the predicted one, no host
        # wait, no host read.  The forward then returns the CAPACITY in place of num_rendered (the kernels read the real
        # count from the device header; the backward only uses the value as an upper bound) and never re-runs: the
        # caller checks `last_num_rendered()` against the capacity after the stream has drained.
        self.static_capacity = None
        self.static_step_tag = None   # capture-safe mode: device word the captured gs_forward_status copies out with the status
        # one-shot request for the next backward: a gsplat_amd.capi.GsStepState (+ the tensors it points into, kept alive
        # by the caller) - run gs_backward_step (backward + activation backward + view statistics + Adam in the same
        # per-Gaussian kernel) instead of gs_backward; the backward then returns no gradients at all
        self.fused_step = None
        self._side_streams = {}
        self._rows_ws = {}        # (device, bytes) -> [persistent gradient-row workspace of the fused step, rows all zero?]
        self.rows_epoch = 0       # bumped whenever a fused backward found (or may have left) that workspace dirty
        self._last = None         # the last non-empty forward (_Last)
        self.two_phase_launches = 0
        self._uninst_done = None
        # one-shot, set together with fused_step by the train step: the opacities / scales / rotations of the next forward
        # (and of its gs_backward_step) are the model's RAW rows, activated inside the kernels
        # (GsGaussians.raw_activations): no activation kernel, no activated copies
        self.raw_activations = False
        # one-shot, set before a forward / a fused backward on raw rows: the model's _features_rest [P,M-1,3]; `sh` is then
        # _features_dc [P,1,3] (GsGaussians.shs_rest: the kernels read the split rows, no torch.cat)
        self.sh_rest = None
        # one-shot, set WITH sh_rest by gsplat_amd.accel (the `dc=` rasterizer call): the split rows hold ACTIVATED values - the
        # forward is the ordinary one on split rows, the backward gs_backward_split.  Without it split rows go with raw activations
        self.sh_rest_activated = False
        # parity probes: keep the backward workspace (the per-Gaussian 16-slot float64 gradient rows of the blend backward)
        self.keep_workspace = False
        self.last_workspace = None
        self._zero_images = {}    # (device, H, W) -> [1,H,W] zeros (_zero_image)
        # the early geometry pass (see EARLY_GEOMETRY): the caller's one-shot request for the view that comes next, its one-shot
        # token of the forward that may use the result, the pass in flight (_Early), and what became of the passes so far
        self.early_request = None
        self.early_token = None
        self._early = None
        self.early_geometry_stats = dict(issued=0, used=0, stale=0)

    # ------------------------------------------------------------------ helpers
    def _stream(self, device):
        if device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        return None

    def _check_device(self, t):
        if t.device.type != self.device_type:
            raise RuntimeError(
                "gsplat %s backend got a tensor on %s - the rasterizer has no fallback path"
                % (self.device_type, t.device))

    def _tile_cull(self, device):
        """GsView.tile_cull of this backend's views: 0 = the reference's lists, 1 = culled lists built by the LSD path,
        2 = by region binning.  (A forward may still take the LSD path for its own lists, see rasterize_gaussians; the
        backward only asks whether they were culled.)"""
        cull = int(self.tile_cull)
        if cull and self.binning in ("region", "auto") and device.type == "cuda":
            return 2
        return cull

    def _view(self, keep, device, bg, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, scale_modifier,
              degree, prefiltered, antialiasing, debug, tile_cull=None):
        v = GsView()
        v.image_height, v.image_width = int(H), int(W)
        v.tanfovx, v.tanfovy = float(tanfovx), float(tanfovy)
        v.scale_modifier = float(scale_modifier)
        v.sh_degree = int(degree)
        v.prefiltered, v.antialiasing, v.debug = int(bool(prefiltered)), int(bool(antialiasing)), int(bool(debug))
        if self.force_rowwise_entries:   # (test hook: GsView.debug bit 1, csrc/gs_tilebin.hip)
            v.debug |= 2
        v.tile_cull = self._tile_cull(device) if tile_cull is None else tile_cull
        bg, viewmatrix, projmatrix, campos = (_prep(x, device) for x in (bg, viewmatrix, projmatrix, campos))
        keep += [bg, viewmatrix, projmatrix, campos]
        v.bg, v.viewmatrix, v.projmatrix, v.campos = _ptr(bg), _ptr(viewmatrix), _ptr(projmatrix), _ptr(campos)
        return v

    def _gauss(self, keep, device, means3D, sh, colors, opacities, scales, rotations, cov3D, extra=None, raw=False,
               extra_gain=None, sh_rest=None):
        g = GsGaussians()
        g.raw_activations = int(bool(raw))
        extra = _prep(extra, device)
        keep.append(extra)
        g.extra_channel = _ptr(extra)
        if extra_gain is not None:  # raw mode: extra holds the RAW row, activated in the kernels with this device scalar
            extra_gain = _prep(extra_gain, device)
            keep.append(extra_gain)
            g.extra_gain = _ptr(extra_gain)
        means3D, sh, colors, opacities, scales, rotations, cov3D = (
            _prep(x, device) for x in (means3D, sh, colors, opacities, scales, rotations, cov3D))
        keep += [means3D, sh, colors, opacities, scales, rotations, cov3D]
        g.P = int(means3D.shape[0]) if means3D is not None else 0
        g.M = int(sh.shape[1]) if sh is not None else 0
        if sh_rest is not None:
            if sh is None or int(sh.shape[1]) != 1 or sh_rest.shape[0] != sh.shape[0]:
                raise RuntimeError("sh_rest goes with sh = the DC rows [P,1,3]")
            sh_rest = _prep(sh_rest, device)
            keep.append(sh_rest)
            g.M = 1 + int(sh_rest.shape[1])
            g.shs_rest = _ptr(sh_rest)
        g.means3D, g.shs, g.colors_precomp, g.opacities = _ptr(means3D), _ptr(sh), _ptr(colors), _ptr(opacities)
        g.scales, g.rotations, g.cov3D_precomp = _ptr(scales), _ptr(rotations), _ptr(cov3D)
        return g

    def _update_hint(self, num_rendered, limited=False):
        # 25 % head-room over the largest recent instance count; decays slowly so one huge view does not pin
        # the capacity (and the 16 B/instance buffer) forever.  Quantised to 1/8-octave steps so that consecutive steps
        # ask for the SAME number of bytes: the caching allocator then hands back the same block every step.
        # Depth-limited views keep their own hint: their lists are several times shorter, and the sort's grids, its
        # histogram tables and the row scan are sized by the capacity, not by the count on the device.
        import math
        old = self._capacity_hint_limited if limited else self._capacity_hint
        want = max(int(num_rendered * 1.25) + 4096, int(old * 0.98))
        new = int(2.0 ** (math.ceil(math.log2(want) * 8.0) / 8.0))
        if limited:
            self._capacity_hint_limited = new
        else:
            self._capacity_hint = new

    def _remember_capacity(self, binning, cap):
        """The binning buffer travels through autograd as a bare byte tensor; its capacity (instances) is kept here, keyed
        by the buffer's address and length, so backward need not recover it by search."""
        if len(self._cap_by_buffer) > 256:
            self._cap_by_buffer.clear()
        self._cap_by_buffer[(binning.data_ptr(), binning.numel())] = int(cap)

    def _capacity_of(self, P, W, H, nbytes, at_least):
        """Instances the binning buffer of `nbytes` bytes was sized for (largest cap with bytes(cap) <= nbytes); only
        reached for buffers this backend did not allocate itself (see _remember_capacity)."""
        key = (P, W, H, nbytes)
        cap = self._cap_memo.get(key)
        if cap is None:
            lo, hi = int(at_least), max(int(at_least), 1)
            while self.scratch_bytes(P, W, H, hi)[2] <= nbytes:
                lo, hi = hi, hi * 2
            while lo < hi - 1:
                mid = (lo + hi) // 2
                if self.scratch_bytes(P, W, H, mid)[2] <= nbytes:
                    lo = mid
                else:
                    hi = mid
            cap = lo
            if len(self._cap_memo) > 64:
                self._cap_memo.clear()
            self._cap_memo[key] = cap
        return cap

    def last_num_rendered(self):
        """num_rendered of the most recent forward on the current device / stream as the device reported it (pinned
        host word written by an asynchronous copy: only valid once that forward has completed)."""
        return None if self._pinned is None else int(self._pinned[0])

    def take_deferred(self):
        """The pending verdict of the last forward run with depth_limit_request = "defer", or None.  -> callable that
        waits for that forward and returns True when its limits held (outputs valid) - on False it has already
        invalidated the camera's limits, and the caller must discard everything computed from that forward.
        (Only depth-limited forwards defer their verdict: see _forward_lists for the record.)"""
        d, self.deferred = self.deferred, None
        if d is None:
            return None

        def verdict():
            d["event"].synchronize()
            st = tuple(int(x) for x in d["status"][:4])
            ok = st[1] == 0 and st[2] == 0
            regions = d["regions"]
            if regions:
                # region binning learns the instance count only here: keep the capacity hint current, and tell a capacity
                # overflow (render again with more room, the limits were fine) from limits that proved too tight
                if st[3] > self.REGION_MAX_ENTRIES:
                    self._region_off.add(d["size"])
                self._update_hint(max(st[0], st[3] * regions), limited=True)
                self.last_deferred_num_rendered = st[0]
            if not ok:
                self.drop_early_geometry()   # (the step is repeated: what comes next is not the view the pass was made for)
                self.depth_limit_stats["failed"] += 1
                if st[2] != 0 or not regions:
                    d["cache"]["limit_ok"] = False
                if st[2] != 0:
                    self.limits_failed(d["cache"])
            else:
                self.limits_held(d["cache"])
            return ok
        return verdict

    def last_status(self):
        """(num_rendered, overflow, trunc_failed) of the most recent forward that copied its status out
        (gs_forward_status: the capture-safe mode and depth-limited forwards do); valid once it has completed."""
        return None if self._pinned is None else tuple(int(x) for x in self._pinned[:3])

    def _capacity_for(self, binning, P, W, H, R):
        if binning.numel() == 0:
            return R
        cap = self._cap_by_buffer.get((binning.data_ptr(), binning.numel()))
        if cap is not None and cap >= R:
            return cap
        return self._capacity_of(P, W, H, binning.numel(), R)

    def scratch_bytes(self, P, W, H, R):
        # (a pure function of four integers, asked two or three times per forward and once per backward: remembered)
        key = (int(P), int(W), int(H), int(R))
        memo = self._scratch_memo
        got = memo.get(key)
        if got is None:
            out = (C.c_size_t * 3)()
            ws = C.c_size_t(0)
            self.api.call("scratch_bytes", P, W, H, R, out, C.byref(ws))
            if len(memo) > 256:
                memo.clear()
            got = memo[key] = (out[0], out[1], out[2], ws.value)
        return got

    def _camera_identity(self, viewmatrix):
        """Who is this camera?  An explicit key when the caller gave one (GaussianRasterizer.camera_key), else a hash of the
        view matrix's CONTENTS - remembered per tensor object and version, so a loop that keeps one tensor per camera pays
        one 64-byte device-to-host copy per camera, and one that re-creates its camera tensors every step still finds its
        state (at the price of that copy per step; pass a key to avoid it).  An address alone is not an identity: the
        allocator hands a freed block to the next camera."""
        ck, self.camera_key = self.camera_key, None
        if ck is not None:
            return ("key", ck)
        import hashlib
        import weakref
        ent = self._vm_ids.get(id(viewmatrix))
        if ent is not None and ent[0]() is viewmatrix and ent[1] == viewmatrix._version:
            return ent[2]
        self.camera_cache_stats["hashed"] += 1
        ident = ("hash", hashlib.blake2b(viewmatrix.detach().to("cpu", torch.float32).contiguous().numpy().tobytes(),
                                         digest_size=8).hexdigest())
        if len(self._vm_ids) > 1024:
            self._vm_ids = {k: v for k, v in self._vm_ids.items() if v[0]() is not None}
        try:
            self._vm_ids[id(viewmatrix)] = (weakref.ref(viewmatrix), viewmatrix._version, ident)
        except TypeError:
            pass
        return ident

    def _camera_cache(self, device, W, H, viewmatrix):
        """What the previous visit of the SAME camera measured, per tile:
        order - the launch order for the forward blend (GsScratch.tile_order_hint; a hint from another camera is
                worthless: 0.203 ms either way at C3; from the same camera 0.204 -> 0.164 ms, tests/tools/fwd_order_probe.py);
        limit - the depth at which each tile's blend stopped (GsScratch.tile_depth_limit).
        Cameras are told apart by _camera_identity.  A stale or foreign entry costs time, never correctness (the order is
        pure scheduling - any permutation of the tiles renders the same image - and the limits are verified by the
        forward).  Both buffers hold valid contents from the start (the default order, +inf = no limit) and the kernels
        leave them alone when a forward overflowed, so whatever is read from them is safe.
        -> dict(order, order_ok, limit, limit_ok) or None"""
        if device.type != "cuda" or not (self.order_hint_on or self.depth_limit_on or self.depth_limit_request is not None
                                         or self.static_capacity is not None or self.camera_key_limits):
            self.camera_key = None
            return None
        key = (device.index, W, H, self._camera_identity(viewmatrix))
        c = self._cam_cache.get(key)
        if c is None:
            self.camera_cache_stats["misses"] += 1
            if len(self._cam_cache) >= self.CAMERA_CACHE_MAX:
                # forget the oldest camera nobody pinned (a captured hipGraph holds the ADDRESSES of its camera's buffers:
                # GraphedStep pins the entry for as long as the graph lives)
                for k in self._cam_cache:
                    if not self._cam_cache[k].get("pinned"):
                        self._cam_cache.pop(k)
                        break
            T = ((W + 15) // 16) * ((H + 15) // 16)
            per_xcd = (T + 7) // 8
            b = torch.arange(per_xcd * 8, dtype=torch.int64)
            default_order = ((b & 7) * per_xcd + (b >> 3)).to(torch.int32)  # the kernel's own XCD-banded mapping
            c = self._cam_cache[key] = dict(order=default_order.to(device), order_ok=False,
                                            limit=torch.full((int(self.api.raw("tile_depth_limit_floats")(W, H)),), float("inf"),
                                                             dtype=torch.float32, device=device),
                                            limit_ok=False, key=key,
                                            # adaptive slack on the exported bounds (GsScratch.tile_depth_limit_slack)
                                            slack=torch.ones((1,), dtype=torch.float32, device=device), slack_level=0, held=0)
        else:
            self.camera_cache_stats["hits"] += 1
        return c

    CAMERA_CACHE_MAX = 256

    def drop_camera_entries(self, key_prefix):
        """Forget the per-camera state filed under explicit keys that start with `key_prefix` (a trainer that is gone:
        its keys are ("trainer", uid, camera index)); pinned entries too - their graphs died with the trainer."""
        n = len(key_prefix)
        for k in [k for k in self._cam_cache if k[3][0] == "key" and isinstance(k[3][1], tuple) and k[3][1][:n] == key_prefix]:
            self._cam_cache.pop(k, None)

    def camera_entry(self, W, H, viewmatrix=None, camera_key=None, device_index=None):
        """The per-camera state kept for a camera (by explicit key, or by the contents of its view matrix), or None - a
        lookup that creates nothing and counts nothing (tests, tools)."""
        if camera_key is not None:
            ident = ("key", camera_key)
        else:
            saved, self.camera_key = self.camera_key, None
            hashed = self.camera_cache_stats["hashed"]
            ident = self._camera_identity(viewmatrix)
            self.camera_key, self.camera_cache_stats["hashed"] = saved, hashed
        if device_index is None:
            device_index = viewmatrix.device.index if viewmatrix is not None and viewmatrix.is_cuda else torch.cuda.current_device()
        return self._cam_cache.get((device_index, int(W), int(H), ident))

    # Adaptive slack of a camera's depth bounds.  The fixed margin (5 % + 0.02 in view depth) holds while the model moves
    # slowly between two visits of a camera (a run that is converging: 2 repeated views in 2 000 at C3); early in training,
    # or on a target the model cannot fit, tiles keep saturating deeper than their last bound allowed (38 % repeated views
    # on bench.py's unrelated target after a few hundred steps).  So the bounds a camera EXPORTS are multiplied by a factor
    # that rises when its limits fail and falls again after they have held for a while: longer lists instead of repeats.
    SLACK = (1.0, 1.25, 1.6, 2.5)
    SLACK_RELAX_AFTER = 24

    def limits_failed(self, c):
        if c is None:
            return
        c["held"] = 0
        if c["slack_level"] < len(self.SLACK) - 1:
            c["slack_level"] += 1
            c["slack"].fill_(self.SLACK[c["slack_level"]])

    def limits_held(self, c):
        if c is None:
            return
        c["held"] += 1
        if c["held"] >= self.SLACK_RELAX_AFTER and c["slack_level"] > 0:
            c["held"] = 0
            c["slack_level"] -= 1
            c["slack"].fill_(self.SLACK[c["slack_level"]])

    @staticmethod
    def _scratch(geom, img=None, binning=None, capacity=0):
        s = GsScratch()
        s.geom, s.geom_bytes = _ptr(geom), geom.numel()
        if img is not None:
            s.img, s.img_bytes = _ptr(img), img.numel()
        if binning is not None:
            s.binning, s.binning_bytes = _ptr(binning), binning.numel()
        s.binning_capacity = int(capacity)
        return s

    # ------------------------------------------------------------------ forward
    # The two-phase train step (gs_step_uninstanced): the Adam update of the Gaussians that emitted no instance in this view
    # is launched on a side stream right before the fused backward and runs NEXT TO the backward blend; the per-Gaussian
    # kernel of gs_backward_step (phase 2) waits for it.  From TWO_PHASE_MIN_P Gaussians on (below, the extra launch and
    # the stream hand-offs cost more than the hidden stream saves); GS_TWO_PHASE_STEP=0 switches it off.
    # depth-limited lists for callers that name their cameras (GaussianRasterizer.camera_key); GS_KEYED_LIMITS=0: never
    force_rowwise_entries = False

    # region binning: which form of the forward geometry kernel fills the buckets (gs_region_coop: True = a wave shares the
    # regions of its large footprints, False = every lane walks its own; same lists bit for bit).  Process-wide, like the
    # library's GS_REGION_COOP it overrides; only the device library has it.
    @property
    def region_coop(self):
        return bool(self.api.raw("region_coop")(-1))

    @region_coop.setter
    def region_coop(self, on):
        self.api.raw("region_coop")(int(bool(on)))

    # test hook: called as scratch_fill(kind, tensor) right after each fresh scratch buffer of rasterize_gaussians is allocated
    # (kind "geom", "img", "binning"), so that a test decides what the buffer holds before the forward runs instead of the
    # caching allocator (tests/test_gpu_scratch_reuse.py); None: nothing happens
    scratch_fill = None
    # test hook: called as output_fill(kind, tensor) for each output tensor of rasterize_gaussians ("color", "invdepth", "radii",
    # "extra") before any kernel runs, so that a test can plant a pattern and see an element nobody wrote; None: nothing happens
    output_fill = None
    KEYED_LIMITS = os.environ.get("GS_KEYED_LIMITS", "1") != "0"
    # region-binned forwards whose verdict is collected later (deferred eager steps, replayed graphs): the status block is
    # written into the pinned host block by the forward's own last kernel (GsScratch.status_host) instead of by a copy
    # command behind it - one launch less on the stream.  False: gs_forward_status as before.
    STATUS_IN_RENDER = True

    def _side_stream(self, device):
        side = self._side_streams.get(device.index)
        if side is None:
            side = self._side_streams[device.index] = torch.cuda.Stream(device=device)
        return side
    TWO_PHASE = os.environ.get("GS_TWO_PHASE_STEP", "1") != "0"
    TWO_PHASE_MIN_P = 100_000
    # GsStepState.reached_split: the fused step's tail counts a Gaussian as instanced only when the backward blend visits one of
    # its list entries (the forward blend leaves the flags); the others - accepted by a tile, but behind every pixel's
    # saturation - take their zero-gradient step on the side stream.  GS_REACHED_SPLIT=0 (which also stops the library's
    # forward from writing the flags) or False: the split stays on tiles_touched.
    REACHED_SPLIT = os.environ.get("GS_REACHED_SPLIT", "1") != "0"

    # The early geometry pass (gs_forward_geometry_early): a train step that knows its next camera has the
    # geometry kernel of THAT view run on the side stream, right behind the Adam stream of this step's unreached Gaussians, over the
    # 256-row blocks without a reached row - their parameters are final there - and in place: into this forward's own buffers,
    # which the next forward then takes over.  What stays in front of the next forward blend is one launch over the blocks the
    # step's tail has just written.  Same lists, records, images and gradients, bit for bit.  GS_EARLY_GEOMETRY=0 or False: off.
    EARLY_GEOMETRY = os.environ.get("GS_EARLY_GEOMETRY", "1") != "0"

    def request_early_geometry(self, settings, camera_key, token):
        """One-shot, before the forward of a fused two-phase train step: `settings` (a GaussianRasterizationSettings) and
        `camera_key` of the view the caller will render NEXT with the same Gaussians.  `token`: anything that compares equal only
        while nothing but this step's own backward has written the rows; the caller sets `early_token` to its current value before
        that next forward, which uses the early result only if the two are equal and it is the very view, rows and limit table."""
        self.early_request = (settings, camera_key, token) if self.EARLY_GEOMETRY else None

    def _retire_early(self, e):
        """An early pass nobody will use: the current stream is ordered behind it, so that its buffers - about to go back to the
        allocator - are not handed to work that runs while it still writes them."""
        self.early_geometry_stats["stale"] += 1
        torch.cuda.current_stream(e.geom.device).wait_event(e.event)

    def drop_early_geometry(self):
        """Forget an early pass in flight (its view is not the one that comes next after all: a step that is being repeated)."""
        if self._early is not None:
            self._retire_early(self._early)
        self._early = self.early_request = None

    def join_early_geometry(self):
        """Order the current stream behind an early pass in flight - it reads the parameter rows - and keep it (no-op without)."""
        if self._early is not None:
            torch.cuda.current_stream(self._early.geom.device).wait_event(self._early.event)

    def _launch_early_geometry(self, f, side):
        """Behind the side launch just issued on `side` for the forward `f` (_Last): the early pass its caller asked for, if
        every condition holds.  Not for a capture-safe forward, under the test hooks that plant patterns in fresh buffers, rows
        that are not the raw parameter arrays on the float4 grid, or a gradient-row workspace that still needs its clear launch
        (that launch reads tiles_touched)."""
        req, self.early_request = self.early_request, None
        if self._early is not None:
            self._retire_early(self._early)
        self._early = None
        if (req is None or not self.EARLY_GEOMETRY or not self.REACHED_SPLIT or os.environ.get("GS_REACHED_SPLIT", "1") == "0"
                or f.binning is None or f.view.tile_cull != 2 or not f.raw or self.static_capacity is not None
                or self.scratch_fill is not None or self.output_fill is not None or f.step.rows_override
                or not hasattr(self.api, "_forward_geometry_early")):
            return
        rs, camera_key, token = req
        device, g = f.geom.device, f.g
        H, W = int(rs.image_height), int(rs.image_width)
        if (H, W) != (f.view.image_height, f.view.image_width) or g.extra_channel or g.shs_rest or g.colors_precomp or g.cov3D_precomp:
            return
        if any((p or 0) % 16 for p in (g.means3D, g.shs, g.opacities, g.scales, g.rotations)):
            return
        ws = self._rows_ws.get((device.index, self.scratch_bytes(f.P, W, H, 0)[3]))
        if ws is None or not ws[1]:
            return
        c = self._cam_cache.get((device.index, W, H, ("key", camera_key)))
        if c is None or not c["limit_ok"]:   # (the next forward will not be a depth-limited one: it sizes its own buffers)
            return
        e = _Early()
        e.keep = list(f.keep)
        e.view = self._view(e.keep, device, rs.bg, rs.viewmatrix, rs.projmatrix, rs.campos, rs.tanfovx, rs.tanfovy, H, W,
                            rs.scale_modifier, rs.sh_degree, rs.prefiltered, rs.antialiasing, rs.debug, tile_cull=2)
        e.g, e.token, e.P, e.geom, e.img, e.binning, e.cap, e.limit = g, token, f.P, f.geom, f.img, f.binning, f.cap, c["limit"]
        e.limit_version = e.limit._version   # (the forward's own last kernel rewrites the table through the library, in stream
        #  order in front of this pass; a write through torch - a test that plants bounds - makes the pass stale)
        e.radii = torch.empty((f.P,), dtype=torch.int32, device=device)
        s = self._scratch(e.geom, e.img, e.binning, e.cap)
        s.tile_depth_limit = e.limit.data_ptr()
        self.api.call("forward_geometry_early", C.byref(e.view), C.byref(g), C.byref(s), e.radii.data_ptr(),
                      C.c_void_p(side.cuda_stream))
        e.event = torch.cuda.Event()
        e.event.record(side)
        self._early = e
        self.early_geometry_stats["issued"] += 1

    def _take_early_geometry(self, view, g, P, limit, request, static, fsgs, extra):
        """The early pass in flight if the forward that starts now may use it (see request_early_geometry), else None; either
        way it is not in flight any more."""
        e, self._early = self._early, None
        token, self.early_token = self.early_token, None
        if e is None:
            return None
        # (... and only with the binning buffer this forward would have sized for itself)
        hint = self._capacity_hint_limited if self._capacity_hint_limited > 0 else self._capacity_hint
        cap = max(hint if hint > 0 else max(8 * P, 1 << 20), _regions(view.image_width, view.image_height))
        if (self.EARLY_GEOMETRY and cap == e.cap and token is not None and token == e.token and request == "defer" and not static and not fsgs
                and extra is None and limit is e.limit and limit._version == e.limit_version and self.fused_step is not None and self.scratch_fill is None
                and self.output_fill is None and P == e.P and bytes(view) == bytes(e.view) and bytes(g) == bytes(e.g)
                and self._arms_side_launch(self.fused_step, P)):
            return e
        self._retire_early(e)
        return None

    def _two_phase(self, step, P):
        """Does the fused backward of `step` over P Gaussians run in two phases?  (Not its gradients-out form; with
        rows_override it does, and issues the side launch itself: see _arms_side_launch.)"""
        return self.TWO_PHASE and P >= self.TWO_PHASE_MIN_P and not step.grad_out[0]

    def _arms_side_launch(self, step, P):
        """Does a forward whose backward is `step`'s arm the early side launch (launch_uninstanced_early)?  Only without
        rows_override."""
        return self._two_phase(step, P) and not step.rows_override

    def launch_uninstanced_early(self):
        """Issue the side launch of the two-phase step NOW (everything enqueued so far on the current stream - the forward,
        the criterion's forward - is waited for by the side stream; what the caller enqueues next runs beside it).  No-op
        unless the last forward armed it.  The rasterizer's backward then only waits for it."""
        f = self._last
        if f is None or f.step is None or f.done is not None:
            return False
        f.done = self._launch_uninstanced(f.geom.device, f.view, f.g, f.radii, self._scratch(f.geom, f.img), f.step)
        self._launch_early_geometry(f, self._side_stream(f.geom.device))
        return True

    def _structs(self, device, bg, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix,
                 projmatrix, campos, tanfovx, tanfovy, H, W, scale_modifier, degree, antialiasing, debug, extra=None, raw=False,
                 extra_gain=None, sh_rest=None):
        """-> (GsView, GsGaussians, tensors they point into) built again for a backward: not prefiltered, the backend's own
        kind of lists (_tile_cull)."""
        keep = []
        view = self._view(keep, device, bg, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, scale_modifier, degree,
                          False, antialiasing, debug)
        g = self._gauss(keep, device, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, extra, raw=raw,
                        extra_gain=extra_gain, sh_rest=sh_rest)
        return view, g, keep

    def _launch_uninstanced(self, device, view, g, radii, s, step):
        main = torch.cuda.current_stream(device)
        # (a CU-masked side stream - hipExtStreamCreateWithCUMask, 64 / 96 / 128 CUs - was tried in round 4: the two
        #  queues then did not overlap at all, every kernel of the step ran ~10 % slower, step 0.98 -> 1.18-1.20 ms)
        side = self._side_stream(device)
        side.wait_stream(main)   # (the forward blend has decided overflow / trunc_failed and left the reached flags)
        step.reached_split = int(self.REACHED_SPLIT)   # (the backward takes the same struct: phase 2 splits the same way)
        self.api.call("step_uninstanced", C.byref(view), C.byref(g), radii.contiguous().data_ptr(), C.byref(s),
                      C.byref(step), C.c_void_p(side.cuda_stream))
        done = torch.cuda.Event()
        done.record(side)
        self.two_phase_launches += 1
        return done

    def rasterize_gaussians(self, bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier,
                            cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, image_height, image_width,
                            sh, degree, campos, prefiltered, antialiasing, debug, extra=None, fsgs=False, extra_gain=None):
        """= RasterizeGaussiansCUDA (rasterize_points.cu:35-124).

        Returns (num_rendered, color[3,H,W], radii[P] int32, geomBuffer, binningBuffer, imgBuffer,
        invdepth[1,H,W]).  binningBuffer carries its capacity in its length (see _capacity).
        extra [P] (not part of the reference's signature): a 4th per-Gaussian channel blended in the same
        pass (gs_forward_render_x); the tuple then ends with its image [1,H,W].
        fsgs=True: the older generation of FSGS / DNGaussian (gs_forward_render_fsgs): the "invdepth" slot of the
        tuple holds depth = sum depth alpha T and the tuple ends with alpha = sum alpha T, both [1,H,W].  It takes the
        one-shot `raw_activations` like the newer generation (the geometry phase is shared); with a `fused_step` armed its
        backward is gs_backward_step_fsgs, and depth limits and the capture-safe forward are refused."""
        if fsgs and (extra is not None or antialiasing):
            raise RuntimeError("the FSGS rasterizer generation has neither anti-aliasing nor a 4th channel")
        if means3D.ndim != 2 or means3D.shape[1] != 3:
            raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:58-60
        self._check_device(means3D)
        device = means3D.device
        P, H, W = int(means3D.shape[0]), int(image_height), int(image_width)
        f32 = dict(dtype=torch.float32, device=device)
        u8 = dict(dtype=torch.uint8, device=device)
        # every pixel and every radius is written by the kernels (gs_forward_geometry / gs_forward_render): empty, not
        # zeros - the reference's three fills (rasterize_points.cu:71-75) are only needed for P == 0
        alloc = torch.empty if P != 0 else torch.zeros
        out_color = alloc((NUM_CHANNELS, H, W), **f32)
        out_invdepth = alloc((1, H, W), **f32)
        radii = alloc((P,), dtype=torch.int32, device=device)
        out_extra = None if (extra is None and not fsgs) else alloc((1, H, W), **f32)
        tail = () if out_extra is None else (out_extra,)
        if self.output_fill is not None and P != 0:
            for kind, t in (("color", out_color), ("invdepth", out_invdepth), ("radii", radii), ("extra", out_extra)):
                if t is not None:
                    self.output_fill(kind, t)
        # (the one-shot requests of this forward are taken here, whatever follows: an empty model must not leave them armed)
        raw, self.raw_activations = self.raw_activations, False
        sh_rest, self.sh_rest = self.sh_rest, None
        sh_activated, self.sh_rest_activated = self.sh_rest_activated, False
        self._last = None
        if P == 0:  # rasterize_points.cu:88
            self.camera_key, self.camera_key_limits, self.depth_limit_request = None, False, None
            e = torch.empty((0,), **u8)
            return (0, out_color, radii, e, e.clone(), e.clone(), out_invdepth) + tail
        # (split rows with ACTIVATED values: the `dc=` call of gsplat_amd.accel says so - the C forward reads them whatever `raw` is)
        if sh_rest is not None and not raw and (not sh_activated or fsgs or extra is not None):
            raise RuntimeError("split SH rows are served with raw activations only (gsplat_amd.render_raw), or on activated "
                               "values by the plain rasterizer call of gsplat_amd.accel")
        if fsgs and self.fused_step is not None:
            # the fused train step of the FSGS generation (gs_backward_step_fsgs) is the one-launch eager form only
            closed = None
            if self.static_capacity is not None:
                closed = "the capture-safe forward (GraphedStep, hipGraph replay) is"
            elif self.depth_limit_request is not None or self.depth_limit_on or self.camera_key_limits:
                closed = "depth-limited lists are"
            if closed is not None:   # (nothing stays armed behind the refusal)
                self.fused_step, self.depth_limit_request, self.camera_key, self.camera_key_limits = None, None, None, False
                raise RuntimeError("%s closed to the fused train step of the FSGS rasterizer generation" % closed)
        if (extra_gain is not None) != (raw and extra is not None):
            raise RuntimeError("extra_gain goes with a RAW 4th channel (raw activations), and only with it")
        if device.type == "cuda":
            self._join_tile_order(device)   # (a forward whose backward never ran: its hints must be complete before this one reads them)
        cache = self._camera_cache(device, W, H, viewmatrix)
        static = self.static_capacity is not None
        request, self.depth_limit_request = self.depth_limit_request, None
        keyed_limits, self.camera_key_limits = self.camera_key_limits and self.KEYED_LIMITS, False
        self.deferred = None
        use_limit = cache is not None and (self.depth_limit_on or request is not None or keyed_limits) and self.tile_cull
        # capture-safe mode always passes the limit buffer (+inf = no limit): the pointer is frozen into the graph
        limit = cache["limit"] if use_limit and (static or cache["limit_ok"]) else None

        tile_cull = self._tile_cull(device)
        # region binning, except for a size whose regions overfilled (_region_off) and, with binning = "auto", for long
        # un-limited lists.  (Depth-limited lists are several times shorter: a size whose FULL lists overfill a region still
        # bins its limited views by region - C2: 0.146 -> 0.04 ms of binning per step.)
        if tile_cull == 2 and ((P, W, H, limit is not None) in self._region_off or (
                self.binning == "auto" and limit is None and not static
                and self._capacity_hint > self.REGION_AUTO_MAX * _regions(W, H))):
            tile_cull = 1
        keep = []
        view = self._view(keep, device, bg, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, scale_modifier,
                          degree, prefiltered, antialiasing, debug, tile_cull=tile_cull)
        g = self._gauss(keep, device, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, extra, raw=raw,
                        extra_gain=extra_gain, sh_rest=sh_rest)

        early = self._take_early_geometry(view, g, P, limit, request, static, fsgs, extra) if device.type == "cuda" else None
        if early is not None:
            # (the previous forward's buffers, where the early pass has left most of this view's geometry, and its radii)
            geom, img, radii = early.geom, early.img, early.radii
        else:
            gb, ib, _, _ = self.scratch_bytes(P, W, H, 0)
            geom = torch.empty((gb,), **u8)
            img = torch.empty((ib,), **u8)
            if self.scratch_fill is not None:
                self.scratch_fill("geom", geom)
                self.scratch_fill("img", img)
        # (the train step's side launch and its backward describe the same view and the same Gaussians: they take these
        #  structs - and the tensors `keep` holds alive - instead of building them again)
        last = self._last = _Last(geom, P, view, g, keep, raw)
        step = self.fused_step
        if step is not None and not fsgs and device.type == "cuda" and self._arms_side_launch(step, P):
            last.step, last.radii, last.img = step, radii, img
        f = _Forward(device, self._stream(device), view, g, P, W, H, geom, img, radii, out_color, out_invdepth, out_extra, fsgs,
                     extra, cache, cache is not None and self.order_hint_on, use_limit, static)
        f.early = early

        if device.type != "cuda":
            nr = (C.c_int32 * 1)()
            self.api.call("forward_geometry", C.byref(view), C.byref(g), C.byref(self._scratch_of(f, None, 0, None)),
                          radii.data_ptr(), C.cast(nr, C.c_void_p), f.stream)
            num_rendered = int(nr[0])
            binning = self._new_binning(f, num_rendered)
            self._render(f, self._scratch_of(f, binning, num_rendered, None))
            return (num_rendered, out_color, radii, geom, binning, img, out_invdepth) + tail

        # one pinned status block per device AND stream: two forwards in flight on different streams must not share it
        # (capture-safe mode: one per device, created before the capture - pinned memory cannot be allocated inside).
        # Words: num_rendered, overflow, trunc_failed, 0 (gs_forward_status; gs_forward_geometry writes word 0 alone)
        f.cur = torch.cuda.current_stream(device)
        pkey = (device.index, "static" if static else f.cur.cuda_stream)
        status = self._pinned_by_device.get(pkey)
        if status is None:
            status = self._pinned_by_device[pkey] = torch.zeros((16,), dtype=torch.int32).pin_memory()
        self._pinned = f.status = status  # (last used: read by bench.py for the instance count of the last view)
        num_rendered, binning = self._forward_lists(f, limit, request == "defer")
        return (num_rendered, out_color, radii, geom, binning, img, out_invdepth) + tail

    REGION_MAX_ENTRIES = 16384  # csrc/gs_common.h RG_MAX_ENTRIES
    REGION_AUTO_MAX = 13000     # binning = "auto": instances of capacity per region above which un-limited forwards take the LSD path

    def _forward_lists(self, f, limit, defer):
        """Instance lists and blend of a forward on the GPU: with the camera's depth `limit` (when there is one), then - if
        the blend found a tile that needed entries the limits cut - again without.  -> (num_rendered, binning buffer)

        The verdict on the limits is known once the blend has finished.  The host waits for it here unless it goes to a
        status block for later: the capture-safe mode's (static_capacity: fixed capacity, no host wait, no host read, no
        re-run; num_rendered is the capacity and the caller reads last_status() once the stream has drained) or a deferred
        one (`defer`: a block of the status ring, collected with take_deferred)."""
        for lim in ((limit, None) if limit is not None else (None,)):
            deferred = defer and lim is not None and not f.static
            block = self._status_block(f.device) if deferred else (f.status if f.static else None)
            if f.view.tile_cull == 2:
                num_rendered, binning, s = self._lists_region(f, lim, block)
                if binning is None:
                    # a region holds more Gaussians than one workgroup sorts: this size goes through the LSD path from now on
                    f.view.tile_cull = 1
                    return self._forward_lists(f, limit, defer)
            else:
                num_rendered, binning, s = self._lists_lsd(f, lim)
            if lim is not None:
                self.depth_limit_stats["used"] += 1   # (capture-safe mode: at capture time only, replays do not pass here)
            if block is not None:
                if not s.status_host:   # (unless the forward's last kernel delivers the status block itself)
                    self.api.call("forward_status", C.byref(s), block.data_ptr(), f.stream)
                if deferred:
                    if s.defer_tile_order:
                        done = self._tile_order_on_side(f.view, s, f.cur)   # (the status block arrives with that kernel)
                    else:
                        done = torch.cuda.Event()
                        done.record(f.cur)
                    # (regions = 0: LSD lists, whose capacity this forward has checked already)
                    self.deferred = dict(status=block, event=done, cache=f.cache, size=(f.P, f.W, f.H, True),
                                         regions=_regions(f.W, f.H) if f.view.tile_cull == 2 else 0)
            elif lim is not None:
                # depth-limited lists: the blend has checked that every bounded tile saturated inside the part of its
                # list that is certainly complete; the host has to know before it hands the image out (this wait ends
                # when the blend does, the un-limited path's when the lists are built)
                self.api.call("forward_status", C.byref(s), f.status.data_ptr(), f.stream)
                f.cur.synchronize()
                if int(f.status[2]) != 0:  # some tile needed entries that were cut: forget the limits, do the view again
                    self.depth_limit_stats["failed"] += 1
                    f.cache["limit_ok"] = False
                    self.limits_failed(f.cache)
                    del binning
                    continue
                self.limits_held(f.cache)
            if f.use_order:
                f.cache["order_ok"] = True
            if f.use_limit:
                f.cache["limit_ok"] = True
            return num_rendered, binning

    def _lists_lsd(self, f, limit):
        """Lists by depth sort + emission + partition by tile (GsView.tile_cull = 0 / 1, csrc/gs_binning.hip): the geometry
        phase counts the instances, the binning buffer is sized by that count.  -> (num_rendered, binning buffer, scratch)"""
        self.api.call("forward_geometry", C.byref(f.view), C.byref(f.g), C.byref(self._scratch_of(f, None, 0, limit)),
                      f.radii.data_ptr(), f.status.data_ptr(), f.stream)
        if f.static:
            cap = int(self.static_capacity)
            binning = self._new_binning(f, cap)
            s = self._scratch_of(f, binning, cap, limit)
            self._render(f, s)
            return cap, binning, s
        cap = self._capacity_hint if self.optimistic else 0
        if cap > 0 and limit is not None and self._capacity_hint_limited > 0:
            cap = self._capacity_hint_limited
        binning = None
        if cap > 0:
            # Optimistic path: the reference blocks the host on a D2H copy of num_rendered before it can
            # size the binning buffer (rasterizer_impl.cu:284-288) and the GPU idles meanwhile.  Here the
            # binning/blend phase is enqueued at once with a capacity predicted from the previous calls
            # (the kernels read num_rendered on the device); the host then waits only for the geometry
            # phase - the GPU is already sorting and blending - and re-runs the phase in the rare case
            # the prediction was too small.
            ev = torch.cuda.Event()
            ev.record(f.cur)
            binning = self._new_binning(f, cap)
            s = self._scratch_of(f, binning, cap, limit)
            self._render(f, s)
            ev.synchronize()
        else:
            f.cur.synchronize()  # the reference's blocking D2H (rasterizer_impl.cu:284)
        num_rendered = int(f.status[0])
        self._update_hint(num_rendered, limited=limit is not None)
        if binning is None or num_rendered > cap:
            binning = self._new_binning(f, num_rendered)
            s = self._scratch_of(f, binning, num_rendered, limit)
            self._render(f, s)
        return num_rendered, binning, s

    def _lists_region(self, f, limit, block):
        """Lists by region binning (GsView.tile_cull = 2, csrc/gs_regionbin.hip).  The region buckets live in the binning
        buffer, so it is allocated BEFORE the geometry phase, from the capacity the previous views needed; the instance count
        is known once the lists are built (gs_forward_bin copies the status words out), which is what the host waits for -
        the blend is already running then.  Too small a capacity (or a bucket that overflowed) sets the overflow flag:
        nothing valid was produced and the view is rendered again with what the status asks for.  With a status `block` the
        host waits for nothing: whoever reads the block checks capacity and limits alike.
        -> (num_rendered, binning buffer, scratch); the buffer is None when a region holds more Gaussians than one workgroup
        can sort."""
        regions = _regions(f.W, f.H)
        limited = limit is not None
        if f.static:
            cap = int(self.static_capacity)
        else:
            hint = self._capacity_hint_limited if (limited and self._capacity_hint_limited > 0) else self._capacity_hint
            cap = hint if hint > 0 else max(8 * f.P, 1 << 20)
        early, f.early = f.early, None
        if early is not None and (block is None or not limited or f.static):   # (not the forward it was taken for)
            self._retire_early(early)
            early = None
        for attempt in range(6):
            if early is not None:
                cap, binning = early.cap, early.binning
            else:
                cap = max(cap, regions)
                binning = self._new_binning(f, cap)
            s = self._scratch_of(f, binning, cap, limit)
            if early is not None:   # (the late launch: gs_forward_geometry waits for the event and serves the blocks left out)
                s.early_geometry_done = early.event.cuda_event
                self._early_done = early.event   # (kept alive until the next one replaces it)
                self.early_geometry_stats["used"] += 1
                early = None
            if self._last is not None and self._last.geom is f.geom:
                self._last.binning, self._last.cap = binning, cap
            self.api.call("forward_geometry", C.byref(f.view), C.byref(f.g), C.byref(s), f.radii.data_ptr(), None, f.stream)
            if block is not None:
                self.api.call("forward_bin", C.byref(f.view), C.byref(f.g), C.byref(s), None, f.stream)
                if self.STATUS_IN_RENDER:   # the forward's last kernel writes the status words into the pinned block
                    s.status_host = block.data_ptr()
                    # Train step (a fused step is armed): that kernel (tile_order: the backward's launch order, the camera's
                    # next hints and depth bounds, the status block) is issued on the SIDE stream - nothing before the
                    # backward blend needs it, so it runs beside the criterion's first kernel instead of in front of it; the
                    # backward waits for it.  Not in the capture-safe mode: inside a captured graph the extra cross-stream
                    # edge costs more than the kernel it takes off the chain (C3 replay 0.96 -> 1.00 ms; the eager step
                    # gains 6-10 us).
                    if self.fused_step is not None and not f.static:
                        s.defer_tile_order = 1
                self._render(f, s)
                return cap, binning, s
            self.api.call("forward_bin", C.byref(f.view), C.byref(f.g), C.byref(s), f.status.data_ptr(), f.stream)
            ev = torch.cuda.Event()
            ev.record(f.cur)
            self._render(f, s)
            ev.synchronize()  # the lists are built (the blend is running): did they fit?
            st = tuple(int(x) for x in f.status[:4])
            if st[1] == 0:
                break
            if st[3] > self.REGION_MAX_ENTRIES:
                self._region_off.add((f.P, f.W, f.H, limited))
                return 0, None, None
            cap = int(max(st[0], st[3] * regions) * 1.25) + 4096
            del binning
        else:
            raise RuntimeError("region binning: the capacity did not settle (status %r)" % (st,))
        self._update_hint(max(st[0], st[3] * regions), limited=limited)
        return st[0], binning, s

    def _status_block(self, device):
        """A pinned status block for a verdict collected later, from a small ring per device: a block is re-used only after
        eight further deferred forwards."""
        ring = self._status_ring.setdefault(device.index, [[], 0])
        if len(ring[0]) < 8:
            ring[0].append(torch.zeros((16,), dtype=torch.int32).pin_memory())
        block = ring[0][ring[1] % len(ring[0])]
        ring[1] += 1
        return block

    def _new_binning(self, f, cap):
        _, _, bb, _ = self.scratch_bytes(f.P, f.W, f.H, cap)
        binning = torch.empty((bb,), dtype=torch.uint8, device=f.device)
        if self.scratch_fill is not None:
            self.scratch_fill("binning", binning)
        self._remember_capacity(binning, cap)
        return binning

    def _scratch_of(self, f, binning, capacity, limit):
        s = self._scratch(f.geom, f.img, binning, capacity)
        if limit is not None:
            s.tile_depth_limit = limit.data_ptr()
        if f.static and self.static_step_tag is not None:
            s.step_tag = self.static_step_tag.data_ptr()
        return s

    def _render(self, f, scratch):
        c = f.cache
        if f.use_order:
            if c["order_ok"]:
                scratch.tile_order_hint = c["order"].data_ptr()
            # what this view measures becomes the hint of this camera's next visit: written by the forward's last launch
            # straight into the camera's buffers (they are read - as this view's hints - before they are written)
            scratch.tile_order_out = c["order"].data_ptr()
        if f.use_limit:
            scratch.tile_depth_limit_out = c["limit"].data_ptr()
            scratch.tile_depth_limit_slack = c["slack"].data_ptr()
        if f.fsgs == _DEPTH_ONLY:
            self.api.call("depth_forward", C.byref(f.view), C.byref(f.g), C.byref(scratch), f.out_invdepth.data_ptr(),
                          f.out_extra.data_ptr(), f.stream)
        elif f.fsgs:
            self.api.call("forward_render_fsgs", C.byref(f.view), C.byref(f.g), C.byref(scratch), f.out_color.data_ptr(),
                          f.out_invdepth.data_ptr(), f.out_extra.data_ptr(), f.stream)
        elif f.extra is None:
            self.api.call("forward_render", C.byref(f.view), C.byref(f.g), C.byref(scratch), f.out_color.data_ptr(),
                          f.out_invdepth.data_ptr(), f.stream)
        else:
            self.api.call("forward_render_x", C.byref(f.view), C.byref(f.g), C.byref(scratch), f.out_color.data_ptr(),
                          f.out_invdepth.data_ptr(), f.out_extra.data_ptr(), f.stream)

    def _tile_order_on_side(self, view, scratch, main):
        """gs_forward_tile_order on the side stream, ordered behind the render just issued on `main`; the event it returns (also
        kept in _tile_order_done) is what the backward - and any later forward - waits for."""
        side = self._side_stream(main.device)
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        # (no `with torch.cuda.stream(side)`: the call takes the stream, the event records on it - the context switch alone
        #  is ~20 us of host time per step)
        self.api.call("forward_tile_order", C.byref(view), C.byref(scratch), C.c_void_p(side.cuda_stream))
        done = torch.cuda.Event()
        done.record(side)
        self._tile_order_done = done
        return done

    def _join_tile_order(self, device):
        """Order the current stream behind a tile_order still pending on the side stream (no-op otherwise)."""
        done, self._tile_order_done = getattr(self, "_tile_order_done", None), None
        if done is not None:
            torch.cuda.current_stream(device).wait_event(done)

    # ------------------------------------------------------------------ the depth-only pass
    def depth_forward(self, means3D, opacities, scales, rotations, cov3D_precomp, scale_modifier, bg, viewmatrix, projmatrix,
                      campos, tanfovx, tanfovy, image_height, image_width, debug=False):
        """gs_depth_forward behind the forward sequence of rasterize_gaussians(fsgs=True): geometry, its one read-back of
        num_rendered, the binning allocation, the backend's kind of lists (tile_cull / binning).  No colour image.
        -> (depth [1,H,W], alpha [1,H,W], radii [P] int32, record for depth_backward or None when P == 0)

        The pass owns its scratch: it neither reads nor writes the last-forward record, the per-camera hints and depth
        limits, the one-shot requests (grad_arena, fused_step, raw_activations, ...) of the general path.  It shares the
        binning capacity hint, which only sizes buffers."""
        if means3D.ndim != 2 or means3D.shape[1] != 3:
            raise RuntimeError("means3D must have dimensions (num_points, 3)")
        self._check_device(means3D)
        device = means3D.device
        P, H, W = int(means3D.shape[0]), int(image_height), int(image_width)
        f32 = dict(dtype=torch.float32, device=device)
        alloc = torch.empty if P != 0 else torch.zeros
        depth, alpha = alloc((1, H, W), **f32), alloc((1, H, W), **f32)
        radii = alloc((P,), dtype=torch.int32, device=device)
        if P == 0:
            return depth, alpha, radii, None
        tile_cull = self._tile_cull(device)
        if tile_cull == 2 and ((P, W, H, False) in self._region_off or (
                self.binning == "auto" and self._capacity_hint > self.REGION_AUTO_MAX * _regions(W, H))):
            tile_cull = 1
        keep = []
        view = self._view(keep, device, bg, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, scale_modifier, 0, False,
                          False, debug, tile_cull=tile_cull)
        # the geometry phase wants a colour source; this pass never reads the colours it leaves in the records, so any
        # [P,3] array serves: the means themselves (no tensor of ones is built)
        g = self._gauss(keep, device, means3D, None, means3D, opacities, scales, rotations, cov3D_precomp)
        gb, ib, _, _ = self.scratch_bytes(P, W, H, 0)
        u8 = dict(dtype=torch.uint8, device=device)
        geom, img = torch.empty((gb,), **u8), torch.empty((ib,), **u8)
        if self.scratch_fill is not None:
            self.scratch_fill("geom", geom)
            self.scratch_fill("img", img)
        f = _Forward(device, self._stream(device), view, g, P, W, H, geom, img, radii, None, depth, alpha, _DEPTH_ONLY, None,
                     None, False, False, False)
        f.cur = torch.cuda.current_stream(device)
        pkey = (device.index, f.cur.cuda_stream)
        status = self._pinned_by_device.get(pkey)
        if status is None:
            status = self._pinned_by_device[pkey] = torch.zeros((16,), dtype=torch.int32).pin_memory()
        f.status = status
        num_rendered, binning = self._forward_lists(f, None, False)
        return depth, alpha, radii, dict(view=f.view, g=g, keep=keep, radii=radii, geom=geom, img=img, binning=binning,
                                         R=int(num_rendered), P=P, W=W, H=H)

    def depth_backward(self, rec, dL_ddepth, dL_dalpha, grad_flags, workspace=None):
        """gs_depth_backward on the record of a depth_forward.  grad_flags: 1 means, 2 opacities, 3 both; a cotangent may be
        None (zero).  -> (dL_dmeans3D [P,3], dL_dmeans2D [P,3], dL_dopacity [P,1]), None for what was not asked for.
        workspace: the caller's uint8 buffer (>= P * 128 rounded up to 256) - it keeps the float64 blend sums afterwards."""
        device = rec["radii"].device
        P, W, H, R = rec["P"], rec["W"], rec["H"], rec["R"]
        f32 = dict(dtype=torch.float32, device=device)
        dL_ddepth, dL_dalpha = _prep(dL_ddepth, device), _prep(dL_dalpha, device)
        # every row of a requested output is written by the per-Gaussian kernel (zeros for culled rows): empty, not zeros
        dm3 = torch.empty((P, 3), **f32) if grad_flags & 1 else None
        dm2 = torch.empty((P, 3), **f32) if grad_flags & 1 else None
        dop = torch.empty((P, 1), **f32) if grad_flags & 2 else None
        ws = workspace
        if ws is None:
            ws = torch.empty((((P * 128 + 255) // 256) * 256,), dtype=torch.uint8, device=device)
        binning = rec["binning"]
        s = self._scratch(rec["geom"], rec["img"], binning, self._capacity_for(binning, P, W, H, R))
        self.api.call("depth_backward", C.byref(rec["view"]), C.byref(rec["g"]), rec["radii"].data_ptr(), C.byref(s), R,
                      _ptr(dL_ddepth), _ptr(dL_dalpha), int(grad_flags), _ptr(dm3), _ptr(dm2), _ptr(dop), ws.data_ptr(),
                      ws.numel(), self._stream(device))
        return dm3, dm2, dop

    def depth_backward_step(self, rec, dL_ddepth, dL_dalpha, which, param, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999),
                            eps=1e-15, flags=0, workspace=None):
        """gs_depth_backward_step on the record of a depth_forward: the blend backward, then ONE per-Gaussian launch that
        steps `param` (which 1: the means [P,3]; 2: the RAW opacities [P,1], the forward's `opacities` being their sigmoid)
        and both moments in place with Adam at (lr, step).  No gradient tensor is made.
        flags / workspace: capi.DEPTH_STEP_ROWS_GIVEN with the workspace a depth_backward call left."""
        device = rec["radii"].device
        P, W, H, R = rec["P"], rec["W"], rec["H"], rec["R"]
        if not hasattr(self.api, "_depth_backward_step"):
            raise RuntimeError("the loaded library has no gs_depth_backward_step - there is no fallback")
        for name, t in (("param", param), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != P * (3 if which == 1 else 1):
                raise RuntimeError("depth_backward_step: %s must be a contiguous fp32 tensor of %d rows on %s" % (name, P, device))
        dL_ddepth, dL_dalpha = _prep(dL_ddepth, device), _prep(dL_dalpha, device)
        ws = workspace
        if ws is None:
            ws = torch.empty((((P * 128 + 255) // 256) * 256,), dtype=torch.uint8, device=device)
        binning = rec["binning"]
        s = self._scratch(rec["geom"], rec["img"], binning, self._capacity_for(binning, P, W, H, R))
        self.api.call("depth_backward_step", C.byref(rec["view"]), C.byref(rec["g"]), rec["radii"].data_ptr(), C.byref(s), R,
                      _ptr(dL_ddepth), _ptr(dL_dalpha), int(which), param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                      float(lr), int(step), float(betas[0]), float(betas[1]), float(eps), int(flags), ws.data_ptr(), ws.numel(),
                      self._stream(device))

    # ------------------------------------------------------------------ backward
    def rasterize_gaussians_backward(self, bg, means3D, radii, colors_precomp, opacities, scales, rotations,
                                     scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy,
                                     dL_dout_color, dL_dout_invdepth, sh, degree, campos, geomBuffer, R,
                                     binningBuffer, imgBuffer, antialiasing, debug, extra=None, dL_dout_extra=None,
                                     fsgs=False, extra_gain=None, raw=False):
        """= RasterizeGaussiansBackwardCUDA (rasterize_points.cu:126-223).

        Returns (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
        dL_drotations) (+ dL_dextra [P] when the forward blended a 4th channel).
        fsgs=True: dL_dout_invdepth is the depth image gradient and dL_dout_extra the alpha image gradient; with an armed
        fused_step the call is gs_backward_step_fsgs (one launch for every Gaussian, no side launch) and returns eight Nones.
        raw=True: the forward read raw rows (GsGaussians.raw_activations) - said by a caller whose forward may not be the last
        one; the last forward's own record says it for its backward."""
        self._check_device(means3D)
        device = means3D.device
        P = int(means3D.shape[0])
        H, W = int(dL_dout_color.shape[1]), int(dL_dout_color.shape[2])
        if device.type == "cuda":
            self._join_tile_order(device)   # (the blend backward reads the launch order that kernel writes)
        arena, self.grad_arena = self.grad_arena, None
        step, self.fused_step = self.fused_step, None
        self.early_request = None   # (a request the side launch did not take: nothing will)
        sh_rest, self.sh_rest = self.sh_rest, None
        sh_activated, self.sh_rest_activated = self.sh_rest_activated, False
        f = self._last if self._last is not None and self._last.geom is geomBuffer else None
        if f is not None:
            raw = f.raw
        # split rows: gs_backward_split on activated values (gsplat_amd.accel's `dc=` call), else the fused step's gradients-out form
        split = sh_rest is not None and sh_activated and step is None and not raw and not fsgs and extra is None
        if sh_rest is not None and not split and (step is None or not raw or not step.grad_out_rest):
            raise RuntimeError("split SH rows: the backward is gs_backward_split (activated values, no 4th channel) or "
                               "gs_backward_step's gradients-out form with grad_out_rest")
        if raw and (step is None or P == 0):
            raise RuntimeError("a forward on raw activations must be followed by the fused train-step backward")
        fused = step is not None and P != 0
        if fused and fsgs and not hasattr(self.api, "_backward_step_fsgs"):
            raise RuntimeError("this library has no fused train-step backward for the FSGS rasterizer generation")
        dL_dout_color, dL_dout_invdepth = _prep(dL_dout_color, device), _prep(dL_dout_invdepth, device)
        # dL_dout_extra from here on: the 4th channel's image gradient (zeros when not given); with fsgs the alpha image's;
        # else None
        if extra is not None:
            dL_dout_extra = _prep(dL_dout_extra, device)
            if dL_dout_extra is None:
                dL_dout_extra = torch.zeros((1, H, W), dtype=torch.float32, device=device)
        elif not fsgs:
            dL_dout_extra = None
        if fused and f is not None:
            view, g = f.view, f.g   # (the forward's own structs: its prefiltered flag and its kind of lists)
        else:   # (`keep` holds what they point into until the backward has been issued)
            view, g, keep = self._structs(device, bg, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                          viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, scale_modifier, degree,
                                          antialiasing, debug, extra, raw=raw, extra_gain=extra_gain if raw else None,
                                          sh_rest=sh_rest)
        args = (view, g, radii.contiguous(), geomBuffer, binningBuffer, imgBuffer, P, W, H, R, dL_dout_color, dL_dout_invdepth,
                dL_dout_extra)
        if fused:
            return self._backward_step(step, f, *args, fsgs=fsgs)
        return self._backward_grads(arena, fsgs, *args)

    def _zero_image(self, device, H, W):
        """One [1,H,W] image of zeros per device and size, never written: the cotangent of an output nobody differentiated."""
        key = (device.index, H, W)
        z = self._zero_images.get(key)
        if z is None:
            if len(self._zero_images) > 8:
                self._zero_images.clear()
            z = self._zero_images[key] = torch.zeros((1, H, W), dtype=torch.float32, device=device)
        return z

    def _backward_step_fsgs(self, step, view, g, radii, geom, binning, img, P, W, H, R, dL_dout_color, dL_ddepth, dL_dalpha):
        """gs_backward_step_fsgs: the fused train-step backward behind gs_forward_render_fsgs.  One launch steps every
        Gaussian: the side launch of the two-phase step is closed to this generation."""
        device = radii.device
        if step.phase != 0 or step.phase1_done:
            raise RuntimeError("the two-phase step (side launch of gs_step_uninstanced) is closed to the FSGS rasterizer "
                               "generation")
        if step.extra:
            raise RuntimeError("the FSGS rasterizer generation has no 4th channel to step")
        _, _, _, wsb = self.scratch_bytes(P, W, H, R)
        ws = self._rows_workspace(step, device, wsb)
        s = self._scratch(geom, img, binning, self._capacity_for(binning, P, W, H, R))
        last = self._last
        if last is not None:
            last.step = last.radii = last.img = last.done = None
        step.reached_split = int(self.REACHED_SPLIT)
        dL_ddepth, dL_dalpha = _prep(dL_ddepth, device), _prep(dL_dalpha, device)
        zeros = self._zero_image(device, H, W) if dL_ddepth is None or dL_dalpha is None else None
        try:
            self.api.call("backward_step_fsgs", C.byref(view), C.byref(g), radii.data_ptr(), C.byref(s), int(R),
                          dL_dout_color.data_ptr(), (dL_ddepth if dL_ddepth is not None else zeros).data_ptr(),
                          (dL_dalpha if dL_dalpha is not None else zeros).data_ptr(), C.byref(step), _ptr(ws), ws.numel(),
                          self._stream(device))
        except Exception:
            self.rows_epoch += 1
            raise
        if step.rows_clean:
            self._rows_ws[(device.index, wsb)][1] = True
        return (None,) * 8

    def _backward_step(self, step, f, view, g, radii, geom, binning, img, P, W, H, R, dL_dout_color, dL_dout_invdepth,
                       dL_dout_extra, fsgs=False):
        """gs_backward_step[_x] for the train step armed as `step` (backward, activation backward, view statistics and Adam
        in one per-Gaussian kernel - or its gradients-out form); `f`: the forward's record when it is the last one.
        Returns no gradients at all."""
        if fsgs:
            return self._backward_step_fsgs(step, view, g, radii, geom, binning, img, P, W, H, R, dL_dout_color,
                                            dL_dout_invdepth, dL_dout_extra)
        device = radii.device
        _, _, _, wsb = self.scratch_bytes(P, W, H, R)
        ws = self._rows_workspace(step, device, wsb)
        s = self._scratch(geom, img, binning, self._capacity_for(binning, P, W, H, R))
        done, last = None, self._last
        if last is not None:   # (a fused backward ends the last forward's arming, whichever forward it belongs to)
            if last is f and last.step is step:
                done = last.done          # (issued by launch_uninstanced_early, under the criterion's backward)
            last.step = last.radii = last.img = last.done = None
        if done is None:
            step.reached_split = int(self.REACHED_SPLIT)
        if self._two_phase(step, P):
            if done is None:
                done = self._launch_uninstanced(device, view, g, radii, s, step)
            self._uninst_done = done          # (kept alive until the next step replaces it)
            step.phase = 2                    # gs_backward_step: the Gaussians with instances only ...
            step.phase1_done = done.cuda_event  # ... its per-Gaussian kernel behind the side launch
        try:
            if dL_dout_extra is not None:
                self.api.call("backward_step_x", C.byref(view), C.byref(g), radii.data_ptr(), C.byref(s), int(R),
                              dL_dout_color.data_ptr(), _ptr(dL_dout_invdepth), dL_dout_extra.data_ptr(), C.byref(step),
                              _ptr(ws), ws.numel(), self._stream(device))
            else:
                self.api.call("backward_step", C.byref(view), C.byref(g), radii.data_ptr(), C.byref(s), int(R),
                              dL_dout_color.data_ptr(), _ptr(dL_dout_invdepth), C.byref(step), _ptr(ws), ws.numel(),
                              self._stream(device))
        except Exception:
            self.rows_epoch += 1   # (the persistent rows may hold sums now: graphs that skip the clear are stale)
            raise
        if step.rows_clean:
            self._rows_ws[(device.index, wsb)][1] = True
        return (None,) * (8 if dL_dout_extra is None else 9)

    def _rows_workspace(self, step, device, wsb):
        """The gradient-row workspace of a fused backward; sets step.rows_clean.  keep_workspace and rows_override: a fresh
        one (rows_clean = 0).  Otherwise one persistent workspace per size: the chain kernel zeroes every row it consumes
        (GsStepState.rows_clean), so the rows are clean again after every step and no clear launch runs.  rows_clean = 1 -
        one clear launch, then clean again - whenever the host is not SURE of that state (first use, a call that raised);
        the caller marks them clean once the call has returned."""
        if self.keep_workspace or step.rows_override:
            step.rows_clean = 0
            return self._fresh_workspace(device, wsb)
        key = (device.index, wsb)
        ent = self._rows_ws.get(key)
        if ent is None:
            if len(self._rows_ws) >= 4:   # (sizes of a model that has since been densified: nothing replays them,
                self._rows_ws.clear()    #  a captured graph is keyed by the number of Gaussians)
            ent = self._rows_ws[key] = [torch.zeros((wsb,), dtype=torch.uint8, device=device), True]
        # (a launch captured into a hipGraph is replayed with this flag frozen: `rows_epoch` counts the calls that may
        #  have left rows dirty, GraphedStep keys its graphs by it and captures again - after an eager step that cleaned)
        step.rows_clean = 2 if ent[1] else 1
        if not ent[1]:
            self.rows_epoch += 1
        ent[1] = False      # (until the call has returned: a failed launch leaves them in an unknown state)
        return ent[0]

    def _fresh_workspace(self, device, wsb):
        # (the backward clears only the rows of Gaussians that emitted instances; a probe that keeps the workspace gets
        #  zeros for the others too)
        ws = (torch.zeros if self.keep_workspace else torch.empty)((wsb,), dtype=torch.uint8, device=device)
        if self.keep_workspace:
            self.last_workspace = ws
        return ws

    def _backward_grads(self, arena, fsgs, view, g, radii, geom, binning, img, P, W, H, R, dL_dout_color, dL_dout_invdepth,
                        dL_dout_extra):
        """gs_backward / _x / _fsgs: the gradients, written into the grad arena's tensors where they fit.
        Split SH rows (g.shs_rest): gs_backward_split - slot 5 of the tuple is the DC rows' gradient [P,1,3] and the tuple ends
        with the rest rows' [P,M-1,3]; both are written in full by the kernel."""
        device = radii.device
        f32 = dict(dtype=torch.float32, device=device)
        # every row is written by gs_backward (culled rows become 0): empty, not zeros
        alloc = torch.empty if P != 0 else torch.zeros

        def out(name, shape):
            t = None if arena is None else arena.get(name)
            if t is not None and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == device \
                    and t.dtype == torch.float32:
                return t
            return alloc(shape, **f32)
        # gradients of inputs that were not given ("absent" colours / covariances) are not produced: the reference
        # returns zero tensors for them (rasterize_points.cu:163-178) which autograd then drops
        dL_dmeans3D = out("means3D", (P, 3))
        ret = (alloc((P, 3), **f32), alloc((P, NUM_CHANNELS), **f32) if g.colors_precomp else None, alloc((P, 1), **f32),
               dL_dmeans3D, alloc((P, 6), **f32) if g.cov3D_precomp else None,
               alloc((P, 1, 3), **f32) if g.shs_rest else out("sh", (P, g.M, 3)), alloc((P, 3), **f32), alloc((P, 4), **f32))
        dsh_rest = alloc((P, g.M - 1, 3), **f32) if g.shs_rest else None
        x = dL_dout_extra is not None and not fsgs   # (a 4th channel)
        if x:
            ret = ret + (alloc((P,), **f32),)
        if P == 0:
            return ret if dsh_rest is None else ret + (dsh_rest,)
        _, _, _, wsb = self.scratch_bytes(P, W, H, R)
        ws = self._fresh_workspace(device, wsb)
        s = self._scratch(geom, img, binning, self._capacity_for(binning, P, W, H, R))
        grads = self._grads(ret)
        if g.scales is None:
            ret[6].zero_()
            ret[7].zero_()
        stream = self._stream(device)
        if dsh_rest is not None:
            self.api.call("backward_split", C.byref(view), C.byref(g), radii.data_ptr(), C.byref(s), int(R),
                          dL_dout_color.data_ptr(), _ptr(dL_dout_invdepth), C.byref(grads), dsh_rest.data_ptr(), _ptr(ws),
                          ws.numel(), stream)
            return ret + (dsh_rest,)
        if fsgs:
            zeros = None
            if dL_dout_invdepth is None or _prep(dL_dout_extra, device) is None:
                zeros = torch.zeros((1, H, W), **f32)
            gd = dL_dout_invdepth if dL_dout_invdepth is not None else zeros
            ga = _prep(dL_dout_extra, device)
            ga = ga if ga is not None else zeros
            self.api.call("backward_fsgs", C.byref(view), C.byref(g), radii.data_ptr(), C.byref(s), int(R),
                          dL_dout_color.data_ptr(), gd.data_ptr(), ga.data_ptr(), C.byref(grads), _ptr(ws), ws.numel(),
                          stream)
        elif not x:
            self.api.call("backward", C.byref(view), C.byref(g), radii.data_ptr(), C.byref(s), int(R),
                          dL_dout_color.data_ptr(), _ptr(dL_dout_invdepth), C.byref(grads), _ptr(ws), ws.numel(), stream)
        else:
            self.api.call("backward_x", C.byref(view), C.byref(g), radii.data_ptr(), C.byref(s), int(R),
                          dL_dout_color.data_ptr(), _ptr(dL_dout_invdepth), dL_dout_extra.data_ptr(), C.byref(grads),
                          _ptr(ws), ws.numel(), stream)
        return ret

    _GRAD_FIELDS = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
                    "dL_drotations", "dL_dextra")

    @classmethod
    def _grads(cls, ret):
        """GsGrads over a backward's return tuple (None: a gradient that is not produced)."""
        grads = GsGrads()
        for name, t in zip(cls._GRAD_FIELDS, ret):
            setattr(grads, name, _ptr(t))
        return grads

    def backward_from_rows(self, rows, bg, means3D, radii, colors_precomp, opacities, scales, rotations, scale_modifier,
                           cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, H, W, sh, degree, campos, geomBuffer,
                           antialiasing, depth_mode=0):
        """Stage 2 of the backward alone (gs_backward_from_rows): the per-Gaussian chain rule applied to GIVEN sums of the
        blend backward, rows [P,16] float64.  Same return tuple as rasterize_gaussians_backward.  Parity tests only."""
        self._check_device(means3D)
        device = means3D.device
        P = int(means3D.shape[0])
        f32 = dict(dtype=torch.float32, device=device)
        view, g, keep = self._structs(device, bg, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                      viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, scale_modifier, degree,
                                      antialiasing, False)
        ret = (torch.empty((P, 3), **f32), torch.empty((P, 3), **f32) if g.colors_precomp else None,
               torch.empty((P, 1), **f32), torch.empty((P, 3), **f32), torch.empty((P, 6), **f32) if g.cov3D_precomp else None,
               torch.empty((P, g.M, 3), **f32) if g.M else None, torch.zeros((P, 3), **f32), torch.zeros((P, 4), **f32))
        rows = rows.to(device=device, dtype=torch.float64).contiguous()
        assert rows.shape == (P, 16)
        _, _, _, wsb = self.scratch_bytes(P, W, H, 0)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=device)
        self.api.call("backward_from_rows", C.byref(view), C.byref(g), radii.contiguous().data_ptr(), C.byref(self._scratch(geomBuffer)),
                      rows.data_ptr(), int(depth_mode), C.byref(self._grads(ret)), ws.data_ptr(), ws.numel(), self._stream(device))
        return ret

    # ------------------------------------------------------------------ markVisible
    def export_row_mask(self, out):
        """out [P] uint8 <- 1 where the Gaussian emitted instances in the LAST forward (gs_export_row_mask: what the
        data-parallel backward later writes into GsStepState.grad_mask).  False when there is no such forward to ask."""
        f = self._last
        if f is None or f.geom.device != out.device or f.P != out.numel() or not hasattr(self.api, "_export_row_mask"):
            return False
        self.api.call("export_row_mask", C.byref(self._scratch(f.geom)), f.P, out.data_ptr(), self._stream(f.geom.device))
        return True

    def mark_visible(self, means3D, viewmatrix, projmatrix):
        """= markVisible (rasterize_points.cu:225-244)."""
        self._check_device(means3D)
        device = means3D.device
        P = int(means3D.shape[0])
        present = torch.zeros((P,), dtype=torch.bool, device=device)
        if P != 0:
            m, vm, pm = (_prep(x, device) for x in (means3D, viewmatrix, projmatrix))
            self.api.call("mark_visible", P, m.data_ptr(), vm.data_ptr(), pm.data_ptr(), present.data_ptr(),
                          self._stream(device))
        return present

    # ------------------------------------------------------------------ parity exports
    def export_reached(self, P, geom):
        """[P] uint8 copy of the flags the last forward blend on `geom` left (GeomView.reached: the last P bytes' 256-B block of
        the geometry buffer): 1 = the backward blend visits a list entry of this Gaussian.  Device library only."""
        gb = self.scratch_bytes(P, 16, 16, 0)[0]
        off = gb - ((P + 255) // 256) * 256
        if geom.device.type == "cuda":
            torch.cuda.current_stream(geom.device).synchronize()
        return geom[off:off + P].clone()

    def export_state(self, P, W, H, R, geom, binning, img):
        """Plain-array copies of the forward's internal state (tests / debugging only)."""
        device = geom.device
        cap = self._capacity_for(binning, P, W, H, R)
        s = self._scratch(geom, img, binning, cap)
        f32 = dict(dtype=torch.float32, device=device)
        T = ((W + 15) // 16) * ((H + 15) // 16)
        out = dict(
            depths=torch.zeros((P,), **f32), means2D=torch.zeros((P, 2), **f32), cov3D=torch.zeros((P, 6), **f32),
            conic_opacity=torch.zeros((P, 4), **f32), rgb=torch.zeros((P, 3), **f32),
            clamped=torch.zeros((P, 3), dtype=torch.uint8, device=device),
            tiles_touched=torch.zeros((P,), dtype=torch.int32, device=device),
            point_offsets=torch.zeros((P,), dtype=torch.int32, device=device),
            keys_sorted=torch.zeros((R,), dtype=torch.int64, device=device),
            point_list=torch.zeros((R,), dtype=torch.int32, device=device),
            final_T=torch.zeros((H, W), **f32), n_contrib=torch.zeros((H, W), dtype=torch.int32, device=device),
            ranges=torch.zeros((T, 2), dtype=torch.int32, device=device))
        st = self._stream(device)
        o = out
        self.api.call("export_geom", C.byref(s), P, _ptr(o["depths"]), _ptr(o["means2D"]), _ptr(o["cov3D"]),
                      _ptr(o["conic_opacity"]), _ptr(o["rgb"]), _ptr(o["clamped"]), _ptr(o["tiles_touched"]),
                      _ptr(o["point_offsets"]), st)
        from .capi import GsError
        try:
            self.api.call("export_binning", C.byref(s), R, _ptr(o["keys_sorted"]), _ptr(o["point_list"]), st)
        except GsError as e:
            if e.code != -5:
                raise
            # lists built by region binning: keys rebuilt from ranges[] (tile lists lie in point_list in no particular order)
            self.api.call("export_binning_region", C.byref(s), W, H, R, _ptr(o["keys_sorted"]), _ptr(o["point_list"]), st)
        self.api.call("export_img", C.byref(s), W, H, _ptr(o["final_T"]), _ptr(o["n_contrib"]), _ptr(o["ranges"]), st)
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()
        return out
