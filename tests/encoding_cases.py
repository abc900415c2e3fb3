"""Constructed cases and bars for DNGaussian's grid and SH encoders (csrc/gs_encoding.hip), pure torch / numpy.
What each case is for is proved in tests/test_encoding_cases_cpu.py; tests/test_gpu_encoding_forms.py runs them on the GPU.

layout() restates the embedding backward's emit + stable sort (entry e = ((b * L + l) << D) + corner, key = global slot,
outside points keyed n_slots) and segment_classes() names the paths grid_slot_kernel takes through a sorted segment.

EXACT cases: D = 2, L = 1, H = 5 (scale 4, a power of two), points at fraction (0.25, 0.5) of chosen cells, integer embeddings
and output gradients.  Every corner weight is a multiple of 1/8, every partial sum an exact multiple of 1/8 far below 2^24, so
outputs, embedding gradient and input gradient are the float64 oracle's bits in ANY summation order.

FORM cases carry derived bars, u = 2^-24, k_w = 2 D (linear) or 6 D (smoothstep) roundings in a corner weight:
  output element     |h - o| <= 2 (k_w + 2^D + 1) u A,    A   = sum_k w_k |emb_k|    (the oracle on |embeddings|)
  embedding slot s   |h - o| <= 2 (k_w + n_s + 1) u A_s,  A_s = sum w |g|            (the oracle's gradient under |g_out|)
the any-order fp32 summation bound over the 2^D / n_s terms (n_s from layout()); a slot with n_s = 0 must be exactly 0.
The input gradient has a tensor-level bar measured on the restatement, never on the kernel: 8 x max|r32 - r64| of
encoding_reference.grid_encode_ref in fp32 against float64, floored at one fp32 ulp of the largest entry (the margin 8: the
restatement's fp32 order is one order among many).  SH bars are the same measure per output column / input component."""
import functools
from collections import namedtuple

import numpy as np
import torch

import encoding_reference as ref

U = 2.0 ** -24
CHUNK = 256
CLASSES = ("inside", "straddle", "one_chunk", "head_chunks", "chunks_tail", "head_chunks_tail", "multi_chunk")

Layout = namedtuple("Layout", "slot lo hi N keys order")


def points(B, D, seed, edges=True, outside=True):
    """tests/test_gpu_encoding.py's points(): uniform in [0,1]^D with exact 0 / 1 coordinates and points outside the cube."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, D), generator=g)
    if edges and B >= 8:
        x[0::7, 0] = 0.0
        x[1::7, D - 1] = 1.0
        x[2] = 1.0
        x[3] = 0.0
    if outside and B >= 8:
        x[4::11, 0] = 1.0 + torch.rand((len(range(4, B, 11)),), generator=g) * 0.1
        x[5::13, D - 1] = -torch.rand((len(range(5, B, 13)),), generator=g) * 0.1
    return x


def entries(x, offsets, per_level_scale, H, gridtype, align_corners, interpolation=0):
    """Every (point, level, corner): its global slot (int64 [B, L, 2^D], n_slots for a point outside [0,1]^D) and its weight
    (float64 from the fp32 fraction, 0 outside), entry e = ((b * L + l) << D) + corner when flattened."""
    x32 = x.detach().float()
    B, D = x32.shape
    L, K, n_slots = len(offsets) - 1, 1 << D, int(offsets[-1])
    oob = ((x32 < 0) | (x32 > 1)).any(dim=1)
    xs = torch.where(oob[:, None], torch.zeros_like(x32), x32)
    keys = torch.full((B, L, K), n_slots, dtype=torch.int64)
    w = torch.zeros((B, L, K), dtype=torch.float64)
    for l, (sc, res) in enumerate(ref.level_geometry(L, per_level_scale, H)):
        pos = xs * torch.tensor(sc, dtype=torch.float32) + torch.tensor(0.0 if align_corners else 0.5, dtype=torch.float32)
        fl = torch.floor(pos)
        cell, frac = fl.long(), (pos - fl).double()
        cfrac = 1.0 - frac
        if interpolation == 1:
            frac, cfrac = frac * frac * (3.0 - 2.0 * frac), cfrac * cfrac * (3.0 - 2.0 * cfrac)
        base, hsize = int(offsets[l]), int(offsets[l + 1]) - int(offsets[l])
        for k in range(K):
            bits = torch.tensor([(k >> d) & 1 for d in range(D)], dtype=torch.int64)
            wk = torch.ones((B,), dtype=torch.float64)
            for d in range(D):
                wk = wk * (frac[:, d] if (k >> d) & 1 else cfrac[:, d])
            keys[:, l, k] = base + ref._slot(cell + bits, D, gridtype, align_corners, hsize, res)
            w[:, l, k] = wk
    keys[oob] = n_slots
    w[oob] = 0.0
    return keys, w


def layout(x, offsets, per_level_scale, H, gridtype, align_corners):
    """Emit + stable sort by key: per non-empty slot (slot, lo, hi) in sorted order, N = B * L << D, and the flat keys with
    their stable sorting permutation."""
    keys, _ = entries(x, offsets, per_level_scale, H, gridtype, align_corners)
    keys = keys.reshape(-1)
    order = torch.argsort(keys, stable=True)
    slot, count = torch.unique_consecutive(keys[order], return_counts=True)
    hi = torch.cumsum(count, 0)
    lo = hi - count
    real = slot < int(offsets[-1])
    return Layout(slot[real], lo[real], hi[real], keys.numel(), keys, order)


def segment_class(lo, hi, chunk=CHUNK):
    """The kinds one sorted segment [lo, hi) belongs to (grid_slot_kernel: c_first = ceil(lo / chunk), c_last = hi // chunk)."""
    whole = hi // chunk - (lo + chunk - 1) // chunk
    if whole <= 0:
        return ("inside",) if lo // chunk == (hi - 1) // chunk else ("straddle",)
    head, tail = lo % chunk != 0, hi % chunk != 0
    kinds = []
    if not head and not tail and whole == 1:
        kinds.append("one_chunk")
    if head and not tail:
        kinds.append("head_chunks")
    if tail and not head:
        kinds.append("chunks_tail")
    if head and tail:
        kinds.append("head_chunks_tail")
    if whole >= 2:
        kinds.append("multi_chunk")
    return tuple(kinds)


def segment_classes(lo, hi, chunk=CHUNK):
    """{class: number of segments} over the segments [lo[i], hi[i])."""
    out = dict.fromkeys(CLASSES, 0)
    for a, b in zip(torch.as_tensor(lo).tolist(), torch.as_tensor(hi).tolist()):
        for k in segment_class(a, b, chunk):
            out[k] += 1
    return out


def sort_passes(n_slots):
    """The kernel's rule: end_bit = bits of n_slots (the sentinel sorts last), 8-bit passes."""
    end_bit = 1
    while end_bit < 32 and (n_slots >> end_bit) != 0:
        end_bit += 1
    return (end_bit + 7) // 8


def k_w(D, interpolation):
    return (6 if interpolation == 1 else 2) * D


def ulp32(v):
    """One fp32 ulp of |v|; 0 for 0 (an all-zero tensor has to be matched exactly)."""
    return float(np.spacing(np.float32(abs(v)))) if v != 0 else 0.0


# ---------------------------------------------------------------- exact cases
EXACT_GROUPS = ((256,), (128,), (384,), (64, 192, 256), (100, 412, 300), (700,), (255, 257), (1,))
EXACT_CELLS = ((1, 0), (3, 0), (1, 2), (3, 2))   # pairwise disjoint corner sets
ExactCase = namedtuple("ExactCase", "name groups C variant")
Tensors = namedtuple("Tensors", "x emb g offsets D C L H pls gridtype align interp")


def _exact_cases():
    out = []
    for gi, groups in enumerate(EXACT_GROUPS):
        tag = "g" + "_".join(map(str, groups))
        for C in (1, 2, 4, 8):
            out.append(ExactCase("%s-C%d-tiled-ac" % (tag, C), groups, C, "base"))
        for vi, variant in enumerate(("sentinel", "hash", "noac")):
            C = (1, 2, 4, 8)[(gi + vi) % 4]
            out.append(ExactCase("%s-C%d-%s" % (tag, C, variant), groups, C, variant))
    return out


EXACT = {c.name: c for c in _exact_cases()}


def exact_tensors(case):
    """base / sentinel: tiled, align_corners, 32 slots; hash: gridtype 0 with a 16-slot table (5^2 > 16: hashed);
    noac: x = (i - 0.25) / 4, pos = 4 x + 0.5.  sentinel: an outside point after every third inside point."""
    align = case.variant != "noac"
    shift = 0.0 if align else 0.5
    rows = []
    for (i, j), n in zip(EXACT_CELLS, case.groups):
        rows += [((i + 0.25 - shift) / 4.0, (j + 0.5 - shift) / 4.0)] * n
    if case.variant == "sentinel":
        mixed = []
        for n, r in enumerate(rows):
            mixed.append(r)
            if n % 3 == 2 or n == len(rows) - 1:
                mixed.append((1.5, 0.25) if n % 2 else (0.25, -0.25))
        rows = mixed
    x = torch.tensor(rows, dtype=torch.float32)
    B, C = x.shape[0], case.C
    gridtype = 0 if case.variant == "hash" else 1
    offsets = [0, 16] if case.variant == "hash" else ref.grid_offsets(2, 1, 2.0, 5, 19, align)
    s, c, b = torch.arange(offsets[-1])[:, None], torch.arange(C)[None, :], torch.arange(B)[:, None]
    emb = ((s * 7 + c * 13) % 61 - 30).float()
    g = ((1 + (b * 5 + c * 11) % 31) * torch.where((b + c) % 3 == 0, -1, 1)).float()
    return Tensors(x, emb, g, offsets, 2, C, 1, 5, 2.0, gridtype, align, 0)


def oracle(t, emb=None, g=None, dtype=torch.float64):
    """encoding_reference.grid_encode_ref forward + backward -> (outputs, embedding gradient, input gradient)."""
    xi = t.x.to(dtype).clone().requires_grad_(True)      # (float64 inputs: the input gradient is not rounded to fp32)
    e = (t.emb if emb is None else emb).detach().to(dtype).clone().requires_grad_(True)
    y = ref.grid_encode_ref(xi, e, t.offsets, t.pls, t.H, t.gridtype, t.align, t.interp, dtype=dtype)
    if t.x.shape[0] == 0:
        return y.detach(), torch.zeros_like(e), torch.zeros_like(t.x, dtype=dtype)
    y.backward((t.g if g is None else g).to(dtype))
    return y.detach(), e.grad.detach(), xi.grad.detach().to(dtype)


@functools.lru_cache(maxsize=None)
def exact_expectation(name):
    """-> (Tensors, Layout, float64 oracle triple)."""
    t = exact_tensors(EXACT[name])
    return t, layout(t.x, t.offsets, t.pls, t.H, t.gridtype, t.align), oracle(t)


def exact_classes(name):
    _, lay, _ = exact_expectation(name)
    return segment_classes(lay.lo, lay.hi)


def exact_id(name):
    """The case name and the segment classes it reaches."""
    return name + "-" + "+".join(k for k, n in exact_classes(name).items() if n)


def sorted_contributions(t, lay, dtype=np.float32):
    """[N, C] per sorted entry: w * grad[b, l, :] as the gather kernel forms it (one product), 0 for sentinel entries."""
    keys, w = entries(t.x, t.offsets, t.pls, t.H, t.gridtype, t.align, t.interp)
    B, L, K = keys.shape
    c = w.numpy().astype(dtype)[..., None] * t.g.view(B, L, 1, t.C).numpy().astype(dtype)
    return c.reshape(B * L * K, t.C)[lay.order.numpy()]


def slot_sums(t, lay, contrib, reverse=False, dtype=np.float32):
    """Dense [n_slots, C]: each slot's sorted entries added one by one, first to last (or last to first), in dtype."""
    out = np.zeros((int(t.offsets[-1]), t.C), dtype)
    for s, lo, hi in zip(lay.slot.tolist(), lay.lo.tolist(), lay.hi.tolist()):
        seg = contrib[lo:hi][::-1] if reverse else contrib[lo:hi]
        out[s] = np.add.accumulate(seg.astype(dtype), axis=0, dtype=dtype)[-1]
    return out


# ---------------------------------------------------------------- form cases
FormCase = namedtuple("FormCase", "name D C L H pls log2T gridtype align interp B kind")
FORM_CONFIGS = (("hash-smooth-noac", 0, False, 1), ("tiled-linear-ac", 1, True, 0))
EDGE_BASE = (0.37, 0.61, 0.23, 0.83, 0.47)


def _form_cases():
    out = []
    for D in (2, 3, 4, 5):
        for C in (1, 2, 4, 8):
            for tag, gt, ac, ip in FORM_CONFIGS:
                out.append(FormCase("D%dC%d-%s" % (D, C, tag), D, C, 4, 3, 1.6, 9, gt, ac, ip, 2000, "random"))
    for D in (2, 3):
        for tag, gt, ac, ip in FORM_CONFIGS:
            out.append(FormCase("edges-D%d-%s" % (D, tag), D, 2, 3, 5, 2.0, 9, gt, ac, ip, 0, "edges"))
    for tag, gt, ac, ip in FORM_CONFIGS:
        out += [FormCase("B1-" + tag, 3, 2, 4, 3, 1.6, 9, gt, ac, ip, 1, "random"),
                FormCase("BL255-" + tag, 3, 2, 3, 3, 1.6, 9, gt, ac, ip, 85, "random"),
                FormCase("BL513-" + tag, 3, 2, 3, 3, 1.6, 9, gt, ac, ip, 171, "random"),
                FormCase("all_outside-" + tag, 3, 2, 4, 3, 1.6, 9, gt, ac, ip, 300, "outside"),
                FormCase("L1-" + tag, 3, 2, 1, 3, 1.6, 9, gt, ac, ip, 300, "random"),
                FormCase("L64-" + tag, 3, 2, 64, 4, 1.02, 9, gt, ac, ip, 300, "random"),
                FormCase("pls1-" + tag, 3, 2, 4, 6, 1.0, 9, gt, ac, ip, 300, "random")]
    return out


FORM = {c.name: c for c in _form_cases()}
DEGENERATE = tuple(n for n in FORM if n.split("-")[0] in ("B1", "BL255", "BL513", "all_outside", "L1", "L64", "pls1"))


def edge_values(L, pls, H):
    """The inside / outside boundary and cell faces i / scale of every level."""
    f = np.float32
    vals = [f(0.0), f(-0.0), f(1.0), np.nextafter(f(1), f(0)), np.nextafter(f(1), f(2)), np.nextafter(f(0), f(-1)),
            f(2.0 ** -149)]
    for sc, _ in ref.level_geometry(L, pls, H):
        vals += [f(i) / f(sc) for i in sorted({1, int(sc) // 2, int(sc) - 1})]
    return vals


def edge_points(D, L, pls, H):
    """One edge value per row, in each dimension in turn, the other coordinates inside."""
    vals = edge_values(L, pls, H)
    x = torch.tensor(EDGE_BASE[:D], dtype=torch.float32).repeat(D * len(vals), 1)
    for d in range(D):
        for n, v in enumerate(vals):
            x[d * len(vals) + n, d] = float(v)
    return x


def form_tensors(case):
    seed = sum(map(ord, case.name))
    gen = torch.Generator().manual_seed(seed)
    if case.kind == "edges":
        x = edge_points(case.D, case.L, case.pls, case.H)
    elif case.kind == "outside":
        x = torch.rand((case.B, case.D), generator=gen)
        x[0::2, 0] = 1.0 + torch.rand((len(range(0, case.B, 2)),), generator=gen)
        x[1::2, case.D - 1] = -0.01 - torch.rand((len(range(1, case.B, 2)),), generator=gen)
    else:
        x = points(case.B, case.D, seed)
    offsets = ref.grid_offsets(case.D, case.L, case.pls, case.H, case.log2T, case.align)
    emb = torch.randn((offsets[-1], case.C), generator=gen)
    g = torch.randn((x.shape[0], case.L * case.C), generator=gen)
    return Tensors(x, emb, g, offsets, case.D, case.C, case.L, case.H, case.pls, case.gridtype, case.align, case.interp)


Expect = namedtuple("Expect", "t out gemb gin bar_out bar_emb bar_in n_s inside r32")


def expect(t):
    """The float64 oracle, the derived per-element / per-slot bars and the measured input-gradient bar of one call."""
    out, gemb, gin = oracle(t)
    A, _, _ = oracle(t, emb=t.emb.abs())
    _, A_s, _ = oracle(t, g=t.g.abs())
    lay = layout(t.x, t.offsets, t.pls, t.H, t.gridtype, t.align)
    n_slots = int(t.offsets[-1])
    n_s = torch.bincount(lay.keys, minlength=n_slots + 1)[:n_slots]
    kw = k_w(t.D, t.interp)
    bar_out = 2.0 * (kw + (1 << t.D) + 1) * U * A
    bar_emb = 2.0 * (kw + n_s[:, None].double() + 1) * U * A_s
    r32 = tuple(v.double() for v in oracle(t, dtype=torch.float32))
    top = float(gin.abs().max()) if gin.numel() else 0.0
    bar_in = max(8.0 * float((r32[2] - gin).abs().max()) if gin.numel() else 0.0, ulp32(top))
    inside = ~((t.x < 0) | (t.x > 1)).any(dim=1)
    return Expect(t, out, gemb, gin, bar_out, bar_emb, bar_in, n_s, inside, r32)


@functools.lru_cache(maxsize=None)
def form_expectation(name):
    return expect(form_tensors(FORM[name]))


# ---------------------------------------------------------------- pass-count cases (raw ABI: arbitrary int32 offsets)
PassCase = namedtuple("PassCase", "name D C H pls offsets B passes")
PASSES = {c.name: c for c in (
    PassCase("passes1-slots248", 2, 2, 12, 2.0, (0, 120, 248), 600, 1),
    PassCase("passes2-slots256", 2, 2, 12, 2.0, (0, 120, 256), 600, 2),
    PassCase("passes2-slots65528", 3, 2, 32, 2.0, (0, 32768, 65528), 600, 2),
    PassCase("passes3-slots65536", 3, 2, 32, 2.0, (0, 32768, 65536), 600, 3),
    PassCase("passes4-slots17x2^20", 3, 1, 16, 1.3, tuple(i << 20 for i in range(18)), 1000, 4))}


def pass_tensors(case):
    seed = sum(map(ord, case.name))
    gen = torch.Generator().manual_seed(seed)
    x = points(case.B, case.D, seed)
    L = len(case.offsets) - 1
    emb = torch.randn((case.offsets[-1], case.C), generator=gen)
    g = torch.randn((case.B, L * case.C), generator=gen)
    return Tensors(x, emb, g, list(case.offsets), case.D, case.C, L, case.H, case.pls, 0, False, 0)


SparseExpect = namedtuple("SparseExpect", "t out bar_out slots gemb bar_emb")


@functools.lru_cache(maxsize=None)
def sparse_expectation(name):
    """The four-pass case without a dense float64 table: outputs from the gathered corner rows, the embedding gradient by
    index_add_ in float64 on the touched slots only (sorted unique `slots`).  (The input gradient does not pass through the
    sort; the form cases hold it.)"""
    t = pass_tensors(PASSES[name])
    keys, w = entries(t.x, t.offsets, t.pls, t.H, t.gridtype, t.align, t.interp)
    B, L, K = keys.shape
    n_slots, C, D = int(t.offsets[-1]), t.C, t.D
    inside = keys[:, 0, 0] < n_slots
    rows = t.emb[keys.clamp(max=n_slots - 1)].double() * inside[:, None, None, None]          # [B, L, K, C]
    out = (w[..., None] * rows).sum(2).reshape(B, L * C)
    A = (w[..., None] * rows.abs()).sum(2).reshape(B, L * C)
    g = t.g.view(B, L, 1, C).double()
    slots, inv = torch.unique(keys.reshape(-1), return_inverse=True)
    contrib = (w[..., None] * g).reshape(-1, C)
    gemb = torch.zeros((slots.numel(), C), dtype=torch.float64).index_add_(0, inv, contrib)
    A_s = torch.zeros((slots.numel(), C), dtype=torch.float64).index_add_(0, inv, contrib.abs())
    n_s = torch.bincount(inv, minlength=slots.numel())
    real = slots < n_slots
    kw = k_w(D, t.interp)
    bar_out = 2.0 * (kw + K + 1) * U * A
    bar_emb = 2.0 * (kw + n_s[:, None].double() + 1) * U * A_s
    return SparseExpect(t, out, bar_out, slots[real], gemb[real], bar_emb[real])


# ---------------------------------------------------------------- spherical harmonics
SH_CASES = ("unit", "scaled", "axes", "B0", "B1", "B255", "B257")
ShExpect = namedtuple("ShExpect", "v gout out gin bar_out bar_in")


def sh_inputs(name, degree):
    gen = torch.Generator().manual_seed(100 * degree + SH_CASES.index(name))
    if name == "axes":
        e = torch.eye(3)
        pole = torch.tensor([[0.0, 0.0, 1.0]])
        v = torch.cat([e, -e, 0.5 * pole, -0.5 * pole, 2.0 * pole, -2.0 * pole, torch.zeros((1, 3))])
    else:
        B = 2000 if name in ("unit", "scaled") else int(name[1:])
        v = torch.randn((B, 3), generator=gen)
        v = v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)
        if name != "unit":
            v = v * (0.5 + 1.5 * torch.rand((B, 1), generator=gen))
    gout = torch.randn((v.shape[0], degree * degree), generator=gen)
    return v.float(), gout


@functools.lru_cache(maxsize=None)
def sh_expectation(name, degree):
    """float64 oracle; per output column (l, m) and per input component: 8 x the fp32 restatement's own distance in that
    column, floored at one fp32 ulp of the column's largest entry."""
    v, gout = sh_inputs(name, degree)
    res = []
    for dtype in (torch.float64, torch.float32):
        xi = v.to(dtype).clone().requires_grad_(True)
        y = ref.sh_encode_ref(xi, degree, dtype=dtype)
        if v.shape[0]:
            y.backward(gout.to(dtype))
            res.append((y.detach().double(), xi.grad.detach().double()))
        else:
            res.append((y.detach().double(), torch.zeros((0, 3), dtype=torch.float64)))
    (o, go), (r, gr) = res

    def bars(a64, a32):
        if a64.shape[0] == 0:
            return torch.zeros((a64.shape[1],), dtype=torch.float64)
        floor = torch.tensor([ulp32(c) for c in a64.abs().max(dim=0).values.tolist()], dtype=torch.float64)
        return torch.maximum(8.0 * (a32 - a64).abs().max(dim=0).values, floor)

    return ShExpect(v, gout, o, go, bars(o, r), bars(go, gr))
