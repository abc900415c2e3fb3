"""Developer tool: DNGaussian's hash-grid encoder (L=16, C=2, H=16, 2^19-slot tables, desired_resolution 512) at
P = 100k and 1M: the HIP forward (with dy_dx, as DNGaussian runs it: xyz requires grad), the embedding backward and
the input backward, against a torch float32 formulation on the same GPU (gather, index_add_) - what a ROCm user has
without csrc/gs_encoding.hip.  Prints the bytes each HIP stage moves (a model, below) and its fraction of 6.3 TB/s
(MI355X HBM, measured float4 copy).  No target is asserted."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sparse-view-3dgs-pack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import encoding_reference as ref  # noqa: E402
from gridencoder import GridEncoder  # noqa: E402
from gsplat_amd._lib import hip_api  # noqa: E402

HBM = 6.3e12
D, L, Cc = 3, 16, 2


def timed(fn, iters):
    for _ in range(2):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_corners(x, enc, geo):
    """fp32 torch: per level the 8 corner rows and weights (the reference's geometry)."""
    rows, ws = [], []
    offs = enc.offsets.tolist()
    for l, (sc, res) in enumerate(geo):
        pos = x * float(sc) + 0.5
        fl = torch.floor(pos)
        cell = fl.long()
        frac = pos - fl
        for k in range(8):
            bits = torch.tensor([(k >> d) & 1 for d in range(D)], device=x.device)
            w = torch.ones_like(frac[:, 0])
            for d in range(D):
                w = w * (frac[:, d] if (k >> d) & 1 else 1.0 - frac[:, d])
            rows.append(offs[l] + ref._slot(cell + bits, D, 0, False, offs[l + 1] - offs[l], res))
            ws.append(w)
    return rows, ws


def main():
    api = hip_api()
    dev = torch.device("cuda")
    enc = GridEncoder(input_dim=3, num_levels=L, level_dim=Cc, base_resolution=16, log2_hashmap_size=19,
                      desired_resolution=512).to(dev)
    S_slots = enc.embeddings.shape[0]
    S = float(np.log2(enc.per_level_scale))
    geo = ref.level_geometry(L, enc.per_level_scale, 16)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("DNGaussian grid: L=%d C=%d, %d slots (%.1f MB fp32)" % (L, Cc, S_slots, S_slots * Cc * 4 / 1e6))
    for P in (100_000, 1_000_000):
        g = torch.Generator().manual_seed(0)
        x = torch.rand((P, D), generator=g).to(dev)
        gout = torch.randn((P, L * Cc), generator=g).to(dev)
        out = torch.empty((P, L * Cc), device=dev)
        dy_dx = torch.empty((P, L * D * Cc), device=dev)
        gemb = torch.empty_like(enc.embeddings)
        gin = torch.empty((P, D), device=dev)
        nbytes = int(api.raw("grid_encode_tmp_bytes")(P, D, L, Cc, S_slots))
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        common = (enc.offsets.data_ptr(), L, S, 16, 0, 0, 0)

        def fwd():
            api.call("grid_encode_fwd", x.data_ptr(), P, D, enc.embeddings.data_ptr(), S_slots, Cc, *common, out.data_ptr(),
                     dy_dx.data_ptr(), stream)

        def bwd_emb():
            api.call("grid_encode_bwd", gout.data_ptr(), x.data_ptr(), P, D, S_slots, Cc, *common, None, gemb.data_ptr(),
                     None, tmp.data_ptr(), nbytes, stream)

        def bwd_in():
            api.call("grid_encode_bwd", gout.data_ptr(), x.data_ptr(), P, D, S_slots, Cc, *common, dy_dx.data_ptr(), None,
                     gin.data_ptr(), None, 0, stream)

        rows, ws = torch_corners(x, enc, geo)
        emb = enc.embeddings.detach()
        g_lc = gout.view(P, L, Cc)

        def t_fwd():
            r, w = torch_corners(x, enc, geo)
            acc = [sum(w[l * 8 + k][:, None] * emb[r[l * 8 + k]] for k in range(8)) for l in range(L)]
            return torch.stack(acc, 1)

        def t_bwd():
            ge = torch.zeros_like(emb)
            for l in range(L):
                for k in range(8):
                    ge.index_add_(0, rows[l * 8 + k], ws[l * 8 + k][:, None] * g_lc[:, l])
            return ge

        it = 20 if P <= 100_000 else 5
        N = P * L * 8
        fwd_b = P * D * 4 + P * L * Cc * 4 + P * L * D * Cc * 4 + N * Cc * 4  # inputs, outputs, dy_dx, one gather per corner
        # emit (keys + ids), 3 sort passes (read + write keys + ids), gather (sorted pairs, inputs, grad, contributions),
        # mark (keys), slot sums (ranges, contributions, table)
        bwd_b = 8 * N + 3 * 16 * N + (8 + D * 4 + Cc * 4 + Cc * 4) * N + 4 * N + 8 * S_slots + Cc * 4 * N + Cc * 4 * S_slots
        in_b = P * L * D * Cc * 4 + P * L * Cc * 4 + P * D * 4
        rows_out = [("HIP forward (+dy_dx)", timed(fwd, it), fwd_b), ("HIP backward, embeddings", timed(bwd_emb, it), bwd_b),
                    ("HIP backward, inputs", timed(bwd_in, it), in_b),
                    ("torch fp32 forward (gather)", timed(t_fwd, max(2, it // 4)), None),
                    ("torch fp32 backward (index_add_)", timed(t_bwd, max(2, it // 4)), None)]
        print("P=%d (%d corner contributions)" % (P, N))
        for name, ms, b in rows_out:
            if b is None:
                print("  %-34s %8.3f ms" % (name, ms))
            else:
                print("  %-34s %8.3f ms  %7.1f MB  %5.1f%% of HBM" % (name, ms, b / 1e6, 100.0 * b / (ms * 1e-3) / HBM))
        del tmp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
