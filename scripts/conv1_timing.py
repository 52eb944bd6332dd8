"""Conv1 delta encode (PCO_GFX_CFG_CONV1) at scale: smooth i32 / i16 series, many chunks of 2^18 numbers in one pco_gfx_compress_chunks call.

For each (dtype, order): per-kernel times of one call (pco_gfx_profile_begin / end), encode GB/s of the call next to the same call under
TryConsecutive(1), and the decode GB/s of the Conv1 chunks (pco_gfx_decompress_chunks; Conv1 decode is a serial recurrence per chunk).
Every chunk is decoded and compared with its input once.  One JSON line per case on stdout.
usage: conv1_timing.py [--chunks K] [--dtypes int32,int16] [--orders 1,2,8,32] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pcodec_amd import _lib as G  # noqa: E402

N = 1 << 18


def smooth_chunks(k, dtype, seed=1):
    """k chunks of N numbers: two sines of per-chunk period plus small integer noise, generated on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    i = torch.arange(N, device="cuda", dtype=torch.float32)[None, :]
    period = torch.randint(50, 900, (k, 1), device="cuda", generator=g).float()
    wave = torch.sin(2 * np.pi * i / period) + 0.3 * torch.sin(2 * np.pi * i / (period * 0.37 + 3))
    amp = 1e8 if dtype == torch.int32 else 12000.0
    noise = torch.randint(-3, 4, (k, N), device="cuda", generator=g).float() * (1000.0 if dtype == torch.int32 else 1.0)
    return torch.round(amp * wave + noise).to(dtype).contiguous()


def profile(L, fn):
    L.pco_gfx_profile_begin()
    fn()
    torch.cuda.synchronize()
    names = C.create_string_buffer(1 << 16)
    ms = (C.c_float * 4096)()
    nk = L.pco_gfx_profile_end(names, len(names), ms, 4096)
    raw = names.raw
    tot = {}
    pos = 0
    for j in range(nk):
        e = raw.index(b"\0", pos)
        nm = raw[pos:e].decode()
        pos = e + 1
        tot[nm] = tot.get(nm, 0.0) + ms[j]
    return {a: round(b, 4) for a, b in sorted(tot.items())}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--dtypes", default="int32,int16")
    ap.add_argument("--orders", default="1,2,8,32")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L = G.lib()
    k = a.chunks
    for dname in a.dtypes.split(","):
        tdt = {"int32": torch.int32, "int16": torch.int16}[dname]
        dt = G.DTYPE_BYTE[dname]
        src = smooth_chunks(k, tdt)
        esz = src.element_size()
        in_bytes = src.numel() * esz
        cap = (L.pco_gfx_guarantee_chunk_size(N, dt) + 64 + 15) // 16 * 16
        dst = torch.zeros(cap * k, dtype=torch.uint8, device="cuda")
        tasks = (G.EncodeTask * k)(*[G.EncodeTask(src.data_ptr() + c * N * esz, N, dst.data_ptr() + c * cap, cap, dt, 0) for c in range(k)])
        res = (G.TaskResult * k)()
        out = torch.zeros_like(src)

        def enc(cfg):
            G.check(L.pco_gfx_compress_chunks(k, tasks, C.byref(cfg), res, None, None))

        cons = G.make_config(level=8, mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1)
        t_cons = timed(lambda: enc(cons), a.reps)
        cons_bytes = sum(res[c].n_out for c in range(k))
        for order in [int(x) for x in a.orders.split(",")]:
            cfg = G.make_config(level=8, mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONV1, delta_order=order, conv1=True)
            t_enc = timed(lambda: enc(cfg), a.reps)
            kernels = profile(L, lambda: enc(cfg))
            comp = sum(res[c].n_out for c in range(k))
            n_fb = sum(res[c].aux & 1 for c in range(k))
            dtasks = (G.DecodeTask * k)(*[G.DecodeTask(dst.data_ptr() + c * cap, res[c].n_out, out.data_ptr() + c * N * esz, N, dt, 0) for c in range(k)])
            dres = (G.TaskResult * k)()

            def dec():
                G.check(L.pco_gfx_decompress_chunks(k, dtasks, dres, None, None))
            t_dec = timed(dec, a.reps)
            ok = bool(torch.equal(out, src))
            conv = {n: v for n, v in kernels.items() if "conv1" in n}
            print(json.dumps({
                "dtype": dname, "order": order, "chunks": k, "n": N, "roundtrip_ok": ok, "fallback_chunks": n_fb,
                "encode_gbps": round(in_bytes / t_enc / 1e9, 1), "encode_ms": round(t_enc * 1e3, 2),
                "consecutive1_encode_gbps": round(in_bytes / t_cons / 1e9, 1), "consecutive1_ratio": round(in_bytes / cons_bytes, 3),
                "ratio": round(in_bytes / comp, 3), "decode_gbps": round(in_bytes / t_dec / 1e9, 1), "decode_ms": round(t_dec * 1e3, 2),
                "conv1_kernels_ms": conv, "conv1_fit_plus_residuals_ms": round(sum(conv.values()), 3), "kernels_ms": kernels}), flush=True)
        del src, dst, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
