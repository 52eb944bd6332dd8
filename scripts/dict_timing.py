"""Dict mode encode (PCO_GFX_CFG_DICT) at scale: chunks of 2^18 IDs drawn from a 64-bit range, k distinct values per chunk, many chunks in one
pco_gfx_compress_chunks call.

For each (dtype, k): encode GB/s of TryDict + NoOp next to Classic + NoOp and Classic + TryConsecutive(1) on the same data, per-kernel times of
the Dict call (pco_gfx_profile_begin / end), and the decode GB/s of the Dict chunks (the general pco_decode_kernel).  Every chunk is decoded
and compared with its input once.  One JSON line per case on stdout.
usage: dict_timing.py [--chunks K] [--dtypes uint64,uint32] [--ks 256,4096,65536,131072] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from conv1_timing import N, profile, timed  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402


def id_chunks(k_chunks, k, dtype, seed=1):
    """k_chunks chunks of N numbers, each drawn uniformly from its own k random IDs of the type's full range, generated on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bits = 64 if dtype == torch.int64 else 32
    ids = torch.randint(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, (k_chunks, k), device="cuda", generator=g, dtype=torch.int64)
    pick = torch.randint(0, k, (k_chunks, N), device="cuda", generator=g)
    return torch.gather(ids, 1, pick).to(dtype).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--dtypes", default="uint64,uint32")
    ap.add_argument("--ks", default="256,4096,65536,131072")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L = G.lib()
    kc = a.chunks
    for dname in a.dtypes.split(","):
        tdt = {"uint64": torch.int64, "uint32": torch.int32}[dname]   # (the same bits: torch has no unsigned 64 / 32-bit arithmetic)
        dt = G.DTYPE_BYTE[dname]
        for k in [int(x) for x in a.ks.split(",")]:
            src = id_chunks(kc, k, tdt)
            esz = src.element_size()
            in_bytes = src.numel() * esz
            cap = (L.pco_gfx_guarantee_chunk_size(N, dt) + 64 + 15) // 16 * 16
            dst = torch.zeros(cap * kc, dtype=torch.uint8, device="cuda")
            tasks = (G.EncodeTask * kc)(*[G.EncodeTask(src.data_ptr() + c * N * esz, N, dst.data_ptr() + c * cap, cap, dt, 0) for c in range(kc)])
            res = (G.TaskResult * kc)()
            out = torch.zeros_like(src)

            def enc(cfg):
                G.check(L.pco_gfx_compress_chunks(kc, tasks, C.byref(cfg), res, None, None))

            rates = {}
            cfg = G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True)
            others = (("classic_noop", G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP)),
                      ("classic_consecutive1", G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1)))
            for c in [cfg] + [c for _, c in others]:   # (every config once before anything is timed: the workspace reaches its size)
                enc(c)
            t_enc = timed(lambda: enc(cfg), a.reps)
            for name, c in others:
                rates[name] = round(in_bytes / timed(lambda: enc(c), a.reps) / 1e9, 1)
            kernels = profile(L, lambda: enc(cfg))
            comp = sum(res[c].n_out for c in range(kc))
            n_fb = sum(res[c].aux & 1 for c in range(kc))
            dtasks = (G.DecodeTask * kc)(*[G.DecodeTask(dst.data_ptr() + c * cap, res[c].n_out, out.data_ptr() + c * N * esz, N, dt, 0) for c in range(kc)])
            dres = (G.TaskResult * kc)()

            def dec():
                G.check(L.pco_gfx_decompress_chunks(kc, dtasks, dres, None, None))
            t_dec = timed(dec, a.reps)
            ok = bool(torch.equal(out, src))
            dk = {n: v for n, v in kernels.items() if "dict" in n}
            print(json.dumps({
                "dtype": dname, "k": k, "chunks": kc, "n": N, "roundtrip_ok": ok, "fallback_chunks": n_fb,
                "encode_gbps": round(in_bytes / t_enc / 1e9, 1), "encode_ms": round(t_enc * 1e3, 2), "ratio": round(in_bytes / comp, 3),
                "classic_noop_encode_gbps": rates["classic_noop"], "consecutive1_encode_gbps": rates["classic_consecutive1"],
                "encode_vs_classic": round(in_bytes / t_enc / 1e9 / rates["classic_noop"], 3),
                "decode_gbps": round(in_bytes / t_dec / 1e9, 1), "decode_ms": round(t_dec * 1e3, 2),
                "dict_kernels_ms": dk, "dict_kernels_total_ms": round(sum(dk.values()), 3), "kernels_ms": kernels}), flush=True)
            del src, dst, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
