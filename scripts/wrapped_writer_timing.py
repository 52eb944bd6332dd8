"""The batched wrapped writer (include/pco_gfx.h section 4c) at scale, one JSON line per measurement on stdout:

  compact_c2paged   pco_gfx_compact_wrapped_chunks on the `c2paged` shape (--chunks chunks of 2^18 u64 in pages of 16 384, Classic +
                    TryConsecutive(1)) against pco_gfx_compact_chunks moving the standalone chunks of the same data in the same process:
                    HIP events around each call, the median of --reps runs after a warm-up, plus the per-kernel times of one call
  compact_tiny      the same entry point over --tiny chunks of ONE number (two pieces each): the scan block's share
  async_overhead    the synchronous and the asynchronous form of the same explicit-spec pco_gfx_compress_wrapped_chunks_ex call: wall time
                    to completion and pco_gfx_workspace_bytes() of each (the asynchronous one takes a latent slot per chunk up front)

usage: wrapped_writer_timing.py [--chunks 1024] [--tiny 60000] [--reps 11]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from conv1_timing import profile  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402

N = 1 << 18
COMPACT_ARGTYPES = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]


def event_ms(fn, reps):
    """median / min of `reps` HIP-event timings of fn() on the default stream, after one warm-up"""
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), out


def c2_chunks(k):
    g = torch.Generator(device="cuda").manual_seed(2)
    base = (1 << 40) + 1000 * torch.arange(N, device="cuda", dtype=torch.int64)
    return (base[None, :] + torch.randint(0, 512, (k, N), device="cuda", generator=g)).contiguous()   # (u64 bits in an int64 tensor)


def wrapped_setup(L, src, n, cfg):
    k = src.shape[0]; esz = src.element_size()
    cap = L.pco_gfx_wrapped_chunk_cap(n, 2, C.addressof(cfg))
    slots = torch.zeros(cap * k, dtype=torch.uint8, device="cuda")
    tasks = (G.WrappedTask * k)(*[G.WrappedTask(src.data_ptr() + c * n * esz, n, slots.data_ptr() + c * cap, cap, 2, 0, None) for c in range(k)])
    n_pieces = k * (1 + L.pco_gfx_wrapped_n_pages(n, cfg.max_page_n))
    d_infos = torch.zeros(n_pieces * 32, dtype=torch.uint8, device="cuda")
    return tasks, slots, d_infos, n_pieces


def compact_wrapped_case(L, name, src, n, cfg, reps):
    k = src.shape[0]
    tasks, slots, d_infos, n_pieces = wrapped_setup(L, src, n, cfg)
    infos = (G.PageInfo * n_pieces)()
    G.check(L.pco_gfx_compress_wrapped_chunks_ex(k, tasks, C.addressof(cfg), infos, d_infos.data_ptr(), None))
    body = sum(infos[j].len for j in range(n_pieces))
    dst = torch.zeros(body + 4 * n_pieces + 64, dtype=torch.uint8, device="cuda"); offs = torch.zeros(n_pieces + 1, dtype=torch.int64, device="cuda")

    def run():
        G.check(L.pco_gfx_compact_wrapped_chunks(k, tasks, C.addressof(cfg), d_infos.data_ptr(), 4, dst.data_ptr(), dst.numel(), 0, offs.data_ptr(), None, None))
    med, best, raw = event_ms(run, reps)
    kernels = profile(L, run)
    assert int(offs[-1].item()) == body + 4 * n_pieces
    return {"case": name, "chunks": k, "n": n, "pieces": n_pieces, "bytes": body, "ms_median": round(med, 4), "ms_min": round(best, 4),
            "gbps_read_plus_written": round(2 * body / med / 1e6, 1), "kernels_ms": kernels, "raw_ms": [round(x, 4) for x in raw]}, body


def compact_standalone_baseline(L, src, cfg, reps):
    k = src.shape[0]; esz = src.element_size()
    L.pco_gfx_compact_chunks.argtypes = COMPACT_ARGTYPES
    cap = (L.pco_gfx_guarantee_chunk_size(N, 2) + 64 + 15) // 16 * 16
    slots = torch.zeros(cap * k, dtype=torch.uint8, device="cuda")
    tasks = (G.EncodeTask * k)(*[G.EncodeTask(src.data_ptr() + c * N * esz, N, slots.data_ptr() + c * cap, cap, 2, 0) for c in range(k)])
    res = (G.TaskResult * k)(); d_res = torch.zeros(k * 24, dtype=torch.uint8, device="cuda")
    G.check(L.pco_gfx_compress_chunks(k, tasks, C.byref(cfg), res, d_res.data_ptr(), None))
    body = sum(res[c].n_out for c in range(k))
    dst = torch.zeros(body + 64, dtype=torch.uint8, device="cuda"); offs = torch.zeros(k + 1, dtype=torch.int64, device="cuda")

    def run():
        G.check(L.pco_gfx_compact_chunks(k, tasks, d_res.data_ptr(), dst.data_ptr(), dst.numel(), 0, offs.data_ptr(), None, None))
    med, best, raw = event_ms(run, reps)
    return {"case": "compact_chunks_baseline", "chunks": k, "pieces": k, "bytes": body, "ms_median": round(med, 4), "ms_min": round(best, 4),
            "gbps_read_plus_written": round(2 * body / med / 1e6, 1), "kernels_ms": profile(L, run), "raw_ms": [round(x, 4) for x in raw]}


def async_overhead(L, src, cfg, reps):
    k = src.shape[0]
    tasks, slots, d_infos, n_pieces = wrapped_setup(L, src, N, cfg)
    infos = (G.PageInfo * n_pieces)()
    out = {"case": "async_overhead", "chunks": k, "pieces": n_pieces}
    for form in ("sync", "async"):
        L.pco_gfx_release_workspace()

        def run():
            G.check(L.pco_gfx_compress_wrapped_chunks_ex(k, tasks, C.addressof(cfg), infos if form == "sync" else None, d_infos.data_ptr(), None))
            torch.cuda.synchronize()
        run(); run()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter(); run(); t.append((time.perf_counter() - t0) * 1e3)
        out[form + "_ms_median"] = round(statistics.median(t), 3); out[form + "_workspace_bytes"] = int(L.pco_gfx_workspace_bytes())
        out[form + "_raw_ms"] = [round(x, 3) for x in t]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1024)
    ap.add_argument("--tiny", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    L = G.lib()
    cfg = G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1, max_page_n=16384)
    src = c2_chunks(a.chunks)
    base = compact_standalone_baseline(L, src, cfg, a.reps)
    new, _ = compact_wrapped_case(L, "compact_c2paged", src, N, cfg, a.reps)
    new["vs_baseline_time"] = round(new["ms_median"] / base["ms_median"], 3)
    print(json.dumps(base), flush=True); print(json.dumps(new), flush=True)
    print(json.dumps(async_overhead(L, src, cfg, max(a.reps // 2, 3))), flush=True)
    del src; torch.cuda.empty_cache(); L.pco_gfx_release_workspace()
    tiny = torch.arange(a.tiny, device="cuda", dtype=torch.int64).reshape(a.tiny, 1).contiguous()
    t, _ = compact_wrapped_case(L, "compact_tiny", tiny, 1, G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), a.reps)
    print(json.dumps(t), flush=True)


if __name__ == "__main__":
    main()
