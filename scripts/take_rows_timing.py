"""DESIGN §8, "Built since (header §4n)": pco_gfx_take_rows against whole-page decode + index_select and against segment-parallel reads + index_select.

64 pages of 2^20 u64 rows (Classic, Consecutive(1)), index stride 4096; uniformly random selections of 0.1 %, 1 %, 10 % and 100 % of the rows, sorted
and unsorted, and one contiguous 1 % run.  Medians of 7 timed calls behind 2 warm-up calls, with the spread (min .. max); wall clock around the call,
the index_select and one stream synchronisation, so host cost counts.  Then the per-kernel times of one take call (pco_gfx_profile_*) and the mark
and gather kernels' bytes per second beside a plain torch copy of as many bytes.

    python scripts/take_rows_timing.py [--pages 64] [--out take_rows_timing.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec, PagingSpec  # noqa: E402

PAGE_N, EVERY, WARM, REPS = 1 << 20, 4096, 2, 7


def timed(fn, torch):
    for _ in range(WARM):
        fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def profile(L, fn, torch):
    """{kernel name: summed ms} of one call"""
    torch.cuda.synchronize(); L.pco_gfx_profile_begin(); fn(); torch.cuda.synchronize()
    names = C.create_string_buffer(1 << 18); ms = (C.c_float * 8192)()
    nk = L.pco_gfx_profile_end(names, len(names), ms, 8192)
    out = {}; pos = 0
    for k in range(nk):
        e = names.raw.index(b"\0", pos); name = names.raw[pos:e].decode(); pos = e + 1
        out[name] = out.get(name, 0.0) + ms[k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    L = G.lib()
    n_pages, total = args.pages, args.pages * PAGE_N
    rng = np.random.default_rng(1)
    x = np.cumsum(rng.integers(0, 1000, total, dtype=np.int64)).astype(np.uint64)
    d_x = torch.from_numpy(x.view(np.int64)).cuda().view(torch.uint64)
    per_chunk = min(n_pages, 16)   # a chunk holds 2^24 numbers at most: 16 pages
    n_chunks = n_pages // per_chunk
    assert n_chunks * per_chunk == n_pages
    where = [(p // per_chunk, p % per_chunk) for p in range(n_pages)]   # page p of the file: (chunk, page of the chunk); its row_base is p * PAGE_N
    cc = paged.compress_chunks([d_x[c * per_chunk * PAGE_N: (c + 1) * per_chunk * PAGE_N] for c in range(n_chunks)], ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_consecutive(1), paging_spec=PagingSpec.equal_pages_up_to(PAGE_N)))
    directory = cc.directory
    src = paged._BlobPages(cc.blob, directory, ["uint64"] * n_chunks)
    assert all(src.ns[c] == [PAGE_N] * per_chunk for c in range(n_chunks))
    index = paged.index_pages(cc.blob, directory, ["uint64"] * n_chunks, EVERY)
    torch.cuda.synchronize()
    saved = paged._saved(index)
    full = torch.empty(total, dtype=torch.int64, device="cuda")
    res_dev = torch.zeros(max(n_pages, 1) * 24, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    page_tasks = (G.PageTask * n_pages)(*[src.page_task(c, i, full.data_ptr() + p * PAGE_N * 8) for p, (c, i) in enumerate(where)])
    reads = [paged._segment_task(src, c, i, full.data_ptr() + (p * PAGE_N + row) * 8, row, min(EVERY, PAGE_N - row), saved.get((c, src.piece[c][i])), s, None)
             for p, (c, i) in enumerate(where) for s, row in enumerate(range(0, PAGE_N, EVERY))]
    read_tasks = (G.PageReadTask * len(reads))(*reads)
    read_res = (G.TaskResult * len(reads))()

    def whole(ids):
        G.check(L.pco_gfx_decompress_pages(n_pages, page_tasks, None, res_dev.data_ptr(), stream))
        return torch.index_select(full, 0, ids)

    def segments(ids):
        G.check(L.pco_gfx_decompress_page_reads(len(reads), read_tasks, read_res, None, stream))
        return torch.index_select(full, 0, ids)

    def take_call(ids, out):
        tasks = (G.TakeTask * n_pages)(*[G.TakeTask(*src.metas[c], *src.pages[c][i], PAGE_N, p * PAGE_N, saved[(c, src.piece[c][i])].cursors.data_ptr(), EVERY,
                                                    ids.data_ptr(), ids.numel(), out.data_ptr(), G.DTYPE_BYTE["uint64"], 4) for p, (c, i) in enumerate(where)])
        return lambda: G.check(L.pco_gfx_take_rows(n_pages, tasks, 0, None, res_dev.data_ptr(), stream))

    selections = []
    for frac in (0.001, 0.01, 0.1, 1.0):
        k = int(total * frac)
        ids = rng.permutation(total)[:k] if frac < 1.0 else rng.permutation(total)
        selections += [(f"{frac * 100:g} % unsorted", ids), (f"{frac * 100:g} % sorted", np.sort(ids))]
    start = total // 3
    selections.append(("1 % contiguous", np.arange(start, start + total // 100)))

    lines = [f"{n_pages} pages of 2^20 u64, Classic / Consecutive(1), stride {EVERY}; ms, median of {REPS} (min .. max) behind {WARM} warm-ups", "",
             "| selection | take_rows | (a) pages + index_select | (b) segment reads + index_select | segments walked | batches walked |", "|---|---|---|---|---|---|"]
    profiles = {}
    for name, ids_np in selections:
        ids = torch.from_numpy(ids_np.astype(np.int64)).cuda()
        out = torch.empty(ids.numel(), dtype=torch.int64, device="cuda")
        take = take_call(ids, out)
        t = timed(take, torch)
        rec = res_dev.cpu().numpy()[: n_pages * 24].view(paged.RESULT_DT)
        assert (rec["status"] == 0).all() and int(rec["n_out"].sum()) == ids.numel()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), x[ids_np]), name
        a = timed(lambda: whole(ids), torch)
        b = timed(lambda: segments(ids), torch)
        assert np.array_equal(segments(ids).cpu().numpy().view(np.uint64), x[ids_np]), name
        fmt = lambda m: f"{m[0]:.2f} ({m[1]:.2f} .. {m[2]:.2f})"   # noqa: E731
        lines.append(f"| {name} | {fmt(t)} | {fmt(a)} | {fmt(b)} | {int(rec['aux'].sum())} | {int(rec['consumed'].sum())} |")
        if name in ("1 % unsorted", "100 % unsorted", "100 % sorted"):
            profiles[name] = (profile(L, take, torch), profile(L, lambda: segments(ids), torch), ids.numel())
        print(lines[-1], flush=True)

    for name, (pt, pb, k) in profiles.items():
        lines += ["", f"per kernel, {name} (ms): take_rows " + ", ".join(f"{n} {v:.3f}" for n, v in sorted(pt.items())),
                  f"    (b) " + ", ".join(f"{n} {v:.3f}" for n, v in sorted(pb.items()))]
        # the mark kernel reads every task's whole id list; the gather kernel reads it again, reads one row and writes one per owned id
        mark_bytes, gather_bytes = n_pages * k * 8, n_pages * k * 8 + 2 * k * 8
        for kernel, nbytes in (("take_mark_kernel", mark_bytes), ("take_gather_kernel", gather_bytes)):
            a_src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"); a_dst = torch.empty_like(a_src)
            copy_ms = timed(lambda: a_dst.copy_(a_src), torch)[0]   # a copy of nbytes / 2 bytes moves nbytes
            lines.append(f"    {kernel}: {nbytes / 1e9 / (pt[kernel] / 1e3):.0f} GB/s over {nbytes / 1e6:.1f} MB; torch copy of as many bytes: {nbytes / 1e9 / (copy_ms / 1e3):.0f} GB/s (wall clock)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
