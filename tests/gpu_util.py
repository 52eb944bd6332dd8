"""Helpers for the -m gpu tests: synthetic BASELINE configs, device buffers, batched calls."""
import ctypes as C

import numpy as np

from pcodec_amd import _lib as G

N18 = 1 << 18


def cfg_pair(kind):
    """(product config, oracle config) for a BASELINE.json config name."""
    import oracle_lib as O
    table = {
        "c1": dict(mode=1, delta=1),                                    # Classic, NoOp
        "c2": dict(mode=1, delta=2, delta_order=1),                     # Classic, TryConsecutive(1)
        "c3": dict(mode=2, mode_f64=0.01, delta=1),                     # TryFloatMult(0.01), NoOp
        "c3d": dict(mode=2, mode_f64=0.01, delta=2, delta_order=1),
        "c4": dict(mode=1, delta=3),                                    # Classic, TryLookback
        "auto": dict(),
        "c2l12": dict(mode=1, delta=2, delta_order=1, level=12),   # BASELINE configs[1] at compression level 12 (up to 4096 bins)
    }[kind]
    return G.make_config(enable_8_bit=True, **table), O.make_config(**table)


def synth(kind, n=N18, seed=None):
    """SURVEY.md section 8(d) synthetic inputs."""
    if kind == "c1":
        return np.random.default_rng(1 if seed is None else seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "c2":
        r = np.random.default_rng(2 if seed is None else seed)
        return (np.uint64(1 << 40) + np.uint64(1000) * np.arange(n, dtype=np.uint64) + r.integers(0, 512, n).astype(np.uint64))
    if kind in ("c3", "c3d"):
        return np.random.default_rng(3 if seed is None else seed).integers(1000, 10000, n) / 100.0
    if kind == "c4":
        base = np.random.default_rng(40).integers(-(1 << 40), 1 << 40, 365)
        return (base[np.arange(n) % 365] + np.random.default_rng(4 if seed is None else seed).integers(-3, 4, n)).astype(np.int64)
    raise KeyError(kind)


def bits_equal(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))


def gpu_simple_decompress(data, np_dtype, cap):
    L = G.lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(max(cap, 1), dtype=np_dtype)
    n = C.c_size_t(0)
    code = L.pco_standalone_simple_decompress_into(buf.ctypes.data_as(C.c_void_p) if len(buf) else None, len(buf),
                                                   G.DTYPE_BYTE[np.dtype(np_dtype).name], out.ctypes.data_as(C.c_void_p),
                                                   cap, C.byref(n))
    G.check(code)
    return out[: n.value].copy()


def gpu_simple_compress(arr, cfg, uniform_type=False):
    L = G.lib()
    arr = np.ascontiguousarray(arr)
    dt = G.DTYPE_BYTE[arr.dtype.name]
    cap = L.pco_gfx_guarantee_file_size(arr.size, dt, cfg.max_page_n) + 64
    dst = np.empty(cap, np.uint8); n = C.c_size_t(0)
    code = L.pco_gfx_simple_compress_into_ex(arr.ctypes.data_as(C.c_void_p), arr.size, dt, C.byref(cfg),
                                             1 if uniform_type else 0, dst.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    G.check(code)
    return dst[: n.value].tobytes()


def gpu_batched(arrays, cfg):
    """One pco_gfx_compress_chunks call over `arrays` (any mix of dtypes / sizes; device buffers through torch), then one
    pco_gfx_decompress_chunks call over what it produced.  Returns ([standalone chunk bytes], [decoded arrays])."""
    import torch
    L = G.lib()
    arrays = [np.ascontiguousarray(a) for a in arrays]
    srcs = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in arrays]
    caps = [(L.pco_gfx_guarantee_chunk_size(a.size, G.DTYPE_BYTE[a.dtype.name]) + 64 + 15) // 16 * 16 for a in arrays]
    dsts = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    k = len(arrays)
    tasks = (G.EncodeTask * k)(*[G.EncodeTask(s.data_ptr(), a.size, d.data_ptr(), c, G.DTYPE_BYTE[a.dtype.name], 0)
                                 for a, s, d, c in zip(arrays, srcs, dsts, caps)])
    res = (G.TaskResult * k)()
    G.check(L.pco_gfx_compress_chunks(k, tasks, C.byref(cfg), res, None, None))
    outs = [torch.empty(max(a.nbytes, 1), dtype=torch.uint8, device="cuda") for a in arrays]
    dtasks = (G.DecodeTask * k)(*[G.DecodeTask(d.data_ptr(), res[i].n_out, o.data_ptr(), a.size, G.DTYPE_BYTE[a.dtype.name], 0)
                                  for i, (a, d, o) in enumerate(zip(arrays, dsts, outs))])
    dres = (G.TaskResult * k)()
    G.check(L.pco_gfx_decompress_chunks(k, dtasks, dres, None, None))
    chunks = [bytes(dsts[i][: res[i].n_out].cpu().numpy()) for i in range(k)]
    back = []
    for i, a in enumerate(arrays):
        assert dres[i].n_out == a.size and dres[i].consumed == res[i].n_out, (i, dres[i].n_out, a.size)
        back.append(outs[i][: a.nbytes].cpu().numpy().view(a.dtype))
    return chunks, back


def chunk_of_file(file_bytes, chunk_len):
    """The single chunk inside an oracle-written one-chunk standalone file (header | chunk | 0x00)."""
    return file_bytes[len(file_bytes) - 1 - chunk_len:-1]


def profile_names(L):
    """Names of the kernels / spans timed since pco_gfx_profile_begin() (pco_gfx_profile_end), as a sorted list without repeats."""
    import ctypes as C
    import torch
    torch.cuda.synchronize()
    names = C.create_string_buffer(1 << 16); ms = (C.c_float * 4096)()
    nk = L.pco_gfx_profile_end(names, len(names), ms, 4096)
    raw = names.raw; out = []; pos = 0
    for _ in range(nk):
        e = raw.index(b"\0", pos); out.append(raw[pos:e].decode()); pos = e + 1
    return sorted(set(out))


def profile_launches(L):
    """Every name timed since pco_gfx_profile_begin(), in launch order, repeats kept (profile_names drops them)."""
    import torch
    torch.cuda.synchronize()
    names = C.create_string_buffer(1 << 18); ms = (C.c_float * 8192)()
    nk = L.pco_gfx_profile_end(names, len(names), ms, 8192)
    raw = names.raw; out = []; pos = 0
    for _ in range(nk):
        e = raw.index(b"\0", pos); out.append(raw[pos:e].decode()); pos = e + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# Batches on device buffers for the stream / thread / compaction tests (test_gpu_streams.py, test_gpu_compact.py): the arrays of a call side
# by side in ONE device tensor, their worst-case slots in a second, their decode outputs in a third, and the task arrays as numpy records
# (so that they can live in pinned memory, be overwritten after a call, and be sliced).
# ---------------------------------------------------------------------------------------------------------------------------------------
RES_DT = np.dtype([("n_out", "<u8"), ("consumed", "<u8"), ("status", "<u4"), ("aux", "<u4")])
ENC_DT = np.dtype([("src", "<u8"), ("n", "<u8"), ("dst", "<u8"), ("dst_cap", "<u8"), ("dtype", "<u4"), ("reserved", "<u4")])
DEC_DT = np.dtype([("src", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("dst_cap", "<u8"), ("dtype", "<u4"), ("flags", "<u4")])
PAGE_DT = np.dtype([("meta", "<u8"), ("meta_len", "<u8"), ("page", "<u8"), ("page_len", "<u8"), ("dst", "<u8"), ("page_n", "<u8"),
                    ("dtype", "<u4"), ("format_major", "<u4")])
COMPACT_ARGTYPES = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]


def standalone_header_len(n_hint):
    """Byte length of the standalone header in front of the first chunk (docs/format.md: magic, standalone version, uniform type byte, the
    varint n_hint -- 6 bits of bit length - 1, then the bits --, wrapped version major.minor), by the format's arithmetic alone."""
    return 4 + 1 + 1 + (6 + max(int(n_hint).bit_length(), 1) + 7) // 8 + 2


def oracle_chunk(a, ocfg):
    """The standalone chunk the oracle writes for `a`: its one-chunk file without header and terminator."""
    f = __import__("oracle_lib").simple_compress(a, ocfg)
    return f[standalone_header_len(np.asarray(a).size):-1]


def pinned(records):
    """A copy of a numpy record array in pinned host memory (an upload from it does not have to wait for the stream)."""
    import torch
    t = torch.empty(max(records.nbytes, 1), dtype=torch.uint8, pin_memory=True)
    out = t.numpy()[: records.nbytes].view(records.dtype)
    out[:] = records
    return out


def ptr(records):
    return C.c_void_p(records.ctypes.data) if records.size else None


def device_delay(stream, ms=30):
    """Bounded device work of tens of milliseconds on `stream`: a chain of 256 MiB device-to-device copies (each moves 0.5 GiB through
    HBM; ~0.15 ms at 3.5 TB/s, so ~7 of them per millisecond).  Nothing open-ended: the chain has a fixed length."""
    import torch
    if not hasattr(device_delay, "bufs"):
        device_delay.bufs = (torch.zeros(1 << 28, dtype=torch.uint8, device="cuda"), torch.zeros(1 << 28, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
    a, b = device_delay.bufs
    with torch.cuda.stream(stream):
        for _ in range(7 * ms):
            b.copy_(a, non_blocking=True)


class Staged:
    """`arrays` (any mix of number types and sizes) staged for the batched entry points.  Everything is allocated and filled on the default
    stream and the device is synchronised before the constructor returns, so a non-blocking caller stream may use the buffers at once."""

    def __init__(self, L, arrays, on_device=True, cap_extra=64):
        import torch
        self.L = L
        self.arrays = [np.ascontiguousarray(a) for a in arrays]
        self.k = len(self.arrays)
        self.dtb = np.array([G.DTYPE_BYTE[a.dtype.name] for a in self.arrays], np.uint32)
        self.n = np.array([a.size for a in self.arrays], np.uint64)
        nb = np.array([(a.nbytes + 15) // 16 * 16 for a in self.arrays], np.int64)
        self.in_off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        self.host_in = np.zeros(int(self.in_off[-1]) + 64, np.uint8)
        for a, o in zip(self.arrays, self.in_off):
            self.host_in[o: o + a.nbytes] = a.view(np.uint8).reshape(-1)
        self.caps = np.array([(L.pco_gfx_guarantee_chunk_size(a.size, int(d)) + cap_extra + 15) // 16 * 16 for a, d in zip(self.arrays, self.dtb)], np.int64)
        self.slot_off = np.concatenate([[0], np.cumsum(self.caps)]).astype(np.int64)
        self.src = torch.from_numpy(self.host_in).cuda() if on_device else torch.zeros(self.host_in.size, dtype=torch.uint8, device="cuda")
        self.slots = torch.zeros(int(self.slot_off[-1]) + 64, dtype=torch.uint8, device="cuda")
        self.out = torch.zeros(self.host_in.size, dtype=torch.uint8, device="cuda")
        self.d_res = torch.zeros(max(self.k, 1) * RES_DT.itemsize, dtype=torch.uint8, device="cuda")
        self.d_dres = torch.zeros(max(self.k, 1) * RES_DT.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def enc_tasks(self, src=None, slots=None, caps=None):
        t = np.zeros(self.k, ENC_DT)
        t["src"] = (src if src is not None else self.src).data_ptr() + self.in_off[:-1].astype(np.uint64)
        t["n"] = self.n
        t["dst"] = (slots if slots is not None else self.slots).data_ptr() + self.slot_off[:-1].astype(np.uint64)
        t["dst_cap"] = self.caps if caps is None else caps
        t["dtype"] = self.dtb
        return t

    def dec_tasks(self, sizes, slots=None, out=None):
        t = np.zeros(self.k, DEC_DT)
        t["src"] = (slots if slots is not None else self.slots).data_ptr() + self.slot_off[:-1].astype(np.uint64)
        t["src_len"] = np.asarray(sizes, np.uint64)
        t["dst"] = (out if out is not None else self.out).data_ptr() + self.in_off[:-1].astype(np.uint64)
        t["dst_cap"] = self.n
        t["dtype"] = self.dtb
        return t

    def slot_bytes(self, sizes, slots=None):
        """[chunk i's first sizes[i] bytes] read back from the slots"""
        host = (slots if slots is not None else self.slots).cpu().numpy()
        return [host[o: o + int(s)].tobytes() for o, s in zip(self.slot_off[:-1], sizes)]

    def put_chunks(self, chunks, slots=None):
        """host chunk bytes into the slots (a tensor of the slots' layout is returned when none is given)"""
        import torch
        host = np.zeros(int(self.slot_off[-1]) + 64, np.uint8)
        for c, o, cap in zip(chunks, self.slot_off[:-1], self.caps):
            assert len(c) + 16 <= cap
            host[o: o + len(c)] = np.frombuffer(c, np.uint8)
        t = torch.from_numpy(host).cuda()
        if slots is None:
            return t
        slots.copy_(t)
        torch.cuda.synchronize()
        return slots

    def outputs_equal(self, out=None):
        """indices of the chunks whose decoded bytes differ from the input, compared over the whole area at once"""
        host = (out if out is not None else self.out).cpu().numpy()
        if np.array_equal(host[: self.in_off[-1]], self.host_in[: self.in_off[-1]]):
            return []
        return [i for i, (a, o) in enumerate(zip(self.arrays, self.in_off)) if not np.array_equal(host[o: o + a.nbytes], self.host_in[o: o + a.nbytes])]

    def results(self, d=None):
        return (d if d is not None else self.d_res).cpu().numpy()[: self.k * RES_DT.itemsize].view(RES_DT).copy()


def tile(distinct, k):
    """k arrays cycling through `distinct` (the oracle's bytes are then needed for the distinct ones only, and still compared for every chunk)"""
    return [distinct[i % len(distinct)] for i in range(k)]
