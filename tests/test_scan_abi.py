"""CPU: pco_gfx_scan_chunks (include/pco_gfx.h section 4m) without a device.

The struct against an offsetof probe compiled from the header; every host check of the entry point, in its order, in both forms, with `results`
untouched; n_tasks == 0; pcodec_amd/csrc/pco_scan.h compiled alone with g++ -- the lines the scan kernel runs on a file's header and a chunk's
preamble -- against the oracle's reader on the reference's 13 golden .pco assets and against the header's table on a header cut after every byte;
and the task lists pcodec_amd.paged builds for scan_files and decompress_files, field for field, under a fake torch and a fake library."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import oracle_lib as O  # noqa: E402
import paged_plan_util as U  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import build as B  # noqa: E402

CSRC = os.path.abspath(os.path.join(HERE, "..", "pcodec_amd", "csrc"))
INCLUDE = os.path.abspath(os.path.join(HERE, "..", "include"))
ASSETS = sorted(glob.glob(os.path.join(HERE, "golden", "ref_assets", "*.pco")))
OK, CORRUPTION, INSUFFICIENT, INVALID = G.ST_OK, G.ST_CORRUPTION, G.ST_INSUFFICIENT_DATA, G.ST_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    if B.needs_build():
        B.build()
    return G.lib()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the struct
# ---------------------------------------------------------------------------------------------------------------------------------------
FIELDS = ["src", "src_len", "d_offsets", "d_counts", "max_chunks", "dtype", "flags", "reserved"]


def test_the_struct_is_the_header_s(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pco_gfx.h"\nint main(void) {\n  printf("%zu", sizeof(PcoGfxScanTask));\n'
                   + "".join(f'  printf(" %zu", offsetof(PcoGfxScanTask, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 48 == C.sizeof(G.ScanTask)
    assert got[1:] == [getattr(G.ScanTask, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert [n for n, _ in G.ScanTask._fields_] == FIELDS


def test_the_header_declares_the_entry_point_and_the_library_exports_it(lib):
    text = open(os.path.join(INCLUDE, "pco_gfx.h")).read()
    assert re.search(r"enum PcoError pco_gfx_scan_chunks\(size_t n_tasks, const PcoGfxScanTask\* tasks, PcoGfxTaskResult\* results,\s*PcoGfxTaskResult\* d_results, void\* stream\);", text)
    assert hasattr(lib, "pco_gfx_scan_chunks") and G.SIGNATURES["pco_gfx_scan_chunks"] == G.SIGNATURES["pco_gfx_decompress_chunks"]
    assert "files of many chunks without a directory, extending" not in text   # (section 4l's list of what is open)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
P = 0x1000   # (never dereferenced: every call below is refused by the argument checks)
GOOD = dict(src=P, src_len=100, d_offsets=P, d_counts=P, max_chunks=4, dtype=1, flags=1, reserved=0)
# in the order of the header's list; the message names the check that fired
CHECKS = [
    ("null src", dict(src=None), "null src"),
    ("null d_offsets", dict(d_offsets=None), "null src"),
    ("null d_counts", dict(d_counts=None), "null src"),
    ("max_chunks 0", dict(max_chunks=0), "max_chunks"),
    ("max_chunks 2^31", dict(max_chunks=1 << 31), "max_chunks"),
    ("max_chunks 2^32 - 1", dict(max_chunks=0xFFFFFFFF), "max_chunks"),
    ("dtype 0", dict(dtype=0), "number type"),
    ("dtype 12", dict(dtype=12), "number type"),
    ("reserved", dict(reserved=1), "reserved"),
    ("flag bit 1", dict(flags=2), "flag"),
    ("flag ONE_CHUNK", dict(flags=8 | 1), "flag"),
    ("flag bit 16", dict(flags=1 << 16), "flag"),
    ("flag bit 31", dict(flags=0x80000000), "flag"),
    ("d_offsets off by 4", dict(d_offsets=P + 4), "aligned"),
    ("d_offsets off by 1", dict(d_offsets=P + 1), "aligned"),
    ("d_counts off by 2", dict(d_counts=P + 2), "aligned"),
    ("d_counts off by 1", dict(d_counts=P + 1), "aligned"),
]


def call(lib, form="sync", task=None, no_tasks=False, no_results=False, n_tasks=1, second=None):
    kw = dict(GOOD); kw.update(task or {})
    arr = (G.ScanTask * 2)(G.ScanTask(**kw), G.ScanTask(**dict(GOOD, **(second or {}))))
    res = (G.TaskResult * 2)()
    for r in res:
        r.n_out, r.consumed, r.status, r.aux = 77, 78, 99, 98
    host, dev = (None if no_results else res, None) if form == "sync" else (None, None if no_results else P)
    code = lib.pco_gfx_scan_chunks(n_tasks, None if no_tasks else arr, host, dev, None)
    untouched = all((r.n_out, r.consumed, r.status, r.aux) == (77, 78, 99, 98) for r in res)
    return code, lib.pco_gfx_last_status(), (lib.pco_gfx_last_error() or b"").decode(), untouched


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("name,kw,word", CHECKS, ids=[c[0] for c in CHECKS])
def test_every_host_check_comes_before_a_device_is_asked_for(lib, name, kw, word, form):
    code, st, msg, untouched = call(lib, form, kw)
    assert code == G.PcoDecompressionError and st == INVALID and word in msg and "task 0" in msg and untouched
    # ... in the second task of two as well
    code, st, msg, untouched = call(lib, form, None, n_tasks=2, second=kw)
    assert code == G.PcoDecompressionError and st == INVALID and word in msg and "task 1" in msg and untouched


@pytest.mark.parametrize("form", ["sync", "async"])
def test_the_checks_fire_in_the_header_s_order(lib, form):
    order = [dict(src=None), dict(max_chunks=0), dict(dtype=0), dict(reserved=7), dict(flags=2), dict(d_offsets=P + 4)]
    words = ["null src", "max_chunks", "number type", "reserved", "flag", "aligned"]
    for i in range(len(order)):
        kw = {}
        for later in order[i:]:
            kw.update(later)
        code, st, msg, untouched = call(lib, form, kw)
        assert (code, st) == (G.PcoDecompressionError, INVALID) and words[i] in msg and untouched, (i, msg)
    # the two call-level checks in front of every task's: a null task array, then no results at all
    code, st, msg, untouched = call(lib, form, dict(src=None), no_tasks=True, no_results=True)
    assert st == INVALID and "null task array" in msg
    code, st, msg, untouched = call(lib, form, dict(src=None), no_results=True)
    assert st == INVALID and "both null" in msg
    # a bad first task is reported although the second is bad as well
    code, st, msg, untouched = call(lib, form, dict(reserved=1), n_tasks=2, second=dict(src=None))
    assert "task 0" in msg and "reserved" in msg


def test_flags_take_the_header_bit_and_a_version(lib):
    """(every one of these passes the checks and goes on to ask for a device: with one, the call would read P)"""
    if lib.pco_gfx_device_count() >= 1:
        return   # (with a device the call would run on P; tests/test_gpu_scan.py passes versions in flags there)
    for flags in (0, 1, 3 << 8, 1 | (4 << 8), 0xFF00, 0xFF01):
        code, st, msg, untouched = call(lib, "sync", dict(flags=flags))
        assert code == G.PcoDecompressionError and st == G.ST_DEVICE_ERROR and untouched, (flags, msg)


@pytest.mark.parametrize("form", ["sync", "async"])
def test_no_tasks_is_a_success_without_a_device(lib, form):
    assert call(lib, form, n_tasks=0)[0] == G.PcoSuccess and call(lib, form, n_tasks=0, no_tasks=True)[0] == G.PcoSuccess
    assert call(lib, form, n_tasks=0, no_results=True)[:2] == (G.PcoDecompressionError, INVALID)


# ---------------------------------------------------------------------------------------------------------------------------------------
# pco_scan.h compiled alone
# ---------------------------------------------------------------------------------------------------------------------------------------
PROBE = r'''
#include "%s/pco_scan.h"
using namespace pcogfx;
// out: status, format_major, uniform_type, len
extern "C" void header(const uint8_t* p, uint64_t len, uint64_t* out) {
  const ScanHeader h = scan_file_header(ScanBytes{p, len});
  out[0] = h.status; out[1] = h.format_major; out[2] = h.uniform_type; out[3] = h.len;
}
// out: status, kind, n
extern "C" void preamble(const uint8_t* p, uint64_t len, uint64_t pos, uint32_t dtype, uint32_t uniform_type, int end_ok, uint64_t* out) {
  const ScanPreamble r = scan_chunk_preamble(ScanBytes{p, len}, pos, dtype, uniform_type, end_ok != 0);
  out[0] = r.status; out[1] = r.kind; out[2] = r.n;
}
extern "C" void behind(const uint8_t* p, uint64_t len, uint64_t pos, int in_file, uint64_t* out) {
  const ScanBehind r = scan_behind_chunk(ScanBytes{p, len}, pos, in_file != 0);
  out[0] = r.status; out[1] = r.aux;
}
extern "C" uint32_t type_bits(uint32_t dtype) { return scan_type_bits(dtype); }
''' % CSRC


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("scan")
    src = d / "probe.cpp"; src.write_text(PROBE)
    out = d / "libprobe.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    lib.header.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]; lib.header.restype = None
    lib.preamble.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]; lib.preamble.restype = None
    lib.behind.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]; lib.behind.restype = None
    lib.type_bits.argtypes = [C.c_uint32]; lib.type_bits.restype = C.c_uint32

    def exact(data):   # a heap block of exactly the bytes (+ 1: an empty block)
        return (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")

    class Pr:
        type_bits = staticmethod(lib.type_bits)

        @staticmethod
        def header(data):
            o = (C.c_uint64 * 4)(); lib.header(exact(data), len(data), o)
            return tuple(int(x) for x in o)

        @staticmethod
        def preamble(data, pos, dtype, uniform=0, end_ok=False):
            o = (C.c_uint64 * 3)(); lib.preamble(exact(data), len(data), pos, dtype, uniform, int(end_ok), o)
            return tuple(int(x) for x in o)

        @staticmethod
        def behind(data, pos, in_file):
            o = (C.c_uint64 * 2)(); lib.behind(exact(data), len(data), pos, int(in_file), o)
            return tuple(int(x) for x in o)
    return Pr


def file_header(f):
    """(bytes in front of the first chunk, the format's major version) by the format's arithmetic (standalone/decompressor.rs:85-137)"""
    assert f[:4] == b"pco!"
    at = 4; sv = f[4]
    if sv >= 2:
        at = 5 + (1 if sv >= 3 else 0)
        at += (6 + 1 + (f[at] & 63) + 7) // 8
    major = f[at]
    return at + (2 if major >= 4 else 1), major


def test_the_type_table(probe):
    assert [probe.type_bits(d) for d in range(14)] == [0] + [G.DTYPE_BYTES[d] * 8 for d in range(1, 12)] + [0, 0]


def test_there_are_13_golden_files():
    assert len(ASSETS) == 13


@pytest.mark.parametrize("path", ASSETS, ids=[os.path.basename(p) for p in ASSETS])
def test_the_header_of_a_golden_file_is_what_the_oracle_s_reader_finds(probe, path):
    f = open(path, "rb").read()
    status, major, uniform, hlen = probe.header(f)
    assert status == OK and (hlen, major) == file_header(f)
    if f[hlen] == 0:   # a file without a chunk: the terminator alone
        assert probe.preamble(f, hlen, 1) == (OK, 1, 0) and hlen + 1 == len(f)
        return
    info, _ = O.inspect_first_chunk(f)
    assert (major, uniform) == (info.fmt_major, info.uniform_type)
    # the chunk start: the preamble there carries the oracle's type and count, and its ChunkMeta ends where the oracle's reader says, behind it
    assert probe.preamble(f, hlen, int(info.dtype), uniform) == (OK, 0, int(info.n)) and hlen + 4 < int(info.meta_end_byte)
    assert probe.preamble(f, hlen, int(info.dtype) % 11 + 1) == (CORRUPTION, 0, 0)
    # cut after every byte of the header: the table's verdicts -- INSUFFICIENT_DATA until the header is whole
    for cut in range(hlen):
        assert probe.header(f[:cut])[0] == INSUFFICIENT, cut
    assert probe.header(f[:hlen]) == (OK, major, uniform, hlen)
    for cut in range(hlen, hlen + 4):   # ... and of the preamble
        assert probe.preamble(f[:cut], hlen, int(info.dtype), uniform)[0] == INSUFFICIENT, cut
        assert probe.preamble(f[:cut], hlen, int(info.dtype), uniform, end_ok=True)[:2] == ((OK, 2) if cut == hlen else (INSUFFICIENT, 0))


def header_bytes(sv=3, uniform=0, n_hint=1000, major=4, minor=1):
    out = bytearray(b"pco!")
    if sv >= 2:
        out.append(sv)
        if sv >= 3:
            out.append(uniform)
        bits = max(int(n_hint).bit_length(), 1)
        v = (bits - 1) | (n_hint << 6); nb = (6 + bits + 7) // 8
        out += v.to_bytes(nb, "little")
    out.append(major)
    if major >= 4:
        out.append(minor)
    return bytes(out)


def test_every_row_of_the_header_s_table(probe):
    good = header_bytes()
    assert probe.header(good) == (OK, 4, 0, len(good)) and probe.header(good + b"\x01\x02") == (OK, 4, 0, len(good))
    assert [probe.header(good[:k])[0] for k in range(4)] == [INSUFFICIENT] * 4                 # fewer than 4 bytes
    assert probe.header(b"pco?" + good[4:])[0] == CORRUPTION and probe.header(b"pco?")[0] == CORRUPTION   # the magic, as soon as it is there
    assert probe.header(b"pc")[0] == INSUFFICIENT
    for sv in (0, 1):                                                                          # no standalone version byte: byte 4 is the major version
        assert probe.header(b"pco!" + bytes([sv])) == (OK, sv, 0, 5)
    assert probe.header(b"pco!")[0] == INSUFFICIENT
    v2 = header_bytes(sv=2, major=2)
    assert probe.header(v2) == (OK, 2, 0, len(v2))
    for u in range(1, 12):                                                                     # the uniform type
        h = header_bytes(uniform=u)
        assert probe.header(h) == (OK, 4, u, len(h))
    for u in (12, 200, 255):
        assert probe.header(header_bytes(uniform=u))[0] == CORRUPTION
        assert probe.header(header_bytes(uniform=u)[:6])[0] == CORRUPTION                      # ... in front of the varint's verdicts
    for n_hint in (0, 1, 3, 255, 1 << 20, (1 << 58) - 1, (1 << 64) - 1):                       # the varint: 7 .. 70 bits
        h = header_bytes(n_hint=n_hint)
        assert probe.header(h) == (OK, 4, 0, len(h)), n_hint
        for cut in range(len(h)):
            assert probe.header(h[:cut])[0] == INSUFFICIENT, (n_hint, cut)
    pad = bytearray(header_bytes(n_hint=1000)); assert len(pad) == 10                           # 6 + 10 bits: no padding; 6 + 3 bits: 7 bits of it
    pad = bytearray(header_bytes(n_hint=5)); pad[7] |= 0x80
    assert probe.header(bytes(pad))[0] == CORRUPTION and probe.header(bytes(pad[:8]))[0] == CORRUPTION
    assert probe.header(bytes(pad[:7]))[0] == INSUFFICIENT                                     # the padded byte is not there: the file ends inside the varint
    assert probe.header(header_bytes(sv=4))[0] == CORRUPTION and probe.header(header_bytes(sv=200))[0] == CORRUPTION
    assert probe.header(header_bytes(sv=4)[:7])[0] == INSUFFICIENT                             # ... behind the varint's verdicts
    for major in (5, 9, 255):
        assert probe.header(header_bytes(major=major))[0] == CORRUPTION
        assert probe.header(header_bytes(major=major)[:-1])[0] == CORRUPTION                   # the major version alone says so
    for major in (0, 1, 2, 3):
        h = header_bytes(major=major)
        assert probe.header(h) == (OK, major, 0, len(h))
    assert probe.header(good[:-1])[0] == INSUFFICIENT                                          # major 4 without its minor version


def test_the_preamble_and_what_stands_behind_a_chunk(probe):
    data = b"\xEE" * 3 + bytes([5, 0x2B, 0x01, 0x00]) + b"\x07"
    assert probe.preamble(data, 3, 5) == (OK, 0, 300) and probe.preamble(data, 3, 5, uniform=5) == (OK, 0, 300)
    assert probe.preamble(data, 3, 1)[0] == CORRUPTION and probe.preamble(data, 3, 5, uniform=1)[0] == CORRUPTION
    assert probe.preamble(b"\xEE" * 3 + b"\x05\xff\xff\xff", 3, 5) == (OK, 0, 1 << 24)
    assert probe.preamble(b"\xEE" * 3 + b"\0", 3, 5) == (OK, 1, 0) and probe.preamble(b"\xEE" * 3 + b"\0", 3, 5, end_ok=True) == (OK, 1, 0)
    assert probe.preamble(b"\xEE" * 3, 3, 5) == (INSUFFICIENT, 0, 0) and probe.preamble(b"\xEE" * 3, 3, 5, end_ok=True) == (OK, 2, 0)
    assert probe.preamble(b"\xEE" * 3 + b"\x01", 3, 5)[0] == CORRUPTION                        # the type byte is judged before the count is asked for
    for k in (1, 2, 3):
        assert probe.preamble(data[: 3 + k], 3, 5) == (INSUFFICIENT, 0, probe.preamble(data[: 3 + k], 3, 5)[2])
    assert probe.behind(data, 7, True) == (OK, 1) and probe.behind(data, 7, False) == (OK, 1)
    assert probe.behind(data[:7] + b"\0", 7, True) == (OK, 2)
    assert probe.behind(data[:7], 7, True) == (INSUFFICIENT, 0) and probe.behind(data[:7], 7, False) == (OK, 0)


def test_a_sanitised_stand_alone_program_reads_nothing_beyond_any_cut(tmp_path):
    """g++ -fsanitize=address,undefined over a program with its own main: every golden file's first 64 bytes cut after every byte into a heap block
    of exactly that many bytes, through the three functions"""
    data = tmp_path / "heads.bin"
    with open(data, "wb") as f:
        for p in ASSETS:
            f.write(open(p, "rb").read()[:64].ljust(64, b"\x55"))
    src = tmp_path / "main.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "%s/pco_scan.h"
using namespace pcogfx;
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  uint8_t head[64]; long runs = 0, ok = 0;
  while (fread(head, 1, 64, f) == 64)
    for (uint64_t cut = 0; cut <= 64; cut++) {
      uint8_t* p = (uint8_t*)malloc(cut + 1); memcpy(p, head, cut);
      const ScanBytes b{p, cut};
      const ScanHeader h = scan_file_header(b);
      if (h.status == kScanOk) { ok++; if (h.len > cut) return 3; }
      for (uint64_t pos = 0; pos <= cut + 1; pos++) { (void)scan_chunk_preamble(b, pos, 1, 0, pos & 1); (void)scan_behind_chunk(b, pos, pos & 1); }
      free(p); runs++;
    }
  printf("%%ld cuts, %%ld whole headers\n", runs, ok);
  return runs == 13 * 65 && ok > 13 * 40 ? 0 : 4;
}
''' % CSRC)
    exe = tmp_path / "main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(src)])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------------------------------------
# pcodec_amd.paged: the task lists of scan_files and decompress_files, field for field
# ---------------------------------------------------------------------------------------------------------------------------------------
class Tensor(U.FakeTensor):
    def copy_(self, other, non_blocking=False):
        self.copied_from = other
        return self

    def __getitem__(self, key):
        t = super().__getitem__(key)
        return Tensor(t._addr, t.shape, t.dtype)

    def view(self, dtype):
        t = super().view(dtype)
        return Tensor(t._addr, t.shape, t.dtype)


class Torch(U.FakeTorch):
    def __init__(self):
        super().__init__()
        self.adds = []

    def _alloc(self, shape, dtype=None, device=None):
        t = super()._alloc(shape, dtype, device)
        return Tensor(t._addr, t.shape, t.dtype)

    empty = zeros = _alloc

    def frombuffer(self, buf, dtype=None):
        return ("host", len(buf))

    def add(self, t, scalar, out=None):
        self.adds.append((t.data_ptr(), t.shape[0], scalar, out.data_ptr(), out.shape[0]))


class Lib(U.FakeLib):
    DIR_FORMS = U.FakeLib.DIR_FORMS + ("pco_gfx_decompress_chunks_dir",)


FILES = [b"\x11" * 1000, b"\x22" * 77, b"\x33" * 8]
NAMES = ["uint32", "float16", "int64"]


@pytest.fixture()
def stand_ins(monkeypatch, lib):
    from pcodec_amd import paged
    real_torch = sys.modules.get("torch")
    torch = sys.modules["torch"] = Torch()
    fake = Lib(G)
    monkeypatch.setattr(paged, "_require_device", lambda: fake)
    try:
        yield paged, fake, torch
    finally:
        if real_torch is None:
            sys.modules.pop("torch", None)
        else:
            sys.modules["torch"] = real_torch


def rows_of(struct, call_):
    return [dict(zip([n for n, _ in struct._fields_], t)) for t in call_["tasks"]]


def test_scan_files_async_is_one_call_over_one_staged_blob(stand_ins):
    paged, fake, torch = stand_ins
    s = paged.scan_files_async(FILES, NAMES)
    (d,) = fake.calls
    assert d["fn"] == "pco_gfx_scan_chunks" and d["n_tasks"] == 3 and d["args"] == [None, s.results.data_ptr(), U.STREAM_HANDLE]
    t = rows_of(G.ScanTask, d)
    bases = [0, 1072, 1216]   # each file behind 64 bytes of slack, on a 16-byte grid
    caps = [126, 10, 2]       # a chunk takes 8 bytes at the least
    assert s.bases == bases and s.lens == [1000, 77, 8]
    assert [(x["src"], x["src_len"], x["max_chunks"], x["dtype"], x["flags"], x["reserved"]) for x in t] == \
        [(s.blob.data_ptr() + b, n, c, G.DTYPE_BYTE[nm], G.TASK_HAS_FILE_HEADER, 0) for b, n, c, nm in zip(bases, s.lens, caps, NAMES)]
    assert s.blob.numel() >= bases[2] + 8 + 64
    assert [x["d_offsets"] for x in t] == [o.data_ptr() for o in s.offsets] and [o.shape[0] for o in s.offsets] == [c + 1 for c in caps]
    assert [x["d_counts"] for x in t] == [c.data_ptr() for c in s.counts] and [c.shape[0] for c in s.counts] == caps
    assert all(x["d_offsets"] % 8 == 0 and x["d_counts"] % 4 == 0 for x in t)
    # the arrays do not overlap, and the counts lie behind the results in ONE tensor: one read-back
    assert t[0]["d_offsets"] + 8 * 127 == t[1]["d_offsets"] and t[1]["d_offsets"] + 8 * 11 == t[2]["d_offsets"]
    assert t[0]["d_counts"] == s.results.data_ptr() + 3 * 24 and t[1]["d_counts"] == t[0]["d_counts"] + 4 * 126
    fake.calls.clear()
    s = paged.scan_files_async(FILES, "uint16", max_chunks=5)
    t = rows_of(G.ScanTask, fake.calls[0])
    assert [(x["max_chunks"], x["dtype"]) for x in t] == [(5, 7)] * 3
    with pytest.raises(TypeError):
        paged.scan_files_async(FILES, ["uint32"])


def fake_read_back(monkeypatch, paged, n_chunks, counts, caps, versions, status=None):
    """what the device would hold behind a scan: results, then every file's counts at its place"""
    k = len(n_chunks)
    res = np.zeros(k, paged.RESULT_DT)
    res["n_out"] = n_chunks; res["consumed"] = [100 + i for i in range(k)]; res["aux"] = [2 | (v << 8) for v in versions]
    if status is not None:
        res["status"] = status
    ns = np.full(sum(caps), 0xA5A5A5A5, np.uint32); at = 0
    for c, cap in zip(counts, caps):
        ns[at: at + len(c)] = c; at += cap
    monkeypatch.setattr(paged, "_to_host", lambda t: np.concatenate([res.view(np.uint8), ns.view(np.uint8)]))


def test_scan_files_reads_back_once_and_trims(stand_ins, monkeypatch):
    paged, fake, torch = stand_ins
    fake_read_back(monkeypatch, paged, [3, 1, 0], [[300, 256, 1], [77], []], [126, 10, 2], [4, 2, 4])
    out = paged.scan_files(FILES, NAMES)
    assert [(f.n_chunks, f.version, f.ns, f.consumed) for f in out] == [(3, 4, [300, 256, 1], 100), (1, 2, [77], 101), (0, 4, [], 102)]
    assert [(f.offsets.shape[0], f.counts.shape[0]) for f in out] == [(4, 3), (2, 1), (1, 0)]
    t = rows_of(G.ScanTask, fake.calls[0])
    assert [f.offsets.data_ptr() for f in out] == [x["d_offsets"] for x in t] and [f.counts.data_ptr() for f in out] == [x["d_counts"] for x in t]
    fake_read_back(monkeypatch, paged, [3, 1, 0], [[300, 256, 1], [77], []], [126, 10, 2], [4, 2, 4], status=[0, CORRUPTION, 0])
    with pytest.raises(G.PcoGfxError) as e:
        paged.scan_files(FILES, NAMES)
    assert e.value.status == CORRUPTION and "file 1" in str(e.value)


def test_decompress_files_is_the_scan_and_one_directory_call(stand_ins, monkeypatch):
    paged, fake, torch = stand_ins
    fake_read_back(monkeypatch, paged, [3, 1, 0], [[300, 256, 1], [77], []], [126, 10, 2], [4, 2, 4])
    outs = paged.decompress_files(FILES, NAMES)
    scan, dec = fake.calls
    assert scan["fn"] == "pco_gfx_scan_chunks" and dec["fn"] == "pco_gfx_decompress_chunks_dir"
    st = rows_of(G.ScanTask, scan)
    # the directory: the staged blob, and the files' offsets moved by their bases into ONE array -- file i's n + 1 entries behind file i - 1's
    blob = st[0]["src"]
    adds = torch.adds
    assert [(a[0], a[1], a[2], a[4]) for a in adds] == [(st[0]["d_offsets"], 4, 0, 4), (st[1]["d_offsets"], 2, 1072, 2), (st[2]["d_offsets"], 1, 1216, 1)]
    combined = adds[0][3]
    assert [a[3] for a in adds] == [combined, combined + 8 * 4, combined + 8 * 6]
    assert dec["n_tasks"] == 4
    d_blob, blob_len, d_offsets, n_pieces, gap, reserved = dec["dir"]
    assert (d_blob, d_offsets, n_pieces, gap, reserved) == (blob, combined, 6, 0, 0) and blob_len >= 1216 + 8
    assert dec["args"] == ["host", None, U.STREAM_HANDLE]
    t = rows_of(G.DirChunkTask, dec)
    assert [(x["page_n"], x["meta_piece"], x["page_piece"], x["dtype"], x["format_major"]) for x in t] == [(300, 0, 0, 1, 4), (256, 1, 1, 1, 4), (1, 2, 2, 1, 4), (77, 4, 4, 9, 2)]
    assert [o.shape[0] for o in outs] == [557, 77, 0] and [o.dtype.name for o in outs] == NAMES
    assert [x["dst"] for x in t] == [outs[0].data_ptr(), outs[0].data_ptr() + 1200, outs[0].data_ptr() + 1200 + 1024, outs[1].data_ptr()]
