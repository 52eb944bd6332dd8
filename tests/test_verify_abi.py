"""Verified encodes (include/pco_gfx.h section 3b) without a device: the verdict of pcodec_amd/csrc/pco_verify.h compiled on its own with g++
(the same lines verify_finish_kernel runs per task) against a table written out by hand -- once as a shared object, once as a stand-alone program
under AddressSanitizer and UBSan --, the constants of the header and of the binding, the flag through make_config and ChunkConfig, the host checks
of pco_gfx_verify_chunks / pco_gfx_verify_wrapped_chunks (made before a device is asked for), and, for every damaged chunk tests/test_gpu_verify.py
uses, the ORACLE's decode of the damaged bytes against the outcome that test expects."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gpu_util as U  # noqa: E402
import oracle_lib as O  # noqa: E402
import verify_util as V  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd.config import ChunkConfig  # noqa: E402

HEADER = os.path.join(HERE, "..", "include", "pco_gfx.h")
CSRC = os.path.abspath(os.path.join(HERE, "..", "pcodec_amd", "csrc"))
ONES = (1 << 64) - 1
OK, CORRUPTION, INSUFFICIENT, INVALID, UNSUPPORTED = G.ST_OK, G.ST_CORRUPTION, G.ST_INSUFFICIENT_DATA, G.ST_INVALID_ARGUMENT, G.ST_UNSUPPORTED

# ---------------------------------------------------------------------------------------------------------------------------------------
# verify_verdict against a table: one row per combination of the encode's status, the decode's status, n_out below / equal to / above n, and the
# first-difference word ~0 / 0 / n - 1 / at or behind the decoded count.  The encode result is {n_out 4321, consumed 0, status, aux}; n = 100.
# ---------------------------------------------------------------------------------------------------------------------------------------
N = 100
ENC_N_OUT = 4321


def expected(enc_status, enc_aux, dec_status, dec_n_out, first):
    """{n_out, consumed, status, aux}, written out case by case from include/pco_gfx.h section 3b (no arithmetic shared with the header under test)"""
    if enc_status != OK:                      # not encoded: untouched, whatever the decode and the compare left
        return (ENC_N_OUT, 0, enc_status, enc_aux)
    bad_aux = enc_aux & 1                     # a failed verdict keeps bit 0 and lacks bit 1
    if dec_status != OK:                      # the decode did not end OK
        return (0, ONES, CORRUPTION, bad_aux)
    if dec_n_out == 99:                       # one number short: 99 were compared
        if first in (0,):
            return (0, 0, CORRUPTION, bad_aux)
        return (0, 99, CORRUPTION, bad_aux)   # first = ~0, or 99 and 100: nothing that was compared differs -> the decoded count
    if dec_n_out == 101:                      # one number too many: 100 were compared
        if first in (0, 99):
            return (0, first, CORRUPTION, bad_aux)
        return (0, 100, CORRUPTION, bad_aux)
    assert dec_n_out == 100
    if first in (0, 99):
        return (0, first, CORRUPTION, bad_aux)
    return (ENC_N_OUT, 0, OK, enc_aux | 2)    # first = ~0, or 100: no number of the hundred differs


def table():
    rows = []
    for enc_status, enc_aux, dec_status, dec_n_out in itertools.product((OK, INVALID, INSUFFICIENT), (0, 1, 2, 3), (OK, CORRUPTION, INSUFFICIENT, INVALID, UNSUPPORTED),
                                                                        (99, 100, 101)):
        for first in (ONES, 0, N - 1, dec_n_out if dec_n_out < N else N):
            rows.append(((enc_status, enc_aux, dec_status, dec_n_out, first), expected(enc_status, enc_aux, dec_status, dec_n_out, first)))
    return rows


VERDICT_CPP = '''
#include "%s/pco_verify.h"
extern "C" void verdict(uint32_t enc_status, uint32_t enc_aux, uint32_t dec_status, uint64_t dec_n_out, uint64_t first, uint64_t n, uint64_t* out) {
  const pcogfx::VerifyResult v = pcogfx::verify_verdict(pcogfx::VerifyResult{%d, 0, enc_status, enc_aux}, dec_status, dec_n_out, n, first);
  out[0] = v.n_out; out[1] = v.consumed; out[2] = v.status; out[3] = v.aux;
}
''' % (CSRC, ENC_N_OUT)


def test_the_verdict_compiled_alone_gives_the_table(tmp_path):
    src = tmp_path / "verdict.cpp"
    src.write_text(VERDICT_CPP)
    out = tmp_path / "libverdict.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    lib.verdict.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.verdict.restype = None
    got = (C.c_uint64 * 4)()
    rows = table()
    assert len(rows) == 3 * 4 * 5 * 3 * 4
    for args, want in rows:
        lib.verdict(*args, N, got)
        assert tuple(got) == want, (args, tuple(got), want)


def test_the_verdict_runs_clean_under_the_sanitizers_in_a_program_of_its_own(tmp_path):
    rows = table()
    body = "\n".join("  {%du, %du, %du, %dull, %dull, %dull, %dull, %du, %du}," % (*args, *want) for args, want in rows)
    src = tmp_path / "verdict_main.cpp"
    src.write_text(VERDICT_CPP + '''
#include <cstdio>
struct Row { uint32_t enc_status, enc_aux, dec_status; uint64_t dec_n_out, first, n_out, consumed; uint32_t status, aux; };
static const Row kRows[] = {
%s
};
int main() {
  int bad = 0;
  for (const Row& r : kRows) {
    uint64_t out[4];
    verdict(r.enc_status, r.enc_aux, r.dec_status, r.dec_n_out, r.first, %d, out);
    if (out[0] != r.n_out || out[1] != r.consumed || out[2] != r.status || out[3] != r.aux) bad++;
  }
  std::printf("%%zu rows, %%d bad\\n", sizeof(kRows) / sizeof(kRows[0]), bad);
  return bad != 0;
}
''' % (body, N))
    exe = tmp_path / "verdict_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "%d rows, 0 bad" % len(rows) and run.stderr == ""


# ---------------------------------------------------------------------------------------------------------------------------------------
# constants, the flag, the host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_header_and_the_binding_agree_on_the_constants():
    text = open(HEADER).read()
    assert int(re.search(r"#define PCO_GFX_CFG_VERIFY (\d+)u", text).group(1)) == G.CFG_VERIFY == 8
    assert int(re.search(r"#define PCO_GFX_AUX_VERIFIED (\d+)u", text).group(1)) == G.AUX_VERIFIED == 2
    assert G.CFG_VERIFY not in (G.CFG_STRICT_HISTOGRAM, G.CFG_CONV1, G.CFG_DICT)
    assert re.search(r"enum PcoError pco_gfx_verify_chunks\(size_t n_tasks, const PcoGfxEncodeTask\* tasks, const PcoGfxTaskResult\* d_encoded, PcoGfxTaskResult\* results,", text)
    assert re.search(r"enum PcoError pco_gfx_verify_wrapped_chunks\(size_t n_tasks, const PcoGfxWrappedTask\* tasks, const PcoChunkConfigEx\* config, const PcoGfxPageInfo\* d_encoded,", text)
    assert hasattr(G.lib(), "pco_gfx_verify_chunks") and hasattr(G.lib(), "pco_gfx_verify_wrapped_chunks")


def compress_with_flags(flags):
    """pco_gfx_simple_compress_into_ex on real host buffers: the config is validated first, a device is asked for behind that: (code, status)"""
    L = G.lib()
    cfg = G.make_config(mode=1, delta=1); cfg.flags = flags
    nums = np.arange(100, dtype=np.uint32)
    cap = L.pco_gfx_guarantee_file_size(nums.size, G.DTYPE_BYTE["uint32"], 0) + 64
    dst = np.zeros(cap, np.uint8); n = C.c_size_t(0)
    code = L.pco_gfx_simple_compress_into_ex(nums.ctypes.data_as(C.c_void_p), nums.size, G.DTYPE_BYTE["uint32"], C.byref(cfg), 0, dst.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return code, L.pco_gfx_last_status()


def test_the_flag_is_known_and_its_neighbours_are_not():
    assert G.make_config(verify=True).flags == 8 and G.make_config().flags == 0
    # accepted: the call gets as far as asking for a device (and, where there is one, succeeds)
    accepted = (G.PcoSuccess, G.ST_OK) if G.lib().pco_gfx_device_count() > 0 else (G.PcoCompressionError, G.ST_DEVICE_ERROR)
    assert compress_with_flags(8) == accepted
    assert compress_with_flags(8 | 1) == accepted
    for flags in (16, 0x80, 1 << 9, 8 | 16):
        assert compress_with_flags(flags) == (G.PcoCompressionError, G.ST_INVALID_ARGUMENT), flags


def test_unknown_flags_are_refused_by_the_config_check_itself():
    # (the check that refuses a flag needs no device either way: the wrapped capacity of a refused config is 0)
    L = G.lib()
    for flags, known in ((8, True), (16, False), (0x80, False), (1 << 9, False), (8 | 16, False)):
        cfg = G.make_config(mode=1, delta=1); cfg.flags = flags
        infos = (G.PageInfo * 4)()
        task = (G.WrappedTask * 1)(G.WrappedTask(0x1000, 10, 0x2000, 1 << 20, G.DTYPE_BYTE["uint32"], 0, None))
        code = L.pco_gfx_wrapped_scratch_estimate(1, task, C.byref(cfg))
        assert (code != 0) == known, flags
        if not known:
            assert L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT


def test_chunk_config_carries_the_flag():
    assert ChunkConfig(verify=True).to_c().flags & G.CFG_VERIFY
    assert not ChunkConfig().to_c().flags & G.CFG_VERIFY
    assert ChunkConfig(verify=True, enable_dict=True).to_c().flags == G.CFG_VERIFY | G.CFG_DICT


P = 0x1000   # (never dereferenced: every call below is refused by the argument checks)
GOOD = dict(src=P, n=10, dst=P, dst_cap=4096, dtype=1)
CHECKS = [
    dict(no_tasks=True),
    dict(no_encoded=True),
    dict(no_results=True),
    dict(task=dict(n=0)),
    dict(task=dict(n=(1 << 24) + 1)),
    dict(task=dict(dtype=0)),
    dict(task=dict(dtype=12)),
    dict(task=dict(dst_cap=15)),
    dict(task=dict(dst_cap=0)),
    dict(task=dict(src=None)),
    dict(task=dict(dst=None)),
    dict(task=dict(src=P + 1, dtype=1)),             # a u32 source on an odd address
    dict(task=dict(src=P + 4, dtype=2)),             # a u64 source aligned to 4
]
WRAPPED_CHECKS = [
    dict(task=dict(n_pages=2)),                      # page_sizes == NULL with n_pages != 0
    dict(pages=[4, 5]),                              # the sizes do not sum to n
    dict(pages=[10, 0]),                             # a page of 0 numbers
]


def verify_call(wrapped, task=None, pages=None, no_tasks=False, no_encoded=False, no_results=False, n_tasks=1):
    L = G.lib()
    kw = dict(GOOD); kw.update(task or {})
    keep = None
    if wrapped:
        kw.setdefault("n_pages", 0); kw.setdefault("page_sizes", None)
        if pages is not None:
            keep = (C.c_uint64 * len(pages))(*pages); kw["n_pages"] = len(pages); kw["page_sizes"] = C.cast(keep, C.c_void_p)
        arr = (G.WrappedTask * 1)(G.WrappedTask(**kw))
        res = (G.PageInfo * 8)()
        for r in res:
            r.offset, r.len, r.n, r.status, r.aux = 71, 72, 73, 99, 98
        cfg = G.make_config()
        code = L.pco_gfx_verify_wrapped_chunks(n_tasks, None if no_tasks else arr, C.byref(cfg), None if no_encoded else P, None if no_results else res, None, None)
        return code, L.pco_gfx_last_status(), [(r.offset, r.len, r.n, r.status, r.aux) for r in res]
    arr = (G.EncodeTask * 1)(G.EncodeTask(kw["src"], kw["n"], kw["dst"], kw["dst_cap"], kw["dtype"], 0))
    res = (G.TaskResult * 1)(); res[0].n_out, res[0].consumed, res[0].status, res[0].aux = 77, 78, 99, 98
    code = L.pco_gfx_verify_chunks(n_tasks, None if no_tasks else arr, None if no_encoded else P, None if no_results else res, None, None)
    return code, L.pco_gfx_last_status(), [(res[0].n_out, res[0].consumed, res[0].status, res[0].aux)]


@pytest.mark.parametrize("wrapped,kw", [(False, kw) for kw in CHECKS] + [(True, kw) for kw in CHECKS + WRAPPED_CHECKS])
def test_host_checks_come_before_a_device_is_asked_for(wrapped, kw):
    code, status, res = verify_call(wrapped, **kw)
    assert code == G.PcoCompressionError and status == G.ST_INVALID_ARGUMENT   # (without a device a check that came too late would say DEVICE_ERROR)
    assert all(r == ((71, 72, 73, 99, 98) if wrapped else (77, 78, 99, 98)) for r in res)   # nothing was written


@pytest.mark.parametrize("wrapped", [False, True])
def test_no_tasks_is_a_success_without_a_device(wrapped):
    code, status, _ = verify_call(wrapped, n_tasks=0)
    assert code == G.PcoSuccess
    code, status, _ = verify_call(wrapped, n_tasks=0, no_tasks=True)
    assert code == G.PcoSuccess
    code, status, _ = verify_call(wrapped, n_tasks=0, no_encoded=True)     # the array checks hold for an empty call too
    assert (code, status) == (G.PcoCompressionError, G.ST_INVALID_ARGUMENT)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the damaged chunks of the GPU test, decoded by the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk():
    a = V.numbers()
    return a, U.oracle_chunk(a, O.make_config(**V.SPEC))


def test_the_undamaged_chunk_is_offsets_back_to_back(chunk):
    a, c = chunk
    assert np.array_equal(O.simple_decompress(V.standalone_file(c, V.N), np.uint32, V.N), a)
    assert np.array_equal(np.frombuffer(c[len(c) - 2 * V.N:], "<u2"), a.astype(np.uint16))   # (one bin from 0, 16-bit offsets, no tANS bits)
    assert c[4] & 15 == 0   # the ChunkMeta starts behind the 4-byte preamble with the mode nibble: Classic


@pytest.mark.parametrize("name", sorted(V.STANDALONE_CASES))
def test_the_oracle_decodes_each_damaged_standalone_chunk_to_the_expected_outcome(chunk, name):
    a, c = chunk
    damage, want = V.STANDALONE_CASES[name]
    bad = damage(c)
    assert bad != c and len(bad) == len(c)
    try:
        got = V.outcome(O.simple_decompress(V.standalone_file(bad, V.N), np.uint32, V.N), a)
    except O.OracleError:
        got = ("fails",)
    assert got == want


@pytest.fixture(scope="module")
def wrapped_chunk():
    a = V.numbers()
    meta, pages, ns = O.wrapped_compress(a, O.make_config(**V.SPEC), exact_pages=V.PAGES)
    assert ns == V.PAGES
    return a, meta, pages


@pytest.mark.parametrize("name", sorted(V.WRAPPED_CASES))
def test_the_oracle_decodes_each_damaged_wrapped_chunk_to_the_expected_outcome(wrapped_chunk, name):
    a, meta, pages = wrapped_chunk
    piece, damage, want = V.WRAPPED_CASES[name]
    starts = np.concatenate([[0], np.cumsum(V.PAGES)])
    pieces = [meta] + list(pages)
    bad = damage(pieces[piece])
    assert bad != pieces[piece] and len(bad) == len(pieces[piece])
    pieces[piece] = bad
    for p in range(len(V.PAGES)):
        rows = a[starts[p]: starts[p + 1]]
        try:
            got_rows, err, in_meta = O.wrapped_page_prefix(pieces[0], pieces[1 + p], np.uint32, V.PAGES[p])
            got = ("fails",) if err else V.outcome(got_rows, rows)
        except O.OracleError:   # (a ChunkMeta the oracle refuses outright)
            got = ("fails",)
        if piece == 0 or piece == 1 + p:
            assert got == want, (p, got)
        else:
            assert got == ("equal",), (p, got)
