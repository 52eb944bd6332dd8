"""CPU: per-chunk specs (include/pco_gfx.h section 3c) without a device -- PcoGfxChunkSpec against the header and a g++ offsetof probe; every host
refusal of pco_gfx_compress_chunks_specs / pco_gfx_compress_wrapped_chunks_specs / pco_gfx_resolve_chunk_specs in the documented order, each beside
the same call made good (which then gets as far as asking for a device); pco_gfx_resolve_chunk_specs under every explicit (mode, delta) x number type
against a table written out by hand; pco_gfx_chunk_spec_from_meta against the oracle's ChunkMeta of Auto-encoded chunks and of the golden assets;
the specs= keyword of pcodec_amd.paged; and the recipes tests/test_gpu_chunk_specs.py relies on, resolved by the oracle."""
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

import chunk_specs_util as S  # noqa: E402
import oracle_lib as O  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import ChunkConfig, DeltaSpec, ModeSpec, paged  # noqa: E402

HEADER = os.path.abspath(os.path.join(HERE, "..", "include", "pco_gfx.h"))
ASSETS = sorted(glob.glob(os.path.join(HERE, "golden", "ref_assets", "*.pco")))
FIELDS = ["mode_kind", "delta_kind", "delta_order", "mode_k", "mode_base", "mode_inv", "reserved"]
INVALID, UNSUPPORTED, DEVICE = G.ST_INVALID_ARGUMENT, G.ST_UNSUPPORTED, G.ST_DEVICE_ERROR
U32, U64, I32, I64, F32, F64, U16, I16, F16, U8, I8 = range(1, 12)
NP = {t.byte: np.dtype(t.name) for t in G.NUMBER_TYPES}


def no_device():
    return G.lib().pco_gfx_device_count() < 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# the struct and the exports
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_lays_the_spec_out_as_the_header_does(tmp_path):
    text = open(HEADER).read()
    body = re.search(r"typedef struct PcoGfxChunkSpec \{(.*?)\} PcoGfxChunkSpec;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(uint32_t|uint64_t)\s+(\w+);", body)
    assert [n for _, n in decl] == FIELDS
    assert [(n, {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}[t]) for t, n in decl] == list(G.ChunkSpec._fields_)
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "%s"\nint main() { printf("%%zu", sizeof(PcoGfxChunkSpec));\n%s\nreturn 0; }\n' % (
        HEADER, "\n".join('printf(" %%zu", offsetof(PcoGfxChunkSpec, %s));' % f for f in FIELDS)))
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    size, *offsets = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert size == C.sizeof(G.ChunkSpec) == 40
    assert offsets == [getattr(G.ChunkSpec, n).offset for n in FIELDS] == [0, 4, 8, 12, 16, 24, 32]


def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    text = open(HEADER).read()
    for name in ("pco_gfx_resolve_chunk_specs", "pco_gfx_chunk_spec_from_meta", "pco_gfx_compress_chunks_specs", "pco_gfx_compress_wrapped_chunks_specs"):
        assert re.search(r"enum PcoError %s\(" % name, text), name
        assert hasattr(G.lib(), name) and name in G.SIGNATURES
    assert " * 3c. " in text and text.index(" * 3b. ") < text.index(" * 3c. ") < text.index(" * 4. Wrapped surface")


# ---------------------------------------------------------------------------------------------------------------------------------------
# host refusals of the two encode entry points, in the header's order
# ---------------------------------------------------------------------------------------------------------------------------------------
FILL = 0xAB


def call(wrapped, dtypes, specs, cfg="default", tasks_null=False, specs_null=False, out_null=False):
    """One call of two fake-pointer tasks (nothing is dereferenced before a device is asked for).  Returns (code, status, message, results untouched)."""
    L = G.lib()
    k = len(dtypes)
    if wrapped:
        tasks = (G.WrappedTask * k)(*[G.WrappedTask(0x10000 * (i + 1), 100, 0x2000000 * (i + 1), 1 << 20, dt, 0, None) for i, dt in enumerate(dtypes)])
        out = (G.PageInfo * (2 * k))()
    else:
        tasks = (G.EncodeTask * k)(*[G.EncodeTask(0x10000 * (i + 1), 100, 0x2000000 * (i + 1), 1 << 20, dt, 0) for i, dt in enumerate(dtypes)])
        out = (G.TaskResult * k)()
    C.memset(out, FILL, C.sizeof(out))
    c = G.make_config(enable_8_bit=True) if cfg == "default" else cfg
    f = L.pco_gfx_compress_wrapped_chunks_specs if wrapped else L.pco_gfx_compress_chunks_specs
    code = f(k, None if tasks_null else tasks, C.byref(c) if c is not None else None, None if specs_null else S.spec_array(specs), None if out_null else out, None, None)
    return code, L.pco_gfx_last_status(), (L.pco_gfx_last_error() or b"").decode(), bytes(out) == bytes([FILL]) * C.sizeof(out)


GOOD = S.spec()
F32_ONE = S.float_bits(1.0, np.float32)
# (what is wrong, the dtypes, the specs, keyword arguments, a word of the message).  Rows are in the header's order; task 1 carries the bad spec.
REFUSALS = [
    ("null tasks", [U32, U32], [GOOD, GOOD], dict(tasks_null=True), "null tasks"),
    ("null specs", [U32, U32], [GOOD, GOOD], dict(specs_null=True), "null specs"),
    ("config mode not Auto", [U32, U32], [GOOD, GOOD], dict(cfg=G.make_config(mode=G.MODE_CLASSIC)), "must be Auto"),
    ("config delta not Auto", [U32, U32], [GOOD, GOOD], dict(cfg=G.make_config(delta=G.DELTA_NOOP)), "must be Auto"),
    ("CONV1 flag", [U32, U32], [GOOD, GOOD], dict(cfg=G.make_config(conv1=True)), "PCO_GFX_CFG_CONV1"),
    ("DICT flag", [U32, U32], [GOOD, GOOD], dict(cfg=G.make_config(dict=True)), "PCO_GFX_CFG_CONV1 or PCO_GFX_CFG_DICT"),
    ("invalid dtype", [U32, 12], [GOOD, GOOD], {}, "chunk spec 1: invalid dtype"),
    ("Auto mode", [U32, U32], [GOOD, S.spec(mode=G.MODE_AUTO)], {}, "chunk spec 1: mode_kind"),
    ("Dict mode", [U32, U32], [GOOD, S.spec(mode=G.MODE_TRY_DICT)], {}, "chunk spec 1: mode_kind"),
    ("unknown mode", [U32, U32], [GOOD, S.spec(mode=6)], {}, "chunk spec 1: mode_kind"),
    ("Auto delta", [U32, U32], [GOOD, S.spec(delta=G.DELTA_AUTO)], {}, "chunk spec 1: delta_kind"),
    ("Conv1 delta", [U32, U32], [GOOD, S.spec(delta=G.DELTA_TRY_CONV1, order=2)], {}, "chunk spec 1: delta_kind"),
    ("unknown delta", [U32, U32], [GOOD, S.spec(delta=5)], {}, "chunk spec 1: delta_kind"),
    ("IntMult on floats", [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, base=10)], {}, "chunk spec 1: unable to use int mult mode on floats"),
    ("FloatMult on ints", [U32, I64], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=F32_ONE)], {}, "chunk spec 1: unable to use float mode for ints"),
    ("FloatQuant on ints", [U32, U16], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=3)], {}, "chunk spec 1: unable to use float mode for ints"),
    ("IntMult base 0", [U32, U32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, base=0)], {}, "chunk spec 1: The chosen mode was invalid for the number type"),
    ("IntMult base 0 at the width", [U32, U16], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, base=1 << 16)], {}, "chunk spec 1: The chosen mode was invalid for the number type"),
    ("FloatMult base 0", [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=0)], {}, "chunk spec 1: The chosen mode was invalid for the number type"),
    ("FloatMult base -0", [U32, F64], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=1 << 63)], {}, "chunk spec 1: The chosen mode was invalid for the number type"),
    ("FloatMult base inf", [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=0x7f800000)], {}, "chunk spec 1: The chosen mode was invalid for the number type"),
    ("FloatMult base NaN", [U32, F16], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=0x7e00)], {}, "chunk spec 1: The chosen mode was invalid for the number type"),
    ("FloatMult base beyond the width", [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=S.float_bits(0.01, np.float64))], {}, "chunk spec 1: The chosen mode was invalid"),
    ("FloatQuant k 0", [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=0)], {}, "chunk spec 1: The chosen mode was invalid for the number type"),
    ("FloatQuant k beyond f32's precision", [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=24)], {}, "chunk spec 1: The chosen mode was invalid"),
    ("FloatQuant k beyond f16's precision", [U32, F16], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=11)], {}, "chunk spec 1: The chosen mode was invalid"),
    ("FloatQuant k beyond f64's precision", [U32, F64], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=53)], {}, "chunk spec 1: The chosen mode was invalid"),
    ("order 0", [U32, U32], [GOOD, S.spec(delta=G.DELTA_TRY_CONSECUTIVE, order=0)], {}, "chunk spec 1: consecutive delta order"),
    ("order 8", [U32, U32], [GOOD, S.spec(delta=G.DELTA_TRY_CONSECUTIVE, order=8)], {}, "chunk spec 1: consecutive delta order"),
    ("reserved", [U32, U32], [GOOD, S.spec(reserved=1)], {}, "chunk spec 1: reserved"),
    ("mode_inv without FloatMult", [U32, U32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, base=3, inv=5)], {}, "chunk spec 1: mode_inv"),
]
# the same calls made good: what replaces the bad spec / keyword
MADE_GOOD = {
    "IntMult on floats": ([U32, I32], None), "FloatMult on ints": ([U32, F32], None), "FloatQuant on ints": ([U32, F16], None), "invalid dtype": ([U32, I8], None),
    "IntMult base 0": (None, S.spec(mode=G.MODE_TRY_INT_MULT, base=7)), "IntMult base 0 at the width": (None, S.spec(mode=G.MODE_TRY_INT_MULT, base=(1 << 16) + 5)),
    "FloatMult base 0": (None, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=1)),                                   # (the smallest subnormal is a base)
    "FloatMult base -0": (None, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=(1 << 63) | 1)),
    "FloatMult base inf": (None, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=0x7f7fffff)),
    "FloatMult base NaN": (None, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=0x7bff)),
    "FloatMult base beyond the width": (None, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=S.float_bits(0.01, np.float32), inv=S.float_bits(100.0, np.float32))),
    "FloatQuant k 0": (None, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=1)), "FloatQuant k beyond f32's precision": (None, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=23)),
    "FloatQuant k beyond f16's precision": (None, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=10)), "FloatQuant k beyond f64's precision": (None, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=52)),
    "order 0": (None, S.spec(delta=G.DELTA_TRY_CONSECUTIVE, order=1)), "order 8": (None, S.spec(delta=G.DELTA_TRY_CONSECUTIVE, order=7)),
    "mode_inv without FloatMult": (None, S.spec(mode=G.MODE_TRY_INT_MULT, base=3)),
}


@pytest.mark.parametrize("wrapped", [False, True], ids=["standalone", "wrapped"])
@pytest.mark.parametrize("row", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_host_refusal_comes_before_a_device_is_asked_for(row, wrapped):
    what, dtypes, specs, kw, word = row
    code, status, msg, untouched = call(wrapped, dtypes, specs, **kw)
    assert code == G.PcoCompressionError and status == INVALID and word in msg and untouched, (what, code, status, msg)
    # the same call made good gets as far as the device
    g_dtypes, g_spec = MADE_GOOD.get(what, (None, None))
    good_specs = [specs[0], g_spec if g_spec is not None else (specs[1] if g_dtypes is not None else GOOD)]
    if not no_device():   # (fake pointers must not reach a device that exists: there the refusal is all that is checked)
        return
    code, status, msg, untouched = call(wrapped, g_dtypes or dtypes, good_specs)
    assert code == G.PcoCompressionError and status == DEVICE and untouched, (what, status, msg)


def test_the_refusals_are_made_in_the_documented_order():
    """two things wrong in one call: the earlier row of the header's table answers"""
    both = G.make_config(mode=G.MODE_CLASSIC, conv1=True)
    bad_all = S.spec(mode=G.MODE_AUTO, delta=G.DELTA_AUTO, order=9, reserved=1, inv=1)
    order = [
        (dict(tasks_null=True, specs_null=True, cfg=both), [U32, U32], [GOOD, bad_all], "null tasks"),
        (dict(specs_null=True, cfg=both), [U32, U32], [GOOD, bad_all], "null specs"),
        (dict(cfg=both), [U32, 12], [GOOD, bad_all], "must be Auto"),
        (dict(cfg=G.make_config(conv1=True)), [U32, 12], [GOOD, bad_all], "PCO_GFX_CFG_CONV1"),
        ({}, [U32, 12], [GOOD, bad_all], "chunk spec 1: invalid dtype"),
        ({}, [U32, U32], [GOOD, bad_all], "chunk spec 1: mode_kind"),
        ({}, [U32, U32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, delta=G.DELTA_AUTO, reserved=1, inv=1)], "chunk spec 1: delta_kind"),
        ({}, [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, delta=G.DELTA_TRY_CONSECUTIVE, order=9, reserved=1, inv=1)], "int mult mode on floats"),
        ({}, [U32, U32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, delta=G.DELTA_TRY_CONSECUTIVE, order=9, reserved=1, inv=1)], "The chosen mode was invalid"),
        ({}, [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=0, delta=G.DELTA_TRY_CONSECUTIVE, order=9, reserved=1)], "The chosen mode was invalid"),
        ({}, [U32, F32], [GOOD, S.spec(mode=G.MODE_TRY_FLOAT_QUANT, k=0, delta=G.DELTA_TRY_CONSECUTIVE, order=9, reserved=1, inv=1)], "The chosen mode was invalid"),
        ({}, [U32, U32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, base=2, delta=G.DELTA_TRY_CONSECUTIVE, order=9, reserved=1, inv=1)], "consecutive delta order"),
        ({}, [U32, U32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, base=2, delta=G.DELTA_TRY_CONSECUTIVE, order=2, reserved=1, inv=1)], "reserved"),
        ({}, [U32, U32], [GOOD, S.spec(mode=G.MODE_TRY_INT_MULT, base=2, delta=G.DELTA_TRY_CONSECUTIVE, order=2, inv=1)], "mode_inv"),
        # the first failing task answers
        ({}, [U32, U32], [S.spec(reserved=1), S.spec(mode=G.MODE_AUTO)], "chunk spec 0: reserved"),
    ]
    for wrapped in (False, True):
        for kw, dtypes, specs, word in order:
            code, status, msg, untouched = call(wrapped, dtypes, specs, **kw)
            assert code == G.PcoCompressionError and status == INVALID and word in msg and untouched, (wrapped, word, msg)
        code, status, msg, _ = call(True, [U32, U32], [GOOD, bad_all], out_null=True, tasks_null=True)
        assert status == INVALID and "null infos and d_infos" in msg


def test_a_null_config_is_the_default_config():
    code, status, msg, untouched = call(False, [U32, U32], [GOOD, S.spec(reserved=1)], cfg=None)
    assert status == INVALID and "chunk spec 1: reserved" in msg and untouched
    if no_device():
        code, status, msg, untouched = call(False, [U32, U32], [GOOD, GOOD], cfg=None)
        assert status == DEVICE and untouched


# ---------------------------------------------------------------------------------------------------------------------------------------
# pco_gfx_resolve_chunk_specs under explicit configs: no device, a table written out by hand
# ---------------------------------------------------------------------------------------------------------------------------------------
def resolve(dt, n=100, **cfg):
    L = G.lib()
    task = G.EncodeTask(0x10000, n, None, 0, dt, 0)
    out = G.ChunkSpec(9, 9, 9, 9, 9, 9, 9)
    c = G.make_config(enable_8_bit=True, **cfg)
    code = L.pco_gfx_resolve_chunk_specs(1, C.byref(task), C.byref(c), C.byref(out), None)
    return code, L.pco_gfx_last_status(), (L.pco_gfx_last_error() or b"").decode(), S.spec_key(out)


INTS, FLOATS = (U32, U64, I32, I64, U16, I16, U8, I8), (F32, F64, F16)
WIDTH = {t.byte: t.width * 8 for t in G.NUMBER_TYPES}
DELTAS = [   # (config, the (delta_kind, delta_order) that comes back)
    (dict(delta=G.DELTA_NOOP), (G.DELTA_NOOP, 0)),
    (dict(delta=G.DELTA_TRY_CONSECUTIVE, delta_order=0), (G.DELTA_NOOP, 0)),
    (dict(delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), (G.DELTA_TRY_CONSECUTIVE, 1)),
    (dict(delta=G.DELTA_TRY_CONSECUTIVE, delta_order=7), (G.DELTA_TRY_CONSECUTIVE, 7)),
    (dict(delta=G.DELTA_TRY_LOOKBACK), (G.DELTA_TRY_LOOKBACK, 0)),
]
# FloatMult rows: (type, the base as the config's double, mode_base bits, mode_inv bits), every bit pattern written out
FLOAT_MULT = [
    (F64, 0.01, 0x3F847AE147AE147B, 0x4059000000000000),                  # 1 / 0.01 = 100 exactly
    (F64, -0.01, 0xBF847AE147AE147B, 0xC059000000000000),                 # a negative base
    (F64, 1.0 / 49.0, 0x3F94E5E0A72F0539, 0x4048800000000001),            # 1 / (1 / 49) = 49.00000000000001: NOT the 49 Auto's snap carries
    (F64, 5e-324, 0x0000000000000001, 0x7FF0000000000000),                # the smallest subnormal base: its inverse overflows to +inf
    (F64, 2.0 ** 1023, 0x7FE0000000000000, 0x0008000000000000),           # a base whose inverse (2^-1023) is subnormal
    (F32, 0.01, 0x3C23D70A, 0x42C80000),                                  # the double rounds to f32 once; 1 / that = 100
    (F32, 0.001, 0x3A83126F, 0x4479FFFF),                                 # 1 / f32(0.001) = 999.99994: NOT the 1000 Auto's snap carries
    (F32, -0.125, 0xBE000000, 0xC1000000),
    (F32, 1e-45, 0x00000001, 0x7F800000),                                 # subnormal base, infinite inverse
    (F32, 2.0 ** 127, 0x7F000000, 0x00400000),                            # subnormal inverse (2^-127)
    (F16, 0.01, 0x211F, 0x5640),                                          # f16(0.01) = 0.010002136; 1 / that rounds to 100
    (F16, -0.5, 0xB800, 0xC000),
    (F16, 6e-8, 0x0001, 0x7C00),                                          # subnormal base, infinite inverse
    (F16, 32768.0, 0x7800, 0x0200),                                       # subnormal inverse (2^-15)
]


def test_resolve_under_explicit_configs_gives_the_table_without_a_device():
    n_rows = 0
    for dcfg, (dk, do) in DELTAS:
        for dt in INTS + FLOATS:
            assert resolve(dt, mode=G.MODE_CLASSIC, **dcfg) == (0, 0, "", (G.MODE_CLASSIC, dk, do, 0, 0, 0, 0)); n_rows += 1
        for dt in INTS:   # the base comes back cut to the type's width
            base = 0x0102030405060709
            want = {8: 0x09, 16: 0x0709, 32: 0x05060709, 64: base}[WIDTH[dt]]
            assert resolve(dt, mode=G.MODE_TRY_INT_MULT, mode_u64=base, **dcfg) == (0, 0, "", (G.MODE_TRY_INT_MULT, dk, do, 0, want, 0, 0)); n_rows += 1
        for dt, prec in ((F32, 23), (F64, 52), (F16, 10)):
            for k in (1, prec):
                assert resolve(dt, mode=G.MODE_TRY_FLOAT_QUANT, mode_u64=k, **dcfg) == (0, 0, "", (G.MODE_TRY_FLOAT_QUANT, dk, do, k, 0, 0, 0)); n_rows += 1
        for dt, base, bits, inv in FLOAT_MULT:
            assert resolve(dt, mode=G.MODE_TRY_FLOAT_MULT, mode_f64=base, **dcfg) == (0, 0, "", (G.MODE_TRY_FLOAT_MULT, dk, do, 0, bits, inv, 0)), (dt, base); n_rows += 1
    assert n_rows == len(DELTAS) * (11 + 8 + 6 + len(FLOAT_MULT))
    # the two rows the field exists for: the inverse an explicit spec computes is not the round one
    assert 0x4048800000000001 != S.float_bits(49.0, np.float64) and 0x4479FFFF != S.float_bits(1000.0, np.float32)


def test_resolve_refuses_what_the_encode_refuses_and_what_a_spec_cannot_carry():
    UNTOUCHED = (9,) * 7
    for cfg, dt, status, word in [
        (dict(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP), U32, UNSUPPORTED, "dictionary"),
        (dict(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True), U32, UNSUPPORTED, "dictionary"),
        (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONV1, delta_order=2), U32, UNSUPPORTED, "Conv1"),
        (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONV1, delta_order=2, conv1=True), U32, UNSUPPORTED, "Conv1"),
        (dict(mode=G.MODE_AUTO, delta=G.DELTA_TRY_CONV1, delta_order=2, conv1=True), U32, UNSUPPORTED, "Conv1"),
        (dict(mode=G.MODE_TRY_INT_MULT, mode_u64=3, delta=G.DELTA_NOOP), F32, INVALID, "unable to use int mult mode on floats"),
        (dict(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.5, delta=G.DELTA_NOOP), I32, INVALID, "unable to use float mode for ints"),
        (dict(mode=G.MODE_TRY_FLOAT_QUANT, mode_u64=3, delta=G.DELTA_NOOP), U64, INVALID, "unable to use float mode for ints"),
        (dict(mode=G.MODE_TRY_INT_MULT, mode_u64=1 << 32, delta=G.DELTA_NOOP), U32, INVALID, "The chosen mode was invalid for the number type"),
        (dict(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.0, delta=G.DELTA_NOOP), F64, INVALID, "The chosen mode was invalid for the number type"),
        (dict(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=float("inf"), delta=G.DELTA_NOOP), F32, INVALID, "The chosen mode was invalid for the number type"),
        (dict(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=1e300, delta=G.DELTA_NOOP), F32, INVALID, "The chosen mode was invalid for the number type"),   # (inf as f32)
        (dict(mode=G.MODE_TRY_FLOAT_QUANT, mode_u64=24, delta=G.DELTA_NOOP), F32, INVALID, "The chosen mode was invalid for the number type"),
        (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=8), U32, INVALID, "consecutive delta order may not exceed 7"),
        (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP, level=13), U32, INVALID, "compression level may not exceed 12"),
        (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), 12, INVALID, "invalid dtype"),
    ]:
        code, st, msg, key = resolve(dt, **cfg)
        assert code == G.PcoCompressionError and st == status and word in msg and key == UNTOUCHED, (cfg, dt, st, msg)
    code, st, msg, key = resolve(U32, n=0, mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP)
    assert st == INVALID and "cannot compress empty chunk" in msg and key == UNTOUCHED
    L = G.lib()
    c = G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP)
    assert L.pco_gfx_resolve_chunk_specs(1, None, C.byref(c), C.byref(G.ChunkSpec()), None) == G.PcoCompressionError and L.pco_gfx_last_status() == INVALID
    task = G.EncodeTask(0x10000, 5, None, 0, U32, 0)
    assert L.pco_gfx_resolve_chunk_specs(1, C.byref(task), C.byref(c), None, None) == G.PcoCompressionError and L.pco_gfx_last_status() == INVALID
    assert L.pco_gfx_resolve_chunk_specs(0, None, None, None, None) == G.PcoSuccess
    if no_device():   # an Auto half needs the device
        for cfg in (dict(), dict(mode=G.MODE_CLASSIC), dict(delta=G.DELTA_NOOP)):
            code, st, msg, key = resolve(U32, **cfg)
            assert code == G.PcoCompressionError and st == DEVICE and key == UNTOUCHED


def test_a_resolved_explicit_spec_passes_the_encode_entry_points_own_checks():
    """what resolve hands out is what the specs calls accept: every row of the table gets as far as the device"""
    if not no_device():   # (the accepted call would launch on fake pointers)
        return
    for dt, base, bits, inv in FLOAT_MULT:
        code, status, msg, untouched = call(False, [dt, dt], [S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=bits, inv=inv), S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=bits)])
        assert status == DEVICE and untouched, (dt, base, msg)


# ---------------------------------------------------------------------------------------------------------------------------------------
# pco_gfx_chunk_spec_from_meta
# ---------------------------------------------------------------------------------------------------------------------------------------
def file_header(f):
    """(bytes in front of the first chunk, the wrapped format's major version) of a standalone file, by the format's arithmetic
    (standalone/decompressor.rs:85-137)"""
    assert f[:4] == b"pco!"
    at = 4; sv = f[4]
    if sv >= 2:
        at = 5 + (1 if sv >= 3 else 0)
        power = 1 + (f[at] & 63)
        at += (6 + power + 7) // 8
    major = f[at]
    return at + (2 if major >= 4 else 1), major


def first_meta(f):
    """(ChunkMeta bytes of the file's first chunk, dtype byte, format major, the oracle's reading of it)"""
    hdr, major = file_header(f)
    info, _ = O.inspect_first_chunk(f)
    assert info.fmt_major == major and info.dtype == f[hdr]
    return f[hdr + 4: int(info.meta_end_byte)], int(info.dtype), major, info


def from_meta(meta, dt, major):
    L = G.lib()
    buf = (C.c_uint8 * max(len(meta), 1)).from_buffer_copy(bytes(meta) or b"\0")
    out = G.ChunkSpec(9, 9, 9, 9, 9, 9, 9)
    code = L.pco_gfx_chunk_spec_from_meta(buf, len(meta), dt, major, C.byref(out))
    return code, L.pco_gfx_last_status(), out


def check_spec_against_meta(meta, dt, major, info, name):
    code, status, spec = from_meta(meta, dt, major)
    assert code == G.PcoSuccess, (name, status)
    mi = G.ChunkMetaInfo()
    buf = (C.c_uint8 * len(meta)).from_buffer_copy(meta)
    assert G.lib().pco_gfx_chunk_meta_info(buf, len(meta), dt, major, C.byref(mi)) == G.PcoSuccess
    for src in (mi, info):   # the library's own reading and the oracle's
        assert spec.mode_kind == S.META_MODE[src.mode_kind] and spec.delta_kind == S.META_DELTA[src.delta_kind], name
        assert spec.delta_order == (src.delta_order if src.delta_kind == 1 else 0) and spec.mode_k == (src.mode_k if src.mode_kind == 3 else 0), name
        want_base = {0: 0, 1: src.mode_base_latent, 2: S.base_from_latent(int(src.mode_base_latent), NP[dt]) if src.mode_kind == 2 else 0, 3: 0}[src.mode_kind]
        assert spec.mode_base == want_base and spec.mode_inv == 0 and spec.reserved == 0, name
    return spec


def test_the_recipes_resolve_as_named_and_their_metas_give_their_specs():
    """the oracle's Auto encode of every case of the GPU tests: the outcome its name says, every Auto outcome reached, and the spec its ChunkMeta
    describes"""
    seen = set()
    for name, a, want in S.cases():
        f = O.simple_compress(a, O.make_config())
        meta, dt, major, info = first_meta(f)
        assert dt == G.DTYPE_BYTE[a.dtype.name] and major == 4
        spec = check_spec_against_meta(meta, dt, major, info, name)
        assert (spec.mode_kind, spec.delta_kind) == want, (name, spec)
        seen.add(want[0]); seen.add(("delta", want[1]))
        if spec.mode_kind == G.MODE_TRY_FLOAT_MULT:   # the base is a finite number of the type, and the spec passes the encode's checks as it stands
            assert np.isfinite(S.bits_float(spec.mode_base, a.dtype)) and S.bits_float(spec.mode_base, a.dtype) > 0
    assert seen == {G.MODE_CLASSIC, G.MODE_TRY_INT_MULT, G.MODE_TRY_FLOAT_MULT, G.MODE_TRY_FLOAT_QUANT,
                    ("delta", G.DELTA_NOOP), ("delta", G.DELTA_TRY_CONSECUTIVE), ("delta", G.DELTA_TRY_LOOKBACK)}
    names = [n for n, _, _ in S.cases()]
    assert {"n9", "n1", "f16_decimal_0.01"} <= set(names) and min(a.size for _, a, _ in S.cases()) == 1 and max(a.size for _, a, _ in S.cases()) == 1 << 16


@pytest.mark.parametrize("path", ASSETS, ids=[os.path.basename(p) for p in ASSETS])
def test_the_golden_assets_give_the_specs_their_metas_describe(path):
    assert len(ASSETS) == 13
    f = open(path, "rb").read()
    hdr, major = file_header(f)
    name = os.path.basename(path)
    if "dict" in name or "conv1" in name:
        dt = f[hdr]
        code, status, spec = from_meta(f[hdr + 4:], dt, major)
        assert code == G.PcoCompressionError and status == UNSUPPORTED and S.spec_key(spec) == (9,) * 7
        return
    if f[hdr] == 0:   # a file without chunks (the terminator follows the header): no ChunkMeta, and none is made up
        assert name == "v0_1_1_standalone_versioned.pco"
        code, status, spec = from_meta(b"", U32, major)
        assert code != G.PcoSuccess and status == G.ST_INSUFFICIENT_DATA and S.spec_key(spec) == (9,) * 7
        return
    meta, dt, major, info = first_meta(f)
    spec = check_spec_against_meta(meta, dt, major, info, name)
    for word, mode in (("classic", G.MODE_CLASSIC), ("float_mult", G.MODE_TRY_FLOAT_MULT), ("int_mult", G.MODE_TRY_INT_MULT), ("float_quant", G.MODE_TRY_FLOAT_QUANT)):
        if word in name:
            assert spec.mode_kind == mode
    if "lookback" in name:
        assert spec.delta_kind == G.DELTA_TRY_LOOKBACK
    if "delta_" in name:
        assert spec.delta_kind == G.DELTA_TRY_CONSECUTIVE and 1 <= spec.delta_order <= 7
    assert paged.spec_from_meta(meta, dt, format_major=major) == spec


def test_spec_from_meta_refuses_a_delta_d_secondary_and_bad_arguments():
    a = (np.arange(1000) * 7 + (np.arange(1000) % 3)).astype(np.int32)
    f = O.test_encode(a, mode=O.MODE_TRY_INT_MULT, mode_u64=7, delta=O.TE_DELTA_CONSECUTIVE, order=1, secondary_uses_delta=True)
    meta, dt, major, info = first_meta(f)
    code, status, spec = from_meta(meta, dt, major)
    assert code == G.PcoCompressionError and status == UNSUPPORTED and S.spec_key(spec) == (9,) * 7
    f = O.test_encode(a, mode=O.MODE_TRY_INT_MULT, mode_u64=7, delta=O.TE_DELTA_CONSECUTIVE, order=1)
    meta, dt, major, info = first_meta(f)
    assert S.spec_key(check_spec_against_meta(meta, dt, major, info, "int mult, consecutive")) == (G.MODE_TRY_INT_MULT, G.DELTA_TRY_CONSECUTIVE, 1, 0, 7, 0, 0)
    code, status, _ = from_meta(meta[:1], dt, major)
    assert code != G.PcoSuccess and status == G.ST_INSUFFICIENT_DATA
    code, status, _ = from_meta(meta, 12, major)
    assert code == G.PcoInvalidType and status == INVALID
    buf = (C.c_uint8 * len(meta)).from_buffer_copy(meta)
    assert G.lib().pco_gfx_chunk_spec_from_meta(buf, len(meta), dt, major, None) == G.PcoInvalidType and G.lib().pco_gfx_last_status() == INVALID


# ---------------------------------------------------------------------------------------------------------------------------------------
# pcodec_amd.paged: the specs= keyword, checked before a device is asked for
# ---------------------------------------------------------------------------------------------------------------------------------------
class FakeTensor:   # enough of a tensor for the argument handling: nothing of it is read before the device check
    pass


def test_the_specs_keyword_is_checked_before_a_device_is_asked_for():
    s1, s2 = S.spec(delta=G.DELTA_TRY_CONSECUTIVE, order=1), S.spec(mode=G.MODE_TRY_INT_MULT, base=1000)
    arr = paged.spec_array([s1, s2], 2)
    assert [S.spec_key(arr[i]) for i in range(2)] == [S.spec_key(s1), S.spec_key(s2)]
    arr = paged.spec_array(s2, 3)   # a single spec is applied to all
    assert [S.spec_key(arr[i]) for i in range(3)] == [S.spec_key(s2)] * 3
    assert C.sizeof(paged.spec_array([], 0)) == 40   # (never a zero-length ctypes array)
    tensors = [FakeTensor(), FakeTensor(), FakeTensor()]
    for f in (paged.compress_chunks, paged.compress_standalone_chunks):
        with pytest.raises(ValueError, match="one ChunkSpec per tensor"):
            f(tensors, specs=[s1, s2])
        with pytest.raises(ValueError, match="one ChunkSpec per tensor"):
            f(tensors, specs=[])
        with pytest.raises(TypeError, match="ChunkSpec"):
            f(tensors, specs=[s1, s2, (1, 1)])
        with pytest.raises(ValueError, match="at Auto"):
            f(tensors, specs=s1, config=ChunkConfig(mode_spec=ModeSpec.classic()))
        with pytest.raises(ValueError, match="at Auto"):
            f(tensors, specs=[s1, s2, s1], config=ChunkConfig(delta_spec=DeltaSpec.try_consecutive(1)))
        if no_device():   # good arguments get as far as the device check
            for kw in (dict(specs=s1), dict(specs=[s1, s2, s1], config=ChunkConfig(compression_level=5, verify=True))):
                with pytest.raises(G.PcoGfxError) as e:
                    f(tensors, **kw)
                assert e.value.status == DEVICE


def test_the_python_surface_names_a_spec():
    import pcodec_amd
    from pcodec_amd.config import ChunkSpec, spec_of
    assert pcodec_amd.ChunkSpec is ChunkSpec is G.ChunkSpec
    s = spec_of(ModeSpec.try_float_mult(0.001), DeltaSpec.try_consecutive(2), np.float32)
    assert S.spec_key(s) == (G.MODE_TRY_FLOAT_MULT, G.DELTA_TRY_CONSECUTIVE, 2, 0, 0x3A83126F, 0x4479FFFF, 0)
    assert s == S.spec(mode=G.MODE_TRY_FLOAT_MULT, delta=G.DELTA_TRY_CONSECUTIVE, order=2, base=0x3A83126F, inv=0x4479FFFF) and s != S.spec()
    assert spec_of(ModeSpec.classic(), DeltaSpec.try_consecutive(0), "uint8") == S.spec()
