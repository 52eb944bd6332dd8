"""Shared by test_chunk_specs_abi.py and test_gpu_chunk_specs.py: the chunks whose Auto resolution reaches every outcome, what each is
expected to resolve to, and the spec <-> config arithmetic of include/pco_gfx.h section 3c done by hand."""
import ctypes as C
import functools

import numpy as np

from pcodec_amd import _lib as G

# ChunkMeta numbering (metadata/mode.rs, delta_encoding.rs) -> the spec kinds of include/pco_gfx.h
META_MODE = {0: G.MODE_CLASSIC, 1: G.MODE_TRY_INT_MULT, 2: G.MODE_TRY_FLOAT_MULT, 3: G.MODE_TRY_FLOAT_QUANT}
META_DELTA = {0: G.DELTA_NOOP, 1: G.DELTA_TRY_CONSECUTIVE, 2: G.DELTA_TRY_LOOKBACK}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _quantised(r, n, k):
    x = r.normal(0.0, 1.0, n).astype(np.float32)
    return (x.view(np.uint32) & np.uint32(~((1 << k) - 1) & 0xffffffff)).view(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, array, expected (mode, delta) spec kinds)]: plain recipes, 1 to 2^16 numbers each.  The expectations are confirmed against the
    oracle's Auto encode on the CPU (test_chunk_specs_abi.py) before the GPU tests rely on them."""
    r = np.random.default_rng(20261021)
    n = 1 << 14
    period = r.integers(-(1 << 40), 1 << 40, 365)
    out = [
        ("u64_ramp", np.uint64(1 << 40) + np.uint64(1000) * np.arange(1 << 16, dtype=np.uint64) + r.integers(0, 512, 1 << 16).astype(np.uint64),
         (G.MODE_CLASSIC, G.DELTA_TRY_CONSECUTIVE)),
        ("i64_periodic", (period[np.arange(n) % 365] + r.integers(-3, 4, n)).astype(np.int64), (G.MODE_CLASSIC, G.DELTA_TRY_LOOKBACK)),
        ("f64_decimal_0.01", r.integers(1000, 1000000, n) / 100.0, (G.MODE_TRY_FLOAT_MULT, G.DELTA_NOOP)),
        ("f32_decimal_0.01", (r.integers(100, 10000, n) / 100.0).astype(np.float32), (G.MODE_TRY_FLOAT_MULT, G.DELTA_NOOP)),
        # 1 / (1 / 49) is not 49 in f64, and 1 / (1 / 1000) is not 1000 in f32: the snapped inverse differs from what TryFloatMult(base) computes
        ("f64_multiples_of_1/49", r.integers(1000, 1000000, n) / 49.0, (G.MODE_TRY_FLOAT_MULT, G.DELTA_NOOP)),
        ("f32_decimal_0.001", (r.integers(100, 10000, n).astype(np.float32) / np.float32(1000.0)), (G.MODE_TRY_FLOAT_MULT, G.DELTA_NOOP)),
        # (FloatMult by trailing zeros; its bid and FloatQuant's are close on such data, so the draw is a fixed one of its own that the oracle confirms)
        ("f32_multiples_of_2^-2", (np.random.default_rng(7).integers(1, 1 << 10, n) / 4.0).astype(np.float32), (G.MODE_TRY_FLOAT_MULT, G.DELTA_NOOP)),
        ("f32_quantised", _quantised(r, n, 12), (G.MODE_TRY_FLOAT_QUANT, G.DELTA_NOOP)),
        ("i32_multiples_of_1000", (r.integers(-(1 << 20), 1 << 20, n) * 1000).astype(np.int32), (G.MODE_TRY_INT_MULT, G.DELTA_NOOP)),
        ("u32_random", r.integers(0, 1 << 32, 5001, dtype=np.uint64).astype(np.uint32), (G.MODE_CLASSIC, G.DELTA_NOOP)),
        # (f16's 10 mantissa bits leave a decimal base nothing to save: the reference keeps Classic; f16 chunks take the detection's host path)
        ("f16_decimal_0.01", (r.integers(1, 200, 4099) / 100.0).astype(np.float16), (G.MODE_CLASSIC, G.DELTA_NOOP)),
        ("n9", np.arange(9, dtype=np.int64) * 7, (G.MODE_CLASSIC, G.DELTA_NOOP)),
        ("n1", np.array([42], np.uint32), (G.MODE_CLASSIC, G.DELTA_NOOP)),
    ]
    return tuple((name, np.ascontiguousarray(a), exp) for name, a, exp in out)


def spec_key(s):
    return (s.mode_kind, s.delta_kind, s.delta_order, s.mode_k, s.mode_base, s.mode_inv, s.reserved)


def float_bits(x, dtype):
    return int(np.array([x], dtype).view(UINT[np.dtype(dtype).itemsize])[0])


def bits_float(b, dtype):
    return np.array([b], UINT[np.dtype(dtype).itemsize]).view(dtype)[0]


def base_from_latent(lat, dtype):
    """The bit pattern of a float whose ordered latent (to_latent_ordered) is `lat`."""
    bits = np.dtype(dtype).itemsize * 8
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    return (lat ^ top) if lat & top else (~lat & mask)


def configs_of_spec(s, dtype, **kw):
    """(product config, oracle config) of the explicit ChunkConfig a spec expresses -- exact for every spec whose mode_inv is 0 or 1 / base."""
    import oracle_lib as O
    d = dict(mode=s.mode_kind, delta=s.delta_kind, delta_order=s.delta_order)
    if s.mode_kind == G.MODE_TRY_INT_MULT: d["mode_u64"] = s.mode_base
    if s.mode_kind == G.MODE_TRY_FLOAT_QUANT: d["mode_u64"] = s.mode_k
    if s.mode_kind == G.MODE_TRY_FLOAT_MULT: d["mode_f64"] = float(bits_float(s.mode_base, dtype))
    okw = {k: v for k, v in kw.items() if k in ("level", "max_page_n")}
    return G.make_config(enable_8_bit=True, **d, **kw), O.make_config(**d, **okw)


def inv_is_one_over_base(s, dtype):
    with np.errstate(all="ignore"):
        one_over = np.array([1], dtype)[0] / bits_float(s.mode_base, dtype)
    return s.mode_inv == 0 or s.mode_inv == float_bits(one_over, dtype)


def spec_array(specs):
    arr = (G.ChunkSpec * max(len(specs), 1))()
    for i, s in enumerate(specs):
        C.memmove(C.addressof(arr[i]), C.addressof(s), C.sizeof(G.ChunkSpec))
    return arr


def spec(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP, order=0, k=0, base=0, inv=0, reserved=0):
    return G.ChunkSpec(mode, delta, order, k, base, inv, reserved)
