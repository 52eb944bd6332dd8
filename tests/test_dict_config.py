"""CPU: the PCO_GFX_CFG_DICT flag is known to the library, validated like ChunkConfig::validate, and counted in the wrapped capacity."""
import ctypes as C

import numpy as np

from pcodec_amd import _lib as G
from pcodec_amd.config import ChunkConfig, ModeSpec


def _status(nums, cfg):
    L = G.lib()
    dst = np.zeros(1 << 16, np.uint8); n = C.c_size_t(0)
    rc = L.pco_gfx_simple_compress_into_ex(nums.ctypes.data_as(C.c_void_p), nums.size, G.DTYPE_BYTE[nums.dtype.name], C.byref(cfg), 0,
                                           dst.ctypes.data_as(C.c_void_p), dst.size, C.byref(n))
    return rc, L.pco_gfx_last_status(), L.pco_gfx_last_error().decode()


def test_validation_before_the_device():
    a = np.arange(100, dtype=np.uint32)
    rc, st, msg = _status(a, G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_TRY_CONV1, delta_order=2, conv1=True, dict=True))
    assert rc != 0 and st == G.ST_UNSUPPORTED, msg
    rc, st, msg = _status(a.astype(np.uint8), G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True))
    assert rc != 0 and st == G.ST_INVALID_ARGUMENT and "8-bit" in msg, msg
    rc, st, msg = _status(a, G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, conv1=True))
    assert rc != 0 and st == G.ST_UNSUPPORTED, msg


def test_python_config_carries_the_flag():
    c = ChunkConfig(mode_spec=ModeSpec.try_dict(), enable_dict=True).to_c()
    assert c.flags & G.CFG_DICT and c.mode_kind == G.MODE_TRY_DICT
    assert not ChunkConfig(mode_spec=ModeSpec.try_dict()).to_c().flags & G.CFG_DICT


def test_wrapped_cap_holds_the_dictionary():
    L = G.lib()
    L.pco_gfx_wrapped_chunk_cap.restype = C.c_size_t
    for dt, w in (("uint64", 8), ("uint8", 1), ("float16", 2)):
        n = 100000
        plain = L.pco_gfx_wrapped_chunk_cap(C.c_size_t(n), C.c_ubyte(G.DTYPE_BYTE[dt]), C.byref(G.make_config(mode=G.MODE_TRY_DICT)))
        with_dict = L.pco_gfx_wrapped_chunk_cap(C.c_size_t(n), C.c_ubyte(G.DTYPE_BYTE[dt]), C.byref(G.make_config(mode=G.MODE_TRY_DICT, dict=True)))
        assert with_dict >= plain + n * w + 4
