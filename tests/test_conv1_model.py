"""CPU checks of the Conv1 fit: the numpy model (tests/conv1_model.py, a restatement of delta/conv1.rs choose_config) against the known-answer
table and the reference's own v1_0_0_conv1.pco asset, the device's floor(log2) rule against the host's math.log2, and the host-side ChunkMeta
accessor pco_gfx_chunk_meta_conv1 on the asset's bytes.  No GPU needed."""
import math
import os

import numpy as np
import pytest

import conv1_model as M
from pcodec_amd import _lib as G

ASSET = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_assets", "v1_0_0_conv1.pco")


@pytest.mark.parametrize("kid,gen,order,q,bias,weights", M.KAT, ids=[f"{k[0]}-o{k[2]}" for k in M.KAT])
def test_model_reproduces_the_kat_table(kid, gen, order, q, bias, weights):
    lat, bits = M.latents_of(gen())
    got = M.choose_config(lat, order, bits)
    assert got is not None
    assert (got[0], got[1]) == (q, bias)
    assert len(got[2]) == order
    if weights is not None:
        assert got[2] == weights


def test_model_with_the_1_0_0_switches_reproduces_the_asset():
    # 1.0.0 had no ridge and no `- 1` in the quantization: with both switched back the fit is the asset's ChunkMeta (compatibility.rs:262-277)
    lat, bits = M.latents_of(M.k1_series())
    assert M.choose_config(lat, 2, bits, v100=True) == M.ASSET_V100
    # ... and the current fit writes different parameters for the same data (the asset is no re-encode golden)
    assert M.choose_config(lat, 2, bits) != M.ASSET_V100


def test_model_noop_cases():
    lat, bits = M.latents_of(np.arange(5, dtype=np.int32))
    assert M.choose_config(lat, 5, bits) is None          # n < order + 1 (conv1.rs:359-361)
    assert M.choose_config(lat, 4, bits) is not None


def _log2_band(k):
    # the doubles just below and at 2^k: where floor(log2 x) can differ from the exponent
    x = 2.0 ** k
    out = [x]
    for _ in range(40):
        x = math.nextafter(x, 0.0)
        out.append(x)
    return out + [2.0 ** k * (1 + 2.0 ** -52), 2.0 ** k * 0.75, 2.0 ** k * (1 - 2.0 ** -20)]


@pytest.mark.parametrize("k", range(1, 64))
def test_floor_log2_rule_matches_host_log2(k):
    # the device takes floor(log2 x) from the exponent of x, and k where log2(x) rounds up to the integer k (encode_conv1.hip
    # conv1_floor_log2); Rust's f64::log2 is the platform libm's, as Python's math.log2 is
    for x in _log2_band(k):
        assert M.floor_log2_rule(x) == math.floor(math.log2(x)), (k, x.hex())


def test_floor_log2_rule_random():
    rng = np.random.default_rng(5)
    for x in np.exp2(rng.uniform(0, 63, 20000)):
        x = float(x)
        assert M.floor_log2_rule(x) == math.floor(math.log2(x)), x.hex()


def test_chunk_meta_conv1_accessor_reads_the_asset():
    blob = open(ASSET, "rb").read()
    at = blob.find(bytes([3, 0xCF, 0x07, 0x00]))     # the chunk: i32 dtype byte, 24-bit n - 1 = 1999, then its ChunkMeta
    assert at > 0
    meta = blob[at + 4:]
    assert G.chunk_meta_conv1(meta, G.DTYPE_BYTE["int32"]) == M.ASSET_V100
    with pytest.raises(G.PcoGfxError):
        G.chunk_meta_conv1(meta[:10], G.DTYPE_BYTE["int32"])
    # a ChunkMeta without Conv1 (Classic, NoOp delta: mode 0, delta 0, ...) gives None
    assert G.chunk_meta_conv1(bytes([0, 0, 0, 0, 0, 0, 0, 0]), G.DTYPE_BYTE["int32"]) is None
