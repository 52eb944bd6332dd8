"""What tests/test_verify_abi.py (CPU) and tests/test_gpu_verify.py (GPU) share: the damaged chunks of the verify tests and what each of them is
expected to decode to.  The CPU test certifies every expectation with the ORACLE's decoder; the GPU test then holds pco_gfx_verify_chunks /
pco_gfx_verify_wrapped_chunks against the same expectations, so that none of them comes from the code under test.

The chunk: 1000 u32 numbers in [0, 2^16) that include both ends, Classic mode without delta at compression level 0.  Level 0 histograms into ONE bin,
so the chunk has no tANS bits at all and its page is the numbers' 16-bit offsets back to back: number i's offset is the two bytes at
len(chunk) - 2 * n + 2 * i, for a standalone chunk and for every page of a wrapped one alike.  A bit flipped there changes number i and nothing else,
and the stream stays decodable -- damage every decoder survives, of the kind tests/test_gpu_page_ranges.py uses."""
import ctypes as C

import numpy as np

from pcodec_amd import _lib as G

N = 1000
SPEC = dict(level=0, mode=1, delta=1)   # Classic, NoOp, one bin
PAGES = [257, 1, 742]                   # the wrapped chunk's PagingSpec::Exact


def numbers():
    a = np.random.default_rng(77).integers(1, 1 << 16, N).astype(np.uint32)
    a[7] = 0; a[N - 2] = (1 << 16) - 1   # (both ends of the range, so that the one bin's offsets are 16 bits wide; the flipped indices below avoid them)
    return a


def flip_offset(chunk, n, i):
    """`chunk` (a standalone chunk or one page of n numbers) with the lowest bit of number i's offset flipped"""
    b = bytearray(chunk)
    b[len(b) - 2 * n + 2 * i] ^= 1
    return bytes(b)


def zero_body(chunk, n):
    """`chunk` with every offset overwritten with zeros: it decodes, to n copies of the bin's lower bound"""
    b = bytearray(chunk)
    b[len(b) - 2 * n:] = bytes(2 * n)
    return bytes(b)


def flip_meta(chunk, at):
    """`chunk` with bit 3 of the ChunkMeta's first byte (at `at`: 4 behind a standalone chunk's preamble, 0 in a wrapped ChunkMeta) flipped: the mode
    nibble (Classic = 0) then names no mode"""
    b = bytearray(chunk)
    b[at] ^= 8
    return bytes(b)


# name -> (damage of a standalone chunk, expected outcome): ("differs", index of the first differing number) or ("fails",)
STANDALONE_CASES = {
    "offset_first_batch": (lambda c: flip_offset(c, N, 5), ("differs", 5)),
    "offset_middle_batch": (lambda c: flip_offset(c, N, 300), ("differs", 300)),
    "offset_last_batch": (lambda c: flip_offset(c, N, N - 1), ("differs", N - 1)),
    "chunk_meta_bit": (lambda c: flip_meta(c, 4), ("fails",)),
    "body_zeroed": (lambda c: zero_body(c, N), ("differs", 0)),   # (number 0 is not the lower bound 0: numbers() draws from [1, 2^16) but for two places)
}
# name -> (piece damaged: 0 = the ChunkMeta, p = page p - 1; its damage; expected outcome OF THAT PAGE -- or, for the ChunkMeta, of every page)
WRAPPED_CASES = {
    "offset_first_page": (1, lambda c: flip_offset(c, PAGES[0], 5), ("differs", 5)),
    "offset_one_number_page": (2, lambda c: flip_offset(c, PAGES[1], 0), ("differs", 0)),
    "offset_last_page": (3, lambda c: flip_offset(c, PAGES[2], PAGES[2] - 1), ("differs", PAGES[2] - 1)),
    "chunk_meta_bit": (0, lambda c: flip_meta(c, 0), ("fails",)),
    "body_zeroed": (3, lambda c: zero_body(c, PAGES[2]), ("differs", 0)),
}


def standalone_file(chunk, n):
    """header | chunk | terminator: what the oracle's standalone decoder reads"""
    buf = (C.c_uint8 * 64)()
    k = G.lib().pco_gfx_write_standalone_header(buf, 64, n, G.DTYPE_BYTE["uint32"])
    return bytes(buf[:k]) + bytes(chunk) + b"\0"


def outcome(decoded, want):
    """("differs", first differing index -- or the decoded count when that is short and everything matched) / ("equal",) for a decode that ended OK"""
    m = min(len(decoded), len(want))
    diff = np.flatnonzero(decoded[:m] != want[:m])
    if diff.size:
        return ("differs", int(diff[0]))
    return ("equal",) if len(decoded) == len(want) else ("differs", m)
