"""A third opinion on tANS tables: a small pure-Python model of the decoder's table construction and of the body of a one-variable
Classic / no-delta page, written from the format description and the reference's text -- ans/spec.rs:37-59 (how the
symbols are spread over the states), ans/decoding.rs:27-47 (what a state reads and where it goes), page_latent_decompressor.rs:89-177 (four
interleaved chains, the ANS bits of a batch, then its offsets; latent = lower.wrapping_add(offset)).  It shares no code with the oracle
(oracle/pco_oracle.hpp: spread_state_symbols is used by BOTH the test generator and the oracle's decoder, so the two cannot check each
other there).  Slow and plain on purpose: Python integers, one bit string."""
import numpy as np

BATCH_N = 256
INTERLEAVING = 4


class Bits:
    """The stream as one integer: bit i of the stream is bit (i mod 8) of byte i // 8, fields are little-endian."""

    def __init__(self, data):
        self.v = int.from_bytes(bytes(data), "little"); self.n = 8 * len(data); self.pos = 0

    def read(self, bits):
        x = (self.v >> self.pos) & ((1 << bits) - 1)
        self.pos += bits
        assert self.pos <= self.n, "read past the end"
        return x

    def align(self):
        pad = -self.pos % 8
        assert self.read(pad) == 0, "non-zero padding"


def spread_state_symbols(size_log, weights):
    """ans/spec.rs:37-59: symbol s takes weights[s] states, stepping through the table with an odd stride of about 3/5 of its size."""
    size = 1 << size_log
    assert sum(weights) == size and all(w > 0 for w in weights), "weights must be positive and sum to the table size"
    stride = 3 * size // 5
    stride += 1 - stride % 2
    out = [None] * size; step = 0
    for s, w in enumerate(weights):
        for _ in range(w):
            out[(stride * step) % size] = s; step += 1
    assert None not in out   # an odd stride visits every state of a power-of-two table
    return out


def decoder_nodes(size_log, weights):
    """ans/decoding.rs:27-47: the k-th state (in table order) of a symbol of weight w stands for x = w + k; it reads as many bits as bring
    x back into [size, 2 size) and lands on state (x << bits) - size + those bits.  [(symbol, bits_to_read, next_state_base)] per state."""
    size = 1 << size_log
    x = list(weights); nodes = []
    for s in spread_state_symbols(size_log, weights):
        bits = size_log - (x[s].bit_length() - 1)
        nodes.append((s, bits, (x[s] << bits) - size)); x[s] += 1
    return nodes


def to_latent(a):
    """Numbers -> their order-preserving unsigned latents (unsigned: as is; signed: the sign bit flipped; floats: negative values with
    every bit flipped, the others with the sign bit flipped)."""
    a = np.ascontiguousarray(a); bits = a.dtype.itemsize * 8
    u = a.view({8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}[bits])
    mid = u.dtype.type(1 << (bits - 1))
    if a.dtype.kind == "u": return u.copy()
    if a.dtype.kind == "i": return u ^ mid
    return np.where(u & mid, ~u, u ^ mid).astype(u.dtype)


def decode_one_chunk_file(data, latent_bits):
    """A standalone file of ONE Classic / no-delta chunk -> (latents as Python ints, the variable's {"ans_size_log", "bins": [(weight,
    lower, offset_bits)]}).  Anything else in the file is an assertion failure: this is a model of one path, not a decoder."""
    r = Bits(data)
    assert r.read(32) == int.from_bytes(b"pco!", "little")
    assert r.read(8) == 3                      # standalone version
    r.read(8)                                  # uniform type
    r.read(1 + r.read(6)); r.align()           # n hint: a varint of (6 bits of length - 1, then the bits)
    major = r.read(8); assert major == 4; r.read(8)
    assert r.read(8) != 0                      # the chunk's number type
    n = r.read(24) + 1
    assert r.read(4) == 0, "Classic mode only"
    assert r.read(4) == 0, "no delta encoding only"
    size_log = r.read(4); n_bins = r.read(15)
    assert size_log <= 14 and n_bins <= 1 << size_log and not (n_bins == 1 and size_log > 0) and n_bins >= 1
    ob_bits = {8: 4, 16: 5, 32: 6, 64: 7}[latent_bits]   # enough bits for 0 .. latent_bits
    bins = []
    for _ in range(n_bins):
        w = r.read(size_log) + 1; lower = r.read(latent_bits); ob = r.read(ob_bits)
        assert ob <= latent_bits
        bins.append((w, lower, ob))
    r.align()
    nodes = decoder_nodes(size_log, [b[0] for b in bins])
    # the page: four final states, padding, then batch after batch (ANS bits of the batch, then its offsets), padding
    state = [r.read(size_log) for _ in range(INTERLEAVING)]
    r.align()
    mask = (1 << latent_bits) - 1
    out = []
    for start in range(0, n, BATCH_N):
        bn = min(BATCH_N, n - start)
        syms = []
        for i in range(bn):
            if n_bins == 1:
                syms.append(0); continue
            j = i % INTERLEAVING
            s, bits, base = nodes[state[j]]
            syms.append(s); state[j] = base + r.read(bits)
        for s in syms:
            _, lower, ob = bins[s]
            out.append((lower + r.read(ob)) & mask)   # lower.wrapping_add(offset)
    r.align()
    assert r.read(8) == 0 and r.pos == r.n, "terminator, then nothing"
    return out, {"ans_size_log": size_log, "bins": bins}
