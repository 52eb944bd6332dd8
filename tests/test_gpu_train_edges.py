"""-m gpu: the training step of the encoder (enc_train_kernel, enc_train_big_kernel: train_var and train_finish) at its edges.

The cases and the plain model that certifies them are in tests/train_edges_util.py and tests/train_model.py; tests/test_train_model.py
pins both on the CPU (model against oracle, every case on its edge and changed by its variant of the model, arrays that realise their
bin lists without the heapsort branch) before anything here runs.

  (a) exact ties between neighbouring candidates of the one-wave kernel, the tied pair on both sides of j = 64, 128 and 192 (the
      boundaries of a lane's four slots and of nq), inside a slot and at the last of 256 bins; 8, 16, 32 and 64-bit latents;
  (b) ties 64 apart in one lane (slots 0/1, 1/2 and 2/3) and 127 apart in different lanes of different slots;
  (c) the block kernel at level 12: the tied pair in one wave, across waves 0 and 1 (127 apart, and 64 apart), across waves 0 and 15, with
      the deciding step in the first 64 bins, below 1024 and beyond; histograms of 257, 1023, 1024, 1025, 4095 and 4096 bins.  A tie of
      one thread with itself, 1024 candidates apart, cannot be made exact: the two last bins would need lengths that differ by 1024 and
      are both powers of two, which only 1024 and 2048 are, and that pair loses to 2048 + 1024 by one bin's metadata;
  (d) bin lists of at most 256 bins through the block kernel (level 9), and level-12 calls that mix chunks too short for it with big ones;
  (e) the single-bin and the trivial-offsets shortcut at f32 equality and one count beyond, both at once, and all bins trivial but one, at
      16, 32 and 64 bits;
  (f) quantize_weights: a float weight of k + 0.5, both repair loops, a surplus cut off at zero and all-even weights down to (1, [1, 1]) at
      16, 32 and 64 bits, a zero total surplus with a full table, the table estimate clamped by the number of latents;
  (g) an int-mult secondary with 200 distinct values (at most 2^6 histogram bins in both kernels), a tie case as order-1 differences, and
      lookback chunks of 16, 32 and 64-bit numbers whose delta variable -- variable 0, 32-bit whatever the numbers are -- holds five tied
      triples, through both kernels;
  (h) should_fallback one byte under, at and one byte over equality.

Every chunk's bytes equal the oracle's, the chunk written by the DEVICE shows the bins, weights, offset bits and table size the model
predicts, and it decodes on the device bit for bit to the input.  Cases that share a config share one synchronous call.  The launched
kernels are checked PER CALL only: enc_train_kernel is launched for every call (it returns at once on a chunk that is not its own), and
enc_train_big_kernel is in the profile exactly when the model says SOME chunk of the call has more than 2^8 histogram bins.  That does not
say which kernel trained which chunk -- a chunk sent to the wrong kernel would show in its bytes only where the two differ -- and in most
calls all chunks take one route; the level-12 mix is the one call in which both kernels train chunks side by side.  Nothing is skipped."""
import collections
import ctypes as C
import functools

import pytest

import gpu_util as U
import oracle_lib as O
import train_edges_util as E
import train_model as M
from pcodec_amd import _lib as G
from test_gpu_width_paths import decode_call, encode_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


@functools.lru_cache(maxsize=None)
def want(name):
    """(the standalone header the oracle writes in front of the case's chunk, the oracle's chunk), once."""
    c = E.BY_NAME()[name]
    x = E.numbers(name)
    f = O.simple_compress(x, O.make_config(enable_8_bit=True, **c.kw))
    k = U.standalone_header_len(x.size)
    return f[:k], f[k:-1]


@functools.lru_cache(maxsize=None)
def predicted(name):
    return E.predicted_chunk(E.BY_NAME()[name])


def config_key(c):
    return tuple(sorted(c.kw.items()))


def by_config(cases):
    groups = collections.OrderedDict()
    for c in cases:
        groups.setdefault(config_key(c), []).append(c)
    return list(groups.values())


def is_big(c):
    return M.choose_unoptimized_bins_log(c.kw["level"], E.numbers(c.name).size) > 8


def check_chunks(cases, chunks):
    bad = [c.name for c, got in zip(cases, chunks) if got != want(c.name)[1]]
    shown_bad = []
    for c, got in zip(cases, chunks):
        info, bins = O.inspect_first_chunk(want(c.name)[0] + got + b"\0")
        if E.shown_chunk(info, bins) != predicted(c.name):
            shown_bad.append(c.name)
    assert not bad and not shown_bad, (len(bad), bad[:6], len(shown_bad), shown_bad[:6])


def run_group(cases):
    """One synchronous call over cases of ONE config: bytes, the plan the device wrote, the training kernels launched, the round trip."""
    assert len(by_config(cases)) == 1
    arrays = [E.numbers(c.name) for c in cases]
    chunks, names = encode_call(arrays, G.make_config(enable_8_bit=True, **cases[0].kw))
    check_chunks(cases, chunks)
    assert "enc_train_kernel" in names and ("enc_train_big_kernel" in names) == any(is_big(c) for c in cases), (cases[0].name, names)
    decode_call(chunks, arrays)
    return chunks


@pytest.mark.parametrize("section", list(E.SECTIONS))
def test_every_case_trains_the_plan_the_model_predicts(L, section):
    cases = [c for c in E.section(section) if c is not None]
    assert cases
    failed = []                       # (every config's call runs, so that one report names every case that is wrong)
    for group in by_config(cases):
        try:
            run_group(group)
        except AssertionError as e:
            failed.append((group[0].name, str(e)[:600]))
    assert not failed, failed


def test_one_bin_list_through_both_kernels(L):
    """(d) the level-8 twin of every level-9 case holds the same numbers' bin list: the one-wave kernel and the block kernel each write the
    plan the model predicts for their level (the table estimate, and with it a bin's metadata cost, differs by one)."""
    pairs = [(E.BY_NAME()[c.name.replace("d-", "a-" if "triples" in c.name else "b-", 1)], c) for c in E.section("d")]
    assert len(pairs) == 7
    for small, big in pairs:
        assert not is_big(small) and is_big(big)
        assert [(lo, hi) for _, lo, hi in small.bins] == [(lo, hi) for _, lo, hi in big.bins]     # (the count per value may differ)
    run_group([s for s, _ in pairs])
    run_group([b for _, b in pairs])


def level12_mix():
    """[(label, numbers)]: every Classic level-12 case, the big ones of (c) and (f), and between them prefixes of 32-bit cases of (a), (b)
    and (e) that level 12 gives at most 2^8 histogram bins (fewer than 1024 numbers: 300, 700 and 1023) or exactly 2^9 (1024)."""
    big = [c for c in E.all_cases() if c.kw == E.classic(12)]
    small = [c for c in E.section("a") + E.section("b") + E.section("e") if c is not None and c.bits == 32]
    out = []
    for i, c in enumerate(big):
        s = small[i % len(small)]
        k = (300, 700, 1023, 1024)[i % 4]
        out += [(c.name, E.numbers(c.name)), (f"{s.name}[:{k}]", E.numbers(s.name)[:k])]
    return out


@functools.lru_cache(maxsize=None)
def level12_wants():
    return tuple(U.oracle_chunk(a, O.make_config(enable_8_bit=True, **E.classic(12))) for _, a in level12_mix())


def test_short_and_big_chunks_in_one_level_12_call_synchronous_and_asynchronous(L):
    """(d) one batched call at level 12 over chunks for both training kernels: the synchronous form, then the asynchronous one (results ==
    NULL, every kernel launched for every chunk); both give the oracle's level-12 bytes."""
    import torch
    labels = [name for name, _ in level12_mix()]
    arrays = [a for _, a in level12_mix()]
    bigs = [M.choose_unoptimized_bins_log(12, a.size) > 8 for a in arrays]
    assert sum(bigs) >= 10 and len(bigs) - sum(bigs) >= 6 and {a.size for a, b in zip(arrays, bigs) if not b} == {300, 700, 1023}
    cfg = G.make_config(enable_8_bit=True, **E.classic(12))
    wants = level12_wants()
    chunks, names = encode_call(arrays, cfg)
    assert [n for n, got, w in zip(labels, chunks, wants) if got != w] == []
    assert "enc_train_kernel" in names and "enc_train_big_kernel" in names
    decode_call(chunks, arrays)
    s = U.Staged(L, arrays)
    tasks = s.enc_tasks()
    G.check(L.pco_gfx_compress_chunks(s.k, U.ptr(tasks), C.byref(cfg), None, s.d_res.data_ptr(), None))
    torch.cuda.synchronize()
    res = s.results()
    assert (res["status"] == 0).all(), res["status"]
    got = s.slot_bytes(res["n_out"])
    assert [n for n, g, w in zip(labels, got, wants) if g != w] == []
