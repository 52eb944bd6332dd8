"""CPU: the rows of offset_edges_util.py cover what they claim, and offset_reader_model.py -- the decoders' offset readers restated from
their own dword and byte arithmetic -- reproduces the true fields of every row, whatever stands in the 16 bytes behind the chunk.

  * coverage: every k, every start residue of a full batch, the last-batch sizes, the register seams of trail_section, the bin counts, the
    two-variable rows on either side of kFlFast2 / kFlTriv2, need_bytes 2048 / 2052, the safe-load tails, the general kernel's sh + ob
    edges -- computed from the layouts; taking any one group of rows away leaves something uncovered;
  * every row is a valid chunk (the oracle decodes it to the input) whose fields are populated up to their top bit;
  * every MUTANT of the model (one-place wrong readings: a window one dword short, a register seam moved by a dword, ...) changes the answer
    of at least one row, and the two HARMLESS ones change none;
  * the constants the model and the rows are written with are read from the kernel sources: a moved threshold fails here and does not
    quietly test something else."""
import os
import re

import pytest

import gpu_util as U
import offset_edges_util as E
import offset_reader_model as M
import oracle_lib as O
import pack_layout_model as P
from pcodec_amd import _lib as G

CSRC = os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "csrc")
FILLS = (0x00, 0xFF)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _has(text, pattern, what):
    m = re.search(pattern, text)
    assert m, f"the kernel sources no longer say {pattern!r} ({what}): re-derive offset_reader_model.py and the rows of offset_edges_util.py"
    return m


@pytest.mark.parametrize("width", E.WIDTHS)
def test_the_rows_cover_every_edge_and_no_group_is_spare(width):
    bs = E.built(width)
    assert E.missing(width, bs) == []
    spare = []
    for g in E.GROUPS:
        if g == "tail": continue   # (the last item of many rows has a safe-load tail; the group only makes sure both kinds are there)
        rest = [b for b in bs if b.group != g]
        if len(rest) < len(bs) and not E.missing(width, rest): spare.append(g)
    assert not spare, f"u{width}: coverage() does not notice when these groups are deleted: {spare}"
    # ... and within a group: any one k of the sweeps, one seam, one of the 2048 / 2052 pair
    for k in E.ks(width, E.K_TRAIL):
        assert E.missing(width, [b for b in bs if not (b.group in ("res", "last") and E.exact(b, 1, k))]), (width, k)
    for b in bs:
        if b.group == "wide" and E.exact(b, 1, 64): continue   # (the 2048 rows carry k = 64 too,
        if b.row.label.startswith("last=256 k=64"): continue   #  and every full batch of theirs off residue 0 reaches dword 512)
        if b.group in ("nd", "2048", "wide", "general", "lb"):
            assert E.missing(width, [x for x in bs if x is not b]), (width, b.row.label)


@pytest.mark.parametrize("width", E.WIDTHS)
def test_every_row_is_a_valid_chunk_with_its_fields_populated(width):
    n_bytes = 0
    for b in E.built(width):
        x = b.row.array
        assert U.bits_equal(O.simple_decompress(b.file, x.dtype, cap=x.size + 8), x), b.row.label
        n_bytes += len(b.chunk)
        assert E.populated(b), (b.row.label, M.top_bit_share(b.chunk, b.layout))
    print(f"u{width}: {len(E.built(width))} rows, {n_bytes} bytes of chunks, {dict(E.coverage(E.built(width))['paths'])}")


def disagreements(b, mutants=(), fills=FILLS, stop=True):
    """[(reader, variable, batch, fill)] where a model function's answer differs from the true fields of row b."""
    out = []
    truth = {}
    for fill in fills:
        mem = M.Mem(b.chunk, fill)
        for name, v, bi, fn in E.readers(b):
            if (v, bi) not in truth: truth[(v, bi)] = M.true_fields(b.chunk, b.layout, v, bi)
            if fn(mem, mutants) != truth[(v, bi)]:
                out.append((name, v, bi, fill))
                if stop: return out
    return out


@pytest.mark.parametrize("width", E.WIDTHS)
def test_the_model_reproduces_the_true_fields_of_every_row(width):
    seen = set()
    for b in E.built(width):
        bad = disagreements(b, stop=False)
        assert not bad, (b.row.label, bad[:6])
        seen |= {name for name, _, _, _ in E.readers(b)}
    want = {"expand", "trail_general", "general", "trail_fast[pair]", "trail_fast[pair2t]", "trail_fast[pair2]"}
    assert seen == want, (width, sorted(seen ^ want))


# which rows can show a mutant at all (the reader it sits in)
MUTANT_WIDTHS = {"no_fetch_beyond_2048": (64,), "bfe_width_mod_32": (32,), "window_path_at_17": (32, 64), "no_second_word": (64,), "mask_at_64": (64,)}


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_revealed(mutant):
    revealed = []
    for width in MUTANT_WIDTHS.get(mutant, E.WIDTHS):
        for b in E.built(width):
            if len(revealed) >= 8: break   # (enough to name in a failure message)
            for name, v, bi, fill in disagreements(b, (mutant,)):
                revealed.append(f"u{width} {b.row.label}: {name}, {P.VAR_NAMES[v]} batch {bi}, fill {fill:#04x}")
    print(f"{mutant}: revealed by\n  " + "\n  ".join(revealed))
    assert revealed, f"no row's answer changes under {mutant}: the rows would let such a reader pass"


@pytest.mark.parametrize("mutant", M.HARMLESS)
def test_the_harmless_variants_change_no_field(mutant):
    """They move a bound inside bits no field uses (offset_reader_model.py says why): if a row's answer changes under one of them, a reader
    has come to depend on its slack."""
    for width in E.WIDTHS:
        for b in E.built(width):
            assert not disagreements(b, (mutant,)), (mutant, width, b.row.label)


def test_the_constants_are_the_sources():
    fast, kern, trail, host = _src("decode_fast.hip"), _src("decode_kernel.hip"), _src("decode_trail.hip"), _src("pco_gfx.hip")
    # the expanders' limits: 64 bins, offsets of up to 16 bits; the straight-line bodies' 7 / 15 / 7
    assert int(_has(fast, r"constexpr uint32_t kTrailMaxBins = (\d+);", "bins in a wave's registers").group(1)) == M.kTrailMaxBins == E.kTrailMaxBins
    assert int(_has(trail, r"nb1 > kTrailMaxBins \|\| mo1 > (\d+) \|\|", "the expanders' widest offset").group(1)) == M.kWindowMaxOb == E.kTrailMaxOb
    assert int(_has(fast, r"vinfo\[1\]\.n_bins <= kTrailMaxBins && vinfo\[1\]\.max_ob <= (\d+) &&", "the walker's mark").group(1)) == E.kTrailMaxOb
    assert int(_has(trail, r"nb1 > 1 && mo1 >= 1 && mo1 <= (\d+) && aligned\) fl \|= kFlFast;", "kFlFast").group(1)) == M.kFastMaxOb
    m = _has(trail, r"two && mo1 <= (\d+) && mo2 <= (\d+) && aligned\) fl \|= kFlFast2;", "kFlFast2")
    assert (int(m.group(1)), int(m.group(2))) == (M.kFast2MaxOb, M.kFast2MaxOb2)
    assert int(_has(trail, r"mo1 >= 1 && mo1 <= (\d+) && nb2 <= 1 && mo2 == 0 && aligned\) fl \|= kFlTriv2;", "kFlTriv2").group(1)) == M.kFast2MaxOb
    # trail_section: the reach, the register seams, the clamp
    assert int(_has(trail, r"nd = c\.max_ob <= 16 \? \(\(\(c\.start_live & 31u\) \+ cnt \* c\.max_ob \+ 31u\) >> 5\) \+ (\d+)u : 0u;", "nd").group(1)) == M.kTrailReach
    assert int(_has(trail, r"const uint32_t nd = \(\(\(c\.start_live & 31u\) \+ cnt \* c\.max_ob \+ 31u\) >> 5\) \+ (\d+)u;", "nd in stage B").group(1)) == M.kTrailReach
    _has(trail, r"if \(nd > 64\) it\.s1 = dword\(64 \+ lane\);\s*if \(nd > 128\) it\.s2 = dword\(128 \+ lane\);", "the register seams")
    _has(trail, r"if \(nd <= 64\) \{ w0 = bperm\(4u \* di, it\.s0\);", "the one-register window")
    _has(trail, r"return i < 64 \? a : \(i < 128 \? b : cc\);", "the three-register fetch")
    clamps = re.findall(r"last = \(uint32_t\)\(\((?:c\.)?src_len \+ (\d+)\) >> 2\)", trail)
    assert len(clamps) == 4 and set(clamps) == {str(M.kTrailClamp)}, clamps
    # dec_expand_kernel: the stage, the reach, the dwords 512.. fetch, the window path, the tail
    assert int(_has(fast, r"constexpr uint32_t kExpStgDwords = (\d+);", "the stage").group(1)) == M.kExpStgDwords
    reaches = re.findall(r"need_bits \+ 31u\) / 32u\) \* 4u \+ (\d+)u;", fast)
    assert len(reaches) == 2 and set(reaches) == {str(M.kExpReach)}, reaches
    _has(fast, r"if \(need_bytes > 2048 && lane < 2\)", "the dwords 512.. fetch")
    _has(fast, r"if \(byte0 \+ off \+ 32 <= src_len \+ 16\)", "the direct / safe-load tail")
    assert int(_has(fast, r"if \(need_bits != 0 && max_ob <= (\d+)\) \{", "the window path").group(1)) == M.kWindowMaxOb
    _has(fast, r"val = ob\[k\] >= 64 \? v64 :", "64-bit fields unmasked"); _has(fast, r"if \(ob\[k\] >= 32\) val = ", "32-bit fields unmasked")
    # pco_decode_kernel
    _has(kern, r"if \(sh \+ ob\[k\] > 64\) val \|= load_u64_le_safe\(src, byte \+ 8, src_len \+ 16\) << \(64 - sh\);", "the second load")
    _has(kern, r"if \(ob\[k\] < 64\) val &= ", "the mask")
    # the selection the rows' paths are predicted with, and the call size arrangement (a) is built on
    assert int(_has(fast, r"constexpr uint32_t kFastMaxBins = (\d+);", "kFastMaxBins").group(1)) == E.kFastMaxBins
    assert int(_has(fast, r"nb > kFastMaxBins \|\| a > (\d+)\) too_big = true;", "kFastMaxAns").group(1)) == E.kFastMaxAns
    off = int(_has(fast, r"constexpr uint32_t kGrpTblOff = (\d+);", "kGrpTblOff").group(1))
    m = _has(fast, r"kGrpBytes = KQ == 8 \? (\d+)u : (\d+)u;", "kGrpBytes")
    assert (int(m.group(1)) - off, int(m.group(2)) - off) == (E.K8_TABLE_BYTES, E.K4_TABLE_BYTES)
    assert int(_has(host, r"constexpr uint32_t kTrailMinChunks = (\d+);", "kTrailMinChunks").group(1)) == E.kTrailMinChunks
