"""-m gpu: the device decoders on legal tANS / bin tables that no reference encoder would write, and on every invalid table header.

The decoders pick their path on ans_size_log, n_bins, the largest offset bits and the table bytes (decode_fast.hip: the 8-chunk walker, the
4-chunk walker, the trailing expanders, the hand-over to pco_decode_kernel; decode_kernel.hip: tables in LDS or in global scratch), and until
now only tables out of the reference's training reached them.  The streams come from the TEST-ONLY generator (TestEncSpec's tbl_* fields,
oracle/pco_oracle_testenc.hpp); the reference is the input array and the oracle's decoder, nothing else.

Which decoder took a chunk: the device does not report a task's internal retry status (kStatusRetryK4 / kStatusRetryLegacy never leave
the plan), so the threshold rows PREDICT the path on the host from the constants named below -- read from the kernel sources, so a changed
constant fails here instead of quietly moving a row to another path -- and assert that both sides of every threshold are in the grid.  What
the device does show is asserted where it exists: a synchronous call runs pco_decode_kernel a SECOND time exactly when a task's tables are
beyond the LDS budget (profile), and a call of 1024+ chunks reports what the trailing expanders took (pco_gfx_trail_marked).

Every call: status OK, bit-exact numbers, the guard bytes behind every output intact.  A valid foreign stream is never Unsupported, and the
module's skip budget is zero: every stream it generates is counted, and test_every_generated_stream_was_decoded compares that with the
streams the device decoded with status OK."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import foreign_tables_util as F
import gpu_util as U
import oracle_lib as O
from pcodec_amd import _lib as G
from test_foreign_tables import ARRANGEMENTS, arrangement_data

pytestmark = pytest.mark.gpu

GUARD = 0xAB
WIDTHS = (8, 16, 32, 64)
UINT = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
NAME = {8: "u8", 16: "u16", 32: "u32", 64: "u64"}
import hashlib
GENERATED, DECODED = set(), set()   # digests of the valid streams this module generated / of those a device call decoded with status OK

CSRC = os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, f"the kernel sources no longer say {pattern!r}: re-derive the threshold rows of this module"
    return int(m.group(1))


# ---- the constants the thresholds below come from (a changed constant fails test_the_constants_the_rows_are_derived_from)
_fast, _kern, _trail, _host = _src("decode_fast.hip"), _src("decode_kernel.hip"), _src("decode_trail.hip"), _src("pco_gfx.hip")
kTrailMaxBins = _const(_fast, r"constexpr uint32_t kTrailMaxBins = (\d+);")
kFastMaxBins = _const(_fast, r"constexpr uint32_t kFastMaxBins = (\d+);")
kGrpTblOff = _const(_fast, r"constexpr uint32_t kGrpTblOff = (\d+);")
kGrpBytes8 = _const(_fast, r"kGrpBytes = KQ == 8 \? (\d+)u : \d+u;")
kGrpBytes4 = _const(_fast, r"kGrpBytes = KQ == 8 \? \d+u : (\d+)u;")
kFastMaxAns = _const(_fast, r"nb > kFastMaxBins \|\| a > (\d+)\) too_big = true;")
kTrailMaxOb = _const(_trail, r"nb1 > kTrailMaxBins \|\| mo1 > (\d+) \|\|")
_lds = {}   # decode_kernel.hip's chain of LDS offsets, each "constexpr uint32_t kLdsX = <number or earlier name> [+ number];", evaluated in order
for _name, _expr in re.findall(r"constexpr uint32_t (kLds\w+) = ([\w +]+);", _kern):
    _lds[_name] = sum(int(t) if t.isdigit() else _lds[t] for t in _expr.split(" + "))
assert "kLdsFixed" in _lds, "decode_kernel.hip no longer defines kLdsFixed: re-derive the LDS budget rows of this module"
kLdsFixed = _lds["kLdsFixed"]       # where the tANS tables start in pco_decode_kernel's LDS
kDecodeLdsBytes = _const(_host, r"g_decode_lds_bytes = (\d+) \* 1024;") * 1024
kTrailMinChunks = _const(_host, r"constexpr uint32_t kTrailMinChunks = (\d+);")
kMaxAnsBits = _const(_src("pco_dev.h"), r"constexpr uint32_t kMaxAnsBits = (\d+);")
K8_TABLE_BYTES = kGrpBytes8 - kGrpTblOff     # what one chunk's tables may take in the 8-chunk walker's slice
K4_TABLE_BYTES = kGrpBytes4 - kGrpTblOff     # ... in the 4-chunk walker's
LDS_TABLE_BUDGET = kDecodeLdsBytes - kLdsFixed   # pco_decode_kernel: tables beyond this are built in global scratch


def test_the_constants_the_rows_are_derived_from():
    assert (kTrailMaxBins, kFastMaxBins, kFastMaxAns, kTrailMaxOb, kMaxAnsBits, kTrailMinChunks) == (64, 256, 12, 16, 14, 1024)
    assert (K8_TABLE_BYTES, K4_TABLE_BYTES) == (4272, 9264)
    assert kLdsFixed == 5472 and LDS_TABLE_BUDGET == 10912
    # the n_bins / ans_size_log / offset-bits grids of this module sit on both sides of each of them
    assert {kTrailMaxBins - 1, kTrailMaxBins, kTrailMaxBins + 1, kFastMaxBins - 1, kFastMaxBins, kFastMaxBins + 1, 1 << kMaxAnsBits} <= set(N_BINS)
    assert {kFastMaxAns - 1, kFastMaxAns, kFastMaxAns + 1, kMaxAnsBits} <= set(ANS_LOGS) and {kTrailMaxOb - 1, kTrailMaxOb, kTrailMaxOb + 1} <= set(MAX_OBS)


N_BINS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 4096, 16384)
ANS_LOGS = (O.TBL_ANS_MIN, 10, 11, 12, 13, 14)
MAX_OBS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64)


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


# ------------------------------------------------------------------------------------------------ host-side prediction
def fast_table_bytes(info):
    """decode_fast.hip, fast_front_impl: entries + bin 0's offset bits per present variable."""
    return sum((4 << info.ans_size_log[v]) + 8 for v in range(3) if info.var_present[v])


def general_table_bytes(info, bits):
    """decode_kernel.hip, var_table_bytes: nodes, lowers, offset bits, cumulative weights, each rounded up to 8 bytes."""
    total = 0
    for v in range(3):
        if not info.var_present[v]: continue
        a, nb = info.ans_size_log[v], info.n_bins[v]
        lb = 4 if v == 0 or (v == 1 and info.mode_kind == 4) else bits // 8
        total += (4 << a) + ((nb * lb + 7) & ~7) + ((nb + 7) & ~7) + (((nb + 1) * 4 + 7) & ~7)
    return total


def predict(data, bits):
    """(walker, global_tables): which decoder the selection in decode_fast.hip gives a one-chunk file ("k8", "k4" or "general"), and whether
    pco_decode_kernel has to build its tables in global scratch."""
    info, _ = O.inspect_first_chunk(data, max_bins=1 << 14)
    nbs = [info.n_bins[v] for v in range(3) if info.var_present[v]]; als = [info.ans_size_log[v] for v in range(3) if info.var_present[v]]
    t = fast_table_bytes(info)
    general = (info.mode_kind == 4 or info.delta_kind == 3 or max(nbs) > kFastMaxBins or max(als) > kFastMaxAns or t > K4_TABLE_BYTES
               or (info.delta_kind == 2 and info.mode_kind != 0))
    walker = "general" if general else ("k4" if t > K8_TABLE_BYTES else "k8")
    return walker, walker == "general" and general_table_bytes(info, bits) > LDS_TABLE_BUDGET


# ------------------------------------------------------------------------------------------------ call helpers
def _slots(sizes, extra=16, align=16):
    offs, pos = [], 0
    for s in sizes:
        offs.append(pos); pos += (s + extra + align - 1) // align * align
    return offs, pos


def decode_files(L, files, want, bad=None, asynchronous=False, bare=False):
    """One pco_gfx_decompress_chunks call over whole one-chunk files (TASK_HAS_FILE_HEADER; with `bare`, over the chunk inside each file, flags 0:
    only such tasks are candidates of the trailing expanders) into one GUARD-filled output buffer.  Every task
    not in `bad` ({index: status}) must be OK, bit-exact and have consumed its file; the bad ones report exactly their status; nothing is
    written past any chunk's numbers.  Returns the launches of the call."""
    import torch
    bad = bad or {}
    k = len(files)
    digests = [hashlib.sha256(f).digest() for f in files]
    if bare: files = [f[U.standalone_header_len(a.size):-1] for f, a in zip(files, want)]
    s_offs, s_total = _slots([len(f) for f in files], extra=64)
    host_src = np.zeros(s_total, np.uint8)
    for o, f in zip(s_offs, files):
        host_src[o:o + len(f)] = np.frombuffer(f, np.uint8)
    src = torch.from_numpy(host_src).cuda()
    d_offs, d_total = _slots([a.nbytes for a in want])
    out = torch.full((d_total,), GUARD, dtype=torch.uint8, device="cuda")
    tasks = (G.DecodeTask * k)(*[G.DecodeTask(src.data_ptr() + s_offs[i], len(files[i]), out.data_ptr() + d_offs[i], want[i].size,
                                              G.DTYPE_BYTE[want[i].dtype.name], 0 if bare else G.TASK_HAS_FILE_HEADER) for i in range(k)])
    L.pco_gfx_profile_begin()
    if asynchronous:
        d_res = torch.zeros(k * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
        G.check(L.pco_gfx_decompress_chunks(k, tasks, None, d_res.data_ptr(), None))
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(U.RES_DT)
        status = [int(r["status"]) for r in res]; n_out = [int(r["n_out"]) for r in res]; consumed = [int(r["consumed"]) for r in res]
    else:
        r = (G.TaskResult * k)()
        rc = L.pco_gfx_decompress_chunks(k, tasks, r, None, None)
        assert (rc != 0) == bool(bad), rc
        status = [int(x.status) for x in r]; n_out = [int(x.n_out) for x in r]; consumed = [int(x.consumed) for x in r]
    launches = U.profile_launches(L)
    host = out.cpu().numpy()
    for i, a in enumerate(want):
        if i in bad:
            assert status[i] == bad[i], (i, "status", status[i], "wanted", bad[i])
        else:
            assert status[i] == G.ST_OK, (i, a.dtype, a.size, "status", status[i])
            assert n_out[i] == a.size and consumed[i] == len(files[i]), (i, n_out[i], a.size, consumed[i], len(files[i]))
            assert U.bits_equal(host[d_offs[i]:d_offs[i] + a.nbytes].view(a.dtype), a), (i, a.dtype, a.size)
            DECODED.add(digests[i])
        end = d_offs[i + 1] if i + 1 < k else d_total
        assert (host[d_offs[i] + a.nbytes:end] == GUARD).all(), ("written past the chunk's numbers", i, a.dtype, a.size)
    return launches


def valid(x, kw, label):
    """A foreign stream that is what it says (n_bins / ans_size_log read back) and that the oracle decodes to the input."""
    data = O.test_encode(x, **kw)
    F.check_meta(data, O.test_encode(x, **F.strip_tbl(kw)), kw, label)
    assert U.bits_equal(O.simple_decompress(data, x.dtype, cap=x.size + 8), x), label
    GENERATED.add(hashlib.sha256(data).digest())
    return data


def standalone(f, x, label):
    """The host standalone entry point on one file."""
    assert U.bits_equal(U.gpu_simple_decompress(f, x.dtype, x.size), x), label
    DECODED.add(hashlib.sha256(f).digest())


def general_kernel_runs(launches, bits):
    return sum(1 for n in launches if n == f"pco_decode_kernel<{NAME[bits]}>")


# ------------------------------------------------------------------------------------------------ one variable: every threshold, both sides
def one_variable_rows(bits):
    """[(label, array, kwargs)]: n_bins 1 .. 2^14 at the smallest ans_size_log; ans_size_log min .. 14 on few bins; the largest offset bits
    0 .. the latent's width on ONE bin beside narrow ones; and the combinations the walkers' table slices turn on."""
    dt = (UINT[bits], {8: np.int8, 16: np.int16, 32: np.float32, 64: np.float64}[bits])
    P = O.TBL_PRIMARY
    small = F.clustered(dt[0], 3000, seed=100 + bits, clusters=5)
    big = F.clustered(dt[1], 17000, seed=200 + bits)
    rows = []
    for nb in N_BINS:
        x = big if nb >= 4096 else small
        if nb == 1:
            rows.append((f"n_bins=1 full width", x, dict(tbl_vars=P, tbl_n_bins=1, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=bits)))
            continue
        if nb in (2, 3):   # fewer bins than training gives: three values, two or three trained bins, kept
            x = UINT[bits](7) + (np.random.default_rng(nb).integers(0, nb, 3000) * 50).astype(UINT[bits])
            rows.append((f"n_bins={nb}", x, dict(tbl_vars=P, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_shuffle=True, tbl_seed=nb)))
            continue
        rows.append((f"n_bins={nb}", x, dict(tbl_vars=P, tbl_n_bins=nb, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_seed=nb, tbl_shuffle=bool(nb % 2),
                                            tbl_weight_style=O.TBL_W_RANDOM if nb % 2 else O.TBL_W_PROPORTIONAL)))
    rows.append(("n_bins=16384 all ones", big, dict(tbl_vars=P, tbl_n_bins=16384, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_ONES, tbl_seed=1)))
    for i, a in enumerate(ANS_LOGS):
        style = (O.TBL_W_PROPORTIONAL, O.TBL_W_FLAT, O.TBL_W_INVERSE, O.TBL_W_RANDOM)[i % 4]
        rows.append((f"ans_size_log={a}", small, dict(tbl_vars=P, tbl_ans_size_log=a, tbl_weight_style=style, tbl_seed=a)))
        if a != O.TBL_ANS_MIN:
            rows.append((f"ans_size_log={a} n_bins=256", small, dict(tbl_vars=P, tbl_ans_size_log=a, tbl_n_bins=256, tbl_weight_style=O.TBL_W_INVERSE, tbl_seed=a, tbl_shuffle=True)))
    narrow = UINT[bits](9) + (np.random.default_rng(bits).integers(0, 6, 3000) * 3).astype(UINT[bits])   # six single-value bins: 0 offset bits each
    for ob in sorted({min(o, bits) for o in MAX_OBS}):
        rows.append((f"max offset bits={ob} beside 0-bit bins", narrow, dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_ONE, tbl_ob_value=ob, tbl_seed=ob, tbl_ans_size_log=O.TBL_ANS_MIN)))
        rows.append((f"max offset bits={ob} wrapped", small, dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_ONE, tbl_ob_value=ob, tbl_seed=ob + 1, tbl_lower_wrap=True)))
    rows.append(("0-bit beside full-width bins", small, dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_ALTERNATE, tbl_n_bins=40, tbl_seed=7, tbl_lower_wrap=True)))
    rows.append(("every bin full width, wrapped", small, dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=bits, tbl_lower_wrap=True, tbl_seed=8)))
    # a variable WITHOUT latents in the body keeps an empty table (n_bins == 0), whatever the spec asks: valid, and decoded
    rows.append(("empty table, order 3 over 3 numbers", np.arange(3, dtype=np.int64).astype(UINT[bits]) * 7, dict(tbl_vars=O.TBL_ALL, tbl_ans_size_log=12, tbl_n_bins=50, delta=O.TE_DELTA_CONSECUTIVE, order=3)))
    rows.append(("64 bins, ans_size_log 10", small, dict(tbl_vars=P, tbl_n_bins=kTrailMaxBins, tbl_ans_size_log=10, tbl_seed=9)))      # the last table an 8-chunk slice holds
    rows.append(("65 bins, ans_size_log 11", small, dict(tbl_vars=P, tbl_n_bins=kTrailMaxBins + 1, tbl_ans_size_log=11, tbl_seed=10)))  # the 4-chunk walker's
    return [(f"{NAME[bits]} {lab}", x, dict(kw, mode=O.MODE_CLASSIC)) for lab, x, kw in rows]


@pytest.mark.parametrize("bits", WIDTHS)
def test_one_variable_thresholds(L, bits):
    """Every n_bins / ans_size_log / offset-bits threshold from both sides on a Classic chunk of each width: through the host standalone
    entry point one file at a time, and through pco_gfx_decompress_chunks in one small synchronous call -- then the same call once more
    without the chunks whose tables are beyond the LDS budget.  Which walker takes a row is PREDICTED (see the module's text: the device
    does not say); the prediction must cover the 8-chunk walker, the 4-chunk walker and the general kernel, with LDS and with global
    tables.  Shown by the device: pco_decode_kernel runs a second time in the first call (global tables) and once in the second."""
    rows = one_variable_rows(bits)
    files = [valid(x, kw, lab) for lab, x, kw in rows]
    paths = [predict(f, bits) for f in files]
    assert {p[0] for p in paths} == {"k8", "k4", "general"}, paths
    assert {p[1] for p in paths if p[0] == "general"} == {False, True}, paths
    for (lab, x, kw), f in zip(rows, files):
        standalone(f, x, lab)
    launches = decode_files(L, files, [r[1] for r in rows])
    assert general_kernel_runs(launches, bits) == 2, launches
    lds = [i for i, p in enumerate(paths) if not p[1]]
    launches = decode_files(L, [files[i] for i in lds], [rows[i][1] for i in lds])
    assert general_kernel_runs(launches, bits) == 1, launches


# ------------------------------------------------------------------------------------------------ several variables
def straddle(x, kw, bits, over):
    """Foreign (ans_size_log, n_bins) for the PRIMARY of a chunk that the general kernel takes (n_bins beyond kFastMaxBins where nothing else sends it there), chosen so that the
    chunk's total table bytes are the largest value <= LDS_TABLE_BUDGET (over=False) or the smallest value beyond it (over=True)."""
    plain = O.test_encode(x, **kw)
    info, _ = O.inspect_first_chunk(plain, max_bins=1 << 14)
    nb_min = max(int(info.n_bins[1]), 2, 0 if predict(plain, bits)[0] == "general" else kFastMaxBins + 1)   # (lookback under int-mult goes there whatever its tables)
    best = None
    for a in (8, 9, 10, 11):
        for nb in range(nb_min, (1 << a) + 1):
            info.ans_size_log[1] = a; info.n_bins[1] = nb
            t = general_table_bytes(info, bits)
            if (t > LDS_TABLE_BUDGET) == over and (best is None or (t < best[0] if over else t > best[0])):
                best = (t, a, nb)
    # the tables grow in steps of 8 bytes (every part is rounded up to 8): the budget itself or one step under it, one or two steps over it
    assert best is not None and (0 < best[0] - LDS_TABLE_BUDGET <= 16 if over else 0 <= LDS_TABLE_BUDGET - best[0] <= 8), best
    return dict(kw, tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=best[1], tbl_n_bins=best[2], tbl_seed=best[2], tbl_shuffle=True), best[0]


TWO_VAR = {8: [(np.uint8, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=5))],
           16: [(np.int16, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=7)), (np.float16, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=4))],
           32: [(np.int32, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=7)), (np.float32, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=12)),
                (np.float32, dict(mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25))],
           64: [(np.int64, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=1000)), (np.float64, dict(mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.01)),
                (np.float64, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=30))]}
VAR_SHAPES = [dict(tbl_ans_size_log=10, tbl_weight_style=O.TBL_W_RANDOM, tbl_seed=31, tbl_shuffle=True),
              dict(tbl_ans_size_log=11, tbl_weight_style=O.TBL_W_INVERSE, tbl_ob_mode=O.TBL_OB_ALTERNATE, tbl_seed=32),
              dict(tbl_ans_size_log=13, tbl_weight_style=O.TBL_W_FLAT, tbl_ob_mode=O.TBL_OB_RANDOM, tbl_seed=33),
              dict(tbl_n_bins=65, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_seed=34), dict(tbl_n_bins=257, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_seed=35, tbl_shuffle=True),
              dict(tbl_n_bins=1024, tbl_ans_size_log=10, tbl_weight_style=O.TBL_W_ONES, tbl_seed=36), dict(tbl_n_bins=1)]


def lookback_data(bits, n):
    """A period of 37 random values plus one of four far-apart steps: under the reference's lookback search the residuals are a few distinct
    values, so the trained primary has a few bins of unequal weight (room for every foreign shape, and for every fault)."""
    r = np.random.default_rng(bits + 1)
    return (r.integers(0, 1 << bits, 37, dtype=np.uint64, endpoint=False)[np.arange(n) % 37] + r.choice([0, 8, 16, 24], n, p=[0.7, 0.15, 0.1, 0.05]).astype(np.uint64)).astype(UINT[bits])


def several_variable_rows(bits):
    rows = []
    for dt, kw in TWO_VAR[bits]:
        x = arrangement_data(dt, kw, n=5000, seed=bits)
        for vars_ in (O.TBL_PRIMARY, O.TBL_SECONDARY, O.TBL_PRIMARY | O.TBL_SECONDARY):
            for s in VAR_SHAPES:
                rows.append((f"{np.dtype(dt).name} two variables vars={vars_} {s}", x, dict(kw, tbl_vars=vars_, **s)))
        rows.append((f"{np.dtype(dt).name} two variables wrapped", x, dict(kw, tbl_vars=6, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=bits, tbl_lower_wrap=True, tbl_seed=37)))
        for over in (False, True):   # two variables at the LDS budget
            skw, t = straddle(x, kw, bits, over)
            rows.append((f"{np.dtype(dt).name} two variables, {t} table bytes", x, skw))
    # lookback: the delta variable's table too; with int-mult under it: three variables at the LDS budget
    lb = dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_LOOKBACK, window_n_log=8)   # (the reference's lookback search: residuals of a few far-apart values, a few bins)
    x = lookback_data(bits, 5000)
    for vars_ in (O.TBL_DELTA, O.TBL_PRIMARY, O.TBL_DELTA | O.TBL_PRIMARY):
        for s in VAR_SHAPES[:5]:
            rows.append((f"{NAME[bits]} lookback vars={vars_} {s}", x, dict(lb, tbl_vars=vars_, **s)))
    lb3 = dict(lb, window_n_log=4, lookback_seed=5, **TWO_VAR[bits][0][1])   # (a short window: a small delta-variable table, so that the primary alone can reach the budget byte by byte)
    x3 = arrangement_data(TWO_VAR[bits][0][0], TWO_VAR[bits][0][1], n=5000, seed=bits + 2)
    for over in (False, True):
        skw, t = straddle(x3, lb3, bits, over)
        rows.append((f"{NAME[bits]} three variables, {t} table bytes", x3, skw))
    rows.append((f"{NAME[bits]} three variables, all foreign", x3, dict(lb3, tbl_vars=O.TBL_ALL, tbl_ans_size_log=12, tbl_weight_style=O.TBL_W_RANDOM, tbl_seed=38, tbl_shuffle=True)))
    # Dict (its u32 primary) and Conv1
    for name, dt, kw in ARRANGEMENTS:
        if np.dtype(dt).itemsize * 8 != bits or not (kw["mode"] == O.MODE_TRY_DICT or kw.get("delta") == O.TE_DELTA_CONV1): continue
        xa = arrangement_data(dt, kw, n=5000, seed=bits + 3)
        for s in VAR_SHAPES:
            rows.append((f"{name} {s}", xa, dict(kw, tbl_vars=O.TBL_PRIMARY, **s)))
    if bits in (8, 32):
        dk = dict(mode=O.MODE_TRY_DICT, dict_first_appearance=True)
        xa = arrangement_data(UINT[bits], dk, n=5000, seed=bits + 4)
        for s in VAR_SHAPES:
            rows.append((f"dict {NAME[bits]} {s}", xa, dict(dk, tbl_vars=O.TBL_PRIMARY, **s)))
    if bits == 8:
        ck = dict(mode=O.MODE_TRY_INT_MULT, mode_u64=3, delta=O.TE_DELTA_CONV1, quantization=3, bias=0, weights=[8])
        xa = arrangement_data(np.uint8, ck, n=5000, seed=12)
        for s in VAR_SHAPES:
            rows.append((f"conv1 + int-mult u8 {s}", xa, dict(ck, tbl_vars=6, **s)))
    return rows


@pytest.mark.parametrize("bits", WIDTHS)
def test_several_variables_and_the_lds_budget(L, bits):
    """Two variables (int-mult, float-mult, float-quant) with foreign tables on the primary only, the secondary only and both; lookback with
    a foreign delta-variable table; Dict; Conv1; and chunks of two and of three variables whose total table bytes are the last value inside
    pco_decode_kernel's LDS budget and the first beyond it.  Standalone entry point and one synchronous batched call; then the batched call
    without the chunks beyond the budget: the second run of pco_decode_kernel (the pass with global table scratch) is gone."""
    rows = several_variable_rows(bits)
    files = [valid(x, kw, lab) for lab, x, kw in rows]
    paths = [predict(f, bits) for f in files]
    at_budget = [(lab, p) for (lab, _, _), p in zip(rows, paths) if "table bytes" in lab]
    assert len(at_budget) == 2 * (len(TWO_VAR[bits]) + 1) and all(p[0] == "general" for _, p in at_budget), at_budget
    assert [p[1] for _, p in at_budget] == [False, True] * (len(at_budget) // 2), at_budget
    for (lab, x, kw), f in zip(rows, files):
        standalone(f, x, lab)
    launches = decode_files(L, files, [r[1] for r in rows])
    assert general_kernel_runs(launches, bits) == 2, launches
    lds = [i for i, p in enumerate(paths) if not p[1]]
    assert len(lds) >= len(TWO_VAR[bits]) + 1
    launches = decode_files(L, [files[i] for i in lds], [rows[i][1] for i in lds])
    assert general_kernel_runs(launches, bits) == 1, launches


# ------------------------------------------------------------------------------------------------ calls of 1024+ chunks
FAULT_STREAMS = [("classic", dict(mode=O.MODE_CLASSIC), (1,)), ("two variables", None, (1, 2)),
                 ("lookback", dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_LOOKBACK, window_n_log=8), (0, 1))]


def fault_files(bits):
    """[(label, array, file)]: one stream per reference check (weights summing below / above 2^ans_size_log: ans/spec.rs:37-44; one bin with
    ans_size_log > 0, 2^ans_size_log < n_bins, ans_size_log 15, offset bits beyond the type: chunk_latent_var.rs:115-132; no bins but latents
    in the body: page_decompressor.rs:52) on each variable of a classic, a two-variable and a lookback chunk.  The oracle calls each one
    Corruption."""
    out = []
    for name, kw, vars_ in FAULT_STREAMS:
        dt, kw = (UINT[bits], kw) if kw is not None else TWO_VAR[bits][0]
        x = lookback_data(bits, 2000) if kw.get("delta") else (arrangement_data(dt, kw, n=2000, seed=bits + 7) if kw["mode"] != O.MODE_CLASSIC else F.clustered(dt, 2000, seed=bits + 7))
        for var in vars_:
            for fname, fault in O.TBL_FAULTS.items():
                f = O.test_encode(x, tbl_fault=fault, tbl_fault_var=var, **kw)
                with pytest.raises(O.OracleError) as ei:
                    O.simple_decompress(f, x.dtype, cap=x.size + 8)
                assert ei.value.kind == O.ERR_CORRUPTION, (name, var, fname)
                out.append((f"{NAME[bits]} {name} {F.VAR_NAMES[var]} {fname}", x, f))
    return out


@pytest.mark.parametrize("bits", WIDTHS)
def test_invalid_tables_are_corruption(L, bits):
    """Every invalid table header, on each present variable: ST_CORRUPTION exactly -- the oracle's kind -- from the standalone entry point
    and from pco_gfx_decompress_chunks, where each bad task fails alone between healthy neighbours."""
    faults = fault_files(bits)
    assert len(faults) == 5 * len(O.TBL_FAULTS)
    for lab, x, f in faults:
        with pytest.raises(G.PcoGfxError) as ei:
            U.gpu_simple_decompress(f, x.dtype, x.size)
        assert ei.value.status == G.ST_CORRUPTION, (lab, ei.value.status)
    good = [(lab, x, valid(x, kw, lab)) for lab, x, kw in one_variable_rows(bits)[::5]]
    mixed = []
    for i, fl in enumerate(faults):
        mixed += [good[i % len(good)], fl]
    mixed.append(good[0])
    decode_files(L, [m[2] for m in mixed], [m[1] for m in mixed], bad={2 * i + 1: G.ST_CORRUPTION for i in range(len(faults))})


@pytest.mark.parametrize("bits", WIDTHS)
def test_a_call_of_1024_chunks_and_more(L, bits):
    """At kTrailMinChunks the publishing walker and the trailing expanders run, and chunks predicted for the 4-chunk stage and for the general
    kernel sit in the same call (that those two stages took them is predicted only: their kernels are launched in every call, whatever it
    holds): foreign chunks of every one-variable and several-variable shape of this width interleaved with ordinary trained chunks
    (the D-trail rows of test_gpu_width_paths.py, whose candidates the expanders are proven to take there), and every invalid table among
    them failing alone.  The walk + expanders span ran (profile), the expanders took chunks (pco_gfx_trail_marked), among them foreign ones
    the host predicts as candidates (<= kTrailMaxBins bins, <= kTrailMaxOb offset bits, forced ans_size_log)."""
    from test_gpu_width_paths import decode_set
    foreign = [(lab, x, valid(x, kw, lab)) for lab, x, kw in one_variable_rows(bits) + several_variable_rows(bits)[::3] if x.size <= 6000]
    trained = [("trained", a, O.simple_compress(a, O.make_config(enable_8_bit=True, **kw))) for a, kw, _, _, _ in decode_set(bits, False, 100 + bits) + decode_set(bits, True, 200 + bits)]
    faults = fault_files(bits)
    assert sum(1 for _, _, f in foreign if expander_kind(f, bits) in (1, 2)) >= 6
    for pool in (trained, None):   # interleaved with ordinary chunks; then foreign chunks alone, so that what the expanders took IS foreign
        calls = []; bad = {}
        count = kTrailMinChunks + 64 + bits
        for i in range(count):
            if i % 23 == 11:
                bad[i] = G.ST_CORRUPTION; calls.append(faults[(i // 23) % len(faults)])
            elif i % 2 or pool is None:
                calls.append(foreign[(i // 2) % len(foreign)])
            else:
                calls.append(pool[(i // 2) % len(pool)])
        kinds = [0 if i in bad else expander_kind(c[2], bits) for i, c in enumerate(calls)]
        lower = sum(1 for k, c in zip(kinds, calls) if k in (1, 2) and len(c[2]) >= 48)
        upper = sum(1 for k in kinds if k)
        m0 = L.pco_gfx_trail_marked()
        launches = decode_files(L, [c[2] for c in calls], [c[1] for c in calls], bad=bad, bare=True)
        marked = L.pco_gfx_trail_marked() - m0
        print(f"{NAME[bits]}: {count} chunks ({'mixed' if pool else 'foreign only'}), {len(bad)} invalid, marked {marked} (candidates {lower}..{upper})")
        assert f"dec_walk+trail<{NAME[bits]}>" in launches, launches
        assert 0 < lower <= marked <= upper, (marked, lower, upper)


def expander_kind(f, bits):
    """test_gpu_width_paths.trail_kind (what the publishing walker's test makes of a chunk), for tables of ANY ans_size_log: the publishing
    walker is the 8-chunk one, so a chunk whose tables do not fit its slice is no candidate however few bins it has."""
    from test_gpu_width_paths import trail_kind
    return trail_kind(f) if predict(f, bits)[0] == "k8" else 0


# ------------------------------------------------------------------------------------------------ asynchronous form, pages
def test_asynchronous_calls_decode_tables_beyond_the_lds_budget(L):
    """include/pco_gfx.h, pco_gfx_decompress_chunks: an asynchronous call (results == NULL) cannot come back for a second pass, so it
    takes pco_decode_kernel's global table scratch up front: a chunk whose tANS tables are beyond the LDS budget decodes there in ONE run
    of the kernel, status OK -- it is never handed back and never Unsupported (only lookback with a delta'd secondary variable is)."""
    for bits in WIDTHS:
        rows = [r for r in one_variable_rows(bits) if "16384" in r[0] or "4096" in r[0] or "ans_size_log=14" in r[0] or "ans_size_log=13" in r[0]]
        files = [valid(x, kw, lab) for lab, x, kw in rows]
        assert all(predict(f, bits) == ("general", True) for f in files)
        launches = decode_files(L, files, [r[1] for r in rows], asynchronous=True)
        assert general_kernel_runs(launches, bits) == 1, launches


def test_pages_of_foreign_chunks(L):
    """pco_gfx_decompress_pages on multi-page wrapped chunks whose ChunkMeta carries foreign tables (one ChunkMeta buffer per chunk, shared by
    its pages): every page decodes to its slice of the input, guard bytes intact."""
    import torch
    cases = []
    for bits in WIDTHS:
        dt2, kw2 = TWO_VAR[bits][0]
        cases.append((F.clustered(UINT[bits], 6000, seed=bits + 40), dict(mode=O.MODE_CLASSIC), dict(tbl_vars=2, tbl_ans_size_log=13, tbl_n_bins=300, tbl_weight_style=O.TBL_W_RANDOM, tbl_ob_mode=O.TBL_OB_RANDOM, tbl_shuffle=True, tbl_seed=41)))
        cases.append((F.clustered(UINT[bits], 6000, seed=bits + 42), dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONSECUTIVE, order=1), dict(tbl_vars=2, tbl_ans_size_log=10, tbl_weight_style=O.TBL_W_INVERSE, tbl_seed=43)))
        cases.append((arrangement_data(dt2, kw2, n=6000, seed=bits + 44), kw2, dict(tbl_vars=6, tbl_ans_size_log=11, tbl_weight_style=O.TBL_W_FLAT, tbl_ob_mode=O.TBL_OB_ALTERNATE, tbl_lower_wrap=True, tbl_seed=45)))
        cases.append((F.clustered(UINT[bits], 6000, seed=bits + 46), dict(mode=O.MODE_CLASSIC), dict(tbl_vars=2, tbl_n_bins=1024, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_seed=47)))
    pages = [1000, 257, 3000, 1743]
    blobs = []; tasks_meta = []   # (index of the ChunkMeta in blobs, index of the page, the page's numbers)
    for x, kw, tkw in cases:
        meta, pgs = O.test_encode(x, pages=pages, **kw, **tkw)
        base = len(blobs); blobs.append(meta); blobs += pgs
        pos = 0
        for j, (pg, pn) in enumerate(zip(pgs, pages)):
            got, err, in_meta = O.wrapped_page_prefix(meta, pg, x.dtype, pn)
            assert err == 0 and not in_meta and U.bits_equal(got, x[pos:pos + pn])
            tasks_meta.append((base, base + 1 + j, x[pos:pos + pn]))
            pos += pn
    s_offs, s_total = _slots([len(b) for b in blobs], extra=64)
    host_src = np.zeros(s_total, np.uint8)
    for o, b in zip(s_offs, blobs):
        host_src[o:o + len(b)] = np.frombuffer(b, np.uint8)
    src = torch.from_numpy(host_src).cuda()
    want = [t[2] for t in tasks_meta]
    d_offs, d_total = _slots([a.nbytes for a in want])
    out = torch.full((d_total,), GUARD, dtype=torch.uint8, device="cuda")
    k = len(tasks_meta)
    pt = (G.PageTask * k)(*[G.PageTask(src.data_ptr() + s_offs[m], len(blobs[m]), src.data_ptr() + s_offs[p], len(blobs[p]), out.data_ptr() + d_offs[i], a.size,
                                       G.DTYPE_BYTE[a.dtype.name], 4) for i, (m, p, a) in enumerate(tasks_meta)])
    res = (G.TaskResult * k)()
    G.check(L.pco_gfx_decompress_pages(k, pt, res, None, None))
    host = out.cpu().numpy()
    for i, a in enumerate(want):
        assert res[i].status == G.ST_OK and res[i].n_out == a.size, (i, res[i].status, res[i].n_out)
        assert U.bits_equal(host[d_offs[i]:d_offs[i] + a.nbytes].view(a.dtype), a), i
        end = d_offs[i + 1] if i + 1 < k else d_total
        assert (host[d_offs[i] + a.nbytes:end] == GUARD).all(), ("written past the page's numbers", i)


def test_every_generated_stream_was_decoded():
    """The module's skip budget is zero: every valid stream it generated (counted in valid()) was decoded by at least one device call with
    status OK and bit-exact numbers (counted where that is asserted).  Runs last; with the whole module, several hundred streams."""
    print(f"{len(GENERATED)} distinct valid streams generated, {len(GENERATED & DECODED)} of them decoded on the device")
    assert GENERATED <= DECODED, len(GENERATED - DECODED)
