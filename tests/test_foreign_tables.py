"""Legal tANS / bin tables that no reference encoder would write (-m "not gpu").

Every stream the suite decoded so far carried tables out of the reference's own training (histogram, optimize_bins, quantize_weights): the
smallest ans_size_log that fits, weights proportional to counts, sorted disjoint tight bins.  The format allows far more
(metadata/chunk_latent_var.rs:115-132, ans/spec.rs:37-44), and the test generator now writes it (TestEncSpec's tbl_* fields).  Here:

  * the oracle's decoder gives the input back bit for bit on a grid of such tables over all 11 number types, and its meta reader finds the
    n_bins / ans_size_log each case names (so a case cannot quietly test another table);
  * a pure-Python model that shares no code with the oracle (tests/tans_model.py) decodes a dozen of them to the input too;
  * every named invalid table header is Corruption on the oracle."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import decode_sweep_util as S  # noqa: E402
import foreign_tables_util as F  # noqa: E402
import oracle_lib as O  # noqa: E402
import tans_model as M  # noqa: E402


def bits_equal(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))


def round_trip(x, kw, label):
    data = O.test_encode(x, **kw)
    plain = O.test_encode(x, **F.strip_tbl(kw))
    info, bins = F.check_meta(data, plain, kw, label)
    back = O.simple_decompress(data, x.dtype, cap=x.size + 8)
    assert bits_equal(back, x), label
    return data, info, bins


@pytest.mark.parametrize("dt", F.ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_oracle_round_trip_of_foreign_tables(dt):
    """Every shape of the issue on a Classic chunk of every number type: forced ans_size_log (minimum .. 14), flat / inverse / all-ones /
    random weights, bin counts forced up to 2^14 by splits and duplicates, widened offsets (full width, 0-bit beside full-width bins), lowers
    moved down so that lower + offset wraps, shuffled bins, one bin with ans_size_log 0 and wide offsets."""
    bits = np.dtype(dt).itemsize * 8
    x = F.clustered(dt, 17000 if bits > 8 else 6000, seed=bits)
    seen_wrap = False
    for name, kw in F.shapes(bits).items():
        label = f"{np.dtype(dt).name} {name}"
        data, info, bins = round_trip(x, dict(kw, mode=O.MODE_CLASSIC), label)
        b = bins[1]
        assert int(b[:, 0].sum()) == 1 << info.ans_size_log[1] and int(b[:, 0].min()) >= 1, label
        if kw.get("tbl_weight_style") == O.TBL_W_ONES: assert int(b[:, 0].max()) == 1, label
        if kw.get("tbl_weight_style") == O.TBL_W_INVERSE: assert int(b[:, 0].max()) == (1 << info.ans_size_log[1]) - (len(b) - 1), label
        if kw.get("tbl_ob_mode") == O.TBL_OB_ALL: assert int(b[:, 2].min()) == kw["tbl_ob_value"], label
        if kw.get("tbl_ob_mode") == O.TBL_OB_ALTERNATE: assert int(b[:, 2].max()) == bits and int(b[:, 2].min()) == 0, (label, b[:, 2].min())
        if kw.get("tbl_lower_wrap"):   # some bin's lower + its largest offset passes 2^bits: the join has to wrap
            top = [int(lo) + (1 << int(ob)) - 1 for _, lo, ob in b]
            seen_wrap |= any(t >= 1 << bits for t in top)
    assert seen_wrap


ARRANGEMENTS = [
    ("int-mult", np.int32, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=7)),
    ("int-mult u8", np.uint8, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=5)),
    ("int-mult i64 consecutive, delta'd secondary", np.int64, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=1000, delta=O.TE_DELTA_CONSECUTIVE, order=2, secondary_uses_delta=True)),
    ("float-mult f64", np.float64, dict(mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.01)),
    ("float-quant f32", np.float32, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=12)),
    ("float-quant f16", np.float16, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=4)),
    ("lookback u64", np.uint64, dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, lookback_seed=5)),
    ("lookback u16 state", np.uint16, dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_LOOKBACK, window_n_log=6, state_n_log=2, lookback_seed=6)),
    ("dict i16", np.int16, dict(mode=O.MODE_TRY_DICT)),
    ("dict f64 first appearance", np.float64, dict(mode=O.MODE_TRY_DICT, dict_first_appearance=True)),
    ("conv1 u16", np.uint16, dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, quantization=4, bias=5, weights=[-16, 32])),
    ("conv1 i32", np.int32, dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, quantization=0, bias=0, weights=[1])),
]


def arrangement_data(dt, kw, n=6000, seed=1):
    rng = np.random.default_rng(seed); dt = np.dtype(dt)
    if kw.get("mode") == O.MODE_TRY_DICT:
        return S._values(rng, dt, n, 300)
    if kw.get("mode") == O.MODE_TRY_INT_MULT:
        b = kw["mode_u64"]; hi = 20 if dt.itemsize == 1 else 3000
        return (rng.integers(0, hi, n) * b + rng.integers(0, 3, n) * (rng.random(n) < 0.3)).astype(dt)
    if kw.get("mode") == O.MODE_TRY_FLOAT_MULT:
        x = (rng.integers(10, 5000, n) * kw["mode_f64"]).astype(dt)
        u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize]
        return (x.view(u) + (rng.random(n) < 0.2).astype(u)).view(dt)
    if kw.get("mode") == O.MODE_TRY_FLOAT_QUANT:
        u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize]; q = kw["mode_u64"]
        with np.errstate(all="ignore"):
            x = rng.normal(0, 100, n).astype(dt).view(u) & u(~((1 << q) - 1) & ((1 << (8 * dt.itemsize)) - 1))
        return np.where(rng.random(n) < 0.2, x | rng.integers(0, 4, n).astype(u), x).astype(u).view(dt)
    if kw.get("delta") == O.TE_DELTA_LOOKBACK:
        top = (1 << (8 * dt.itemsize)) - 1
        per = rng.integers(0, top, 37, dtype=np.uint64)
        return (per[np.arange(n) % 37] + rng.integers(0, 3, n).astype(np.uint64)).astype(dt)
    return S._smooth(rng, dt, n)


ARR_SHAPES = {
    "asl=14 random": dict(tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_RANDOM, tbl_seed=21, tbl_shuffle=True),
    "bins=257 min": dict(tbl_n_bins=257, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_seed=22),
    "bins=1024 ones": dict(tbl_n_bins=1024, tbl_ans_size_log=10, tbl_weight_style=O.TBL_W_ONES, tbl_seed=23, tbl_ob_mode=O.TBL_OB_RANDOM),
    "inverse@11 alternate": dict(tbl_ans_size_log=11, tbl_weight_style=O.TBL_W_INVERSE, tbl_ob_mode=O.TBL_OB_ALTERNATE, tbl_seed=24),
    "one bin": dict(tbl_n_bins=1),
}


@pytest.mark.parametrize("name,dt,kw", ARRANGEMENTS, ids=[a[0] for a in ARRANGEMENTS])
def test_oracle_round_trip_under_every_variable_arrangement(name, dt, kw):
    """Two variables (foreign tables on the primary only, the secondary only, both), lookback (the delta variable's table too), Dict (its
    u32 primary), Conv1."""
    x = arrangement_data(dt, kw)
    present = [O.TBL_PRIMARY]
    if kw["mode"] in (O.MODE_TRY_INT_MULT, O.MODE_TRY_FLOAT_MULT, O.MODE_TRY_FLOAT_QUANT): present += [O.TBL_SECONDARY, O.TBL_PRIMARY | O.TBL_SECONDARY]
    if kw.get("delta") == O.TE_DELTA_LOOKBACK: present += [O.TBL_DELTA, O.TBL_ALL]
    for sname, skw in ARR_SHAPES.items():
        for vars_ in present:
            round_trip(x, dict(kw, tbl_vars=vars_, **skw), f"{name} {sname} vars={vars_}")
    if kw["mode"] != O.MODE_TRY_DICT and kw.get("delta") != O.TE_DELTA_LOOKBACK:
        round_trip(x, dict(kw, tbl_vars=O.TBL_ALL, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=np.dtype(dt).itemsize * 8, tbl_lower_wrap=True, tbl_seed=25), f"{name} wrap")


def test_a_variable_without_latents_keeps_an_empty_table():
    """n_bins == 0 is valid exactly where a variable has no latent in the page body (a standalone chunk cannot hold n == 0 -- it stores
    n - 1 --, so the body is emptied by a delta order of at least n): the generator leaves such a table empty whatever the spec asks, and
    the oracle decodes it."""
    x = np.arange(3, dtype=np.uint32) * 7
    kw = dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONSECUTIVE, order=3, tbl_vars=O.TBL_ALL, tbl_ans_size_log=12, tbl_n_bins=50)
    data = O.test_encode(x, **kw)
    info, _ = O.inspect_first_chunk(data)
    assert info.n_bins[1] == 0 and info.ans_size_log[1] == 0
    assert bits_equal(O.simple_decompress(data, x.dtype, cap=16), x)


def test_the_generator_refuses_what_it_cannot_write():
    x = F.clustered(np.uint16, 3000, seed=4)
    bad = [dict(tbl_ans_size_log=15), dict(tbl_n_bins=300, tbl_ans_size_log=8), dict(tbl_n_bins=1, tbl_ans_size_log=3), dict(tbl_n_bins=2),
           dict(tbl_n_bins=16385), dict(tbl_n_bins=100, tbl_ans_size_log=7, tbl_weight_style=O.TBL_W_ONES), dict(tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=17),
           dict(tbl_weight_style=9), dict(tbl_ob_mode=9)]
    assert O.inspect_first_chunk(O.test_encode(x))[0].n_bins[1] > 2
    for kw in bad:
        with pytest.raises(O.OracleError) as ei:
            O.test_encode(x, tbl_vars=O.TBL_PRIMARY, **kw)
        assert ei.value.kind == O.ERR_INVALID_ARGUMENT, kw
    lb = dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_LOOKBACK, window_n_log=6, lookback_seed=1)
    with pytest.raises(O.OracleError) as ei:   # the lookback variable's lowers must stay inside [1, window]
        O.test_encode(x, tbl_vars=O.TBL_DELTA, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=32, tbl_lower_wrap=True, **lb)
    assert ei.value.kind == O.ERR_INVALID_ARGUMENT
    with pytest.raises(O.OracleError) as ei:   # a fault on a variable the chunk does not have
        O.test_encode(x, tbl_fault=O.TBL_FAULT_ANS_15, tbl_fault_var=2)
    assert ei.value.kind == O.ERR_INVALID_ARGUMENT


MODEL_CASES = [
    ("ones@14", np.uint16, 17000, dict(tbl_n_bins=16384, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_ONES, tbl_seed=3)),
    ("wrapped lower full width", np.uint32, 1500, dict(tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=32, tbl_lower_wrap=True, tbl_seed=10)),
    ("wrapped lower random widths", np.int64, 1500, dict(tbl_ob_mode=O.TBL_OB_RANDOM, tbl_lower_wrap=True, tbl_seed=13, tbl_n_bins=100, tbl_shuffle=True)),
    ("inverse@12", np.uint8, 2000, dict(tbl_ans_size_log=12, tbl_weight_style=O.TBL_W_INVERSE)),
    ("flat@13", np.int16, 1500, dict(tbl_ans_size_log=13, tbl_weight_style=O.TBL_W_FLAT, tbl_n_bins=70, tbl_seed=2)),
    ("random@14 shuffled", np.float32, 1500, dict(tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_RANDOM, tbl_seed=12, tbl_shuffle=True)),
    ("bins=257 min", np.uint64, 3000, dict(tbl_n_bins=257, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_seed=257)),
    ("bins=4096 duplicates", np.uint8, 9000, dict(tbl_n_bins=4096, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_seed=5, tbl_weight_style=O.TBL_W_RANDOM)),
    ("0-bit beside full-width bins", np.float64, 1500, dict(tbl_ob_mode=O.TBL_OB_ALTERNATE, tbl_n_bins=40, tbl_seed=7)),
    ("one bin, ans_size_log 0, full width, wrapped", np.int32, 700, dict(tbl_n_bins=1, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=32, tbl_lower_wrap=True, tbl_seed=15)),
    ("one wide bin beside narrow ones", np.float16, 1500, dict(tbl_ob_mode=O.TBL_OB_ONE, tbl_ob_value=16, tbl_seed=9, tbl_shuffle=True)),
    ("asl=min, 3 bins", np.int8, 600, dict(tbl_n_bins=0, tbl_ans_size_log=O.TBL_ANS_MIN)),
    ("trained table (nothing foreign)", np.uint32, 1500, dict()),
]


@pytest.mark.parametrize("name,dt,n,kw", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_python_model_decodes_foreign_streams(name, dt, n, kw):
    """The generator and the oracle's decoder share spread_state_symbols; the model (tests/tans_model.py) builds its table from the format's
    text alone and must read the same latents: input == oracle == model."""
    x = F.clustered(dt, n, seed=n + len(name))
    full = dict(kw, mode=O.MODE_CLASSIC, tbl_vars=O.TBL_PRIMARY) if kw else dict(mode=O.MODE_CLASSIC)
    data, info, bins = round_trip(x, full, name)
    lat, var = M.decode_one_chunk_file(data, x.dtype.itemsize * 8)
    assert var["ans_size_log"] == info.ans_size_log[1] and len(var["bins"]) == info.n_bins[1]
    assert [tuple(int(v) for v in b) for b in bins[1]] == var["bins"], name
    assert np.array_equal(np.array(lat, dtype=np.uint64), M.to_latent(x).astype(np.uint64)), name


def test_model_spread_matches_the_oracle_on_odd_weight_vectors():
    """The one function the generator and the oracle's decoder share, against the model, on weight vectors no quantize_weights produces."""
    rng = np.random.default_rng(2)
    for size_log in (0, 1, 2, 5, 10, 14):
        for style in range(4):
            size = 1 << size_log
            if style == 0: w = [1] * size
            elif style == 1: w = [size]
            elif style == 2: w = [1] * min(size - 1, 9) + [size - min(size - 1, 9)] if size > 1 else [1]
            else:
                cuts = np.sort(rng.choice(np.arange(1, size), size=min(size - 1, 13), replace=False)) if size > 1 else np.array([], int)
                w = np.diff(np.concatenate([[0], cuts, [size]])).tolist()
            assert O.spread_state_symbols(w) == M.spread_state_symbols(size_log, w), (size_log, style)


FAULT_CASES = [
    ("classic", np.uint32, dict(mode=O.MODE_CLASSIC), (1,)),
    ("int-mult", np.int16, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=7), (1, 2)),
    ("lookback", np.uint64, dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, lookback_seed=5), (0, 1)),
    ("dict", np.float32, dict(mode=O.MODE_TRY_DICT), (1,)),
]


@pytest.mark.parametrize("name,dt,kw,vars_", FAULT_CASES, ids=[c[0] for c in FAULT_CASES])
def test_every_table_fault_is_corruption_on_the_oracle(name, dt, kw, vars_):
    """One stream per reference check (chunk_latent_var.rs:115-132: 2^ans_size_log < n_bins, one bin with ans_size_log > 0, ans_size_log
    beyond 14, offset bits beyond the type; ans/spec.rs:37-44: weights that do not sum to the table size; page_decompressor.rs:52: no bins
    but latents in the body), on each variable the chunk has."""
    x = arrangement_data(dt, kw, n=3000, seed=9)
    assert bits_equal(O.simple_decompress(O.test_encode(x, **kw), x.dtype, cap=x.size + 8), x)
    for var in vars_:
        for fname, fault in O.TBL_FAULTS.items():
            data = O.test_encode(x, tbl_fault=fault, tbl_fault_var=var, **kw)
            with pytest.raises(O.OracleError) as ei:
                O.simple_decompress(data, x.dtype, cap=x.size + 8)
            assert ei.value.kind == O.ERR_CORRUPTION, (name, var, fname, str(ei.value))


def test_wrapped_pages_of_a_foreign_chunk_decode_on_the_oracle():
    """The generator's wrapped form (one chunk in several pages, for pco_gfx_decompress_pages): every page decodes to its slice of the
    input through the oracle's PageDecompressor, under a foreign table shared by the pages."""
    for dt, kw in ((np.uint32, dict(mode=O.MODE_CLASSIC)), (np.int64, dict(mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONSECUTIVE, order=1)),
                   (np.float32, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=12))):
        x = arrangement_data(dt, kw, n=5000, seed=3) if kw["mode"] != O.MODE_CLASSIC else F.clustered(dt, 5000, seed=3)
        pages = [1000, 257, 3000, 743]
        meta, pgs = O.test_encode(x, pages=pages, tbl_vars=O.TBL_ALL, tbl_ans_size_log=13, tbl_n_bins=300, tbl_weight_style=O.TBL_W_RANDOM,
                                  tbl_ob_mode=O.TBL_OB_RANDOM, tbl_shuffle=True, tbl_seed=4, **kw)
        pos = 0
        for pg, pn in zip(pgs, pages):
            got, err, in_meta = O.wrapped_page_prefix(meta, pg, x.dtype, pn)
            assert err == 0 and not in_meta and bits_equal(got, x[pos: pos + pn]), (np.dtype(dt).name, pos)
            pos += pn


def test_the_old_entry_point_still_takes_the_old_spec():
    """pco_oracle_test_encode keeps the argument it had before the tbl_* fields (a spec that ends at dict_first_appearance): a caller built
    against that layout gets the bytes it always got, whatever lies behind its struct in memory."""
    import ctypes as C

    class OldSpec(C.Structure):
        _fields_ = O.TestEncSpec._fields_[:[f[0] for f in O.TestEncSpec._fields_].index("tbl_vars")]

    class Padded(C.Structure):   # the old spec with junk right behind it, where the new fields would be read from
        _fields_ = [("spec", OldSpec), ("junk", C.c_uint32 * 16)]

    x = F.clustered(np.int32, 3000, seed=77)
    p = Padded(OldSpec(O.MODE_TRY_INT_MULT, O.TE_DELTA_CONSECUTIVE, 0.0, 7, 2, 1, 0, 0, 0, 0, 0, (C.c_int32 * 32)(), 8, 0), (C.c_uint32 * 16)(*[0xdeadbeef] * 16))
    dst = np.empty(x.nbytes * 2 + 70000, np.uint8); n_written = C.c_size_t(0); cs = (C.c_size_t * 1)(x.size)
    rc = O.lib().pco_oracle_test_encode(x.ctypes.data_as(C.c_void_p), C.c_size_t(x.size), C.c_uint8(O.dtype_byte(x)), C.byref(p), cs, C.c_size_t(1),
                                        dst.ctypes.data_as(C.c_void_p), C.c_size_t(dst.size), C.byref(n_written))
    assert rc == 0, O.lib().pco_oracle_last_error()
    assert dst[: n_written.value].tobytes() == O.test_encode(x, mode=O.MODE_TRY_INT_MULT, mode_u64=7, delta=O.TE_DELTA_CONSECUTIVE, order=2, secondary_uses_delta=True)
