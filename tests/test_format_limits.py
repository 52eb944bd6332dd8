"""-m "not gpu": the oracle at the ends of the mode-parameter ranges, pinned by a model that shares no code with it.

The oracle judges the device, and the reference's golden files pin the oracle -- but none of them carries an int-mult base near the type's
maximum, a float-quant k at the mantissa width, or a float-mult base that is subnormal, negative, or has an infinite or subnormal inverse.
tests/format_limits_util.py restates the three splits and joins on Python integers and numpy scalars; here the oracle's split
(`O.split_latents`), the mode payload it writes and its full encode -> decode round trip are compared with that model on every row of the
grid, at 300 and 3000 numbers, and the parameters beyond the ranges are refused as InvalidArgument."""
import numpy as np
import pytest

import format_limits_util as F
import gpu_util as U
import oracle_lib as O

SIZES = (300, 3000)
ROWS = [r for n in SIZES for r in F.grid(n)]


def as_ints(a):
    return [int(x) for x in a]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_oracle_split_and_round_trip_equal_the_model(row):
    _, arr, kw = row
    cfg = O.make_config(enable_8_bit=True, **kw)
    p, s, payload = F.model_split(arr, kw)
    op, os_, mk, mp = O.split_latents(arr, cfg)
    assert mk == {F.MODE_INT_MULT: 1, F.MODE_FLOAT_MULT: 2, F.MODE_FLOAT_QUANT: 3}[kw["mode"]] and mp == payload, (mk, mp, payload)
    bad = [i for i in range(arr.size) if int(op[i]) != p[i] or int(os_[i]) != s[i]]
    assert not bad, (len(bad), [(i, arr[i], int(op[i]), p[i], int(os_[i]), s[i]) for i in bad[:5]])
    # the model's join gives the input back from these latents, bit for bit (NaN payloads, -0 and the extremes included)
    assert U.bits_equal(F.model_join(p, s, kw, arr.dtype), arr)
    # and so does the oracle, through a whole file
    f = O.simple_compress(arr, cfg)
    assert U.bits_equal(O.simple_decompress(f, arr.dtype, cap=arr.size + 8), arr)
    # The encoder falls back to a classic chunk where the two tables cost more than they save: only 8- and 16-bit rows may (their raw
    # numbers are that small).  The generator never falls back, so the oracle's JOIN runs on every row.
    info, _ = O.inspect_first_chunk(f)
    assert info.mode_kind == mk or (info.mode_kind == 0 and F.width(arr.dtype) <= 16), (info.mode_kind, mk)
    g = O.test_encode(arr, mode=kw["mode"], mode_f64=kw.get("mode_f64", 0.0), mode_u64=kw.get("mode_u64", 0))
    info, _ = O.inspect_first_chunk(g)
    assert info.mode_kind == mk and info.n == arr.size and info.var_present[2]
    assert (info.mode_k if mk == 3 else info.mode_base_latent) == payload
    assert U.bits_equal(O.simple_decompress(g, arr.dtype, cap=arr.size + 8), arr)


def test_grid_holds_what_it_promises():
    """The data of the grid really carries the values the parameters go wrong at."""
    for _, arr, kw in F.grid(300):
        w = F.width(arr.dtype)
        if arr.dtype.kind != "f":
            ii = np.iinfo(arr.dtype)
            assert ii.min in arr and ii.max in arr and 0 in arr and np.array([(1 << w) - 1], F.UINT[w]).view(arr.dtype)[0] in arr
            continue
        bits = set(F.patterns(arr)); prec = F.PREC[w]
        mant = (1 << prec) - 1; exp = ((1 << (w - 1)) - 1) ^ mant
        assert 0 in bits and (1 << (w - 1)) in bits and exp in bits and (exp | 1 << (w - 1)) in bits     # +-0, +-inf
        assert any(b & exp == exp and b & mant and not b & (1 << (prec - 1)) for b in bits)           # a signalling NaN
        assert len({b & mant for b in bits if b & exp == exp and b & mant}) >= 5                       # NaNs of several payloads
        assert any(b & exp == 0 and b & mant for b in bits)                                           # subnormals
        assert F._bits(np.finfo(arr.dtype).max) in bits
        if kw["mode"] == F.MODE_FLOAT_MULT and abs(kw["mode_f64"]) * 2.0 ** (prec + 1) <= float(np.finfo(arr.dtype).max):
            p, _, _ = F.model_split(arr, kw)
            gpi = 1 << (prec + 1); mid = 1 << (w - 1)
            assert any(gpi < abs(l - mid) < gpi + (exp >> 1) for l in p), kw     # finite multipliers beyond 2^(prec + 1)


@pytest.mark.parametrize("row", F.refused(), ids=[r[0] for r in F.refused()])
def test_oracle_refuses_parameters_beyond_the_ranges(row):
    _, arr, kw = row
    cfg = O.make_config(enable_8_bit=True, **kw)
    for call in (lambda: O.simple_compress(arr, cfg), lambda: O.split_latents(arr, cfg)):
        with pytest.raises(O.OracleError) as ei:
            call()
        assert ei.value.kind == O.ERR_INVALID_ARGUMENT, str(ei.value)


@pytest.mark.parametrize("dt", F.INT_TYPES + F.FLOAT_TYPES, ids=lambda d: np.dtype(d).name)
def test_classic_ordering_equals_the_model(dt):
    rng = np.random.default_rng(F.width(dt))
    arr = F.int_data(dt, 300, 3, rng) if np.dtype(dt).kind != "f" else F.float_data(dt, 300, 0.1, rng)
    kw = dict(mode=F.MODE_CLASSIC, delta=1)
    p, _, _ = F.model_split(arr, kw)
    op, _, mk, _ = O.split_latents(arr, O.make_config(enable_8_bit=True, **kw))
    assert mk == 0 and as_ints(op) == p
    if np.dtype(dt).kind != "f":   # the ordering is the numbers' own
        order = np.argsort(arr, kind="stable")
        assert all(p[order[i]] <= p[order[i + 1]] for i in range(arr.size - 1))
    assert U.bits_equal(F.model_join(p, None, kw, dt), arr)
