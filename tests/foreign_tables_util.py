"""Foreign tables: legal tANS / bin tables that no reference encoder would write (oracle/pco_oracle_testenc.hpp, TestEncSpec's tbl_* fields),
for tests/test_foreign_tables.py (oracle, Python model) and tests/test_gpu_foreign_tables.py (the device decoders)."""
import numpy as np

import oracle_lib as O

ALL_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.float16, np.uint32, np.int32, np.float32, np.uint64, np.int64, np.float64]
MAX_ANS = 14   # ans/spec.rs / metadata: ans_size_log is at most 14
VAR_NAMES = ("delta", "primary", "secondary")


def ceil_log2(x):
    return 0 if x <= 1 else (x - 1).bit_length()


def clustered(dt, n, seed, clusters=12, spread=40):
    """n numbers of dtype dt around a few unequal clusters (several trained bins, single-value bins among them) plus rare far values: plenty
    of distinct values to split at, repeated values to duplicate bins over."""
    rng = np.random.default_rng(seed); dt = np.dtype(dt); bits = dt.itemsize * 8
    u = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}[bits]
    top = (1 << bits) - 1
    centres = rng.integers(0, top, clusters, dtype=np.uint64, endpoint=True)
    p = rng.random(clusters) ** 3 + 0.01; p /= p.sum()
    which = rng.choice(clusters, n, p=p)
    noise = rng.integers(0, spread, n, dtype=np.uint64) * (which % 3 != 0)        # every third cluster is one value: 0 offset bits
    lat = ((centres[which] + noise) & np.uint64(top)).astype(u)
    far = rng.random(n) < 0.01
    lat[far] = rng.integers(0, top, int(far.sum()), dtype=np.uint64, endpoint=True).astype(u)
    return lat.view(dt)   # (floats: the bit patterns as they come, NaNs and infinities included -- decode is bit-exact)


def expected_meta(plain_info, var, kw):
    """(n_bins, ans_size_log) the generator must have written for variable `var` (0 delta, 1 primary, 2 secondary) under the tbl_* kwargs,
    given the trained chunk's info; ans_size_log None where the spec leaves it to the trained value."""
    if not (kw.get("tbl_vars", 0) >> var) & 1 or not plain_info.var_present[var] or plain_info.n_bins[var] == 0:
        return plain_info.n_bins[var], plain_info.ans_size_log[var]
    nb = kw.get("tbl_n_bins", 0) or plain_info.n_bins[var]
    a = kw.get("tbl_ans_size_log", 0)
    if nb == 1: return 1, 0
    if a == O.TBL_ANS_MIN: return nb, ceil_log2(nb)
    if a: return nb, a
    return nb, max(ceil_log2(nb), plain_info.ans_size_log[var])


def check_meta(data, plain, kw, label=""):
    """The stream really holds the table it names: n_bins and ans_size_log per variable as asked (read back by the oracle's meta reader)."""
    info, bins = O.inspect_first_chunk(data, max_bins=1 << MAX_ANS)
    pinfo, _ = O.inspect_first_chunk(plain, max_bins=1 << MAX_ANS)
    for v in range(3):
        assert info.var_present[v] == pinfo.var_present[v], (label, v)
        if info.var_present[v]:
            assert (info.n_bins[v], info.ans_size_log[v]) == expected_meta(pinfo, v, kw), (label, VAR_NAMES[v], info.n_bins[v], info.ans_size_log[v], expected_meta(pinfo, v, kw))
    return info, bins


def strip_tbl(kw):
    return {k: v for k, v in kw.items() if not k.startswith("tbl_")}


def shapes(latent_bits):
    """name -> tbl_* kwargs: the table shapes of the issue, for a variable of `latent_bits` bits."""
    B = latent_bits
    P = O.TBL_PRIMARY
    s = {}
    for a in (O.TBL_ANS_MIN, 10, 11, 12, 13, 14):
        s[f"asl={'min' if a == O.TBL_ANS_MIN else a}"] = dict(tbl_vars=P, tbl_ans_size_log=a)
    s["flat@12"] = dict(tbl_vars=P, tbl_ans_size_log=12, tbl_weight_style=O.TBL_W_FLAT)
    s["inverse@12"] = dict(tbl_vars=P, tbl_ans_size_log=12, tbl_weight_style=O.TBL_W_INVERSE)
    s["inverse@14"] = dict(tbl_vars=P, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_INVERSE, tbl_shuffle=True, tbl_seed=3)
    s["random@9"] = dict(tbl_vars=P, tbl_ans_size_log=9, tbl_weight_style=O.TBL_W_RANDOM, tbl_seed=11)
    s["random@14"] = dict(tbl_vars=P, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_RANDOM, tbl_seed=12)
    s["ones@6"] = dict(tbl_vars=P, tbl_n_bins=64, tbl_ans_size_log=6, tbl_weight_style=O.TBL_W_ONES, tbl_seed=1)
    s["ones@10"] = dict(tbl_vars=P, tbl_n_bins=1024, tbl_ans_size_log=10, tbl_weight_style=O.TBL_W_ONES, tbl_seed=2, tbl_shuffle=True)
    s["ones@14"] = dict(tbl_vars=P, tbl_n_bins=16384, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_ONES, tbl_seed=3)
    for nb in (63, 64, 65, 255, 256, 257, 1024, 4096):
        s[f"bins={nb}"] = dict(tbl_vars=P, tbl_n_bins=nb, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_seed=nb, tbl_weight_style=O.TBL_W_RANDOM if nb % 2 else O.TBL_W_PROPORTIONAL)
    s["bins=16384 flat"] = dict(tbl_vars=P, tbl_n_bins=16384, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_FLAT, tbl_seed=5, tbl_shuffle=True)
    s["bins=300@14"] = dict(tbl_vars=P, tbl_n_bins=300, tbl_ans_size_log=14, tbl_seed=6, tbl_shuffle=True)
    s["ob=all full"] = dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=B)
    s["ob=alternate 0/full"] = dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_ALTERNATE, tbl_n_bins=40, tbl_seed=7)
    s["ob=random"] = dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_RANDOM, tbl_seed=8, tbl_shuffle=True)
    s["ob=one wide"] = dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_ONE, tbl_ob_value=B - 1, tbl_seed=9)
    s["wrap all full"] = dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=B, tbl_lower_wrap=True, tbl_seed=10)
    s["wrap random"] = dict(tbl_vars=P, tbl_ob_mode=O.TBL_OB_RANDOM, tbl_lower_wrap=True, tbl_seed=13, tbl_n_bins=100, tbl_shuffle=True)
    s["shuffle"] = dict(tbl_vars=P, tbl_shuffle=True, tbl_seed=14)
    s["one bin full"] = dict(tbl_vars=P, tbl_n_bins=1, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=B)
    s["one bin full wrapped"] = dict(tbl_vars=P, tbl_n_bins=1, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=B, tbl_lower_wrap=True, tbl_seed=15)
    s["one bin tight"] = dict(tbl_vars=P, tbl_n_bins=1)
    return s
