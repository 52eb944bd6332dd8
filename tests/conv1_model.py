"""A CPU model of the reference's Conv1 fit, delta/conv1.rs choose_config (reference 1.0.3), in numpy and exact Python floats.

Every f64 operation is the reference's, in its order: numpy's elementwise multiply and add round once each (no contraction), np.add.accumulate
sums one element after the other, and mul_add is formed exactly through fractions.Fraction and rounded once.  `v100=True` switches back the two
places where 1.0.0 differs (no 0.1 ridge, no `- 1` in the quantization): that form reproduces the reference's own v1_0_0_conv1.pco asset.
Test infrastructure only: the product computes the same on the device (pcodec_amd/csrc/encode_conv1.hip).
"""
import math
from fractions import Fraction

import numpy as np

BATCH = 512           # conv1.rs:11 ENCODE_BATCH_SIZE
RIDGE = 0.1           # conv1.rs:12 L2_REGULARIZATION
MAX_QUANTIZATION = 31
# latent type -> (L::MAX, Conv::MAX as f64, Conv::BITS)
LATENT = {8: (0xFF, 32767.0, 16), 16: (0xFFFF, 2147483647.0, 32), 32: (0xFFFFFFFF, float(2**63 - 1), 64)}


def mul_add(a, b, c):
    """Rust f64::mul_add: a * b + c rounded once."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def choose_pivot(x):
    """sort_utils.rs:5-56"""
    n = len(x)
    a, b, c = n // 4, n // 2, (n * 3) // 4
    if n >= 8:
        def sort2(i, j):
            return (j, i) if x[j] < x[i] else (i, j)

        def sort3(i, j, k):
            i, j = sort2(i, j)
            j, k = sort2(j, k)
            i, j = sort2(i, j)
            return i, j, k
        if n >= 50:
            _, a, _ = sort3(a - 1, a, a + 1)
            _, b, _ = sort3(b - 1, b, b + 1)
            _, c, _ = sort3(c - 1, c, c + 1)
        a, b, c = sort3(a, b, c)
    return int(x[b])


def autocov_dots(v, order):
    """conv1.rs:256-286: four strided lanes per (batch, sep), combined pairwise, added to the dot in batch order; the tail one by one."""
    n = len(v)
    almost_n = (n - order) // BATCH * BATCH
    nb = almost_n // BATCH
    dots = [0.0] * (order + 1)
    if nb:
        lanes = np.zeros((nb, order + 1, 4))
        base = np.arange(nb)[:, None, None] * BATCH + np.arange(4)[None, None, :]
        sep = np.arange(order + 1)[None, :, None]
        for s in range(0, BATCH, 4):
            lanes = lanes + v[base + s] * v[base + s + sep]
        part = (lanes[:, :, 0] + lanes[:, :, 1]) + (lanes[:, :, 2] + lanes[:, :, 3])
        acc = np.add.accumulate(part, axis=0)[-1]
        dots = [float(d) for d in acc]
    for i in range(almost_n, n - order):
        for s in range(order + 1):
            dots[s] += float(v[i]) * float(v[i + s])
    return dots


def autocov_mats(v, order, ridge):
    """conv1.rs:288-343 (column-major h x h xtx, h-vector xty)"""
    n = len(v)
    h = order + 1
    initial_sum = float(np.add.accumulate(v[: n - order])[-1])
    dots = autocov_dots(v, order)
    V = [float(x) for x in v[:order]] + [0.0]
    T = [float(x) for x in v[n - order - 1:]]   # T[k] = v[n - order - 1 + k]
    vt = lambda i: T[i - (n - order - 1)]
    X = [[0.0] * h for _ in range(h)]            # X[i][j]
    y = [0.0] * h
    for i in range(order):
        X[i][0] = dots[i]
        X[0][i] = dots[i]
    X[order][0] = initial_sum
    X[0][order] = initial_sum
    y[0] = dots[order]
    for i in range(1, order):
        for j in range(1, i + 1):
            d = X[i - 1][j - 1] + (vt(n - order + i - 1) * vt(n - order + j - 1) - V[i - 1] * V[j - 1])
            X[i][j] = d
            X[j][i] = d
        s = X[order][i - 1] + (vt(n - order + i - 1) - V[i - 1])
        X[order][i] = s
        X[i][order] = s
    for i in range(1, order):
        y[i] = X[order - 1][i - 1] + (vt(n - order + i - 1) * vt(n - 1) - V[i - 1] * V[order - 1])
    X[order][order] = float(n - order)
    y[order] = X[order][order - 1] + (vt(n - 1) - V[order - 1])
    for i in range(h):
        X[i][i] = X[i][i] + ridge
    return X, y


def cholesky(X):
    """conv1.rs:59-96 (Cholesky-Crout with mul_add)"""
    h = len(X)
    for j in range(h):
        for i in range(j):
            X[i][j] = 0.0
        s = 0.0
        for k in range(j):
            s = mul_add(X[j][k], X[j][k], s)
        d = X[j][j] - s
        d = math.sqrt(max(d, 0.0)) if not math.isnan(d) else 0.0   # safe_sqrt: f64::max ignores a NaN
        X[j][j] = d
        scale = 0.0 if d == 0.0 else 1.0 / d
        for i in range(j + 1, h):
            s = 0.0
            for k in range(j):
                s = mul_add(X[i][k], X[j][k], s)
            X[i][j] = scale * (X[i][j] - s)
    return X


def _div(a, b):
    if b == 0.0:
        if a == 0.0 or math.isnan(a):
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def solve(X, y):
    """forward_sub_into (:122-144), then transposed_backward_sub_into (:98-120)"""
    h = len(X)
    y = list(y)
    for j in range(h):
        d = _div(y[j], X[j][j])
        y[j] = d
        for i in range(j + 1, h):
            y[i] = y[i] - d * X[i][j]
    for j in reversed(range(h)):
        d = _div(y[j], X[j][j])
        y[j] = d
        for i in range(j):
            y[i] = y[i] - d * X[j][i]
    return y


def as_i64(x):
    """Rust `f64 as i64`: truncating, saturating, NaN -> 0"""
    if math.isnan(x):
        return 0
    if x >= 2.0**63:
        return 2**63 - 1
    if x <= -(2.0**63):
        return -(2**63)
    return int(x)


def round_half_away(x):
    if not math.isfinite(x):
        return x
    ax = abs(x)
    if ax >= 2.0**52:
        return x
    r = float(math.floor(ax))
    if ax - r >= 0.5:   # (exact below 2^52)
        r += 1.0
    return math.copysign(r, x)


def choose_config(latents, order, latent_bits, v100=False):
    """conv1.rs:358-421 on unsigned latents (a numpy array of the latent type); None = NoOp delta, else (quantization, bias, weights)."""
    x = np.asarray(latents).astype(np.uint64)
    n = len(x)
    if n < order + 1:
        return None
    center = choose_pivot(x)
    v = np.where(x < center, -((np.uint64(center) - x).astype(np.float64)), (x - np.uint64(center)).astype(np.float64))
    X, y = autocov_mats(v, order, 0.0 if v100 else RIDGE)
    beta = solve(cholesky(X), y)
    total = 0.0
    total_abs = 0.0
    for w in beta[:order]:
        total_abs += abs(w)
        total += w
    if not (math.isfinite(total) and math.isfinite(total_abs)):
        return None
    float_bias = ((1.0 - total) * float(center)) + beta[order]
    lmax, conv_max, conv_bits = LATENT[latent_bits]
    ratio = conv_max / (total_abs * float(lmax) + abs(float_bias) + 1.0)
    if math.isnan(ratio) or ratio <= 0.0:
        return None
    q = math.floor(math.log2(ratio)) - (0 if v100 else 1)
    q = min(q, MAX_QUANTIZATION, conv_bits - 1)
    if q < 0:
        return None
    f = 2.0**q
    weights = [as_i64(round_half_away(w * f)) for w in beta[:order]]
    return q, as_i64(float_bias * f), weights


def latents_of(nums):
    """Classic-mode primary latents (to_latent_ordered) of an integer or float array, and their bit width."""
    a = np.asarray(nums)
    bits = a.dtype.itemsize * 8
    u = np.dtype(f"u{a.dtype.itemsize}")
    raw = a.view(u)
    mid = u.type(1 << (bits - 1))
    if a.dtype.kind == "u":
        return raw.copy(), bits
    if a.dtype.kind == "i":
        return (raw ^ mid).astype(u), bits
    neg = (raw & mid) != 0
    return np.where(neg, ~raw, raw | mid).astype(u), bits


def floor_log2_rule(x):
    """The device's rule for floor(log2(x)) (encode_conv1.hip conv1_floor_log2), restated for the host check."""
    m, e = math.frexp(x)
    delta = 1.0 - m
    k = e
    if k <= 0:
        return e - 1
    kexp = k.bit_length() - 1
    half_ulp = math.ldexp(1.0, kexp - 54 if (k & (k - 1)) == 0 else kexp - 53)
    return k if delta * 1.4426950408889634 <= half_ulp else e - 1


# ---- data of the known-answer table ----
def k1_series():
    """the v1_0_0_conv1 generator (compatibility.rs:262-277, f32 arithmetic)"""
    xm1 = 0.0
    xm2 = 0.0
    nums = []
    for i in range(2000):
        x = np.float32(np.float32(np.float32(np.float32(xm1) * np.float32(1.99)) - np.float32(xm2)) + np.float32((i * 47) % 77 - 38))
        nums.append(int(np.int32(np.float32(x + np.float32(10000.0)))))
        xm2 = xm1
        xm1 = float(x)
    return np.array(nums, dtype=np.int32)


def _hash(i):
    return (i.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(2**32)


def k2_series():
    i = np.arange(65536, dtype=np.int64)
    t = i % 400
    tri = np.where(t < 200, t, 400 - t)
    return (tri * 100 - 10000 + ((_hash(i) >> np.uint64(7)) % np.uint64(31)).astype(np.int64)).astype(np.int16)


def k3_series():
    i = np.arange(10000, dtype=np.int64)
    return ((3 * i) % 200 + ((_hash(i) >> np.uint64(9)) % np.uint64(7)).astype(np.int64)).astype(np.uint8)


def k4_series():
    i = np.arange(1 << 22, dtype=np.int64)
    t = i % 4096
    tri = np.where(t < 2048, t, 4096 - t)
    return (tri * 2000000 + (_hash(i) % np.uint64(100003)).astype(np.int64)).astype(np.uint32)


# (id, series, order, quantization, bias, weights); weights None: not tabulated
KAT = [
    ("K1", k1_series, 1, 30, 11592707818972048, [1068343574]),
    ("K1", k1_series, 2, 28, 5616951535236820, [-245669610, 511489481]),
    ("K1", k1_series, 6, 28, 14185455320018030, [-136687389, 210259740, -110250838, -3459219, -93069282, 395036857]),
    ("K1", k1_series, 32, 27, 5647842422218357, None),
    ("K2", k2_series, 3, 12, 63378, [-2359, 702, 5751]),
    ("K2", k2_series, 8, 11, 26764, [-105, 911, -2013, 1824, -899, -244, -792, 3366]),
    ("K3", k3_series, 3, 5, 309, [-1, 0, 30]),
    ("K4", k4_series, 4, 28, 2213646424065, [-41434958, 14522079, -172884606, 468231860]),
]
# the reference's own asset (1.0.0 fit: no ridge, no `- 1`), its ChunkMeta
ASSET_V100 = (29, 11234584282202004, [-491339413, 1022978839])
