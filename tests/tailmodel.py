"""The tail stage (long-term filter, sign-log LMS cascade, zig-zag fold sum) in plain Python integers: a third opinion beside
the oracle (oracle/sla_oracle.c) and the reference, with every wrap to int32 / int64 written out.  Slow (one Python loop per
sample and tap); the C checkers are what long inputs are compared with.  Also the operand families the tail tests share, so
that the CPU pins (tests/test_oracle_vs_ref.py, tests/test_tail_model.py) and the GPU tests (tests/test_gpu_tail.py,
tests/test_gpu_predictor_api.py) speak of the same inputs."""
import zlib

import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def wrap32(v):
    return ((v + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31


def wrap64(v):
    return ((v + 2 ** 63) & 0xFFFFFFFFFFFFFFFF) - 2 ** 63


def sign(v):
    return (v > 0) - (v < 0)


def ltm_predict(x, pitch, coef):
    """out[s] = x[s] - int32((2^30 + sum_j coef[j] x[s - delay + j]) >> 31) for s >= delay = pitch + ntaps // 2, a copy before
    that and everywhere for pitch 0 (reference src/SLAPredictor.c:1063-1099)"""
    x = [int(v) for v in x]
    coef = [int(c) for c in coef]
    out = list(x)
    if pitch != 0:
        delay = pitch + len(coef) // 2
        for s in range(delay, len(x)):
            acc = 1 << 30
            for j, c in enumerate(coef):
                acc += c * x[s - delay + j]
            out[s] = wrap32(x[s] - wrap32(wrap64(acc) >> 31))
    return np.array(out, np.int64).astype(np.int32)


def lms_predict(x, order):
    """(error plane, largest |FIR coefficient|, largest |IIR coefficient|, number of errors equal to INT32_MIN)
    reference src/SLAPredictor.c:1202-1331: two adaptive filters, one over the past inputs (FIR) and one over the past
    predictions (IIR), both histories primed with the first `order` samples; fewer samples than taps: a copy"""
    x = [int(v) for v in x]
    n = len(x)
    out = list(x)
    if n < order:
        return np.array(out, np.int64).astype(np.int32), 0, 0, 0
    hx = x[:order][::-1]                                   # newest first
    hp = list(hx)
    sx = [sign(v) for v in hx]
    sp = list(sx)
    cf, ci = [0] * order, [0] * order
    max_f = max_i = num_min = 0
    for s in range(order, n):
        acc = 1 << 9
        for i in range(order):
            acc += cf[i] * hx[i] + ci[i] * hp[i]
        pred = wrap32(acc) >> 10
        e = wrap32(x[s] - pred)
        out[s] = e
        num_min += (e == INT32_MIN)
        step = sign(e) * (abs(e).bit_length() >> 1)         # |INT32_MIN| = 2^31 has 32 bits: step -16
        for i in range(order):
            cf[i] = wrap32(cf[i] + step * sx[i])
            ci[i] = wrap32(ci[i] + step * sp[i])
        max_f = max(max_f, max(abs(c) for c in cf))
        max_i = max(max_i, max(abs(c) for c in ci))
        hx = [x[s]] + hx[:-1]
        hp = [pred] + hp[:-1]
        sx = [sign(x[s])] + sx[:-1]
        sp = [sign(pred)] + sp[:-1]
    return np.array(out, np.int64).astype(np.int32), max_f, max_i, num_min


def fold_sum(e):
    """sum of the zig-zag map v >= 0 -> 2 v, v < 0 -> ~(2 v) as uint32 (reference src/SLAUtility.h:37), in 64 unsigned bits;
    INT32_MIN maps to 0xFFFFFFFF"""
    total = 0
    for v in np.asarray(e).tolist():
        total += ((v << 1) & 0xFFFFFFFF) ^ (0xFFFFFFFF if v < 0 else 0)
    return total & 0xFFFFFFFFFFFFFFFF


# ---- operand families --------------------------------------------------------------------------------------------

FAMILIES = ("full", "minmax", "allmin", "allmax", "alt", "small", "24bit", "ramp")


def family(name, n, seed=0):
    """n int32 samples of an operand family; the same (name, n, seed) gives the same samples everywhere"""
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d" % (name, n, seed)).encode()))
    if name == "full":
        x = rng.integers(INT32_MIN, INT32_MAX + 1, n, dtype=np.int64)
    elif name == "minmax":
        x = rng.choice(np.array([INT32_MIN, INT32_MAX], np.int64), n)
    elif name == "allmin":
        x = np.full(n, INT32_MIN, np.int64)
    elif name == "allmax":
        x = np.full(n, INT32_MAX, np.int64)
    elif name == "alt":
        x = np.where(np.arange(n) % 2 == 0, INT32_MAX, INT32_MIN).astype(np.int64)
    elif name == "small":
        x = rng.integers(-2, 3, n, dtype=np.int64)
    elif name == "24bit":
        x = rng.integers(-2 ** 23, 2 ** 23, n, dtype=np.int64)
    elif name == "ramp":
        x = 100000 * np.arange(n, dtype=np.int64)           # steep ramp, wrapped to int32 below
    else:
        raise KeyError(name)
    return x.astype(np.int32)


# long-term tap sets: at the ends of int32 (one, three and five taps) and ordinary ones with sum |coef| < 1 in Q31
LTM_TAPS = {
    "min1": [INT32_MIN],
    "ends3": [INT32_MIN, 0x7FFF0000, INT32_MIN],
    "ends3b": [0x7FFF0000, INT32_MIN, 0x7FFF0000],
    "ends5": [INT32_MIN, INT32_MIN, 0x7FFF0000, INT32_MIN, 0x7FFF0000],
    "plain1": [0x30000000],
    "plain3": [0x10000000, -0x38000000, 0x0C000000],
    "plain5": [-0x08000000, 0x18000000, 0x30000000, -0x14000000, 0x04000000],
}


def taps(name):
    return np.array(LTM_TAPS[name], np.int64).astype(np.int32)
