"""numpy model of k_ltm_acf_int (sla_amd/csrc/kernels/longterm.inc): the autocorrelation of an int32 block at the lags
0 .. 263 from int8 matrix products.

Every sample is split into balanced base-256 digits, x = sum_a d_a 2^(8a) with d_a in [-128, 127].  With a sample indexed
m = 16 kappa + i, a shift s = 0 .. 17 and a digit pair (a, b)

    A_a[i][kappa]    = d_a(x[16 kappa + i])                (16 x K)
    B_bs[kappa][c]   = d_b(x[16 (kappa + s) + c])          (K x 16, zeros beyond the block)
    C = A_a B_bs,    C[i][c] adds 2^(8 (a + b)) C[i][c] to the lag k = 16 s + c - i      (s = 0: c >= i only)

and every (m, k) with 0 <= k <= 263 occurs exactly once.  All pairs of one weight w = a + b share an i32 cell; the cells
of a diagonal and of the two shifts that meet in a lag are added in i32 as well, the weights are combined in exact
integers.  The model keeps the kernel's number formats: int8 operands, cells and per-weight lag sums asserted to fit i32.
"""
import numpy as np

LAGS = 264
SHIFTS = 18

# D digits cover [-128 (256^D - 1) / 255, 127 (256^D - 1) / 255]
DIGIT_LO = [-128 * ((256 ** d - 1) // 255) for d in range(1, 6)]
DIGIT_HI = [127 * ((256 ** d - 1) // 255) for d in range(1, 6)]
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def digit_count(lo, hi):
    """digits needed for a block whose samples lie in [lo, hi] (the kernel includes 0: the padding)"""
    lo, hi = min(int(lo), 0), max(int(hi), 0)
    for d in range(1, 5):
        if lo >= DIGIT_LO[d - 1] and hi <= DIGIT_HI[d - 1]:
            return d
    return 5


def digits(x, count):
    """balanced digits of int32 samples: (count, n) int8; the remainder after `count` digits must be zero"""
    v = np.asarray(x, dtype=np.int64).copy()
    out = np.zeros((count, len(v)), np.int8)
    for a in range(count):
        d = ((v + 128) & 255) - 128
        out[a] = d.astype(np.int8)
        v = (v - d) >> 8
    assert not v.any(), "more digits needed"
    return out


def acf_int(x, stats=None):
    """the lags 0 .. 263 of sum_m x[m] x[m + k] as Python integers, by the kernel's route"""
    x = np.asarray(x, dtype=np.int64)
    n = len(x)
    D = digit_count(x.min(), x.max()) if n else 1
    K = 64 * ((n + 1023) // 1024)                                  # kappa count: whole tiles of 64
    dg = np.zeros((D, 16 * (K + SHIFTS + 16)), np.int8)
    dg[:, :n] = digits(x, D)
    planes = dg.reshape(D, -1, 16).transpose(0, 2, 1).astype(np.int64)      # [a][i][kappa]
    W = 2 * D - 1
    lag_sum = np.zeros((W, LAGS + 32), np.int64)
    max_cell = 0
    ii, cc = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    for s in range(SHIFTS):
        cells = np.zeros((W, 16, 16), np.int64)
        for a in range(D):
            A = planes[a][:, :K]                                   # 16 x K
            for b in range(D):
                B = planes[b][:, s:s + K].T                        # K x 16
                cells[a + b] += A @ B
        max_cell = max(max_cell, int(np.abs(cells).max()))
        assert max_cell < 2 ** 31, "cell overflows i32"
        k = 16 * s + cc - ii
        ok = (k >= 0) & (k < LAGS)
        for w in range(W):
            np.add.at(lag_sum[w], k[ok], cells[w][ok])
    assert int(np.abs(lag_sum).max()) < 2 ** 31, "per-weight lag sum overflows i32"
    if stats is not None:
        stats["digits"] = D
        stats["max_cell"] = max(stats.get("max_cell", 0), max_cell)
        stats["max_lag_sum"] = max(stats.get("max_lag_sum", 0), int(np.abs(lag_sum).max()))
    return [sum(int(lag_sum[w][k]) << (8 * w) for w in range(W)) for k in range(LAGS)]


def acf_exact(x, lags=LAGS):
    """the same sums in Python integers, directly"""
    v = [int(t) for t in np.asarray(x).tolist()]
    n = len(v)
    if n and max(abs(t) for t in v) < 2 ** 23 and n <= 2 ** 15:           # every sum below 2^61: int64 dot products are exact
        a = np.asarray(v, np.int64)
        return [int(np.dot(a[:n - k], a[k:])) if k < n else 0 for k in range(lags)]
    hi = np.asarray([t >> 16 for t in v], np.int64)                        # x = hi 2^16 + lo, |hi| <= 2^15, 0 <= lo < 2^16
    lo = np.asarray([t & 0xFFFF for t in v], np.int64)
    out = []
    for k in range(lags):
        if k >= n:
            out.append(0)
            continue
        hh = int(np.dot(hi[:n - k], hi[k:]))
        hl = int(np.dot(hi[:n - k], lo[k:])) + int(np.dot(lo[:n - k], hi[k:]))
        ll = int(np.dot(lo[:n - k], lo[k:]))
        out.append((hh << 32) + (hl << 16) + ll)
    return out


def scaled(total, fft_size):
    """what the kernel stores: the integer rounded to double once, times 2^-62 * fft_size / 2 (a power of two)"""
    return float(total) * (2.0 ** -62 * (fft_size // 2))
