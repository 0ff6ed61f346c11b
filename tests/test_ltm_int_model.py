"""The identity behind k_ltm_acf_int, checked without a device: the numpy model (ltmintmodel.py: balanced digits, the
18-shift tiling, per-weight i32 cells, diagonals, combination) against Python integers, at the block lengths where the
tiling changes, on both sides of every boundary of the digit table and on the extreme int32 blocks."""
import numpy as np
import pytest

import ltmintmodel as M

LENGTHS = [1, 15, 16, 17, 263, 264, 265, 300, 1023, 1024, 1025, 2049, 4096, 16384]


def test_digit_table():
    """the ranges of DESIGN section 2c; INT32_MIN fits four digits, INT32_MAX needs five"""
    assert (M.DIGIT_LO, M.DIGIT_HI) == ([-128, -32896, -8421504, -2155905152, -551911719040],
                                        [127, 32639, 8355711, 2139062143, 547599908735])
    assert M.digit_count(M.INT32_MIN, 0) == 4 and M.digit_count(0, M.INT32_MAX) == 5
    for d in range(1, 5):
        assert M.digit_count(M.DIGIT_LO[d - 1], M.DIGIT_HI[d - 1]) == d
        assert M.digit_count(M.DIGIT_LO[d - 1] - 1, 0) == d + 1 and M.digit_count(0, M.DIGIT_HI[d - 1] + 1) == d + 1


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
def test_digits_recombine(count):
    lo, hi = max(M.DIGIT_LO[count - 1], M.INT32_MIN), min(M.DIGIT_HI[count - 1], M.INT32_MAX)
    rng = np.random.default_rng(count)
    x = np.concatenate([[lo, hi, lo + 1, hi - 1, 0, -1, 1], rng.integers(lo, hi + 1, 500)]).astype(np.int64)
    d = M.digits(x, count).astype(np.int64)
    assert d.min() >= -128 and d.max() <= 127
    assert np.array_equal(sum(d[a] << (8 * a) for a in range(count)), x)
    if count < 5:
        with pytest.raises(AssertionError):
            M.digits(np.array([M.DIGIT_HI[count - 1] + 1]), count)
        with pytest.raises(AssertionError):
            M.digits(np.array([M.DIGIT_LO[count - 1] - 1]), count)


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(n):
    """24-bit Gaussian material (three digits) at every length where the tiling changes"""
    rng = np.random.default_rng(n)
    x = np.clip(np.rint(rng.standard_normal(n) * 2.0 ** 20), -2 ** 23, 2 ** 23 - 1).astype(np.int64)
    assert M.acf_int(x) == M.acf_exact(x)


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("side", ["lo", "hi"])
def test_digit_boundaries(d, side):
    """one sample on a boundary of the digit table and one just beyond it (both sides of the table)"""
    edge = M.DIGIT_LO[d - 1] if side == "lo" else M.DIGIT_HI[d - 1]
    step = -1 if side == "lo" else 1
    rng = np.random.default_rng(10 * d + (side == "hi"))
    for value, want in ((edge, d), (edge + step, d + 1)):
        if not M.INT32_MIN <= value <= M.INT32_MAX:
            continue
        x = rng.integers(-100, 100, 300).astype(np.int64)
        x[[0, 17, 299]] = value
        st = {}
        assert M.acf_int(x, st) == M.acf_exact(x)
        assert st["digits"] == want


def test_int32_extremes():
    """INT32_MIN and INT32_MAX as single samples, the constant INT32_MIN block and the alternating INT32_MAX / INT32_MIN
    block of 16384 samples: the i32 cells and lag sums hold (asserted inside the model)"""
    st = {}
    for v in (M.INT32_MIN, M.INT32_MAX):
        x = np.zeros(300, np.int64)
        x[[3, 200]] = v
        assert M.acf_int(x, st) == M.acf_exact(x)
    x = np.full(16384, M.INT32_MIN, np.int64)
    assert M.acf_int(x, st) == M.acf_exact(x) and st["digits"] == 4
    x = np.where(np.arange(16384) % 2 == 0, M.INT32_MAX, M.INT32_MIN).astype(np.int64)
    assert M.acf_int(x, st) == M.acf_exact(x) and st["digits"] == 5
    print("largest |cell| 2^%.1f, largest per-weight lag sum 2^%.1f" % (np.log2(st["max_cell"]), np.log2(st["max_lag_sum"])))
    assert st["max_cell"] < 2 ** 27 and st["max_lag_sum"] < 2 ** 31


def test_all_zero_block():
    assert M.acf_int(np.zeros(4096, np.int64)) == [0] * M.LAGS


def test_scaling_rounds_once():
    """the stored double is the integer rounded once: exact below 2^53, else within half an ulp"""
    assert M.scaled(2 ** 53 - 1, 8192) == (2 ** 53 - 1) * 2.0 ** -50
    assert M.scaled(2 ** 76 + 2 ** 23 + 1, 32768) == (2 ** 76 + 2 ** 24) * 2.0 ** -48
