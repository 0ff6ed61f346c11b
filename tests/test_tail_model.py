"""The plain-Python model of the tail stage (tests/tailmodel.py) against the CPU oracle, bit for bit, on the operand families
of tests/test_gpu_tail.py -- and the three properties of those families the GPU test relies on, evaluated on the model:
which inputs make the error INT32_MIN, which drive the coefficients high, which produce the smallest steps."""
import os

import numpy as np
import pytest

import slalibs as S
import tailmodel as M

A_WAV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "a.wav")
ORDERS = (4, 8, 16, 32)


def lengths(order):
    return (1, order - 1, order, order + 1, 1500)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", M.FAMILIES)
def test_lms_model_equals_oracle(oracle, name, order):
    for n in lengths(order) + ((4096,) if order == 8 else ()):
        x = M.family(name, n)
        got = M.lms_predict(x, order)[0]
        assert np.array_equal(got, oracle.lms_predict(x, order)), (name, order, n)
        assert M.fold_sum(got) == int(np.sum(np.where(got < 0, ~(got.astype(np.int64) << 1), got.astype(np.int64) << 1) & 0xFFFFFFFF))


@pytest.mark.parametrize("name", M.FAMILIES)
def test_ltm_model_equals_oracle(oracle, name):
    x = M.family(name, 1500)
    for tapset in M.LTM_TAPS:
        coef = M.taps(tapset)
        for pitch in (0, 3, 7, 100, 255, 1497, 1500, 4000):
            assert np.array_equal(M.ltm_predict(x, pitch, coef), oracle.ltm_predict(x, pitch, coef)), (name, tapset, pitch)
    for n in (1, 3, 5, 6, 7):
        x = M.family(name, n)
        assert np.array_equal(M.ltm_predict(x, 3, M.taps("ends5")), oracle.ltm_predict(x, 3, M.taps("ends5"))), (name, n)


def test_model_on_a_wav_residual(oracle):
    """an ordinary case: the lattice residual of the reference's own test file through both stages"""
    pcm, bits, rate = S.read_wav(A_WAV)
    p = S.make_params(1, bits, rate, 16, 3, 8, 0, 1, 4096)
    ret, _, tr = oracle.encode_trace(p, pcm)
    assert ret == 0 and tr.blk_type[4] == 0 and tr.blk_nsmpl[4] == 4096
    res = tr.res_lattice[0, 16384:16384 + 4096]
    assert res.any()
    for pitch, tapset in ((0, "plain1"), (57, "plain3")):
        y = M.ltm_predict(res, pitch, M.taps(tapset))
        assert np.array_equal(y, oracle.ltm_predict(res, pitch, M.taps(tapset)))
        e = M.lms_predict(y, 8)[0]
        assert np.array_equal(e, oracle.lms_predict(y, 8))


def test_fold_sum_at_the_ends():
    assert M.fold_sum(np.array([0, -1, 1, -2, 2], np.int32)) == 0 + 1 + 2 + 3 + 4
    assert M.fold_sum(np.array([M.INT32_MIN], np.int32)) == 0xFFFFFFFF
    assert M.fold_sum(np.array([M.INT32_MAX], np.int32)) == 0xFFFFFFFE
    assert M.fold_sum(np.full(5, M.INT32_MIN, np.int32)) == 5 * 0xFFFFFFFF          # beyond 32 bits: the sum is 64 bits wide


def test_properties_the_gpu_test_relies_on(oracle):
    """allmin makes the error INT32_MIN (the unsigned reading of max(e, -e)); allmin and ramp take the FIR coefficients
    beyond 2^16 within 8192 samples (24-bit products with large coefficients); small produces errors 0, +-1, +-2, +-3
    (steps 0 and 1, and the count-leading-zeros of 0).  The largest |IIR coefficient| of every family is printed: no
    input is known that drives it high, and nothing is asserted about it."""
    n = 8192
    stats = {}
    for name in M.FAMILIES:
        x = M.family(name, n)
        e, max_f, max_i, num_min = M.lms_predict(x, 8)
        assert np.array_equal(e, oracle.lms_predict(x, 8)), name
        stats[name] = (e, max_f, max_i, num_min)
        print("family %-7s order 8, %d samples: max |FIR coef| %7d  max |IIR coef| %6d  errors == INT32_MIN %5d"
              % (name, n, max_f, max_i, num_min))
    assert stats["allmin"][3] > 0
    assert stats["allmin"][1] >= 2 ** 16 and stats["ramp"][1] >= 2 ** 16
    for order in ORDERS:                                   # the 16384-sample jobs of the GPU test, every order
        seen = set(M.lms_predict(M.family("small", 16384), order)[0][order:].tolist())
        assert {0, 1, -1, 2, -2, 3, -3} <= seen, (order, sorted(seen))
