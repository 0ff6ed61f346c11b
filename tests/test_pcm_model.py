"""Device-free checks of tests/pcmmodel.py, the model the ingest and unpack kernels are held against: the numpy F32
quantiser against the same rule in exact rational arithmetic, the S32 range, the round trips include/sla_hip.h promises,
and the entry model's strides and zero gap."""
import numpy as np
import pytest

import pcmmodel as P
from pcmmodel import F32, S16, S32, S32_LEFT
from test_gpu_encode_batch_device import crafted_floats


def quantiser_inputs(bps):
    """2535 floats: the crafted ones, the edges of the grid, uniform noise, and ties (k + 1/2) steps around +-full scale"""
    rng = np.random.default_rng(1000 + bps)
    u = 2.0 ** -(bps - 1)
    top = 1 << (bps - 1)
    k = np.concatenate([np.arange(top - 125, top + 125), np.arange(-top - 125, -top + 125)]).astype(np.float64)
    parts = [crafted_floats(bps), P.quantiser_edges(bps), rng.uniform(-1.1, 1.1, 2000).astype(np.float32),
             ((k + 0.5) * u).astype(np.float32)]
    return np.concatenate(parts)


@pytest.mark.parametrize("bps", [1, 2, 8, 12, 16, 20, 24, 25, 32])
def test_the_numpy_quantiser_is_the_exact_one(bps):
    x = quantiser_inputs(bps)
    assert x.dtype == np.float32 and len(x) == 2535
    got = P.left(x, F32, bps)
    want = np.array([P.exact_left_f32(v, bps) for v in x], np.int64)
    bad = np.nonzero(got.astype(np.int64) != want)[0]
    assert bad.size == 0, (bps, bad[:8], x[bad[:8]], got[bad[:8]], want[bad[:8]])
    # what the header names: ties to even, saturation at both ends, the infinities
    top = 1 << (bps - 1)
    sat = {np.inf: top - 1, -np.inf: -top, 3.0e38: top - 1, -3.0e38: -top, 1.0: top - 1, -1.0: -top}
    for v, q in sat.items():
        assert P.exact_left_f32(np.float32(v), bps) == int(P.wrap32(q << (32 - bps))), (bps, v)
    assert P.exact_left_f32(np.float32(np.nan), bps) is None and P.left(np.array([np.nan], np.float32), F32, bps) is None


def test_exact_quantiser_rounds_ties_to_even():
    u = 2.0 ** -15
    q = [P.exact_left_f32(np.float32(k * u), 16) >> 16 for k in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.75, -0.75)]
    assert q == [0, 2, 2, 0, -2, -2, 1, -1]


@pytest.mark.parametrize("bps", [1, 8, 16, 24, 32])
def test_s32_refuses_exactly_what_is_out_of_range(bps):
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    rng = np.random.default_rng(bps)
    cand = [lo - 2, lo - 1, lo, lo + 1, -1, 0, 1, hi - 1, hi, hi + 1, hi + 2, -2 ** 31, 2 ** 31 - 1]
    cand += [int(v) for v in rng.integers(-2 ** 31, 2 ** 31, 200)]
    cand = [v for v in cand if -2 ** 31 <= v <= 2 ** 31 - 1]
    for v in cand:
        got = P.left(np.array([0, v, 0], np.int32), S32, bps)
        inside = lo <= v <= hi
        assert (got is not None) == inside, (bps, v)
        assert bool(P.offenders(np.array([v], np.int32), S32, bps)[0]) == (not inside), (bps, v)
        if inside:
            assert int(got[1]) == int(P.wrap32(v << (32 - bps))), (bps, v)
    if bps == 32:
        assert all(P.left(np.array([v], np.int32), S32, 32) is not None for v in cand)
    else:
        assert P.left(np.array([hi + 1], np.int32), S32, bps) is None and P.left(np.array([lo - 1], np.int32), S32, bps) is None


@pytest.mark.parametrize("fmt,depths", [(S32_LEFT, (1, 8, 16, 24, 32)), (S32, (1, 8, 16, 24, 32)), (S16, (1, 8, 16)),
                                        (F32, (1, 8, 16, 24))], ids=["s32_left", "s32", "s16", "f32"])
def test_elements_then_left_is_the_identity(fmt, depths):
    for bps in depths:
        rng = np.random.default_rng(10 * fmt + bps)
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        q = np.concatenate([[lo, hi, -1, 0, 1, lo + 1, hi - 1], rng.integers(lo, hi + 1, 3000)]).astype(np.int64)
        q = np.clip(q, lo, hi)
        words = P.wrap32(q << (32 - bps))
        back = P.left(P.elements(words, fmt, bps), fmt, bps)
        assert back is not None and back.dtype == np.int32
        assert np.array_equal(back, words), (fmt, bps)


def test_ingest_expect_honours_strides_and_the_zero_gap():
    src = np.arange(100, dtype=np.int32) * 3 - 50
    e = {"src_off": 5, "channel_stride": 1, "sample_stride": 2, "num_samples": 7, "fill_end": 10, "bits_per_sample": 16}
    words, err, bad = P.ingest_expect(src, e, S32_LEFT, 2)
    assert words.shape == (2, 10) and err == 0 and bad == []
    assert np.array_equal(words[0, :7], src[5:19:2]) and np.array_equal(words[1, :7], src[6:20:2])
    assert (words[:, 7:] == 0).all()
    e = {"src_off": 0, "channel_stride": 40, "sample_stride": 3, "num_samples": 4, "fill_end": 0, "bits_per_sample": 8}
    src = np.zeros(100, np.int32)
    src[[0, 3, 6, 9]] = [-128, 127, 128, -1]
    src[[40, 43, 46, 49]] = [1, -129, 0, 5]
    words, err, bad = P.ingest_expect(src, e, S32, 2)
    assert err == P.ERR_RANGE and bad == [(0, 2), (1, 1)]
    assert list(words[0]) == [-128 << 24, 127 << 24, 0, -1 << 24] and list(words[1]) == [1 << 24, 0, 0, 5 << 24]
    f = np.array([0.5, np.nan, -1.0], np.float32)
    words, err, bad = P.ingest_expect(f, dict(e, channel_stride=0, sample_stride=1, num_samples=3, bits_per_sample=16), F32, 1)
    assert err == P.ERR_NAN and bad == [(0, 1)] and list(words[0]) == [1 << 30, 0, -2 ** 31]
    words, err, bad = P.ingest_expect(f, dict(e, num_samples=0, fill_end=6), F32, 3)
    assert words.shape == (3, 6) and not words.any() and err == 0 and bad == []


def test_unpack24_expect():
    raw = bytes([0x01, 0x02, 0x03, 0xFF, 0xFF, 0x7F, 0x00, 0x00, 0x80, 0xAA])
    assert list(P.unpack24_expect(raw, 3)) == [0x03020100, 0x7FFFFF00, -2 ** 31]
    assert len(P.unpack24_expect(raw, 0)) == 0
