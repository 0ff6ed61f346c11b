"""A device-free model of the sample conversions of the encode side (include/sla_hip.h: the table of
sla_hip_encode_batch_device, sla_hip_enc_ingest, sla_hip_launch_unpack16 / _unpack24): elements of the four sample formats to
the left-justified int32 words of the planes and back, one table entry of sla_hip_launch_enc_ingest_batch as the planes
should hold it, the F32 quantiser once more in exact rational arithmetic, and the three-byte unpack.  Written from the
header's text; the tests hold the kernels of kernels/ingest.inc and kernels/pack.inc against it."""
import math
from fractions import Fraction

import numpy as np

S32_LEFT, S32, S16, F32 = range(4)
DTYPES = {S32_LEFT: np.int32, S32: np.int32, S16: np.int16, F32: np.float32}
ERR_RANGE, ERR_NAN = 1, 2                                 # the bits of d_error


def wrap32(a):
    """int64 values -> int32 of their low 32 bits"""
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def left(x, fmt, bps):
    """the table of sla_hip_encode_batch_device in numpy: elements -> left-justified int32 words; None: the item is refused"""
    x = np.asarray(x)
    if fmt == S32_LEFT:
        return x.astype(np.int32)
    if fmt == S16:
        return wrap32(x.astype(np.int64) << 16)
    if fmt == S32:
        v = x.astype(np.int64)
        if (v < -(1 << (bps - 1))).any() or (v > (1 << (bps - 1)) - 1).any():
            return None
        return wrap32(v << (32 - bps))
    v = x.astype(np.float32)
    if np.isnan(v).any():
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint(v * np.float32(2.0 ** (bps - 1)))            # exact scale, ties to even
    q = np.clip(q.astype(np.float64), -(2.0 ** (bps - 1)), 2.0 ** (bps - 1) - 1).astype(np.int64)
    return wrap32(q << (32 - bps))


def elements(pcm, fmt, bps):
    """what a producer holding left-justified PCM hands over in format fmt (the decode side's conversions)"""
    v = np.asarray(pcm, np.int32)
    if fmt == S32_LEFT:
        return v
    if fmt == S32:
        return v >> np.int32(32 - bps)
    if fmt == S16:
        return (v >> np.int32(16)).astype(np.int16)
    return v.astype(np.float32) * np.float32(2.0 ** -31)


def exact_left_f32(v, bps):
    """the F32 row of the table for one float, in rational arithmetic: q = v * 2^(bps-1) rounded to the nearest integer, ties
    to even, saturated to [-2^(bps-1), 2^(bps-1) - 1] (+-inf saturate), then q << (32 - bps) as an int32.  None for a NaN."""
    v = float(v)
    top = 1 << (bps - 1)
    if math.isnan(v):
        return None
    if math.isinf(v):
        q = top - 1 if v > 0 else -top
    else:
        x = Fraction(v) * top
        q = math.floor(x)
        rest = x - q
        if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and q % 2 == 1):
            q += 1
        q = min(max(q, -top), top - 1)
    w = (q << (32 - bps)) & 0xFFFFFFFF
    return w - (1 << 32) if w >= 1 << 31 else w


def quantiser_edges(bps):
    """floats at the edges of the F32 quantiser of a bps-bit file: the largest float below 1 and its negative, and the two
    floats just below and just above half a step of the grid"""
    u = np.float32(2.0 ** -(bps - 1))
    below_one = np.nextafter(np.float32(1), np.float32(0))
    return np.array([below_one, -below_one, np.float32(0.49999997) * u, np.float32(0.50000006) * u], np.float32)


def offenders(x, fmt, bps):
    """boolean mask of the elements that refuse their file: an S32 value outside the depth's range, an F32 NaN"""
    x = np.asarray(x)
    if fmt == S32:
        v = x.astype(np.int64)
        return (v < -(1 << (bps - 1))) | (v > (1 << (bps - 1)) - 1)
    if fmt == F32:
        return np.isnan(x.astype(np.float32))
    return np.zeros(x.shape, bool)


def ingest_expect(src, entry, fmt, C):
    """One entry of sla_hip_launch_enc_ingest_batch.  src: the numpy source buffer (elements of the format's type); entry: a
    mapping with src_off (the element of src that is sample 0 of channel 0), channel_stride, sample_stride, num_samples,
    fill_end, bits_per_sample.  Returns (words, err, bad): the plane words int32 [C][max(num_samples, fill_end)] -- the
    converted samples, then the zero gap --, the bits the file's error word gets, and the (channel, sample) positions of the
    offending elements, whose plane words (0 here) are not part of the contract."""
    n, bps = int(entry["num_samples"]), int(entry["bits_per_sample"])
    lim = max(n, int(entry["fill_end"]))
    cs, ss, off = int(entry["channel_stride"]), int(entry["sample_stride"]), int(entry["src_off"])
    at = off + np.arange(C, dtype=np.int64)[:, None] * cs + np.arange(n, dtype=np.int64)[None, :] * ss
    x = np.asarray(src)[at].astype(DTYPES[fmt])
    bad = offenders(x, fmt, bps)
    words = np.zeros((C, lim), np.int32)
    words[:, :n] = left(np.where(bad, DTYPES[fmt](0), x), fmt, bps)
    err = 0
    if bad.any():
        err = ERR_RANGE if fmt == S32 else ERR_NAN
    return words, err, [(int(c), int(i)) for c, i in zip(*np.nonzero(bad))]


def unpack24_expect(data, count):
    """sla_hip_launch_unpack24: `count` samples of three little-endian bytes -> the int32's upper three bytes"""
    b = np.frombuffer(bytes(data), np.uint8)[:3 * count].reshape(count, 3).astype(np.uint32)
    return ((b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)).astype(np.uint32).view(np.int32)
