"""numpy model of the silence run list (include/sla_hip.h, sla_hip_launch_zero_runs), written from its definition:

    every maximal run of zero samples inside a segment that is at least `min_run` samples long, or that ends at the
    segment's last sample whatever its length; a run never crosses a segment boundary.

Nothing here is derived from the kernels or from the encoder's host code."""
import numpy as np


def mask_words(bits, span=None):
    """bool array (True = some channel is non-zero) -> the prepass mask: uint64 words, bit s of word s // 64 = sample s,
    bits at or above the span zero"""
    bits = np.asarray(bits, bool)
    span = len(bits) if span is None else span
    padded = np.zeros(max((span + 63) // 64, 1) * 64, np.uint8)
    padded[:span] = bits[:span]
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1).copy()


def mask_bits(words, span):
    """the inverse: uint64 words -> bool array of `span` samples"""
    return np.unpackbits(np.asarray(words, "<u8").view(np.uint8), bitorder="little")[:span].astype(bool)


def zero_runs(bits, segments=None, min_run=2048):
    """bits: bool array over the whole span; segments: list of (start, length), default one segment = everything.
    Returns the run list as a sorted list of (start, length)."""
    bits = np.asarray(bits, bool)
    if segments is None:
        segments = [(0, len(bits))]
    out = []
    for lo, n in segments:
        if n == 0:
            continue
        z = np.concatenate(([False], ~bits[lo:lo + n], [False]))
        edge = np.flatnonzero(z[1:] != z[:-1])                 # run starts at even entries, ends (exclusive) at odd ones
        for a, b in zip(edge[0::2], edge[1::2]):
            if b - a >= min_run or b == n:
                out.append((int(lo + a), int(b - a)))
    return sorted(out)


def rebuilt_bits(runs, span):
    """the mask of someone who knows the run list only: every sample outside the listed runs is non-zero"""
    bits = np.ones(span, bool)
    for a, n in runs:
        bits[a:a + n] = False
    return bits
