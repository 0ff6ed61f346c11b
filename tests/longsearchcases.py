"""Two 24-bit inputs for the long-block tile-sum search (option "long_tile_search"), each encoded by the oracle as
tests/longenccases.py encodes its cases.  The ten cases there are either 16-bit (every search group under the exactness limit
of exact_bits 53) or 24-bit at ordinary loudness (every group over it); these two fill the gap on 24-bit material:

    * quiet throughout: every (super-frame, channel) group under the limit -- for a 65535-sample window that is about
      -31 dBFS rms -- so nothing is rerun;
    * a quiet first super-frame and a loud second: the groups of the second are flagged and rerun as far chains, those of the
      first keep their tile-sum results.

Both keep their low bits alive, so the unit of the samples stays 2^-23.  tests/test_long_search_model.py asserts the split."""
import functools

import numpy as np

import longenccases as E
import waveforms as W

QUIET = 0.004                      # music_like's level: peaks near 2^15 in 24 bits


def _quiet():
    return W.music_like(2, 70000, 24, seed=31, level=QUIET)


def _mixed():
    a = W.music_like(2, 65535, 24, seed=32, level=QUIET)
    b = W.music_like(2, 20000, 24, seed=33, level=0.5)
    return np.ascontiguousarray(np.concatenate([a, b], axis=1))


def _inputs():
    return [
        E.EncCase("stereo24_ms_quiet_70000_max65535", _quiet(), 24, 16, 3, 8, 1, 65535),
        E.EncCase("stereo24_quiet_then_loud_85535_max65535", _mixed(), 24, 16, 1, 8, 0, 65535),
    ]


@functools.lru_cache(maxsize=None)
def inputs():
    """the cases without the oracle's work (the CPU model needs only the samples)"""
    return tuple(_inputs())


@functools.lru_cache(maxsize=None)
def cases():
    import slalibs as S
    out = []
    for c in _inputs():
        ret, c.data, c.trace = S.oracle().encode_trace(c.params(), c.pcm)
        assert ret == 0, c.name
        out.append(c)
    return tuple(out)


def by_name():
    return {c.name: c for c in cases()}


NAMES = ("stereo24_ms_quiet_70000_max65535", "stereo24_quiet_then_loud_85535_max65535")
