"""Inputs for the encoder with max_num_block_samples above 16384, each encoded by the oracle (test infrastructure).

The format's block length is a 16-bit field and the reference's library writes blocks of up to 65535 samples as soon as the
encode parameter asks for them.  tests/test_long_enc_model.py asserts, on the CPU, the coverage claimed here (block lengths
and types of every case, the split, the RAW and SILENT blocks, the boundary lengths) and pins the host planner to the
oracle's partitions; tests/test_gpu_long_enc.py puts every case through the HIP encoder's long-block routes.

Files stay at or below about 150000 samples and order 16 (one order-32 case of one super-frame) so that the oracle's 65-node
partition search stays at a few seconds.
"""
import functools
from dataclasses import dataclass

import numpy as np

import slalibs as S
import waveforms as W

# capacity of every handle that encodes or decodes these files: channels, block samples, PARCOR order, long-term taps, LMS order
CAP = (8, 65535, 255, 5, 32)
COMPRESS, SILENT, RAW = 0, 1, 2


@dataclass
class EncCase:
    name: str
    pcm: np.ndarray               # planar left-justified int32 [C][N]
    bits: int
    order: int
    ltm: int
    lms: int
    ms: int
    max_block: int
    data: bytes = None            # the oracle's .sla bytes
    trace: object = None          # the oracle's trace (slalibs.Trace)

    @property
    def num_channels(self):
        return self.pcm.shape[0]

    @property
    def num_samples(self):
        return self.pcm.shape[1]

    def params(self):
        return S.make_params(self.num_channels, self.bits, 48000, self.order, self.ltm, self.lms, self.ms, 1, self.max_block, cap=CAP)

    def blocks(self):
        nb = self.trace.num_blocks
        return [(int(n), int(t)) for n, t in zip(self.trace.blk_nsmpl[:nb], self.trace.blk_type[:nb])]


def _changing(n, at, bits):
    """a quiet low tone up to `at`, loud coloured noise behind it: a super-frame whose best partition is not one block"""
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(41)
    x = 0.02 * np.sin(2 * np.pi * 110.0 * t / 48000.0)
    e = rng.standard_normal(n)
    x[at:] = 0.45 * np.clip(0.5 * (e[at:] + np.roll(e, 1)[at:]), -2.0, 2.0)
    full = float(1 << (bits - 1))
    q = np.clip(np.rint(x * full), -full, full - 1).astype(np.int64)
    return np.ascontiguousarray((q << (32 - bits)).astype(np.int32))[None, :]


def _with_silence():
    x = W.music_like(1, 115000, 24, seed=9)
    x[:, 30000:70000] = 0          # a SILENT run of 40000 samples
    x[:, 90000:] = 0               # the file ends in 25000 samples of silence
    return x


def _inputs():
    return [
        # blocks of exactly 65535 and 32768 samples, mid/side, 3 and 1 long-term taps
        EncCase("stereo16_ms_140000_max65535", W.music_like(2, 140000, 16, seed=3), 16, 16, 3, 8, 1, 65535),
        EncCase("stereo16_ms_70000_max32768", W.music_like(2, 70000, 16, seed=3), 16, 16, 1, 8, 1, 32768),
        # file length = max: one super-frame the oracle splits into unequal parts
        EncCase("mono16_changing_65535_max65535", _changing(65535, 23000, 16), 16, 16, 1, 16, 0, 65535),
        # file length = max - 1: one RAW block of full-scale noise
        EncCase("mono16_white_19999_max20000", W.gen("white", 1, 19999, 16, seed=5), 16, 8, 1, 8, 0, 20000),
        # a SILENT run over 16384 and silence at the end of the file, 24 bits, 5 taps
        EncCase("mono24_silence_115000_max65535", _with_silence(), 24, 16, 5, 32, 0, 65535),
        # max 16385: file lengths max and max + 2047
        EncCase("stereo24_16385_max16385", W.music_like(2, 16385, 24, seed=12), 24, 16, 3, 8, 0, 16385),
        EncCase("mono16_18432_max16385", W.music_like(1, 16385 + 2047, 16, seed=13), 16, 16, 1, 8, 0, 16385),
        # max + 2048
        EncCase("stereo16_ms_34816_max32768", W.music_like(2, 32768 + 2048, 16, seed=14), 16, 16, 5, 8, 1, 32768),
        # eight channels
        EncCase("eight16_22048_max20000", W.music_like(8, 20000 + 2048, 16, seed=15), 16, 4, 5, 4, 0, 20000),
        # order 32, one super-frame
        EncCase("mono24_order32_65535_max65535", W.music_like(1, 65535, 24, seed=16), 24, 32, 1, 8, 0, 65535),
    ]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for c in _inputs():
        ret, c.data, c.trace = S.oracle().encode_trace(c.params(), c.pcm)
        assert ret == 0, c.name
        out.append(c)
    return tuple(out)


def by_name():
    return {c.name: c for c in cases()}


# (the names without the oracle's work, for parametrised tests)
NAMES = ("stereo16_ms_140000_max65535", "stereo16_ms_70000_max32768", "mono16_changing_65535_max65535", "mono16_white_19999_max20000",
         "mono24_silence_115000_max65535", "stereo24_16385_max16385", "mono16_18432_max16385", "stereo16_ms_34816_max32768",
         "eight16_22048_max20000", "mono24_order32_65535_max65535")


def ordinary_pcm():
    """an ordinary short stereo file for batches that mix it with long-block ones (a batch shares its handle's parameters)"""
    return W.music_like(2, 9000, 16, seed=60)
