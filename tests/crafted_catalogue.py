"""A catalogue of legal .sla streams that the project's encoder never writes (test infrastructure).

Every stream is written field by field with tests/slastream.py: PARCOR codes at the ends of their fields and with
every shift, unstable lattices, long-term taps at full scale, even tap counts and pitches beyond what an analysis
picks, initial Rice parameters on both sides of the Golomb threshold and beyond 2^24, quotients at the gamma
boundary, residuals at the ends of int32, tiles that cost more than 64 bits per sample, 4/12/20/32-bit formats,
33-bit side channels, 1/2/3/8 channels and block lengths from 1 to 16384.  tests/test_crafted_streams.py pins the
oracle's decoder to the reference on all of them; tests/test_gpu_crafted_streams.py puts them through the HIP
decoders.  The module docstring of tests/test_crafted_streams.py lists what is left out and why.
"""
import functools
from dataclasses import dataclass

import numpy as np

import slastream as SS

# capacity of every decode of the catalogue: channels, block samples, PARCOR order, long-term taps, LMS order
CAP = (8, 16384, 255, 5, 32)
LTM_BUFFER_TAPS = CAP[3]       # the reference decoder's ring buffer holds 2 * (max taps + 256) words


@dataclass
class Case:
    name: str
    fmt: SS.Format
    blocks: list
    data: bytes = b""
    stats: SS.Stats = None
    offsets: list = None

    @property
    def num_samples(self):
        return sum(b.n for b in self.blocks)


def _codes(rng, order, full=True):
    """PARCOR codes: uniform over the whole field (an unstable filter), or small ones (a gentle filter)"""
    out = []
    for o in range(1, order + 1):
        lim = (1 << 15) if o < 4 else (1 << 7)
        if not full:
            lim = lim // 8
        out.append(int(rng.integers(-lim, lim)))
    return out


def _res(rng, n, bits):
    """residuals of `bits` magnitude bits; 31 = the whole int32 range"""
    if bits >= 31:
        return rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    return rng.integers(-(1 << bits), 1 << bits, n, dtype=np.int64).astype(np.int32)


def _chan(rng, fmt, n, bits=10, rshift=0, codes=None, ltm=None, init=None, res=None, full=True):
    return SS.Chan(rshift, _codes(rng, fmt.order, full) if codes is None else codes, ltm, init,
                   _res(rng, n, bits) if res is None else res)


def _comp(rng, fmt, n, **kw):
    return SS.Block(SS.COMPRESS, n, [_chan(rng, fmt, n, **kw) for _ in range(fmt.num_channels)])


def _raw(rng, fmt, n):
    """random RAW codes of the full field width.  A 33-bit field keeps its top bit clear where the reference reads it
    with exactly one bit left in its byte buffer (a field that starts at bit 7 of a byte; see test_crafted_streams)"""
    widths = SS.raw_widths(fmt)
    raw = [rng.integers(0, 1 << w, n, dtype=np.uint64) for w in widths]
    for ch, w in enumerate(widths):
        if w > 32:
            start = np.arange(n) * sum(widths) + sum(widths[:ch])     # from the body's start, which is byte-aligned
            raw[ch][start % 8 == 7] &= np.uint64(SS.M32)
    return SS.Block(SS.RAW, n, raw=raw)


def adaptive_codes(init, n, choose):
    """folded residuals for one channel of a recursive-Rice block, chosen sample by sample from the parameters the
    decoder will hold at that sample: choose(i, m0, m1) -> code, with m0 / m1 the moduli of the first / tail stage"""
    p = [SS._rp_set(init)] * 2
    out = np.zeros(n, np.uint64)
    for i in range(n):
        m0, m1 = SS._rp_rice(p[0]), SS._rp_rice(p[1])
        c = int(choose(i, m0, m1)) & SS.M32
        out[i] = c
        p[0] = SS._rp_update(p[0], c)
        if c >= m0:
            p[1] = SS._rp_update(p[1], c - m0)
    return out


def _parcor_cases():
    out = []
    rng = np.random.default_rng(101)
    f = SS.Format(2, 16, order=8, ntaps=1, lms=8)
    ext = [-32768, 32767, -32768, 127, -128, 127, -128, 127]
    blocks = [SS.Block(SS.COMPRESS, 4096, [_chan(rng, f, 4096, 12, codes=ext), _chan(rng, f, 4096, 12, codes=[-c - 1 for c in ext])]),
              SS.Block(SS.COMPRESS, 3000, [_chan(rng, f, 3000, 31, codes=ext, rshift=15), _chan(rng, f, 3000, 31, codes=ext[::-1] * 1)])]
    out.append(Case("parcor_field_extremes", f, blocks))
    f = SS.Format(1, 16, order=4, ntaps=1, lms=4)
    out.append(Case("parcor_every_rshift", f, [_comp(rng, f, 512, bits=14, rshift=r) for r in range(16)]))
    for order in (1, 16, 17, 32, 33, 64, 65, 128, 255):
        f = SS.Format(2 if order in (17, 65) else 1, 24, order=order, ntaps=1, lms=16)
        blocks = [_comp(rng, f, 1500, bits=12, rshift=int(rng.integers(0, 16))),
                  _comp(rng, f, 700, bits=20, rshift=0, full=False)]
        out.append(Case("parcor_order_%d" % order, f, blocks))
    # an unstable lattice on a full-range input: its k * b products wrap int32 (asserted by the GPU coverage test)
    f = SS.Format(1, 32, order=6, ntaps=1, lms=4)
    out.append(Case("parcor_wrapping_products", f, [_comp(rng, f, 2048, bits=31, codes=[32767, -32768, 32767, 127, -128, 127])]))
    return out


def _ltm_cases():
    out = []
    for ntaps in range(1, 6):
        rng = np.random.default_rng(200 + ntaps)
        f = SS.Format(2, 16, order=4, ntaps=ntaps, lms=8)
        top = LTM_BUFFER_TAPS + 256 - ntaps // 2          # the largest pitch inside the reference's ring buffer
        low = (ntaps + 1) // 2
        ext = [32767 if (k & 1) else -32768 for k in range(ntaps)]

        def taps():
            return [int(t) for t in rng.integers(-32768, 32768, ntaps)]

        blocks = []
        for pitch, tp in [(100, ext), (3, taps()), (max(low, 1), taps()), (255, taps()), (256, ext), (top, taps()), (top, ext)]:
            blocks.append(SS.Block(SS.COMPRESS, 2048, [_chan(rng, f, 2048, 14, ltm=(pitch, tp), full=False),
                                                       _chan(rng, f, 2048, 14, ltm=None, full=False)]))
        blocks.append(SS.Block(SS.COMPRESS, 1000, [_chan(rng, f, 1000, 14, ltm=(0, taps()), full=False),     # flag set, pitch 0
                                                   _chan(rng, f, 1000, 14, ltm=(17, ext), full=False)]))
        for dn in (-1, 0, 1):                                # delay = pitch + taps/2 equal to n - 1, n, n + 1
            pitch = 40
            n = pitch + ntaps // 2 - dn
            blocks.append(SS.Block(SS.COMPRESS, n, [_chan(rng, f, n, 14, ltm=(pitch, ext), full=False),
                                                    _chan(rng, f, n, 14, ltm=(pitch, taps()), full=False)]))
        out.append(Case("ltm_taps_%d" % ntaps, f, blocks))
    return out


def _rice_cases():
    out = []
    rng = np.random.default_rng(300)
    f = SS.Format(1, 16, order=4, ntaps=1, lms=4)
    blocks = []
    for init in (0, 1, 8, 9, 10):
        blocks.append(_comp(rng, f, 1024, bits=3, init=init, full=False))
    out.append(Case("rice_init_threshold", f, blocks))
    # Golomb with non-power-of-two moduli: channel averages of exactly 8 (Golomb) and 9 (recursive Rice)
    for C, inits in [(8, [57, 1, 1, 1, 1, 1, 1, 1]), (8, [65, 1, 1, 1, 1, 1, 1, 1]), (3, [20, 3, 1]), (3, [21, 5, 1]),
                     (2, [11, 5]), (8, [9, 7, 10, 6, 11, 5, 12, 4])]:
        f = SS.Format(C, 16, order=4, ntaps=1, lms=4)
        chans = [_chan(rng, f, 2000, res=rng.integers(-4 * m, 4 * m, 2000).astype(np.int32), init=m, full=False) for m in inits]
        out.append(Case("rice_mixed_inits_%s" % "_".join(map(str, inits)), f, [SS.Block(SS.COMPRESS, 2000, chans)]))
    # initial parameters at and beyond 2^24: SLACODER_PARAMETER_SET's `init << 8` wraps in 32 bits
    f = SS.Format(2, 32, order=4, ntaps=1, lms=4)
    blocks = []
    for a, b, bits in [(1 << 16, 1 << 16, 31), ((1 << 24) - 1, 9, 31), ((1 << 32) - 1, (1 << 32) - 1, 31),
                       ((1 << 24) + 5, (1 << 31) + 3, 4),      # wrap to 5 and 3: Golomb
                       (1 << 24, 1 << 24, 1)]:                  # both wrap to 0: Golomb with m = 1
        blocks.append(SS.Block(SS.COMPRESS, 1500, [_chan(rng, f, 1500, bits, init=a), _chan(rng, f, 1500, bits, init=b)]))
    out.append(Case("rice_init_wide", f, blocks))
    # quotients 15 / 16 / 17 around the gamma escape, and int32's extremes
    f = SS.Format(1, 24, order=4, ntaps=1, lms=8)
    qs = [15, 16, 17, 1, 2, 16, 0, 17, 15, 300, 16]
    codes = adaptive_codes(5000, 3000, lambda i, m0, m1: (m0 + m1 * (qs[i % len(qs)] - 1) + (i * 7919) % m1)
                           if qs[i % len(qs)] else (i % m0))
    ext = np.array([-(1 << 31), (1 << 31) - 1, -1, 0, 1] * 400, np.int32)
    out.append(Case("rice_gamma_boundary_and_int32_extremes", f,
                    [SS.Block(SS.COMPRESS, 3000, [SS.Chan(0, _codes(rng, 4, False), None, 5000, codes, folded=True)]),
                     SS.Block(SS.COMPRESS, 2000, [SS.Chan(0, _codes(rng, 4, False), None, 1 << 20, ext)]),
                     SS.Block(SS.COMPRESS, 2000, [SS.Chan(0, _codes(rng, 4, False), None, (1 << 24) - 1, ext)])]))
    # tiles of more than 64 bits per sample and channel: codes k * 2^24 + m0 leave both parameters where they are
    # (`code << 8` wraps to m0 << 8, `(code - m0) << 8` to 0), so every sample costs a gamma escape of ~2 x 32 bits
    for C in (1, 2):
        f = SS.Format(C, 16, order=4, ntaps=1, lms=4)
        chans = []
        for ch in range(C):
            ks = rng.integers(1, 256, 4096)
            codes = adaptive_codes(9, 4096, lambda i, m0, m1: (int(ks[i]) << 24) + m0)
            chans.append(SS.Chan(0, _codes(rng, 4, False), None, 9, codes, folded=True))
        out.append(Case("rice_over_64_bits_per_sample_%dch" % C, f, [SS.Block(SS.COMPRESS, 4096, chans)]))
    return out


def _format_cases():
    out = []
    rng = np.random.default_rng(400)
    for bits, lshift in [(4, 0), (4, 2), (12, 0), (12, 5), (20, 0), (20, 7), (32, 0), (32, 9)]:
        for ms in (0, 1):
            f = SS.Format(2, bits, order=8, ntaps=3, lms=8, ms=ms, lshift=lshift)
            amp = max(bits - lshift - 2, 1)
            blocks = [_comp(rng, f, 1200, bits=amp, full=False, ltm=(60, [1000, -20000, 9000])),
                      SS.Block(SS.SILENT, 700), _raw(rng, f, 900), _comp(rng, f, 333, bits=31, init=(1 << bits) - 1),
                      _raw(rng, f, 65), SS.Block(SS.SILENT, 1), _comp(rng, f, 2100, bits=amp)]
            out.append(Case("format_%dbit_lshift%d_ms%d" % (bits, lshift, ms), f, blocks))
    # 32-bit mid/side RAW: the side channel is a 33-bit field.  Its top bit is set only where the reference reads it
    # with more than one bit left in its byte buffer (see tests/test_crafted_streams.py)
    f = SS.Format(2, 32, order=4, ntaps=1, lms=4, ms=1)
    n = 1000
    mid = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    side = rng.integers(0, 1 << 33, n, dtype=np.uint64)
    side[:4] = [0, (1 << 33) - 1, 1 << 32, (1 << 32) - 1]
    side[(np.arange(n) * 65 + 32) % 8 == 7] &= np.uint64(SS.M32)
    out.append(Case("format_32bit_ms_raw_33bit_side", f,
                    [SS.Block(SS.RAW, n, raw=[mid, side]), _comp(rng, f, 500, bits=31), SS.Block(SS.RAW, 7, raw=[mid[:7], side[:7]])]))
    for C in (1, 3, 8):
        f = SS.Format(C, 24, order=16, ntaps=5, lms=16)
        blocks = [_comp(rng, f, 1024, bits=16, ltm=(77, [-32768, 32767, 100, -100, 5])), _raw(rng, f, 300),
                  SS.Block(SS.SILENT, 64), _comp(rng, f, 999, bits=31)]
        out.append(Case("format_%d_channels" % C, f, blocks))
    return out


def _length_cases():
    out = []
    rng = np.random.default_rng(500)
    for lms in (4, 8, 16, 32):
        f = SS.Format(1, 32, order=4, ntaps=1, lms=lms, max_block=16384)
        blocks = [_comp(rng, f, n, bits=31, full=False) for n in (1, lms - 1, lms, 63, 64, 65, 4097, 16384)]
        out.append(Case("lengths_lms%d" % lms, f, blocks))
    return out


@functools.lru_cache(maxsize=None)
def catalogue():
    cases = _parcor_cases() + _ltm_cases() + _rice_cases() + _format_cases() + _length_cases()
    for c in cases:
        c.data, c.stats, c.offsets = SS.write_file(c.fmt, c.blocks)
    return tuple(cases)


def by_name():
    return {c.name: c for c in catalogue()}
