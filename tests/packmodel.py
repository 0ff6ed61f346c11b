"""What the pack stage must produce for a block the independent writer describes (test infrastructure, plain Python / numpy).

Everything here comes from tests/slastream.py -- the block's bytes, the coder mode and the Golomb moduli (`_rp_set` / `_rp_get` and
the threshold 8), the log2 of both Rice moduli before every sample (an `_rp_rice` / `_rp_update` walk) and the body bits of
every channel -- and nothing from the product's packer, so tests/test_gpu_pack.py (the device kernels) and
tests/test_host_logic.py (sla_pack.c) compare against a second opinion.
"""
import functools
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import crafted_catalogue as CC
import slastream as SS

BLOCK_FIXED_BITS = 16 + 32 + 16 + 16 + 2          # sync, size, CRC16, sample count, type
LTM_MIN_PITCH = 3                                 # an encoder sets the long-term flag from this pitch on


def unfold(codes):
    """int32 residuals of folded codes below 2^32 (the inverse of slastream.fold_array)"""
    u = np.asarray(codes, np.uint64) & np.uint64(SS.M32)
    return ((u >> np.uint64(1)).astype(np.int64) ^ -(u & np.uint64(1)).astype(np.int64)).astype(np.int32)


def header_len(fmt, blk):
    """bytes in front of a block's body: the fixed fields and, for a compressed block, every channel's parameters"""
    bits = BLOCK_FIXED_BITS
    if blk.type == SS.COMPRESS:
        coef = 16 * min(fmt.order, 3) + 8 * max(fmt.order - 3, 0)
        for c in blk.chans:
            bits += 4 + coef + 1 + fmt.bits + (SS.LTM_PERIOD_BITS + 16 * fmt.ntaps if c.ltm is not None else 0)
    return (bits + 7) // 8


def coding_mode(inits):
    """per channel: 0 in a recursive-Rice block, the Golomb modulus in a fixed-parameter block (src/SLACoder.c:443-466)"""
    ms = [SS._rp_get(SS._rp_set(i)) for i in inits]
    return [0] * len(ms) if sum(ms) // len(ms) > SS.RICE_LOW_THRESHOLD else ms


def walk(init, codes):
    """k0 | k1 << 8 for every sample: log2 of the first and the tail stage's modulus as they stand before the sample"""
    p0 = p1 = SS._rp_set(init)
    out = np.empty(len(codes), np.uint16)
    for i, c in enumerate([int(x) for x in codes]):
        m0, m1 = SS._rp_rice(p0), SS._rp_rice(p1)
        out[i] = (m0.bit_length() - 1) | ((m1.bit_length() - 1) << 8)
        p0 = SS._rp_update(p0, c)
        if c >= m0:
            p1 = SS._rp_update(p1, c - m0)
    return out


@dataclass
class Expected:
    blk: SS.Block
    data: bytes                                   # the whole block as the writer lays it out
    header_bytes: int
    inits: Optional[List[int]] = None             # COMPRESS: initial parameters as the stream holds them
    golomb_m: Optional[List[int]] = None          # COMPRESS: coding_mode(inits)
    res: Optional[np.ndarray] = None              # COMPRESS: [C][n] int32 residuals
    kk: Optional[List[np.ndarray]] = None         # COMPRESS: per channel walk(), None for a Golomb channel
    chan_bits: Optional[List[int]] = None         # COMPRESS: body bits of every channel
    pcm: Optional[np.ndarray] = None              # RAW: [C][n] left-justified input the codes were derived from, where a test has one

    @property
    def header(self):
        """the header bytes a caller of sla_hip_launch_rice_write supplies: size and CRC16 still zero"""
        h = bytearray(self.data[:self.header_bytes])
        h[2:8] = bytes(6)
        return bytes(h)


def expect_block(fmt, blk, data, chan_bits=None):
    e = Expected(blk, data, header_len(fmt, blk))
    if blk.type == SS.COMPRESS:
        codes, e.inits = SS.block_codes(fmt, blk)
        assert all(int(c.max(initial=0)) <= SS.M32 for c in codes)
        e.golomb_m = coding_mode(e.inits)
        e.res = np.stack([unfold(c) for c in codes]) if blk.n else np.zeros((len(codes), 0), np.int32)
        e.kk = [None if m else walk(i, c) for m, i, c in zip(e.golomb_m, e.inits, codes)]
        e.chan_bits = list(chan_bits)
    return e


def expect_blocks(fmt, blocks):
    """Expected of every block of a list, and the writer's Stats over them"""
    st, out = SS.Stats(), []
    for b in blocks:
        before = len(st.chan_bits)
        data = SS.block_bytes(fmt, b, st)
        out.append(expect_block(fmt, b, data, st.chan_bits[before] if b.type == SS.COMPRESS else None))
    return out, st


@functools.lru_cache(maxsize=None)
def catalogue_expected():
    """{case name: [Expected of every block]} for the crafted catalogue, from the bytes and Stats its build already holds"""
    out = {}
    for case in CC.catalogue():
        ends = list(case.offsets[1:]) + [len(case.data)]
        bits = iter(case.stats.chan_bits)
        out[case.name] = [expect_block(case.fmt, b, case.data[o:e], next(bits) if b.type == SS.COMPRESS else None)
                          for b, o, e in zip(case.blocks, case.offsets, ends)]
        assert next(bits, None) is None
    return out


# ---- what an encoder can express -------------------------------------------------------------------------------

def inexpressible(fmt, blk):
    """None, or why no encoder writes this block (the product's packer takes an encoder's fields, not a stream's):
      * "init": a channel's initial parameter is outside [1, 2^24) or not below 2^bps -- the packer's header writes the rounded
        value of `init << 8` in 32 bits (sla_pack.c: put_block_header), which is the init itself only inside that range;
      * "ltm": the long-term flag is set with a pitch below 3 -- the packer derives the flag from the pitch;
      * "raw": a RAW code has bit 32 set -- the packer folds an int32, and so does every encoder (see tests/test_gpu_pack.py)"""
    if blk.type == SS.COMPRESS:
        codes = [np.asarray(c.res, np.uint64) if c.folded else SS.fold_array(c.res) for c in blk.chans]
        for c, k in zip(blk.chans, codes):
            v = SS.natural_init(k) if c.init is None else int(c.init)
            if not 1 <= v < (1 << 24) or v >= (1 << fmt.bits):
                return "init"
            if c.ltm is not None and c.ltm[0] < LTM_MIN_PITCH:
                return "ltm"
    if blk.type == SS.RAW and any(int(np.asarray(r, np.uint64).max(initial=0)) >> 32 for r in blk.raw):
        return "raw"
    return None


# ---- RAW blocks ------------------------------------------------------------------------------------------------

def full_scale_noise(nch, n, bits, seed, corners=True):
    """left-justified PCM, uniform over the whole `bits`-bit range, the corner pairs (min, max), (max, min), (min, min),
    (max, max) of channels 0 / 1 first"""
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    x = rng.integers(lo, hi + 1, (nch, n), dtype=np.int64)
    if corners:
        for i, pair in enumerate([(lo, hi), (hi, lo), (lo, lo), (hi, hi)][:n]):
            x[:2, i] = pair[:min(nch, 2)]
    return ((x << (32 - bits)) & SS.M32).astype(np.uint32).view(np.int32)


def raw_codes(pcm, shift, mid_side):
    """the coded values of a RAW block, [C][n] uint64: the samples shifted down to their width and, with mid/side,
    mid = (int32)(l + r wrapped to 32 bits) >> 1, side = (int32)(l - r wrapped to 32 bits), each zig-zag folded
    modulo 2^32.  Spelled in int64 with explicit masks; at 32 bits the sums wrap, and the side code keeps bit 32 of
    its 33-bit field clear"""
    x = np.asarray(pcm, np.int32).astype(np.int64) >> shift

    def int32(v):
        v = v & SS.M32
        return np.where(v >> 31, v - (1 << 32), v)

    if mid_side:
        assert x.shape[0] == 2
        l, r = x[0], x[1]
        x = np.stack([int32(l + r) >> 1, int32(l - r)])
    u = (x << 1) & SS.M32
    return [np.where(row < 0, ~urow & SS.M32, urow).astype(np.uint64) for row, urow in zip(x, u)]
