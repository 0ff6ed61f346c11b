"""Legal .sla streams with blocks of more than 16384 samples (test infrastructure).

The block length is a 16-bit field, so blocks of up to 65535 samples are legal; the project's encoder stops at 16384.
Three streams are written field by field with tests/slastream.py, two come from the oracle's encoder asked for
max_num_block_samples of 65535 and 32768 (its partition search then picks blocks of exactly that length).
tests/test_long_blocks_model.py pins the oracle's decoder to the reference on those whose pitches the reference defines and
asserts the coverage claimed here; tests/test_gpu_long_blocks.py puts all of them through every route of the HIP decoder.
"""
import functools
from dataclasses import dataclass

import numpy as np

import crafted_catalogue as CC
import slalibs as S
import slastream as SS
import waveforms as W

# capacity of every decode of these files: channels, block samples, PARCOR order, long-term taps, LMS order
CAP = (8, 65535, 255, 5, 32)


@dataclass
class LongCase:
    name: str
    data: bytes
    num_samples: int
    num_channels: int
    block_lengths: tuple          # expected, asserted against the bytes by the CPU test
    ltm_channels: int             # (block, channel) pairs of compressed blocks with the long-term flag set and a pitch
    pitches: tuple                # their pitches, sorted
    ref_defined: bool             # every pitch lies inside the reference decoder's ring buffer
    blocks: list = None           # the writer's blocks (crafted files)
    offsets: list = None          # byte offset of every block (crafted files)


def reference_defines(ntaps, pitch, max_taps=CAP[3]):
    """tests/test_crafted_streams.py, 'Left out': ceil(taps / 2) <= pitch <= max taps + 256 - taps / 2"""
    return (ntaps + 1) // 2 <= pitch <= max_taps + 256 - ntaps // 2


def _crafted(name, fmt, blocks):
    data, _, offs = SS.write_file(fmt, blocks)
    lt = [c.ltm[0] for b in blocks if b.type == SS.COMPRESS for c in b.chans if c.ltm is not None and c.ltm[0] != 0]
    return LongCase(name, data, sum(b.n for b in blocks), fmt.num_channels, tuple(b.n for b in blocks), len(lt),
                    tuple(sorted(lt)), all(reference_defines(fmt.ntaps, p) for p in lt), blocks, offs)


def _mono():
    rng = np.random.default_rng(700)
    f = SS.Format(1, 16, order=8, ntaps=5, lms=8, max_block=65535)
    blocks = [CC._comp(rng, f, 65535, bits=9, full=False, ltm=(1023, [3000, -9000, 12000, -7000, 2000])),
              CC._raw(rng, f, 2048),
              CC._comp(rng, f, 40897, bits=9, full=False, ltm=(1, [-4000, 9000, -11000, 6000, 1500])),
              SS.Block(SS.SILENT, 3000),
              CC._comp(rng, f, 16385, bits=11, full=False)]
    return _crafted("mono_16bit_65535_2048raw_40897_3000silent_16385", f, blocks)


def _stereo():
    rng = np.random.default_rng(701)
    f = SS.Format(2, 24, order=16, ntaps=3, lms=16, ms=1, max_block=65535)
    blocks = [SS.Block(SS.COMPRESS, 40000, [CC._chan(rng, f, 40000, 12, ltm=(100, [5000, 14000, -3000]), full=False),
                                            CC._chan(rng, f, 40000, 12, ltm=(258, [-32768, 32767, -32768]), full=False)]),
              SS.Block(SS.COMPRESS, 50000, [CC._chan(rng, f, 50000, 14, ltm=(3, [900, -15000, 7000]), full=False),
                                            CC._chan(rng, f, 50000, 14, ltm=None, full=False)])]
    return _crafted("stereo_24bit_ms_40000_50000", f, blocks)


def _eight():
    rng = np.random.default_rng(702)
    f = SS.Format(8, 16, order=4, ntaps=5, lms=4, max_block=20000)
    ltms = [(3, [100, -200, 9000, 400, -50]), None, (77, [-32768, 32767, 100, -100, 5]), (200, [1000, 2000, 3000, 2000, 1000]),
            (259, [-3000, 5000, 11000, 5000, -3000]), (0, [1, 2, 3, 4, 5]), (64, [0, 0, 20000, 0, 0]), None]
    blocks = [SS.Block(SS.COMPRESS, 20000, [CC._chan(rng, f, 20000, 10, ltm=lt, full=False) for lt in ltms])]
    return _crafted("eight_channels_20000", f, blocks)


def block_lengths(data):
    """the sample counts of the block chain, read from the bytes"""
    data = bytes(data)
    total = int.from_bytes(data[15:19], "big")
    out, off, pos = [], SS.HEADER_SIZE, 0
    while pos < total:
        assert data[off:off + 2] == b"\xff\xff"
        n = int.from_bytes(data[off + 8:off + 10], "big")
        out.append(n)
        off += int.from_bytes(data[off + 2:off + 6], "big") + 6
        pos += n
    return tuple(out)


def _encoded(name, n, max_block, want_lengths):
    pcm = W.music_like(2, n, 16, seed=3)
    p = S.make_params(2, 16, 48000, 16, 3, 8, 1, 1, max_block, cap=CAP)
    ret, data, tr = S.oracle().encode_trace(p, pcm)
    assert ret == 0
    nb = tr.num_blocks
    lt = [int(tr.pitch[b, ch]) for b in range(nb) if tr.blk_type[b] == SS.COMPRESS for ch in range(2) if tr.pitch[b, ch] != 0]
    return LongCase(name, data, n, 2, want_lengths, len(lt), tuple(sorted(lt)), all(reference_defines(3, q) for q in lt))


@functools.lru_cache(maxsize=None)
def cases():
    return (_mono(), _stereo(), _eight(),
            _encoded("encoded_140000_max65535", 140000, 65535, (65535, 65535, 8930)),
            _encoded("encoded_70000_max32768", 70000, 32768, (32768, 32768, 4464)))


def by_name():
    return {c.name: c for c in cases()}


@functools.lru_cache(maxsize=None)
def ordinary_files():
    """encoder-written files of 4096-sample blocks, for batches that mix them with the long-block ones"""
    out = []
    for i, (nch, bits) in enumerate([(2, 16), (1, 24), (8, 16)]):
        pcm = W.music_like(nch, 9000 + 777 * i, bits, seed=60 + i)
        p = S.make_params(nch, bits, 48000, 16, 3, 8, 1 if nch == 2 else 0, 1, 4096, cap=CAP)
        ret, data = S.oracle().encode_whole(p, pcm)
        assert ret == 0
        out.append(data)
    return tuple(out)


def ltm_synth(x, pitch, coef):
    """oracle.ltm_synth with zeros behind the block.  With 5 taps at pitch 1 the last tap of sample s lies at s + 1, so
    the block's last sample reads position n: the decoder's kernels read 0 there (k_dec_ltm: `at < n`), while the oracle's
    loop (oracle/sla_oracle.c: ltm_run) reads out[n] -- one word past the array slalibs.ltm_synth hands it.  Here the
    same function gets an output array two words longer, zero behind the block, so that the read is inside the array and
    finds the 0 the kernels define.  Every other (pitch, taps) never reaches n, and the two calls are the same."""
    x = np.ascontiguousarray(x, np.int32)
    coef = np.ascontiguousarray(coef, np.int32)
    n = len(x)
    out = np.zeros(n + 2, np.int32)
    rc = S.oracle().fn("ltm_synth")(S._ptr(x, S.i32p), S.C.c_uint32(n), S.C.c_uint32(pitch), S._ptr(coef, S.i32p),
                                    S.C.c_uint32(len(coef)), S._ptr(out, S.i32p))
    assert rc == 0 and out[n] == 0 and out[n + 1] == 0
    return out[:n].copy()


def reads_past_the_block(ntaps, pitch):
    """whether the last sample's furthest tap, at s - (pitch + taps / 2) + taps - 1, lies behind the block"""
    return pitch != 0 and ntaps - 1 - (pitch + ntaps // 2) >= 1


def synthesis_chain(case):
    """a crafted file's samples from the writer's fields through the oracle's unit functions (LMS -> long-term -> lattice
    -> de-emphasis, mid/side, left-justification), as tests/test_crafted_streams.py does, with ltm_synth above"""
    from decbitsmodel import kint_of, unfold
    o = S.oracle()
    f = SS.Format(case.num_channels)
    hdr = case.data
    f.bits, f.lshift, f.ntaps, f.lms, f.ms = hdr[23], hdr[24], hdr[26], hdr[27], hdr[28]
    out = np.zeros((f.num_channels, case.num_samples), np.int32)
    pos = 0
    for b in case.blocks:
        buf = np.zeros((f.num_channels, b.n), np.int32)
        if b.type == SS.RAW:
            for ch in range(f.num_channels):
                buf[ch] = unfold(b.raw[ch])
        elif b.type == SS.COMPRESS:
            for ch, c in enumerate(b.chans):
                x = o.lms_synth(np.asarray(c.res, np.int32), f.lms)
                if c.ltm is not None and c.ltm[0] != 0:
                    taps = np.array([SS.fold(t) for t in c.ltm[1]], np.int64)
                    taps = ((((taps >> 1) ^ -(taps & 1)) << 16) & SS.M32).astype(np.uint32).view(np.int32)
                    x = ltm_synth(x, c.ltm[0], taps)
                buf[ch] = o.deemph_i32(o.lattice_synth(x, kint_of(c)))
        if f.ms:
            side = buf[1].astype(np.int64)
            mid = (buf[0].astype(np.int64) << 1) | (side & 1)
            buf[0] = ((((mid + side) & SS.M32).astype(np.uint32).view(np.int32)).astype(np.int64) >> 1).astype(np.int32)
            buf[1] = ((((mid - side) & SS.M32).astype(np.uint32).view(np.int32)).astype(np.int64) >> 1).astype(np.int32)
        sh = 32 - f.bits + f.lshift
        out[:, pos:pos + b.n] = ((buf.astype(np.int64) << sh) & SS.M32).astype(np.uint32).view(np.int32)
        pos += b.n
    return out


def undefined_in_the_oracle_decoder(case):
    """(channel, sample) positions of a crafted file where the oracle's DECODER is not a yardstick: the last sample of a
    block channel whose long-term taps reach behind the block (5 taps at pitch 1).  There its ltm_run reads one word past
    the block in a work buffer that still holds an earlier block's output (or, for a block of the full capacity, past the
    buffer), where the HIP kernels read 0; the reference is undefined for such a pitch altogether."""
    out, pos = [], 0
    ntaps = case.data[26]
    for b in case.blocks or []:
        if b.type == SS.COMPRESS:
            out += [(ch, pos + b.n - 1) for ch, c in enumerate(b.chans) if c.ltm is not None and reads_past_the_block(ntaps, c.ltm[0])]
        pos += b.n
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(result code, samples [C][n]): the yardstick of every route.  The oracle's decoder with capacity CAP; for the
    crafted files its code and the samples of synthesis_chain, which tests/test_long_blocks_model.py holds equal to the
    oracle decoder's everywhere but at undefined_in_the_oracle_decoder (one sample of the mono file)."""
    c = by_name()[name]
    rc, pcm, _ = S.oracle().decode_whole(S.make_params(cap=CAP), c.data, c.num_samples)
    if c.blocks is not None:
        pcm = synthesis_chain(c)
    pcm.setflags(write=False)
    return rc, pcm


@functools.lru_cache(maxsize=None)
def oracle_decoded(name):
    c = by_name()[name]
    rc, pcm, _ = S.oracle().decode_whole(S.make_params(cap=CAP), c.data, c.num_samples)
    return rc, pcm
