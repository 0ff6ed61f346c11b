"""The numpy model of the prepass and of the batch scan (tests/prepassmodel.py) on hand-made inputs, and the values
it takes from the oracle: what the encoder calls silent at 32 bits with mid/side, where L + R and L - R wrap, and the
offset_lshift byte of the file header (prepass_done, the model of the two words of sla_hip_launch_prepass_early)."""
import numpy as np
import pytest

import prepassmodel as M
import slalibs as S
import waveforms as W

INT32_MIN = -2 ** 31


def test_oracle_calls_wrapped_mid_side_silent(oracle):
    """a leading run of L = R = INT32_MIN at 32 bits with mid/side: mid = (L + R) >> 1 and side = L - R are both zero in the
    encoder's wrapping arithmetic, and the oracle's encoder writes a SILENT block over it; the same samples in the left
    channel alone are not silent.  The model's mask says the same."""
    n = 12000
    pcm = np.ascontiguousarray(W.music_like(2, n, 32, seed=3))
    pcm[:, :4096] = INT32_MIN
    p = S.make_params(2, 32, 48000, parcor=16, ltm=1, lms=8, ms=1, max_block=4096)
    ret, _, tr = oracle.encode_trace(p, pcm)
    assert ret == 0 and int(tr.blk_type[0]) == 1 and int(tr.blk_start[0]) == 0 and int(tr.blk_nsmpl[0]) >= 4096
    mask = M.prepass(pcm, 32, 1)[1]
    assert (mask[:64] == 0).all() and mask[64] != 0
    pcm[1, :4096] = 0
    ret, _, tr = oracle.encode_trace(p, pcm)
    assert ret == 0 and int(tr.blk_type[0]) != 1
    assert (M.prepass(pcm, 32, 1)[1][:64] == np.uint64(2 ** 64 - 1)).all()


def test_prepass_model_by_hand():
    pcm = np.zeros((2, 130), np.int32)
    pcm[1, 64] = 1 << 16                                        # the lowest bit of a 16-bit sample
    pcm[0, 129] = 0xFFFF                                        # below the shift: raw bits only
    orw, mask, zero, tiles = M.prepass(pcm, 16, 0)
    assert orw == 0x1FFFF and [int(w) for w in mask] == [0, 1, 0] and zero == 2 and tiles.tolist() == [0x1FFFF, 0, 0, 0]
    pcm[:, 3] = [5 << 16, -5 << 16]                             # mid 0, side 10
    pcm[:, 4] = [1 << 16, 0]                                    # mid 0, side 1
    pcm[:, 5] = [1 << 16, 1 << 16]                              # mid 1, side 0
    assert int(M.prepass(pcm, 16, 1)[1][0]) == 0b111000
    assert M.prepass(np.zeros((3, 0), np.int32), 24, 0)[:1] == (0,)


def test_batch_scan_tail_cases():
    """the model's tail flag on hand-made files: set exactly when 1 <= len % max_block < 127 and those samples are zero"""
    for ln, maxb, want in ((4096 + 126, 4096, 1), (4096 + 127, 4096, 0), (126, 4096, 1), (127, 2048, 0), (1, 16384, 1),
                           (4096, 4096, 0), (4096 + 126, 0, 0), (2048 + 100, 2048, 1), (2048 + 100, 4096, 0)):
        bits = np.ones(8192, bool)
        rem = ln % maxb if maxb else 0
        bits[1024 + ln - rem:1024 + ln] = False
        bits[1024 + ln:] = False
        info = M.batch_scan(M.Z.mask_words(bits), np.full(8, 5, np.uint32), [1024], [ln], maxb)
        assert info[2] == want, (ln, maxb)
        if want:                                                # the tail straddles a word boundary where ln says so; one bit clears it
            for p in (1024 + ln - rem, 1024 + ln - 1):
                b2 = bits.copy()
                b2[p] = True
                assert M.batch_scan(M.Z.mask_words(b2), np.full(8, 5, np.uint32), [1024], [ln], maxb)[2] == 0


def test_prepass_done_by_hand():
    """(OR word, all-zero mask words, bits) -> (cancel, lshift), every branch"""
    table = [
        # nothing to encode: called off, shift 0 -- whatever the count says
        ((0, 0, 16), (1, 0)), ((0, 5, 16), (1, 0)), ((0, 0, 32), (1, 0)), ((0, 1, 8), (1, 0)),
        # the lowest bit of the unit is used: shift 0, and the start stands
        ((1 << 16, 0, 16), (0, 0)), ((0xFFFF0000, 0, 16), (0, 0)), ((1 << 8, 0, 24), (0, 0)), ((1 << 24, 0, 8), (0, 0)),
        ((1, 0, 32), (0, 0)), ((0xFFFFFFFF, 0, 32), (0, 0)),
        # always-zero bits above the unit: that many
        ((1 << 17, 0, 16), (0, 1)), ((0xFFF80000, 0, 16), (0, 3)), ((0xFFF80000, 0, 24), (0, 11)), ((0x00000800, 0, 24), (0, 3)),
        ((0x50000000, 0, 8), (0, 4)), ((8, 0, 32), (0, 3)), ((0x12345600, 0, 32), (0, 9)),
        # the largest legal shift, bits - 1: the sign bit alone
        ((1 << 31, 0, 8), (0, 7)), ((1 << 31, 0, 16), (0, 15)), ((1 << 31, 0, 24), (0, 23)), ((1 << 31, 0, 32), (0, 31)),
        # silence somewhere: called off, the shift is still the file's
        ((1 << 16, 1, 16), (1, 0)), ((0xFFF80000, 1000, 16), (1, 3)), ((1 << 31, 2, 32), (1, 31)), ((1 << 31, 1, 24), (1, 23)),
        # a bit below the unit: wider than declared -- called off, shift 0, with or without silence
        ((0x0000FFFF, 0, 16), (1, 0)), ((0x00018000, 0, 16), (1, 0)), ((0xFFFF0080, 0, 24), (1, 0)), ((1 << 23, 0, 8), (1, 0)),
        ((0x80000001, 7, 24), (1, 0)), ((0x00008000, 3, 16), (1, 0)),
    ]
    for args, want in table:
        assert M.prepass_done(*args) == want, (args, want)
    # bits = 32: no sample can be wider than declared; the lowest set bit is the shift
    for ntz in range(32):
        assert M.prepass_done((0xFFFFFFFF << ntz) & 0xFFFFFFFF, 0, 32) == (0, ntz)
        assert M.prepass_done(1 << ntz, 9, 32) == (1, ntz)
    # every (bits, lowest set bit): wide below the unit, the distance to the unit at and above it
    for bits in range(1, 33):
        for ntz in range(32):
            want = (1, 0) if ntz < 32 - bits else (0, ntz - (32 - bits))
            assert M.prepass_done((1 << ntz) | (1 << 31), 0, bits) == want, (bits, ntz)


@pytest.mark.parametrize("bits", [8, 16, 24])
def test_prepass_done_gives_the_oracles_header_byte(oracle, bits):
    """one channel, one block of 4096 samples, every sample an odd multiple of 2^(32 - bits + L): the oracle's encoder writes
    offset_lshift into byte 24 of the file header (tests/slastream.py: file_header), the model says the same for the OR word
    of the samples.  A shift the oracle's encoder refuses is noted and left out; the others still count."""
    rng = np.random.default_rng(bits)
    p = S.make_params(1, bits, 48000, 16, 1, 8, 0, 1, 4096)
    refused, seen = [], []
    for L in range(bits):
        half = 1 << (bits - L - 1)                              # odd k in [-half, half)
        k = rng.integers(-half, half, 4096, dtype=np.int64) | 1 if half > 1 else np.full(4096, -1, np.int64)
        pcm = (k << (32 - bits + L)).astype(np.int32).reshape(1, 4096)
        assert (pcm.astype(np.int64) == k << (32 - bits + L)).all()
        ret, data = oracle.encode_whole(p, pcm)
        if ret != 0:
            refused.append((L, ret))
            continue
        orw, _, zero, _ = M.prepass(pcm, bits, 0)
        assert zero == 0
        assert M.prepass_done(orw, zero, bits) == (0, data[24]), (bits, L)
        assert data[23] == bits and data[24] == L, (bits, L, data[23], data[24])
        seen.append(L)
    print("bits %d: offset_lshift seen %s, refused by the oracle's encoder (shift, result) %s" % (bits, seen, refused))
    assert 0 in seen and 1 in seen and 3 in seen                # what the GPU tests rely on
