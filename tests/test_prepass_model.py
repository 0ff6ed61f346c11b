"""The numpy model of the prepass and of the batch scan (tests/prepassmodel.py) on hand-made inputs, and the one value
it takes from the oracle: what the encoder calls silent at 32 bits with mid/side, where L + R and L - R wrap."""
import numpy as np

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
