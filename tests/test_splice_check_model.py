"""CPU-only checks of the check kernel's model (tests/splicemodel.py: check_code, check_verdicts), the yardstick of
tests/test_gpu_splice_check.py: every block of the splice sources is clean under its true row and the model agrees with
tests/indexmodel.py's judge_row on the chain-header and CRC rules; the fit rule at both ends of every field width, and
against the RAW writer of tests/slastream.py and the oracle's decoder; the 40-bit verdict word."""
import numpy as np

import crafted_catalogue as CC
import indexmodel as IM
import slalibs as S
import slastream as SS
import splicemodel as SM

CORRUPT, NG = 11, 1
HEADER_BYTES = (0, 1, 2, 3, 4, 5, 8, 9)


def blocks_with_rows():
    """(case, row, type) of every block of every source"""
    for files in SM.sources().values():
        for case in files:
            rows = IM.index_of(case.data).rows
            assert len(rows) == len(case.blocks)
            for row, blk in zip(rows, case.blocks):
                yield case, row, blk.type


def verbatim(off, blen, n):
    return SM.CheckEntry(off, blen, n)


def code(entry, memory, crc_check):
    return SM.check_code(entry, memory, [], 0, 1, 16, 0, [], crc_check)


def test_every_source_block_is_clean_under_its_true_row():
    count = 0
    for case, (off, blen, _, n), _ in blocks_with_rows():
        for crc in (0, 1):
            assert code(verbatim(off, blen, n), case.data, crc) == 0, (case.name, off, crc)
        count += 1
    assert count == len(SM.FORMATS) * sum(len(k) for k in SM.KINDS)


def test_header_and_crc_rules_agree_with_the_judge():
    """judge_row with a clean info reaches its rules 1 and 2 only: the model gives the same code for every single-byte
    change of the chain header, every bit of the CRC field and every change of the row"""
    for case, (off, blen, pos, n), typ in blocks_with_rows():
        image = bytearray(case.data)
        info = (typ, blen, int.from_bytes(case.data[off + 6:off + 8], "big"), 0)
        assert info[2] == SS.crc16(case.data[off + 8:off + blen])

        def both(row, crc):
            want = IM.judge_row(image, row, info, crc, True)
            got = code(verbatim(row[0], row[1], row[3]), image, crc)
            assert got == want, (case.name, row, crc, got, want)
            return got

        for at in HEADER_BYTES:
            old = image[off + at]
            for v in range(256):
                if v != old:
                    image[off + at] = v
                    assert both((off, blen, pos, n), 0) == both((off, blen, pos, n), 1) == CORRUPT, (case.name, at, v)
            image[off + at] = old
        for at in (6, 7):
            for bit in range(8):
                image[off + at] ^= 1 << bit
                assert both((off, blen, pos, n), 0) == 0 and both((off, blen, pos, n), 1) == CORRUPT
                image[off + at] ^= 1 << bit
        assert bytes(image) == case.data
        for row in ((off, blen + 1, pos, n), (off, blen - 1, pos, n), (off, blen, pos, n + 1), (off, blen, pos, n - 1),
                    (off, blen, pos, n + 65536), (off, 10, pos, n), (off, 0, pos, n)):
            for crc in (0, 1):
                assert both(row, crc) == CORRUPT, (case.name, row)


def raw_header(n, blen=12, typ=2):
    return b"\xff\xff" + (blen - 6).to_bytes(4, "big") + b"\0\0" + n.to_bytes(2, "big") + bytes([typ << 6]) + bytes(blen - 11)


def test_the_fit_rule_at_both_ends_of_every_field():
    """w = 1 .. 33: a field of w bits holds -(2^(w-1)) .. 2^(w-1) - 1 and nothing beyond; fields of 32 bits and more are
    not looked at (every int32 fits them)"""
    memory = raw_header(4)
    for w in range(1, 34):
        lo, hi = -(1 << (w - 1)), (1 << (w - 1)) - 1
        assert [SM.fits(s, w) for s in (lo - 1, lo, hi, hi + 1)] == [False, True, True, False], w
        # through check_code: one edge entry of four kept samples, each of the four values alone among zeros
        C, width, ms, ch = (1, w, 0, 0) if w <= 32 else (2, 32, 1, 1)
        for s, fit in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
            for at in range(4):
                planes = [[0] * 6 for _ in range(C)]
                planes[ch][1 + at] = s
                e = SM.CheckEntry(0, 12, 4, edge=0, plane_off=1, keep=4)
                want = 0 if (fit or w >= 32) else CORRUPT
                assert SM.check_code(e, memory, planes, 6, C, width, ms, [0], 1) == want, (w, s, at)
    # the side channel takes one bit more than channel 0; other channels do not
    for width in (1, 8, 16, 31):
        hi = 1 << (width - 1)
        for ch, ms, want in ((0, 1, CORRUPT), (1, 1, 0), (1, 0, CORRUPT), (0, 0, CORRUPT)):
            planes = [[0] * 3, [0] * 3]
            planes[ch][1] = hi
            e = SM.CheckEntry(0, 12, 4, edge=0, plane_off=1, keep=1)
            assert SM.check_code(e, memory, planes, 3, 2, width, ms, [0], 0) == want, (width, ch, ms)
    # samples outside the kept range, a SILENT block's planes and the judge's code
    planes = [[1 << 20, 0, 0, 1 << 20]]
    assert SM.check_code(SM.CheckEntry(0, 12, 4, edge=0, plane_off=1, keep=2), memory, planes, 4, 1, 16, 0, [0], 0) == 0
    assert SM.check_code(SM.CheckEntry(0, 12, 4, edge=0, plane_off=1, keep=3), memory, planes, 4, 1, 16, 0, [0], 0) == CORRUPT
    assert SM.check_code(SM.CheckEntry(0, 12, 4, edge=0, plane_off=1, keep=4), memory, planes, 4, 1, 16, 0, [0], 0) == NG
    assert SM.check_code(SM.CheckEntry(0, 12, 4, edge=1, plane_off=1, keep=2), memory, planes, 4, 1, 16, 0, [0], 0) == NG
    assert SM.check_code(SM.CheckEntry(0, 12, 4, edge=0, plane_off=0, keep=4), memory, planes, 4, 1, 16, 0, [8], 0) == 8
    assert SM.check_code(SM.CheckEntry(0, 11, 4, edge=0, plane_off=0, keep=4), raw_header(4, 11, 1), planes, 4, 1, 16, 0, [0], 0) == 0


def test_the_fitting_extremes_pass_the_raw_writer_and_the_oracles_decoder():
    """what the rule lets through is what a RAW field stores: both ends of every channel's field, written by
    slastream.block_bytes and read by the oracle's decoder, come back unchanged"""
    formats = {k: SM.FORMATS[k] for k in ("mono16", "stereo8", "stereo16ms", "eight24", "stereo24l3", "mono32l3")}
    formats["mono32"] = SS.Format(1, 32, order=4, ntaps=1, lms=4, max_block=2048)      # (mid/side at 32 bits wraps in the decoder)
    for name, fmt in formats.items():
        widths = SS.raw_widths(fmt)
        cols = []
        for k, w in enumerate(widths):                                # every channel at either end while the others rest
            lo, hi = -(1 << (min(w, 32) - 1)), (1 << (min(w, 32) - 1)) - 1
            assert SM.fits(lo, w) and SM.fits(hi, w) and (w >= 32 or not (SM.fits(lo - 1, w) or SM.fits(hi + 1, w)))
            for v in (lo, hi):
                col = [0] * len(widths)
                col[k] = v
                cols.append(col)
        v = np.array(cols, np.int64).T
        n = v.shape[1]
        data = SS.write_file(fmt, [SS.Block(SS.RAW, n, raw=[SS.fold_array(v[ch]) for ch in range(fmt.num_channels)])])[0]
        rc, got, _ = S.oracle().decode_whole(S.make_params(cap=CC.CAP), data, n)
        assert rc == 0 and got.shape == v.shape, name
        if fmt.ms:
            mid = (v[0] << 1) | (v[1] & 1)
            v = np.stack([(mid + v[1]) >> 1, (mid - v[1]) >> 1])
        want = ((v << (32 - fmt.bits + fmt.lshift)) & SS.M32).astype(np.uint32).view(np.int32)
        assert np.array_equal(got, want), name
        if not fmt.ms:                                                # and back: the decoder's samples are the planes'
            assert np.array_equal(got.astype(np.int64) >> (32 - fmt.bits + fmt.lshift), np.array(cols, np.int64).T), name


def test_verdict_words_are_40_bits_wide():
    memory = raw_header(4)
    bad = SM.CheckEntry(0, 13, 4)                                     # a row one byte too long: CORRUPT
    entries = [SM.CheckEntry(0, 13, 4, verdict=0, ordinal=(1 << 24) + 5), SM.CheckEntry(0, 13, 4, verdict=1, ordinal=(1 << 32) - 1),
               SM.CheckEntry(0, 13, 4, verdict=2, ordinal=(1 << 31) + 1), SM.CheckEntry(0, 13, 4, verdict=2, ordinal=(1 << 24)),
               SM.CheckEntry(0, 12, 4, verdict=3, ordinal=0),         # clean
               SM.CheckEntry(0, 13, 4, verdict=4, ordinal=0), SM.CheckEntry(0, 13, 4, verdict=5, ordinal=0),
               SM.CheckEntry(0, 13, 4, verdict=6, ordinal=9), SM.CheckEntry(0, 13, 4, verdict=SM.NO_EDGE, ordinal=9)]
    assert code(bad, memory, 0) == CORRUPT
    words = SM.check_verdicts(entries, [SM.ALL_ONES] * 4 + [5, SM.ALL_ONES, SM.ALL_ONES], 6, memory, [], 0, 1, 16, 0, [], 0)
    assert words == [(((1 << 24) + 5) << 8) | 11, (0xFFFFFFFF << 8) | 11, ((1 << 24) << 8) | 11, SM.ALL_ONES, 5, 11, SM.ALL_ONES]
    assert words[1] == 0xFFFFFFFF0B and words[1].bit_length() == 40
