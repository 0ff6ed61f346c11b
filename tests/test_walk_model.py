"""CPU-only checks that pin tests/walkmodel.py, the device-free restatement of the block-chain walk: on streams the
oracle's encoder wrote its rows are the encoder trace's blocks, on the crafted catalogue its byte offsets are those the
stream writer recorded, and on damaged chains its stop reasons are the ones the host decoder documents."""
import numpy as np
import pytest

import crafted_catalogue as CC
import slalibs as S
import walkmodel as WM
import waveforms as W

SPECS = [
    (S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096), lambda: W.music_like(2, 30000, 16, seed=9)),
    (S.make_params(1, 16, 48000, 16, 1, 8, 0, 1, 4096), lambda: W.gen("sine", 1, 17001, 16, lshift=3, seed=7)),
    (S.make_params(2, 24, 48000, 32, 3, 8, 1, 1, 4096), lambda: W.gen("white", 2, 13003, 24, seed=6)),
    (S.make_params(8, 16, 48000, 8, 1, 4, 0, 1, 2048), lambda: W.gen("white", 8, 9000, 16, seed=3)),
]


@pytest.mark.parametrize("k", range(len(SPECS)))
def test_rows_are_the_oracle_traces_blocks(oracle, k):
    p, make = SPECS[k]
    pcm = make()
    ret, data, tr = oracle.encode_trace(p, pcm)
    assert ret == 0
    nb = int(tr.num_blocks)
    total = WM.header_total(data)
    assert total == pcm.shape[1]
    w = WM.walk(data, total, total, 16384)
    assert w.stop == WM.OK and w.num_blocks == nb and w.extent == total
    assert [r[2] for r in w.rows] == [int(v) for v in tr.blk_start[:nb]]
    assert [r[3] for r in w.rows] == [int(v) for v in tr.blk_nsmpl[:nb]]
    assert [r[1] for r in w.rows] == [int(v) for v in tr.blk_bytes[:nb]]
    assert [r[0] for r in w.rows] == [43 + int(v) for v in np.concatenate(([0], np.cumsum(tr.blk_bytes[:nb])))[:nb]]
    assert all(r[4] == 0 for r in w.rows)
    # every row's CRC field is the stored one
    for off, _, _, _, _, crc in w.rows:
        assert crc == int.from_bytes(bytes(data[off + 6:off + 8]), "big")


def test_byte_offsets_on_the_crafted_catalogue():
    cases = CC.catalogue()
    assert len(cases) == 52
    for c in cases:
        w = WM.walk(c.data, c.num_samples, c.num_samples, CC.CAP[1])
        assert w.stop == WM.OK, c.name
        assert [r[0] for r in w.rows] == list(c.offsets), c.name
        assert [r[3] for r in w.rows] == [b.n for b in c.blocks], c.name
        assert w.extent == c.num_samples, c.name


def test_stop_reasons_and_header_only_rows(oracle):
    p, make = SPECS[0]
    ret, data, tr = oracle.encode_trace(p, make())
    assert ret == 0
    data = bytearray(data)
    total = WM.header_total(data)
    offs = [43 + int(v) for v in np.concatenate(([0], np.cumsum(tr.blk_bytes[:tr.num_blocks])))]
    assert WM.walk(data[:offs[4]], total, total, 16384).stop == WM.DATA            # off == data_size
    assert WM.walk(data[:offs[4] + 10], total, total, 16384).stop == WM.DATA       # fewer than 11 bytes left
    assert WM.walk(data[:offs[2] + 100], total, total, 16384).stop == WM.DATA      # a size field past the end
    assert WM.walk(data[:offs[2] + 100], total, total, 16384).num_blocks == 2
    bad = bytearray(data); bad[offs[2]] = 0x7F
    w = WM.walk(bad, total, total, 16384)
    assert (w.stop, w.num_blocks) == (WM.SYNC_LOST, 2)
    wrap = bytearray(data); wrap[offs[1] + 2:offs[1] + 6] = b"\xff\xff\xff\xff"     # size field + 6 wraps to 5 < 8
    w = WM.walk(wrap, total, total, 16384)
    assert (w.stop, w.num_blocks) == (WM.DATA, 1)
    cap = int(tr.blk_start[3]) + 10                                                # block 3 does not fit
    w = WM.walk(data, total, cap, 16384, crc_check=1)
    assert (w.stop, w.num_blocks, w.rows[-1][4], w.extent) == (WM.BUF, 4, WM.HEADER_ONLY, int(tr.blk_start[3]))
    w = WM.walk(data, total, cap, 16384, crc_check=0)
    assert (w.stop, w.num_blocks, w.extent) == (WM.BUF, 3, int(tr.blk_start[3]))
    w = WM.walk(data, total, total, 2048, crc_check=1)                             # larger than the handle's blocks
    assert (w.stop, w.num_blocks, w.rows[0][4], w.extent) == (WM.BUF, 1, WM.HEADER_ONLY, 0)
    assert WM.walk(data, total, total, 2048, crc_check=0).num_blocks == 0
