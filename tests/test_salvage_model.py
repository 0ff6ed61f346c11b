"""tests/salvagemodel.py, the device-free statement of the salvage rule (sla_hip_salvage_resident), pinned without a GPU:
on undamaged streams its rows are tests/walkmodel.py's and nothing is lost; on every damage kind of tests/salvagecases.py
the mode is the listed one and the lost ranges are the sample ranges of the blocks the case damaged, worked out by the
catalogue from the clean stream; the accepted limits (a second break, appended bytes, the embedded block) come out as
include/sla_hip.h states them."""
import numpy as np
import pytest

import salvagecases as SC
import salvagemodel as SM
import slastream as W
import walkmodel as WM


@pytest.fixture(scope="module", params=list(SC.SHAPES))
def stream(request, oracle):
    return SC.oracle_stream(oracle, request.param)


def check_case(case):
    name, data, mode, lost, patches, undec = case
    m = SM.salvage(data, SC.CAP_N, undec)
    total = WM.header_total(data)
    assert m.mode == mode, name
    assert m.lost == lost, (name, m.lost, lost)
    assert m.samples_lost == sum(n for _, n, _ in lost)
    # rows: in sample order, inside [0, N), disjoint from each other and -- but for concealed rows -- from the lost ranges
    covered = np.zeros(total, np.int32)
    for off, blen, smp, n, flags, crcf in m.rows:
        assert 0 <= smp and smp + n <= total, name
        covered[smp:smp + n] += 1
    for start, length, reason in m.lost:
        if reason == SM.GAP:
            covered[start:start + length] += 1
    assert np.all(covered == 1), name                     # every sample is decoded, concealed or lost, exactly once
    assert [r[2] for r in m.rows] == sorted(r[2] for r in m.rows), name
    return m


def test_crc_is_the_formats():
    data = bytes(range(256)) * 3
    assert SM.crc16(data) == W.crc16(data) and SM.crc16(b"") == 0


def test_undamaged_streams_are_the_walks(stream):
    data, pcm = stream
    total = WM.header_total(data)
    m = SM.salvage(data, SC.CAP_N)
    w = WM.walk(data, total, total, SC.CAP_N, 1)
    assert m.mode == 1 and m.rows == w.rows and m.lost == [] and m.concealed == 0 and m.decoded == len(w.rows)


def test_catalogue(stream):
    data, pcm = stream
    blocks = SC.blocks_of(data)
    for case in SC.catalogue(data):
        m = check_case(case)
        if case[2] == 2:
            assert m.prefix_blocks + m.suffix_blocks == len(m.rows)
            assert m.sound_nodes <= m.nodes
            # prefix and suffix are blocks of the clean stream at their own sample positions (the embedded block aside)
            clean = {(smp, n) for _, _, smp, n in blocks}
            assert all((r[2], r[3]) in clean for r in m.rows), case[0]


def test_hand_written_streams():
    for cases, pcm in SC.raw_cases():
        for case in cases:
            check_case(case)


def test_decoy_is_a_node_and_not_sound():
    (cases, pcm), = [c for c in SC.raw_cases() if c[0][0][0].startswith("a decoy")]
    data = cases[0][1]
    pos, bsize, n, crcf, ok = SM.sound_nodes(data, 1, SC.CAP_N)
    blocks = SC.blocks_of(data)
    decoys = [i for i in range(len(pos)) if int(pos[i]) not in {b[0] for b in blocks}]
    assert decoys and not any(ok[i] for i in decoys)
    assert any(bsize[i] == 38 and n[i] == 16 and crcf[i] == 0x1234 for i in decoys)
    m = SM.salvage(cases[1][1], SC.CAP_N)
    assert m.nodes == len(pos) - 1 and m.sound_nodes == len(blocks) - 1       # the block whose sync code went is no node


def test_embedded_block_is_picked_and_right_aligned():
    (cases, pcm), = [c for c in SC.raw_cases() if c[0][0][0].startswith("an embedded")]
    name, data, mode, lost, patches, undec = cases[1]
    blocks = SC.blocks_of(cases[0][1])
    m = SM.salvage(data, SC.CAP_N)
    total = WM.header_total(data)
    inner = blocks[5][0] + blocks[5][1] - blocks[2][1]                      # where the copy of block 2 starts
    assert m.suffix_byte == inner and m.prefix_blocks == 5 and m.suffix_blocks == 4
    assert m.suffix_samples == blocks[2][3] + sum(b[3] for b in blocks[6:]) and m.suffix_sample == total - m.suffix_samples
    want = SC.expected_pcm(pcm, lost, patches)
    s5, n5, n2 = blocks[5][2], blocks[5][3], blocks[2][3]
    assert np.all(want[:, s5:s5 + n5 - n2] == 0) and np.array_equal(want[:, s5 + n5 - n2:s5 + n5], pcm[:, blocks[2][2]:blocks[2][2] + n2])


def test_limits():
    data, pcm, _ = SC.raw_stream()
    b = SC.blocks_of(data)
    total = WM.header_total(data)
    # sample count too large for the handle: not sound
    m = SM.salvage(data, 2500)
    assert m.mode == 2 and m.prefix_blocks == 1 and m.lost == [(b[1][2], total - b[1][2] - m.suffix_samples, SM.GAP)]
    # the length cap: 64 + 16 C max(n, 1)
    assert SM.max_block_bytes(2, 0) == 96 and SM.max_block_bytes(3, 4096) == 64 + 16 * 3 * 4096
    # a chain that is intact but does not account for N samples is not trusted: header says more than the blocks hold
    d = bytearray(data)
    d[15:19] = (total + 5).to_bytes(4, "big")
    d[8:10] = W.crc16(d[10:43]).to_bytes(2, "big")
    m = SM.salvage(bytes(d), SC.CAP_N)
    assert m.mode == 2 and m.prefix_blocks == len(b) and m.suffix_blocks == 0 and m.lost == [(total, 5, SM.GAP)]
