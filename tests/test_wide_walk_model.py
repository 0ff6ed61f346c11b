"""CPU-only checks that pin tests/widewalkmodel.py -- the wide walk restated in numpy: node test, successor table,
doubling rounds, cut -- to tests/walkmodel.py::walk, the specification of both device walks: on the crafted catalogue,
on the damaged chains of tests/test_gpu_dec_walk.py (rebuilt here) and on every chain tests/test_gpu_dec_walk_wide.py
gives the kernels."""
import numpy as np
import pytest

import crafted_catalogue as CC
import slastream as SS
import walkmodel as WM
import widewalkcases as WC
import widewalkmodel as WW

FMT = SS.Format(1, 16, order=4, ntaps=1, lms=4)


def _same(data, total, cap, cap_n, crc, name, node_capacity=1 << 20):
    want = WM.walk(data, total, cap, cap_n, crc)
    got = WW.wide_walk(data, total, cap, cap_n, crc, node_capacity)
    assert got.overflow == 0, name
    assert (got.rows, got.stop, got.extent) == (want.rows, want.stop, want.extent), (name, crc)
    return got


def test_nodes_are_the_positions_the_lane_walk_would_keep_a_block_at():
    """the definition, byte by byte, on a stream dense with sync codes and on its last 11 bytes"""
    data = WC.decoy_cases()[3][1][:4000] + b"\xff\xff\x00\x00\x00\x05" + bytes(5)
    size = len(data)
    want = []
    for p in range(43, size):
        if p + 11 > size or data[p] != 0xFF or data[p + 1] != 0xFF:
            continue
        b = (int.from_bytes(data[p + 2:p + 6], "big") + 6) & 0xFFFFFFFF
        if 8 <= b <= size - p:
            want.append(p)
    assert len(want) > 500 and want[-1] == size - 11
    assert list(WW.nodes(data)) == want
    assert len(WW.nodes(data[:53])) == 0 and len(WW.nodes(b"")) == 0


def test_crafted_catalogue():
    for c in CC.catalogue():
        for crc in (1, 0):
            got = _same(c.data, c.num_samples, c.num_samples, CC.CAP[1], crc, c.name)
            assert [r[0] for r in got.rows] == list(c.offsets), c.name
            _same(c.data, c.num_samples, c.num_samples // 2, CC.CAP[1], crc, c.name)


def _lane_cases():
    """the chains of tests/test_gpu_dec_walk.py::_cases, rebuilt"""
    def chain(lengths, seed, total=None):
        rng = np.random.default_rng(seed)
        blocks = [SS.Block(SS.SILENT, n) if (k % 2 or n == 0) else CC._comp(rng, FMT, n, bits=6, full=False) for k, n in enumerate(lengths)]
        data, _, offs = SS.write_file(FMT, blocks, num_samples=total)
        return data, offs
    put = WC.put
    lens = [300, 200, 0, 500, 123]
    n = sum(lens)
    data, offs = chain(lens, 1)
    short, _ = chain(lens, 3, total=n + 50)
    size3 = int.from_bytes(data[offs[4] + 2:offs[4] + 6], "big")
    return [
        ("clean", data, n, n, 4096), ("room to spare", data, n, n + 1000, 4096),
        ("zero-sample blocks at both ends", chain([0, 0, 77, 0], 2)[0], 77, 77, 4096),
        ("ends before total", short, n + 50, n + 50, 4096),
        ("fewer than 11 bytes left", short + b"\xff\xff\x00\x00\x00", n + 50, n + 50, 4096),
        ("ten bytes left", short + b"\xff\xff" + bytes(8), n + 50, n + 50, 4096),
        ("header only", data[:43], n, n, 4096), ("shorter than its header", data[:20], n, n, 4096),
        ("no sync at the first block", put(data, offs[0], 0xFFFE, 2), n, n, 4096),
        ("no sync at a later block", put(data, offs[3], 0x7FFF, 2), n, n, 4096),
        ("size field runs past the end", put(data, offs[4] + 2, size3 + 1, 4), n, n, 4096),
        ("size field ends at the end", data + b"\x00", n, n, 4096),
        ("size field 0xFFFFFFFF wraps", put(data, offs[1] + 2, 0xFFFFFFFF, 4), n, n, 4096),
        ("size field 0xFFFFFFFA wraps to 0", put(data, offs[1] + 2, 0xFFFFFFFA, 4), n, n, 4096),
        ("size field below the CRC start", put(data, offs[3] + 2, 1, 4), n, n, 4096),
        ("size field just at the CRC start", put(data, offs[3] + 2, 2, 4), n, n, 4096),
        ("block larger than capacity - pos", data, n, 300 + 200 + 499, 4096),
        ("first block larger than the capacity", data, n, 299, 4096), ("capacity zero", data, n, 0, 4096),
        ("block larger than the handle's blocks", data, n, n, 499),
        ("first block larger than the handle's blocks", data, n, n, 200),
        ("no samples in the header", data, 0, n, 4096),
    ]


@pytest.mark.parametrize("crc", [1, 0])
def test_lane_walk_cases(crc):
    for name, data, total, cap, cap_n in _lane_cases():
        _same(data, total, cap, cap_n, crc, name)


@pytest.mark.parametrize("crc", [1, 0])
def test_gpu_cases(crc):
    cases = WC.all_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) >= len(names) - len(WC.tile_cases(0))             # (the tile cases come once per source alignment)
    by = {}
    for name, data, total, cap, cap_n in cases:
        by[name] = _same(data, total, cap, cap_n, crc, name)
    # the cases do what their names say
    for L in WC.ROUND_LENGTHS:
        assert by["chain of %d" % L].num_blocks == L
    long = by["70000 eleven-byte blocks"]
    assert long.num_blocks == 70000 and long.rounds > 16 and long.stop == WM.OK
    assert by["decoys that chain among themselves"].num_nodes == 79 and by["decoys that chain among themselves"].num_blocks == 40
    assert by["decoys that merge into the chain"].num_nodes == 80 and by["decoys that merge into the chain"].num_blocks == 40
    assert by["a decoy chain longer than the real one"].num_nodes == 183
    assert by["dense field, period 6"].num_nodes > 4500 and by["dense field, period 8"].num_nodes > 4500
    assert by["lost sync at the second block"].stop == WM.SYNC_LOST and by["lost sync at the second block"].num_blocks == 1
    assert by["lost sync at the last block"].stop == WM.SYNC_LOST and by["lost sync at the last block"].num_blocks == 5
    assert by["size beyond the bytes left"].stop == WM.DATA and by["size ends at the end"].stop == WM.OK
    assert by["ten bytes left"].stop == WM.DATA and by["five bytes left"].stop == WM.DATA
    assert by["total reached mid-chain"].num_blocks == 2 and by["total reached mid-chain"].stop == WM.OK
    assert by["total reached in front of zero-sample blocks"].num_blocks == 2
    assert by["total larger than the chain"].stop == WM.DATA and by["total larger than the chain"].num_blocks == 6
    for name, kept in (("capacity stop", 5), ("capacity stop at the first block", 1), ("block stop", 5), ("block stop at the first block", 1)):
        m = by[name]
        assert m.stop == WM.BUF and m.num_blocks == (kept if crc == 1 else kept - 1), name
    for v in range(0xFFFFFFFA, 0x100000000):
        m = by["size field %08X wraps" % v]
        assert (m.stop, m.num_blocks) == (WM.DATA, 1)
    assert by["zero-sample blocks in a row"].num_blocks == 4 and by["zero-sample blocks only"].stop == WM.DATA


def test_overflow_and_rounds():
    name, data, total, cap, cap_n = WC.decoy_cases()[0]
    n = len(WW.nodes(data))
    assert n == 79
    assert _same(data, total, cap, cap_n, 1, name, node_capacity=n).num_nodes == n
    over = WW.wide_walk(data, total, cap, cap_n, 1, node_capacity=n - 1)
    assert (over.overflow, over.rows, over.stop, over.extent, over.num_nodes) == (WW.OVERFLOW, [], WM.OK, 0, n)
    assert [WW.rounds(s, 1 << 20) for s in (0, 53, 54, 61, 62, 69, 70, 54 + 8 * 1023, 54 + 8 * 1024)] == [0, 0, 0, 0, 1, 1, 2, 10, 11]
    assert WW.rounds(1 << 30, 1000) == 10 and WW.rounds(1 << 30, 1) == 0
    assert WW.scratch_bytes(54, 1) % 16 == 0 and WW.scratch_bytes(0xFFFFFFFF, 0xFFFFFFFF) % 16 == 0
