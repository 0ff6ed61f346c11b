"""GPU tests of sla_hip_launch_dec_walk (k_dec_walk; run with -m gpu on an MI355X): the block-chain walk on the device
against tests/walkmodel.py, in count mode and in write mode, on chains written with tests/slastream.py and damaged by
hand.  Every case is walked at a source misalignment of its own, in one launch with the others; the write-mode tables
are sentinel-filled with spare rows behind every file's rows, which must stay as they were.  Nothing here reads
/root/reference."""
import ctypes as C

import numpy as np
import pytest

import crafted_catalogue as CC
import slastream as SS
import walkmodel as WM

pytestmark = pytest.mark.gpu

BLOCK_DT = np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"), ("num_samples", "<u4"), ("flags", "<u4")])
FILE_DT = np.dtype([("src", "<u8"), ("img_off", "<u8"), ("data_size", "<u4"), ("total", "<u4"), ("capacity", "<u4"),
                    ("first", "<u4"), ("max_rows", "<u4"), ("plane_off", "<u4")])
RESULT_DT = np.dtype([("num_blocks", "<u4"), ("stop", "<u4"), ("extent", "<u4"), ("reserved", "<u4")])
SPARE = 3                        # sentinel rows behind every file's rows
FMT = SS.Format(1, 16, order=4, ntaps=1, lms=4)


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _chain(lengths, seed=0, total=None):
    """(.sla bytes, block offsets) of a chain of blocks of the given lengths: silent and small compressed ones"""
    rng = np.random.default_rng(seed)
    blocks = [SS.Block(SS.SILENT, n) if (k % 2 or n == 0) else CC._comp(rng, FMT, n, bits=6, full=False) for k, n in enumerate(lengths)]
    data, _, offs = SS.write_file(FMT, blocks, num_samples=total)
    return data, offs


def _put(data, at, value, width):
    d = bytearray(data)
    d[at:at + width] = int(value).to_bytes(width, "big")
    return bytes(d)


def _cases():
    """(name, data, total, capacity, max_block_samples)"""
    out = []
    lens = [300, 200, 0, 500, 123]
    n = sum(lens)
    data, offs = _chain(lens, seed=1)
    out.append(("clean, total reached at the last block", data, n, n, 4096))
    out.append(("clean, room to spare", data, n, n + 1000, 4096))
    out.append(("zero-sample blocks at both ends", _chain([0, 0, 77, 0], seed=2)[0], 77, 77, 4096))
    short, soffs = _chain(lens, seed=3, total=n + 50)
    out.append(("the stream ends before total (off == data_size)", short, n + 50, n + 50, 4096))
    out.append(("fewer than 11 bytes left", short + b"\xff\xff\x00\x00\x00", n + 50, n + 50, 4096))
    out.append(("ten bytes left", short + b"\xff\xff" + bytes(8), n + 50, n + 50, 4096))
    out.append(("header only", data[:43], n, n, 4096))
    out.append(("shorter than its header", data[:20], n, n, 4096))
    out.append(("no sync at the first block", _put(data, offs[0], 0xFFFE, 2), n, n, 4096))
    out.append(("no sync at a later block", _put(data, offs[3], 0x7FFF, 2), n, n, 4096))
    size3 = int.from_bytes(data[offs[4] + 2:offs[4] + 6], "big")
    out.append(("size field runs past the end", _put(data, offs[4] + 2, size3 + 1, 4), n, n, 4096))
    out.append(("size field ends at the end", data + b"\x00", n, n, 4096))
    out.append(("size field 0xFFFFFFFF wraps", _put(data, offs[1] + 2, 0xFFFFFFFF, 4), n, n, 4096))
    out.append(("size field 0xFFFFFFFA wraps to 0", _put(data, offs[1] + 2, 0xFFFFFFFA, 4), n, n, 4096))
    out.append(("size field below the CRC start", _put(data, offs[3] + 2, 1, 4), n, n, 4096))
    out.append(("size field just at the CRC start", _put(data, offs[3] + 2, 2, 4), n, n, 4096))
    out.append(("block larger than capacity - pos", data, n, 300 + 200 + 499, 4096))
    out.append(("first block larger than the capacity", data, n, 299, 4096))
    out.append(("capacity zero", data, n, 0, 4096))
    out.append(("block larger than the handle's blocks", data, n, n, 499))
    out.append(("first block larger than the handle's blocks", data, n, n, 200))
    out.append(("no samples in the header", data, 0, n, 4096))
    return out


def _place(torch, datas, misaligns):
    """every file in one device buffer, file k at a 16-byte boundary plus misaligns[k]; -> (tensor, offsets)"""
    offs, pos = [], 64
    for d, m in zip(datas, misaligns):
        pos = (pos + 15) // 16 * 16 + m
        offs.append(pos)
        pos += len(d) + 16
    host = np.full(pos + 64, 0xEE, np.uint8)
    for d, o in zip(datas, offs):
        host[o:o + len(d)] = np.frombuffer(d, np.uint8)
    return torch.from_numpy(host).cuda(), offs


def _walk_all(hip, cases, crc, misaligns, img_offs=None, plane_offs=None):
    """count mode, then write mode with every file's rows behind SPARE sentinel rows; everything against the model"""
    import torch
    L = hip.lib()
    nf = len(cases)
    img_offs = img_offs or [0] * nf
    plane_offs = plane_offs or [0] * nf
    buf, offs = _place(torch, [c[1] for c in cases], misaligns)
    models = [WM.walk(data, total, cap, cap_n, crc) for _, data, total, cap, cap_n in cases]
    # a launch has one max_block_samples: group the cases by it
    for cap_n in sorted({c[4] for c in cases}):
        idx = [k for k, c in enumerate(cases) if c[4] == cap_n]
        ft = np.zeros(len(idx), FILE_DT)
        for j, k in enumerate(idx):
            ft[j] = (buf.data_ptr() + offs[k], 0, len(cases[k][1]), cases[k][2], cases[k][3], 0, 0, 0)
        d_ft = torch.from_numpy(ft.view(np.uint8).copy()).cuda()
        d_res = torch.full((len(idx) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.sla_hip_launch_dec_walk(C.c_void_p(d_ft.data_ptr()), len(idx), cap_n, crc, C.c_void_p(d_res.data_ptr()),
                                         None, None, None, None) == 0
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(RESULT_DT)
        for j, k in enumerate(idx):
            m = models[k]
            assert (int(res[j]["num_blocks"]), int(res[j]["stop"]), int(res[j]["extent"])) == (m.num_blocks, m.stop, m.extent), \
                ("count", cases[k][0], crc)
        # write mode
        first, rows = [], 1
        for j, k in enumerate(idx):
            first.append(rows)
            rows += models[k].num_blocks + SPARE
        for j, k in enumerate(idx):
            ft[j]["img_off"], ft[j]["plane_off"] = img_offs[k], plane_offs[k]
            ft[j]["first"], ft[j]["max_rows"] = first[j], models[k].num_blocks
        d_ft = torch.from_numpy(ft.view(np.uint8).copy()).cuda()
        d_blk = torch.full((rows * BLOCK_DT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        d_end = torch.full((rows * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        d_crc = torch.full((rows * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        d_res.fill_(0xA5)
        torch.cuda.synchronize()
        assert L.sla_hip_launch_dec_walk(C.c_void_p(d_ft.data_ptr()), len(idx), cap_n, crc, C.c_void_p(d_res.data_ptr()),
                                         C.c_void_p(d_blk.data_ptr()), C.c_void_p(d_end.data_ptr()), C.c_void_p(d_crc.data_ptr()),
                                         None) == 0
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(RESULT_DT)
        blk = d_blk.cpu().numpy().view(BLOCK_DT)
        end = d_end.cpu().numpy().view("<u8")
        crcf = d_crc.cpu().numpy().view("<u4")
        want_blk = np.frombuffer(bytes([0xA5]) * (rows * BLOCK_DT.itemsize), BLOCK_DT).copy()
        want_end = np.full(rows, 0xA5A5A5A5A5A5A5A5, "<u8")
        want_crc = np.full(rows, 0xA5A5A5A5, "<u4")
        for j, k in enumerate(idx):
            m = models[k]
            assert (int(res[j]["num_blocks"]), int(res[j]["stop"]), int(res[j]["extent"])) == (m.num_blocks, m.stop, m.extent), \
                ("write", cases[k][0], crc)
            for b, (off, blen, pos, n, flags, crcv) in enumerate(m.rows):
                want_blk[first[j] + b] = (img_offs[k] + off, blen, plane_offs[k] + pos, n, flags)
                want_end[first[j] + b] = img_offs[k] + len(cases[k][1])
                want_crc[first[j] + b] = crcv
        bad = np.nonzero(blk != want_blk)[0]
        assert bad.size == 0, ("rows", crc, cap_n, bad[:8], blk[bad[:4]], want_blk[bad[:4]])
        assert np.array_equal(end, want_end) and np.array_equal(crcf, want_crc), (crc, cap_n)
    # the sources are only read
    host = buf.cpu().numpy()
    for (name, data, *_), o in zip(cases, offs):
        assert bytes(host[o:o + len(data)]) == data, name
    return models


@pytest.mark.parametrize("crc", [1, 0])
def test_walk_cases_against_the_model(hip, crc):
    cases = _cases()
    models = _walk_all(hip, cases, crc, [(k * 5 + 1) % 16 for k in range(len(cases))])
    by = {c[0]: m for c, m in zip(cases, models)}
    # the cases do what their names say (the model is pinned by tests/test_walk_model.py)
    assert by["clean, total reached at the last block"].stop == WM.OK and by["clean, total reached at the last block"].num_blocks == 5
    assert by["the stream ends before total (off == data_size)"].stop == WM.DATA
    assert by["fewer than 11 bytes left"].stop == WM.DATA and by["ten bytes left"].stop == WM.DATA
    assert by["no sync at the first block"].num_blocks == 0 and by["no sync at a later block"].num_blocks == 3
    assert by["no sync at a later block"].stop == WM.SYNC_LOST
    assert by["size field runs past the end"].stop == WM.DATA and by["size field ends at the end"].stop == WM.OK
    assert by["size field 0xFFFFFFFF wraps"].stop == WM.DATA and by["size field 0xFFFFFFFF wraps"].num_blocks == 1
    assert by["size field below the CRC start"].stop == WM.DATA and by["size field below the CRC start"].num_blocks == 3
    assert by["size field just at the CRC start"].num_blocks >= 4
    for name, kept in (("block larger than capacity - pos", 4), ("first block larger than the capacity", 1),
                       ("block larger than the handle's blocks", 4), ("first block larger than the handle's blocks", 1)):
        m = by[name]
        assert m.stop == WM.BUF and m.num_blocks == (kept if crc == 1 else kept - 1), name
        assert (m.rows[-1][4] == WM.HEADER_ONLY) if crc == 1 else all(r[4] == 0 for r in m.rows), name
    assert by["no samples in the header"].num_blocks == 0


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_source_misalignments(hip, mis):
    cases = [c for c in _cases() if c[4] == 4096][:12]
    _walk_all(hip, cases, 1, [mis + 4 * (k % 4) for k in range(len(cases))])


def test_130_two_block_files_in_one_launch(hip):
    """more than a wave and more than a workgroup, with image and plane offsets of a pass and spare rows between files"""
    cases, img_offs, plane_offs = [], [], []
    img, span = 4096, 640
    for k in range(130):
        a, b = 50 + 7 * (k % 11), 1 + (k * 13) % 97
        data, _ = _chain([a, b], seed=100 + k)
        if k % 10 == 3:
            data = data[:-2]                                  # some end inside their second block
        cases.append(("file %d" % k, data, a + b, a + b if k % 7 else a + b - 1, 4096))
        img_offs.append(img); plane_offs.append(span)
        img += (len(data) + 3) // 4 * 4
        span += (a + b + 63) // 64 * 64
    models = _walk_all(hip, cases, 1, [k % 16 for k in range(130)], img_offs, plane_offs)
    assert {m.num_blocks for m in models} == {1, 2}
    assert {m.stop for m in models} == {WM.OK, WM.DATA, WM.BUF}


def test_rows_never_reach_behind_max_rows(hip):
    """write mode with max_rows below the chain's length: only max_rows rows are written; above it, the spare rows
    become empty header-only rows at the file's start"""
    import torch
    L = hip.lib()
    data, offs = _chain([10, 20, 30, 40], seed=5)
    buf, so = _place(torch, [data], [3])
    for max_rows, want_rows in ((2, 2), (6, 6)):
        ft = np.zeros(1, FILE_DT)
        ft[0] = (buf.data_ptr() + so[0], 1000, len(data), 100, 100, 2, max_rows, 64)
        d_ft = torch.from_numpy(ft.view(np.uint8).copy()).cuda()
        d_res = torch.zeros(16, dtype=torch.uint8, device="cuda")
        d_blk = torch.full((10 * BLOCK_DT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        d_end = torch.full((10 * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        d_crc = torch.full((10 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.sla_hip_launch_dec_walk(C.c_void_p(d_ft.data_ptr()), 1, 4096, 1, C.c_void_p(d_res.data_ptr()),
                                         C.c_void_p(d_blk.data_ptr()), C.c_void_p(d_end.data_ptr()), C.c_void_p(d_crc.data_ptr()),
                                         None) == 0
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(RESULT_DT)
        assert int(res[0]["num_blocks"]) == 4 and int(res[0]["stop"]) == WM.OK
        blk = d_blk.cpu().numpy().view(BLOCK_DT)
        crcf = d_crc.cpu().numpy().view("<u4")
        touched = [r for r in range(10) if int(crcf[r]) != 0xA5A5A5A5]
        assert touched == list(range(2, 2 + want_rows)), (max_rows, touched)
        m = WM.walk(data, 100, 100, 4096)
        for b in range(min(max_rows, 4)):
            assert tuple(blk[2 + b]) == (1000 + m.rows[b][0], m.rows[b][1], 64 + m.rows[b][2], m.rows[b][3], 0)
        for b in range(4, max_rows):
            assert tuple(blk[2 + b]) == (1000, 8, 64, 0, WM.HEADER_ONLY)
