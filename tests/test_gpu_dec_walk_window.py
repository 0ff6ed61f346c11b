"""GPU tests of sla_hip_launch_dec_walk_window (k_dec_walk_window; run with -m gpu on an MI355X): the block-chain walk for
a window of samples against tests/windowmodel.py, in count mode and in write mode, on the chains and damage cases of
tests/test_gpu_dec_walk.py.  Every case's bytes lie at a source misalignment of their own and all windows of all cases
go through one launch per max_block_samples; the write-mode tables are sentinel-filled with spare rows behind every
file's rows, which must stay as they were.  Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_dec_walk as TW
import test_window_model as TM
import walkmodel as WM
import windowmodel as WN

pytestmark = pytest.mark.gpu

BLOCK_DT = TW.BLOCK_DT
FILE_DT = np.dtype([("src", "<u8"), ("img_off", "<u8"), ("data_size", "<u4"), ("total", "<u4"), ("win_start", "<u4"),
                    ("win_len", "<u4"), ("seek_byte", "<u4"), ("seek_sample", "<u4"), ("range_bytes", "<u4"), ("base_byte", "<u4"),
                    ("base_sample", "<u4"), ("plane_off", "<u4"), ("first", "<u4"), ("max_rows", "<u4")])
RESULT_DT = np.dtype([("num_blocks", "<u4"), ("stop", "<u4"), ("skipped", "<u4"), ("first_byte", "<u4"), ("first_sample", "<u4"),
                      ("end_byte", "<u4"), ("end_sample", "<u4"), ("reserved", "<u4")])
SPARE = 3                        # sentinel rows behind every file's rows
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _windows():
    """(case name, index of its bytes, total, start, length, max_block_samples, seek_byte, seek_sample) and the bytes"""
    datas, wins = [], []
    cases = TW._cases()
    clean = TM.chain_only(cases[0][1], cases[0][2])             # the undamaged chain: its block starts are hints behind damage
    for name, data, total, _, cap_n in cases:
        k = len(datas)
        datas.append(data)
        full = TM.chain_only(data, total)
        hint_rows = full.rows + ([r for r in clean.rows if r not in full.rows] if len(data) == len(cases[0][1]) else [])
        for start, length in TM.grid(TM.bounds_of(full, total), total):
            wins.append((name, k, total, start, length, cap_n, 0, 0))
        wins.append((name, k, total, 400, M32, cap_n, 0, 0))                    # start + length above 2^32
        wins.append((name, k, total, M32, M32, cap_n, 0, 0))
        wins.append((name, k, total, 0, M32, cap_n, 0, 0))
        # hints: every block of the chain at or before the window, and hints that are wrong
        for start, length in ((0, 10), (299, 2), (450, 100), (999, 2), (1001, 40), (1100, 500)):
            for r in hint_rows:
                if r[2] <= start:
                    wins.append((name, k, total, start, length, cap_n, r[0], r[2]))
            for seek in (43, 44, 50, len(data) - 11, len(data) - 10, len(data), len(data) + 1, M32):
                if seek >= 43:
                    wins.append((name, k, total, start, length, cap_n, seek, min(start, 100)))
    return datas, wins


def _result(res):
    return tuple(int(res[f]) for f in ("num_blocks", "stop", "skipped", "first_byte", "first_sample", "end_byte", "end_sample", "reserved"))


def _model_result(m):
    return (m.num_blocks, m.stop, m.skipped, m.first_byte, m.first_sample, m.end_byte, m.end_sample, 0)


def _launch(L, torch, ft, cap_n, tables=None):
    d_ft = torch.from_numpy(ft.view(np.uint8).copy()).cuda()
    d_res = torch.full((len(ft) * RESULT_DT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    ptrs = [C.c_void_p(t.data_ptr()) for t in tables] if tables else [None, None, None]
    torch.cuda.synchronize()
    assert L.sla_hip_launch_dec_walk_window(C.c_void_p(d_ft.data_ptr()), len(ft), cap_n, C.c_void_p(d_res.data_ptr()), *ptrs, None) == 0
    torch.cuda.synchronize()
    return d_res.cpu().numpy().view(RESULT_DT)


def test_windows_of_every_case_against_the_model(hip):
    import torch
    L = hip.lib()
    datas, wins = _windows()
    buf, offs = TW._place(torch, datas, [(k * 5 + 1) % 16 for k in range(len(datas))])
    assert len({o % 16 for o in offs}) == 16
    models = [WN.walk(datas[k], total, start, length, cap_n, sb, ss) for _, k, total, start, length, cap_n, sb, ss in wins]
    for cap_n in sorted({w[5] for w in wins}):
        idx = [j for j, w in enumerate(wins) if w[5] == cap_n]
        ft = np.zeros(len(idx), FILE_DT)
        for j, i in enumerate(idx):
            _, k, total, start, length, _, sb, ss = wins[i]
            ft[j]["src"], ft[j]["data_size"], ft[j]["total"] = buf.data_ptr() + offs[k], len(datas[k]), total
            ft[j]["win_start"], ft[j]["win_len"], ft[j]["seek_byte"], ft[j]["seek_sample"] = start, length, sb, ss
        # count mode: only the results are written
        res = _launch(L, torch, ft, cap_n)
        for j, i in enumerate(idx):
            assert _result(res[j]) == _model_result(models[i]), ("count", wins[i])
        # write mode: every file's rows behind SPARE sentinel rows, image and plane offsets of a pass
        first, rows = [], 1
        for j, i in enumerate(idx):
            m = models[i]
            first.append(rows)
            rows += m.num_blocks + SPARE
            ft[j]["img_off"], ft[j]["plane_off"] = 4096 + 8 * j, 64 * j
            ft[j]["range_bytes"], ft[j]["base_byte"], ft[j]["base_sample"] = m.end_byte - m.first_byte, m.first_byte, m.first_sample
            ft[j]["first"], ft[j]["max_rows"] = first[j], m.num_blocks
        d_blk = torch.full((rows * BLOCK_DT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        d_end = torch.full((rows * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        d_crc = torch.full((rows * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        res = _launch(L, torch, ft, cap_n, (d_blk, d_end, d_crc))
        blk = d_blk.cpu().numpy().view(BLOCK_DT)
        end = d_end.cpu().numpy().view("<u8")
        crcf = d_crc.cpu().numpy().view("<u4")
        want_blk = np.frombuffer(bytes([0xA5]) * (rows * BLOCK_DT.itemsize), BLOCK_DT).copy()
        want_end = np.full(rows, 0xA5A5A5A5A5A5A5A5, "<u8")
        want_crc = np.full(rows, 0xA5A5A5A5, "<u4")
        for j, i in enumerate(idx):
            m = models[i]
            assert _result(res[j]) == _model_result(m), ("write", wins[i])
            trows, tend, tcrc = WN.table_rows(m, img_off=4096 + 8 * j, plane_off=64 * j)
            for b, row in enumerate(trows):
                want_blk[first[j] + b] = row
                want_end[first[j] + b] = tend
                want_crc[first[j] + b] = tcrc[b]
        bad = np.nonzero(blk != want_blk)[0]
        assert bad.size == 0, ("rows", cap_n, bad[:8], blk[bad[:4]], want_blk[bad[:4]])
        assert np.array_equal(end, want_end) and np.array_equal(crcf, want_crc), cap_n
    # the sources are only read
    host = buf.cpu().numpy()
    for data, o in zip(datas, offs):
        assert bytes(host[o:o + len(data)]) == data
    # the cases did what this test is for
    by = {}
    for w, m in zip(wins, models):
        by.setdefault(w[0], []).append((w, m))
    plain = lambda name: {m.stop for w, m in by[name] if w[6] == 0}
    assert plain("no sync at a later block") == {WM.OK, WM.SYNC_LOST}
    assert plain("size field 0xFFFFFFFF wraps") == {WM.OK, WM.DATA}
    assert plain("block larger than the handle's blocks") == {WM.OK, WM.BUF}
    big =[(w, m) for w, m in by["block larger than the handle's blocks"] if w[6] == 0]
    assert any(m.stop == WM.OK and m.num_blocks == 1 and m.first_sample == 1000 and m.skipped == 4 for _, m in big)   # passed over
    assert any(m.stop == WM.BUF and w[3] >= 500 for w, m in big)                                                      # inside: stops
    assert any(w[4] == M32 and m.num_blocks == 3 for w, m in by["clean, total reached at the last block"])
    hinted = [(w, m) for w, m in by["no sync at a later block"] if w[6] > 43 and w[3] >= 1000]
    assert any(m.stop == WM.OK and m.num_blocks == 1 for _, m in hinted)                  # a hint behind the damage


def test_rows_never_reach_behind_max_rows(hip):
    """write mode with max_rows below the kept blocks: only max_rows rows are written; above it, the spare rows become
    empty header-only rows at the range's start"""
    import torch
    L = hip.lib()
    data, _ = TW._chain([10, 20, 30, 40], seed=5)
    buf, so = TW._place(torch, [data], [3])
    m = WN.walk(data, 100, 15, 60, 4096)
    assert m.num_blocks == 3 and m.skipped == 1
    for max_rows in (2, 6):
        ft = np.zeros(1, FILE_DT)
        ft[0] = (buf.data_ptr() + so[0], 1000, len(data), 100, 15, 60, 0, 0, m.end_byte - m.first_byte, m.first_byte, m.first_sample,
                 64, 2, max_rows)
        d_blk = torch.full((10 * BLOCK_DT.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        d_end = torch.full((10 * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        d_crc = torch.full((10 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        res = _launch(L, torch, ft, 4096, (d_blk, d_end, d_crc))
        assert _result(res[0]) == _model_result(m)
        blk = d_blk.cpu().numpy().view(BLOCK_DT)
        crcf = d_crc.cpu().numpy().view("<u4")
        end = d_end.cpu().numpy().view("<u8")
        touched = [r for r in range(10) if int(crcf[r]) != 0xA5A5A5A5]
        assert touched == list(range(2, 2 + max_rows)), (max_rows, touched)
        trows, tend, _ = WN.table_rows(m, img_off=1000, plane_off=64)
        for b in range(min(max_rows, 3)):
            assert tuple(blk[2 + b]) == trows[b] and int(end[2 + b]) == tend
        for b in range(3, max_rows):
            assert tuple(blk[2 + b]) == (1000, 8, 64, 0, WM.HEADER_ONLY) and int(end[2 + b]) == tend
