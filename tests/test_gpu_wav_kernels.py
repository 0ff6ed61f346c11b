"""GPU tests of the two WAV kernels' launchers (sla_hip_launch_wav_ingest_batch, sla_hip_launch_wav_emit_batch; run with
-m gpu on an MI355X) against the model of tests/wavmodel.py.

Ingest: every bytes-per-sample x channel count, files of lengths around the 4-frame run, the 64-lane wave and the 1024-frame
workgroup row, their first bytes at every offset 0 .. 15 of a 16-byte word, several files per launch, plane regions at
4-word-aligned and at odd positions; the extremes of each width among the operands.  The planes are pre-filled with a
sentinel and compared whole: the converted words, the zero gap [n, fill_end) and every word outside.  One more launch per
width crosses every source offset 0 .. 15 with every count of frames in a lane's last run (files of 1 .. 9 frames).
Emit: the same grid, mid/side on and off, the left shifts of every depth, with and without the 44-byte header, the files of
a launch packed back to back from every start offset 0 .. 15 in a sentinel-filled buffer that is compared whole."""
import ctypes as C

import numpy as np
import pytest

import wavmodel as W

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 2
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 1023, 1025, 4099]
SENTINEL = 0x5A5AA5A5
BYTE_SENTINEL = 0xC3
EXTREMES = {1: (b"\x00", b"\xff"), 2: (b"\x00\x80", b"\xff\x7f"), 3: (b"\x00\x00\x80", b"\xff\xff\x7f"),
            4: (b"\x00\x00\x00\x80", b"\xff\xff\xff\x7f")}


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def to_device(table):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()


def frames_of(n, nch, B, seed):
    """n frames of random bytes with the extremes of the width as the first and the last samples"""
    rng = np.random.default_rng(seed)
    raw = bytearray(rng.integers(0, 256, size=n * nch * B, dtype=np.uint8).tobytes())
    lo, hi = EXTREMES[B]
    ns = n * nch
    for k, v in ((0, lo), (1, hi), (ns - 2, hi), (ns - 1, lo)):
        if 0 <= k < ns:
            raw[k * B:(k + 1) * B] = v
    return bytes(raw)


@pytest.mark.parametrize("nch", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_ingest_against_the_model(hip, B, nch):
    import torch
    L = hip.lib()
    for variant in (0, 1):                                   # plane regions 4-word aligned / at odd positions
        src = np.full(sum(n * nch * B + 32 for n in LENGTHS) + 64, BYTE_SENTINEL, np.uint8)
        table = (hip.WavIngest * len(LENGTHS))()
        regions, pos, plane_pos, max_lim = [], 0, 0, 0
        for i, n in enumerate(LENGTHS):
            raw = frames_of(n, nch, B, 100 * B + 10 * nch + i)
            off = (i + 11 * variant) % 16
            pos = (pos + 15) // 16 * 16 + off
            src[pos:pos + len(raw)] = np.frombuffer(raw, np.uint8)
            fill_end = [0, n, n + 1, n + 5, (n + 63) // 64 * 64, n + 130][i % 6]
            plane_pos = (plane_pos + 3) // 4 * 4 + ([0, 0, 0][i % 3] if variant == 0 else [1, 3, 2][i % 3])
            regions.append((plane_pos, n, max(n, fill_end), raw, pos))
            table[i].plane_off, table[i].num_samples, table[i].fill_end = plane_pos, n, fill_end
            pos += len(raw)
            plane_pos += max(n, fill_end) + 2                # (two sentinel words between the regions)
            max_lim = max(max_lim, n, fill_end)
        stride = (plane_pos + 8 + 3) // 4 * 4 + (0 if variant == 0 else 1)
        d_src = torch.from_numpy(src).cuda()
        for i, (_, _, _, _, p) in enumerate(regions):
            table[i].src = d_src.data_ptr() + p
        d_table = to_device(table)
        planes = torch.from_numpy(np.full(nch * stride + 4, SENTINEL, np.uint32).view(np.int32)).cuda()
        base = planes if variant == 0 else planes[1:]        # (variant 1: the plane base is not 16-byte aligned either)
        want = np.full(nch * stride + 4, SENTINEL, np.uint32).view(np.int32).copy()
        wbase = want if variant == 0 else want[1:]
        for po, n, lim, raw, _ in regions:
            conv = W.planes_from_frames(raw, nch, 8 * B)
            for c in range(nch):
                wbase[c * stride + po:c * stride + po + n] = conv[c]
                wbase[c * stride + po + n:c * stride + po + lim] = 0
        rc = L.sla_hip_launch_wav_ingest_batch(d_table.data_ptr(), len(LENGTHS), max_lim, nch, B, base.data_ptr(), stride, None)
        assert rc == 0
        torch.cuda.synchronize()
        got = planes.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (variant, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_ingest_every_offset_with_every_tail(hip, B, nch):
    """k_wav_ingest realigns by the source's byte offset and cuts 1 .. 4 frames out of a lane's last run: every offset 0 .. 15
    with every n = 1 .. 9 in one launch, the last file ending at the last byte of the source tensor"""
    import torch
    L = hip.lib()
    cases = [(off, n) for off in range(16) for n in range(1, 10)]
    assert len(cases) == 144
    for variant in (0, 1):                                   # plane regions 4-word aligned / at odd positions
        chunks, pos = [], 0
        for i, (off, n) in enumerate(cases):
            raw = frames_of(n, nch, B, 5000 + 100 * B + 10 * nch + i)
            pos = (pos + 15) // 16 * 16 + off
            chunks.append((pos, raw))
            pos += len(raw)
        src = np.full(pos, BYTE_SENTINEL, np.uint8)          # (ends with the last file)
        for p, raw in chunks:
            src[p:p + len(raw)] = np.frombuffer(raw, np.uint8)
        d_src = torch.from_numpy(src).cuda()
        assert d_src.data_ptr() % 16 == 0 and chunks[-1][0] + len(chunks[-1][1]) == d_src.numel()
        table = (hip.WavIngest * len(cases))()
        regions, plane_pos, max_lim = [], 0, 0
        for i, ((off, n), (p, raw)) in enumerate(zip(cases, chunks)):
            fill_end = [0, n, n + 1, n + 5, n + 3][i % 5]
            plane_pos = (plane_pos + 3) // 4 * 4 + (0 if variant == 0 else [1, 3, 2][i % 3])
            regions.append((plane_pos, n, max(n, fill_end), raw))
            table[i].src, table[i].plane_off, table[i].num_samples, table[i].fill_end = d_src.data_ptr() + p, plane_pos, n, fill_end
            plane_pos += max(n, fill_end) + 2                # (two sentinel words between the regions)
            max_lim = max(max_lim, n, fill_end)
        assert {(int(table[i].src) % 16, n) for i, (_, n) in enumerate(cases)} == set(cases)
        stride = (plane_pos + 8 + 3) // 4 * 4 + (0 if variant == 0 else 1)
        d_table = to_device(table)
        planes = torch.from_numpy(np.full(nch * stride + 4, SENTINEL, np.uint32).view(np.int32)).cuda()
        base = planes if variant == 0 else planes[1:]
        want = np.full(nch * stride + 4, SENTINEL, np.uint32).view(np.int32).copy()
        wbase = want if variant == 0 else want[1:]
        for po, n, lim, raw in regions:
            conv = W.planes_from_frames(raw, nch, 8 * B)
            for c in range(nch):
                wbase[c * stride + po:c * stride + po + n] = conv[c]
                wbase[c * stride + po + n:c * stride + po + lim] = 0
        rc = L.sla_hip_launch_wav_ingest_batch(d_table.data_ptr(), len(cases), max_lim, nch, B, base.data_ptr(), stride, None)
        assert rc == 0
        torch.cuda.synchronize()
        got = planes.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        owner = [i for i, r in enumerate(regions) if bad.size and r[0] <= (bad[0] - variant) % stride]
        assert len(bad) == 0, (variant, "file (offset, n)", cases[owner[-1]] if owner else None, bad[:8], got[bad[:8]], want[bad[:8]])
        assert np.array_equal(d_src.cpu().numpy(), src)


def finish(planes, ms, shift):
    """what k_dec_emit_batch makes of a file's planes: mid/side undone, left shift; in 32-bit wrapping arithmetic"""
    u = planes.astype(np.int64) & 0xFFFFFFFF
    if ms:
        mid = ((u[0] << 1) | (u[1] & 1)) & 0xFFFFFFFF
        l = ((mid + u[1]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32) >> 1
        r = ((mid - u[1]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32) >> 1
        u = np.stack([l, r]).astype(np.int64) & 0xFFFFFFFF
    return ((u << shift) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("nch", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_emit_against_the_model(hip, B, nch):
    import torch
    L = hip.lib()
    shifts = [0, 8, 16] + ([24] if B == 1 else [])
    case = 0
    for ms in ((0, 1) if nch == 2 else (0,)):
        for hb in (0, 44):
            rng = np.random.default_rng(1000 * B + 100 * nch + 10 * ms + hb)
            stride = sum((n + 3) // 4 * 4 + 4 for n in LENGTHS) + 1
            planes = rng.integers(-2 ** 31, 2 ** 31, size=(nch, stride), dtype=np.int64).astype(np.int32)
            planes[:, :8] = np.array([-2 ** 31, 2 ** 31 - 1, -1, 0, 1, -2, 2 ** 30, -2 ** 30], np.int32)    # side words odd and even
            start = (5 * B + 3 * nch + 7 * case) % 16
            case += 1
            total = sum(hb + n * nch * B for n in LENGTHS)
            want = np.full(start + total + 64, BYTE_SENTINEL, np.uint8)
            d_dst = torch.from_numpy(want.copy()).cuda()
            table = (hip.WavEmit * len(LENGTHS))()
            pos, ppos = start, 0
            for i, n in enumerate(LENGTHS):
                shift = shifts[i % len(shifts)]
                header = W.header44(W.Info(nch, 8 * B, 44100 + i, n, 44, n * nch * B))
                ppos += [0, 1, 3, 2][i % 4]                  # plane regions at every word alignment
                table[i].plane_off, table[i].dst, table[i].num_samples = ppos, d_dst.data_ptr() + pos, n
                table[i].mid_side, table[i].shift, table[i].header_bytes = ms, shift, hb
                C.memmove(table[i].header, header, 44)
                body = W.frames_from_planes(finish(planes[:, ppos:ppos + n], ms, shift), 8 * B)
                file = (header if hb else b"") + body
                want[pos:pos + len(file)] = np.frombuffer(file, np.uint8)
                pos += len(file)                             # back to back, no padding
                ppos += n
            assert ppos <= stride and pos == start + total
            d_table = to_device(table)
            d_planes = torch.from_numpy(planes).cuda()
            rc = L.sla_hip_launch_wav_emit_batch(d_planes.data_ptr(), stride, d_table.data_ptr(), len(LENGTHS), max(LENGTHS), nch, B,
                                                 ms, None)
            assert rc == 0
            torch.cuda.synchronize()
            got = d_dst.cpu().numpy()
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (ms, hb, start, bad[:8], got[bad[:8]], want[bad[:8]])


def test_emit_skips_an_entry_with_another_header_size_and_ignores_mid_side_when_the_launch_says_so(hip):
    import torch
    L = hip.lib()
    planes = np.arange(2 * 64, dtype=np.int32).reshape(2, 64) * 1000003
    d_planes = torch.from_numpy(planes).cuda()
    d_dst = torch.from_numpy(np.full(1024, BYTE_SENTINEL, np.uint8)).cuda()
    table = (hip.WavEmit * 2)()
    table[0].plane_off, table[0].dst, table[0].num_samples, table[0].header_bytes = 0, d_dst.data_ptr() + 3, 40, 43
    table[1].plane_off, table[1].dst, table[1].num_samples, table[1].mid_side = 8, d_dst.data_ptr() + 501, 40, 1
    d_table = to_device(table)
    assert L.sla_hip_launch_wav_emit_batch(d_planes.data_ptr(), 64, d_table.data_ptr(), 2, 40, 2, 2, 0, None) == 0
    torch.cuda.synchronize()
    want = np.full(1024, BYTE_SENTINEL, np.uint8)
    body = W.frames_from_planes(planes[:, 8:48], 16)
    want[501:501 + len(body)] = np.frombuffer(body, np.uint8)
    assert np.array_equal(d_dst.cpu().numpy(), want)


def test_launchers_refuse_bad_arguments(hip):
    import torch
    L = hip.lib()
    t = torch.zeros(256, dtype=torch.int32, device="cuda")
    p = t.data_ptr()
    for nch, B in ((0, 2), (9, 2), (2, 0), (2, 5)):
        assert L.sla_hip_launch_wav_ingest_batch(p, 1, 1, nch, B, p, 64, None) == INVALID_ARGUMENT
        assert L.sla_hip_launch_wav_emit_batch(p, 64, p, 1, 1, nch, B, 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_wav_ingest_batch(None, 1, 1, 2, 2, p, 64, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_wav_ingest_batch(p, 1, 1, 2, 2, None, 64, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_wav_emit_batch(None, 64, p, 1, 1, 2, 2, 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_wav_emit_batch(p, 64, None, 1, 1, 2, 2, 0, None) == INVALID_ARGUMENT
    for nch in (1, 3, 8):                                    # mid/side is a matter of two channels
        assert L.sla_hip_launch_wav_emit_batch(p, 64, p, 1, 1, nch, 2, 1, None) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert int(t.abs().sum()) == 0                           # nothing was launched
