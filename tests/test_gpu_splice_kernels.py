"""GPU tests of the two delivery kernels of sla_hip_splice_resident through their plain launchers (run with -m gpu on an
MI355X): sla_hip_launch_splice_edges on hand-made planes -- every byte of every block against tests/slastream.py's
block_bytes, blocks packed back to back at every destination alignment between canaries -- and sla_hip_launch_splice_copy on
every pair of source and destination alignments, with entries that share words and 16-byte chunks.

Blocks of 65 535 samples would take slastream's bit-by-bit writer minutes, so `pack_raw` below packs RAW blocks with numpy
and takes the CRC from the library's host routine; every small block of the same tests holds it against block_bytes."""
import ctypes as C

import numpy as np
import pytest

import slastream as SS

pytestmark = pytest.mark.gpu

CANARY = 0xA5
INVALID_ARGUMENT = 2


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    L = sla_amd.lib()
    L.slai_crc16.argtypes = [C.c_void_p, C.c_size_t]
    L.slai_crc16.restype = C.c_uint32
    return sla_amd


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(entries):
    arr = (type(entries[0]) * len(entries))(*entries)
    return dev(np.frombuffer(bytes(arr), np.uint8))


def fmt_of(C_, width, ms):
    return SS.Format(C_, width, ms=ms)


def pack_raw(hip, fmt, planes):
    """block bytes of a RAW block of planes [C][n] (int64, unfolded), numpy-packed"""
    n = planes.shape[1]
    cols = []
    for ch, w in enumerate(SS.raw_widths(fmt)):
        u = SS.fold_array(planes[ch]).astype(np.uint64)
        sh = np.arange(w - 1, -1, -1, dtype=np.uint64)
        cols.append(((u[:, None] >> np.minimum(sh, np.uint64(63))) & np.uint64(1)).astype(np.uint8) * (sh < 32))
    body = np.packbits(np.concatenate(cols, axis=1).reshape(-1))
    out = bytearray(b"\xff\xff" + (len(body) + 5).to_bytes(4, "big") + b"\0\0" + n.to_bytes(2, "big") + b"\x80") + body.tobytes()
    a = np.frombuffer(bytes(out[8:]), np.uint8)
    out[6:8] = int(hip.lib().slai_crc16(a.ctypes.data, len(a))).to_bytes(2, "big")
    return bytes(out)


def expected_block(hip, fmt, planes, silent):
    n = planes.shape[1]
    if silent:
        return SS.block_bytes(fmt, SS.Block(SS.SILENT, n))
    fast = pack_raw(hip, fmt, planes)
    if n <= 1000:
        slow = SS.block_bytes(fmt, SS.Block(SS.RAW, n, raw=[SS.fold_array(planes[ch]) for ch in range(fmt.num_channels)]))
        assert fast == slow
    return fast


def full_range(rng, fmt, n):
    """[C][n] int64 plane values over the whole range of each channel's field, its two ends among them"""
    out = []
    for w in SS.raw_widths(fmt):
        b = min(w, 32)
        v = rng.integers(-(1 << (b - 1)), 1 << (b - 1), n, dtype=np.int64)
        v[:2] = [-(1 << (b - 1)), (1 << (b - 1)) - 1][:len(v[:2])]
        out.append(v)
    return np.stack(out)


def run_edges(hip, fmt, lens, silent_every, start, seed):
    """blocks of `lens` samples from one set of planes, written back to back from byte `start` of a canary buffer"""
    import torch
    rng = np.random.default_rng(seed)
    stride = sum(lens) + 5
    planes = full_range(rng, fmt, stride)
    want = bytearray([CANARY]) * start
    entries, pos = [], 3
    for k, n in enumerate(lens):
        silent = silent_every and k % silent_every == 1
        entries.append((len(want), pos, n, silent))
        want += expected_block(hip, fmt, planes[:, pos:pos + n], silent)
        pos += n
    want += bytearray([CANARY]) * 40
    buf = torch.full((len(want),), CANARY, dtype=torch.uint8, device="cuda")
    d_planes = dev(planes.astype(np.int32))
    t = table([hip.SpliceEdge(buf.data_ptr() + off, p, n, int(s)) for off, p, n, s in entries])
    rc = hip.lib().sla_hip_launch_splice_edges(d_planes.data_ptr(), stride, t.data_ptr(), len(entries), fmt.num_channels,
                                               fmt.bits, fmt.ms, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy().tobytes()
    if got != bytes(want):
        bad = next(i for i in range(len(want)) if got[i] != want[i])
        blk = max(k for k, e in enumerate(entries) if e[0] <= bad) if bad >= start else -1
        raise AssertionError("byte %d differs (block %d of %s, W %d, start %d)" % (bad, blk, entries[blk] if blk >= 0 else None,
                                                                                    sum(SS.raw_widths(fmt)), start))


SMALL = [1, 7, 8, 9, 63, 64, 65]


@pytest.mark.parametrize("width", range(1, 33))
def test_edges_every_width_mono(hip, width):
    """W = 1 .. 32: every small length, SILENT rows between, packed back to back"""
    run_edges(hip, fmt_of(1, width, 0), SMALL + SMALL[::-1], 3, width % 16, 100 + width)


@pytest.mark.parametrize("shape", [(2, 16, 1), (2, 32, 1), (2, 32, 0), (2, 8, 0), (8, 24, 0), (8, 32, 0), (3, 20, 0), (2, 1, 1)],
                         ids=lambda s: "C%d_w%d_ms%d" % s)
def test_edges_channel_sets(hip, shape):
    """W = 33 (16-bit mid/side), 65 with the 33-bit side field, 64, 16, 192, 256, 60, 3"""
    fmt = fmt_of(*shape)
    run_edges(hip, fmt, SMALL + [1000] + SMALL[::-1], 4, 5, 200 + sum(shape))


@pytest.mark.parametrize("start", range(16))
def test_edges_every_destination_alignment(hip, start):
    for k, shape in enumerate([(2, 16, 1), (1, 8, 0), (2, 24, 0)]):
        run_edges(hip, fmt_of(*shape), [9, 1, 64, 7, 65, 8], 3, start, 300 + start + k)


@pytest.mark.parametrize("shape", [(1, 1, 0), (1, 16, 0), (2, 16, 1), (2, 32, 1), (8, 32, 0)], ids=lambda s: "C%d_w%d_ms%d" % s)
def test_edges_longest_block(hip, shape):
    """65 535 samples: up to 2 MB of block through the LDS tiles, its CRC joined from theirs; a neighbour on either side"""
    run_edges(hip, fmt_of(*shape), [7, 65535, 9], 0, 11, 400 + sum(shape))


def test_edges_refusals_and_skipped_entries(hip):
    import torch
    L = hip.lib()
    planes = dev(np.zeros((2, 64), np.int32))
    buf = torch.full((256,), CANARY, dtype=torch.uint8, device="cuda")
    t = table([hip.SpliceEdge(buf.data_ptr() + 8, 0, 0, 0), hip.SpliceEdge(buf.data_ptr() + 8, 60, 5, 0), hip.SpliceEdge(0, 0, 4, 0),
               hip.SpliceEdge(buf.data_ptr() + 8, 65, 1, 1), hip.SpliceEdge(buf.data_ptr() + 8, 0, 65536, 0)])
    for args in ((None, 64, t.data_ptr(), 5, 2, 16, 0), (planes.data_ptr(), 64, None, 5, 2, 16, 0), (planes.data_ptr(), 64, t.data_ptr(), 5, 0, 16, 0),
                 (planes.data_ptr(), 64, t.data_ptr(), 5, 9, 16, 0), (planes.data_ptr(), 64, t.data_ptr(), 5, 2, 0, 0),
                 (planes.data_ptr(), 64, t.data_ptr(), 5, 2, 33, 0), (planes.data_ptr(), 64, t.data_ptr(), 5, 1, 16, 1)):
        assert L.sla_hip_launch_splice_edges(*args, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_splice_edges(planes.data_ptr(), 64, t.data_ptr(), 5, 2, 16, 0, None) == 0      # every entry is skipped
    assert L.sla_hip_launch_splice_edges(planes.data_ptr(), 64, t.data_ptr(), 0, 2, 16, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())


COPY_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 4096 + 5]


def run_copy(hip, entries, src_np, dst_size):
    """entries: (src offset, dst offset, bytes) -> the destination buffer after one launch, and what it must hold"""
    import torch
    src = dev(src_np)
    dst = torch.full((dst_size,), CANARY, dtype=torch.uint8, device="cuda")
    t = table([hip.SpliceCopy(src.data_ptr() + s, dst.data_ptr() + d, n, 0) for s, d, n in entries])
    assert hip.lib().sla_hip_launch_splice_copy(t.data_ptr(), len(entries), max(n for _, _, n in entries), None) == 0
    torch.cuda.synchronize()
    want = np.full(dst_size, CANARY, np.uint8)
    for s, d, n in entries:
        want[d:d + n] = src_np[s:s + n]
    return dst.cpu().numpy(), want


def test_copy_every_pair_of_alignments(hip):
    rng = np.random.default_rng(1)
    src_np = rng.integers(0, 256, 16 * 4200 + 64, dtype=np.uint8)
    slot = 4096 + 5 + 16 + 27                       # canaries between the destinations
    entries = []
    for n in COPY_LENGTHS:
        for sa in range(16):
            for da in range(16):
                entries.append((sa * 4200 + sa, len(entries) * slot // 16 * 16 + da + 16, n))
    got, want = run_copy(hip, entries, src_np, (len(entries) + 1) * slot + 64)
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])


def test_copy_adjacent_entries_share_words(hip):
    rng = np.random.default_rng(2)
    src_np = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    for start in range(16):
        entries, pos = [], start
        for k in range(120):
            n = COPY_LENGTHS[int(rng.integers(0, len(COPY_LENGTHS) - 1))] if k % 40 else 4096 + 5
            entries.append((int(rng.integers(0, len(src_np) - 5000)), pos, n))
            pos += n
        got, want = run_copy(hip, entries, src_np, pos + 33)
        assert np.array_equal(got, want), (start, int(np.flatnonzero(got != want)[0]))


def test_copy_refusals(hip):
    import torch
    L = hip.lib()
    assert L.sla_hip_launch_splice_copy(None, 1, 16, None) == INVALID_ARGUMENT
    buf = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda")
    t = table([hip.SpliceCopy(0, buf.data_ptr(), 16, 0), hip.SpliceCopy(buf.data_ptr(), 0, 16, 0)])
    assert L.sla_hip_launch_splice_copy(t.data_ptr(), 2, 16, None) == 0                  # NULL pointers: skipped
    assert L.sla_hip_launch_splice_copy(t.data_ptr(), 0, 16, None) == 0
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
