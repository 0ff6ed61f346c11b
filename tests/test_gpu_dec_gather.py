"""GPU tests of sla_hip_launch_dec_gather (k_dec_gather; run with -m gpu on an MI355X): files at any byte address into
an image at 4-byte-aligned offsets.  For every size of the list and every source misalignment 0..15 the destination
bytes are the source's, the pad up to the 4-byte boundary is zero and the rest of a sentinel-filled image is as it was;
the destination offsets take every residue of 16 that a multiple of 4 has, so that heads, bodies and tails of the
16-byte chunks are all met.  Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GATHER_DT = np.dtype([("src", "<u8"), ("dst_off", "<u8"), ("bytes", "<u4"), ("reserved", "<u4")])
SIZES = [0, 1, 3, 4, 5, 15, 16, 17, 43, 63, 64, 65, 4099]


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _run(hip, entries, image_bytes, src_host, declared=None, max_bytes=None):
    """entries: (source offset, bytes, dst_off); -> the image after the launch over a 0xA5-filled image"""
    import torch
    L = hip.lib()
    src = torch.from_numpy(src_host).cuda()
    t = np.zeros(len(entries), GATHER_DT)
    for k, (so, n, do) in enumerate(entries):
        t[k] = (src.data_ptr() + so, do, n, 0)
    d_t = torch.from_numpy(t.view(np.uint8).copy()).cuda()
    img = torch.full((image_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_dec_gather(C.c_void_p(d_t.data_ptr()), len(entries),
                                     max((n for _, n, _ in entries), default=0) if max_bytes is None else max_bytes,
                                     C.c_void_p(img.data_ptr()), image_bytes if declared is None else declared, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), src_host)                # sources are only read
    return img.cpu().numpy()


def _expect(entries, image_bytes, src_host):
    want = np.full(image_bytes + 64, 0xA5, np.uint8)
    for so, n, do in entries:
        want[do:do + n] = src_host[so:so + n]
        want[do + n:do + (n + 3) // 4 * 4] = 0
    return want


@pytest.mark.parametrize("mis", range(16))
def test_every_size_at_this_source_misalignment(hip, mis):
    """all sizes in one table, the sources slices of one buffer at misalignment `mis`, gaps of sentinel between the
    destinations and destination offsets at every residue 0 / 4 / 8 / 12 of 16"""
    rng = np.random.default_rng(mis)
    entries, so, do = [], 256, 0
    for k, n in enumerate(SIZES * 2):
        so = (so + 15) // 16 * 16 + mis
        do = (do + 15) // 16 * 16 + 4 * ((k + mis) % 4) + 16 * (k % 2)
        entries.append((so, n, do))
        so += n
        do += (n + 3) // 4 * 4 + 4
    src_host = rng.integers(1, 256, so + 256, dtype=np.uint8)          # no zero byte: a pad cannot pass for data
    got = _run(hip, entries, do + 32, src_host)
    want = _expect(entries, do + 32, src_host)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (mis, bad[:16])


def test_back_to_back_files_as_in_a_pass_image(hip):
    """files packed as a pass packs them -- each at the 4-byte boundary behind the one before, no gap -- from sources at
    odd offsets of one buffer: the whole image is the padded concatenation"""
    rng = np.random.default_rng(99)
    sizes = [4099, 1, 43, 65, 7, 128, 3, 4097, 16, 2, 1000, 5]
    entries, so, do = [], 1, 0
    for n in sizes:
        entries.append((so, n, do))
        so += n + (n % 5)
        do += (n + 3) // 4 * 4
    src_host = rng.integers(1, 256, so + 64, dtype=np.uint8)
    got = _run(hip, entries, do, src_host)
    assert np.array_equal(got, _expect(entries, do, src_host))


def test_a_long_file_takes_the_grid_stride(hip):
    """max_bytes understated: fewer workgroup rows than chunks, every lane strides"""
    rng = np.random.default_rng(7)
    n = 300001
    src_host = rng.integers(1, 256, n + 64, dtype=np.uint8)
    entries = [(5, n, 8), (3, 100, (8 + n + 3) // 4 * 4 + 4)]
    total = entries[1][2] + 104
    got = _run(hip, entries, total, src_host, max_bytes=4096)
    assert np.array_equal(got, _expect(entries, total, src_host))


def test_entries_outside_the_image_are_skipped(hip):
    rng = np.random.default_rng(8)
    src_host = rng.integers(1, 256, 512, dtype=np.uint8)
    good = (3, 50, 16)
    entries = [good, (1, 40, 100), (1, 40, 80 + 2), (1, 10, 200)]     # past the declared end, misaligned, wholly outside
    got = _run(hip, entries, 256, src_host, declared=128)
    assert np.array_equal(got, _expect([good], 256, src_host))
