"""GPU tests of k_enc_emit alone (sla_hip_launch_enc_emit_batch, include/sla_hip.h; run with -m gpu on an MI355X): crafted
images and tables against numpy.  The kernel copies files from any byte offset of a pack image to any byte address and puts
a header from the table in front; its contract is that exactly [dst, dst + bytes) of every entry is written and nothing
else, because files packed back to back share words and 16-byte chunks that other lanes write in the same launch.  Every
test therefore compares the WHOLE destination buffer, pre-filled with a per-byte pattern, with the numpy expectation.

Covered: every pair of source and destination misalignment (mod 16) for four sizes and a diagonal for the other sizes of
the list, with and without a header; 64 files of 43..106 bytes packed without gaps; a file longer than one sweep of the
grid; more entries than the grid has rows; entries the kernel has to skip; the empty table."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [43, 44, 45, 46, 47, 58, 59, 60, 61, 75, 76, 107, 4096 + 5]
FULL = [43, 61, 107, 4096 + 5]                        # every (source, destination) misalignment pair


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def pattern(n):
    """the canary: a per-byte pattern with period 251, so a byte moved by a power of two never matches"""
    return ((np.arange(n, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8)


def random_image(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def run_emit(hip, image, image_bytes, dest, entries):
    """image, dest: numpy uint8; entries: [(img_off, dst offset in dest, bytes, header_bytes, header (48 bytes) or None)].
    Returns (launcher's code, dest afterwards).  The image tensor has room behind image_bytes, as the driver's has."""
    import torch
    d_image = torch.from_numpy(np.concatenate([image, np.zeros(32, np.uint8)])).cuda()
    d_dest = torch.from_numpy(dest).cuda()
    assert d_image.data_ptr() % 16 == 0 and d_dest.data_ptr() % 16 == 0
    n = len(entries)
    table = (hip.EncEmit * max(n, 1))()
    for k, (off, dst, nbytes, hb, header) in enumerate(entries):
        table[k].img_off, table[k].dst, table[k].bytes, table[k].header_bytes = off, d_dest.data_ptr() + dst, nbytes, hb
        if header is not None:
            C.memmove(table[k].header, np.ascontiguousarray(header, np.uint8).ctypes.data, 48)
    d_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()
    rc = hip.lib().sla_hip_launch_enc_emit_batch(d_table.data_ptr(), n, max([e[2] for e in entries], default=0),
                                                 d_image.data_ptr(), image_bytes,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, d_dest.cpu().numpy()


def expectation(image, dest, entries):
    want = dest.copy()
    for off, dst, nbytes, hb, header in entries:
        want[dst:dst + hb] = header[:hb] if hb else []
        want[dst + hb:dst + nbytes] = image[off + hb:off + nbytes]
    return want


def headers(n, seed):
    """n table headers: 43 random bytes, then five the kernel must ignore"""
    h = np.random.default_rng(seed).integers(0, 256, (n, 48), dtype=np.uint8)
    h[:, 43:] = 0xEE
    return h


@pytest.mark.parametrize("hb", [43, 0], ids=["header", "bare"])
def test_alignment_sweep(hip, hb):
    pairs = []
    for size in SIZES:
        if size in FULL:
            pairs += [(size, sm, dm) for sm in range(16) for dm in range(16)]
        else:
            pairs += [(size, k, (5 * k + 3) % 16) for k in range(16)]
    image = random_image(32768, 1)
    slots = (len(image) - max(SIZES) - 16) // 16
    hd = headers(len(pairs), 2)
    entries, pos = [], 0
    for k, (size, sm, dm) in enumerate(pairs):
        pos += 32                                         # at least 16 canary bytes between neighbours
        entries.append((16 * ((k * 37) % slots) + sm, pos + dm, size, hb, hd[k]))
        pos = (pos + dm + size + 15) // 16 * 16
    dest = pattern(pos + 64)
    rc, got = run_emit(hip, image, len(image), dest, entries)
    want = expectation(image, dest, entries)
    assert rc == 0
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "first differing byte %d of %d" % (bad[0], len(got))
    assert {e[0] % 16 for e in entries} == set(range(16)) == {e[1] % 16 for e in entries}


def test_64_files_packed_without_gaps(hip):
    """the arena case: sizes 43..106 back to back in the image (headers zero, as the packer leaves them) and in the
    destination, which starts at an odd byte"""
    sizes = list(range(43, 107))
    image = random_image(sum(sizes) + 3, 3)
    hd = headers(len(sizes), 4)
    entries, off, dst = [], 3, 5
    for k, size in enumerate(sizes):
        image[off:off + 43] = 0
        entries.append((off, dst, size, 43, hd[k]))
        off += size; dst += size
    dest = pattern(dst + 37)
    rc, got = run_emit(hip, image, len(image), dest, entries)
    assert rc == 0
    files = np.concatenate([np.concatenate([hd[k][:43], image[e[0] + 43:e[0] + e[2]]]) for k, e in enumerate(entries)])
    assert np.array_equal(got[5:dst], files)
    assert np.array_equal(got[:5], dest[:5]) and np.array_equal(got[dst:], dest[dst:])


def test_a_file_longer_than_one_sweep_of_the_grid(hip):
    """the grid is capped at 1024 x 256 lanes of 16 bytes: a file of more than 4 MiB takes the grid-stride loop"""
    size = (4 << 20) + 3 * 4096 + 7
    image = random_image(size + 3, 5)
    hd = headers(1, 6)
    dest = pattern(size + 64)
    entries = [(3, 25, size, 43, hd[0])]
    rc, got = run_emit(hip, image, len(image), dest, entries)
    assert rc == 0 and np.array_equal(got, expectation(image, dest, entries))


def test_more_entries_than_grid_rows(hip):
    """blockIdx.y is capped at 65535: the entries beyond are reached by the stride over the table"""
    n, size = 66000, 44
    image = random_image(n * size, 7)
    dest = pattern(n * size + 48)
    entries = [(k * size, 9 + k * size, size, 0, None) for k in range(n)]
    rc, got = run_emit(hip, image, len(image), dest, entries)
    assert rc == 0
    assert np.array_equal(got[9:9 + n * size], image)
    assert np.array_equal(got[:9], dest[:9]) and np.array_equal(got[9 + n * size:], dest[9 + n * size:])


def test_skipped_entries_write_nothing(hip):
    image = random_image(1000, 8)
    hd = headers(6, 9)
    dest = pattern(6 * 256)
    entries = [(10, 7, 100, 43, hd[0]),                  # good
               (901, 256 + 7, 100, 43, hd[1]),           # ends one byte behind the image
               (10, 512 + 7, 100, 7, hd[2]),             # a header size the format does not have
               (10, 768 + 7, 20, 43, hd[3]),             # a header longer than the file
               (900, 1024 + 7, 100, 43, hd[4]),          # ends with the image: good
               (2000, 1280 + 7, 0, 0, hd[5])]            # starts behind the image
    rc, got = run_emit(hip, image, len(image), dest, entries)
    assert rc == 0
    want = expectation(image, dest, [entries[0], entries[4]])
    assert np.array_equal(got, want)
    assert not np.array_equal(want, dest)


def test_empty_table_is_a_no_op(hip):
    image = random_image(256, 10)
    dest = pattern(256)
    rc, got = run_emit(hip, image, len(image), dest, [])
    assert rc == 0 and np.array_equal(got, dest)
