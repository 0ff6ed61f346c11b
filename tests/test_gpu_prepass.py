"""sla_hip_launch_prepass / sla_hip_launch_prepass_tiles (k_prepass) and sla_hip_launch_batch_scan (k_batch_scan,
kernels/prepass.inc) against the numpy model of tests/prepassmodel.py: the OR word, the silence mask after right-justify and
mid/side, the count of all-zero mask words, the per-1024 tile words, and the three words per file of a batch.  Planes are
mostly zero with single crafted samples at the places where the kernels' indexing can go wrong; every buffer carries
sentinels behind what the call may write."""
import ctypes as C

import numpy as np
import pytest

import prepassmodel as M
import sla_amd

pytestmark = pytest.mark.gpu

SENT32 = 0xDEADBEEF
SENT64 = 0xDEADBEEFCAFEF00D
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 70001)
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def L():
    import torch
    torch.cuda.init()
    return sla_amd.lib()


def _positions(n):
    pos = {0, 63, 64, n - 1}
    for b in range(1024, n + 1, 1024):                          # both sides of every 1024 (and so every 4096) boundary
        pos |= {b - 1, b}
    return sorted(p for p in pos if 0 <= p < n)


def _planes(nch, n, bits, ms, variant):
    """int32 [nch, n].  "crafted": one sample per listed position, its kind cycling; "last": one sample at n - 1 only;
    "zero": nothing"""
    shift = 32 - bits
    pcm = np.zeros((nch, n), np.int64)
    if variant == "last" and n:
        pcm[nch - 1, n - 1] = 1 << shift
    if variant == "crafted":
        kinds = ["one", "minus"] + (["below"] if shift else []) + (["l=-r", "l=1", "l=r=1", "l=r=-1"] if ms else [])
        kinds += ["l=r=min"] if ms and bits == 32 else []
        for i, p in enumerate(_positions(n)):
            kind = kinds[i % len(kinds)]
            ch = nch - 1 if i % 3 else i % nch                  # mostly the last channel only (the generic path's last read)
            if kind == "one":
                pcm[ch, p] = 1 << shift
            elif kind == "minus":
                pcm[ch, p] = -1 << shift
            elif kind == "below":                               # only bits below the shift: the OR word sees them, the mask not
                pcm[ch, p] = (1 << shift) - 1 if i % 2 else 1
            elif kind == "l=-r":
                pcm[0, p], pcm[1, p] = 3 << shift, -3 << shift
            elif kind == "l=1":
                pcm[0, p] = 1 << shift
            elif kind == "l=r=1":
                pcm[0, p] = pcm[1, p] = 1 << shift
            elif kind == "l=r=-1":
                pcm[0, p] = pcm[1, p] = -1 << shift
            elif kind == "l=r=min":                             # mid and side both wrap to zero: silent, as the oracle has it
                pcm[0, p] = pcm[1, p] = INT32_MIN
    return pcm.astype(np.int32)


def _run(L, pcm, bits, ms, tiles):
    import torch
    nch, n = pcm.shape
    stride = n + 37
    planes = np.full((nch, stride), 0x7FFFFFFF, np.int32)       # poison behind every plane
    planes[:, n::2] = -1
    planes[:, :n] = pcm
    nwords, ntile = (n + 63) // 64, (n + 4095) // 4096 * 4
    mask_len = (nwords + 15) // 16 * 16 + 16
    d_pcm = torch.from_numpy(planes).cuda()
    d_or = torch.from_numpy(np.full(4, SENT32, np.uint32).view(np.int32)).cuda()
    d_nz = torch.from_numpy(np.full(mask_len, SENT64, np.uint64).view(np.int64)).cuda()
    d_tile = torch.from_numpy(np.full(ntile + 8, SENT32, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    args = [C.c_void_p(d_pcm.data_ptr()), C.c_uint64(stride), nch, n, bits, ms, C.c_void_p(d_or.data_ptr()), C.c_void_p(d_nz.data_ptr())]
    if tiles:
        rc = L.sla_hip_launch_prepass_tiles(*args, C.c_void_p(d_tile.data_ptr()), None)
    else:
        rc = L.sla_hip_launch_prepass(*args, None)
    assert rc == 0
    torch.cuda.synchronize()
    orw = d_or.cpu().numpy().view(np.uint32)
    nz = d_nz.cpu().numpy().view(np.uint64)
    tl = d_tile.cpu().numpy().view(np.uint32)
    want_or, want_mask, want_zero, want_tiles = M.prepass(pcm, bits, ms)
    where = (nch, n, bits, ms, tiles)
    assert orw.tolist() == [want_or, want_zero, SENT32, SENT32], where
    assert np.array_equal(nz[:nwords], want_mask), where
    assert (nz[nwords:] == SENT64).all(), where                  # nothing behind ceil(n / 64) words
    if tiles:
        assert np.array_equal(tl[:ntile], want_tiles), where
        assert (tl[ntile:] == SENT32).all(), where
    else:
        assert (tl == SENT32).all(), where
    if n % 64:
        assert int(nz[nwords - 1]) >> (n % 64) == 0, where       # bits at or above n: sla_hip_launch_zero_runs depends on it
    return want_zero


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
@pytest.mark.parametrize("nch,ms", [(1, 0), (2, 0), (2, 1), (3, 0), (5, 0), (8, 0)])
def test_prepass(L, nch, ms, bits):
    zero_words = 0
    for n in SIZES:
        for variant in ("crafted", "last", "zero"):
            pcm = _planes(nch, n, bits, ms, variant)
            zero_words += _run(L, pcm, bits, ms, True)
            if variant == "crafted":
                _run(L, pcm, bits, ms, False)
    assert zero_words > 1000


def test_prepass_values_the_model_takes_from_the_oracle(L):
    """mid/side in wrapping arithmetic at 32 bits: L = R = INT32_MIN is silent, L = INT32_MIN alone is not"""
    pcm = np.zeros((2, 200), np.int32)
    pcm[:, 10:90] = INT32_MIN
    pcm[0, 150] = INT32_MIN
    pcm[:, 160] = [INT32_MIN, 2 ** 31 - 1]
    _, mask, zero, _ = M.prepass(pcm, 32, 1)
    assert [int(w) for w in mask] == [0, 0, (1 << (150 - 128)) | (1 << (160 - 128)), 0] and zero == 3
    _run(L, pcm, 32, 1, True)
    assert M.prepass(pcm, 32, 0)[2] == 1                          # without mid/side those samples are loud
    _run(L, pcm, 32, 0, True)


# ---- batch scan ----------------------------------------------------------------------------------------------------------

LENS = (1, 63, 64, 126, 127, 1024, 4096 + 126, 4096 + 127, 3 * 4096, 70001)
VARIANTS = 8


def _batch(num_files, max_block, seed):
    """files back to back on 1024-sample starts (every third with an empty tile between): mask, tile words, starts, lengths.
    Inside a file every bit is set except what the file's variant clears; the gaps are zero."""
    rng = np.random.default_rng(seed)
    starts, lens, pos = [], [], 1024 * 3
    for f in range(num_files):
        ln = LENS[(f + seed) % len(LENS)]
        starts.append(pos)
        lens.append(ln)
        pos = (pos + ln + 1023) // 1024 * 1024 + (1024 if f % 3 == 0 else 0)
    bits = np.zeros(pos + 1024, bool)
    for f, (s, ln) in enumerate(zip(starts, lens)):
        b = bits[s:s + ln]
        b[:] = True
        v = (f // len(LENS) + f + seed) % VARIANTS
        rem = ln % max_block if max_block else ln % 4096
        whole = ln // 64
        if v == 1 and whole:                                    # zero words at the first and at the last whole word
            b[:64] = False
            b[(whole - 1) * 64:whole * 64] = False
        elif v == 2:                                            # the tail of the last super-frame all zero
            b[ln - rem:] = False
        elif v == 3 and rem:                                    # .. but for its first sample
            b[ln - rem:] = False
            b[ln - rem] = True
        elif v == 4 and rem:                                    # .. but for its last sample
            b[ln - rem:] = False
            b[ln - 1] = True
        elif v == 5:                                            # the whole file
            b[:] = False
        elif v == 6:                                            # the partial last word only
            b[whole * 64:] = False
        elif v == 7 and whole >= 3:                             # a word in the middle
            b[64:128] = False
    mask = M.Z.mask_words(bits)
    tile_or = rng.integers(1, 2 ** 32, len(bits) // 1024, dtype=np.uint64).astype(np.uint32)    # the gaps' tiles too
    return mask, tile_or, np.array(starts, np.uint32), np.array(lens, np.uint32)


@pytest.mark.parametrize("max_block", [2048, 4096, 16384, 0])
@pytest.mark.parametrize("num_files", [1, 2, 7, 300])
def test_batch_scan(L, num_files, max_block):
    import torch
    seen_tail = seen_zero = 0
    for seed in range(10 if num_files < 300 else 1):
        mask, tile_or, starts, lens = _batch(num_files, max_block, seed)
        want = M.batch_scan(mask, tile_or, starts, lens, max_block)
        d_mask = torch.from_numpy(mask.view(np.int64)).cuda()
        d_tile, d_start, d_len = (torch.from_numpy(a.view(np.int32)).cuda() for a in (tile_or, starts, lens))
        d_info = torch.from_numpy(np.full(3 * num_files + 5, SENT32, np.uint32).view(np.int32)).cuda()
        torch.cuda.synchronize()
        rc = L.sla_hip_launch_batch_scan(C.c_void_p(d_mask.data_ptr()), C.c_void_p(d_tile.data_ptr()), C.c_void_p(d_start.data_ptr()),
                                         C.c_void_p(d_len.data_ptr()), num_files, max_block, C.c_void_p(d_info.data_ptr()), None)
        assert rc == 0
        torch.cuda.synchronize()
        got = d_info.cpu().numpy().view(np.uint32)
        assert (got[3 * num_files:] == SENT32).all()
        bad = np.flatnonzero(got[:3 * num_files] != want)
        assert len(bad) == 0, [(int(i) // 3, int(i) % 3, int(lens[i // 3]), int(got[i]), int(want[i])) for i in bad[:8]]
        seen_tail += int(want[2::3].sum())
        seen_zero += int(want[1::3].sum())
    assert seen_zero > 0 and (seen_tail > 0) == (max_block != 0)
