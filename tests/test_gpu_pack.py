"""The device bit-pack kernels (sla_amd/csrc/kernels/pack.inc: k_rice_k / k_rice_k2 / k_rice_bits / k_rice_write / k_block_crc, and
sla_crc_dev.h) through the C-ABI launchers sla_hip_launch_rice_len / sla_hip_launch_rice_write, against the independent writer
tests/slastream.py (tests/packmodel.py: bytes, coder mode, moduli per sample, bits per channel), bit for bit.  Whole-file encodes
of audio never strain what these kernels claim:
    rice_adapt32 / rice_k32 restate the 64-bit parameter update in 32-bit pieces -- here with initial parameters up to 2^32 - 1,
      `code << 8` that wraps and residuals at the ends of int32;
    rrice_len and the write path escape to a gamma code at a quotient of 16 -- here with quotients 15 / 16 / 17 / 300 and up to
      2^32 / modulus (32 gamma digits, a codeword of about 100 bits in 32-bit pieces);
    the tile prefix sum of k_rice_write -- here with tiles of more than 64 bits per sample and 1 / 2 / 3 / 5 / 7 / 8 channels;
    k_rice_k2 walks eight jobs per wave, its B lane a batch behind -- here with jobs of 1 .. 1001 samples and Golomb jobs (nothing
      to walk) mixed in one wave, and job counts that leave a wave ragged;
    k_rice_k moves 8 samples per 16-byte access once the residual and the k address are aligned TOGETHER -- here with block offsets
      of every residue mod 8 under an odd plane stride (a prologue of 0 .. 7 samples), with offsets and stride that are multiples
      of 8 (none), and with the k plane one element off the residual plane (the two never align: the scalar loop alone);
    crc16_wave cuts a block into 64 slices at whatever byte offset it landed on -- here with blocks of 11 bytes (3 bytes under the
      CRC), below 64, of 64 + 8 and 65 + 8 bytes and of several KB, at every offset mod 4, back to back (neighbours share a 32-bit
      word), with gaps, in descending order, and split over two launches inside a shared word (as the encoder does for big files);
    RAW blocks of 4 .. 32 bits with and without mid/side.
Everything a launch must NOT write carries a sentinel or is compared afterwards: the image outside the blocks stays zero, the k
planes outside adaptive jobs and the bit counts beyond num_jobs keep their fill, residual and PCM planes are unchanged.

32-bit mid/side RAW blocks: the side channel is a 33-bit field whose top bit is always clear -- side = (int32)(l - r) folded is
below 2^32, a set top bit cannot come out of an encoder (and k_rice_write's input is int32 PCM, so no call can ask for one; the
catalogue's RAW blocks, which do set it for the decoders, are replaced by the RAW cases here).  The reference's bit writer is
undefined at those fields where they start at bit 7 of a byte (tests/test_oracle_vs_ref.py::
test_32bit_mid_side_raw_blocks_follow_the_format), so the yardstick is the format as tests/slastream.py writes it.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import crafted_catalogue as CC
import packmodel as PM
import slastream as SS

gpu = pytest.mark.gpu                             # the tests that launch; the ones that only check what the tables hold run anywhere

DEVICE = "cuda"
KK_SENTINEL = 0xA5C3
BITS_SENTINEL = 0xA5A5A5A5A5A5A5A5
INVALID_ARGUMENT = 2                              # include/SLA.h
RICE_K2_MAX_JOBS = 32768                          # pack.inc: beyond it the launcher walks one lane per job (k_rice_k)
IMAGE_PAD = 8                                     # bytes of slack the encoder leaves behind the last block (sla_encoder.c)


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


class RiceJob(C.Structure):                       # sla_hip_rice_job
    _fields_ = [("blk_off", C.c_uint64), ("blk_len", C.c_uint32), ("channel", C.c_uint32), ("rice_init", C.c_uint32),
                ("golomb_m", C.c_uint32)]


class PackBlock(C.Structure):                     # sla_hip_pack_block
    _fields_ = [("blk_off", C.c_uint64), ("out_off", C.c_uint64), ("num_samples", C.c_uint32), ("type", C.c_uint32),
                ("header_off", C.c_uint32), ("header_bytes", C.c_uint32), ("out_bytes", C.c_uint32), ("raw_bits", C.c_uint32),
                ("golomb_m", C.c_uint32 * 8)]


class Tuning(C.Structure):                        # sla_hip_tuning
    _fields_ = [("lpc_pack", C.c_uint32), ("lpc_threads", C.c_uint32), ("lpc_blocks_chains", C.c_uint32), ("tail_waves", C.c_uint32),
                ("lpc_tile", C.c_uint32), ("tail_taps", C.c_uint32), ("plan_margin", C.c_double), ("rice_lanes", C.c_uint32),
                ("lattice_plain", C.c_uint32), ("cert_audit", C.c_uint32)]


assert C.sizeof(RiceJob) == 24 and C.sizeof(PackBlock) == 72


@contextlib.contextmanager
def rice_lanes(L, lanes):
    t = Tuning()
    t.rice_lanes = lanes
    L.sla_hip_use_tuning(C.byref(t))
    try:
        yield
    finally:
        L.sla_hip_use_tuning(None)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEVICE)


def sync():
    if DEVICE == "cuda":
        import torch
        torch.cuda.synchronize()


def ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def struct_bytes(arr):
    return np.frombuffer(bytes(arr), np.uint8).copy()


# ---- a plane set with its blocks ---------------------------------------------------------------------------------------

LAYOUTS = ("odd", "mult8", "skewed")


class Table:
    """blocks (packmodel.Expected) laid out in channel planes.  layout "odd": an odd plane stride and block offsets of every
    residue mod 8; "mult8": stride and offsets are multiples of 8; "skewed": as "odd", and the k plane starts one element
    (2 bytes) behind a 16-byte boundary while the residual plane starts on one.  Words no block owns hold noise."""

    def __init__(self, fmt, expected, layout="odd", name=""):
        assert layout in LAYOUTS
        self.fmt, self.C, self.blocks, self.layout, self.name = fmt, fmt.num_channels, list(expected), layout, name
        self.off, cursor = [], 5
        for i, e in enumerate(self.blocks):
            off = cursor + 1                      # at least one word between neighbours that no block owns
            while off % 8 != (0 if layout == "mult8" else (3 * i + 1) % 8):
                off += 1
            self.off.append(off)
            cursor = off + e.blk.n
        self.stride = cursor + 37
        while (self.stride % 8 != 0) if layout == "mult8" else (self.stride % 2 == 0):
            self.stride += 1
        self.kk_skew = 1 if layout == "skewed" else 0
        rng = np.random.default_rng(self.stride)
        self.res = rng.integers(-2 ** 31, 2 ** 31, (self.C, self.stride), dtype=np.int64).astype(np.int32)
        self.pcm = rng.integers(-2 ** 31, 2 ** 31, (self.C, self.stride), dtype=np.int64).astype(np.int32)
        for e, off in zip(self.blocks, self.off):
            if e.blk.type == SS.COMPRESS:
                self.res[:, off:off + e.blk.n] = e.res
            elif e.blk.type == SS.RAW:
                self.pcm[:, off:off + e.blk.n] = e.pcm
        self.jobs = [(b, ch) for b, e in enumerate(self.blocks) if e.blk.type == SS.COMPRESS for ch in range(self.C)]

    def job_len(self, j):
        return self.blocks[self.jobs[j][0]].blk.n

    def upload(self):
        self.d_res, self.d_pcm = dev(self.res), dev(self.pcm)
        self.new_kk()

    def new_kk(self):
        """a k plane full of the sentinel, with guard elements in front of and behind the planes"""
        self.kk_words = self.kk_skew + self.C * self.stride + 8
        self.d_kk = dev(np.full(self.kk_words, KK_SENTINEL, np.uint16).view(np.int16))
        self.kk_ptr = ptr(self.d_kk, 2 * self.kk_skew)
        assert self.d_res.data_ptr() % 16 == 0 and self.d_kk.data_ptr() % 16 == 0

    def want_kk(self, num_jobs):
        want = np.full(self.kk_words, KK_SENTINEL, np.uint16)
        for b, ch in self.jobs[:num_jobs]:
            e = self.blocks[b]
            if e.kk[ch] is not None:
                at = self.kk_skew + ch * self.stride + self.off[b]
                want[at:at + e.blk.n] = e.kk[ch]
        return want

    def planes_unchanged(self, what):
        assert np.array_equal(self.d_res.cpu().numpy(), self.res), what + ("the residual planes changed",)
        assert np.array_equal(self.d_pcm.cpu().numpy(), self.pcm), what + ("the PCM planes changed",)


def check_len(hip, table, lanes, num_jobs=None, what=()):
    """one sla_hip_launch_rice_len over the first num_jobs jobs of the table (fresh k planes): k0 | k1 << 8 of every sample
    of every adaptive job, the body bits of every job, sentinels everywhere else"""
    L = hip.lib()
    nj = len(table.jobs) if num_jobs is None else num_jobs
    what = (table.name, table.layout, "rice_lanes", lanes, "num_jobs", nj) + what
    jobs = (RiceJob * max(len(table.jobs), 1))()
    for j, (b, ch) in enumerate(table.jobs):
        e = table.blocks[b]
        jobs[j] = RiceJob(table.off[b], e.blk.n, ch, e.inits[ch], e.golomb_m[ch])
    d_jobs = dev(struct_bytes(jobs))
    d_bits = dev(np.full(len(table.jobs) + 4, BITS_SENTINEL, np.uint64).view(np.int64))
    table.new_kk()
    sync()
    with rice_lanes(L, lanes):
        rc = L.sla_hip_launch_rice_len(ptr(table.d_res), C.c_uint64(table.stride), ptr(d_jobs), C.c_uint32(nj), table.kk_ptr,
                                       ptr(d_bits), None)
    assert rc == 0, what
    sync()
    kk = table.d_kk.cpu().numpy().view(np.uint16)
    bits = d_bits.cpu().numpy().view(np.uint64)
    for j, (b, ch) in enumerate(table.jobs[:nj]):
        e = table.blocks[b]
        ctx = what + ("job", j, "block", b, "channel", ch, "len", e.blk.n, "init", e.inits[ch], "golomb_m", e.golomb_m[ch])
        if e.kk[ch] is not None:
            at = table.kk_skew + ch * table.stride + table.off[b]
            got = kk[at:at + e.blk.n]
            assert np.array_equal(got, e.kk[ch]), ctx + ("first k difference at sample", int(np.argmax(got != e.kk[ch])),
                                                         "got", hex(int(got[np.argmax(got != e.kk[ch])])),
                                                         "want", hex(int(e.kk[ch][np.argmax(got != e.kk[ch])])))
        assert int(bits[j]) == e.chan_bits[ch], ctx + ("body bits", int(bits[j]), e.chan_bits[ch])
    assert np.array_equal(kk, table.want_kk(nj)), what + ("a k outside every adaptive job's range was written",)
    assert all(int(v) == BITS_SENTINEL for v in bits[nj:]), what + ("a bit count beyond num_jobs was written",)
    table.planes_unchanged(what)


SPACINGS = ("back", "gaps", "descending", "split")


def place(table, spacing, first=43):
    """(byte offset of every block in the image, table order, launches as (first, count) of the block table)"""
    n = len(table.blocks)
    offs, cur = [], first
    for i, e in enumerate(table.blocks):
        cur += (1 + i % 5) if spacing == "gaps" else 0
        offs.append(cur)
        cur += len(e.data)
    order = list(range(n))[::-1] if spacing == "descending" else list(range(n))
    runs = [(0, n)]
    if spacing == "split":
        cut = next((i for i in range(n // 2, n) if offs[i] % 4), None) or next(i for i in range(1, n) if offs[i] % 4)
        runs = [(0, cut), (cut, n - cut)]
    return offs, order, runs


def check_write(hip, table, spacing="back", what=()):
    """sla_hip_launch_rice_write over the table's blocks into a zeroed image (the k planes as the last check_len left them):
    every block's bytes with size and CRC16, zero everywhere else, and nothing else touched"""
    L = hip.lib()
    fmt = table.fmt
    what = (table.name, table.layout, spacing) + what
    offs, order, runs = place(table, spacing)
    end = max(o + len(e.data) for o, e in zip(offs, table.blocks))
    img_bytes = (end + IMAGE_PAD + 3) & ~3
    rng = np.random.default_rng(end)
    pool, hoff = bytearray(), []
    for i, e in enumerate(table.blocks):          # headers at arbitrary places of a pool of noise
        pool += bytes(rng.integers(0, 256, 1 + (7 * i) % 5, dtype=np.uint8))
        hoff.append(len(pool))
        pool += e.header
    pool += bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    blocks = (PackBlock * len(order))()
    for t, b in enumerate(order):
        e = table.blocks[b]
        blocks[t] = PackBlock(table.off[b], offs[b], e.blk.n, e.blk.type, hoff[b], e.header_bytes, len(e.data),
                              fmt.bits - fmt.lshift, (C.c_uint32 * 8)(*((e.golomb_m or []) + [0] * 8)[:8]))
    d_blocks, d_pool = dev(struct_bytes(blocks)), dev(np.frombuffer(bytes(pool), np.uint8))
    d_img = dev(np.zeros(img_bytes // 4 + 4, np.int32))                   # four guard words behind the image
    kk_before = table.d_kk.cpu().numpy().copy()
    sync()
    for lo, cnt in runs:
        rc = L.sla_hip_launch_rice_write(ptr(table.d_res), ptr(table.d_pcm), C.c_uint64(table.stride), table.kk_ptr,
                                         ptr(d_blocks, lo * C.sizeof(PackBlock)), C.c_uint32(cnt), ptr(d_pool), C.c_uint32(table.C),
                                         C.c_uint32(32 - fmt.bits + fmt.lshift), C.c_uint32(fmt.ms), ptr(d_img), None)
        assert rc == 0, what
    sync()
    img = d_img.cpu().numpy().view(np.uint8)
    want = np.zeros(len(img), np.uint8)
    for b, e in enumerate(table.blocks):
        got = img[offs[b]:offs[b] + len(e.data)]
        exp = np.frombuffer(e.data, np.uint8)
        want[offs[b]:offs[b] + len(e.data)] = exp
        if not np.array_equal(got, exp):
            at = int(np.argmax(got != exp))
            where = "size / CRC16 field" if 2 <= at < 8 else ("header" if at < e.header_bytes else "body byte %d" % (at - e.header_bytes))
            raise AssertionError(what + ("block", b, "type", e.blk.type, "samples", e.blk.n, "bytes", len(e.data), "out_off", offs[b],
                                         "golomb_m", e.golomb_m, "first difference at byte", at, where,
                                         "got", hex(int(got[at])), "want", hex(int(exp[at]))))
    assert np.array_equal(img, want), what + ("an image byte outside every block was written",
                                              int(np.argmax(img != want)))
    assert np.array_equal(table.d_kk.cpu().numpy(), kk_before), what + ("the k planes changed",)
    table.planes_unchanged(what)
    return offs


# ---- a. the crafted catalogue --------------------------------------------------------------------------------------------

CASES = CC.catalogue()


def catalogue_table(case, layout="odd"):
    """every COMPRESS and SILENT block of a case in one plane set (its RAW blocks hold codes no PCM gives: see test_raw_blocks)"""
    return Table(case.fmt, [e for e in PM.catalogue_expected()[case.name] if e.blk.type != SS.RAW], layout, case.name)


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_catalogue(hip, case):
    """one rice_len launch and one rice_write launch over all blocks of the case, with both walk kernels: the moduli of every
    sample, the bits of every (block, channel), the bytes of every block with its size and CRC16"""
    table = catalogue_table(case)
    assert len(table.blocks) == sum(b.type != SS.RAW for b in case.blocks) and table.jobs
    table.upload()
    for lanes in (1, 2):
        check_len(hip, table, lanes)
        check_write(hip, table, "back", what=("k planes of rice_lanes", lanes))


def test_catalogue_puts_the_kernels_under_strain():
    """what test_catalogue hands the kernels, from the writer's Stats over the blocks it launches (as
    tests/test_crafted_streams.py::test_catalogue_reaches_every_target does for the decoders): a tile of more than 64 bits
    per sample, a Golomb modulus above 8 that is no power of two, gamma escapes, quotients 15 / 16 / 17, an initial parameter
    of at least 2^24 and both coder modes; and in the job tables themselves the inits and lengths of the issue"""
    st = SS.Stats()
    for c in CASES:
        st.merge(c.stats)                         # (RAW blocks add nothing to the fields read here)
    assert st.max_tile_bits_per_sample > 64
    assert any(m & (m - 1) and m > 8 for ms in st.golomb_m for m in ms)
    assert st.gamma_escapes > 0 and {15, 16, 17} <= st.quotients and st.max_quotient >= 300
    assert st.max_init >= 1 << 24
    assert {"rice", "golomb"} <= set(st.coder)
    inits, lens, chans, modes = set(), set(), set(), set()
    for c in CASES:
        t = catalogue_table(c)
        chans.add(t.C)
        for b, ch in t.jobs:
            e = t.blocks[b]
            inits.add(e.inits[ch]); lens.add(e.blk.n); modes.add(bool(e.golomb_m[ch]))
            if e.golomb_m[ch] == 0:
                assert len(e.kk[ch]) == e.blk.n
    assert {0, 1, 8, 9, 1 << 16, (1 << 24) - 1, 1 << 24, (1 << 32) - 1} <= inits
    assert {1, 63, 64, 65, 4097, 16384} <= lens and chans >= {1, 2, 3, 8} and modes == {False, True}
    assert len(st.chan_bits) == sum(b.type == SS.COMPRESS for c in CASES for b in c.blocks)


# ---- b. a table made for the walk kernels and the scan -------------------------------------------------------------------

WALK_LENGTHS = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 193, 1001)
WALK_KINDS = ("tiny", "16bit", "31bit", "extremes")
ESCAPE_INITS = (9, 10, 300)                       # of the blocks whose every sample is a long gamma escape
ADAPTIVE_INITS = (9, (1 << 24) - 1, (1 << 32) - 1, 1 << 16, 300, 10)
GOLOMB_INITS = (1, 3, 8, 5, 2, 7, 6, 4)
JOB_COUNTS = (1, 7, 9, 31, 33, 75)                # and the whole table


def walk_residuals(rng, kind, n, span=4):
    if kind == "tiny":
        return rng.integers(-span, span + 1, n).astype(np.int32)
    if kind == "16bit":
        return rng.integers(-(1 << 15), 1 << 15, n).astype(np.int32)
    if kind == "31bit":
        return rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    return np.resize(np.array([-(1 << 31), (1 << 31) - 1, -1, 0, 1], np.int64), n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def walk_blocks(nch):
    """(format, Expected of every block, job order).  At least 75 jobs; every third block is in Golomb mode (tiny residuals:
    a Golomb quotient is written in unary), the others adaptive with a residual family and an init per channel; channel 1
    of every fourth adaptive block starts from init 1; every fifth block costs more than 64 bits per sample in every channel"""
    rng = np.random.default_rng(700 + nch)
    fmt = SS.Format(nch, 32, order=2, ntaps=1, lms=4)
    nb = max(15, -(-75 // nch))
    blocks = []
    for i in range(nb):
        n = WALK_LENGTHS[i % len(WALK_LENGTHS)]
        chans = []
        for ch in range(nch):
            if i % 3 == 1:
                init = GOLOMB_INITS[(i + ch) % 8]
                res = walk_residuals(rng, "tiny", n, 4 * init)
            else:
                init = ADAPTIVE_INITS[(i - (i + 2) // 3 + ch) % 6]          # (the count of adaptive blocks before this one)
                if ch == 1 and i % 4 == 0:
                    init = 1
                if ch == 0 and nch > 1 and i % 4 == 0:
                    init = (1 << 24) - 1          # keeps the block's mean parameter above the threshold
                res = walk_residuals(rng, WALK_KINDS[(i * nch + ch + i // len(WALK_LENGTHS)) % 4], n)
                if i % 5 == 2:                    # codes k 2^24 + m0, as the catalogue's tiles of more than 64 bits per sample
                    init, ks = ESCAPE_INITS[ch % 3], rng.integers(1, 256, n)
                    res = PM.unfold(CC.adaptive_codes(init, n, lambda s, m0, m1: (int(ks[s]) << 24) + m0))
            chans.append(SS.Chan(int(rng.integers(0, 16)), [int(c) for c in rng.integers(-100, 100, fmt.order)], None, init, res))
        blocks.append(SS.Block(SS.COMPRESS, n, chans))
    expected, st = PM.expect_blocks(fmt, blocks)
    for i, e in enumerate(expected):
        assert all(bool(m) == (i % 3 == 1) for m in e.golomb_m), (i, e.inits, e.golomb_m)
    return fmt, expected, st


def mixed_order(table):
    """the table's jobs reordered so that every wave of eight holds jobs of one batch of 64 samples and jobs of several: the
    jobs of at most 64 samples and the longer ones, each list with its lengths spread out, dealt out evenly over the table"""
    by_len = sorted(range(len(table.jobs)), key=lambda j: (table.job_len(j), j))
    def dealt(jobs):                              # a walk through the sorted list in steps coprime to its length
        step = next(p for p in (5, 7, 11, 13) if len(jobs) % p)
        return [jobs[(i * step) % len(jobs)] for i in range(len(jobs))]

    short = dealt([j for j in by_len if table.job_len(j) <= 64])
    long_ = dealt([j for j in by_len if table.job_len(j) > 64])
    keyed = [((i + 0.5) / len(short), j) for i, j in enumerate(short)] + [((i + 0.5) / len(long_), j) for i, j in enumerate(long_)]
    out = [j for _, j in sorted(keyed)]
    assert sorted(out) == list(range(len(table.jobs)))
    return [table.jobs[j] for j in out]


def walk_table(nch, layout):
    fmt, expected, _ = walk_blocks(nch)
    table = Table(fmt, expected, layout, "walk table, %d channels" % nch)
    table.jobs = mixed_order(table)
    return table


def check_walk_table_shape(table):
    """the properties the table is made for (asserted, so a change of the lists cannot quietly lose them)"""
    nj = len(table.jobs)
    assert nj >= 75 and set(WALK_LENGTHS) == {table.job_len(j) for j in range(nj)}
    mixed_modes = 0
    for w in range(0, nj - 7, 8):
        lens = [table.job_len(j) for j in range(w, w + 8)]
        assert min(lens) <= 64 < max(lens) and len(set(lens)) >= 3, (w, lens)
        modes = {bool(table.blocks[b].golomb_m[ch]) for b, ch in table.jobs[w:w + 8]}
        blocks = {b for b, _ in table.jobs[w:w + 8]}
        mixed_modes += modes == {False, True} and len(blocks) > 1
    assert mixed_modes >= 3
    inits = {table.blocks[b].inits[ch] for b, ch in table.jobs if not table.blocks[b].golomb_m[ch]}
    assert inits >= ({9, (1 << 24) - 1, (1 << 32) - 1} | ({1} if table.C > 1 else set()))
    if table.layout != "mult8":
        assert {o % 8 for o in table.off} == set(range(8)) and table.stride % 2 == 1
    else:
        assert all(o % 8 == 0 for o in table.off) and table.stride % 8 == 0


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nch", [1, 3, 5, 7, 8])
def test_walk_kernels_on_mixed_waves(hip, nch, layout):
    """both walk kernels on job tables whose waves mix 1-sample and 1001-sample jobs, adaptive and Golomb jobs of different
    blocks, at job counts 1 / 7 / 9 / 31 / 33 / 75 / all (a ragged last wave, a ragged last workgroup), in the three plane
    layouts; then the write kernels over the same blocks (the scan with 1 / 3 / 5 / 7 / 8 interleaved channels)"""
    table = walk_table(nch, layout)
    check_walk_table_shape(table)
    assert len(table.jobs) % 8 != 0 or nch == 8
    table.upload()
    for lanes in (1, 2):
        for nj in JOB_COUNTS:
            check_len(hip, table, lanes, nj)
        check_len(hip, table, lanes)
        check_write(hip, table, "back" if lanes == 1 else "gaps")


def test_walk_table_reaches_its_targets():
    """the writer's Stats over the walk tables: gamma escapes with the longest quotients a 32-bit code has, tiles of more than
    64 bits per sample, both modes"""
    for nch in (1, 3, 5, 7, 8):
        _, _, st = walk_blocks(nch)
        assert st.gamma_escapes > 100 and st.max_quotient >= 1 << 27 and st.max_tile_bits_per_sample > 64
        assert {"rice", "golomb"} <= set(st.coder)
        check_walk_table_shape(walk_table(nch, "odd"))


@functools.lru_cache(maxsize=None)
def one_sample_jobs(count):
    """`count` blocks of one channel and one sample: (inits, residuals, moduli, k of the sample or None, body bits)"""
    rng = np.random.default_rng(count)
    inits_of = (1, 5, 8, 9, 300, 1 << 16, (1 << 24) - 1, (1 << 32) - 1, 0, 1 << 24)
    inits = [inits_of[int(i)] for i in rng.integers(0, len(inits_of), count)]
    res = np.empty(count, np.int32)
    golomb, kk, bits = [], [], []
    for j, init in enumerate(inits):
        m = PM.coding_mode([init])[0]
        res[j] = walk_residuals(rng, WALK_KINDS[j % 4] if m == 0 else "tiny", 1)[0]
        code = SS.fold_array(res[j:j + 1])
        st = SS.put_residuals(SS.BitWriter(), [code], [init])
        golomb.append(m); bits.append(st.chan_bits[0][0])
        kk.append(None if m else int(PM.walk(init, code)[0]))
    return inits, res, golomb, kk, bits


@gpu
def test_many_one_sample_jobs_take_the_one_lane_walk(hip):
    """more than 32768 jobs under rice_lanes = 0: the launcher's own choice is k_rice_k (513 workgroups of 64 one-sample
    walks at consecutive offsets, every alignment); a prefix of 100 jobs takes its other choice"""
    L = hip.lib()
    count = RICE_K2_MAX_JOBS + 72
    inits, res, golomb, kk, bits = one_sample_jobs(count)
    stride = count + 11
    plane = np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, stride, dtype=np.int64).astype(np.int32)
    plane[3:3 + count] = res
    jobs = (RiceJob * count)()
    for j in range(count):
        jobs[j] = RiceJob(3 + j, 1, 0, inits[j], golomb[j])
    d_res, d_jobs = dev(plane), dev(struct_bytes(jobs))
    for nj in (count, 100):
        d_kk = dev(np.full(stride + 8, KK_SENTINEL, np.uint16).view(np.int16))
        d_bits = dev(np.full(count + 4, BITS_SENTINEL, np.uint64).view(np.int64))
        sync()
        with rice_lanes(L, 0):
            rc = L.sla_hip_launch_rice_len(ptr(d_res), C.c_uint64(stride), ptr(d_jobs), C.c_uint32(nj), ptr(d_kk), ptr(d_bits), None)
        assert rc == 0
        sync()
        want_kk = np.full(stride + 8, KK_SENTINEL, np.uint16)
        want_kk[3:3 + nj] = [KK_SENTINEL if k is None else k for k in kk[:nj]]
        want_bits = np.full(count + 4, BITS_SENTINEL, np.uint64)
        want_bits[:nj] = bits[:nj]
        got_kk, got_bits = d_kk.cpu().numpy().view(np.uint16), d_bits.cpu().numpy().view(np.uint64)
        bad = np.nonzero(got_kk != want_kk)[0]
        assert len(bad) == 0, ("num_jobs", nj, "first k difference at job", int(bad[0]) - 3, "init", inits[int(bad[0]) - 3],
                               "residual", int(res[int(bad[0]) - 3]), hex(int(got_kk[bad[0]])), hex(int(want_kk[bad[0]])))
        bad = np.nonzero(got_bits != want_bits)[0]
        assert len(bad) == 0, ("num_jobs", nj, "first bit count difference at job", int(bad[0]), int(got_bits[bad[0]]), int(want_bits[bad[0]]))
        assert np.array_equal(d_res.cpu().numpy(), plane)
    assert {False, True} == {g == 0 for g in golomb}


# ---- c. RAW blocks and the layout of the image -------------------------------------------------------------------------

RAW_FORMATS = {4: (4, 0), 12: (16, 4), 16: (16, 0), 24: (24, 0), 31: (32, 1), 32: (32, 0)}     # width: (bits, lshift)
RAW_CASES = [(w, ms, 2) for w in RAW_FORMATS for ms in (0, 1)] + [(16, 0, 1), (24, 0, 3), (12, 0, 8)]


def raw_lengths(per_sample_bits):
    """block lengths for: a few bytes, under 64 bytes, 64 + 8 and 65 + 8 bytes where a length gives exactly that
    (11 header bytes, so 61 and 62 body bytes), one 64-sample tile over / under, and at least 3000 bytes"""
    out = [1, 3, 255, 256, 257]
    for body in (61, 62):
        n = (8 * body) // per_sample_bits
        if n and -(-n * per_sample_bits // 8) == body:
            out.append(n)
    out.append(max(900, -(-8 * 3000 // per_sample_bits)))
    return out


@functools.lru_cache(maxsize=None)
def raw_blocks(width, ms, nch):
    bits, lshift = RAW_FORMATS[width]
    fmt = SS.Format(nch, bits, order=4, ntaps=1, lms=4, ms=ms, lshift=lshift)
    assert fmt.bits - fmt.lshift == width
    blocks, pcms = [SS.Block(SS.SILENT, 700)], [None]
    for i, n in enumerate(raw_lengths(sum(SS.raw_widths(fmt)))):
        pcm = PM.full_scale_noise(nch, n, width, seed=1000 * width + 10 * i + ms)      # left-justified: width bits on top
        blocks.append(SS.Block(SS.RAW, n, raw=PM.raw_codes(pcm, 32 - width, ms)))
        pcms.append(pcm)
        if i % 3 == 1:
            blocks.append(SS.Block(SS.SILENT, 1 + i)); pcms.append(None)
    expected, st = PM.expect_blocks(fmt, blocks)
    for e, pcm in zip(expected, pcms):
        e.pcm = pcm
    return fmt, expected, st


@gpu
@pytest.mark.parametrize("width,ms,nch", RAW_CASES, ids=["%dbit-ms%d-%dch" % c for c in RAW_CASES])
def test_raw_blocks(hip, width, ms, nch):
    """RAW and SILENT blocks from full-scale L / R input (the corner pairs first) in the four spacings of the image; the
    codes are packmodel.raw_codes' wrap model, at 32-bit mid/side a 33-bit side field"""
    fmt, expected, st = raw_blocks(width, ms, nch)
    assert max(st.raw_widths) == width + ms and (ms == 0 or len(st.raw_widths) == 2)
    if width == 32 and ms:
        side = np.concatenate([e.blk.raw[1] for e in expected if e.blk.type == SS.RAW])
        assert int(side.max()) >> 31 == 1 and int(side.max()) >> 32 == 0          # the whole 32 bits, never the 33rd
    table = Table(fmt, expected, "odd", "raw %d bit, ms %d" % (width, ms))
    assert not table.jobs
    table.upload()
    residues = set()
    for spacing in SPACINGS:
        offs = check_write(hip, table, spacing)
        residues |= {o % 4 for o in offs}
    assert residues == {0, 1, 2, 3}


def test_raw_tables_reach_the_block_sizes():
    """the block sizes crc16_wave is cut by: 11 bytes, under 64, 64 + 8, 65 + 8, several KB; neighbours that share a word in
    every back-to-back table, and a split inside a shared word"""
    sizes = set()
    for width, ms, nch in RAW_CASES:
        fmt, expected, _ = raw_blocks(width, ms, nch)
        sizes |= {len(e.data) for e in expected}
        table = Table(fmt, expected, "odd")
        offs, _, runs = place(table, "split")
        assert len(runs) == 2 and runs[0][1] >= 1 and offs[runs[1][0]] % 4 != 0
        assert {o % 4 for sp in SPACINGS for o in place(table, sp)[0]} == {0, 1, 2, 3}
    assert {11, 72, 73} <= sizes and any(11 < s < 64 for s in sizes) and any(s >= 3000 for s in sizes)


# ---- e. arguments ------------------------------------------------------------------------------------------------------

@gpu
def test_argument_refusals(hip):
    """NULL pointers, 0 or 9 channels and a RAW shift of 32 are INVALID_ARGUMENT; no jobs / no blocks return 0; none of them
    launches anything"""
    L = hip.lib()
    fmt, expected, _ = walk_blocks(3)
    table = Table(fmt, expected[:3], "odd", "refusals")
    table.upload()
    jobs = (RiceJob * len(table.jobs))()
    for j, (b, ch) in enumerate(table.jobs):
        e = table.blocks[b]
        jobs[j] = RiceJob(table.off[b], e.blk.n, ch, e.inits[ch], e.golomb_m[ch])
    blocks = (PackBlock * 3)()
    pool, off = b"", 43
    for b, e in enumerate(table.blocks):
        blocks[b] = PackBlock(table.off[b], off, e.blk.n, e.blk.type, len(pool), e.header_bytes, len(e.data), 32,
                              (C.c_uint32 * 8)(*(e.golomb_m + [0] * 8)[:8]))
        pool += e.header
        off += len(e.data)
    d_jobs, d_blocks, d_pool = dev(struct_bytes(jobs)), dev(struct_bytes(blocks)), dev(np.frombuffer(pool, np.uint8))
    d_bits = dev(np.full(len(table.jobs) + 4, BITS_SENTINEL, np.uint64).view(np.int64))
    d_img = dev(np.zeros((off + IMAGE_PAD + 3) // 4 + 4, np.int32))
    sync()
    good_len = dict(res=ptr(table.d_res), jobs=ptr(d_jobs), nj=len(table.jobs), kk=table.kk_ptr, bits=ptr(d_bits))
    good_write = dict(res=ptr(table.d_res), pcm=ptr(table.d_pcm), kk=table.kk_ptr, blocks=ptr(d_blocks), nb=3, pool=ptr(d_pool),
                      nch=3, shift=0, img=ptr(d_img))

    def rice_len(**kw):
        a = dict(good_len, **kw)
        return L.sla_hip_launch_rice_len(a["res"], C.c_uint64(table.stride), a["jobs"], C.c_uint32(a["nj"]), a["kk"], a["bits"], None)

    def rice_write(**kw):
        a = dict(good_write, **kw)
        return L.sla_hip_launch_rice_write(a["res"], a["pcm"], C.c_uint64(table.stride), a["kk"], a["blocks"], C.c_uint32(a["nb"]),
                                           a["pool"], C.c_uint32(a["nch"]), C.c_uint32(a["shift"]), C.c_uint32(0), a["img"], None)

    for name in ("res", "jobs", "kk", "bits"):
        assert rice_len(**{name: None}) == INVALID_ARGUMENT, name
    for name in ("res", "pcm", "kk", "blocks", "pool", "img"):
        assert rice_write(**{name: None}) == INVALID_ARGUMENT, name
    assert rice_write(nch=0) == INVALID_ARGUMENT and rice_write(nch=9) == INVALID_ARGUMENT
    assert rice_write(shift=32) == INVALID_ARGUMENT
    assert rice_len(nj=0) == 0 and rice_write(nb=0) == 0
    sync()
    assert np.all(table.d_kk.cpu().numpy().view(np.uint16) == KK_SENTINEL)
    assert np.all(d_bits.cpu().numpy().view(np.uint64) == BITS_SENTINEL)
    assert not d_img.cpu().numpy().any()
    table.planes_unchanged(("refusals",))
    # the same arguments, valid, do run
    check_len(hip, table, 1)
    assert rice_write(kk=table.kk_ptr) == 0
    sync()
    img = d_img.cpu().numpy().view(np.uint8)
    assert bytes(img[43:off]) == b"".join(e.data for e in table.blocks) and not img[:43].any() and not img[off:].any()
