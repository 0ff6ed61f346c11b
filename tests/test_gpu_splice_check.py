"""GPU tests of the check kernel of sla_hip_splice_resident through its plain launcher, sla_hip_launch_splice_check (run
with -m gpu on an MI355X): crafted tables over synthetic blocks -- a chain header, a random body and the right CRC; the kernel
does not decode -- and hand-made planes.  The yardstick is tests/splicemodel.py's check_verdicts, written from the contract
text of include/sla_hip.h: every launch's whole verdict buffer, the guard words around it included, equals the model's.

Every pointer a table names lies inside a live allocation with slack on both sides; every table is followed by entries the
launch must not look at, which would fail into a word of their own."""
import ctypes as C

import numpy as np
import pytest

import indexmodel as IM
import slastream as SS
import splicemodel as SM
from splicemodel import ALL_ONES, NO_EDGE, CheckEntry

pytestmark = pytest.mark.gpu

OK, NG, INVALID_ARGUMENT, CORRUPT = 0, 1, 2, 11
JUDGE_CODES = [IM.NG, IM.BUF, IM.SYNTH, IM.DATA, IM.HEADER_FORMAT, IM.CORRUPT, 12]     # judge_row's and judge's (stop codes: 4, 9, 12)
GUARD, SLACK, PAD = 8, 64, 4
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    L = sla_amd.lib()
    L.slai_crc16.argtypes = [C.c_void_p, C.c_size_t]
    L.slai_crc16.restype = C.c_uint32
    assert sla_amd.SPLICE_NO_EDGE == NO_EDGE
    return sla_amd


def dev(a):
    import torch
    return torch.from_numpy(np.require(a, requirements=["C", "W"])).cuda()


def lib_crc(hip):
    """the library's host CRC16: what the model uses where slastream's bit-by-bit routine would take minutes"""
    def crc(data):
        a = np.frombuffer(bytes(data), np.uint8)
        return int(hip.lib().slai_crc16(a.ctypes.data, len(a))) if len(a) else 0
    return crc


class Mem:
    """the bytes the tables point into: blocks between filler, slack at both ends"""

    def __init__(self):
        self.parts, self.size = [], 0
        self._fill(SLACK)

    def _fill(self, n):
        self.parts.append(np.full(n, 0xEE, np.uint8))
        self.size += n

    def put(self, block, align=None):
        """-> the offset of the block's first byte; align: that offset modulo 16"""
        self._fill(3 if align is None else (align - self.size - 1) % 16 + 1)
        off = self.size
        self.parts.append(np.frombuffer(bytes(block), np.uint8))
        self.size += len(block)
        return off

    def done(self):
        self._fill(SLACK)
        return np.concatenate(self.parts)


def block(n, body, typ, crc16=SS.crc16, low=0):
    """a synthetic block: the chain header of n samples, type bits, `low` in the six bits behind them, the body, the CRC"""
    out = bytearray(b"\xff\xff" + (len(body) + 5).to_bytes(4, "big") + b"\0\0" + n.to_bytes(2, "big") + bytes([(typ << 6) | low]) + bytes(body))
    out[6:8] = crc16(bytes(out[8:])).to_bytes(2, "big")
    return bytes(out)


def with_byte(b, at, v):
    return b[:at] + bytes([v]) + b[at + 1:]


def run_check(hip, entries, memory, planes=None, nch=1, width=16, ms=0, outcomes=(0,), initial=None, crcs=(0, 1), crc16=SS.crc16,
              num_entries=None):
    """one launch per crc_check over the first num_entries entries (default: all).  Verdict buffer: GUARD words | the
    items' words `initial` (default: all ones, as many as the entries name) | one word for the PAD entries behind the table
    | GUARD words; num_verdicts covers the middle two.  The whole buffer against the model.  -> {crc_check: the items' words}"""
    import torch
    n = len(entries) if num_entries is None else num_entries
    if initial is None:
        initial = [ALL_ONES] * (1 + max(e.verdict for e in entries if e.verdict < (1 << 31)))
    nv = len(initial) + 1
    planes = np.zeros((nch, 4), np.int64) if planes is None else np.asarray(planes)
    stride = planes.shape[1]
    assert planes.shape[0] == nch and planes.min() >= I32_MIN and planes.max() <= I32_MAX
    d_mem = dev(memory)
    base = d_mem.data_ptr()
    assert base % 16 == 0
    flat = np.concatenate([np.full(SLACK, 0x55555555, np.int64), planes.reshape(-1), np.full(SLACK, 0x55555555, np.int64)])
    d_planes = dev(flat.astype(np.int32))
    oc = np.full((len(outcomes) + 2 * GUARD, 2), CORRUPT, np.int32)
    oc[GUARD:GUARD + len(outcomes), 0] = outcomes
    d_oc = dev(oc)
    pad = [CheckEntry(None, 0, 0, verdict=len(initial), ordinal=k) for k in range(PAD)]
    rows = [hip.SpliceCheck(None if e.src is None else base + e.src, e.plane_off, e.byte_len, e.num_samples, e.verdict, e.ordinal,
                            e.edge, e.keep) for e in list(entries) + pad]
    d_table = dev(np.frombuffer(bytes((hip.SpliceCheck * len(rows))(*rows)), np.uint8))
    start = [ALL_ONES] * GUARD + list(initial) + [ALL_ONES] * (1 + GUARD)
    got = {}
    for crc in crcs:
        d_words = dev(np.array(start, np.uint64).view(np.int64))
        rc = hip.lib().sla_hip_launch_splice_check(d_table.data_ptr(), n, crc, d_planes.data_ptr() + 4 * SLACK, stride, nch, width, ms,
                                                   d_oc.data_ptr() + 8 * GUARD, len(outcomes), d_words.data_ptr() + 8 * GUARD, nv, None)
        assert rc == 0
        torch.cuda.synchronize()
        words = [int(w) for w in d_words.cpu().numpy().view(np.uint64)]
        want = SM.check_verdicts(entries[:n], start[GUARD:], nv, memory, planes, stride, nch, width, ms, list(outcomes), crc, crc16)
        assert words[:GUARD] == [ALL_ONES] * GUARD
        if words[GUARD:] != want:
            k = next(i for i in range(len(want)) if words[GUARD + i] != want[i])
            mine = [e for e in entries[:n] if e.verdict == k]
            raise AssertionError("crc_check %d: word %d is %#x, the model's %#x; its entries: %s" % (crc, k, words[GUARD + k], want[k], mine[:4]))
        got[crc] = words[GUARD:GUARD + len(initial)]
    return got


def fail_word(e, code=CORRUPT):
    return (e.ordinal << 8) | code


# ---- verbatim entries: the header rule -------------------------------------------------------------------------------------

def test_verbatim_header_rule(hip):
    rng = np.random.default_rng(11)
    body = rng.integers(0, 256, 29, dtype=np.uint8).tobytes()
    silent = block(300, b"", 1)
    long_ = {t: block(0x1234, body, t, low=int(rng.integers(0, 64))) for t in (0, 2, 3)}
    assert len(silent) == 11 and silent == SS.block_bytes(SS.Format(), SS.Block(SS.SILENT, 300)) and len(long_[0]) == 40
    mem, entries, want = Mem(), [], []

    def add(b, blen, n, code, src=True):
        off = mem.put(b)
        entries.append(CheckEntry(off if src else None, blen, n, verdict=len(entries), ordinal=len(entries) + 1))
        want.append(code)

    for b, n in ((silent, 300), (long_[0], 0x1234)):
        add(b, len(b), n, OK)
        for at in (0, 1, 2, 3, 4, 5, 8, 9):
            for v in range(256):
                if v != b[at]:
                    add(with_byte(b, at, v), len(b), n, CORRUPT)
        for blen, nn in ((len(b) + 1, n), (len(b) - 1, n), (len(b), n + 1), (len(b), n - 1), (len(b), n + 65536), (10, n), (0, n)):
            add(b, blen, nn, CORRUPT)
        add(b, len(b), n, CORRUPT, src=False)
    for t in (0, 2, 3):
        add(block(300, b"", t), 11, 300, CORRUPT)                   # 11 bytes are a SILENT block's, whatever the CRC says
        add(long_[t], 40, 0x1234, OK)
    add(block(0x1234, body, 1), 40, 0x1234, CORRUPT)
    got = run_check(hip, entries, mem.done())
    for crc in (0, 1):
        assert got[crc] == [ALL_ONES if c == OK else fail_word(e, c) for e, c in zip(entries, want)]


# ---- verbatim entries: the CRC -----------------------------------------------------------------------------------------------

BODY_LENGTHS = [3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1087, 1088, 1089]


def flips_of(blen, every_bit):
    """(byte, bit) of the single-bit flips of a block of blen bytes: the CRC field, the first covered byte, the six bits of
    byte 10 that only the CRC covers, the last byte and one in the middle (the type bits stay: they have a rule of their own)"""
    sites = [6, 7, 8, 10, blen - 1, 8 + (blen - 8) // 2]
    out = []
    for k, at in enumerate(dict.fromkeys(sites)):
        bits = range(6 if at == 10 else 8)
        out += [(at, bit) for bit in (bits if every_bit else [(k + blen) % len(bits)])]
    return out


def crc_world(blocks, every_bit):
    """every block clean and with each of its flips, at all 16 source alignments.  The row follows the count bytes: a flip
    there is the CRC's to find.  -> (memory, entries, which entries are flipped)"""
    mem, entries, flipped = Mem(), [], []
    for b in blocks:
        for align in range(16):
            for at, bit in [(None, 0)] + flips_of(len(b), every_bit):
                v = b if at is None else with_byte(b, at, b[at] ^ (1 << bit))
                off = mem.put(v, align)
                assert off % 16 == align
                entries.append(CheckEntry(off, len(v), int.from_bytes(v[8:10], "big"), verdict=len(entries), ordinal=len(entries)))
                flipped.append(at is not None)
    return mem.done(), entries, flipped


def check_crc_world(hip, blocks, every_bit, crc16):
    memory, entries, flipped = crc_world(blocks, every_bit)
    got = run_check(hip, entries, memory, crc16=crc16)
    assert got[0] == [ALL_ONES] * len(entries)                       # without the check every flip passes
    assert got[1] == [fail_word(e) if f else ALL_ONES for e, f in zip(entries, flipped)]


def test_verbatim_crc_every_length_and_alignment(hip):
    rng = np.random.default_rng(12)
    crc = lib_crc(hip)
    blocks = []
    for k, n in enumerate(BODY_LENGTHS):
        body = rng.integers(0, 256, n - 3, dtype=np.uint8).tobytes()
        b = block(int(rng.integers(1, 65536)), body, 1 if n == 3 else (0, 2, 3)[k % 3], low=int(rng.integers(0, 64)))
        assert len(b) - 8 == n and crc(b[8:]) == SS.crc16(b[8:]) == int.from_bytes(b[6:8], "big")
        blocks.append(b)
    check_crc_world(hip, blocks, True, crc)


def test_verbatim_crc_of_the_largest_raw_block(hip):
    """11 + 65535 * 32 bytes: 8 channels of 32 bits.  The library's host CRC, held against slastream's on a small block"""
    rng = np.random.default_rng(13)
    crc = lib_crc(hip)
    small = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    assert crc(small) == SS.crc16(small)
    big = block(65535, rng.integers(0, 256, 65535 * 32, dtype=np.uint8).tobytes(), 2, crc16=crc)
    assert len(big) == 11 + 65535 * 32
    check_crc_world(hip, [big], False, crc)


# ---- edge entries ------------------------------------------------------------------------------------------------------------

def test_edge_precedence_and_table_bounds(hip):
    rng = np.random.default_rng(14)
    body = rng.integers(0, 256, 21, dtype=np.uint8).tobytes()
    good = block(500, body, 2)
    mem = Mem()
    at = {"good": mem.put(good), "sync": mem.put(with_byte(good, 1, 0xFE)), "size": mem.put(with_byte(good, 5, good[5] ^ 1)),
          "count": mem.put(with_byte(good, 9, good[9] ^ 1)), "type1": mem.put(block(500, body, 1)),
          "crc": mem.put(with_byte(good, 6, good[6] ^ 0x80)), "body": mem.put(with_byte(good, 20, good[20] ^ 4)),
          "silent": mem.put(block(500, b"", 1)), "silent_type2": mem.put(block(500, b"", 2))}
    blen = {k: (11 if k.startswith("silent") else len(good)) for k in at}
    stride, nch, width = 200, 2, 16
    planes = rng.integers(-(1 << 15), 1 << 15, (nch, stride), dtype=np.int64)
    planes[1, 100:110] = [I32_MIN, I32_MAX] * 5                    # [100, 110): out of range; everything else fits
    planes[0, 0] = planes[1, 0] = I32_MAX
    outcomes = [0] + JUDGE_CODES + [0]                               # the first and the last are clean
    last = len(outcomes) - 1
    entries, want = [], []

    def add(src, edge, plane_off, keep, code):
        entries.append(CheckEntry(at[src], blen[src], 500, verdict=len(entries), ordinal=7 * len(entries) + 1, edge=edge,
                                  plane_off=plane_off, keep=keep))
        want.append(code)

    for k, code in enumerate(JUDGE_CODES, start=1):                   # the judge's code, whatever else is wrong
        add("good", k, 10, 50, code)
        add("sync", k, 95, 20, code)
        add("silent_type2", k, 95, 20, code)
    add("good", last + 1, 10, 50, NG)                                # the outcome table's bounds
    add("good", last, 10, 50, OK)
    add("good", last, 95, 20, CORRUPT)
    add("good", NO_EDGE - 1, 10, 50, NG)
    add("good", 0, 150, 50, OK)                                      # the planes' bounds: plane_off + keep == stride
    add("good", 0, 150, 51, NG)
    add("good", 0, 200, 0, OK)
    add("good", 0, 201, 0, NG)
    add("good", 0, 1 << 63, 1, NG)
    add("good", 0, (1 << 64) - 1, 2, NG)
    add("sync", last + 1, 10, 50, NG)                                # NG comes before the header
    for src in ("sync", "size", "count", "type1", "silent_type2"):   # a bad chain header or type, clean outcome
        add(src, 0, 10, 50, CORRUPT)
    add("crc", 0, 10, 50, OK)                                        # the judge owns the CRC of edge blocks
    add("body", 0, 10, 50, OK)
    add("silent", 0, 95, 20, OK)                                     # SILENT: the planes are not looked at
    add("silent", last, 0, 200, OK)
    add("good", 0, 1, 99, OK)                                        # up to the poison, and into it
    add("good", 0, 1, 100, CORRUPT)
    add("good", 0, 110, 90, OK)
    add("good", 0, 109, 1, CORRUPT)
    add("good", 0, 0, 1, CORRUPT)
    got = run_check(hip, entries, mem.done(), planes, nch, width, 0, outcomes)
    for crc in (0, 1):
        assert got[crc] == [ALL_ONES if c == OK else fail_word(e, c) for e, c in zip(entries, want)]


KEEPS = [1, 63, 64, 65, 129, 1000]
ROW_SAMPLES = 2000


def width_world(rng, nch, width, ms):
    """per channel and keep: a clean block -- random over the whole field of every channel, both ends among them -- and
    the same block with one sample of that channel one step outside either end, at kept index 0, 63, 64, keep - 1 and one
    more.  Every block has its own range of the planes; everything outside the kept ranges is INT32_MIN or INT32_MAX.
    -> (planes, entries, the expected code of each)"""
    widths = [width + (1 if (ms and c == 1) else 0) for c in range(nch)]
    ends = [(-(1 << (min(w, 32) - 1)), (1 << (min(w, 32) - 1)) - 1) for w in widths]
    cols, entries, want = [np.tile(np.array([[I32_MIN], [I32_MAX]] * 4, np.int64)[:nch], (1, 2))], [], []
    pos = 2
    for ch in range(nch):
        for keep in KEEPS:
            base = np.stack([rng.integers(lo, hi + 1, keep, dtype=np.int64) for lo, hi in ends])
            for c, (lo, hi) in enumerate(ends):
                where = rng.permutation(keep)[:2]
                base[c, where] = [lo, hi][:len(where)]
            variants = [(base, OK)]
            if widths[ch] < 32:
                for k in sorted({0, 63, 64, keep - 1, keep // 3} & set(range(keep))):
                    for v in (ends[ch][0] - 1, ends[ch][1] + 1):
                        x = base.copy()
                        x[ch, k] = v
                        variants.append((x, CORRUPT))
            for x, code in variants:
                poison = np.array([[I32_MIN, I32_MAX][(c + len(entries)) % 2] for c in range(nch)], np.int64)[:, None]
                cols += [x, poison, -poison - 1]
                entries.append(CheckEntry(None, 16, ROW_SAMPLES, verdict=len(entries), ordinal=len(entries), edge=0, plane_off=pos, keep=keep))
                want.append(code)
                pos += keep + 2
    return np.concatenate(cols, axis=1), entries, want


def check_widths(hip, shapes, seed, crc):
    rng = np.random.default_rng(seed)
    mem = Mem()
    src = mem.put(block(ROW_SAMPLES, b"\x12\x34\x56\x78\x9a", 2))
    memory = mem.done()
    for nch, width, ms in shapes:
        planes, entries, want = width_world(rng, nch, width, ms)
        for e in entries:
            e.src = src
        assert planes.shape[1] == entries[-1].plane_off + entries[-1].keep + 2 and entries[0].plane_off >= 1
        got = run_check(hip, entries, memory, planes, nch, width, ms, crcs=(crc,))[crc]
        assert got == [ALL_ONES if c == OK else fail_word(e) for e, c in zip(entries, want)], (nch, width, ms)
        fails = sum(c != OK for c in want)
        w32 = sum(1 for c in range(nch) if width + (1 if (ms and c == 1) else 0) >= 32)
        assert fails == (nch - w32) * sum(2 * len({0, 63, 64, k - 1, k // 3} & set(range(k))) for k in KEEPS)


@pytest.mark.parametrize("width", range(1, 33))
def test_edge_width_test_every_width_mono(hip, width):
    check_widths(hip, [(1, width, 0)], 500 + width, width & 1)


@pytest.mark.parametrize("shape", [(2, 16, 1), (2, 31, 1), (2, 32, 1), (2, 32, 0), (8, 24, 0), (8, 31, 0), (3, 20, 0)],
                         ids=lambda s: "C%d_w%d_ms%d" % s)
def test_edge_width_test_channel_sets(hip, shape):
    check_widths(hip, [shape], 600 + sum(shape), 1)


def test_the_side_channel_takes_exactly_one_more_bit(hip):
    """the same planes with and without mid/side: 2^(w-1) and -(2^(w-1)) - 1 fit channel 1 under mid/side only, channel 0
    never; 2^w and -(2^w) - 1 fit neither"""
    mem = Mem()
    src = mem.put(block(ROW_SAMPLES, b"\x01\x02\x03", 2))
    memory = mem.done()
    for width in (1, 2, 15, 16, 24, 30):
        h = 1 << (width - 1)
        vals = [h - 1, -h, h, -h - 1, 2 * h - 1, -2 * h, 2 * h, -2 * h - 1]
        planes = np.zeros((2, 3 * 2 * len(vals) + 2), np.int64)
        entries = []
        for ch in range(2):
            for v in vals:
                pos = 1 + 3 * len(entries)
                planes[ch, pos + 1] = v
                entries.append(CheckEntry(src, 14, ROW_SAMPLES, verdict=len(entries), ordinal=len(entries), edge=0, plane_off=pos, keep=3))
        for ms in (0, 1):
            got = run_check(hip, entries, memory, planes, 2, width, ms, crcs=(ms,))[ms]
            fit = [True, True] + [False] * 6
            want = fit + ([True] * 6 + [False, False] if ms else fit)
            assert got == [ALL_ONES if ok else fail_word(e) for e, ok in zip(entries, want)], (width, ms)


# ---- verdict words ---------------------------------------------------------------------------------------------------------

def test_verdict_words_first_failure_by_ordinal(hip):
    rng = np.random.default_rng(15)
    good = block(64, rng.integers(0, 256, 40, dtype=np.uint8).tobytes(), 0)
    mem = Mem()
    ok_at, bad_at = mem.put(good), mem.put(with_byte(good, 9, good[9] ^ 2))
    outcomes = [0] + JUDGE_CODES
    planes = np.zeros((1, 16), np.int64)
    NV = 7                                                           # the items' words; the PAD word is word 7
    fails = {0: [((1 << 24) + 5, 10), ((1 << 24) + 9, 11), ((1 << 31) + 1, 1), ((1 << 24) + 6, 8)],
             1: [((1 << 32) - 1, 11), ((1 << 31) + 1, 8), ((1 << 31) + 2, 11)],
             2: [(0, 11), (1, 10), (300, 4)],                         # its word starts at 5 and stays
             4: [(50000, 12), (200, 4), (50, 11), (51, 9), (7000, 11)],
             6: [(0, 1)],
             NV + 1: [(3, 11), (0, 10)], 0xFFFFFFFF: [(2, 11), (0, 8)]}   # no such word: nothing changes

    def entry(item, ordinal, code):
        if code == 0:
            return CheckEntry(ok_at, len(good), 64, item, ordinal, *((NO_EDGE, 0, 0) if ordinal % 2 else (0, 2, 9)))
        if code == CORRUPT and ordinal % 2:
            return CheckEntry(bad_at, len(good), 64, item, ordinal)
        return CheckEntry(ok_at, len(good), 64, item, ordinal, edge=outcomes.index(code), plane_off=2, keep=9)

    entries, late = [], []
    for item in range(NV):
        taken = {o for o, _ in fails.get(item, [])}
        clean = [o for o in dict.fromkeys(list(range(2, 6)) + rng.integers(0, 1 << 32, 50).tolist()) if o not in taken]
        entries += [entry(item, o, 0) for o in clean[:40]]
    for item, fs in fails.items():
        first = min(fs)
        entries += [entry(item, o, c) for o, c in fs if (o, c) != first]
        late.append(entry(item, *first))
    order = rng.permutation(len(entries))
    entries = [entries[k] for k in order] + late                     # every item's smallest failing ordinal sits last in the table
    assert 280 <= len(entries) <= 320
    initial = [ALL_ONES, ALL_ONES, 5, ALL_ONES, ALL_ONES, ALL_ONES, ALL_ONES]
    got = run_check(hip, entries, mem.done(), planes, 1, 16, 0, outcomes, initial=initial)
    for crc in (0, 1):
        assert got[crc] == [(((1 << 24) + 5) << 8) | 10, (((1 << 31) + 1) << 8) | 8, 5, ALL_ONES, (50 << 8) | 11, ALL_ONES, 1]


def test_wave_tails(hip):
    """num_entries 1 .. 9 over a table of 12: the entries beyond it all fail, each into its own word"""
    rng = np.random.default_rng(16)
    good = block(64, rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), 2)
    mem = Mem()
    ok_at, bad_at = mem.put(good), mem.put(with_byte(good, 0, 0x7F))
    memory = mem.done()
    for n in range(1, 10):
        entries = [CheckEntry(bad_at if (k >= n or k % 3 == 1) else ok_at, len(good), 64, verdict=k, ordinal=k + 1) for k in range(12)]
        got = run_check(hip, entries, memory, num_entries=n, crcs=(n & 1,))[n & 1]
        assert got == [fail_word(entries[k]) if (k < n and k % 3 == 1) else ALL_ONES for k in range(12)], n


def test_refusals(hip):
    import torch
    L = hip.lib()
    good = block(64, b"\x01\x02\x03\x04", 2)
    d_mem = dev(np.frombuffer(bytes(SLACK) + with_byte(good, 0, 0) + bytes(SLACK), np.uint8))
    rows = [hip.SpliceCheck(d_mem.data_ptr() + SLACK, 0, len(good), 64, k, k, NO_EDGE, 0) for k in range(4)]      # all of them fail
    # (the tensors stay bound to names: a pointer taken from a temporary outlives its memory)
    d_table, d_planes, d_oc = dev(np.frombuffer(bytes((hip.SpliceCheck * 4)(*rows)), np.uint8)), dev(np.zeros((3, 8), np.int32)), dev(np.zeros((4, 2), np.int32))
    words = dev(np.full(16, -1, np.int64))
    t, planes, oc, v = d_table.data_ptr(), d_planes.data_ptr(), d_oc.data_ptr(), words.data_ptr() + 32
    #        table planes outcomes verdicts  C  width ms
    for a in ((None, planes, oc, v, 2, 16, 0), (t, None, oc, v, 2, 16, 0), (t, planes, None, v, 2, 16, 0), (t, planes, oc, None, 2, 16, 0),
              (t, planes, oc, v, 0, 16, 0), (t, planes, oc, v, 9, 16, 0), (t, planes, oc, v, 2, 0, 0), (t, planes, oc, v, 2, 33, 0),
              (t, planes, oc, v, 1, 16, 1), (t, planes, oc, v, 3, 16, 1)):
        for crc in (0, 1):
            assert L.sla_hip_launch_splice_check(a[0], 4, crc, a[1], 8, a[4], a[5], a[6], a[2], 4, a[3], 4, None) == INVALID_ARGUMENT, a
    assert L.sla_hip_launch_splice_check(t, 0, 1, planes, 8, 2, 16, 0, oc, 4, v, 4, None) == 0
    torch.cuda.synchronize()
    assert bool((words == -1).all())
    assert L.sla_hip_launch_splice_check(t, 4, 1, planes, 8, 2, 16, 0, oc, 4, v, 4, None) == 0      # the table is a live one
    torch.cuda.synchronize()
    assert [int(w) for w in words.cpu().numpy().view(np.uint64)] == [ALL_ONES] * 4 + [(k << 8) | 11 for k in range(4)] + [ALL_ONES] * 8
