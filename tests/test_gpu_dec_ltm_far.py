"""The long-term synthesis kernels alone, through sla_hip_launch_dec_ltm (run with -m gpu on an MI355X).

The launcher picks the kernel from its max_block_samples argument: up to 40896 samples (SLA_HIP_LDS_BUDGET / 4) k_dec_ltm,
which stages the whole block in LDS; above, k_dec_ltm_far, which slides the block through a fixed ring of LDS in chunks of
W = sla_hip_dec_ltm_window() samples.  Both must compute

    out[s] = in[s] + ((2^30 + sum_k coef[k] * out[s - delay + k]) >> 31)      for s >= delay = pitch + taps / 2,

in place, with a tap at or past the current sample reading input that is not yet synthesised (5 taps at pitch 1 or 2, 3 or 4
taps at pitch 1), a tap at or past n reading 0, wrapping adds, and nothing written outside [smp_off + delay, smp_off + n) of
compressed rows that are not HEADER_ONLY and have a pitch.

Hand-made sla_hip_dec_block / info / chan tables, one launch per table and many jobs per launch:
  lengths  1, 7, 64, 65, 2048, W - 1, W, W + 1, 2 W + 1, 40896, 40897, 65534, 65535 at (pitch, taps) = (1, 5), (64, 3),
           (257, 5), (1023, 5) -- among them delay >= n;
  pitches  1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 255, 256, 257, 1022, 1023 x 1..5 taps at n = 65535 and n = W + 1;
  operands small residuals with moderate taps, and full-range int32 with taps of -2^31 and 0x7FFF0000 (the ends of the
           16-bit tap field, << 16);
  rows     the flag set with pitch 0, SILENT and RAW rows, HEADER_ONLY rows, all with live pitches in their chan entries;
  planes   of 1, 2 and 8 channels, canary words between the blocks and behind the last one.
Expected is oracle.ltm_synth per job (tests/longblockcases.py: ltm_synth, the oracle's function with zeros behind the
block), never another run of a kernel.  Every table whose longest block is at most 40896 samples runs twice, with
max_block_samples 40896 (k_dec_ltm) and 40897 (k_dec_ltm_far): the planes must be equal bit for bit.  The per-call API
(SLALongTermSynthesizer_SynthesizeInt32) goes through the same launcher with max_block_samples = n.
"""
import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np
import pytest

import decbitsmodel as DM
import longblockcases as LB

LDS_SAMPLES = (160 * 1024 - 256) // 4              # SLA_HIP_LDS_BUDGET (include/sla_hip.h) in samples: 40896
PITCHES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 255, 256, 257, 1022, 1023)
PAIRS = ((1, 5), (64, 3), (257, 5), (1023, 5))
GAP = 67                                           # canary words behind every block
CANARY = np.int32(DM.CANARY)
CHANNELS = {1: 1, 2: 2, 3: 8, 4: 2, 5: 8}          # planes of a table, by its tap count
i32p = C.POINTER(C.c_int32)


def window():
    import os
    import sla_amd
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return int(sla_amd.lib().sla_hip_dec_ltm_window())


def lengths():
    w = window()
    return (1, 7, 64, 65, 2048, w - 1, w, w + 1, 2 * w + 1, 40896, 40897, 65534, 65535)


@dataclass
class Table:
    name: str
    ntaps: int
    C: int
    blocks: np.ndarray            # DM.BLOCK_DT [rows]
    info: np.ndarray              # uint32 [rows][4]
    chan: np.ndarray              # uint32 [rows][C][8]
    planes: np.ndarray            # int32 [C][stride]: the input
    want: np.ndarray              # int32 [C][stride]: the expected output
    active: int                   # jobs that must change something
    longest: int


def operands(rng, n, ntaps, kind):
    if kind == "full":
        x = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
        coef = np.array([-2 ** 31 if rng.integers(0, 2) else 0x7FFF0000 for _ in range(ntaps)], np.int64).astype(np.int32)
    else:
        x = rng.integers(-3000, 3000, n).astype(np.int32)
        coef = (rng.integers(-9000, 9000, ntaps).astype(np.int64) << 16).astype(np.int32)
    return x, coef


@functools.lru_cache(maxsize=None)
def table(ntaps, long_blocks):
    """the jobs of one launch: (n, pitch, kind) grouped by n into rows of C channels, rows short of C jobs filled with
    pitch-0 channels; then the rows no kernel may touch"""
    w = window()
    Cn = CHANNELS[ntaps]
    rng = np.random.default_rng(900 + 10 * ntaps + int(long_blocks))
    jobs = [(65535 if long_blocks else w + 1, p, kind) for p in PITCHES for kind in ("small", "full")]
    for pitch, taps in PAIRS:
        if taps == ntaps:
            jobs += [(n, pitch, kind) for n in lengths() if (n > LDS_SAMPLES) == long_blocks for kind in ("small", "full")]
    rows = []                                       # (n, type, flags, [(pitch, kind)] * C)
    for n in sorted({j[0] for j in jobs}):
        mine = [(p, k) for m, p, k in jobs if m == n]
        for i in range(0, len(mine), Cn):
            part = mine[i:i + Cn]
            rows.append((n, 0, 0, part + [(0, "small")] * (Cn - len(part))))
    live = [(64, "full"), (1, "small"), (1023, "full"), (3, "small"), (257, "full"), (2, "small"), (33, "full"), (255, "small")][:Cn]
    rows.append((2048, 0, 0, [(0, "full")] * Cn))                       # the flag set, pitch 0
    rows.append((3000, 1, 0, live))                                     # SILENT
    rows.append((w + 1, 2, 0, live))                                    # RAW
    rows.append((2 * w + 1, 0, DM.HEADER_ONLY, live))                   # header only, compressed
    rows.append((777, 3, 0, live))                                      # not a block type
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]

    nb = len(rows)
    blocks = np.zeros(nb, DM.BLOCK_DT)
    info = np.zeros((nb, 4), np.uint32)
    chan = np.zeros((nb, Cn, DM.CHAN_WORDS), np.uint32)
    stride = sum(r[0] + GAP for r in rows)
    planes = np.full((Cn, stride), CANARY, np.int32)
    want = planes.copy()
    pos, active = 0, 0
    for r, (n, typ, flags, chans) in enumerate(rows):
        blocks[r] = (0, 0, pos, n, flags)
        info[r] = (typ, 0, 0, 0)
        for ch, (pitch, kind) in enumerate(chans):
            x, coef = operands(rng, n, ntaps, kind)
            chan[r, ch, 0] = pitch
            chan[r, ch, 1:1 + ntaps] = coef.view(np.uint32)
            planes[ch, pos:pos + n] = x
            y = x
            if typ == 0 and flags == 0 and pitch != 0:
                y = LB.ltm_synth(x, pitch, coef)
                delay = pitch + ntaps // 2
                assert np.array_equal(y[:delay], x[:delay])
                active += int(delay < n and not np.array_equal(y, x))
            want[ch, pos:pos + n] = y
        pos += n + GAP
    assert pos == stride
    for a in (blocks, info, chan, planes, want):
        a.setflags(write=False)
    name = "taps%d_%s" % (ntaps, "long" if long_blocks else "short")
    return Table(name, ntaps, Cn, blocks, info, chan, planes, want, active, max(r[0] for r in rows))


TABLES = [(t, lb) for t in range(1, 6) for lb in (False, True)]
TABLE_IDS = ["taps%d_%s" % (t, "long" if lb else "short") for t, lb in TABLES]


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def launch(hip, t, max_block_samples):
    import torch
    L = hip.lib()
    d_planes = torch.from_numpy(t.planes.copy()).cuda()
    d_blk = torch.from_numpy(t.blocks.view(np.uint8).copy()).cuda()
    d_info = torch.from_numpy(t.info.view(np.int32).copy()).cuda()
    d_chan = torch.from_numpy(t.chan.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_dec_ltm(C.c_void_p(d_planes.data_ptr()), C.c_uint64(t.planes.shape[1]), C.c_void_p(d_blk.data_ptr()),
                                  C.c_void_p(d_info.data_ptr()), C.c_void_p(d_chan.data_ptr()), C.c_uint32(len(t.blocks)),
                                  C.c_uint32(t.C), C.c_uint32(t.ntaps), C.c_uint32(max_block_samples), None)
    assert rc == 0, (t.name, max_block_samples, rc)
    torch.cuda.synchronize()
    # the tables came through untouched
    assert np.array_equal(d_blk.cpu().numpy(), t.blocks.view(np.uint8)) and np.array_equal(d_chan.cpu().numpy().view(np.uint32), t.chan)
    return d_planes.cpu().numpy()


def explain(t, got):
    """where the first difference lies: the row, its length, the channel's pitch, the sample inside the block or the gap"""
    ch, pos = (int(v) for v in np.argwhere(got != t.want)[0])
    r = int(np.searchsorted(t.blocks["smp_off"], pos, side="right")) - 1
    b = t.blocks[r]
    at = pos - int(b["smp_off"])
    where = "sample %d" % at if at < int(b["num_samples"]) else "the gap behind it, word %d" % (at - int(b["num_samples"]))
    return (t.name, "row", r, "n", int(b["num_samples"]), "type", int(t.info[r, 0]), "flags", int(b["flags"]), "channel", ch,
            "pitch", int(t.chan[r, ch, 0]), where, "got", int(got[ch, pos]), "want", int(t.want[ch, pos]),
            "mismatches", int((got != t.want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("ntaps,long_blocks", TABLES, ids=TABLE_IDS)
def test_launcher_against_the_oracle(hip, ntaps, long_blocks):
    t = table(ntaps, long_blocks)
    assert t.active >= 30 and (t.longest > LDS_SAMPLES) == long_blocks
    assert (t.want != t.planes).any() and (t.want == CANARY).sum() >= GAP * len(t.blocks) * t.C
    if long_blocks:
        got = launch(hip, t, 65535)
        assert np.array_equal(got, t.want), explain(t, got)
        return
    near = launch(hip, t, LDS_SAMPLES)               # today's kernel: the block in LDS
    assert np.array_equal(near, t.want), ("k_dec_ltm",) + explain(t, near)
    far = launch(hip, t, LDS_SAMPLES + 1)            # the ring kernel on the same table
    assert np.array_equal(far, t.want), ("k_dec_ltm_far",) + explain(t, far)
    assert np.array_equal(near, far)


def test_tables_cover_what_they_claim():
    w = window()
    assert w >= 64
    seen_len, seen_pairs, seen_c = set(), set(), set()
    kinds = set()
    for ntaps, lb in TABLES:
        t = table(ntaps, lb)
        seen_c.add(t.C)
        for r in range(len(t.blocks)):
            n, typ, flags = int(t.blocks["num_samples"][r]), int(t.info[r, 0]), int(t.blocks["flags"][r])
            for ch in range(t.C):
                pitch = int(t.chan[r, ch, 0])
                if typ == 0 and flags == 0:
                    seen_pairs.add((pitch, ntaps, n))
                    if pitch == 0:
                        kinds.add("pitch 0")
                    elif pitch + ntaps // 2 >= n:
                        kinds.add("delay >= n")
                elif typ in (1, 2) and pitch:
                    kinds.add("type %d" % typ)
                elif flags and pitch:
                    kinds.add("header only")
            seen_len.add(n)
    assert set(lengths()) <= seen_len and seen_c == {1, 2, 8}
    for p in PITCHES:
        for taps in range(1, 6):
            assert (p, taps, 65535) in seen_pairs and (p, taps, w + 1) in seen_pairs
    for p, taps in PAIRS:
        for n in lengths():
            assert (p, taps, n) in seen_pairs
    assert kinds == {"pitch 0", "delay >= n", "type 1", "type 2", "header only"}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65535, 40897])
def test_per_call_synthesizer_on_long_blocks(hip, n):
    """SLALongTermSynthesizer_SynthesizeInt32 beyond the LDS budget (odd tap counts: the per-call API takes no others)"""
    L = hip.lib()
    L.SLALongTermSynthesizer_Create.restype = C.c_void_p
    L.SLALongTermSynthesizer_Destroy.restype = None
    L.SLALongTermSynthesizer_Destroy.argtypes = [C.c_void_p]
    rng = np.random.default_rng(n)
    h = L.SLALongTermSynthesizer_Create(5, 1023)
    assert h
    try:
        for pitch, taps in [(1023, 5), (1, 5), (2, 5), (64, 3), (1, 3), (257, 1)]:
            for kind in ("small", "full"):
                x, coef = operands(rng, n, taps, kind)
                out = np.zeros(n, np.int32)
                assert L.SLALongTermSynthesizer_Reset(C.c_void_p(h)) == 0
                rc = L.SLALongTermSynthesizer_SynthesizeInt32(C.c_void_p(h), x.ctypes.data_as(i32p), n, pitch, coef.ctypes.data_as(i32p),
                                                              taps, out.ctypes.data_as(i32p))
                assert rc == 0, (pitch, taps, kind)
                want = LB.ltm_synth(x, pitch, coef)
                assert np.array_equal(out, want), (pitch, taps, kind, int(np.argmax(out != want)))
    finally:
        L.SLALongTermSynthesizer_Destroy(C.c_void_p(h))
