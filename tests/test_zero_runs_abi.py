"""Checks of the silence run list (option "silence_runs", include/sla_hip.h) that need no kernel: the header's entry points,
the exported symbols, the launcher's refusals (which come before any device work), and the fact the feature rests on -- the
super-frame hop gets the same answers from the run list as from the mask -- through the product's own host code
(sla_hip_shard_bounds walks the hop; slai_runs_zero_run is the encoder's lookup).  Only the option check needs a handle,
and a handle needs a device: that one test is marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd
import zerorunmodel as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_launch_zero_runs", "sla_hip_last_silence")
RUN_LENGTHS = (1, 63, 64, 100, 1023, 2047, 2048, 2049, 3000, 5000, 20000)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


class ZeroRun(C.Structure):                                     # sla_hip_zero_run
    _fields_ = [("start", C.c_uint32), ("length", C.c_uint32)]


def _define(text, name):
    m = re.search(r"#define\s+%s\s+(0[xX][0-9a-fA-F]+|\d+)u?\b" % name, text)
    assert m, name
    return int(m.group(1), 0)


def test_header_declares_the_run_list():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    assert re.search(r"typedef struct sla_hip_zero_run\s*\{\s*uint32_t start;\s*uint32_t length;\s*\}\s*sla_hip_zero_run;", text)
    assert _define(text, "SLA_HIP_ZERO_RUN_MIN") == 2048
    tile = _define(text, "SLA_HIP_ZERO_RUN_TILE")
    assert tile >= 64 and tile % 2 == 0
    assert "SLA_HIP_ZERO_RUN_SCRATCH_BYTES" in text              # the scratch formula is stated
    assert '"silence_runs"' in text                             # the option is documented with the others
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "silence_runs" in open(os.path.join(ROOT, doc)).read(), doc


def test_symbols_are_exported(L):
    for name in NAMES:
        assert hasattr(L, name), name
    assert hasattr(sla_amd.Encoder, "last_silence")
    assert C.sizeof(ZeroRun) == 8


def test_launcher_refuses_before_any_device_work(L):
    # dangling, suitably aligned values: nothing behind them is touched when an argument is refused
    mask, runs, count, scratch, table = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))

    def launch(mask=mask, span=100000, seg_start=None, seg_len=None, nsegs=0, min_run=2048, runs=runs, cap=16, count=count,
               scratch=scratch):
        return L.sla_hip_launch_zero_runs(mask, span, seg_start, seg_len, nsegs, min_run, runs, cap, count, scratch, None)

    assert launch(mask=None) == INVALID_ARGUMENT
    assert launch(runs=None) == INVALID_ARGUMENT
    assert launch(count=None) == INVALID_ARGUMENT
    assert launch(scratch=None) == INVALID_ARGUMENT
    assert launch(cap=0) == INVALID_ARGUMENT
    assert launch(min_run=63) == INVALID_ARGUMENT
    assert launch(min_run=0) == INVALID_ARGUMENT
    assert launch(seg_start=table, seg_len=table, nsegs=0) == INVALID_ARGUMENT
    assert launch(seg_start=table, seg_len=None, nsegs=3) == INVALID_ARGUMENT
    assert launch(mask=C.c_void_p(0x1008)) == INVALID_ARGUMENT   # 16-byte loads
    assert launch(span=0xFFFFFFFF) == INVALID_ARGUMENT
    c = (C.c_uint32 * 4)(*([7] * 4))
    assert L.sla_hip_last_silence(None, c) == INVALID_ARGUMENT
    assert L.sla_hip_last_silence(C.c_void_p(0x10), None) == INVALID_ARGUMENT
    assert list(c) == [7] * 4


@pytest.mark.gpu
def test_option_range():
    import torch
    torch.cuda.init()
    enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
    try:
        for v in (0, 1, 65536):
            enc.set_option("silence_runs", v)
        for v in (-1, 65537, 1.5):
            with pytest.raises(sla_amd.SlaError):
                enc.set_option("silence_runs", v)
        assert enc.last_silence() == (0, 0, 0, 0)
    finally:
        enc.close()


# ---- the equivalence, through the product's host code --------------------------------------------------------------

def _random_file(rng):
    """(bits, n): a file of 1..60000 samples with zero runs of the listed lengths at random offsets, sometimes a zero tail,
    sometimes nothing but zeros"""
    n = int(rng.integers(1, 60001))
    bits = np.ones(n, bool)
    kind = int(rng.integers(0, 12))
    if kind == 0:
        bits[:] = False
        return bits, n
    for _ in range(int(rng.integers(0, 7))):
        ln = int(rng.choice(RUN_LENGTHS))
        at = int(rng.integers(0, n))
        bits[at:at + ln] = False
    if kind <= 4:
        bits[n - min(n, int(rng.integers(1, 4001))):] = False
    return bits, n


def _files(count, seed):
    rng = np.random.default_rng(seed)
    return [_random_file(rng) for _ in range(count)]


def test_the_hop_is_the_same_on_the_mask_and_on_the_run_list(L):
    """every super-frame start of the hop (sla_hip_shard_bounds with targets closer than any two starts) is the same on the
    true mask and on the mask someone rebuilds from the run list alone, at all three maximum block lengths"""
    seen_moved = 0
    for bits, n in _files(120, 2024):
        runs = Z.zero_runs(bits, None, 2048)
        true_mask = Z.mask_words(bits)
        from_runs = Z.mask_words(Z.rebuilt_bits(runs, n))
        for maxb in (4096, 8192, 16384):
            world = min(n, 2000)                               # targets at most 30 samples apart: every start of the hop comes back
            a = sla_amd.shard_bounds(n, maxb, true_mask, world)
            b = sla_amd.shard_bounds(n, maxb, from_runs, world)
            assert a == b, (n, maxb, runs)
            seen_moved += a != sla_amd.shard_bounds(n, maxb, None, world)
    assert seen_moved > 0                                       # (the inputs are not all files whose silence leaves the grid alone)


def _lookup(L):
    L.slai_runs_zero_run.restype = C.c_uint32
    L.slai_runs_zero_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]
    L.slai_zero_run.restype = C.c_uint32
    L.slai_zero_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.slai_sort_runs.restype = None
    L.slai_sort_runs.argtypes = [C.c_void_p, C.c_uint32]


def test_the_encoders_lookup_answers_as_the_rebuilt_mask(L):
    """slai_runs_zero_run (binary search in the sorted list) against slai_zero_run on the mask rebuilt from the list, and --
    where it decides something -- against the true mask: hop questions at every 1024-sample position, block questions for
    every admissible block of the search grid"""
    _lookup(L)
    rng = np.random.default_rng(7)
    for bits, n in _files(60, 99):
        runs = Z.zero_runs(bits, None, 2048)
        arr = (ZeroRun * max(len(runs), 1))()
        for i, k in enumerate(rng.permutation(len(runs))):      # the device's order is unspecified: the host sorts
            arr[i].start, arr[i].length = runs[k]
        L.slai_sort_runs(arr, len(runs))
        assert [(arr[i].start, arr[i].length) for i in range(len(runs))] == runs
        rebuilt = Z.mask_words(Z.rebuilt_bits(runs, n))
        true_mask = Z.mask_words(bits)
        probes = list(range(0, n, 1024)) + [int(x) for x in rng.integers(0, n, 40)] + [a for a, _ in runs] + [a + ln - 1 for a, ln in runs]
        for pos in probes:
            remain = n - pos
            for limit in {min(4096, remain), min(16384, remain), min(2048, remain), 1}:
                got = L.slai_runs_zero_run(arr, len(runs), pos, limit)
                assert got == L.slai_zero_run(rebuilt.ctypes.data, pos, limit), (n, pos, limit, runs)
                min_blk = min(2048, remain)
                if limit >= min_blk:                           # a decision of the hop or of the block test
                    true = L.slai_zero_run(true_mask.ctypes.data, pos, limit)
                    assert (got >= min_blk) == (true >= min_blk) and (got == limit) == (true == limit), (n, pos, limit)
                    if got >= min_blk:
                        assert got == true
    assert L.slai_runs_zero_run(None, 0, 5, 100) == 0
