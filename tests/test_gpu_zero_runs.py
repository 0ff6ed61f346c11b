"""sla_hip_launch_zero_runs alone, on crafted masks, against the numpy model of the run list (tests/zerorunmodel.py).

T = SLA_HIP_ZERO_RUN_TILE x 64 samples is what one workgroup scans; every span stays below 4 T.  The cases sit where the
kernels change behaviour: word boundaries (64 samples), the groups of one wave-wide load, tile boundaries, the scan across
all-zero tiles, segment boundaries on 1024-sample multiples with ragged ends, the end of the mask inside a word, and a list
that is too short."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import zerorunmodel as Z

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
TILE_WORDS = int(re.search(r"#define\s+SLA_HIP_ZERO_RUN_TILE\s+(\d+)", _HEADER).group(1))
T = TILE_WORDS * 64
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _scratch_bytes(span):
    """SLA_HIP_ZERO_RUN_SCRATCH_BYTES of the header"""
    tiles = ((span + 63) // 64 + TILE_WORDS - 1) // TILE_WORDS
    return 4 * (TILE_WORDS // 128 + 1) * (tiles + 1)


def _launch(hip, bits, span=None, segments=None, min_run=2048, capacity=64):
    """(count, sorted entries the device wrote -- at most `capacity` --, the words behind the list)"""
    import torch
    span = len(bits) if span is None else span
    words = Z.mask_words(bits, span)
    d_mask = torch.from_numpy(words.view(np.int64)).cuda()
    d_runs = torch.full((2 * (capacity + 8),), CANARY, dtype=torch.int32, device="cuda")
    d_count = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    d_scratch = torch.full((_scratch_bytes(span) // 4,), -1, dtype=torch.int32, device="cuda")    # (nothing may rely on zeros)
    d_start = d_len = None
    nsegs = 0
    if segments is not None:
        d_start = torch.tensor([s for s, _ in segments], dtype=torch.int64).to(torch.int32).cuda()
        d_len = torch.tensor([n for _, n in segments], dtype=torch.int64).to(torch.int32).cuda()
        nsegs = len(segments)
    torch.cuda.synchronize()
    rc = hip.lib().sla_hip_launch_zero_runs(
        C.c_void_p(d_mask.data_ptr()), span, C.c_void_p(d_start.data_ptr()) if nsegs else None,
        C.c_void_p(d_len.data_ptr()) if nsegs else None, nsegs, min_run, C.c_void_p(d_runs.data_ptr()), capacity,
        C.c_void_p(d_count.data_ptr()), C.c_void_p(d_scratch.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    count = int(d_count.cpu().numpy().view(np.uint32)[0])
    flat = d_runs.cpu().numpy().view(np.uint32)
    kept = min(count, capacity)
    entries = sorted((int(flat[2 * i]), int(flat[2 * i + 1])) for i in range(kept))
    return count, entries, flat[2 * capacity:]


def _check(hip, bits, span=None, segments=None, min_run=2048):
    span = len(bits) if span is None else span
    want = Z.zero_runs(np.asarray(bits, bool)[:span], segments, min_run)
    count, got, behind = _launch(hip, bits, span, segments, min_run)
    assert count == len(want), (count, want, got)
    assert got == want
    assert (behind == CANARY).all()
    return want


def _ones(n):
    return np.ones(n, bool)


def test_all_ones_and_all_zeros(hip):
    assert _check(hip, _ones(2 * T + 777)) == []
    n = 2 * T + 777
    assert _check(hip, np.zeros(n, bool)) == [(0, n)]
    assert _check(hip, np.zeros(64, bool)) == [(0, 64)]


@pytest.mark.parametrize("min_run", [2048, 64, 4096])
def test_runs_around_min_run_and_word_boundaries(hip, min_run):
    """runs of min_run - 1, min_run, min_run + 1 that start and end on word boundaries and one sample to either side"""
    for length in (min_run - 1, min_run, min_run + 1):
        for start_off in (-1, 0, 1):
            for end_on_word in (False, True):
                bits = _ones(T + 3 * min_run + 500)
                start = 64 * 37 + start_off
                if end_on_word:                                 # the END on (or next to) a word boundary instead
                    start = 64 * 300 + start_off - length
                bits[start:start + length] = False
                want = _check(hip, bits, min_run=min_run)
                assert want == ([(start, length)] if length >= min_run else [])


def test_run_across_a_tile_boundary(hip):
    bits = _ones(2 * T + 100)
    bits[T - 1500:T + 1500] = False
    assert _check(hip, bits) == [(T - 1500, 3000)]
    bits = _ones(2 * T + 100)
    bits[T - 2048:T] = False                                    # ends exactly with the tile: the next tile's first bit ends it
    assert _check(hip, bits) == [(T - 2048, 2048)]
    bits = _ones(2 * T + 100)
    bits[T:T + 2048] = False                                    # starts exactly with a tile
    assert _check(hip, bits) == [(T, 2048)]


def test_run_over_two_whole_tiles(hip):
    """the cross-tile scan: the run's start is two all-zero tiles in front of the word that ends it"""
    bits = _ones(3 * T + 5000)
    bits[T - 700:3 * T + 1234] = False
    assert _check(hip, bits) == [(T - 700, 2 * T + 1934)]
    bits = _ones(3 * T + 64 * 200)
    bits[5:3 * T + 64 * 130 + 5] = False                        # ... and all-zero groups of the last tile in front of it
    assert _check(hip, bits) == [(5, 3 * T + 64 * 130)]


def test_short_spans(hip):
    for span in (1, 17, 63):                                    # shorter than one word
        assert _check(hip, np.zeros(span, bool), min_run=64) == [(0, span)]
        assert _check(hip, _ones(span), min_run=64) == []
        bits = _ones(span)
        bits[span - 1] = False
        assert _check(hip, bits, min_run=64) == [(span - 1, 1)]
    for span in (65, 64 * 128 + 1, T + 64 * 129 - 7, 2 * T - 63):       # not a multiple of 64; a lone word behind a group / a tile
        bits = _ones(span)
        bits[span - 30:] = False
        bits[3:3 + min(2100, span // 2)] = False
        _check(hip, bits)
        assert _check(hip, np.zeros(span, bool)) == [(0, span)]


def test_a_64_sample_run_without_an_all_zero_word(hip):
    bits = _ones(T + 999)
    bits[64 * 50 + 31:64 * 51 + 31] = False                     # straddles two words
    bits[64 * 70 + 1:64 * 71] = False                           # 63 zeros inside one word: not a run of 64
    bits[T - 32:T + 32] = False                                 # ... and across the tile boundary
    assert _check(hip, bits, min_run=64) == [(64 * 50 + 31, 64), (T - 32, 64)]


def test_tail_runs(hip):
    bits = _ones(T + 4321)
    bits[-1] = False
    assert _check(hip, bits) == [(T + 4320, 1)]
    bits = _ones(2 * T + 4321)
    bits[9000:9000 + 30000] = False
    bits[-777:] = False
    assert _check(hip, bits) == [(9000, 30000), (2 * T + 4321 - 777, 777)]
    bits = _ones(2 * T + 64)                                    # a tail that reaches back over a whole tile
    bits[T - 5:] = False
    assert _check(hip, bits) == [(T - 5, T + 69)]


def test_segments(hip):
    """five files on 1024-sample multiples with ragged ends; file 1's zero tail meets file 2's zero head across the gap:
    two runs -- the tail whatever its length, the head only when it reaches min_run; a file that ends inside a word; an empty
    file; gaps are zero in the mask and belong to nobody"""
    lens = [5000, 3 * 1024 - 100, 70000, 0, 1024 * 5 + 33]
    starts, pos = [], 0
    for n in lens:
        starts.append(pos)
        pos += -(-n // 1024) * 1024
    span = pos
    assert span < 4 * T
    for head in (2047, 2048, 5000):
        bits = np.zeros(span, bool)
        for s, n in zip(starts, lens):
            bits[s:s + n] = True                                # (the gaps stay zero)
        bits[starts[0] + 1000:starts[0] + 1000 + 2500] = False              # a plain run inside file 0
        bits[starts[1] + lens[1] - 40:starts[1] + lens[1]] = False          # file 1: 40 zeros at its end ...
        bits[starts[2]:starts[2] + head] = False                            # ... file 2 begins with `head` zeros
        bits[starts[2] + lens[2] - 3000:starts[2] + lens[2]] = False        # and ends with 3000, inside a word
        bits[starts[4] + 10:starts[4] + 10 + 2048] = False
        segments = list(zip(starts, lens))
        want = _check(hip, bits, span, segments)
        assert (starts[1] + lens[1] - 40, 40) in want
        assert ((starts[2], head) in want) == (head >= 2048)
        assert (starts[2] + lens[2] - 3000, 3000) in want
        assert len(want) == (4 if head < 2048 else 5)
    # every file all zero: one run each, the empty one none; the model and the device agree on the order-free set
    bits = np.zeros(span, bool)
    assert _check(hip, bits, span, list(zip(starts, lens))) == [(s, n) for s, n in zip(starts, lens) if n]
    # one segment that is the whole mask, given as a table
    bits = _ones(T + 5)
    bits[100:3000] = False
    assert _check(hip, bits, None, [(0, T + 5)]) == [(100, 2900)]


def test_capacity_too_small(hip):
    bits = _ones(T + 20000)
    want = []
    for k in range(5):
        at = 3000 + k * 13001
        bits[at:at + 2048 + k] = False
        want.append((at, 2048 + k))
    count, got, behind = _launch(hip, bits, capacity=2)
    assert count == 5
    assert (behind == CANARY).all()                             # nothing at or behind d_runs[2]
    count, got, behind = _launch(hip, bits, capacity=5)
    assert count == 5 and got == want and (behind == CANARY).all()
