"""Streams with blocks of more than 16384 samples (tests/longblockcases.py), on the CPU.

The block length is a 16-bit field: blocks of up to 65535 samples are legal, and the reference's library writes them as soon
as a caller asks for max_num_block_samples above its CLI's 16384.  The yardstick of the HIP decoder on such streams
(tests/test_gpu_long_blocks.py, tests/test_gpu_dec_ltm_far.py) is the oracle's decoder with capacity (8, 65535, 255, 5, 32)
and its ltm_synth.  Here the oracle is pinned to the unmodified reference on every file whose pitches the reference defines
(tests/test_crafted_streams.py, 'Left out'), the files' claimed coverage is asserted from their bytes, the oracle's
long-term synthesis is held against the formula where taps reach at or past the current sample, and the chunk length the
windowed kernel exports is checked for sanity.
"""
import os
import re

import numpy as np
import pytest

import indexmodel as IM
import longblockcases as LB
import sla_amd
import slalibs as S
import slastream as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = LB.cases()
IDS = [c.name for c in CASES]
EXCEED_HANDLE_CAPACITY = 3


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def test_the_set_covers_what_it_claims():
    by = LB.by_name()
    mono = by["mono_16bit_65535_2048raw_40897_3000silent_16385"]
    assert mono.block_lengths == (65535, 2048, 40897, 3000, 16385) and mono.pitches == (1, 1023) and not mono.ref_defined
    assert [b.type for b in mono.blocks] == [SS.COMPRESS, SS.RAW, SS.COMPRESS, SS.SILENT, SS.COMPRESS]
    assert mono.blocks[0].chans[0].ltm[0] == 1023 and mono.blocks[2].chans[0].ltm[0] == 1 and mono.blocks[4].chans[0].ltm is None
    assert by["stereo_24bit_ms_40000_50000"].block_lengths == (40000, 50000)
    assert by["eight_channels_20000"].block_lengths == (20000,) and by["eight_channels_20000"].num_channels == 8
    assert by["encoded_140000_max65535"].block_lengths == (65535, 65535, 8930)
    assert by["encoded_70000_max32768"].block_lengths == (32768, 32768, 4464)
    # every file but the first stays inside the reference's ring buffer, and each of them has long-term channels
    assert [c.ref_defined for c in CASES] == [False, True, True, True, True]
    assert all(c.ltm_channels >= 2 and len(c.pitches) == c.ltm_channels for c in CASES)
    assert by["stereo_24bit_ms_40000_50000"].pitches == (3, 100, 258)
    assert by["eight_channels_20000"].pitches == (3, 64, 77, 200, 259)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_block_lengths_and_header(case):
    assert LB.block_lengths(case.data) == case.block_lengths and sum(case.block_lengths) == case.num_samples
    assert max(case.block_lengths) > 16384
    assert int.from_bytes(case.data[33:35], "big") >= max(case.block_lengths)        # the header's max_num_block_samples
    assert case.data[14] == case.num_channels


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_decodes_and_a_16384_handle_refuses(oracle, case):
    rc, pcm = LB.oracle_decoded(case.name)
    assert rc == 0 and pcm.shape == (case.num_channels, case.num_samples)
    assert LB.expected(case.name)[0] == 0 and LB.expected(case.name)[1].shape == pcm.shape
    assert oracle.decode_whole(S.make_params(cap=(8, 16384, 255, 5, 32)), case.data, case.num_samples)[0] == EXCEED_HANDLE_CAPACITY


@pytest.mark.parametrize("case", [c for c in CASES if c.ref_defined], ids=[c.name for c in CASES if c.ref_defined])
def test_oracle_equals_the_reference(ref, case):
    assert LB.undefined_in_the_oracle_decoder(case) == []
    ro, do = LB.oracle_decoded(case.name)
    assert np.array_equal(do, LB.expected(case.name)[1])
    rr, dr, _ = ref.decode_whole(S.make_params(cap=LB.CAP), case.data, case.num_samples)
    assert ro == rr == 0
    assert do.shape == dr.shape and np.array_equal(do, dr)


def test_encoded_pitches_match_the_traced_flags(oracle):
    """the oracle-encoded files: the long-term channels counted from the trace are compressed-block channels with a pitch
    of at least 3 (what its analysis picks), and there are some in the 65535-sample blocks"""
    for name in ("encoded_140000_max65535", "encoded_70000_max32768"):
        c = LB.by_name()[name]
        assert c.ltm_channels >= 4 and min(c.pitches) >= 3 and max(c.pitches) <= 259


@pytest.mark.parametrize("case", [c for c in CASES if c.blocks is not None], ids=[c.name for c in CASES if c.blocks is not None])
def test_crafted_files_decode_to_the_synthesis_chain(case):
    """the yardstick of the crafted files (LB.expected) is the oracle's unit functions on the writer's fields; the oracle's
    decoder gives the same samples everywhere but at the last sample of a block channel with 5 taps at pitch 1, where it
    reads a word behind the block that the kernels define as 0 (LB.undefined_in_the_oracle_decoder)"""
    rc, dec = LB.oracle_decoded(case.name)
    chain = LB.expected(case.name)[1]
    free = LB.undefined_in_the_oracle_decoder(case)
    differ = [(int(c), int(s)) for c, s in np.argwhere(dec != chain)]
    assert rc == 0 and set(differ) <= set(free), differ[:4]
    if case.name.startswith("mono"):
        assert free == [(0, 65535 + 2048 + 40897 - 1)]
    else:
        assert free == []


def test_only_five_taps_at_pitch_one_reach_behind_the_block():
    assert [(t, p) for t in range(1, 6) for p in range(1, 1024) if LB.reads_past_the_block(t, p)] == [(5, 1)]


def formula(x, pitch, coef):
    """out[s] = in[s] + ((2^30 + sum_k coef[k] * out[s - delay + k]) >> 31) for s >= delay = pitch + taps / 2, in place:
    a tap at or past s reads input not yet synthesised, a tap at or past n reads 0; the add wraps"""
    out = [int(v) for v in x]
    n, taps = len(out), len(coef)
    delay = pitch + taps // 2
    for s in range(delay, n):
        acc = 1 << 30
        for k in range(taps):
            at = s - delay + k
            acc += int(coef[k]) * (out[at] if at < n else 0)
        v = (out[s] + (acc >> 31)) & SS.M32
        out[s] = v - (1 << 32) if v >> 31 else v
    return np.array(out, np.int64).astype(np.int32)


@pytest.mark.parametrize("pitch,taps", [(1, 5), (2, 5), (1, 4), (1, 3), (1, 1), (3, 5), (64, 3), (1023, 5)])
def test_oracle_ltm_synth_is_the_formula(oracle, pitch, taps):
    rng = np.random.default_rng(pitch * 8 + taps)
    for n in (7, 1500):
        for full in (False, True):
            if full:
                x = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
                coef = np.array([-2 ** 31 if k & 1 else 0x7FFF0000 for k in range(taps)], np.int64).astype(np.int32)
            else:
                x = rng.integers(-1000, 1000, n).astype(np.int32)
                coef = (rng.integers(-12000, 12000, taps).astype(np.int64) << 16).astype(np.int32)
            want = formula(x, pitch, coef)
            assert np.array_equal(LB.ltm_synth(x, pitch, coef), want), (pitch, taps, n, full)
            if not LB.reads_past_the_block(taps, pitch):             # then slalibs' plain call stays inside its arrays
                assert np.array_equal(oracle.ltm_synth(x, pitch, coef), want), (pitch, taps, n, full)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_index_rows(case):
    """sla_hip_index_build has no cap on the block length: its rows are the model's"""
    want = IM.index_of(case.data)
    x = sla_amd.Index.build(case.data)
    try:
        rows = [(int(r["byte_off"]), int(r["byte_len"]), int(r["smp_off"]), int(r["num_samples"])) for r in x.blocks()]
        assert rows == want.rows and x.stop == want.stop == 0 and x.extent == want.extent == case.num_samples
        assert tuple(r[3] for r in rows) == case.block_lengths
    finally:
        x.close()


def test_window_function_is_exported_and_sane(L):
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    assert re.search(r"\bsla_hip_dec_ltm_window\s*\(", text)
    assert "sla_hip_dec_ltm_window" in sla_amd.EXPORTED_SYMBOLS and hasattr(L, "sla_hip_dec_ltm_window")
    w = int(L.sla_hip_dec_ltm_window())
    assert 64 <= w <= 65535                          # a step of up to 64 outputs fits a chunk; chunks are no longer than a block
    assert w == int(L.sla_hip_dec_ltm_window())      # a constant
