"""No GPU: the exactness limit of the long-block tile-sum search on the twelve inputs its GPU tests encode
(tests/longenccases.py, tests/longsearchcases.py), by the integer model of tests/longsearchmodel.py -- the claims that
tests/test_gpu_long_tile_search.py takes its expected rerun counts from:

    * at exact_bits 53 every (super-frame, channel) group of the seven 16-bit cases lies under the limit and every group of
      the three 24-bit cases of longenccases lies at or over it;
    * the quiet 24-bit file lies under it throughout, the mixed one has both kinds: its first super-frame's channels under,
      its second's over;
    * the model's super-frames are the oracle's: every one starts and ends on a block boundary of the oracle's stream and
      holds no SILENT block of a hop;
    * the candidate grid of a 65535-sample window has 2015 entries, all on tile boundaries."""
import numpy as np
import pytest

import longenccases as E
import longsearchcases as Q
import longsearchmodel as M


def all_inputs():
    return list(E._inputs()) + list(Q.inputs())


def test_there_are_twelve_cases_with_the_names_the_gpu_tests_use():
    names = [c.name for c in all_inputs()]
    assert tuple(names) == E.NAMES + Q.NAMES and len(names) == 12


@pytest.mark.parametrize("index", range(12))
def test_the_split_at_exact_bits_53(index):
    c = all_inputs()[index]
    over, groups = M.flagged(c.pcm, c.max_block, c.ms)
    assert groups >= c.num_channels
    if c.bits == 16:
        assert over == 0, c.name
    elif c.name in E.NAMES:
        assert over == groups, c.name                     # 24 bits at ordinary loudness: every group reruns
    elif c.name == "stereo24_ms_quiet_70000_max65535":
        assert over == 0 and groups == 4
    else:
        e = M.group_energies(c.pcm, c.max_block, c.ms)
        assert [(g[0], g[1], g[2]) for g in e] == [(0, 65535, 0), (0, 65535, 1), (65535, 20000, 0), (65535, 20000, 1)]
        assert [g[3] >= 1 << 53 for g in e] == [False, False, True, True]      # really mixed
    if c.bits == 24:
        assert M.ntz_of(c.pcm) == 8, c.name               # the low bits are alive: the unit is 2^-23


def test_sixteen_bit_material_cannot_be_flagged():
    """|x| < 2 in the search's unit, so 4 x the window bounds the energy: under 2^53 units^2 at 16 bits for any window"""
    for ms in (0, 1):
        unit_log2 = 16 - 31 - ms                           # ntz = 16
        assert 4 * 65535 < 2 ** (53 + 2 * unit_log2)


def test_exact_bits_1_flags_every_group_of_a_16_bit_case():
    c = all_inputs()[0]
    over, groups = M.flagged(c.pcm, c.max_block, c.ms, exact_bits=1)
    assert over == groups == 6


@pytest.mark.parametrize("index", range(12))
def test_super_frames_are_the_oracles(index):
    c = (list(E.cases()) + list(Q.cases()))[index]
    edges, silent = set(), []
    for s, (n, t) in zip(c.trace.blk_start[:c.trace.num_blocks], c.blocks()):
        edges.add(int(s))
        edges.add(int(s) + n)
        if t == E.SILENT:
            silent.append((int(s), n))
    frames = M.super_frames(c.pcm, c.max_block)
    covered = sum(w for _, w in frames)
    hopped = 0
    for s, n in silent:
        inside = any(f <= s and s + n <= f + w for f, w in frames)
        hopped += 0 if inside else n
    assert covered + hopped == c.num_samples, c.name
    for f, w in frames:
        assert f in edges and f + w in edges, (c.name, f, w)


def test_the_candidate_grid_of_65535():
    g = M.grid(65535)
    assert len(g) == 2015 and len(set(g)) == 2015
    for s, n in g:
        assert s % 1024 == 0 and (s + n == 65535 or (s + n) % 1024 == 0) and n >= 2048
    assert len(M.grid(16385)) == 135
