"""The inputs of tests/longenccases.py on the CPU: the coverage the GPU tests of the long-block encoder rely on, and the host
planner (slai_code_length, slai_shortest_path through tests/planmodel.py) at 18, 33 and 65 nodes against the oracle's
partitions of these inputs -- the long-block routes plan on the host, and the existing planner tests stop at 17 nodes."""
import ctypes as C
import os

import numpy as np
import pytest

import longenccases as E
import planmodel as P
import sla_amd

f64p, u32p = sla_amd.f64p, sla_amd.u32p


def test_names_match():
    assert tuple(c.name for c in E.cases()) == E.NAMES


def test_every_case_has_a_long_block_and_a_bounded_cost():
    for c in E.cases():
        assert max(n for n, _ in c.blocks()) > 16384, c.name
        assert sum(n for n, _ in c.blocks()) == c.num_samples, c.name
        assert c.num_samples <= 150000 and (c.order <= 16 or (c.order == 32 and c.num_samples <= c.max_block)), c.name
        assert 16384 < c.max_block <= 65535


def test_block_lengths_and_types():
    b = {c.name: c.blocks() for c in E.cases()}
    assert b["stereo16_ms_140000_max65535"] == [(65535, E.COMPRESS), (65535, E.COMPRESS), (8930, E.COMPRESS)]
    assert b["stereo16_ms_70000_max32768"] == [(32768, E.COMPRESS), (32768, E.COMPRESS), (4464, E.COMPRESS)]
    assert b["mono24_order32_65535_max65535"] == [(65535, E.COMPRESS)]
    assert b["stereo24_16385_max16385"] == [(16385, E.COMPRESS)]
    assert b["mono16_18432_max16385"] == [(16385, E.COMPRESS), (2047, E.COMPRESS)]
    assert b["stereo16_ms_34816_max32768"] == [(32768, E.COMPRESS), (2048, E.COMPRESS)]
    assert b["eight16_22048_max20000"] == [(20000, E.COMPRESS), (2048, E.COMPRESS)]


def test_the_split_super_frame():
    """one 65535-sample super-frame whose character changes inside it: unequal parts, one of them over 16384"""
    parts = [n for n, t in E.by_name()["mono16_changing_65535_max65535"].blocks()]
    assert sum(parts) == 65535 and len(parts) >= 2 and len(set(parts)) == len(parts) and max(parts) > 16384
    assert all(t == E.COMPRESS for _, t in E.by_name()["mono16_changing_65535_max65535"].blocks())


def test_raw_and_silent_blocks_over_16384():
    assert E.by_name()["mono16_white_19999_max20000"].blocks() == [(19999, E.RAW)]
    sil = E.by_name()["mono24_silence_115000_max65535"].blocks()
    assert any(t == E.SILENT and n > 16384 for n, t in sil) and sil[-1][1] == E.SILENT
    assert any(t == E.COMPRESS and n > 16384 for n, t in sil)


def test_boundaries_and_formats():
    cs = E.cases()
    assert {16385, 20000, 32768, 65535} <= {c.max_block for c in cs}
    rel = {(c.num_samples - c.max_block) for c in cs}
    assert {-1, 0, 2047, 2048} <= rel
    assert {1, 2, 8} <= {c.num_channels for c in cs} and {16, 24} <= {c.bits for c in cs} and {1, 3, 5} <= {c.ltm for c in cs}
    assert any(c.ms for c in cs) and any(c.order == 32 for c in cs)
    assert all(c.ms == 0 or c.num_channels == 2 for c in cs)


# ---- the host planner at 18, 33 and 65 nodes -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    lib = sla_amd.lib()
    lib.slai_code_length.restype = C.c_double
    lib.slai_code_length.argtypes = [C.c_double, C.c_uint32, C.c_uint32, f64p, C.c_uint32]
    return lib


def first_super_frame_table(oracle, case):
    """the slots the search leaves for the case's first super-frame: per channel (after mid/side) and candidate of the
    encoder's grid { r0, parcor[0..order] } from the oracle's own autocorrelation and recursion"""
    window = min(case.max_block, case.num_samples)
    x = case.pcm[:, :window].astype(np.float64) * 2.0 ** -31
    if case.ms:
        x = np.stack([(x[0] + x[1]) / 2, x[0] - x[1]])
    cands = [(s, n) for s, n in P.full_lattice(window) if n >= min(2048, window)]
    slots = np.zeros((case.num_channels, len(cands), case.order + 2))
    for ch in range(case.num_channels):
        for k, (s, n) in enumerate(cands):
            xs = np.ascontiguousarray(x[ch, s:s + n])
            slots[ch, k, 0] = oracle.autocorr(xs, 1)[0]
            ret, slots[ch, k, 1:] = oracle.parcor(xs, case.order)
            assert ret == 0
    return P.Table(window, case.num_channels, case.order, case.bits, cands, slots), window


@pytest.mark.parametrize("name,nodes", [("mono16_18432_max16385", 18), ("stereo16_ms_34816_max32768", 33),
                                        ("mono16_changing_65535_max65535", 65)])
def test_host_planner_decides_the_oracles_partition(L, oracle, name, nodes):
    case = E.by_name()[name]
    t, window = first_super_frame_table(oracle, case)
    assert t.nodes == nodes
    # the oracle's partition of the first super-frame
    want, acc = [], 0
    for n, _ in case.blocks():
        want.append(n)
        acc += n
        if acc == window:
            break
    assert acc == window
    # code lengths: the model and the product's host function, bit for bit, on every slot
    for ch in range(t.nch):
        for k, (_, n) in enumerate(t.cands):
            s = np.ascontiguousarray(t.slots[ch, k])
            m = P.code_length(float(s[0]), n, t.bps, s[1:].tolist(), t.order)
            h = L.slai_code_length(float(s[0]), n, t.bps, s[1:].ctypes.data_as(f64p), t.order)
            assert m.hex() == h.hex(), (name, ch, k)
    # the shortest path: model, product and the oracle's partition
    adj = P.host_adjacency(t)
    ret, path = P.dijkstra(adj, t.nodes)
    a = np.ascontiguousarray(np.array(adj, np.float64))
    got = np.zeros(t.nodes, np.uint32)
    assert L.slai_shortest_path(a.ctypes.data_as(f64p), t.nodes, got.ctypes.data_as(u32p)) == 0 and ret == 0
    assert got.tolist() == path
    assert P.back_walk(path, t.nodes, window) == want
