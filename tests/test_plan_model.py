"""The device-free model of the partition planner (tests/planmodel.py) against the product's host code and the oracle:
the code length bit for bit (slai_code_length, oracle.code_length), Dijkstra predecessor for predecessor
(slai_shortest_path, oracle.dijkstra), the decision gap on hand-made tables, the drop rate of the separated-table
generator that tests/test_gpu_plan.py draws from, and the refusals of the launchers tested there and in
tests/test_gpu_prepass.py (they come before any device work)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import planmodel as P
import sla_amd

f64p, u32p = sla_amd.f64p, sla_amd.u32p
INVALID_ARGUMENT = 2
D = P.D


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    lib = sla_amd.lib()
    lib.slai_code_length.restype = C.c_double
    lib.slai_code_length.argtypes = [C.c_double, C.c_uint32, C.c_uint32, f64p, C.c_uint32]
    return lib


def ptr(a, t):
    return a.ctypes.data_as(t)


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a.hex() == b.hex()


def three_ways(L, oracle, x, bits, par):
    """(model, slai_code_length, oracle.code_length) for the samples x, whose energy is summed as the oracle sums it"""
    r0 = 0.0
    for v in x.tolist():
        r0 += v * v
    order = len(par) - 1
    model = P.code_length(r0, len(x), bits, par.tolist(), order)
    host = L.slai_code_length(r0, len(x), bits, ptr(par, f64p), order)
    return model, host, oracle.code_length(x, bits, par), r0


def test_code_length_random_operands(L, oracle):
    rng = np.random.default_rng(5)
    for order in (1, 5, 8, 9, 16, 17, 32, 48):
        for bits in (8, 16, 24, 32):
            for _ in range(12):
                n = int(rng.integers(1, 200))
                x = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -0.5)
                par = np.zeros(order + 1)
                par[1:] = rng.uniform(-0.999, 0.999, order) * 0.9 ** np.arange(order)
                par[0] = rng.standard_normal()                   # never read
                m, h, o, _ = three_ways(L, oracle, x, bits, par)
                assert same(m, h) and same(m, o), (order, bits, m, h, o)
                assert m > 0


def _x_with_length(bits, par, target):
    """one sample x whose code length before the clamp is as close to `target` as a double allows (bisection in the
    high-precision model over the doubles)"""
    order = len(par) - 1

    def raw(xb):
        x = float(np.array(xb, np.int64).view(np.float64))
        kind, v = P.hp_raw_length(x * x, 1, bits, par.tolist(), order)
        assert kind == "len"
        return v
    lo, hi = (int(np.array(v, np.float64).view(np.int64)) for v in (2.0 ** -40, 1.0))
    assert raw(lo) < target < raw(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if raw(mid) < target:
            lo = mid
        else:
            hi = mid
    return float(np.array(hi, np.int64).view(np.float64)), float(raw(hi))


def test_code_length_edge_operands(L, oracle):
    zeros = np.zeros(17)
    # r0 = 0
    m, h, o, _ = three_ways(L, oracle, np.zeros(5), 16, zeros)
    assert m == 0.0 and same(m, h) and same(m, o)
    # just above, at and just below the FLT_MIN branch: r0 * 2^30 against 2^-126 at 16 bits
    seen = []
    for x in (2.0 ** -78 * (1 + 2.0 ** -52), 2.0 ** -78, 2.0 ** -78 * (1 - 2.0 ** -53)):
        m, h, o, r0 = three_ways(L, oracle, np.array([x]), 16, zeros)
        assert same(m, h) and same(m, o)
        seen.append((r0 * 2.0 ** 30 > P.FLT_MIN, m))
    assert seen == [(True, 0.125), (False, 0.0), (False, 0.0)]      # above the branch the length is far below zero: clamped
    # within 1e-12 of the clamp, on both sides, and as close as doubles get
    par = np.zeros(9)
    par[1:] = [0.5, -0.25, 0.125, 0.1, 0.0, -0.05, 0.01, 0.3]
    for target in (1e-12, -1e-12, 1e-16, -1e-16, 0.0):
        x, got = _x_with_length(16, par, D(target))
        assert abs(got - target) < 1e-15
        m, h, o, _ = three_ways(L, oracle, np.array([x]), 16, par)
        assert same(m, h) and same(m, o), (target, m, h, o)
        assert m == 0.125 or 0 < m < 2e-12
    # k = +-1 exactly: log(0) = -inf, both sides clamp
    for k in (1.0, -1.0):
        par = np.zeros(17)
        par[3] = k
        m, h, o, _ = three_ways(L, oracle, np.array([0.25, -0.125]), 16, par)
        assert m == 0.125 and same(m, h) and same(m, o)
    # one |k| > 1; two in one octet (1..8), two in the second octet (9..16): NaN on the host side every time
    for idx in ((4,), (2, 7), (9, 16), (1, 8), (8, 9)):
        par = np.zeros(17)
        par[1:] = 0.1
        for i in idx:
            par[i] = -1.25 if i % 2 else 1.5
        m, h, o, _ = three_ways(L, oracle, np.array([0.25, -0.125]), 16, par)
        assert math.isnan(m) and math.isnan(h) and math.isnan(o), (idx, m, h, o)
        assert P.hp_raw_length(0.07, 2, 16, par.tolist(), 16)[0] == "nan"
    # a non-finite energy never gives a usable length
    for r0 in (P.INF, P.NAN, -1.0):
        m = P.code_length(r0, 100, 16, zeros.tolist(), 16)
        h = L.slai_code_length(r0, 100, 16, ptr(zeros, f64p), 16)
        assert same(m, h) and not (m < P.BIG)


def _matrices():
    rng = np.random.default_rng(11)
    for nodes in (2, 3, 9, 17):
        for density in (1.0, 0.5, 0.2):
            for kind in ("small-int", "real", "nan", "no-goal"):
                for _ in range(6):
                    adj = np.full((nodes, nodes), P.BIG)
                    for i in range(nodes):
                        for j in range(i + 1, nodes):
                            if rng.random() < density or (j == i + 1 and kind != "no-goal"):
                                adj[i, j] = float(rng.integers(1, 6)) if kind == "small-int" else float(rng.uniform(300, 3000))
                    if kind == "nan":
                        for _ in range(nodes):
                            i, j = sorted(rng.integers(0, nodes, 2))
                            if i < j:
                                adj[i, j] = P.NAN
                    if kind == "no-goal":
                        adj[:, nodes - 1] = P.BIG
                    yield nodes, kind, adj


def test_dijkstra_equals_host_and_oracle(L, oracle):
    unreachable = 0
    for nodes, kind, adj in _matrices():
        ret, path = P.dijkstra(adj.tolist(), nodes)
        got = np.zeros(nodes, np.uint32)
        hret = L.slai_shortest_path(ptr(adj, f64p), nodes, ptr(got, u32p))
        oret, _, want = oracle.dijkstra(adj, 0, nodes - 1)
        assert hret == ret and (oret == 0) == (ret == 0), (nodes, kind)
        assert got.tolist() == path and want.tolist() == path, (nodes, kind, adj)
        unreachable += ret != 0
        if ret == 0:
            parts = P.back_walk(path, nodes, (nodes - 1) * 1024 - 5)
            assert sum(parts) == (nodes - 1) * 1024 - 5 and parts[-1] % 1024 == 1019
    assert unreachable >= 20


def test_gap_of_hand_made_tables():
    big = D(P.BIG)

    def matrix(nodes, edges):
        adj = [[big] * nodes for _ in range(nodes)]
        for (i, j), c in edges.items():
            adj[i][j] = None if c is None else D(c)
        return adj
    assert P.gap_of(matrix(3, {(0, 1): 10, (1, 2): 10, (0, 2): 20}), 3) == 0.0                     # exact tie at a relaxation
    assert P.gap_of(matrix(3, {(0, 1): 10, (1, 2): 10, (0, 2): 25}), 3) == 5.0                     # two paths, 20 against 25
    assert P.gap_of(matrix(3, {(0, 1): 20, (1, 2): 10, (0, 2): 20}), 3) == 0.0                     # tie in a selection round
    assert P.gap_of(matrix(4, {(0, 1): 10, (1, 3): 7, (0, 2): 17.5, (2, 3): 1}), 4) == 0.5         # goal 17 against node 2 at 17.5
    assert P.gap_of(matrix(2, {(0, 1): 3}), 2) > 1e6                                               # nothing to compare with
    assert P.gap_of(matrix(3, {(0, 1): 10, (1, 2): None, (0, 2): 10.25}), 3) == 0.25               # an unusable edge is no comparison


def test_gap_and_clamp_in_one_pass():
    t = P.first_separated(1, 3 * 1024 + 9, 2, 8, 16)
    for c in (t, P.certify(t, 1e-8)):
        assert P.gap_and_clamp(c) == (P.decision_gap(c), P.clamp_distance(c))


def test_near_ties_have_the_gap_they_were_built_for():
    t = P.first_separated(0, 8192, 1, 5, 16)
    for place in ("select", "relax", "goal"):
        for delta in (0.0, 1e-9, -1e-6, 5e-5, -2e-4, 1e-2):
            tuned, got = P.near_tie(t, place, delta)
            assert abs(P.decision_gap(tuned) - abs(delta)) < 1e-11
            if abs(delta) >= 2e-4:
                assert P.host_decide(tuned) == P.hp_decide(tuned)


def test_certified_model():
    t = P.first_separated(4, 3 * 1024 + 100, 2, 8, 16)
    c = P.certify(t, 1e-9)
    assert P.hp_decide(c) == P.hp_decide(t) == P.host_decide(c) == P.host_decide(t)
    for k in range(len(t.cands)):
        assert abs(float(P.hp_edge_cost(c, k) - P.hp_edge_cost(t, k))) < 1e-9                       # log2(e_p / r0) rounded to a double
        hw = P.half_width(c, k)
        assert hw == sum(t.cands[k][1] * 1e-9 / 16 for _ in range(2))
        up = P.hp_edge_cost(c, k, lambda k_, ch: 1.0) - P.hp_edge_cost(c, k)
        assert abs(float(up) - hw) < 1e-18
    assert P.redecide(c, lambda k, ch: -1.0) == P.hp_decide(t)


@pytest.mark.parametrize("nch,order,bits", P.SEPARATED_COMBOS)
def test_separated_generator_drops_at_most_15_percent(nch, order, bits):
    """the filter of test_gpu_plan.py's well-separated tables (gap >= 1e-2), from the model alone, for every shape it uses"""
    for window in P.SEPARATED_WINDOWS:
        count = 20
        kept, made = P.separated_tables(window, nch, order, bits, count)
        assert made == count and len(kept) >= 0.85 * made, (window, len(kept), made)


# ---- refusals: they come before any device work, dangling (suitably aligned) pointers are never followed ----------------

def test_plan_launcher_refusals(L):
    g, c, o, p, n, s = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000))

    def launch(g=g, nsf=3, nch=2, order=16, bits=16, c=c, o=o, p=p, n=n, s=s):
        return L.sla_hip_launch_plan(g, nsf, nch, order, bits, c, o, p, n, s, None)
    for name in ("g", "c", "o", "p", "n", "s"):
        assert launch(**{name: None}) == INVALID_ARGUMENT, name
    for kw in ({"nch": 0}, {"nch": 9}, {"order": 0}, {"bits": 0}, {"bits": 33}):
        assert launch(**kw) == INVALID_ARGUMENT, kw
    assert launch(nsf=0) == 0


def test_prepass_launcher_refusals(L):
    pcm, orw, nz, tiles = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))

    def launch(pcm=pcm, stride=100, nch=2, n=100, bits=16, ms=0, orw=orw, nz=nz):
        return L.sla_hip_launch_prepass(pcm, C.c_uint64(stride), nch, n, bits, ms, orw, nz, None)

    def launch_tiles(nch=2, stride=100, n=100, ms=0, tiles=tiles):
        return L.sla_hip_launch_prepass_tiles(pcm, C.c_uint64(stride), nch, n, 16, ms, orw, nz, tiles, None)
    for kw in ({"pcm": None}, {"orw": None}, {"nz": None}, {"stride": 99}, {"nch": 0}, {"nch": 9}, {"bits": 0}, {"bits": 33},
               {"nch": 1, "ms": 1}, {"nch": 3, "ms": 1}):
        assert launch(**kw) == INVALID_ARGUMENT, kw
    assert launch_tiles(tiles=None) == INVALID_ARGUMENT
    assert launch_tiles(stride=99) == INVALID_ARGUMENT
    assert launch_tiles(nch=3, ms=1) == INVALID_ARGUMENT
    a, b, c, d, e = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))
    for args in ((None, b, c, d, e), (a, None, c, d, e), (a, b, None, d, e), (a, b, c, None, e), (a, b, c, d, None)):
        assert L.sla_hip_launch_batch_scan(args[0], args[1], args[2], args[3], 4, 4096, args[4], None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_batch_scan(a, b, c, d, 0, 4096, e, None) == 0
