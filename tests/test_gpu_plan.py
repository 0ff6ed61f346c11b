"""sla_hip_launch_plan (k_plan, kernels/search.inc) on crafted candidate tables against the device-free model of
tests/planmodel.py.  No audio: the kernel's inputs are plain tables of doubles.

The tested contract.  The kernel accepts a comparison decided by more than PLAN_MARGIN = 1e-4 bytes and claims that the
device/host discrepancy of a path cost stays below "a few 1e-8".  That figure is the kernel's own claim, not a measurement,
so the thresholds stay a factor of two clear of the margin on either side:

    model gap <= 5e-5 (planmodel.MUST_FLAG)    must be flagged (status != 0)
    model gap >= 2e-4 (planmodel.MUST_ACCEPT)  must come back status 0
    in between                                 either answer

and in every case status 0 means num_parts and parts are the model's.  Every launch goes through launch(), which lays the
super-frames out at non-zero, differing slot_first / cand_first, fills the group entries of channels 1..C-1 with values that
would change the answer, and checks the sentinels: parts beyond num_parts, whole rows of flagged super-frames, guard words
behind every output array, and d_lpc_out bit for bit except the NaN flags of a status-2 super-frame."""
import ctypes as C
import functools

import numpy as np
import pytest

import planmodel as P
import sla_amd

pytestmark = pytest.mark.gpu

SENT = 0xDEADBEEF
SLOT_SENT = -7.25e100
NODES = 17


class Group(C.Structure):                                       # sla_hip_lpc_group
    _fields_ = [("pcm_off", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


@pytest.fixture(scope="module")
def L():
    import torch
    torch.cuda.init()
    return sla_amd.lib()


def launch(L, tables, num_sf=None):
    """one sla_hip_launch_plan over the tables (same channels, order, bits).  Returns [(status, parts or None)]."""
    import torch
    nch, order, bps = tables[0].nch, tables[0].order, tables[0].bps
    assert all((t.nch, t.order, t.bps) == (nch, order, bps) for t in tables)
    O2 = order + 2
    cands, slots, groups, where = [(7, 3)] * 3, [np.full((5, O2), SLOT_SENT)], [], []
    nslots = 5
    for t in tables:
        nc = len(t.cands)
        where.append((nslots, nc))
        groups.append(Group(0, t.window, 0, 0xFFFFFFFF, 32 - bps, len(cands), nc, nslots, 0))
        for ch in range(1, nch):                                # only channel 0's entry is documented as read
            groups.append(Group(0, 1024, ch, 0xFFFFFFFF, 0, 0, 1, 0, 0))
        cands += t.cands + [(7, 3)]
        slots += [t.slots.reshape(nch * nc, O2), np.full((2, O2), SLOT_SENT)]
        nslots += nch * nc + 2
    slots.append(np.full((4, O2), SLOT_SENT))
    lpc = np.ascontiguousarray(np.concatenate(slots))
    n = len(tables) if num_sf is None else num_sf
    d_g = torch.frombuffer(bytearray(b"".join(bytes(g) for g in groups)), dtype=torch.uint8).cuda()
    d_c = torch.from_numpy(np.array(cands, np.uint32)).cuda()
    d_o = torch.from_numpy(lpc).cuda()
    d_parts = torch.from_numpy(np.full(len(tables) * NODES + 8, SENT, np.uint32).view(np.int32)).cuda()
    d_np = torch.from_numpy(np.full(len(tables) + 8, SENT, np.uint32).view(np.int32)).cuda()
    d_st = torch.from_numpy(np.full(len(tables) + 8, SENT, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_plan(C.c_void_p(d_g.data_ptr()), n, nch, order, bps, C.c_void_p(d_c.data_ptr()), C.c_void_p(d_o.data_ptr()),
                               C.c_void_p(d_parts.data_ptr()), C.c_void_p(d_np.data_ptr()), C.c_void_p(d_st.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    parts, nparts, status = (x.cpu().numpy().view(np.uint32) for x in (d_parts, d_np, d_st))
    out = d_o.cpu().numpy()
    assert (parts[n * NODES:] == SENT).all() and (nparts[n:] == SENT).all() and (status[n:] == SENT).all()
    expect = lpc.copy()
    res = []
    for sf in range(n):
        t = tables[sf]
        row = parts[sf * NODES:(sf + 1) * NODES]
        st, cnt = int(status[sf]), int(nparts[sf])
        assert st in (0, 1, 2), (sf, st)
        if st == 0:
            assert 1 <= cnt <= t.nodes - 1 and (row[cnt:] == SENT).all(), (sf, cnt, row)
            res.append((0, row[:cnt].tolist()))
        else:
            assert cnt == 0 and (row == SENT).all(), (sf, st, cnt, row)
            res.append((st, None))
        if st == 2:                                             # every slot of this super-frame flagged, nothing else
            assert (t.slots[:, :, 1] != 0).any(), "status 2 without a certified slot"
            first, nc = where[sf]
            assert np.isnan(out[first:first + nch * nc, 0]).all(), sf
            expect[first:first + nch * nc, 0] = out[first:first + nch * nc, 0]
    assert np.array_equal(out.view(np.uint64), expect.view(np.uint64))
    return res


def check(L, tables, wants):
    """wants per table: "accept" (status 0), "flag" (status != 0), 1 or 2 (that status), "either"; status 0 always means
    the model's partition"""
    got = launch(L, tables)
    for sf, (t, want, (st, parts)) in enumerate(zip(tables, wants, got)):
        if st == 0:
            try:
                model = P.host_decide(t)
            except ValueError as e:                             # a candidate that is no edge of the lattice
                raise AssertionError("super-frame %d: status 0 for a table the model refuses (%s)" % (sf, e))
            assert parts == model, (sf, want, parts, model)
        if want == "accept":
            assert st == 0, (sf, st)
        elif want == "flag":
            assert st != 0, (sf, parts)
        elif want != "either":
            assert st == want, (sf, want, st, parts)
    return got


def separated(seed, window, nch, order, bps, min_gap=1e-2):
    t = P.first_separated(seed, window, nch, order, bps, min_gap)
    assert P.host_decide(t) == P.hp_decide(t)
    return t


# ---- well-separated random tables ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch,order,bits", P.SEPARATED_COMBOS)
def test_separated_random_tables(L, nch, order, bits):
    """full lattices of 2, 3, 9, 16 and 17 nodes (136 candidates at 17: three passes of the 64 lanes), windows mixed within
    the launch; the first tables that the filter keeps of the streams whose drop rate tests/test_plan_model.py bounds"""
    tables = []
    for w in P.SEPARATED_WINDOWS:
        kept, _ = P.separated_tables(w, nch, order, bits, 20, limit=3 if w < 8192 else 2 if nch < 8 else 1)
        assert kept
        tables += kept
    tables = [tables[i] for i in np.random.default_rng(nch).permutation(len(tables))]
    for t in tables:
        assert P.decision_gap(t) >= 1e-2 and len(t.cands) == t.nodes * (t.nodes - 1) // 2
    check(L, tables, ["accept"] * len(tables))


# ---- near ties by construction -------------------------------------------------------------------------------------------

DELTAS = (0.0, 1e-9, 1e-6, 5e-5, 2e-4, 1e-2)


@functools.lru_cache(maxsize=None)
def _tie_set(window, place):
    """a separated table in which the tie of every delta and sign can be built at `place`, and those tables"""
    for seed in range(40):
        base = P.first_separated(seed, window, 1, 5, 16)
        made = []
        for d in DELTAS:
            for sign in (1.0, -1.0):
                r = P.near_tie(base, place, sign * d)
                if r is None:
                    break
                made.append((sign * d, r[0]))
            else:
                continue
            break
        else:
            return base, made
    raise AssertionError("no table takes a tie at " + place)


@pytest.mark.parametrize("place", ["select", "relax", "goal"])
@pytest.mark.parametrize("window", [2047, 8192, 16384])
def test_near_ties(L, window, place):
    """select: the two cheapest edges out of node 0 (the first selection round that has a choice; at 3 nodes the goal is
    one of the two); relax: 0 -> 2 against 0 -> 1 -> 2 when node 1 relaxes node 2; goal: the goal against the cheapest node
    still open in the round that settles the goal.  One r0 tuned by bisection in the model, every other comparison >= 1e-2."""
    base, made = _tie_set(window, place)
    tables, wants = [base], ["accept"]
    for delta, t in made:
        gap = P.decision_gap(t)
        assert abs(gap - abs(delta)) < 1e-11
        tables.append(t)
        assert abs(delta) <= P.MUST_FLAG or abs(delta) >= P.MUST_ACCEPT
        wants.append(1 if abs(delta) <= P.MUST_FLAG else "accept")       # (the tuned gap is delta to within 1e-11)
    got = check(L, tables, wants)
    routes = {d: parts for (d, _), (_, parts) in zip(made, got[1:])}
    if place == "relax" and 2048 in np.cumsum(routes[1e-2]).tolist():
        assert routes[1e-2] != routes[-1e-2]                    # the route runs over node 2: the other sign, the other route


def test_everything_clamped(L):
    """8-bit tables so quiet that every length is clamped: every edge costs len * 0.125 * C + 350 exactly, routes with equal
    edge counts tie exactly.  With blocks of at most two tiles (a max block length) the routes 0-1-3 and 0-2-3 of a
    three-tile window meet in a relaxation at cost 0: never decided on the device.  (With the full lattice the single
    edge 0-3 wins and no comparison is closer than the bytes of the last tile, in exact arithmetic on both sides: the model's answer is required.)"""
    for nch in (1, 3):
        for window in (3 * 1024, 2 * 1024 + 77 + 1024):
            cands = [c for c in P.full_lattice(window) if c[1] <= 2048]
            slots = np.zeros((nch, len(cands), 7))
            for k, (_, n) in enumerate(cands):
                slots[:, k, 0] = 1e-20 * n * (1 + 0.1 * k)
                slots[:, k, 2:] = 0.01
            t = P.Table(window, nch, 5, 8, cands, slots)
            for k in range(len(cands)):
                assert P.host_edge_cost(t, k) == cands[k][1] * 0.125 * nch + 350
            assert P.decision_gap(t) == 0.0
            full = P.full_lattice(window)
            slots = np.zeros((nch, len(full), 7))
            slots[:, :, 0] = 1e-17
            f = P.Table(window, nch, 5, 8, full, slots)
            assert P.decision_gap(f) >= 1.0 and P.host_decide(f) == [window]
            check(L, [t, f], [1, "accept"])


# ---- branches of the estimate --------------------------------------------------------------------------------------------

def _base(order=16, seed=2):
    t = separated(seed, 4 * 1024 + 100, 2, order, 16)
    parts = P.host_decide(t)
    return t, parts, P.route_edges(t, parts)


def _model_separated(t):
    assert P.decision_gap(t) >= 1e-2 and P.host_decide(t) == P.hp_decide(t)


def test_estimate_zero_energy_and_clamp(L):
    t, parts, edges = _base()
    k = edges[0]
    zero = t.copy()
    zero.slots[1, k, 0] = 0.0                                  # the channel contributes 0 bytes
    assert P.code_length(0.0, t.cands[k][1], 16, zero.slots[1, k, 1:].tolist(), 16) == 0.0
    room = t.copy()
    room.slots[1, k, 0] = 1e-14                                # far below the clamp: 0.125 bytes per sample
    assert P.code_length(1e-14, t.cands[k][1], 16, room.slots[1, k, 1:].tolist(), 16) == 0.125
    ones = []
    for kk in (1.0, -1.0):                                      # log(0) = -inf: both sides clamp
        c = t.copy()
        c.slots[0, k, 2 + 3] = kk
        assert P.code_length(c.slots[0, k, 0], t.cands[k][1], 16, c.slots[0, k, 1:].tolist(), 16) == 0.125
        ones.append(c)
    tables = [zero, room] + ones
    for c in tables:
        _model_separated(c)
        assert P.clamp_distance(c) > 1e-6
    check(L, tables, ["accept"] * 4)


def test_estimate_length_next_to_the_clamp(L):
    """a length within 1e-10 of zero, either side: the branch hangs on the logarithm's last bits"""
    t, parts, edges = _base()
    tables = []
    for target in (5e-11, -5e-11, 1e-15):
        for k in (edges[-1], (edges[-1] + 1) % len(t.cands)):
            c = P.tune_length(t, k, 1, target)
            assert c is not None and abs(P.clamp_distance(c) - abs(target)) < 1e-15
            assert P.decision_gap(c) >= 1e-2                     # nothing else is close
            tables.append(c)
    check(L, tables, [1] * len(tables))


def _sign_flipped(t, k, ch, idx):
    """coefficients idx of slot (ch, k) replaced by sqrt(2 - k*k): each factor 1 - k*k changes its sign and keeps its size, so
    a product over a pair of them is what it was"""
    c = t.copy()
    for i in idx:
        v = c.slots[ch, k, 1 + i]
        c.slots[ch, k, 1 + i] = np.sqrt(2.0 - v * v)
        assert c.slots[ch, k, 1 + i] > 1.0
    return c


def test_estimate_coefficients_beyond_one(L):
    """|k| > 1 makes the host's logarithm NaN and the edge unusable: the reference's Dijkstra never takes it.  The tables
    put such coefficients on an edge of the route that wins without them.  One of them: flagged.  A pair inside one group of
    eight factors (orders 1..8, and 9..16): the product of the group is positive again, with the size it had; the kernel
    must flag, or answer with the model's partition, which avoids the edge."""
    t, parts, edges = _base()
    tables, wants = [], []
    for k in (edges[0], edges[-1]):
        one = _sign_flipped(t, k, 0, (4,))
        assert np.isnan(P.host_edge_cost(one, k)) and P.host_decide(one) != parts
        tables.append(one)
        wants.append("flag")
        for idx in ((2, 7), (9, 16), (1, 8), (3, 12)):
            for ch in (0, 1):
                two = _sign_flipped(t, k, ch, idx)
                assert np.isnan(P.host_edge_cost(two, k)) and P.hp_edge_cost(two, k) is None
                avoid = P.host_decide(two)
                assert avoid is not None and avoid != parts and k not in P.route_edges(two, avoid)
                tables.append(two)
                wants.append("either")                          # status 0 only with the model's partition (check())
    check(L, tables, wants)


def test_estimate_non_finite_energy(L):
    t, parts, edges = _base()
    tables = []
    for v in (P.NAN, P.INF, -P.INF, -1.0):
        for k, ch in ((edges[0], 0), ((edges[0] + 1) % len(t.cands), 1)):
            c = t.copy()
            c.slots[ch, k, 0] = v
            tables.append(c)
    check(L, tables, [1] * len(tables))


# ---- malformed and missing candidates ------------------------------------------------------------------------------------

def test_malformed_candidates(L):
    t = separated(5, 2047, 2, 16, 16)                           # candidates (0,1024) (0,2047) (1024,1023)
    assert t.cands == [(0, 1024), (0, 2047), (1024, 1023)]
    bad = []
    for k, cand in ((2, (1100, 947)), (0, (5, 1019)), (2, (1024, 1024)), (1, (0, 2048)), (0, (0, 0)), (2, (1024, 0)),
                    (2, (2048, 1024)), (0, (0, 1000)), (1, (0, 3000)), (2, (1024, 0xFFFFFC00)), (2, (0xFFFFFC00, 2047))):
        c = t.copy()
        c.cands[k] = cand
        bad.append(c)
    t3 = separated(6, 3 * 1024, 2, 16, 16)
    c = t3.copy()
    c.cands[t3.find(1, 2)] = (1100, 948)                        # i = 1, j = 2 by rounding alone
    bad.append(c)
    check(L, bad, ["flag"] * len(bad))
    # a lattice without any edge into the goal; no candidates at all
    nogoal = [k for k in range(len(t3.cands)) if t3.edge(k)[1] != t3.nodes - 1]
    ng = P.Table(t3.window, 2, 16, 16, [t3.cands[k] for k in nogoal], t3.slots[:, nogoal])
    assert P.host_decide(ng) is None
    empty = P.Table(t3.window, 2, 16, 16, [], np.zeros((2, 0, 18)))
    check(L, [ng, empty, t3], [1, 1, "accept"])


def test_window_of_18_nodes(L):
    t = separated(7, 16384, 1, 5, 16)
    big = P.Table(16385, 1, 5, 16, t.cands, t.slots)
    assert big.nodes == 18
    assert launch(L, [t, big, t]) == [(0, P.host_decide(t)), (1, None), (0, P.host_decide(t))]


# ---- certified candidates ------------------------------------------------------------------------------------------------

def _margin(t):
    return P.PLAN_MARGIN + 2 * (t.nodes - 1) * max(P.half_width(t, k) for k in range(len(t.cands)))


@pytest.mark.parametrize("window,nch,order", [(2047, 1, 5), (8192, 2, 16), (16384, 3, 32), (15 * 1024 + 333, 8, 16)])
def test_certified_separated(L, window, nch, order):
    """widths 1e-12 .. 1e-6, every comparison at least 10 x (1e-4 + 2 (nodes - 1) wmax) apart: status 0, and the partition
    is the model's at the midpoints, at the adversarial corner (the chosen route at +w, everything else at -w) and at 50
    random corners"""
    rng = np.random.default_rng(window)
    tables = []
    for i, w in enumerate((1e-12, 1e-9, 1e-6, None)):
        base = separated(20 + i, window, nch, order, 16, min_gap=5.0)
        if w is None:
            ws = 10.0 ** rng.uniform(-12, -6, (len(base.cands), nch))
            c = P.certify(base, lambda k, ch: ws[k, ch])
        else:
            c = P.certify(base, w)
        assert P.decision_gap(c) >= 10 * _margin(c)
        tables.append(c)
    got = check(L, tables, ["accept"] * len(tables))
    for c, (_, parts) in zip(tables, got):
        assert parts == P.redecide(c, None)
        chosen = set(P.route_edges(c, parts))
        assert parts == P.redecide(c, lambda k, ch: 1.0 if k in chosen else -1.0)
        for _ in range(50 if c.nodes <= 9 else 10 if nch < 8 else 3):
            corner = rng.choice([-1.0, 1.0], (len(c.cands), nch))
            assert parts == P.redecide(c, lambda k, ch: corner[k, ch])


def _undecidable(nch, exact_channel):
    """3 nodes; the half widths of the three edges are all H = 1e-2 bytes, the routes 0-2 and 0-1-2 differ by 2.9e-2 at
    the midpoints: no more than the summed half widths of both routes (3 H), so the truth is undecidable -- and more than
    1e-4 + 2 (nodes - 1) (H / 2), so a planner that took half the widths would accept it"""
    H = 1e-2
    base = P.first_separated(31, 2048, nch, 8, 16)
    certified = 1 if exact_channel else nch

    def width(k, ch):
        if exact_channel and ch == 0:
            return 0.0
        return H * 16.0 / base.cands[k][1] / certified
    c = P.certify(base, width)
    if exact_channel:                                           # channel 0 keeps its coefficients
        c.slots[0] = base.slots[0]
    for sign in (1.0, -1.0):
        r = P.near_tie(c, "relax", sign * 2.9e-2, others=1.0)
        assert r is not None
        t = r[0]
        k02, k01, k12 = t.find(0, 2), t.find(0, 1), t.find(1, 2)
        total = sum(P.half_width(t, k) for k in (k02, k01, k12))
        assert abs(total - 3 * H) < 1e-12 and abs(r[1]) <= total
        assert abs(r[1]) > P.PLAN_MARGIN + 2 * 2 * (H / 2) and abs(r[1]) < _margin(t)
        up = P.redecide(t, lambda k, ch: 1.0 if k == k02 else -1.0)
        down = P.redecide(t, lambda k, ch: -1.0 if k == k02 else 1.0)
        assert up != down                                       # the widths do decide
        yield t


def test_certified_undecidable(L):
    tables = list(_undecidable(1, False)) + list(_undecidable(2, False))[:1]
    check(L, tables[:2], [2, 2])
    check(L, tables[2:], [2])


def test_certified_with_an_exact_channel(L):
    """one channel exact, one certified: an undecidable tie is status 2 (the chains can still decide it), not 1"""
    check(L, list(_undecidable(2, True)), [2, 2])


def test_certified_unusable_widths(L):
    base = separated(33, 3 * 1024 + 5, 2, 8, 16)
    c = P.certify(base, 1e-9)
    inf = c.copy()
    inf.slots[1, 2, 1] = P.INF
    zero = c.copy()
    zero.slots[0, 1, 0] = 0.0                                   # a certified slot without energy
    huge = c.copy()
    huge.slots[:, :, 1] = 100.0                                 # half widths of thousands of bytes: nothing is certain
    got = check(L, [c, inf, zero, huge, c], ["accept", 2, 2, 2, "accept"])
    assert got[0] == got[4]


# ---- layout --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count,nch", [(1, 1), (3, 2), (4, 3), (5, 2), (9, 1)])
def test_launch_layout(L, count, nch):
    """1 .. 9 super-frames: up to four waves per workgroup and a ragged last workgroup; windows, candidate counts and
    statuses mixed, so that a flagged super-frame sits between accepted ones"""
    rng = np.random.default_rng(count)
    tables, wants = [], []
    for sf in range(count):
        window = int(rng.choice([700, 1024, 2047, 3 * 1024 + 1, 5 * 1024, 8192]))
        t = separated(40 + sf, window, nch, 8, 16)
        kind = (sf + count) % 4
        if kind == 1 and t.nodes >= 3:
            tie = P.near_tie(t, "relax", 0.0)
            t = tie[0] if tie is not None else t
            wants.append(1 if P.decision_gap(t) <= P.MUST_FLAG else "accept")
        elif kind == 2:
            t = P.certify(t, 100.0)
            wants.append(2 if t.nodes >= 3 else "either")
        elif kind == 3:
            t = P.certify(t, 1e-10)
            wants.append("accept")
        else:
            wants.append("accept")
        tables.append(t)
    got = check(L, tables, wants)
    if count >= 4:
        assert len({st for st, _ in got}) >= 2


def test_no_superframes_writes_nothing(L):
    t = separated(3, 2047, 2, 16, 16)
    assert launch(L, [t, t], num_sf=0) == []
