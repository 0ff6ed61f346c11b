"""Device-free model of the partition planner (include/sla_hip.h, sla_hip_launch_plan), written from the reference's host
arithmetic and from the header's slot layout, not from the kernel:

  a. the decision itself in plain Python floats -- code length, edge cost, Dijkstra, back-walk -- operation by operation as
     the host does it (math.log is the C library's log); this is what status 0 promises to reproduce;
  b. the same costs with `decimal` at 60 digits, and from them the DECISION GAP of a table: the smallest difference over
     every comparison that Dijkstra makes.  A table with a large gap is decided the same way by any arithmetic that is
     accurate to less than the gap, a table with gap 0 is a tie that only the host's own rounding decides;
  c. certified candidates (slot layout { r0, w, log2(e_p / r0), 0, .. }): the cost at the midpoint, the half width in bytes,
     and the partition re-decided with every candidate's log2(e_p) moved to a chosen point of [mid - w, mid + w].

High precision means: the operands the host hands to log() (r0 * 2^(2 bits - 2), n, the rounded doubles 1 - k*k) are taken
as they are, the logarithms, their sum and everything after them are exact to 60 digits.

Thresholds of the planner's tested contract (tests/test_gpu_plan.py).  The kernel accepts a comparison that is decided by
more than PLAN_MARGIN = 1e-4 bytes; its own comment bounds the device/host discrepancy of a path cost by "a few 1e-8".
That bound is the kernel's claim, not a measurement, so the tests stay a factor of two clear of the margin on either side:
a model gap <= MUST_FLAG has to be flagged, a model gap >= MUST_ACCEPT has to come back with status 0."""
import decimal
import functools
import math

import numpy as np

D = decimal.Decimal
CTX = decimal.Context(prec=60, Emin=-999999, Emax=999999)
TILE = 1024
MAX_NODES = 17
BIG = 16777216.0                       # 2^24
FLT_MIN = 1.1754943508222875e-38       # 2^-126
L2E = 1.4426950408889634
C0 = 1.9426950408889634
PLAN_MARGIN = 1e-4
MUST_FLAG = 5e-5
MUST_ACCEPT = 2e-4
NOPRED = 0xFFFFFFFF
INF = float("inf")
NAN = float("nan")


def _hp(fn):
    """run fn with the 60-digit context current, so that plain + and - on Decimals are as exact as the CTX calls"""
    @functools.wraps(fn)
    def inner(*a, **kw):
        with decimal.localcontext(CTX):
            return fn(*a, **kw)
    return inner


# ---- a. the host's arithmetic -------------------------------------------------------------------------------------------

def c_log(x):
    """log() of the C library on a double, with its answers at and below zero"""
    if x != x:
        return NAN
    if x == 0.0:
        return -INF
    if x < 0.0:
        return NAN
    return math.log(x)


def log2_libm(x):
    return c_log(x) * L2E


def code_length(sumsq, n, bps, parcor, order):
    """bytes per sample; parcor[1..order] are read (parcor[0] is not)"""
    power = sumsq * math.ldexp(1.0, 2 * (bps - 1))
    if abs(power) <= FLT_MIN:
        return 0.0
    power = log2_libm(power) - log2_libm(float(n))
    gain = 0.0
    for k in range(1, order + 1):
        gain += log2_libm(1.0 - parcor[k] * parcor[k])
    ln = C0 + 0.5 * (power + gain)
    ln /= 8
    return 0.125 if ln <= 0 else ln


def code_length_cert(sumsq, n, bps, gain):
    """the same with gain = log2(e_p / r0) given (certified slot)"""
    power = sumsq * math.ldexp(1.0, 2 * (bps - 1))
    if abs(power) <= FLT_MIN:
        return 0.0
    power = log2_libm(power) - log2_libm(float(n))
    ln = C0 + 0.5 * (power + gain)
    ln /= 8
    return 0.125 if ln <= 0 else ln


def dijkstra(adj, nodes, big=BIG, trace=None):
    """adj: nodes x nodes (list of lists); an entry None is an edge the arithmetic cannot use (the host's NaN).
    Returns (0 or -1, path).  With a list as `trace`, every comparison is recorded as (kind, round, node, difference)."""
    zero = big - big
    cost = [big] * nodes
    done = [False] * nodes
    path = [NOPRED] * nodes
    cost[0] = zero
    cur = 0
    for rnd in range(nodes + 1):
        best = big
        for i in range(nodes):
            if not done[i] and cost[i] < best:
                best = cost[i]
                cur = i
        if trace is not None and best < big:
            others = [cost[i] for i in range(nodes) if not done[i] and i != cur and cost[i] < big]
            if others:
                trace.append(("select", rnd, cur, min(others) - best))
        if cur == nodes - 1:
            return 0, path
        for i in range(nodes):
            a = adj[cur][i]
            if a is None:
                continue
            via = a + cost[cur]
            if trace is not None and a < big:
                trace.append(("relax", rnd, i, abs(cost[i] - via)))
            if cost[i] > via:
                cost[i] = via
                path[i] = cur
        done[cur] = True
    return -1, path


def back_walk(path, nodes, window):
    """block lengths of the chosen route, or None when the predecessors do not lead back to node 0"""
    count, node = 0, nodes - 1
    while node != 0:
        if path[node] >= node:
            return None
        count += 1
        node = path[node]
    parts = [0] * count
    node = nodes - 1
    for q in range(count):
        pr = path[node]
        ln = (node - pr) * TILE
        if ln > window - pr * TILE:
            ln = window - pr * TILE
        parts[count - q - 1] = ln
        node = pr
    return parts


# ---- tables -------------------------------------------------------------------------------------------------------------

def nodes_of(window):
    return (window + TILE - 1) // TILE + 1


def full_lattice(window):
    nodes = nodes_of(window)
    return [(i * TILE, min((j - i) * TILE, window - i * TILE)) for i in range(nodes) for j in range(i + 1, nodes)]


class Table:
    """one super-frame: slots[ch, cand] = { r0, parcor[0] = w, parcor[1..order] } as the search kernels leave them"""

    def __init__(self, window, nch, order, bps, cands, slots):
        self.window, self.nch, self.order, self.bps = window, nch, order, bps
        self.cands = [(int(s), int(n)) for s, n in cands]
        self.slots = np.array(slots, np.float64).reshape(nch, len(self.cands), order + 2)
        self.nodes = nodes_of(window)

    def copy(self):
        return Table(self.window, self.nch, self.order, self.bps, self.cands, self.slots.copy())

    def edge(self, k):
        """(i, j) of candidate k; ValueError when it is no edge of the lattice"""
        s, n = self.cands[k]
        end = s + n
        if s % TILE or n == 0 or end > self.window or (end % TILE and end != self.window):
            raise ValueError("candidate %d (%d, %d) is off the lattice of a %d-sample window" % (k, s, n, self.window))
        return s // TILE, (end + TILE - 1) // TILE

    def find(self, i, j):
        for k in range(len(self.cands)):
            if self.edge(k) == (i, j):
                return k
        raise KeyError((i, j))


def host_edge_cost(t, k):
    ln = t.cands[k][1]
    est = 0.0
    for ch in range(t.nch):
        s = t.slots[ch, k].tolist()
        if s[1] != 0.0:
            est += ln * code_length_cert(s[0], ln, t.bps, s[2])
        else:
            est += ln * code_length(s[0], ln, t.bps, s[1:], t.order)
    est += 50.0
    est += 300.0
    return est


def host_adjacency(t):
    adj = [[BIG] * t.nodes for _ in range(t.nodes)]
    for k in range(len(t.cands)):
        i, j = t.edge(k)
        adj[i][j] = host_edge_cost(t, k)
    return adj


def host_decide(t):
    """the partition the host's arithmetic decides: list of block lengths, or None (the goal is never settled)"""
    ret, path = dijkstra(host_adjacency(t), t.nodes)
    return back_walk(path, t.nodes, t.window) if ret == 0 else None


# ---- b. high precision --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4096)
def _hp_log2(x):
    return CTX.multiply(CTX.ln(D(x)), D(L2E))


@_hp
def hp_raw_length(sumsq, n, bps, parcor, order, gain=None):
    """(kind, value): ("zero", 0) below the FLT_MIN branch, ("nan", None) where the host's length is NaN or +inf,
    ("-inf", None) where a factor 1 - k*k is zero, else ("len", bytes per sample before the clamp)"""
    power = sumsq * math.ldexp(1.0, 2 * (bps - 1))
    if abs(power) <= FLT_MIN:
        return "zero", D(0)
    if power != power or power < 0.0 or power == INF:
        return "nan", None
    if gain is None:
        prod = D(power)                                        # one logarithm of power * prod(1 - k*k): the same number
        for k in range(1, order + 1):
            f = 1.0 - parcor[k] * parcor[k]                    # the rounded double the host hands to log()
            if f != f or f < 0.0:
                return "nan", None
            prod = CTX.multiply(prod, D(f))
        if prod == 0:
            return "-inf", None
        total = CTX.subtract(CTX.multiply(CTX.ln(prod), D(L2E)), _hp_log2(float(n)))
    else:
        if gain != gain or gain == INF:
            return "nan", None
        if gain == -INF:
            return "-inf", None
        total = CTX.add(CTX.subtract(_hp_log2(power), _hp_log2(float(n))), D(gain))
    ln = CTX.divide(CTX.add(D(C0), CTX.multiply(D("0.5"), total)), D(8))
    return "len", ln


def hp_length(kind, value):
    if kind == "nan":
        return None
    if kind == "-inf":
        return D("0.125")
    if kind == "zero":
        return value
    return D("0.125") if value <= 0 else value


@_hp
def hp_edge_cost(t, k, point=None):
    """cost of candidate k in bytes (None: unusable).  point: None = midpoints, else a function (k, ch) -> u in [-1, 1] that
    moves log2(e_p) of a certified slot to mid + u * w"""
    ln = t.cands[k][1]
    est = D(0)
    for ch in range(t.nch):
        s = t.slots[ch, k].tolist()
        if s[1] != 0.0:
            kind, v = hp_raw_length(s[0], ln, t.bps, None, 0, gain=s[2])
            if point is not None and kind == "len":
                v = CTX.add(v, CTX.divide(CTX.multiply(D(point(k, ch)), D(s[1])), D(16)))
        else:
            kind, v = hp_raw_length(s[0], ln, t.bps, s[1:], t.order)
        c = hp_length(kind, v)
        if c is None:
            return None
        est = CTX.add(est, CTX.multiply(D(ln), c))
    return CTX.add(est, D(350))


@_hp
def hp_adjacency(t, point=None, costs=None):
    adj = [[D(BIG)] * t.nodes for _ in range(t.nodes)]
    for k in range(len(t.cands)):
        i, j = t.edge(k)
        adj[i][j] = costs[k] if costs is not None else hp_edge_cost(t, k, point)
    return adj


@_hp
def hp_decide(t, point=None, costs=None):
    ret, path = dijkstra(hp_adjacency(t, point, costs), t.nodes, D(BIG))
    return back_walk(path, t.nodes, t.window) if ret == 0 else None


@_hp
def comparisons(adj, nodes):
    """every comparison Dijkstra makes on a high-precision matrix: list of (kind, round, node, difference)"""
    trace = []
    dijkstra(adj, nodes, D(BIG), trace)
    return trace


@_hp
def gap_of(adj, nodes):
    tr = comparisons(adj, nodes)
    return float(min(x[3] for x in tr)) if tr else INF


@_hp
def decision_gap(t, point=None):
    return gap_of(hp_adjacency(t, point), t.nodes)


@_hp
def clamp_distance(t):
    """smallest |length before the clamp| over the slots, bytes per sample: the other branch a rounding could flip"""
    best = INF
    for k in range(len(t.cands)):
        for ch in range(t.nch):
            s = t.slots[ch, k].tolist()
            if s[1] != 0.0:
                kind, v = hp_raw_length(s[0], t.cands[k][1], t.bps, None, 0, gain=s[2])
            else:
                kind, v = hp_raw_length(s[0], t.cands[k][1], t.bps, s[1:], t.order)
            if kind == "len":
                best = min(best, abs(float(v)))
    return best


@_hp
def gap_and_clamp(t):
    """(decision_gap(t), clamp_distance(t)) with every slot's logarithm taken once"""
    costs, clamp = [], INF
    for k, (_, n) in enumerate(t.cands):
        est = D(350)
        for ch in range(t.nch):
            s = t.slots[ch, k].tolist()
            kind, v = hp_raw_length(s[0], n, t.bps, s[1:], t.order, gain=(s[2] if s[1] != 0.0 else None))
            if kind == "len":
                clamp = min(clamp, abs(float(v)))
            c = hp_length(kind, v)
            est = None if (c is None or est is None) else est + n * c
        costs.append(est)
    return gap_of(hp_adjacency(t, costs=costs), t.nodes), clamp


@_hp
def routes(adj, nodes):
    """every route 0 -> nodes-1 over the usable edges, as (cost, [nodes on the way]) sorted by cost (small lattices only)"""
    big = D(BIG)
    out = []

    def walk(node, cost, seen):
        if node == nodes - 1:
            out.append((cost, seen))
            return
        for j in range(node + 1, nodes):
            a = adj[node][j]
            if a is not None and a < big:
                walk(j, cost + a, seen + [j])
    walk(0, D(0), [0])
    return sorted(out, key=lambda r: r[0])


# ---- c. certified candidates --------------------------------------------------------------------------------------------

def half_width(t, k):
    """half width of candidate k's cost in bytes: len * w / 16, channels summed"""
    return sum(t.cands[k][1] * float(t.slots[ch, k, 1]) / 16.0 for ch in range(t.nch))


def route_edges(t, parts):
    """candidate indices of a partition"""
    out, off = [], 0
    for ln in parts:
        i = off // TILE
        j = (off + ln + TILE - 1) // TILE
        out.append(t.find(i, j))
        off += ln
    return out


def redecide(t, point):
    """the partition with every certified candidate's log2(e_p) at mid + point(k, ch) * w"""
    return hp_decide(t, point)


# ---- generators ---------------------------------------------------------------------------------------------------------

def random_table(rng, window, nch, order, bps, cands=None):
    """exact slots (w = 0): r0 of a signal of amplitude 1e-4 .. 0.3 (log-uniform) over the candidate's samples, PARCOR
    decaying with the order and well inside (-1, 1)"""
    cands = full_lattice(window) if cands is None else cands
    slots = np.zeros((nch, len(cands), order + 2))
    for k, (_, n) in enumerate(cands):
        for ch in range(nch):
            amp = 10.0 ** rng.uniform(-4.0, math.log10(0.3))
            slots[ch, k, 0] = amp * amp * n
            slots[ch, k, 2:] = rng.uniform(-0.9, 0.9, order) * 0.8 ** np.arange(order)
    return Table(window, nch, order, bps, cands, slots)


SEPARATED_WINDOWS = (700, 2047, 8192, 15 * 1024 + 333, 16384)   # 2, 3, 9, 16, 17 nodes; 136 candidates at 17
# (channels, order, bits).  8 bits go with three and eight channels: with one or two, whole edges are clamped in every channel
# so often that more than 15 % of the tables hold an exact tie (test_gpu_plan.py has those ties in a test of their own)
SEPARATED_COMBOS = ((1, 16, 16), (2, 32, 24), (3, 17, 8), (8, 5, 8))


def separated_tables(window, nch, order, bps, count, limit=None, min_gap=1e-2, min_clamp=1e-6):
    """(kept tables, generated): the fixed-seed stream of random tables of one shape, filtered by the model alone; stops
    after `count` tables, or once `limit` are kept"""
    rng = np.random.default_rng([window, nch, order, bps])
    kept, made = [], 0
    while made < count and (limit is None or len(kept) < limit):
        t = random_table(rng, window, nch, order, bps)
        made += 1
        gap, clamp = gap_and_clamp(t)
        if gap >= min_gap and clamp >= min_clamp:
            kept.append(t)
    return kept, made


def first_separated(seed, window, nch, order, bps, min_gap=1e-2):
    rng = np.random.default_rng(seed)
    for _ in range(200):
        t = random_table(rng, window, nch, order, bps)
        gap, clamp = gap_and_clamp(t)
        if gap >= min_gap and clamp >= 1e-6:
            return t
    raise AssertionError("no separated table")


@_hp
def certify(t, w):
    """the same table as certified slots { r0, w, log2(e_p / r0), 0, .. } of half width w (a number, or a function of k, ch)"""
    c = t.copy()
    for k in range(len(t.cands)):
        for ch in range(t.nch):
            ks = t.slots[ch, k, 2:].tolist()
            g = sum(D(1.0 - x * x).ln(CTX) for x in ks) * D(L2E)
            c.slots[ch, k, 1] = w(k, ch) if callable(w) else w
            c.slots[ch, k, 2] = float(g)
            c.slots[ch, k, 3:] = 0.0
    return c


# ---- near ties by construction ------------------------------------------------------------------------------------------

@_hp
def tune_r0(t, k, objective, target, ch=0):
    """bisect r0 of (candidate k, channel ch) over the doubles until objective(table) -- which must grow with that r0 -- is as
    close to `target` as one double allows.  Returns the tuned copy."""
    c = t.copy()
    lo = np.array(c.slots[ch, k, 0] * 2.0 ** -60, np.float64).view(np.int64).item()
    hi = np.array(c.slots[ch, k, 0] * 2.0 ** 60, np.float64).view(np.int64).item()

    def at(bits):
        c.slots[ch, k, 0] = np.array(bits, np.int64).view(np.float64)
        return objective(c)
    if not (at(lo) < target < at(hi)):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if at(mid) < target:
            lo = mid
        else:
            hi = mid
    a, b = at(lo), at(hi)
    at(lo if abs(a - target) <= abs(b - target) else hi)
    return c


@_hp
def tune_length(t, k, ch, target):
    """a copy of t with r0 of slot (ch, k) tuned until its length before the clamp is as close to `target` (bytes per
    sample) as one double allows"""
    def objective(c):
        s = c.slots[ch, k].tolist()
        kind, v = hp_raw_length(s[0], c.cands[k][1], c.bps, s[1:], c.order, gain=(s[2] if s[1] != 0.0 else None))
        return v if kind == "len" else D(-10 ** 6)
    return tune_r0(t, k, objective, D(target), ch=ch)


class _Cached:
    """edge costs of a table in high precision, recomputed for one candidate only"""

    def __init__(self, t):
        self.costs = [hp_edge_cost(t, k) for k in range(len(t.cands))]
        self.edges = [t.edge(k) for k in range(len(t.cands))]

    def adjacency(self, t, k):
        costs = list(self.costs)
        costs[k] = hp_edge_cost(t, k)
        return hp_adjacency(t, costs=costs), costs


@_hp
def near_tie(t, place, delta, others=1e-2):
    """A copy of the separated table t with one r0 tuned so that two costs that Dijkstra compares differ by `delta`
    (signed: second minus first), every other comparison left >= `others` apart.  place:
      "select": the two cheapest edges out of node 0, compared in the first selection round that has a choice;
      "relax":  the routes 0 -> 2 and 0 -> 1 -> 2, compared when node 1 relaxes node 2;
      "goal":   the goal and the cheapest node still unsettled in the round that settles the goal.
    Returns (table, gap of the tuned comparison as the model sees it) or None when this table does not lend itself to it."""
    cache = _Cached(t)
    nodes = t.nodes
    if place == "select":
        out0 = sorted((cache.costs[k], k) for k in range(len(t.cands)) if cache.edges[k][0] == 0 and cache.costs[k] is not None)
        if len(out0) < 2:
            return None
        first, k = out0[0][1], out0[1][1]

        def objective(c):
            return hp_edge_cost(c, k) - cache.costs[first]
    elif place == "relax":
        if nodes < 3:
            return None
        k01, k12, k = t.find(0, 1), t.find(1, 2), t.find(0, 2)

        def objective(c):
            return hp_edge_cost(c, k) - (cache.costs[k01] + cache.costs[k12])
    elif place == "goal":
        adj = hp_adjacency(t, costs=cache.costs)
        state = _final_state(adj, nodes)
        if state is None:
            return None
        cost, done, path = state
        open_nodes = sorted((cost[i], i) for i in range(nodes - 1) if not done[i] and cost[i] < D(BIG))
        if not open_nodes:
            return None
        m = open_nodes[0][1]
        k = t.find(path[m], m)
        goal_cost = cost[nodes - 1]

        def objective(c):
            a, _ = cache.adjacency(c, k)
            st = _final_state(a, nodes, stop_at_goal=False)
            return st[0][m] - goal_cost
    else:
        raise ValueError(place)
    tuned = tune_r0(t, k, objective, D(delta))
    if tuned is None:
        return None
    got = float(objective(tuned))
    tr = sorted(float(x[3]) for x in comparisons(hp_adjacency(tuned), nodes))
    if abs(got - delta) > 1e-11 or abs(tr[0] - abs(got)) > 1e-12 or (len(tr) > 1 and tr[1] < others) or clamp_distance(tuned) < 1e-6:
        return None
    return tuned, got


@_hp
def _final_state(adj, nodes, stop_at_goal=True):
    """(cost, done, path) at the moment the goal is selected (stop_at_goal) or with every reachable node settled"""
    big = D(BIG)
    cost = [big] * nodes
    done = [False] * nodes
    path = [NOPRED] * nodes
    cost[0] = D(0)
    for _ in range(nodes + 1):
        best, cur = big, None
        for i in range(nodes):
            if not done[i] and cost[i] < best:
                best, cur = cost[i], i
        if cur is None:
            return (cost, done, path) if not stop_at_goal else None
        if cur == nodes - 1 and stop_at_goal:
            return cost, done, path
        for i in range(nodes):
            a = adj[cur][i]
            if a is not None and cost[i] > a + cost[cur]:
                cost[i] = a + cost[cur]
                path[i] = cur
        done[cur] = True
    return cost, done, path
