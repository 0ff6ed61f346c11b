"""GPU tests of the autocorrelation sums where they are NOT exact: loud 24- and 32-bit material, the rounded regime the two
certificates exist for.  The reference is tests/acfmodel.py (correctly rounded sums of error-free products; its CPU tests are
tests/test_acf_error_model.py), the bounds are the roundings counted from the kernels' code, never measured ones:

  * block stage: sla_hip_launch_acf_blocks runs k_acf_blocks alone, in the instantiation the encoder runs, and shows r[0..order]:
        |r_kernel - r_exact| <= roundings_blocks(N) 2^-53 S_lag (1 + 1e-6) + ulp(r_exact)          for every lag <= order,
        |r_kernel - r_oracle| <= (N + 64) 2^-53 r_kernel[0]                                         (the certificate's premise;
    k_blocks_finish's delta allows the same or more: acfmodel.budget_blocks), rshift = the oracle's, slot element 0 untouched;
  * search stage: sla_hip_launch_search_exact_x shows the tile sums: P_t and X_t within roundings_tile 2^-53 S of the exact
    split, r[] of the whole window assembled as k_search_finish does within 48 2^-53 (sum of P_t[0]) of the exact sum (a window's
    own X is exactly zero, which is why 48 -- not the certificate's 64 -- holds here), sentinels beyond the window.

A pair dropped or doubled at a tile edge is off by about r0 / N, some 10^9 times these bounds; a wrong carry of the
pre-emphasis across a tile shows at lag 1.  measured() keeps the largest error / (2^-53 S) per kernel and length;
tests/tools/acf_error_bounds.py writes them to profiles/acf_error_bounds.txt (measurements: no assertion uses them).
"""
import ctypes as C
import math

import numpy as np
import pytest

import acfmodel as A
import slalibs as S

pytestmark = pytest.mark.gpu

XTILES = 16
SENTINEL = -7.25e100
U = A.U


class Group(C.Structure):                                       # sla_hip_lpc_group
    _fields_ = [("pcm_off", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


@pytest.fixture(scope="module")
def oracle():
    return S.oracle()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _groups_dev(groups):
    import torch
    return torch.frombuffer(bytearray(b"".join(bytes(g) for g in groups)), dtype=torch.uint8).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr())


_measured = {}


def measured():
    """{(stage, kernel, what, length): largest error / (2^-53 S)} of the launches this process has judged"""
    return _measured


def _keep(stage, kernel, what, n, value):
    key = (stage, kernel, what, n)
    _measured[key] = max(_measured.get(key, 0.0), float(value))


# ------------------------------------------------------------------ block stage

BLOCK_ORDERS = (8, 16, 18, 32, 31, 48, 51)                      # the seven instantiations: 12 / 17 / 20 / 33 / 36 / 49 / 52 live lags
_block_cache = {}


def block_reference(oracle, ms):
    """the layout of one launch (acfmodel.block_layout: every material x length x window x plane) and, per case, the exact sums,
    the oracle's serial sums and the oracle's quantiser shift.  Computed once per process and mid/side mode, never changed."""
    if "layout" not in _block_cache:
        _block_cache["layout"] = A.block_layout({n: oracle.window(1, n) for n in A.BLOCK_LENGTHS})
    pcm, pool, cases = _block_cache["layout"]
    if ms not in _block_cache:
        ref = []
        for c in cases:
            x = A.staged(pcm, c, pool[c.win_off:c.win_off + c.num_samples], ms)
            bw = oracle.bitwidth(A.int_samples(pcm, c, ms).astype(np.int32))
            ref.append((A.exact_lag_sums(x, 51, tiles=False), oracle.autocorr(x, 52), bw - 16 if bw > 16 else 0))
        _block_cache[ms] = ref
    return pcm, pool, cases, _block_cache[ms]


def launch_blocks(L, pcm, pool, cases, order, ms):
    import torch
    groups = [Group(c.pcm_off, c.num_samples, c.channel, c.win_off, c.int_shift, gi, 1, gi, 0) for gi, c in enumerate(cases)]
    ng = len(groups)
    d_pcm, d_g, d_w = _dev(pcm), _groups_dev(groups), _dev(pool)
    d_out = torch.full((ng * (order + 2),), SENTINEL, dtype=torch.float64, device="cuda")
    d_rs = torch.full((ng,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_acf_blocks(_p(d_pcm), C.c_uint64(pcm.shape[1]), ms, order, _p(d_g), ng, _p(d_w), _p(d_out), _p(d_rs), None)
    assert rc == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy().reshape(ng, order + 2), d_rs.cpu().numpy()


@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("order", BLOCK_ORDERS)
def test_block_sums_lie_within_their_roundings(hip, oracle, order, ms):
    pcm, pool, cases, ref = block_reference(oracle, ms)
    out, rshift = launch_blocks(hip.lib(), pcm, pool, cases, order, ms)
    kernel = "k_acf_blocks<%d,%d>" % A.instantiation(order)
    bad, inexact = [], 0
    for gi, (c, (ex, r_or, rs)) in enumerate(zip(cases, ref)):
        n, got = c.num_samples, out[gi, 1:]
        if out[gi, 0] != SENTINEL:
            bad.append(("slot element 0 written", gi, c))
        ok = A.within(got, ex.r[:order + 1], ex.S[:order + 1], A.roundings_blocks(n))
        if not ok.all():
            bad.append(("exact", c, np.nonzero(~ok)[0].tolist(), A.ratio(got, ex.r[:order + 1], ex.S[:order + 1]).max()))
        premise = np.abs(got - r_or[:order + 1]) <= (n + 64) * U * got[0]
        if not premise.all():
            bad.append(("premise", c, np.nonzero(~premise)[0].tolist()))
        if int(rshift[gi]) != rs:
            bad.append(("rshift", c, int(rshift[gi]), rs))
        inexact += int((got != ex.r[:order + 1]).sum())
        _keep("block", kernel, "r", n, A.ratio(got, ex.r[:order + 1], ex.S[:order + 1]).max())
        _keep("block", "oracle", "r", n, A.ratio(r_or[:order + 1], ex.r[:order + 1], ex.S[:order + 1]).max())
    assert not bad, bad[:8]
    assert inexact > len(cases)                                   # the rounded regime: these sums are not the exact ones bit for bit


def test_order_52_is_refused_without_writing(hip, oracle):
    import torch
    pcm, pool, cases, _ = block_reference(oracle, 0)
    L = hip.lib()
    groups = [Group(c.pcm_off, c.num_samples, c.channel, c.win_off, c.int_shift, gi, 1, gi, 0) for gi, c in enumerate(cases[:4])]
    d_pcm, d_g, d_w = _dev(pcm), _groups_dev(groups), _dev(pool)
    d_out = torch.full((4 * 54,), SENTINEL, dtype=torch.float64, device="cuda")
    d_rs = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_acf_blocks(_p(d_pcm), C.c_uint64(pcm.shape[1]), 0, 52, _p(d_g), 4, _p(d_w), _p(d_out), _p(d_rs), None)
    assert rc == 3                                                # SLA_APIRESULT_EXCEED_HANDLE_CAPACITY
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all() and (d_rs.cpu().numpy() == 77).all()


# ------------------------------------------------------------------ search stage

SEARCH_ORDERS = (16, 32, 48, 15, 51, 8)                        # (8: k_acf_tiles<3>, the 12-lag kernel with partners by DPP)
SEARCH_LENGTHS = (1, 1023, 1024, 1025, 2049, 4096, 16384)
SEARCH_OFFSETS = (0, 1, 3)
SEARCH_MATERIAL = {24: ("nyquist", "coloured"), 32: ("dc", "uniform", "coloured")}
FRONT = 16
_search_cache = {}


def search_reference(bits, ms):
    """one launch's PCM (a segment per material), its cases (material x length x offset x plane) and their exact tile split"""
    key = (bits, ms)
    if key not in _search_cache:
        seg = FRONT + max(SEARCH_OFFSETS) + max(SEARCH_LENGTHS) + 64
        kinds = SEARCH_MATERIAL[bits]
        pcm = np.concatenate([A.material(k, bits, seg, seed=2) for k in kinds], axis=1)
        cases = [A.Case(mi * seg + FRONT + off, n, ch, 0xFFFFFFFF, 32 - bits, k, bits, None)
                 for mi, k in enumerate(kinds) for n in SEARCH_LENGTHS for off in SEARCH_OFFSETS for ch in (0, 1)]
        ref = [A.exact_lag_sums(A.staged(pcm, c, None, ms), 51) for c in cases]
        _search_cache[key] = (pcm, cases, ref)
    return _search_cache[key]


def launch_search(L, pcm, cases, order, ms, bits):
    import torch
    lags = L.sla_hip_search_exact_lags(order)
    groups = [Group(c.pcm_off, c.num_samples, c.channel, 0xFFFFFFFF, c.int_shift, gi, 1, gi, 0) for gi, c in enumerate(cases)]
    ng = len(groups)
    d_pcm, d_g = _dev(pcm), _groups_dev(groups)
    d_c = _dev(np.array([(0, c.num_samples) for c in cases], np.uint32))
    d_ts = torch.full((ng * XTILES * 2 * lags,), SENTINEL, dtype=torch.float64, device="cuda")
    d_out = torch.zeros(ng * (order + 2), dtype=torch.float64, device="cuda")
    limit = 2.0 ** (53 + 2 * ((32 - bits) - 31 - ms))           # the encoder's exactness limit for this width
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_search_exact_x(_p(d_pcm), C.c_uint64(pcm.shape[1]), ms, order, _p(d_g), ng, max(SEARCH_LENGTHS), 1,
                                         _p(d_c), _p(d_ts), _p(d_out), C.c_double(limit), C.c_double(64.0), None, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    return d_ts.cpu().numpy().reshape(ng, XTILES, 2, lags), limit


@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("order", SEARCH_ORDERS)
def test_tile_sums_lie_within_their_roundings(hip, order, ms):
    lags, top = A.instantiation(order)
    kernel = "k_acf_tiles<%d,%d>" % (lags, top) if lags == 12 else "k_acf_tiles_lds<%d,%d>" % (lags, top)
    x_count = np.array([A.roundings_tile(lags, top, lag, "X") for lag in range(order + 1)])
    bad, inexact, over = [], 0, 0
    for bits in (24, 32):
        pcm, cases, ref = search_reference(bits, ms)
        ts, limit = launch_search(hip.lib(), pcm, cases, order, ms, bits)
        for gi, (c, ex) in enumerate(zip(cases, ref)):
            n = c.num_samples
            nt = (n + A.XTILE - 1) // A.XTILE
            P, X = ts[gi, :nt, 0, :order + 1], ts[gi, :nt, 1, :order + 1]
            eP, eX, sP, sX = (a[:, :order + 1] for a in (ex.P, ex.X, ex.SP, ex.SX))
            p_count = np.array([[A.roundings_tile(lags, top, 0, "P", min(A.XTILE, n - t * A.XTILE))] for t in range(nt)])
            okP, okX = A.within(P, eP, sP, p_count), A.within(X, eX, sX, x_count[None, :])
            if not okP.all():
                bad.append(("P", c, np.argwhere(~okP)[:4].tolist(), A.ratio(P, eP, sP).max()))
            if not okX.all():
                bad.append(("X", c, np.argwhere(~okX)[:4].tolist(), A.ratio(X, eX, sX).max()))
            if not (ts[gi, nt:] == SENTINEL).all():
                bad.append(("tiles beyond the window", c))
            # r[] of the whole window as k_search_finish assembles it: P over the tiles in order, minus X of the last tile
            r = np.zeros(order + 1)
            for t in range(nt):
                r = r + P[t]
            r = r - X[nt - 1]
            energy = float(np.add.reduce(P[:, 0]))
            if not (np.abs(r - ex.r[:order + 1]) <= 48.0 * U * energy).all():
                bad.append(("window", c, A.ratio(r, ex.r[:order + 1], np.full(order + 1, energy)).max()))
            # a candidate that ends inside the window gives X back: tiles 0 .. k minus X_k, against the same combination of the
            # exact split (k + 2 correctly rounded values, whose magnitudes add up to at most 1.5 energies, summed by math.fsum
            # and rounded once more: at most 3 roundings away from the exact sum), in units of the window's energy -- the derived
            # count of the candidate, which the certificate's 64 covers
            for k in range(nt - 1):
                rk = np.zeros(order + 1)
                for t in range(k + 1):
                    rk = rk + P[t]
                rk = rk - X[k]
                ek = np.array([math.fsum(list(eP[:k + 1, lag]) + [-eX[k, lag]]) for lag in range(order + 1)])
                allowed = np.array([A.roundings_window(lags, top, lag, k + 1) + 3 for lag in range(order + 1)])
                assert allowed.max() <= A.SEARCH_BUDGET + 3
                if not (np.abs(rk - ek) <= allowed * U * energy).all():
                    bad.append(("candidate of %d tiles" % (k + 1), c, (np.abs(rk - ek) / (U * energy)).max()))
            inexact += int((P != eP).sum())
            over += int(energy >= limit)
            _keep("search", kernel, "P", n, A.ratio(P, eP, sP).max())
            _keep("search", kernel, "X", n, A.ratio(X, eX, sX).max())
            _keep("search", kernel, "window / energy", n, A.ratio(r, ex.r[:order + 1], np.full(order + 1, energy)).max())
    assert not bad, bad[:8]
    assert inexact > 1000 and over > 100                          # rounded sums, windows over the exactness limit
