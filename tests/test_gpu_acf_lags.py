"""GPU tests of the autocorrelation kernels that only compute the lags somebody reads (kernels/search.inc: k_acf_tiles_lds<NB, TOP>,
k_acf_blocks<NB, TOP, MS>; TOP = order + 1 at the orders 16 / 32 / 48, the full lag blocks everywhere else) and that fetch whole
tiles without per-sample guards.  Three things must hold:

  * tile sums: on 16-bit material (every product and sum exact in a double) P_t[lag] and X_t[lag] are the integers Python
    computes, for every lag <= order, at window lengths around every tile and sub-tile boundary and at unaligned starts,
    with non-zero samples on both sides of every window (a dropped guard shows as a wrong sum);
  * consumers: k_search_cert, k_plan and the block stage, launched by hand on loud 24-bit material, arrive at the encoder's and
    the oracle's partition, codes, kint and rshift;
  * block slots: what sla_hip_launch_lpc_blocks_cert leaves for the chosen blocks is, bit for bit, what the build before this
    change left (tests/golden/unit_acf_block_slots.npz, recorded from our own kernels at that commit).  The launcher runs
    k_blocks_finish right behind k_acf_blocks, so the slot shows r[0] itself and r[1..order] through the reflection
    coefficients that a fixed sequence of operations makes of them (plus codes, kint, rshift and the certificate's verdict):
    r[] is compared as far as the launcher lets anybody see it.
"""
import ctypes as C
import os

import numpy as np
import pytest

import slalibs as S

pytestmark = pytest.mark.gpu

XTILE, XTILES, NODES = 1024, 16, 17
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unit_acf_block_slots.npz")


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


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


# ------------------------------------------------------------------ tile sums against exact integers

LENGTHS = (1, 35, 255, 256, 257, 1023, 1024, 1025, 2049, 4096)
OFFSETS = (0, 1, 3, 4099)
MARGIN = 512                     # samples in front of pcm_off = 0 and behind the longest window: noise, inside the allocation
PLANE = MARGIN + max(OFFSETS) + max(LENGTHS) + MARGIN


def _noise16(seed):
    """two planes of 16-bit noise, left-justified in int32, never zero"""
    rng = np.random.default_rng(seed)
    q = rng.integers(-32768, 32768, (2, PLANE), dtype=np.int64)
    q[q == 0] = 1
    return q


@pytest.fixture(scope="module")
def noise():
    q = _noise16(7)
    return q, _dev((q << 16).astype(np.int32))


def _expected_tiles(w, order, scale):
    """P_t[lag], X_t[lag] of window w (Python integers in int64: |sum| < 2^47), as doubles"""
    n = len(w)
    ntiles = (n + XTILE - 1) // XTILE
    P = np.zeros((ntiles, order + 1), np.int64)
    X = np.zeros((ntiles, order + 1), np.int64)
    for lag in range(min(order, n - 1) + 1):
        prod = w[:n - lag] * w[lag:]                             # indexed by the pair's first sample
        for t in range(ntiles):
            t0, t1 = t * XTILE, min((t + 1) * XTILE, n)
            hi = min(t1, n - lag)
            P[t, lag] = prod[t0:hi].sum() if hi > t0 else 0
            lo = max(t0, t1 - lag)
            X[t, lag] = prod[lo:hi].sum() if hi > lo else 0
    return P.astype(np.float64) * scale, X.astype(np.float64) * scale


@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("order", [16, 32, 48, 15, 18, 31, 49, 51])
def test_tile_sums_are_the_exact_integers(hip, noise, order, ms):
    import torch
    L = hip.lib()
    lags = L.sla_hip_search_exact_lags(order)
    q, d_pcm = noise
    nch = 2 if ms else 1
    cases = [(n, off, ch) for n in LENGTHS for off in OFFSETS for ch in range(nch)]
    groups = [Group(off, n, ch, 0xFFFFFFFF, 16, gi, 1, gi, 0) for gi, (n, off, ch) in enumerate(cases)]
    cands = np.array([(0, n) for n, _, _ in cases], np.uint32)
    d_g, d_c = _groups_dev(groups), _dev(cands)
    sentinel = -7.25e100
    d_ts = torch.full((len(cases) * XTILES * 2 * lags,), sentinel, dtype=torch.float64, device="cuda")
    d_out = torch.zeros(len(cases) * (order + 2), dtype=torch.float64, device="cuda")
    limit = 2.0 ** (53 + 2 * (16 - 31 - ms))                    # the encoder's exactness limit for 16-bit material: every window is exact
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_search_exact_x(_p(d_pcm, 4 * MARGIN), C.c_uint64(PLANE), ms, order, _p(d_g), len(cases), max(LENGTHS), 1,
                                         _p(d_c), _p(d_ts), _p(d_out), C.c_double(limit), C.c_double(64.0), None, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    ts = d_ts.cpu().numpy().reshape(len(cases), XTILES, 2, lags)
    if ms:
        x = [q[0] + q[1], q[0] - q[1]]                          # mid = (l + r) / 2 in units of 2^-16, side = l - r in units of 2^-15
        scale = [2.0 ** -32, 2.0 ** -30]
    else:
        x, scale = [q[0]], [2.0 ** -30]
    for gi, (n, off, ch) in enumerate(cases):
        w = x[ch][MARGIN + off:MARGIN + off + n]
        P, X = _expected_tiles(w, order, scale[ch])
        nt = P.shape[0]
        got_p, got_x = ts[gi, :nt, 0, :order + 1] + 0.0, ts[gi, :nt, 1, :order + 1] + 0.0      # (+ 0.0: one sign of zero)
        assert np.array_equal(got_p.view(np.uint64), P.view(np.uint64)), ("P", order, ms, n, off, ch)
        assert np.array_equal(got_x.view(np.uint64), X.view(np.uint64)), ("X", order, ms, n, off, ch)
        assert (ts[gi, nt:] == sentinel).all(), ("tiles beyond the window", order, ms, n, off, ch)


def test_order_51_is_the_last_with_tile_sums(hip, noise):
    """the widest kernels compute 52 lags, 0 .. 51: order 51 is the last they serve.  At order 52 sla_hip_search_exact_lags says
    0, and both launchers that need the sums refuse the call before anything is launched or written (the encoder then takes the
    serial chains: tests/test_gpu_high_orders.py)"""
    import torch
    L = hip.lib()
    assert [L.sla_hip_search_exact_lags(o) for o in (48, 49, 51, 52, 53, 64, 255)] == [52, 52, 52, 0, 0, 0, 0]
    order, n, sentinel = 52, 4096, -7.25e100
    _, d_pcm = noise
    d_g, d_c = _groups_dev([Group(0, n, 0, 0xFFFFFFFF, 16, 0, 1, 0, 0)]), _dev(np.array([(0, n)], np.uint32))
    d_ts = torch.full((XTILES * 2 * 56,), sentinel, dtype=torch.float64, device="cuda")
    d_out = torch.full((order + 2,), sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_search_exact_x(_p(d_pcm, 4 * MARGIN), C.c_uint64(PLANE), 0, order, _p(d_g), 1, n, 1, _p(d_c), _p(d_ts), _p(d_out),
                                         C.c_double(2.0 ** 23), C.c_double(64.0), None, None, None)
    assert rc == 3                                                # SLA_APIRESULT_EXCEED_HANDLE_CAPACITY
    d_w = _dev(np.ones(n))
    d_i = [torch.full((order + 1,), 77, dtype=torch.int32, device="cuda") for _ in range(6)]
    d_wg = _groups_dev([Group(0, n, 0, 0, 16, 0, 1, 0, 0)])
    rc = L.sla_hip_launch_lpc_blocks_cert_x(_p(d_pcm, 4 * MARGIN), C.c_uint64(PLANE), 0, order, _p(d_wg), 1, n, _p(d_c), _p(d_w), _p(d_out),
                                            _p(d_i[0]), _p(d_i[1]), _p(d_i[2]), _p(d_i[3]), _p(d_i[4]), _p(d_i[5]), C.c_double(16.0), 16, None, None)
    assert rc == 3
    torch.cuda.synchronize()
    assert (d_ts.cpu().numpy() == sentinel).all() and (d_out.cpu().numpy() == sentinel).all()
    assert all((t.cpu().numpy() == 77).all() for t in d_i)


# ------------------------------------------------------------------ consumers agree

def _encode(hip, p, pcm):
    enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    try:
        enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
        enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method, p.window_type, p.max_block_samples)
        enc.set_option("stream", 0)
        data = enc.encode_whole(pcm)
        return data, enc.trace()
    finally:
        enc.close()


def consumers(hip, oracle, order, maxb, nch, ms, seed):
    """the search (tile sums, k_search_cert), k_plan and the block stage launched by hand on two super-frames of loud 24-bit
    material, beside the encoder's own analysis and the oracle's.  Returns (plan status per super-frame, mismatches)."""
    import torch
    L = hip.lib()
    bits, n = 24, 2 * maxb
    pcm = S.synth_pcm(nch, n, bits, seed=seed)
    p = S.make_params(nch, bits, 48000, order, 3, 8, ms, 1, maxb, cap=(nch, maxb, order, 3, 8))
    ret, want, to = oracle.encode_trace(p, pcm)
    assert ret == 0
    data, tr = _encode(hip, p, pcm)
    nb = to.num_blocks
    bad = []
    if data != want or tr.num_blocks != nb:
        bad.append("encoder bytes")
    lags = L.sla_hip_search_exact_lags(order)
    # the encoder's candidate lattice: starts on multiples of 1024, lengths from 2048 to the window
    nodes = maxb // XTILE + 1
    cands = [(i * XTILE, (j - i) * XTILE) for i in range(nodes) for j in range(i + 1, nodes) if (j - i) * XTILE >= 2048]
    nc = len(cands)
    groups = [Group(sf * maxb, maxb, ch, 0xFFFFFFFF, 32 - bits, 0, nc, (sf * nch + ch) * nc, 0) for sf in range(2) for ch in range(nch)]
    d_pcm, d_g, d_c = _dev(pcm), _groups_dev(groups), _dev(np.array(cands, np.uint32))
    d_ts = torch.zeros(len(groups) * XTILES * 2 * lags, dtype=torch.float64, device="cuda")
    d_out = torch.zeros(len(groups) * nc * (order + 2), dtype=torch.float64, device="cuda")
    d_any = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_parts = torch.zeros(2 * NODES, dtype=torch.int32, device="cuda")
    d_np = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_st = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    ntz = 32 - bits
    limit = 2.0 ** (53 + 2 * (ntz - 31 - ms))
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_search_exact_x(_p(d_pcm), C.c_uint64(n), ms, order, _p(d_g), len(groups), maxb, nc, _p(d_c), _p(d_ts), _p(d_out),
                                         C.c_double(limit), C.c_double(64.0), _p(d_any), None, None)
    assert rc == 0
    rc = L.sla_hip_launch_plan(_p(d_g), 2, nch, order, bits, _p(d_c), _p(d_out), _p(d_parts), _p(d_np), _p(d_st), None)
    assert rc == 0
    torch.cuda.synchronize()
    energy = d_ts.cpu().numpy().reshape(len(groups), XTILES, 2 * lags)[:, :maxb // XTILE, 0].sum(axis=1)
    assert (energy >= limit).all(), "the material is meant to take the certified route"
    status = d_st.cpu().numpy().tolist()
    parts = d_parts.cpu().numpy().reshape(2, NODES)
    nparts = d_np.cpu().numpy()
    blocks = []
    for sf in range(2):
        pos = sf * maxb
        for k in range(int(nparts[sf]) if status[sf] == 0 else 0):
            blocks.append((pos, int(parts[sf, k])))
            pos += int(parts[sf, k])
    if blocks != [(int(to.blk_start[b]), int(to.blk_nsmpl[b])) for b in range(nb)]:
        bad.append("partition against the oracle")
    if blocks != [(int(tr.blk_start[b]), int(tr.blk_nsmpl[b])) for b in range(tr.num_blocks)]:
        bad.append("partition against the encoder")
    if bad or not blocks:
        return status, bad
    # the block stage on the planned blocks
    lens = sorted({ln for _, ln in blocks})
    woff, pool = {}, []
    for ln in lens:
        woff[ln] = sum(len(w) for w in pool)
        pool.append(oracle.window(p.window_type, ln))
    bgroups = [Group(s, ln, ch, woff[ln], 32 - bits, b * nch + ch, 1, b * nch + ch, 0) for b, (s, ln) in enumerate(blocks) for ch in range(nch)]
    bcands = np.array([(0, ln) for _, ln in blocks for _ in range(nch)], np.uint32)
    ng, O1 = len(bgroups), order + 1
    d_bg, d_bc, d_w = _groups_dev(bgroups), _dev(bcands), _dev(np.concatenate(pool))
    d_bo = torch.zeros(ng * (order + 2), dtype=torch.float64, device="cuda")
    d_code = torch.zeros(ng * O1, dtype=torch.int32, device="cuda")
    d_kint = torch.zeros(ng * O1, dtype=torch.int32, device="cuda")
    d_rs = torch.zeros(ng, dtype=torch.int32, device="cuda")
    d_flag = torch.zeros(ng, dtype=torch.int32, device="cuda")
    d_fl = torch.zeros(ng, dtype=torch.int32, device="cuda")
    d_fc = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_lpc_blocks_cert_x(_p(d_pcm), C.c_uint64(n), ms, order, _p(d_bg), ng, max(lens), _p(d_bc), _p(d_w), _p(d_bo), _p(d_code),
                                            _p(d_kint), _p(d_rs), _p(d_flag), _p(d_fl), _p(d_fc), C.c_double(16.0), bits, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    code = d_code.cpu().numpy().reshape(len(blocks), nch, O1)
    kint = d_kint.cpu().numpy().reshape(len(blocks), nch, O1)
    rshift = d_rs.cpu().numpy().view(np.uint32).reshape(len(blocks), nch)
    comp = to.blk_type[:nb] == 0
    for name, got, ref_o, ref_e in (("code", code, to.code, tr.code), ("kint", kint, to.kint, tr.kint), ("rshift", rshift, to.rshift, tr.rshift)):
        if not np.array_equal(got[comp], ref_o[:nb][comp]):
            bad.append(name + " against the oracle")
        if not np.array_equal(got[comp], ref_e[:nb][comp]):
            bad.append(name + " against the encoder")
    if not comp.any():
        bad.append("no compressed block")
    return status, bad


CONSUMER_CASES = [(32, 4096, 2, 1, 12345), (48, 8192, 1, 0, 12345), (49, 4096, 2, 1, 12345), (51, 8192, 1, 0, 12345)]


@pytest.mark.parametrize("order,maxb,nch,ms,seed", CONSUMER_CASES)
def test_consumers_agree(hip, oracle, order, maxb, nch, ms, seed):
    status, bad = consumers(hip, oracle, order, maxb, nch, ms, seed)
    assert status == [0, 0], status          # k_plan decided both super-frames from the certified sums
    assert not bad, bad


# ------------------------------------------------------------------ block slots against the build before

BLOCK_LENGTHS = (1, 255, 256, 257, 1000, 4096, 8192)
BLOCK_ORDERS = (8, 16, 31, 32, 48, 51)
BLOCK_PLANE = 16 + len(BLOCK_LENGTHS) * 2 * 11 + max(BLOCK_LENGTHS) + MARGIN


def _coloured(bits, seed):
    """two planes of coloured integer noise over a slow triangle (integer arithmetic only: the same samples on every
    machine), left-justified in int32"""
    rng = np.random.default_rng(seed)
    n = BLOCK_PLANE
    a = 1 << (bits - 3)
    e = rng.integers(-a, a, (2, n + 2), dtype=np.int64)
    t = np.arange(n, dtype=np.int64)
    tri = np.abs((t * 37) % (4 * a) - 2 * a) - a                 # period 4a / 37 samples, amplitude a
    q = (2 * e[:, 2:] + 3 * e[:, 1:-1] + e[:, :-2]) // 2 + np.stack([tri, -tri // 2])
    full = 1 << (bits - 1)
    q = np.clip(q, -full, full - 1)
    return (q << (32 - bits)).astype(np.int32)


def sine_windows(oracle):
    return {n: oracle.window(1, n) for n in BLOCK_LENGTHS}


def block_slots(L, sine, order, ms, bits):
    """one sla_hip_launch_lpc_blocks_cert over every (length, window, channel).  Returns the arrays the launch leaves."""
    import torch
    nch = 2 if ms else 1
    pcm = _coloured(bits, 100 * order + 10 * ms + bits)
    pool, woff = [], {}
    for kind in ("rect", "sine"):
        for n in BLOCK_LENGTHS:
            woff[kind, n] = sum(len(w) for w in pool)
            pool.append(np.ones(n) if kind == "rect" else sine[n])
    cases = [(n, kind, ch) for kind in ("rect", "sine") for n in BLOCK_LENGTHS for ch in range(nch)]
    groups = [Group(16 + 11 * (gi // nch), n, ch, woff[kind, n], 32 - bits, gi, 1, gi, 0) for gi, (n, kind, ch) in enumerate(cases)]
    cands = np.array([(0, n) for n, _, _ in cases], np.uint32)
    ng, O1 = len(cases), order + 1
    d_pcm, d_g, d_c, d_w = _dev(pcm), _groups_dev(groups), _dev(cands), _dev(np.concatenate(pool))
    d_out = torch.zeros(ng * (order + 2), dtype=torch.float64, device="cuda")
    d_code = torch.zeros(ng * O1, dtype=torch.int32, device="cuda")
    d_kint = torch.zeros(ng * O1, dtype=torch.int32, device="cuda")
    d_rs = torch.zeros(ng, dtype=torch.int32, device="cuda")
    d_flag = torch.zeros(ng, dtype=torch.int32, device="cuda")
    d_fl = torch.zeros(ng, dtype=torch.int32, device="cuda")
    d_fc = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_lpc_blocks_cert_x(_p(d_pcm), C.c_uint64(BLOCK_PLANE), ms, order, _p(d_g), ng, max(BLOCK_LENGTHS), _p(d_c), _p(d_w),
                                            _p(d_out), _p(d_code), _p(d_kint), _p(d_rs), _p(d_flag), _p(d_fl), _p(d_fc), C.c_double(16.0), bits, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    return {"out": d_out.cpu().numpy().view(np.uint64), "code": d_code.cpu().numpy(), "kint": d_kint.cpu().numpy(), "rshift": d_rs.cpu().numpy(),
            "flag": d_flag.cpu().numpy(), "redone": d_fc.cpu().numpy()[:1]}


def block_key(order, ms, bits, name):
    return "o%d_ms%d_b%d_%s" % (order, ms, bits, name)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("order", BLOCK_ORDERS)
def test_block_slots_are_the_parents(hip, golden, order, ms, bits):
    sine = {n: golden["sine_%d" % n] for n in BLOCK_LENGTHS}     # the windows the values were recorded with
    got = block_slots(hip.lib(), sine, order, ms, bits)
    for name, a in got.items():
        assert np.array_equal(a, golden[block_key(order, ms, bits, name)]), (name, order, ms, bits)
