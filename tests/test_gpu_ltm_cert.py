"""GPU tests of the long-term stage's certified route (option "ltm_cert", k_ltm_acf_fast + k_ltm_solve_cert): the
autocorrelation comes from an any-order FMA transform of at most half the reference's size, every decision taken from
it is certified against an error bound, and what is not certified goes through the exact kernels from a device list.
What must hold: bytes, pitch and quantised taps are the oracle's with the route on and off; ordinary material is
certified (>= 99 % of the jobs -- the tests must not pass by falling back); every audited job agrees with the exact
kernels; crafted dense residuals that cannot be decided (two exactly tied largest peaks; a tap within 1e-12 code steps of a
rounding boundary of the quantiser, at 1, 3 and 5 taps; an autocorrelation value of exactly zero) fall back for that
reason and still give the exact result."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import slalibs as S
import waveforms as W

pytestmark = pytest.mark.gpu

ORDINARY = ("white", "gauss", "music")


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


def encode(hip, p, pcm, **options):
    enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    try:
        enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
        enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method,
                                 p.window_type, p.max_block_samples)
        for k, v in options.items():
            enc.set_option(k, v)
        data = enc.encode_whole(pcm)
        return data, enc.trace(), enc.last_ltm_cert()
    finally:
        enc.close()


def material(name, nch, n, bits, seed):
    if name == "music":
        return W.music_like(nch, n, bits, seed=seed + 1)
    if name == "pitched":
        rng = np.random.default_rng(seed)
        base = rng.integers(-6000, 6000, 131)
        x = np.stack([np.tile(np.roll(base, 7 * ch), n // 131 + 1)[:n] + rng.integers(-300, 300, n) for ch in range(nch)])
        return np.ascontiguousarray((x.astype(np.int64) << (32 - 16)).astype(np.int32)) if bits == 16 else \
            np.ascontiguousarray((x.astype(np.int64) << (32 - 24 + 6)).astype(np.int32))
    return W.gen(name, nch, n, bits, seed=seed)


def run_case(hip, oracle, name, nch, bits, ms, taps, max_block, n, seed, chunks):
    pcm = material(name, nch, n, bits, seed)
    p = S.make_params(nch, bits, 48000, parcor=16, ltm=taps, lms=8, ms=ms, max_block=max_block,
                      cap=(nch, max_block, 16, taps, 8))
    ret, want, to = oracle.encode_trace(p, pcm)
    assert ret == 0
    nb = to.num_blocks
    exact, tr0, st0 = encode(hip, p, pcm, ltm_cert=0, chunks=chunks)
    assert st0 == (0, 0, 0, 0, 0)
    got, tr1, st = encode(hip, p, pcm, ltm_cert=1, cert_audit=1, chunks=chunks)
    jobs, certified, fallback, audit_ok, audit_bad = st
    print("%-8s nch %d bits %2d ms %d taps %d block %5d n %6d chunks %d: jobs %d certified %d fallback %d audit %d/%d"
          % (name, nch, bits, ms, taps, max_block, n, chunks, jobs, certified, fallback, audit_ok, audit_bad))
    assert exact == want and got == want
    comp = to.blk_type[:nb] == 0
    for tr in (tr0, tr1):
        assert np.array_equal(tr.pitch[:nb][comp], to.pitch[:nb][comp])
        assert np.array_equal(tr.ltm_coef[:nb][comp], to.ltm_coef[:nb][comp])
    assert audit_bad == 0
    assert certified + fallback == jobs and audit_ok == certified
    return jobs, certified, fallback


@pytest.mark.parametrize("taps", [1, 3, 5])
@pytest.mark.parametrize("name", ORDINARY)
def test_ordinary_material_is_certified(hip, oracle, name, taps):
    """white / gauss / music_like at 16 and 24 bits, mono and mid/side, block capacities 2048 .. 16384, a ragged last block
    shorter than 257 + taps samples, one and three chunks: the oracle's bytes, pitch and taps; every audited job equal;
    at least 99 % of the jobs certified (a short last block may fall back: lags beyond its end are rounding noise)."""
    total = cert = 0
    for i, (max_block, bits, nch, ms, chunks) in enumerate([(2048, 16, 1, 0, 1), (4096, 24, 2, 1, 3), (8192, 16, 2, 1, 1),
                                                            (16384, 24, 1, 0, 1)]):
        n = 150 * max_block + 100 + 37 * taps                 # ragged tail of 100 + 37 taps < 257 + taps samples
        jobs, certified, fallback = run_case(hip, oracle, name, nch, bits, ms, taps, max_block, n, 10 * taps + i, chunks)
        assert jobs > 0
        total += jobs
        cert += certified
    assert cert >= 0.99 * total, (cert, total)


@pytest.mark.parametrize("name", ["silence", "sine", "posconst", "nyquist", "chirp", "pitched"])
def test_degenerate_and_pitched_material(hip, oracle, name):
    """the families that leave near-zero residuals, and a strongly pitched signal: bytes, pitch and taps only (they may
    fall back as they like)"""
    for taps, bits, nch, ms in ((1, 16, 1, 0), (3, 24, 2, 1), (5, 16, 2, 1)):
        run_case(hip, oracle, name, nch, bits, ms, taps, 4096, 50000 + 123, 3, 1 if taps != 3 else 3)


# ---- the launcher on crafted residuals ----------------------------------------------------------------------------

class Group(C.Structure):
    _fields_ = [("pcm_off", C.c_uint64)] + [(nm, C.c_uint32) for nm in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


class Job(C.Structure):
    _fields_ = [("blk_off", C.c_uint64), ("blk_len", C.c_uint32), ("channel", C.c_uint32), ("pitch", C.c_uint32),
                ("ltm_coef", C.c_int32 * 5), ("pad_", C.c_uint32 * 2)]


class AcfJob(C.Structure):
    _fields_ = [("blk_off", C.c_uint64), ("blk_len", C.c_uint32), ("channel", C.c_uint32)]


def launch_both(hip, blocks, ntaps, fft_size=8192, scratch=None, scratch_slots=0):
    """the certified launcher and the exact pair (sla_hip_launch_ltm_acf + sla_hip_launch_ltm_solve) on the same residual
    blocks: (jobs of the certified call, jobs of the exact pair, counters).  scratch: a device tensor of scratch_slots x
    fft_size doubles for the transform sizes that do not fit the LDS."""
    import torch
    L = hip.lib()
    n = len(blocks)
    stride = max(len(b) for b in blocks)
    plane = np.zeros(n * stride, np.int32)
    aj, gr = (AcfJob * n)(), (Group * n)()
    for i, b in enumerate(blocks):
        plane[i * stride:i * stride + len(b)] = b
        aj[i] = AcfJob(i * stride, len(b), 0)
        gr[i] = Group(i * stride, len(b), 0, 0, 0, 0, 1, i, 0)
    L.slai_fft_plan_create.restype = C.c_void_p
    L.slai_fft_plan_create.argtypes = [C.c_uint32]
    L.slai_fft_plan_export.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.slai_fft_plan_destroy.argtypes = [C.c_void_p]
    L.sla_hip_ltm_fast_twiddles.argtypes = [C.c_uint32, C.POINTER(C.c_double)]
    tw = np.zeros(6 * fft_size)
    plan = L.slai_fft_plan_create(fft_size)
    L.slai_fft_plan_export(plan, tw.ctypes.data_as(C.POINTER(C.c_double)))
    L.slai_fft_plan_destroy(plan)
    ftw = np.zeros(6 * fft_size)
    assert L.sla_hip_ltm_fast_twiddles(fft_size, ftw.ctypes.data_as(C.POINTER(C.c_double))) == 0
    d_res = torch.from_numpy(plane).cuda()
    d_aj = torch.frombuffer(bytearray(bytes(aj)), dtype=torch.uint8).cuda()
    d_gr = torch.frombuffer(bytearray(bytes(gr)), dtype=torch.uint8).cuda()
    d_tw, d_ftw = torch.from_numpy(tw).cuda(), torch.from_numpy(ftw).cuda()
    d_rec = torch.zeros(12 * n, dtype=torch.float64, device="cuda")
    d_eps = torch.zeros(n, dtype=torch.float64, device="cuda")
    d_list = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_jobs = torch.full((n * C.sizeof(Job),), 0xAB, dtype=torch.uint8, device="cuda")
    d_jobs2 = torch.full((n * C.sizeof(Job),), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    d_scr = vp(scratch) if scratch is not None else None
    L.sla_hip_launch_ltm_cert_x.restype = C.c_int
    rc = L.sla_hip_launch_ltm_cert_x(vp(d_res), C.c_uint64(len(plane)), vp(d_aj), vp(d_gr), C.c_uint32(n), C.c_uint32(fft_size),
                                     vp(d_tw), vp(d_ftw), d_scr, C.c_uint32(scratch_slots), vp(d_rec), vp(d_eps), C.c_uint32(ntaps),
                                     C.c_double(16.0), vp(d_jobs), vp(d_list), vp(d_cnt), None, None)
    assert rc == 0
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy().copy()
    eps = d_eps.cpu().numpy().copy()
    lst = d_list.cpu().numpy().copy()
    rc = L.sla_hip_launch_ltm_acf(vp(d_res), C.c_uint64(len(plane)), vp(d_aj), C.c_uint32(n), C.c_uint32(fft_size), vp(d_tw), d_scr,
                                  C.c_uint32(scratch_slots), vp(d_rec), C.c_uint32(12), None)
    assert rc == 0
    rc = L.sla_hip_launch_ltm_solve(vp(d_rec), vp(d_gr), C.c_uint32(n), C.c_uint32(ntaps), vp(d_jobs2), None)
    assert rc == 0
    torch.cuda.synchronize()
    a = (Job * n).from_buffer_copy(d_jobs.cpu().numpy().tobytes())
    b = (Job * n).from_buffer_copy(d_jobs2.cpu().numpy().tobytes())
    return a, b, cnt, eps, lst


NL = 262
EPS_REL = 1.5e-12          # about the built-in eps / r[0] at F = 8192


def acf_int(x, lags):
    x = x.astype(np.int64)
    n = len(x)
    assert int(np.abs(x).max()) ** 2 * n < 2 ** 62
    return {k: int(np.dot(x[:n - k], x[k:])) for k in lags}


def dense_margins_ok(x, factor=1e3):
    """every sign and neighbour comparison of the lags 0 .. 259 clear of the bound by `factor`"""
    r = acf_int(x, range(NL))
    lim = factor * 2 * EPS_REL * r[0]
    return all(abs(r[j]) > lim for j in range(260)) and all(abs(r[j] - r[j - 1]) > lim for j in range(1, 260))


def background(n, seed, period, amp=2.0 ** 19):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(period)
    x = amp * (rng.standard_normal(n) + 0.9 * np.tile(base, n // period + 1)[:n])
    return np.clip(np.rint(x), -2 ** 22, 2 ** 22).astype(np.int64)


def peaks(r):
    """candidate peaks of the reference's scan on exact values (no zero among them: dense_margins_ok): (value, lag)"""
    out, i = [], 1
    while i < 256:
        start = next((j for j in range(i, 256) if r[j - 1] < 0 < r[j]), 256)
        end = next((j for j in range(start + 1, 256) if r[j] > 0 > r[j + 1]), 256) if start < 256 else 257
        seg = [(r[j], j) for j in range(start, end + 1) if j <= 257 and r[j] > r[j - 1] and r[j] > r[j + 1] and r[j] > 0]
        if seg:
            out.append(max(seg, key=lambda t: (t[0], -t[1])))
        i = end + 1
    return out


def tie_block(n=4096, seed=3, period=60):
    """dense block whose two largest candidate peaks (lags period and 2 period) are made EXACTLY equal by integer tweaks"""
    x = background(n, seed, period)
    p1, p2 = period, 2 * period
    # the difference r[p1] - r[p2] is linear in every single sample: d diff / d x[i] = g[i].  Sample i0 is given g = 1 (by
    # moving one of its four neighbours) and kept for the last step; greedy steps on the other samples bring the difference
    # below every |g|, then x[i0] takes the rest exactly.
    i0 = n // 2
    keep = [i0, i0 + p1, i0 - p1, i0 + p2, i0 - p2]
    x[i0 + p1] -= (x[i0 + p1] + x[i0 - p1]) - (x[i0 + p2] + x[i0 - p2]) - 1
    for _ in range(20000):
        r = acf_int(x, (p1, p2))
        diff = r[p1] - r[p2]
        xp = np.concatenate([np.zeros(p2, np.int64), x, np.zeros(p2, np.int64)])
        c = np.arange(n) + p2
        g = (xp[c + p1] + xp[c - p1]) - (xp[c + p2] + xp[c - p2])       # d(diff) / d x[i]
        assert g[i0] == 1
        g[keep] = 0
        cand = np.nonzero((np.abs(g) <= abs(diff)) & (g != 0))[0]
        if len(cand) == 0:
            x[i0] -= diff
            break
        i = cand[np.argmax(np.abs(g[cand]))]
        x[i] += -int(np.sign(diff) * np.sign(g[i])) * max(1, min(4096, abs(diff) // abs(int(g[i]))))
    r = acf_int(x, range(NL))
    assert r[p1] == r[p2]
    pk = sorted(peaks(r), reverse=True)
    assert {pk[0][1], pk[1][1]} == {p1, p2} and pk[0][0] == pk[1][0] and pk[2][0] < pk[0][0] - 2e3 * EPS_REL * r[0]
    assert dense_margins_ok(x)
    return x.astype(np.int32)


def taps_exact(r, p, D):
    """the Wiener taps around lag p from exact integers, as fractions (the reference's system: R[i][j] = r[|i-j|], b = r[p-D/2+i])"""
    A = [[Fraction(r[abs(i - j)]) for j in range(D)] + [Fraction(r[p - D // 2 + i])] for i in range(D)]
    for c in range(D):
        piv = A[c][c]
        for rr in range(D):
            if rr != c:
                f = A[rr][c] / piv
                A[rr] = [a - f * b for a, b in zip(A[rr], A[c])]
    return [A[i][D] / A[i][i] for i in range(D)]


def boundary_block(D, n=4096, seed=7, period=83, tap=0, tol=1e-12):
    """dense block whose tap `tap` times 2^15 lies within tol code steps of a rounding boundary (half-integer), found by
    integer tweaks of single samples: least-squares steps, then pairs of small moves chosen from the sorted list of their
    first-order effects; every step re-evaluated exactly"""
    x = background(n, seed, period)
    r = acf_int(x, range(NL))
    p = max(peaks(r))[1]
    lags = sorted(set(range(D)) | {p - D // 2 + i for i in range(D)})

    def value(xx):
        rr = acf_int(xx, lags)
        t = taps_exact(rr, p, D)
        assert sum(abs(v) for v in t) < Fraction(9, 10)
        return t[tap] * 32768

    def gradient(xx):
        rr = acf_int(xx, lags)
        rf = {k: float(v) for k, v in rr.items()}
        def vf(q):
            R = np.array([[q[abs(i - j)] for j in range(D)] for i in range(D)])
            return np.linalg.solve(R, np.array([q[p - D // 2 + i] for i in range(D)]))[tap] * 32768.0
        v0 = vf(rf)
        xp = np.concatenate([np.zeros(NL, np.int64), xx, np.zeros(NL, np.int64)]).astype(np.float64)
        c = np.arange(n) + NL
        g = np.zeros(n)
        d0 = 0.0
        for k in lags:
            q = dict(rf); h = 1e-7 * rf[0]; q[k] += h
            dv = (vf(q) - v0) / h
            g += dv * ((xp[c + k] + xp[c - k]) if k else 2.0 * xp[c])
            if k == 0:
                d0 = dv
        return g, d0                                        # (r[0] also moves by the square of a step: d0 per unit)

    v = value(x)
    target = Fraction(int(v * 2) // 2 * 2 + 1, 2) if v > 0 else -Fraction(int(-v * 2) // 2 * 2 + 1, 2)
    for it in range(40):
        err = float(value(x) - target)
        if abs(err) < tol:
            break
        g, d0 = gradient(x)
        step = np.rint(-err * g / np.dot(g, g)).astype(np.int64)
        if np.any(step):
            x = x + step
            continue
        # pairs of moves (i, a), (j, b), a, b in +-1..3: first-order effects a g_i + b g_j closest to -err
        mult = np.array([-3, -2, -1, 1, 2, 3])
        eff = (g[:, None] * mult[None, :] + d0 * (mult * mult)[None, :]).ravel()
        order = np.argsort(eff)
        se = eff[order]
        pos = np.clip(np.searchsorted(se, -err - eff), 1, len(se) - 1)
        best = np.minimum(np.abs(se[pos] + eff + err), np.abs(se[pos - 1] + eff + err))
        for a in np.argsort(best)[:8]:
            b = order[pos[a]] if abs(se[pos[a]] + eff[a] + err) <= abs(se[pos[a] - 1] + eff[a] + err) else order[pos[a] - 1]
            if a // 6 == b // 6:
                continue
            y = x.copy(); y[a // 6] += mult[a % 6]; y[b // 6] += mult[b % 6]
            if abs(float(value(y) - target)) < abs(err):
                x = y; break
        else:
            raise AssertionError("no improving pair")
    err = value(x) - target
    assert abs(err) < Fraction(1, 10 ** 12), float(err)
    r = acf_int(x, range(NL))
    assert max(peaks(r))[1] == p and dense_margins_ok(x)
    return x.astype(np.int32), p, float(err)


def ordinary_blocks():
    rng = np.random.default_rng(5)
    return [(rng.standard_normal(4096 - 7 * i) * 3000 + 2000 * np.sin(np.arange(4096 - 7 * i) * 2 * np.pi / (37.3 + i))).astype(np.int32)
            for i in range(5)]


def check_equal_to_exact(oracle, blocks, a, b, ntaps):
    for i, x in enumerate(blocks):
        assert a[i].pitch == b[i].pitch and list(a[i].ltm_coef) == list(b[i].ltm_coef), i
        ret, pitch, coef, _ = oracle.ltm_analyze(x, 8192, ntaps, want_autocorr=True)
        assert a[i].pitch == (pitch if (ret == 0 and pitch < 256) else 0), (i, a[i].pitch, ret, pitch)


@pytest.mark.parametrize("ntaps", [1, 3, 5])
def test_tied_peaks_fall_back(hip, oracle, ntaps):
    """a dense block (every sign and neighbour comparison of the lags 0 .. 259 clear of the bound by 1000 x, checked on the
    exact integer autocorrelation) whose two largest candidate peaks, lags 60 and 120, are exactly equal: the only refusal
    it can meet is the arg-max separation, and it must meet it -- the pick is not certified (eps < 0), the job falls back
    and comes out as the exact kernels' -- while the ordinary blocks beside it certify"""
    blocks = [tie_block()] + ordinary_blocks()
    a, b, cnt, eps, lst = launch_both(hip, blocks, ntaps)
    print("tie taps", ntaps, "counters", cnt.tolist(), "eps", eps.tolist(), "pitch", [j.pitch for j in a])
    assert eps[0] < 0 and (eps[1:] >= 0).all()
    assert cnt[1] == 1 and 0 in [int(v) & 0x7FFFFFFF for v in lst[:cnt[0]] if not int(v) & 0x80000000]
    assert cnt[0] == cnt[1] + cnt[2] + cnt[3] and cnt[3] == 0     # (list = fallbacks + audited jobs, if an earlier test left the audit on)
    check_equal_to_exact(oracle, blocks, a, b, ntaps)


@pytest.mark.parametrize("ntaps", [1, 3, 5])
def test_tap_on_rounding_boundary_falls_back(hip, oracle, ntaps):
    """a dense block, found by an integer search against the exact rational solve, whose first tap times 2^15 lies within
    1e-12 code steps of a rounding boundary of the quantiser (1, 3 and 5 taps: the multi-tap ones are not r[p] / r[0]).  Its
    pick IS certified (eps >= 0: margins 1000 x the bound, one dominant peak), so the refusal comes from the solve
    certificate's boundary margin: the job is on the fallback list and comes out as the exact kernels'"""
    x, p, err = boundary_block(ntaps)
    # (control: the block the search started from -- the same but for a few dozen units per sample -- must certify, so
    # conditioning, pivots and sum|coef| are not what refuses the crafted one)
    blocks = [x, background(4096, 7, 83).astype(np.int32)] + ordinary_blocks()
    a, b, cnt, eps, lst = launch_both(hip, blocks, ntaps)
    print("boundary taps", ntaps, "lag", p, "distance %.2e code steps" % err, "counters", cnt.tolist(), "eps", eps.tolist())
    assert (eps >= 0).all()                                      # every pick certified, the crafted one included
    assert cnt[1] == 1 and 0 in [int(v) & 0x7FFFFFFF for v in lst[:cnt[0]] if not int(v) & 0x80000000]
    assert cnt[0] == cnt[1] + cnt[2] + cnt[3] and cnt[3] == 0
    check_equal_to_exact(oracle, blocks, a, b, ntaps)
    assert a[0].pitch == p


def test_zero_autocorrelation_falls_back(hip, oracle):
    """r[j] exactly 0 at a lag (samples only at even positions: every odd lag): the sign test refuses"""
    rng = np.random.default_rng(5)
    x = np.zeros(4096, np.int32)
    x[::2] = rng.integers(-20000, 20000, 2048)
    blocks = [x] + ordinary_blocks()
    for ntaps in (1, 3, 5):
        a, b, cnt, eps, lst = launch_both(hip, blocks, ntaps)
        assert eps[0] < 0 and (eps[1:] >= 0).all() and cnt[1] == 1 and cnt[3] == 0
        check_equal_to_exact(oracle, blocks, a, b, ntaps)


def test_fast_autocorrelation_error(hip, oracle):
    """|r' - exact| of k_ltm_acf_fast against the integer autocorrelation, relative to r[0], at the lags the record shows (0 .. 4
    and pitch - 2 .. pitch + 2, pitches spread over 24 .. 249), over block lengths on both sides of every transform size and
    inside the range of the wrap correction (capacity - 0 .. 264): the certificate's eps must be >= 16 x the largest seen"""
    import torch
    L = hip.lib()
    L.sla_hip_ltm_cert_eps_rel.restype = C.c_double
    L.sla_hip_ltm_cert_eps_rel.argtypes = [C.c_uint32, C.c_double]
    rng = np.random.default_rng(9)
    worst = 0.0
    for fft_size in (4096, 8192, 16384):
        cap = fft_size // 2
        lens = sorted({cap, cap - 1, cap - 2, cap - 5, cap - 17, cap - 50, cap - 100, cap - 150, cap - 200, cap - 261, cap - 262,
                       cap - 263, cap - 264, cap - 300, cap // 2, cap // 2 + 1, cap // 2 - 100, 1024, 1025, 2048 - 263, 600, 300, 40})
        lens = [n for n in lens if 0 < n <= cap]
        # the record only shows the lags 0 .. 4 and pitch - 2 .. pitch + 2: every length with seven sine periods, so that the
        # pitches (and with them the lags measured, wrap term included) spread over 24 .. 249
        periods = (23.7, 61.7, 97.3, 131.1, 173.9, 211.3, 249.1)
        lens = [n for n in lens for _ in periods]
        blocks = [(rng.standard_normal(n) * 2.0 ** 20 + 2.0 ** 21 * np.sin(np.arange(n) * 2 * np.pi / periods[i % 7])).astype(np.int32)
                  for i, n in enumerate(lens)]
        n = len(blocks)
        stride = cap
        plane = np.zeros(n * stride, np.int32)
        aj, gr = (AcfJob * n)(), (Group * n)()
        for i, b in enumerate(blocks):
            plane[i * stride:i * stride + len(b)] = b
            aj[i] = AcfJob(i * stride, len(b), 0)
            gr[i] = Group(i * stride, len(b), 0, 0, 0, 0, 1, i, 0)
        L.slai_fft_plan_create.restype = C.c_void_p
        L.slai_fft_plan_create.argtypes = [C.c_uint32]
        L.slai_fft_plan_export.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.slai_fft_plan_destroy.argtypes = [C.c_void_p]
        L.sla_hip_ltm_fast_twiddles.argtypes = [C.c_uint32, C.POINTER(C.c_double)]
        tw, ftw = np.zeros(6 * fft_size), np.zeros(6 * fft_size)
        plan = L.slai_fft_plan_create(fft_size)
        L.slai_fft_plan_export(plan, tw.ctypes.data_as(C.POINTER(C.c_double)))
        L.slai_fft_plan_destroy(plan)
        assert L.sla_hip_ltm_fast_twiddles(fft_size, ftw.ctypes.data_as(C.POINTER(C.c_double))) == 0
        vp = lambda t: C.c_void_p(t.data_ptr())
        d_res = torch.from_numpy(plane).cuda()
        d_aj = torch.frombuffer(bytearray(bytes(aj)), dtype=torch.uint8).cuda()
        d_gr = torch.frombuffer(bytearray(bytes(gr)), dtype=torch.uint8).cuda()
        d_tw, d_ftw = torch.from_numpy(tw).cuda(), torch.from_numpy(ftw).cuda()
        d_rec = torch.zeros(12 * n, dtype=torch.float64, device="cuda")
        d_eps = torch.zeros(n, dtype=torch.float64, device="cuda")
        d_list = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
        d_jobs = torch.zeros(n * C.sizeof(Job), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        L.sla_hip_launch_ltm_cert_x.restype = C.c_int
        # (safety so large that nothing certifies would rewrite the records: keep the default and read the certified ones)
        rc = L.sla_hip_launch_ltm_cert_x(vp(d_res), C.c_uint64(len(plane)), vp(d_aj), vp(d_gr), C.c_uint32(n), C.c_uint32(fft_size),
                                         vp(d_tw), vp(d_ftw), None, C.c_uint32(0), vp(d_rec), vp(d_eps), C.c_uint32(5),
                                         C.c_double(16.0), vp(d_jobs), vp(d_list), vp(d_cnt), None, None)
        assert rc == 0
        torch.cuda.synchronize()
        rec = d_rec.cpu().numpy().reshape(n, 12)
        eps = d_eps.cpu().numpy()
        eps_rel = L.sla_hip_ltm_cert_eps_rel(fft_size, 16.0)
        seen = 0
        for i, b in enumerate(blocks):
            if eps[i] < 0:
                continue                                    # not certified: the record was rewritten by the exact kernel
            x = b.astype(np.int64)
            assert np.abs(x).max() < 2 ** 24               # every sum below 2^62
            chosen = int(rec[i, 1])
            lags = list(range(5)) + [chosen - 2 + k for k in range(5) if chosen >= 2]
            vals = list(rec[i, 2:7]) + (list(rec[i, 7:12]) if chosen >= 2 else [])
            r0 = int(np.dot(x, x))
            for lag, v in zip(lags, vals):
                ex = int(np.dot(x[:len(x) - lag], x[lag:])) if lag < len(x) else 0
                err = abs(v / (fft_size // 2) * 2.0 ** 62 - ex) / r0
                worst = max(worst, err)
            seen += 1
            assert abs(eps[i] - eps_rel * rec[i, 2]) <= 1e-12 * eps[i]
        print("fft", fft_size, "certified", seen, "of", n, "worst |r' - exact| / r[0] so far %.3e" % worst, "eps_rel %.3e" % eps_rel)
        assert seen >= n - 4 * len(periods)
        print('pitches measured', sorted({int(rec[i, 1]) for i in range(n) if eps[i] >= 0}))
        assert eps_rel >= 16.0 * worst
