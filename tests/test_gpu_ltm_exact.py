"""GPU tests of the long-term stage's exact route: k_ltm_acf<true|false>, k_ltm_acf2<L, T, REC>, k_ltm_acf2_list and the
wave-parallel pitch scan of acf_emit (and its twin in acf_emit_cert), held directly against the oracle through the
device-free model tests/ltmscanmodel.py.  Everything is bit for bit: the doubles of every lag, the 12-double record, the
jobs the solver makes of it, the jobs of the certified launcher, the public API's result, pitch and taps.
  1. all fft_size lags of every kernel form (and head 5 / 300)          2. blocks longer than half the transform
  3. records of the whole catalogue, both lag sweeps included           4. the same device records through the solver
  5. the certified launcher (transform and integer route) on the same blocks, ending with the exact answer
  6. SLALongTermCalculator_CalculateCoef on the hand-checked blocks and one short whole-file encode
The job tables lie over two channel planes with blocks at odd offsets and gaps of unrelated values between them; every
output buffer is prefilled with a NaN pattern and followed by a guard region that must come back untouched.
Which kernel runs at which size (sla_hip_launch_ltm_acf_x, SLA_HIP_LDS_BUDGET = 160 KiB - 256): 1024 and 2048
k_ltm_acf<true>; 4096 / 8192 / 16384 k_ltm_acf2<11 / 12 / 13>; 32768 and 131072 (256 KiB and 1 MiB of doubles)
k_ltm_acf<false> in scratch slots."""
import ctypes as C
import functools

import numpy as np
import pytest

import ltmscanmodel as M
import slalibs as S

pytestmark = pytest.mark.gpu

f64p, u32p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
RECORD = 12                                                     # SLA_HIP_ACF_RECORD
GUARD = 512                                                     # doubles behind every output buffer
NAN_BITS = 0x7FF8DEADBEEF1234
SLOTS = 3                                                       # scratch slots: fewer than jobs, so that they are reused
LDS_BUDGET = 160 * 1024 - 256                                   # SLA_HIP_LDS_BUDGET


class AcfJob(C.Structure):
    _fields_ = [("blk_off", C.c_uint64), ("blk_len", C.c_uint32), ("channel", C.c_uint32)]


class Group(C.Structure):
    _fields_ = [("pcm_off", C.c_uint64)] + [(nm, C.c_uint32) for nm in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


class Job(C.Structure):
    _fields_ = [("blk_off", C.c_uint64), ("blk_len", C.c_uint32), ("channel", C.c_uint32), ("pitch", C.c_uint32),
                ("ltm_coef", C.c_int32 * 5), ("pad_", C.c_uint32 * 2)]


class Tuning(C.Structure):                                      # sla_hip_tuning
    _fields_ = [("lpc_pack", C.c_uint32), ("lpc_threads", C.c_uint32), ("lpc_blocks_chains", C.c_uint32), ("tail_waves", C.c_uint32),
                ("lpc_tile", C.c_uint32), ("tail_taps", C.c_uint32), ("plan_margin", C.c_double), ("rice_lanes", C.c_uint32),
                ("lattice_plain", C.c_uint32), ("cert_audit", C.c_uint32), ("ltm_int", C.c_uint32)]


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    L = sla_amd.lib()
    L.slai_fft_plan_create.restype = C.c_void_p
    L.slai_fft_plan_create.argtypes = [C.c_uint32]
    L.slai_fft_plan_export.argtypes = [C.c_void_p, f64p]
    L.slai_fft_plan_destroy.argtypes = [C.c_void_p]
    L.slai_ltm_solve.argtypes = [f64p, C.c_uint32, u32p, f64p]
    L.slai_ltm_solve.restype = C.c_int
    L.sla_hip_launch_ltm_acf.restype = C.c_int
    L.sla_hip_launch_ltm_solve.restype = C.c_int
    return sla_amd


@functools.lru_cache(maxsize=None)
def twiddles(fft_size):
    import sla_amd
    L = sla_amd.lib()
    tw = np.zeros(6 * fft_size)
    plan = L.slai_fft_plan_create(fft_size)
    assert plan
    L.slai_fft_plan_export(plan, tw.ctypes.data_as(f64p))
    L.slai_fft_plan_destroy(plan)
    return tw


def vp(t):
    return C.c_void_p(t.data_ptr())


def nan_buffer(n):
    """n + GUARD doubles of a NaN pattern on the device"""
    import torch
    return torch.from_numpy(np.full(n + GUARD, NAN_BITS, np.uint64).view(np.float64)).cuda()


def guard_intact(t, n):
    return bool((t[n:].cpu().numpy().view(np.uint64) == NAN_BITS).all())


class Table:
    """the blocks dealt out over two channel planes: odd offsets, gaps of one to six samples, unrelated values in the gaps"""

    def __init__(self, blocks):
        import torch
        n = len(blocks)
        fill = [1, 3]
        self.jobs = (AcfJob * n)()
        self.groups = (Group * n)()
        for i, b in enumerate(blocks):
            ch = i & 1
            self.jobs[i] = AcfJob(fill[ch], len(b), ch)
            self.groups[i] = Group(fill[ch], len(b), ch, 0, 0, 0, 1, i, 0)
            fill[ch] += len(b) + 1 + 2 * (i % 3)
            fill[ch] += 1 - (fill[ch] & 1)                      # odd again
        self.n = n
        self.stride = max(fill) + 5
        plane = np.full(2 * self.stride, 0x12345678, np.int32)
        for i, b in enumerate(blocks):
            o = self.jobs[i].channel * self.stride + self.jobs[i].blk_off
            assert o + len(b) <= len(plane) and (self.jobs[i].channel == 1 or o + len(b) < self.stride)
            plane[o:o + len(b)] = b
        self.d_res = torch.from_numpy(plane).cuda()
        self.d_jobs = torch.frombuffer(bytearray(bytes(self.jobs)), dtype=torch.uint8).cuda()
        self.d_groups = torch.frombuffer(bytearray(bytes(self.groups)), dtype=torch.uint8).cuda()


def run_acf(hip, table, fft_size, head):
    """sla_hip_launch_ltm_acf over the table: ([job][head] doubles, the device buffer).  Scratch slots where the transform does
    not fit the LDS; the guards behind the output and behind the scratch are checked here."""
    import torch
    L = hip.lib()
    d_tw = torch.from_numpy(twiddles(fft_size)).cuda()
    d_out = nan_buffer(table.n * head)
    in_scratch = 8 * fft_size > LDS_BUDGET
    d_scr = nan_buffer(SLOTS * fft_size) if in_scratch else None
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_ltm_acf(vp(table.d_res), C.c_uint64(table.stride), vp(table.d_jobs), C.c_uint32(table.n), C.c_uint32(fft_size),
                                  vp(d_tw), vp(d_scr) if in_scratch else None, C.c_uint32(SLOTS if in_scratch else 0), vp(d_out),
                                  C.c_uint32(head), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guard_intact(d_out, table.n * head), "the kernel wrote behind num_jobs * head doubles"
    if in_scratch:
        assert guard_intact(d_scr, SLOTS * fft_size), "the kernel wrote behind its scratch slots"
    return d_out[:table.n * head].cpu().numpy().reshape(table.n, head), d_out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def first_difference(a, b):
    d = np.nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))[0]
    return (len(d), int(d[0]), float(a[d[0]]), float(b[d[0]])) if len(d) else None


# ---- 1. all lags, every kernel form -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fft_size", [1024, 2048, 4096, 8192, 16384, 32768, 131072])
def test_all_lags(hip, fft_size):
    """head = fft_size on the catalogue without the sweep: every double the reference's.  1024, 2048: k_ltm_acf<true>; 4096,
    8192, 16384: k_ltm_acf2<.., false>; 32768, 131072: k_ltm_acf<false>, three scratch slots for 26 jobs"""
    cases = M.prepared(fft_size, sweep=False)
    got, _ = run_acf(hip, Table([c.x for c in cases]), fft_size, fft_size)
    for i, c in enumerate(cases):
        assert same_bits(got[i], c.ac), (fft_size, c.name, first_difference(got[i], c.ac))


@pytest.mark.parametrize("head", [5, 300])
def test_short_heads(hip, head):
    """head = 5 and 300 at 8192: the first `head` lags of every job, nothing behind num_jobs * head"""
    cases = M.prepared(8192, sweep=False)
    got, _ = run_acf(hip, Table([c.x for c in cases]), 8192, head)
    for i, c in enumerate(cases):
        assert same_bits(got[i], c.ac[:head]), (head, c.name, first_difference(got[i], c.ac[:head]))


# ---- 2. blocks longer than half the transform -------------------------------------------------------------------------

@pytest.mark.parametrize("fft_size", [2048, 4096, 8192, 16384])
def test_blocks_longer_than_half_the_transform(hip, oracle, fft_size):
    """fft_size / 2 + 1, + 2, 3 fft_size / 4 + 1 and fft_size samples (the autocorrelation wraps): the generic kernel at 2048,
    the branch n > 2^L of acf2_first_pass at 4096 .. 16384; full-range noise and the two-impulse block"""
    rng = np.random.default_rng(fft_size + 1)
    blocks = []
    for n in (fft_size // 2 + 1, fft_size // 2 + 2, 3 * fft_size // 4 + 1, fft_size):
        t = np.arange(n)
        blocks.append(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32))
        blocks.append((1000000 * (t == 10) + 900000 * (t == 50)).astype(np.int32))
    got, _ = run_acf(hip, Table(blocks), fft_size, fft_size)
    for i, x in enumerate(blocks):
        want = M.reference_acf(oracle, x, fft_size)
        assert same_bits(got[i], want), (fft_size, len(x), i & 1, first_difference(got[i], want))


# ---- 3. records, 4. through the solver --------------------------------------------------------------------------------

RECORD_SIZES = [(2048, False), (4096, True), (8192, True), (16384, True), (32768, False)]


@pytest.mark.parametrize("fft_size,sweep", RECORD_SIZES)
def test_records(hip, fft_size, sweep):
    """head = SLA_HIP_ACF_RECORD: the whole catalogue with both sweeps at 4096, 8192, 16384 (k_ltm_acf2<.., true>, the pruned
    inverse), the blocks outside the sweep at 2048 (generic kernel in LDS) and 32768 (in scratch): all 12 doubles"""
    cases = M.prepared(fft_size, sweep)
    got, _ = run_acf(hip, Table([c.x for c in cases]), fft_size, RECORD)
    print("fft", fft_size, "jobs", len(cases), "flags", M.flag_counts(cases))
    bad = [(c.name, got[i].tolist(), c.record.tolist()) for i, c in enumerate(cases) if not same_bits(got[i], c.record)]
    assert not bad, (fft_size, len(bad), bad[:3])


def quantised(L, rec, ntaps):
    """(pitch, five taps) k_tail must be given for this record: the host solve (pinned to the oracle by the CPU suite), the
    reference's quantiser, pitch 0 where the analysis failed or chose lag 256 or 257"""
    pitch, coef = C.c_uint32(0), np.zeros(5)
    rec = np.ascontiguousarray(rec)
    ret = L.slai_ltm_solve(rec.ctypes.data_as(f64p), ntaps, C.byref(pitch), coef.ctypes.data_as(f64p))
    if ret != 0:
        coef[:] = 0
    wp = 0 if (ret != 0 or pitch.value >= 256) else pitch.value
    q = []
    for t in range(5):
        v = (coef[t] if t < ntaps else 0.0) * 32768.0
        rv = np.floor(v + 0.5) if v >= 0 else -np.floor(-v + 0.5)
        qi = -2 ** 31 if not (-2147483649.0 < rv < 2147483648.0) else int(rv)
        q.append(((qi << 16) & 0xFFFFFFFF) - (1 << 32) if ((qi << 16) & 0x80000000) else (qi << 16) & 0xFFFFFFFF)
    return wp, q


@pytest.mark.parametrize("fft_size,sweep", RECORD_SIZES)
def test_records_through_the_solver(hip, fft_size, sweep):
    """the device records of the exact kernels, as they lie in device memory, through sla_hip_launch_ltm_solve at 1, 3 and 5
    taps: pitch and quantised taps of the host solve on the model's record; pitch 0 wherever lag 256 or 257 was chosen"""
    import torch
    L = hip.lib()
    cases = M.prepared(fft_size, sweep)
    table = Table([c.x for c in cases])
    _, d_rec = run_acf(hip, table, fft_size, RECORD)
    n = table.n
    for ntaps in (1, 3, 5):
        d_jobs = torch.full((n * C.sizeof(Job) + 256,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.sla_hip_launch_ltm_solve(vp(d_rec), vp(table.d_groups), C.c_uint32(n), C.c_uint32(ntaps), vp(d_jobs), None) == 0
        torch.cuda.synchronize()
        raw = d_jobs.cpu().numpy()
        assert (raw[n * C.sizeof(Job):] == 0xAB).all()
        jobs = (Job * n).from_buffer_copy(raw[:n * C.sizeof(Job)].tobytes())
        late = 0
        for i, c in enumerate(cases):
            wp, q = quantised(L, c.record, ntaps)
            j = jobs[i]
            assert (j.blk_off, j.blk_len, j.channel) == (table.jobs[i].blk_off, len(c.x), i & 1)
            assert j.pitch == wp and list(j.ltm_coef) == q, (fft_size, ntaps, c.name, j.pitch, wp, list(j.ltm_coef), q)
            if c.chosen >= 256:
                assert j.pitch == 0
                late += 1
        assert late >= 3                                         # (lags 256 and 257 were reached: the table rows at least)


# ---- 5. the certified launcher on the same blocks ---------------------------------------------------------------------

@pytest.mark.parametrize("fft_size", [4096, 8192, 16384, 32768])
def test_certified_launcher_ends_with_the_exact_answer(hip, fft_size):
    """sla_hip_launch_ltm_cert_x, cert_audit = 1, transform and integer route, 1, 3 and 5 taps, the whole catalogue (about 620
    jobs: the 64-workgroup list kernels stride; at 32768 the list form of k_ltm_acf<false> on three scratch slots): the jobs
    of test_records_through_the_solver, no audited job different, the all-zero block certified.  Whether an edge block is
    certified is free."""
    import torch
    import test_gpu_ltm_cert as T
    L = hip.lib()
    cases = M.prepared(fft_size)
    blocks = [c.x for c in cases]
    zero = next(i for i, c in enumerate(cases) if c.name == "zeros")
    in_scratch = 8 * fft_size > LDS_BUDGET
    d_scr = nan_buffer(SLOTS * fft_size) if in_scratch else None
    want = {ntaps: [quantised(L, c.record, ntaps) for c in cases] for ntaps in (1, 3, 5)}
    try:
        for ltm_int in (0, 1):
            t = Tuning()
            t.cert_audit, t.ltm_int = 1, ltm_int
            L.sla_hip_use_tuning(C.byref(t))
            for ntaps in (1, 3, 5):
                a, b, cnt, eps, lst = T.launch_both(hip, blocks, ntaps, fft_size, scratch=d_scr, scratch_slots=SLOTS if in_scratch else 0)
                print("fft", fft_size, "ltm_int", ltm_int, "taps", ntaps, "counters", cnt.tolist())
                for i, c in enumerate(cases):
                    wp, q = want[ntaps][i]
                    assert (a[i].pitch, list(a[i].ltm_coef)) == (wp, q), ("certified", fft_size, ltm_int, ntaps, c.name, a[i].pitch, wp)
                    assert (b[i].pitch, list(b[i].ltm_coef)) == (wp, q), ("exact pair", fft_size, ltm_int, ntaps, c.name, b[i].pitch, wp)
                assert cnt[3] == 0 and cnt[2] == len(cases) - cnt[1], cnt.tolist()
                assert cnt[0] == cnt[1] + cnt[2]
                assert eps[zero] >= 0 and zero not in [int(v) for v in lst[:cnt[0]] if not int(v) & 0x80000000]
                if in_scratch:
                    assert guard_intact(d_scr, SLOTS * fft_size)
    finally:
        L.sla_hip_use_tuning(None)


# ---- 6. the public API ------------------------------------------------------------------------------------------------

def test_calculate_coef_on_the_table_rows(hip, oracle):
    """SLALongTermCalculator_CalculateCoef on the eight hand-checked blocks at fft_size 8192: result, pitch (256 and 257
    come back as they are) and tap doubles of the oracle"""
    L = hip.lib()
    L.SLALongTermCalculator_Create.restype = C.c_void_p
    L.SLALongTermCalculator_Destroy.restype = None
    L.SLALongTermCalculator_Destroy.argtypes = [C.c_void_p]
    h = L.SLALongTermCalculator_Create(8192, 256, 10, 5)
    assert h
    try:
        pitches = set()
        for name, x in M.table_rows(8192):
            for taps in (1, 3, 5):
                pitch, coef = C.c_uint32(), np.zeros(5)
                rc = L.SLALongTermCalculator_CalculateCoef(C.c_void_p(h), x.ctypes.data_as(i32p), len(x), C.byref(pitch),
                                                           coef.ctypes.data_as(f64p), taps)
                ret, wp, wc = oracle.ltm_analyze(x, 8192, taps)
                assert rc == ret, (name, taps, rc, ret)
                if ret == 0:
                    assert pitch.value == wp and same_bits(coef[:taps], wc), (name, taps, pitch.value, wp)
                    pitches.add(wp)
        assert {256, 257, 4, 40, 2} <= pitches
    finally:
        L.SLALongTermCalculator_Destroy(C.c_void_p(h))


def test_encode_whole_with_a_pitch_beyond_the_range(hip, oracle):
    """a stationary 16-bit mono file 2 + 46 [t % 256 == 0] (left-justified: about 1e5 + 3e6 [..]), PARCOR order 4, 3 taps: the
    oracle's bytes and trace pitch through the certified routes, the exact kernels and the host solve"""
    n = 5 * 4096 + 300
    t = np.arange(n)
    pcm = np.ascontiguousarray(((2 + 46 * (t % 256 == 0)).astype(np.int32) << 16)[None, :])
    p = S.make_params(1, 16, 48000, parcor=4, ltm=3, lms=8, ms=0, max_block=4096, cap=(1, 4096, 4, 3, 8))
    ret, want, to = oracle.encode_trace(p, pcm)
    assert ret == 0
    nb = to.num_blocks
    comp = to.blk_type[:nb] == 0
    assert comp.any()
    # (the test is about the scan's lag 256: the oracle's lattice residual must take it there, whatever becomes of the pitch)
    late = [M.scan(M.reference_acf(oracle, to.res_lattice[0, int(s):int(s) + int(m)], 8192))[0] for s, m in zip(to.blk_start[:nb], to.blk_nsmpl[:nb])]
    print("oracle pitch", to.pitch[:nb, 0].tolist(), "lag chosen by the scan", late)
    assert late.count(256) >= 4
    routes = [{"ltm_cert": c, "ltm_int": i} for c in (0, 1) for i in (0, 1)] + [{"device_ltm": 0}]
    for opts in routes:
        enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
        try:
            enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
            enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method, p.window_type, p.max_block_samples)
            for k, v in opts.items():
                enc.set_option(k, v)
            got = enc.encode_whole(pcm)
            tr = enc.trace()
        finally:
            enc.close()
        assert got == want, opts
        assert np.array_equal(tr.pitch[:nb][comp], to.pitch[:nb][comp]), opts
        assert np.array_equal(tr.ltm_coef[:nb][comp], to.ltm_coef[:nb][comp]), opts
