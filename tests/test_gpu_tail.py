"""The tail kernel k_tailk<ORDER, K> (sla_amd/csrc/kernels/tail.inc: long-term filter, sign-log LMS cascade, zig-zag fold sum)
against the oracle's ltm_predict -> lms_predict (reference src/SLAPredictor.c:1031-1119, 1202-1331), through the C-ABI launchers
sla_hip_launch_tail / _tail_x / _tail_stages, bit for bit.  The kernel's arithmetic rests on operand arguments:
    the prediction-history products are v_mad_i32_i24 once the priming samples have left the history (block >= 2 ORDER) and
      while no job of the wave is longer than 2^18 samples;
    the step sign(e) * (bitlen|e| >> 1) is one clamp of e to [-m, m], |e| = max(e, -e) read as unsigned (e = INT32_MIN -> -16),
      and the count of leading zeros of |e| = 0 leans on the clamp;
    a job's sum is a DPP rotation tree over 2 .. 16 lanes, the histories move by row_shr;
    samples cross memory in 16-byte runs, with a scalar path at ragged ends and where the long-term delay cuts a run.
Whole-file encodes hand it ordinary material in equal blocks.  Here: every one of the ten (ORDER, K) instantiations (a mirror of
the launcher's selection rule says which a call takes, and the test fails if one goes untested), on operands at the ends of int32
(tests/tailmodel.py, pinned to the reference in tests/test_oracle_vs_ref.py::test_unit_prediction_on_extreme_operands), at
lengths around the kernel's own edges, with jobs of very different lengths and pitches in one wave, and with a sentinel in every
word the launch must not write."""
import ctypes as C

import numpy as np
import pytest

import slalibs as S
import tailmodel as M

pytestmark = pytest.mark.gpu

TAILK_BLK = 32                                    # samples per job and block of the kernel's loop (tail.inc)
TAILK2_WAVES = 2048                               # launchers.inc: one-tap waves beyond which two taps per lane are chosen
# every case of the launcher's switch, as (lms_order, tuning tail_taps)
FORMS = [(4, 1), (8, 1), (16, 1), (4, 2), (8, 2), (16, 2), (32, 2), (8, 4), (16, 4), (32, 4)]
SENTINEL = 0x5A5A5A5A
FOLD_SENTINEL = 0xA5A5A5A5A5A5A5A5
INVALID_ARGUMENT, EXCEED_HANDLE_CAPACITY = 2, 3   # include/SLA.h

REACHED = set()                                   # (ORDER, K) of every launch this module made


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


class Job(C.Structure):                           # sla_hip_tail_job, 48 bytes
    _fields_ = [("blk_off", C.c_uint64), ("blk_len", C.c_uint32), ("channel", C.c_uint32), ("pitch", C.c_uint32),
                ("ltm_coef", C.c_int32 * 5), ("pad_", C.c_uint32 * 2)]


class Tuning(C.Structure):
    _fields_ = [("lpc_pack", C.c_uint32), ("lpc_threads", C.c_uint32), ("lpc_blocks_chains", C.c_uint32), ("tail_waves", C.c_uint32),
                ("lpc_tile", C.c_uint32), ("tail_taps", C.c_uint32), ("plan_margin", C.c_double), ("rice_lanes", C.c_uint32),
                ("lattice_plain", C.c_uint32), ("cert_audit", C.c_uint32)]


def kernel_of(order, num_jobs, taps):
    """mirror of launch_tail_impl's selection: the (ORDER, K) instantiation a call takes"""
    k = taps
    k1_waves = (num_jobs * order + 63) // 64
    if k not in (1, 2, 4):
        k = 2 if (order > 16 or k1_waves > TAILK2_WAVES) else 1
    if k == 1 and order > 16:
        k = 2
    k = min(k, order // 2)
    return order, k


def spl_of(order, k):
    return TAILK_BLK * k // order                 # consecutive samples a lane moves per block


class Table:
    """jobs laid out in channel planes: every block starts at an offset that is not a multiple of 4 words (the kernel's
    16-byte runs are only 4-byte aligned), with at least one word between neighbours that no job owns"""

    def __init__(self, channels=1):
        self.cursor = [c + 1 for c in range(channels)]
        self.jobs = []                            # (x, channel, off, pitch, coef)

    def add(self, x, channel=0, pitch=0, coef=()):
        off = self.cursor[channel] + 1
        while off % 4 != (1, 2, 3)[len(self.jobs) % 3]:
            off += 1
        self.cursor[channel] = off + len(x)
        self.jobs.append((np.ascontiguousarray(x, np.int32), channel, off, pitch, [int(c) for c in coef]))
        return self


def launch(hip, table, ntaps, order, taps=0, waves=0, entry="tail", skip_lms=0, num_jobs=None):
    """one launch over the table's planes: (output planes, fold sums with four guard entries, input planes afterwards, (ORDER, K))"""
    import torch
    L = hip.lib()
    stride = max(table.cursor) + 37               # odd tail of unowned words behind the last job of every plane
    rng = np.random.default_rng(stride)
    plane = rng.integers(-2 ** 31, 2 ** 31, (len(table.cursor), stride), dtype=np.int64).astype(np.int32)   # noise in unowned words
    jobs = (Job * len(table.jobs))()
    for i, (x, ch, off, pitch, coef) in enumerate(table.jobs):
        assert off + len(x) <= stride
        plane[ch, off:off + len(x)] = x
        jobs[i] = Job(off, len(x), ch, pitch, (C.c_int32 * 5)(*(coef + [0x7FFF0000] * 5)[:5]))    # taps beyond longterm_order: not read
    nj = len(table.jobs) if num_jobs is None else num_jobs
    d_in = torch.from_numpy(plane.copy()).cuda()
    d_out = torch.full(plane.shape, SENTINEL, dtype=torch.int32, device="cuda")
    d_jobs = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).cuda()
    d_fold = torch.from_numpy(np.full(len(table.jobs) + 4, FOLD_SENTINEL, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    t = Tuning()
    t.tail_taps, t.tail_waves = taps, waves
    L.sla_hip_use_tuning(C.byref(t))
    try:
        args = [C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_uint64(stride), C.c_void_p(d_jobs.data_ptr()),
                C.c_uint32(nj), C.c_uint32(ntaps), C.c_uint32(order)]
        if entry == "tail":
            rc = L.sla_hip_launch_tail(*args, C.c_void_p(d_fold.data_ptr()), None)
        elif entry == "tail_x":
            rc = L.sla_hip_launch_tail_x(*args, C.c_void_p(d_fold.data_ptr()), None, None)
        else:
            rc = L.sla_hip_launch_tail_stages(*args, C.c_uint32(skip_lms), C.c_void_p(d_fold.data_ptr()), None)
    finally:
        L.sla_hip_use_tuning(None)
    assert rc == 0
    torch.cuda.synchronize()
    form = kernel_of(order, nj, taps)
    REACHED.add(form)
    return d_out.cpu().numpy(), d_fold.cpu().numpy().view(np.uint64), d_in.cpu().numpy(), plane, form


_expected = {}


def expected(oracle, x, pitch, coef, ntaps, order, skip_lms, key=None):
    """oracle.ltm_predict -> oracle.lms_predict -> fold_sum, each stage skipped where the call skips it"""
    if key is not None and key in _expected:
        return _expected[key]
    y = oracle.ltm_predict(x, pitch, np.array(coef[:ntaps], np.int64).astype(np.int32)) if pitch >= 3 and len(x) else x
    e = y if skip_lms or len(x) == 0 else oracle.lms_predict(y, order)
    out = (e, M.fold_sum(e))
    if key is not None:
        _expected[key] = out
    return out


def check(hip, oracle, table, ntaps, order, taps, waves, entry="tail", skip_lms=0, num_jobs=None, keys=None, what=()):
    out, fold, after, plane, form = launch(hip, table, ntaps, order, taps, waves, entry, skip_lms, num_jobs)
    nj = len(table.jobs) if num_jobs is None else num_jobs
    want = np.full(plane.shape, SENTINEL, np.uint32).view(np.int32)
    for i, (x, ch, off, pitch, coef) in enumerate(table.jobs[:nj]):
        e, fs = expected(oracle, x, pitch, coef, ntaps, order, skip_lms, None if keys is None else keys[i] + (order, skip_lms))
        want[ch, off:off + len(x)] = e
        got = out[ch, off:off + len(x)]
        ctx = what + (form, "waves", waves, entry, "job", i, "len", len(x), "pitch", pitch, "ntaps", ntaps, None if keys is None else keys[i])
        assert np.array_equal(got, e), ctx + ("first difference at", int(np.argmax(got != e)))
        assert int(fold[i]) == fs, ctx + ("fold sum", int(fold[i]), fs)
    assert np.array_equal(out, want), what + (form, "a word outside every job's block was written")
    assert all(int(v) == FOLD_SENTINEL for v in fold[nj:]), what + (form, "a fold sum beyond num_jobs was written")
    assert np.array_equal(after, plane), what + (form, "the input plane changed")
    return form


def dedup(seq):
    return sorted(set(seq), key=seq.index)


def edge_lengths(order, k):
    return dedup([order - 1, order, order + 1,                          # pass-through, priming only, one filtered sample
            31, 32, 33,                                          # one block of 32
            2 * order + 31, 2 * order + 32, 2 * order + 33,      # the first block with 24-bit prediction-history products
            4096 + spl_of(order, k) - 1,                         # a ragged last run
            16384])


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("order,taps", FORMS, ids=["order%d-k%d" % f for f in FORMS])
def test_extreme_operands_at_the_kernels_edges(hip, oracle, order, taps, waves):
    """every family at every edge length: one launch per length (the wave's longest job IS that length), the eight families
    as its jobs, in three channel planes"""
    assert kernel_of(order, len(M.FAMILIES), taps) == (order, taps)
    for n in edge_lengths(order, taps):
        table, keys = Table(3), []
        for i, name in enumerate(M.FAMILIES):
            table.add(M.family(name, n), channel=i % 3)
            keys.append((name, n))
        assert check(hip, oracle, table, 1, order, taps, waves, keys=keys, what=(n,)) == (order, taps)


MIXED_LENGTHS = (1, 7, 33, 4096, 16384)


def mixed_table():
    """67 jobs (no multiple of the 4 .. 32 jobs of a wave): neighbouring jobs -- the lanes of one DPP row -- differ in length
    by up to 2^14 and in family; one job has no samples at all (sla_hip_tail_job allows blk_len = 0: nothing is read or
    written for it but fold_sum[j] = 0, which is also how the kernel treats the lanes of a wave beyond num_jobs)"""
    table, keys = Table(3), []
    for i in range(67):
        n = 0 if i == 20 else MIXED_LENGTHS[i % 5]
        name = M.FAMILIES[(i * 3 + i // 5) % len(M.FAMILIES)]
        table.add(M.family(name, n), channel=i % 3)
        keys.append((name, n))
    return table, keys


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("order,taps", FORMS, ids=["order%d-k%d" % f for f in FORMS])
def test_mixed_waves(hip, oracle, order, taps, waves):
    table, keys = mixed_table()
    assert kernel_of(order, 67, taps) == (order, taps)
    check(hip, oracle, table, 1, order, taps, waves, keys=keys)
    check(hip, oracle, table, 1, order, taps, waves, entry="tail_x", keys=keys)
    # num_jobs = 1: the first job only, every other word and fold sum keeps its sentinel; and a lone long job
    check(hip, oracle, table, 1, order, taps, waves, num_jobs=1, keys=keys)
    lone = Table(1).add(M.family("full", 4096))
    check(hip, oracle, lone, 1, order, taps, waves, keys=[("full", 4096)])


def test_default_selection_by_the_number_of_jobs(hip, oracle):
    """without tuning the launcher goes by the number of jobs: one tap per lane, two from 2048 one-tap waves on (and always
    for order 32) -- here with 16400 short jobs in 65 .. 513 workgroups"""
    assert kernel_of(8, 100, 0) == (8, 1) and kernel_of(32, 100, 0) == (32, 2) and kernel_of(8, 16400, 0) == (8, 2)
    assert kernel_of(4, 16400, 0) == (4, 1) and kernel_of(16, 16400, 0) == (16, 2)
    lengths = (40, 1, 33, 64, 7, 97)
    table, keys = Table(3), []
    for i in range(16400):
        name, n = M.FAMILIES[i % len(M.FAMILIES)], lengths[i % len(lengths)]
        table.add(M.family(name, n, seed=i % 41), channel=i % 3)
        keys.append((name, n, i % 41))
    for order in (4, 8, 16, 32):
        check(hip, oracle, table, 1, order, 0, 0, keys=keys)
        check(hip, oracle, table, 1, order, 0, 0, num_jobs=100, keys=keys)


# ---- long-term stage ----------------------------------------------------------------------------------------------

TAPSETS = {1: ("min1", "plain1"), 3: ("ends3", "ends3b", "plain3"), 5: ("ends5", "plain5")}
LTM_FAMILIES = ("full", "24bit", "allmin", "minmax", "alt", "ramp")


def ltm_table(ntaps, order, k):
    """pitch 0 beside pitches 3, 4, 17, 255 in one wave, per tap set; delays pitch + ntaps / 2 that are no multiple of the
    lane's run (a run straddles s >= delay: the scalar path beside the vector path), a delay beyond the block (nothing is
    filtered), equal to the block, and equal to blk_len - 1 (one filtered sample)"""
    half, spl = ntaps // 2, spl_of(order, k)
    table, keys = Table(3), []

    def add(name, n, pitch, tapset):
        table.add(M.family(name, n), channel=len(table.jobs) % 3, pitch=pitch, coef=M.LTM_TAPS[tapset])
        keys.append((name, n, pitch, tapset))

    i = 0
    for tapset in TAPSETS[ntaps]:
        for pitch in (0, 3, 4, 17, 255):
            add(LTM_FAMILIES[i % len(LTM_FAMILIES)], 1500 + i, pitch, tapset)
            i += 1
    ends = TAPSETS[ntaps][0]
    assert any((p + half) % spl for p in (3, 4, 17, 255))
    add("full", 200, 255, ends)                                   # delay > blk_len
    add("full", 255 + half, 255, ends)                            # delay == blk_len
    add("full", 255 + half + 1, 255, ends)                        # delay == blk_len - 1
    add("minmax", 17 + half + 1, 17, ends)
    add("allmin", 3 + half + 1, 3, ends)
    add("full", 3 + half, 3, ends)
    add("24bit", 4096 + spl - 1, 100, TAPSETS[ntaps][-1])         # ragged last run behind the long-term stage
    add("full", 4096 + spl + 1, 2 * spl + 1 - half if 2 * spl + 1 - half >= 3 else 3 * spl + 1 - half, ends)   # delay = a multiple of the run + 1
    add("full", 2048, 4 * spl - half if 4 * spl - half >= 3 else 8 * spl - half, ends)      # delay = a multiple of the run: no straddle
    return table, keys


@pytest.mark.parametrize("ntaps", [1, 3, 5])
@pytest.mark.parametrize("order,taps", FORMS, ids=["order%d-k%d" % f for f in FORMS])
def test_long_term_stage(hip, oracle, order, taps, ntaps):
    table, keys = ltm_table(ntaps, order, taps)
    for waves in (1, 4):
        check(hip, oracle, table, ntaps, order, taps, waves, keys=keys)                                    # long-term + LMS
        check(hip, oracle, table, ntaps, order, taps, waves, entry="stages", skip_lms=1, keys=keys)        # the per-call long-term API's path
    check(hip, oracle, table, ntaps, order, taps, 4, entry="stages", skip_lms=0, keys=keys)
    # skip_lms with pitch 0 everywhere: a copy, fold sums of the input
    plain = Table(2)
    for i, name in enumerate(M.FAMILIES):
        plain.add(M.family(name, 100 + i), channel=i % 2)
    check(hip, oracle, plain, ntaps, order, taps, 4, entry="stages", skip_lms=1)


# ---- beyond 2^18 samples ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,taps", [(8, 1), (16, 2), (32, 4)], ids=["order8-k1", "order16-k2", "order32-k4"])
def test_blocks_beyond_2_18_samples(hip, oracle, order, taps):
    """a job of 2^18 + 33 samples switches the 24-bit prediction-history products off for its whole wave; the 4096-sample
    jobs beside it and the same jobs launched on their own (24-bit products on) must both equal the oracle -- on the two
    families with the largest coefficients (tests/test_tail_model.py: |FIR coefficient| >= 2^16 within 8192 samples)"""
    big = 2 ** 18 + 33
    for name in ("allmin", "ramp"):
        shared = Table(2)
        shared.add(M.family(name, big), channel=0).add(M.family("allmin", 4096), channel=1).add(M.family("ramp", 4096), channel=1)
        keys = [(name, big), ("allmin", 4096), ("ramp", 4096)]
        assert (order // taps) * 3 <= 64                                  # the three jobs share one wave
        check(hip, oracle, shared, 1, order, taps, 4, keys=keys, what=("shared wave",))
        alone = Table(1).add(M.family(name, 4096))
        check(hip, oracle, alone, 1, order, taps, 4, keys=[(name, 4096)], what=("alone",))


# ---- fold sums and refusals ---------------------------------------------------------------------------------------

def test_fold_sum_of_int32_min(hip, oracle):
    """outputs of INT32_MIN fold to 0xFFFFFFFF each, and the sum is kept in 64 bits: allmin through every path that
    produces them (pass-through of a short block, skip_lms copy, LMS errors)"""
    for order, taps in ((4, 2), (16, 1), (32, 4)):
        table = Table(1).add(M.family("allmin", order - 1)).add(M.family("allmin", 5000)).add(M.family("allmax", 5000))
        form = check(hip, oracle, table, 1, order, taps, 4)
        assert form == (order, taps)
        out, fold, _, _, _ = launch(hip, table, 1, order, taps, 4, entry="stages", skip_lms=1)
        assert int(fold[0]) == (order - 1) * 0xFFFFFFFF and int(fold[1]) == 5000 * 0xFFFFFFFF and int(fold[2]) == 5000 * 0xFFFFFFFE
        e = oracle.lms_predict(M.family("allmin", 5000), order)
        assert int(np.sum(e == M.INT32_MIN)) > 4000 and M.fold_sum(e) > 2 ** 32


def test_argument_refusals(hip, oracle):
    """launch_tail_impl's checks: NULL pointers and an even or > 5 long-term order -> INVALID_ARGUMENT, an LMS order off the
    list -> EXCEED_HANDLE_CAPACITY, no jobs -> 0; nothing is launched in any of them"""
    import torch
    L = hip.lib()
    n = 256
    d_in = torch.from_numpy(M.family("full", n + 8)).cuda()
    d_out = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    d_jobs = torch.frombuffer(bytearray(bytes(Job(3, n, 0, 0, (C.c_int32 * 5)()))), dtype=torch.uint8).cuda()
    d_fold = torch.from_numpy(np.full(2, FOLD_SENTINEL, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    pin, pout, pjobs, pfold = (C.c_void_p(t.data_ptr()) for t in (d_in, d_out, d_jobs, d_fold))

    def call(a_in=pin, a_out=pout, a_jobs=pjobs, nj=1, ntaps=1, order=8, a_fold=pfold):
        common = (a_in, a_out, C.c_uint64(n + 8), a_jobs, C.c_uint32(nj), C.c_uint32(ntaps), C.c_uint32(order))
        rcs = {L.sla_hip_launch_tail(*common, a_fold, None), L.sla_hip_launch_tail_x(*common, a_fold, None, None),
               L.sla_hip_launch_tail_stages(*common, C.c_uint32(0), a_fold, None),
               L.sla_hip_launch_tail_stages(*common, C.c_uint32(1), a_fold, None)}
        assert len(rcs) == 1, rcs
        return rcs.pop()

    assert call(a_in=None) == INVALID_ARGUMENT
    assert call(a_out=None) == INVALID_ARGUMENT
    assert call(a_jobs=None) == INVALID_ARGUMENT
    assert call(a_fold=None) == INVALID_ARGUMENT
    for ntaps in (0, 2, 4, 6, 7, 9):
        assert call(ntaps=ntaps) == INVALID_ARGUMENT, ntaps
    for order in (0, 1, 2, 3, 5, 12, 24, 33, 40, 64):
        assert call(order=order) == EXCEED_HANDLE_CAPACITY, order
    assert call(nj=0) == 0
    assert call(nj=0, ntaps=2) == INVALID_ARGUMENT and call(nj=0, order=64) == EXCEED_HANDLE_CAPACITY     # checked before the job count
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy().view(np.uint32) == SENTINEL)
    assert np.all(d_fold.cpu().numpy().view(np.uint64) == FOLD_SENTINEL)
    assert L.sla_hip_launch_tail(pin, pout, C.c_uint64(n + 8), pjobs, C.c_uint32(1), C.c_uint32(1), C.c_uint32(8), pfold, None) == 0
    torch.cuda.synchronize()                                              # the same arguments, valid, do run
    assert np.array_equal(d_out.cpu().numpy()[3:3 + n], oracle.lms_predict(M.family("full", n + 8)[3:3 + n], 8))


def test_every_instantiation_is_exercised(hip):
    """the parametrised cases above reach all ten cases of the launcher's switch (mirror of its rule) and no call falls
    outside them, so none is green by not running"""
    ten = {(4, 1), (8, 1), (16, 1), (4, 2), (8, 2), (16, 2), (32, 2), (8, 4), (16, 4), (32, 4)}
    planned = {kernel_of(order, len(M.FAMILIES), taps) for order, taps in FORMS}
    planned |= {kernel_of(order, 67, taps) for order, taps in FORMS}
    print("k_tailk instantiations planned:", sorted(planned))
    print("k_tailk instantiations launched by this module so far:", sorted(REACHED))
    assert planned == ten
    assert REACHED <= ten
    # clamps of the rule: taps the order cannot take fall onto a listed kernel
    assert kernel_of(4, 10, 4) == (4, 2) and kernel_of(32, 10, 1) == (32, 2) and kernel_of(8, 10, 3) == (8, 1)
