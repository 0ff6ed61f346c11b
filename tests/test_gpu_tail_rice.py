"""The Rice initial parameter k_tailk stores beside a job's folded sum (sla_hip_launch_extra.d_rice_init), and the encoder's
route that uses it (device long-term solve, one tail for the file: the job table comes home under the tail, only four bytes
per job behind it).  The parameter is the coder's (reference src/SLACoder.c:371-384): the mean of the folded residual, at
least 1, as the value that survives the coder's 32-bit 24.8 fixed-point word -- `init << 8` wraps at 2^24, a word that comes
back as 0 is sent as 1 -- and 1 for a job without samples.
Launcher: every (ORDER, K) instantiation on the block lengths 0, 1, ORDER - 1, ORDER, 33, 256, 4096 as the ragged jobs of one
launch, the default selection on both sides of the one-tap / two-tap switch, the corners of the formula on pass-through jobs
whose folded sum the test chooses, and a zeroed sla_hip_launch_extra that must leave the array alone.
Encoder: small files against the oracle's bytes, rice_init, pitch and taps over the routes that share the code."""
import ctypes as C

import numpy as np
import pytest

import slalibs as S
import tailmodel as M
import waveforms as W

pytestmark = pytest.mark.gpu

TAILK2_WAVES = 2048                               # launchers.inc: one-tap waves beyond which two taps per lane are chosen
FORMS = [(4, 1), (8, 1), (16, 1), (4, 2), (8, 2), (16, 2), (32, 2), (8, 4), (16, 4), (32, 4)]
SENTINEL = 0x5A5A5A5A
RICE_CANARY = 0xC3C3C3C3
FOLD_SENTINEL = 0xA5A5A5A5A5A5A5A5
REACHED = set()


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
    if k not in (1, 2, 4):
        k = 2 if (order > 16 or (num_jobs * order + 63) // 64 > TAILK2_WAVES) else 1
    if k == 1 and order > 16:
        k = 2
    return order, min(k, order // 2)


def rice_of(fold, n):
    """the formula in uint32 / uint64 arithmetic, every wrap written out"""
    if n == 0:
        return 1
    mean = (fold & 0xFFFFFFFFFFFFFFFF) // n
    init = (mean if mean > 1 else 1) & 0xFFFFFFFF
    kept = ((((init << 8) & 0xFFFFFFFF) + 128) >> 8) & 0xFFFFFFFF
    return kept if kept else 1


def test_the_formula_itself():
    """rice_of against values worked out by hand, so that the expected side of the GPU tests is pinned"""
    assert rice_of(0, 0) == 1 and rice_of(12345, 0) == 1
    assert rice_of(0, 7) == 1 and rice_of(6, 7) == 1 and rice_of(7, 7) == 1 and rice_of(13, 7) == 1 and rice_of(14, 7) == 2
    assert rice_of(7 * (2 ** 24 - 1), 7) == 2 ** 24 - 1            # 0xFFFFFF00 + 128 >> 8
    assert rice_of(7 * 2 ** 24, 7) == 1                            # init << 8 wraps to 0, 128 >> 8 = 0 -> 1
    assert rice_of(7 * 2 ** 24 - 1, 7) == 2 ** 24 - 1
    assert rice_of(7 * (2 ** 24 + 5), 7) == 5                      # the high bits are lost, not saturated
    assert rice_of(7 * 2 ** 31, 7) == 1                            # 7 samples of +-2^30
    assert rice_of(7 * 0xFFFFFFFF, 7) == 0xFFFFFF                  # 7 samples of INT32_MIN


def launch(hip, blocks, order, taps=0, extra="rice", num_jobs=None):
    """one sla_hip_launch_tail_x over the blocks (one channel plane, unowned noise words between them):
    (output plane, fold sums + 4 guards, Rice words + 4 guards, block offsets, (ORDER, K))"""
    import torch
    L = hip.lib()
    offs, at = [], 3
    for x in blocks:
        offs.append(at)
        at += len(x) + 1 + (len(offs) % 3)
    stride = at + 37
    rng = np.random.default_rng(stride)
    plane = rng.integers(-2 ** 31, 2 ** 31, stride, dtype=np.int64).astype(np.int32)
    jobs = (Job * len(blocks))()
    for i, x in enumerate(blocks):
        plane[offs[i]:offs[i] + len(x)] = x
        jobs[i] = Job(offs[i], len(x), 0, 0, (C.c_int32 * 5)())
    nj = len(blocks) if num_jobs is None else num_jobs
    d_in = torch.from_numpy(plane.copy()).cuda()
    d_out = torch.full((stride,), SENTINEL, dtype=torch.int32, device="cuda")
    d_jobs = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).cuda()
    d_fold = torch.from_numpy(np.full(len(blocks) + 4, FOLD_SENTINEL, np.uint64).view(np.int64)).cuda()
    d_rice = torch.from_numpy(np.full(len(blocks) + 4, RICE_CANARY, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    x = hip.LaunchExtra()
    assert C.sizeof(x) == 64                      # two pointers, three pointers, three words + padding, one pointer
    if extra == "rice":
        x.d_rice_init = d_rice.data_ptr()
    t = Tuning()
    t.tail_taps = taps
    L.sla_hip_use_tuning(C.byref(t))
    try:
        rc = L.sla_hip_launch_tail_x(C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_uint64(stride),
                                     C.c_void_p(d_jobs.data_ptr()), C.c_uint32(nj), C.c_uint32(1), C.c_uint32(order),
                                     C.c_void_p(d_fold.data_ptr()), None, None if extra is None else C.byref(x))
    finally:
        L.sla_hip_use_tuning(None)
    assert rc == 0
    torch.cuda.synchronize()
    form = kernel_of(order, nj, taps)
    REACHED.add(form)
    return (d_out.cpu().numpy(), d_fold.cpu().numpy().view(np.uint64), d_rice.cpu().numpy().view(np.uint32), offs, form)


_expected = {}


def expected(oracle, x, order, key):
    """(LMS errors from the oracle, folded sum from tests/tailmodel.py), computed once per key"""
    k = key + (order,)
    if k not in _expected:
        e = x if len(x) == 0 else oracle.lms_predict(x, order)
        _expected[k] = (e, M.fold_sum(e))
    return _expected[k]


def check(hip, oracle, blocks, keys, order, taps, num_jobs=None):
    out, fold, rice, offs, form = launch(hip, blocks, order, taps, num_jobs=num_jobs)
    nj = len(blocks) if num_jobs is None else num_jobs
    for i, x in enumerate(blocks[:nj]):
        e, fs = expected(oracle, x, order, keys[i])
        ctx = (form, "job", i, keys[i])
        assert np.array_equal(out[offs[i]:offs[i] + len(x)], e), ctx
        assert int(fold[i]) == fs, ctx + ("fold", int(fold[i]), fs)
        assert int(rice[i]) == rice_of(fs, len(x)), ctx + ("rice", int(rice[i]), rice_of(fs, len(x)), "fold", fs)
    assert all(int(v) == FOLD_SENTINEL for v in fold[nj:]) and all(int(v) == RICE_CANARY for v in rice[nj:]), form
    return form


@pytest.mark.parametrize("order,taps", FORMS, ids=["order%d-k%d" % f for f in FORMS])
def test_every_instantiation_on_ragged_lengths(hip, oracle, order, taps):
    """block lengths 0, 1, ORDER - 1 (pass-through), ORDER (priming only), 33, 256, 4096 as neighbouring jobs of one launch --
    the lanes of one DPP row and wave differ in length by up to 4096 -- over the operand families of tests/tailmodel.py
    (sums from 0 to n * 0xFFFFFFFF); then the first job alone, which must leave every other word untouched"""
    lengths = (0, 1, order - 1, order, 33, 256, 4096)
    blocks, keys = [], []
    for i in range(23):                           # no multiple of the 4 .. 32 jobs of a wave
        n, name = lengths[i % len(lengths)], M.FAMILIES[(i * 3 + i // 7) % len(M.FAMILIES)]
        blocks.append(M.family(name, n))
        keys.append((name, n, 0))
    assert check(hip, oracle, blocks, keys, order, taps) == (order, taps)
    assert check(hip, oracle, blocks[3:], keys[3:], order, taps, num_jobs=1) == (order, taps)


def test_default_selection_on_both_sides_of_the_switch(hip, oracle):
    """without tuning the launcher goes by the number of jobs: 20000 jobs of 64 samples are 1250 one-tap waves at order 4
    (one tap per lane) and 2500 and more from order 8 on (two); 100 of them stay on one tap up to order 16"""
    assert kernel_of(4, 20000, 0) == (4, 1) and kernel_of(8, 20000, 0) == (8, 2) and kernel_of(16, 20000, 0) == (16, 2)
    assert kernel_of(32, 20000, 0) == (32, 2) and kernel_of(8, 100, 0) == (8, 1) and kernel_of(16, 100, 0) == (16, 1)
    blocks, keys = [], []
    for i in range(20000):
        name, seed = M.FAMILIES[i % len(M.FAMILIES)], i % 5
        blocks.append(M.family(name, 64, seed=seed))
        keys.append((name, 64, seed))
    for order in (4, 8, 16, 32):
        check(hip, oracle, blocks, keys, order, 0)
        check(hip, oracle, blocks, keys, order, 0, num_jobs=100)


def folded(total, n):
    """n int32 samples whose zig-zag folds (v >= 0 -> 2 v, v < 0 -> -2 v - 1) add up to `total`"""
    base, rest = divmod(total, n)
    vals = [base + (1 if i < rest else 0) for i in range(n)]
    assert all(0 <= f <= 0xFFFFFFFF for f in vals)
    x = np.array([f // 2 if f % 2 == 0 else -(f + 1) // 2 for f in vals], np.int64)
    assert M.fold_sum(x.astype(np.int32)) == total
    return x.astype(np.int32)


@pytest.mark.parametrize("order,taps", FORMS, ids=["order%d-k%d" % f for f in FORMS])
def test_corners_of_the_formula(hip, oracle, order, taps):
    """pass-through jobs (blk_len < ORDER: the output is the input) make the folded sum what the test chooses: mean 0, the
    last sum below mean 1, mean exactly 1, the last below 2, mean 2; around 2^24, where `init << 8` wraps (one below -> 2^24 - 1,
    at it -> the word comes back 0 -> 1, above it only the low 24 bits count); every multiple of 2^24 up to 2^31 (samples of
    +-2^30) -> 1; INT32_MIN throughout -> 0xFFFFFF; and a job without samples"""
    n = min(7, order - 1)
    totals = [0, n - 1, n, 2 * n - 1, 2 * n, 3 * n + 1,
              n * (2 ** 24 - 1), n * 2 ** 24 - 1, n * 2 ** 24, n * 2 ** 24 + n - 1, n * (2 ** 24 + 1), n * (2 ** 24 + 5),
              n * 2 ** 25, n * (2 ** 25 + 2 ** 23) + 1, n * 2 ** 31, n * 0xFFFFFFFF]
    blocks = [folded(t, n) for t in totals] + [np.zeros(0, np.int32), folded(2 ** 24, 1), folded(2 ** 24 - 1, 1)]
    totals += [0, 2 ** 24, 2 ** 24 - 1]
    assert np.array_equal(blocks[14], np.full(n, 2 ** 30, np.int32))      # n samples of 2^30
    out, fold, rice, offs, form = launch(hip, blocks, order, taps)
    assert form == (order, taps)
    want = [1, 1, 1, 1, 2, 3, 2 ** 24 - 1, 2 ** 24 - 1, 1, 1, 1, 5, 1, 2 ** 23, 1, 0xFFFFFF, 1, 1, 2 ** 24 - 1]
    for i, x in enumerate(blocks):
        assert np.array_equal(out[offs[i]:offs[i] + len(x)], x), (form, i)
        assert int(fold[i]) == totals[i], (form, i, int(fold[i]), totals[i])
        assert rice_of(totals[i], len(x)) == want[i], (i, totals[i])
        assert int(rice[i]) == want[i], (form, i, "total", totals[i], "got", int(rice[i]), "want", want[i])


def test_zeroed_extra_leaves_the_array_alone(hip, oracle):
    """a zeroed sla_hip_launch_extra, and none at all, are the launch as it was: fold sums written, no Rice word touched"""
    blocks = [M.family(name, n) for name, n in (("full", 100), ("small", 4096), ("allmin", 3), ("24bit", 0), ("ramp", 33))]
    for order, taps in ((8, 1), (32, 2), (16, 4)):
        ref = launch(hip, blocks, order, taps, extra="rice")
        for extra in ("zero", None):
            out, fold, rice, offs, form = launch(hip, blocks, order, taps, extra=extra)
            assert all(int(v) == RICE_CANARY for v in rice), (form, extra)
            assert np.array_equal(fold, ref[1]) and np.array_equal(out, ref[0]), (form, extra)
        assert all(int(v) != RICE_CANARY for v in ref[2][:len(blocks)])


def test_every_instantiation_was_launched(hip):
    assert {kernel_of(o, 23, k) for o, k in FORMS} == set(FORMS)
    print("k_tailk instantiations launched by this module so far:", sorted(REACHED))
    assert REACHED <= set(FORMS)


# ---- the encoder's routes ------------------------------------------------------------------------------------------

def pitched(nch, n, bits, seed):
    """a period of 131 samples plus noise: long-term pitches >= 3 and taps that are not zero"""
    rng = np.random.default_rng(seed)
    base = rng.integers(-6000, 6000, 131)
    x = np.stack([np.tile(np.roll(base, 7 * ch), n // 131 + 1)[:n] + rng.integers(-300, 300, n) for ch in range(nch)]).astype(np.int64)
    return np.ascontiguousarray((x << (32 - 16 if bits == 16 else 32 - 24 + 6)).astype(np.int32))


def small_file(kind, nch, bits, seed):
    """three blocks of at most 4096 samples, the last one ragged; "raw": the middle block is white full-scale noise"""
    n = 2 * 4096 + 1234 + seed
    pcm = pitched(nch, n, bits, seed)
    if kind == "raw":
        pcm[:, 4096:8192] = W.gen("white", nch, 4096, bits, seed=seed)
    return pcm


def hip_encode(enc, p, pcm, **options):
    enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
    enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method, p.window_type, p.max_block_samples)
    for k, v in options.items():
        enc.set_option(k, v)
    data = enc.encode_whole(pcm)
    return data, enc.trace(want_residuals=False)


_oracle_runs = {}


def oracle_run(oracle, key, p, pcm):
    if key not in _oracle_runs:
        ret, want, to = oracle.encode_trace(p, pcm)
        assert ret == 0
        _oracle_runs[key] = (want, to)
    return _oracle_runs[key]


def same_as_oracle(got, tr, want, to, ctx):
    nb = to.num_blocks
    assert got == want, ctx
    assert tr.num_blocks == nb and np.array_equal(tr.blk_type[:nb], to.blk_type[:nb]), ctx
    comp = to.blk_type[:nb] == 0
    assert np.array_equal(tr.rice_init[:nb][comp], to.rice_init[:nb][comp]), ctx
    assert np.array_equal(tr.pitch[:nb][comp], to.pitch[:nb][comp]), ctx
    assert np.array_equal(tr.ltm_coef[:nb][comp], to.ltm_coef[:nb][comp]), ctx


ROUTES = [{}, {"ltm_cert": 0}, {"single_tail": 0}, {"single_tail": 0, "ltm_cert": 0}, {"device_ltm": 0},
          {"device_ltm": 0, "single_tail": 0}]
FILES = [("plain", 1, 16, 0, 1), ("plain", 2, 24, 1, 3), ("raw", 2, 16, 1, 1), ("raw", 1, 24, 0, 5), ("plain", 2, 16, 0, 3)]


@pytest.mark.parametrize("kind,nch,bits,ms,taps", FILES, ids=["%s-%dch-%dbit-ms%d-ltm%d" % f for f in FILES])
def test_small_files_over_every_route(hip, oracle, kind, nch, bits, ms, taps):
    """three blocks, mono and mid/side, 16 and 24 bits, a ragged last block, a RAW block in the middle: bytes, rice_init,
    pitch and taps are the oracle's with the certified long-term stage on and off, one tail and one per chunk, and with the
    long-term solve on the host (which keeps the folded sums' route)"""
    pcm = small_file(kind, nch, bits, 7 * taps + nch)
    p = S.make_params(nch, bits, 48000, parcor=16, ltm=taps, lms=8, ms=ms, max_block=4096, cap=(nch, 4096, 16, taps, 8))
    want, to = oracle_run(oracle, (kind, nch, bits, ms, taps), p, pcm)
    nb = to.num_blocks
    assert nb >= 3 and (to.blk_type[:nb] == 2).any() == (kind == "raw") and (to.blk_type[:nb] == 0).any()
    assert (to.pitch[:nb] >= 3).any()
    for opts in ROUTES:
        enc = hip.Encoder(nch, 4096, 16, taps, 8)
        try:
            got, tr = hip_encode(enc, p, pcm, **opts)
        finally:
            enc.close()
        same_as_oracle(got, tr, want, to, (kind, nch, bits, ms, taps, opts))


def long_file(seed):
    """100 blocks and a ragged one, a RAW stretch and a silent one: enough super-frames for three chunks"""
    n = 100 * 4096 + 777
    pcm = pitched(2, n, 16, seed)
    pcm[:, 5 * 4096:7 * 4096] = W.gen("white", 2, 2 * 4096, 16, seed=seed)
    pcm[:, 40 * 4096:42 * 4096] = 0
    return pcm


def test_three_chunks_and_a_handle_reused(hip, oracle):
    """chunks forced to 3 (one tail behind three block stages, and a tail per chunk), and one handle through two different
    files in turn -- long, short, long again, and short first on a second handle -- so that the work arrays kept in the handle
    are seen to grow, to be reused at a smaller size and to be cleared between files"""
    p = S.make_params(2, 16, 48000, parcor=16, ltm=3, lms=8, ms=1, max_block=4096, cap=(2, 4096, 16, 3, 8))
    big, small = long_file(3), small_file("raw", 2, 16, 11)
    want_big, to_big = oracle_run(oracle, "big", p, big)
    want_small, to_small = oracle_run(oracle, "small", p, small)
    assert (to_big.blk_type[:to_big.num_blocks] == 2).any() and (to_big.blk_type[:to_big.num_blocks] == 1).any()
    for opts in ({"chunks": 3}, {"chunks": 3, "single_tail": 0}, {"chunks": 3, "ltm_cert": 0}, {}):
        enc = hip.Encoder(2, 4096, 16, 3, 8)
        try:
            for pcm, want, to, what in ((big, want_big, to_big, "big"), (small, want_small, to_small, "small"),
                                        (big, want_big, to_big, "big again")):
                got, tr = hip_encode(enc, p, pcm, **opts)
                same_as_oracle(got, tr, want, to, (opts, what))
        finally:
            enc.close()
    enc = hip.Encoder(2, 4096, 16, 3, 8)
    try:
        for pcm, want, to, what in ((small, want_small, to_small, "small first"), (big, want_big, to_big, "then big")):
            got, tr = hip_encode(enc, p, pcm)
            same_as_oracle(got, tr, want, to, what)
    finally:
        enc.close()
