"""GPU tests of k_ltm_acf_int: the long-term stage's autocorrelation from exact integer sums on the int8 matrix pipe
(tuning / option "ltm_int").
  1. the raw sums of sla_hip_launch_ltm_acf_int against Python integers: bit-equal where |sum| < 2^53, else within one ulp;
     lengths around every 16-, 64- and 1024-sample boundary, every amplitude class and digit boundary, two-sample blocks
     that place one product at a chosen lag and position (fragment maps, shifts, the 18th shift)
  2. sla_hip_launch_ltm_cert_x with ltm_int 0 and 1: byte-identical job tables, no audited job different, and the new
     route certifies what the transform certifies
  3. the encoder with ltm_int 0 / 1 and with ltm_cert 0: the oracle's bytes."""
import ctypes as C

import numpy as np
import pytest

import ltmintmodel as M
import slalibs as S
import waveforms as W

pytestmark = pytest.mark.gpu

LAGS = M.LAGS


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


class AcfJob(C.Structure):
    _fields_ = [("blk_off", C.c_uint64), ("blk_len", C.c_uint32), ("channel", C.c_uint32)]


class Tuning(C.Structure):
    _fields_ = [("lpc_pack", C.c_uint32), ("lpc_threads", C.c_uint32), ("lpc_blocks_chains", C.c_uint32), ("tail_waves", C.c_uint32),
                ("lpc_tile", C.c_uint32), ("tail_taps", C.c_uint32), ("plan_margin", C.c_double), ("rice_lanes", C.c_uint32),
                ("lattice_plain", C.c_uint32), ("cert_audit", C.c_uint32), ("ltm_int", C.c_uint32)]


def raw_sums(hip, blocks, fft_size):
    """sla_hip_launch_ltm_acf_int over `blocks`, dealt out over two channel planes at odd offsets: [job][264] doubles"""
    import torch
    L = hip.lib()
    n = len(blocks)
    fill = [1, 3]                                               # next free offset of each channel: odd, not a multiple of 4
    aj = (AcfJob * n)()
    for i, b in enumerate(blocks):
        ch = i & 1
        aj[i] = AcfJob(fill[ch], len(b), ch)
        fill[ch] += len(b) + 1
        fill[ch] += 1 - (fill[ch] & 1)                          # odd again
    stride = max(fill) + 5
    plane = np.full(2 * stride, 0x12345678, np.int32)           # (whatever lies between the blocks must not matter)
    for i, b in enumerate(blocks):
        o = aj[i].channel * stride + aj[i].blk_off
        plane[o:o + len(b)] = b
    d_res = torch.from_numpy(plane).cuda()
    d_aj = torch.frombuffer(bytearray(bytes(aj)), dtype=torch.uint8).cuda()
    d_out = torch.full((n * LAGS,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = L.sla_hip_launch_ltm_acf_int(vp(d_res), C.c_uint64(stride), vp(d_aj), C.c_uint32(n), C.c_uint32(fft_size), vp(d_out), None)
    assert rc == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy().reshape(n, LAGS)


def check_exact(blocks, got, fft_size, what):
    for i, b in enumerate(blocks):
        want = M.acf_exact(b)
        for k in range(LAGS):
            w = M.scaled(want[k], fft_size)
            if abs(want[k]) < 2 ** 53:
                assert got[i, k] == w, (what, i, len(b), k, got[i, k], w)
            else:
                assert abs(got[i, k] - w) <= np.spacing(abs(w)), (what, i, len(b), k, got[i, k], w)
        if len(b) < LAGS:
            assert not got[i, len(b):].any()


def gaussian(rng, n, log2_amp):
    lim = 2.0 ** 31
    return np.clip(np.rint(rng.standard_normal(n) * 2.0 ** log2_amp), -lim, lim - 1).astype(np.int64).astype(np.int32)


LENGTHS_8K = [1, 15, 16, 17, 255, 263, 264, 265, 1023, 1024, 1025, 1287, 2048, 2049, 4095, 4096]
LENGTHS_32K = [8192, 16383, 16384]
AMPS = [6, 14, 20, 23, 30]
BOUNDARY = [127, 128, -128, -129, 32639, 32640, -32896, -32897, 8355711, 8355712, -8421504, -8421505,
            2139062143, 2139062144, -2 ** 31, 2 ** 31 - 1]


@pytest.mark.parametrize("fft_size,lengths", [(8192, LENGTHS_8K), (32768, LENGTHS_32K)])
def test_raw_sums_gaussian(hip, fft_size, lengths):
    """Gaussian blocks at 2^6 .. 2^30 (one to five digits) at every length"""
    rng = np.random.default_rng(fft_size)
    blocks = [gaussian(rng, n, a) for n in lengths for a in AMPS]
    check_exact(blocks, raw_sums(hip, blocks, fft_size), fft_size, "gaussian")


def test_raw_sums_digit_boundaries(hip):
    """one sample (three places, the first and the last of the block among them) forced to every boundary of the digit
    table and to its neighbour, INT32_MIN and INT32_MAX, in small noise"""
    rng = np.random.default_rng(2)
    blocks = []
    for v in BOUNDARY:
        for n in (1287, 4096):
            x = rng.integers(-100, 100, n).astype(np.int32)
            x[[0, n // 2 + 1, n - 1]] = v
            blocks.append(x)
    check_exact(blocks, raw_sums(hip, blocks, 8192), 8192, "digit boundary")


def test_raw_sums_extreme_blocks(hip):
    """constant INT32_MIN and alternating INT32_MAX / INT32_MIN over 16384 samples: sums up to 2^76, no overflow on the way"""
    blocks = [np.full(16384, -2 ** 31, np.int32),
              np.where(np.arange(16384) % 2 == 0, 2 ** 31 - 1, -2 ** 31).astype(np.int32),
              np.zeros(16384, np.int32)]
    got = raw_sums(hip, blocks, 32768)
    check_exact(blocks, got, 32768, "extreme")
    assert not got[2].any()


@pytest.mark.parametrize("n", [1300, 4096])
def test_lag_placement(hip, n):
    """blocks that are zero except x[p] = 3, x[p + k] = -5: only r[0] = 34 and r[k] = -15 may be non-zero"""
    cases = [(k, p) for k in (1, 15, 16, 17, 31, 32, 255, 256, 257, 263)
             for p in (0, 14, 15, 16, 63, 64, 1008, 1023, 1024, n - k - 1)]
    blocks = []
    for k, p in cases:
        x = np.zeros(n, np.int32)
        x[p], x[p + k] = 3, -5
        blocks.append(x)
    got = raw_sums(hip, blocks, 8192) / (2.0 ** -62 * 4096)
    for (k, p), r in zip(cases, got):
        want = np.zeros(LAGS)
        want[0], want[k] = 34.0, -15.0
        assert np.array_equal(r, want), (k, p, np.nonzero(r != want)[0].tolist(), r[r != want].tolist())


# ---- the certified launcher either way -----------------------------------------------------------------------------

def cert_blocks(kind, count=64, n=4096):
    rng = np.random.default_rng({"white": 1, "gauss": 2, "music": 3}[kind])
    if kind == "white":
        return [rng.integers(-2 ** 20, 2 ** 20, n - 3 * i).astype(np.int32) for i in range(count)]
    if kind == "gauss":
        return [(rng.standard_normal(n - 7 * i) * 3000 + 2000 * np.sin(np.arange(n - 7 * i) * 2 * np.pi / (37.3 + i))).astype(np.int32)
                for i in range(count)]
    pcm = W.music_like(1, count * n, 24, seed=4)[0] >> 8                                   # 24-bit samples, first difference
    d = np.diff(pcm.astype(np.int64), prepend=0).astype(np.int32)
    return [d[i * n:(i + 1) * n - 5 * (i % 3)] for i in range(count)]


@pytest.mark.parametrize("ntaps", [1, 3, 5])
def test_cert_launcher_same_jobs_either_way(hip, ntaps):
    """sla_hip_launch_ltm_cert_x under tuning ltm_int = 0 and 1, cert_audit = 1: the job tables (pitch, taps) are
    byte-identical, no audited job differs, and the integer route certifies at least 99 % wherever the transform does (a
    route that certified nothing would pass every byte comparison)"""
    import test_gpu_ltm_cert as T
    L = hip.lib()
    held = 0
    try:
        for kind in ("white", "gauss", "music"):
            blocks = cert_blocks(kind)
            res = []
            for ltm_int in (0, 1):
                t = Tuning()
                t.cert_audit, t.ltm_int = 1, ltm_int
                L.sla_hip_use_tuning(C.byref(t))
                a, b, cnt, eps, lst = T.launch_both(hip, blocks, ntaps)
                assert cnt[3] == 0 and cnt[2] == len(blocks) - cnt[1], (kind, ltm_int, cnt.tolist())
                for ja, jb in zip(a, b):                                                      # (and equal to the exact pair)
                    assert ja.pitch == jb.pitch and list(ja.ltm_coef) == list(jb.ltm_coef), (kind, ltm_int)
                res.append((bytes(a), len(blocks) - int(cnt[1])))
            print("%-6s taps %d: certified %d (transform) / %d (integer) of %d" % (kind, ntaps, res[0][1], res[1][1], len(blocks)))
            assert res[0][0] == res[1][0], kind
            if res[0][1] >= 0.99 * len(blocks):
                held += 1
                assert res[1][1] >= 0.99 * len(blocks), (kind, res[0][1], res[1][1])
        assert held >= 2                                                                      # (the condition was not vacuous)
    finally:
        L.sla_hip_use_tuning(None)


# ---- the encoder ------------------------------------------------------------------------------------------------------

def encode(hip, p, pcm, enc=None, **options):
    own = enc is None
    if own:
        enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    try:
        enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
        enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method,
                                 p.window_type, p.max_block_samples)
        for k, v in options.items():
            enc.set_option(k, v)
        return enc.encode_whole(pcm), enc.last_ltm_cert()
    finally:
        if own:
            enc.close()


ROUTES = ({"ltm_cert": 1, "ltm_int": 0}, {"ltm_cert": 1, "ltm_int": 1}, {"ltm_cert": 0, "ltm_int": 1})


@pytest.mark.parametrize("max_block", [2048, 4096, 8192, 16384])
def test_encoder_bytes_either_way(hip, oracle, max_block):
    """three blocks and a ragged last block of under 264 samples, 16 / 24 / 32 bits, mono and mid/side: the oracle's bytes
    with ltm_int 0 and 1 and with ltm_cert 0; the certified routes did run (jobs counted)"""
    for i, (bits, nch, ms) in enumerate([(16, 1, 0), (16, 2, 1), (24, 1, 0), (24, 2, 1), (32, 1, 0), (32, 2, 1)]):
        n = 3 * max_block + 150 + 17 * i
        pcm = W.gen("gauss", nch, n, bits, seed=max_block + i) if i % 2 else W.music_like(nch, n, bits, seed=max_block + i)
        p = S.make_params(nch, bits, 48000, parcor=16, ltm=3, lms=8, ms=ms, max_block=max_block, cap=(nch, max_block, 16, 3, 8))
        ret, want, _ = oracle.encode_trace(p, pcm)
        assert ret == 0
        for opts in ROUTES:
            got, st = encode(hip, p, pcm, **opts)
            assert got == want, (bits, nch, ms, opts)
            assert (st[0] > 0) == bool(opts["ltm_cert"]), (opts, st)


def test_encoder_silent_block_and_one_handle(hip, oracle):
    """a file with a silent block in the middle, and one handle taken through all three routes in turn (and back)"""
    max_block, nch, bits = 4096, 2, 24
    pcm = W.music_like(nch, 5 * max_block + 200, bits, seed=9)
    pcm[:, 2 * max_block:3 * max_block] = 0
    p = S.make_params(nch, bits, 48000, parcor=16, ltm=3, lms=8, ms=1, max_block=max_block, cap=(nch, max_block, 16, 3, 8))
    ret, want, _ = oracle.encode_trace(p, pcm)
    assert ret == 0
    enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    try:
        for opts in ROUTES + ROUTES[:2]:
            got, st = encode(hip, p, pcm, enc=enc, **opts)
            assert got == want, opts
    finally:
        enc.close()
