"""GPU tests of the encoder above PARCOR order 48, route by route (run with -m gpu on an MI355X).  A handle accepts orders up to
255 and the encoder changes its code path exactly above 48 (kernels/launchers.inc, sla_encoder.c):

    49 .. 51   tile sums of 52 lags (k_acf_tiles_lds<13, 52>) + k_search_finish<64>; chosen blocks k_acf_blocks<13, 52> +
               k_blocks_finish<64, true> (certificate), what it hands over k_lpc_blocks + k_blocks_finish<64, false>
    52 .. 64   no tile sums: the search takes k_lpc's serial chains; chosen blocks k_lpc_blocks + k_blocks_finish<64, false>
    65 .. 255  k_lpc for the search and for the chosen blocks (Levinson-Durbin and quantiser inside the kernel)

(Order 52 needs 53 lags, one more than the widest tile-sum kernels compute: sla_hip_search_exact_lags(52) == 0, pinned by
tests/test_gpu_acf_lags.py::test_order_51_is_the_last_with_tile_sums.)  First the launchers alone on known operands (k_lpc, the lattice in its pipeline form; the 52-lag tile sums are in
tests/test_gpu_acf_lags.py), then whole files on every route against the oracle, which tests/test_oracle_vs_ref.py pins to the
reference at these orders.  Every comparison is bit for bit, except the PARCOR doubles of certified blocks (slalibs.parcor_same)."""
import ctypes as C

import numpy as np
import pytest

import slalibs as S
import waveforms as W
from test_gpu_parity import assert_same_as_oracle

pytestmark = pytest.mark.gpu

EXCEED_HANDLE_CAPACITY = 3
CAP = lambda nch, maxb: (nch, maxb, 255, 5, 32)
LDS_DOUBLES = (160 * 1024 - 256) // 8          # SLA_HIP_LDS_BUDGET (include/sla_hip.h) in doubles
LAT_T = 17                                     # samples per lane of the lattice wave (kernels/lattice_wave.inc)
SENTINEL = -7.25e100


class Group(C.Structure):                      # sla_hip_lpc_group
    _fields_ = [("pcm_off", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


class Tuning(C.Structure):                     # sla_hip_tuning
    _fields_ = [("lpc_pack", C.c_uint32), ("lpc_threads", C.c_uint32), ("lpc_blocks_chains", C.c_uint32), ("tail_waves", C.c_uint32),
                ("lpc_tile", C.c_uint32), ("tail_taps", C.c_uint32), ("plan_margin", C.c_double), ("rice_lanes", C.c_uint32),
                ("lattice_plain", C.c_uint32), ("cert_audit", C.c_uint32), ("ltm_int", C.c_uint32)]


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _groups_dev(groups):
    import torch
    return torch.frombuffer(bytearray(b"".join(bytes(g) for g in groups)), dtype=torch.uint8).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ sla_hip_launch_lpc (k_lpc)

def run_lpc(hip, pcm, order, window, slices, cands, max_cands):
    """sla_hip_launch_lpc in its search form on one un-windowed window: group g carries the candidates slices[g] = (first,
    count) and writes slot 1 + first onwards.  Returns (result code, slots [len(cands) + 2][order + 2]): slot 0 and the
    last slot belong to nobody"""
    import torch
    L = hip.lib()
    groups = [Group(0, window, 0, 0xFFFFFFFF, 8, first, count, 1 + first, 0) for first, count in slices]
    d_pcm, d_g, d_c = _dev(pcm), _groups_dev(groups), _dev(np.array(cands, np.uint32))
    d_out = torch.full(((len(cands) + 2) * (order + 2),), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_lpc(_p(d_pcm), C.c_uint64(len(pcm)), 0, order, _p(d_g), len(groups), window, max_cands, _p(d_c), None,
                              _p(d_out), None, None, None, None)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy().reshape(len(cands) + 2, order + 2)


def check_lpc(oracle, out, pcm, cands, order):
    """r0 and the order + 1 PARCOR doubles of every candidate: the oracle's bit patterns; nothing written beside them"""
    x = pcm.astype(np.float64) * 2.0 ** -31
    for i, (s, n) in enumerate(cands):
        xs = np.ascontiguousarray(x[s:s + n])
        r0 = oracle.autocorr(xs, 1)[0]
        ret, par = oracle.parcor(xs, order)
        assert ret == 0
        assert out[1 + i, 0].hex() == r0.hex(), (order, i, s, n)
        assert np.array_equal(out[1 + i, 1:].view(np.uint64), par.view(np.uint64)), (order, i, s, n)
        if n < order:
            assert not par.any()
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all()


@pytest.mark.parametrize("order", [49, 64, 65, 128, 255])
def test_lpc_launcher_at_order(oracle, hip, order):
    """the eight sub-ranges of tests/test_gpu_parity.py::test_lpc_launcher_candidates and candidates of order - 1, order,
    order + 1, 1 and 2 samples: the n < order zero branch and the chains whose lag reaches the candidate's length"""
    window = 4096
    pcm = W.music_like(1, window, 24, seed=12)[0]
    cands = [(0, 2048), (0, 3072), (0, 4096), (1024, 2048), (1024, 3072), (2048, 2048), (100, 37), (5, 9),
             (7, order - 1), (11, order), (13, order + 1), (4000, 1), (4001, 2)]
    rc, out = run_lpc(hip, pcm, order, window, [(0, len(cands))], cands, len(cands))
    assert rc == 0
    check_lpc(oracle, out, pcm, cands, order)


def test_lpc_launcher_slices_a_16384_window_at_order_255(oracle, hip):
    """the slicing rule of the encoder's search tables: a group carries as many candidates as the LDS budget leaves room for
    r[] behind its window -- 15 at 16384 samples and order 255 -- and one candidate more goes to a second group"""
    order, window = 255, 16384
    per_group = (LDS_DOUBLES - window) // (order + 1)
    assert per_group == 15
    pcm = W.music_like(1, window, 24, seed=13)[0]
    cands = [(i * 1024, window - i * 1024) for i in range(8)] + [(0, (k + 2) * 1024) for k in range(8)]
    assert len(cands) == per_group + 1
    rc, out = run_lpc(hip, pcm, order, window, [(0, per_group), (per_group, 1)], cands, per_group)
    assert rc == 0
    check_lpc(oracle, out, pcm, cands, order)
    # one candidate more in a group does not fit: refused by the launcher, before anything is launched
    rc, out = run_lpc(hip, pcm, order, window, [(0, per_group + 1)], cands, per_group + 1)
    assert rc == EXCEED_HANDLE_CAPACITY and (out == SENTINEL).all()


def test_lpc_launcher_work_vectors_wider_than_the_window(oracle, hip):
    """2048 samples, 6 candidates, order 255: the Levinson work vectors that overlay the window, 2 * 6 * (order + 2) doubles,
    are longer than the window itself, and the window's region grows to hold them"""
    order, window = 255, 2048
    cands = [(0, 2048), (0, 1024), (1024, 1024), (512, 1536), (100, 300), (1700, 256)]
    assert 2 * len(cands) * (order + 2) > window
    pcm = W.music_like(1, window, 24, seed=14)[0]
    rc, out = run_lpc(hip, pcm, order, window, [(0, len(cands))], cands, len(cands))
    assert rc == 0
    check_lpc(oracle, out, pcm, cands, order)


def test_lpc_launcher_search_slices_of_an_8192_window_at_order_255(oracle, hip):
    """The 28 search candidates of an 8192-sample super-frame at order 255.  Their r[] fits behind the window
    (8192 + 28 * 256 doubles), their work vectors do not fit in front of it (28 * 514 + 28 * 256 doubles): one group of 28 is
    refused by the launcher -- the encoder used to build exactly that group and failed in the middle of EncodeWhole -- and
    the slices the encoder makes now, 26 + 2, give the oracle's doubles"""
    order, window = 255, 8192
    nodes = window // 1024 + 1
    cands = [(i * 1024, (j - i) * 1024) for i in range(nodes) for j in range(i + 2, nodes)]
    assert len(cands) == 28 and window + len(cands) * (order + 1) <= LDS_DOUBLES
    per_group = min((LDS_DOUBLES - window) // (order + 1), LDS_DOUBLES // (2 * (order + 2) + order + 1))
    assert per_group == 26
    pcm = W.music_like(1, window, 24, seed=15)[0]
    rc, out = run_lpc(hip, pcm, order, window, [(0, len(cands))], cands, len(cands))
    assert rc == EXCEED_HANDLE_CAPACITY and (out == SENTINEL).all()
    rc, out = run_lpc(hip, pcm, order, window, [(0, per_group), (per_group, len(cands) - per_group)], cands, per_group)
    assert rc == 0
    check_lpc(oracle, out, pcm, cands, order)


def run_chosen_blocks(hip, oracle, order, fused):
    """sla_hip_launch_lpc in its quantiser form (fused: sla_hip_launch_lpc_blocks, the lattice in the same launch) on the two
    channels of a one-block file.  Returns (result code, the oracle's trace of that file, what the launch left)"""
    import torch
    L = hip.lib()
    n, nch, bits = 4096, 2, 24
    pcm = W.music_like(nch, n, bits, seed=order)
    p = S.make_params(nch, bits, 48000, order, 1, 8, 0, 1, n, cap=CAP(nch, n))
    ret, _, to = oracle.encode_trace(p, pcm)
    assert ret == 0 and to.num_blocks == 1 and to.blk_type[0] == 0 and to.offset_lshift == 0
    groups = [Group(0, n, ch, 0, 32 - bits, ch, 1, ch, 0) for ch in range(nch)]
    d_pcm, d_g, d_c, d_w = _dev(pcm), _groups_dev(groups), _dev(np.array([(0, n)] * nch, np.uint32)), _dev(oracle.window(1, n))
    d_out = torch.full(((nch + 1) * (order + 2),), SENTINEL, dtype=torch.float64, device="cuda")      # (one slot more than written)
    d_code = torch.full(((nch + 1) * (order + 1),), 77, dtype=torch.int32, device="cuda")
    d_kint = torch.full(((nch + 1) * (order + 1),), 77, dtype=torch.int32, device="cuda")
    d_rs = torch.full((nch + 1,), 77, dtype=torch.int32, device="cuda")
    d_res = torch.full((nch * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if fused:
        rc = L.sla_hip_launch_lpc_blocks(_p(d_pcm), C.c_uint64(n), 0, order, _p(d_g), nch, n, _p(d_c), _p(d_w), _p(d_out), _p(d_code),
                                         _p(d_kint), _p(d_rs), _p(d_res), None)
    else:
        rc = L.sla_hip_launch_lpc(_p(d_pcm), C.c_uint64(n), 0, order, _p(d_g), nch, n, 1, _p(d_c), _p(d_w), _p(d_out), _p(d_code),
                                  _p(d_kint), _p(d_rs), None)
    torch.cuda.synchronize()
    left = {"out": d_out.cpu().numpy().reshape(nch + 1, order + 2), "code": d_code.cpu().numpy().reshape(nch + 1, order + 1),
            "kint": d_kint.cpu().numpy().reshape(nch + 1, order + 1), "rshift": d_rs.cpu().numpy(), "res": d_res.cpu().numpy().reshape(nch, n)}
    return rc, to, left


def check_chosen_blocks(to, left, nch=2):
    assert np.array_equal(left["out"][:nch, 1:].view(np.uint64), to.parcor[0].view(np.uint64))
    assert np.array_equal(left["code"][:nch], to.code[0]) and np.array_equal(left["kint"][:nch], to.kint[0])
    assert np.array_equal(left["rshift"][:nch].view(np.uint32), to.rshift[0])
    assert (left["out"][nch] == SENTINEL).all() and (left["code"][nch] == 77).all() and (left["kint"][nch] == 77).all() and left["rshift"][nch] == 77


@pytest.mark.parametrize("order", [49, 51, 63, 64, 65])
def test_lpc_launcher_quantiser_form_at_order(oracle, hip, order):
    """the chosen blocks' exact launcher: k_lpc_blocks + k_blocks_finish<64, false> from order 49 to 64 -- at 64 the 65
    autocorrelation values of a window are one more than the wave that hands them over has lanes -- and k_lpc from 65 on:
    PARCOR doubles, codes, lattice coefficients and shift of the oracle's trace, in buffers that held a sentinel (a whole-file
    encode reuses device memory that an earlier encode may have left the right codes in)"""
    rc, to, left = run_chosen_blocks(hip, oracle, order, fused=False)
    assert rc == 0
    check_chosen_blocks(to, left)
    assert (left["res"] == 0x5A5A5A5A).all()


def test_lpc_blocks_launcher_fuses_the_lattice_up_to_order_63(oracle, hip):
    """sla_hip_launch_lpc_blocks runs the recursion inside k_lpc_blocks, coefficient j in lane j of one wave: order 63 is the
    last that fits, order 64 is refused and nothing is written"""
    rc, to, left = run_chosen_blocks(hip, oracle, 63, fused=True)
    assert rc == 0
    check_chosen_blocks(to, left)
    assert np.array_equal(left["res"], to.res_lattice[:, :4096])
    rc, to, left = run_chosen_blocks(hip, oracle, 64, fused=True)
    assert rc == 2                                               # SLA_APIRESULT_INVALID_ARGUMENT
    assert (left["out"] == SENTINEL).all() and (left["code"] == 77).all() and (left["res"] == 0x5A5A5A5A).all()


# ------------------------------------------------------------------ the lattice in its pipeline form (k_lattice_groups)

@pytest.mark.parametrize("order", [64, 65, 255])
def test_lattice_groups_at_order(oracle, hip, order):
    """sla_hip_launch_lattice_groups on two blocks of one plane, 2048 samples and two full waves + 5 (4, 5 and 15 halo lanes
    per wave), left-justified 24-bit input with its shift, certified stage forms and plain ones"""
    import torch
    L = hip.lib()
    rng = np.random.default_rng(order)
    per = (64 - (order + LAT_T - 1) // LAT_T) * LAT_T
    lens = [2048, 2 * per + 5]
    offs = [3, 3 + lens[0] + 7]
    plane = offs[1] + lens[1] + 11
    x24 = rng.integers(-(1 << 23), 1 << 23, plane, dtype=np.int64).astype(np.int32)
    kint = np.zeros((2, order + 1), np.int32)
    kint[:, 1:] = rng.integers(-120, 121, (2, order))
    groups = [Group(offs[g], lens[g], 0, 0xFFFFFFFF, 8, g, 1, g, 0) for g in range(2)]
    d_pcm, d_g, d_k = _dev((x24.astype(np.int64) << 8).astype(np.int32)), _groups_dev(groups), _dev(kint)
    for plain in (0, 1):
        d_res = torch.full((plane,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        tuning = Tuning()
        tuning.lattice_plain = plain
        L.sla_hip_use_tuning(C.byref(tuning))
        try:
            rc = L.sla_hip_launch_lattice_groups(_p(d_pcm), C.c_uint64(plane), 0, order, _p(d_g), 2, max(lens), _p(d_k), _p(d_res), None)
        finally:
            L.sla_hip_use_tuning(None)
        assert rc == 0
        torch.cuda.synchronize()
        res = d_res.cpu().numpy()
        touched = np.zeros(plane, bool)
        for g in range(2):
            want = oracle.lattice_predict(oracle.preemph_i32(x24[offs[g]:offs[g] + lens[g]]), kint[g])
            assert np.array_equal(res[offs[g]:offs[g] + lens[g]], want), (order, g, plain)
            touched[offs[g]:offs[g] + lens[g]] = True
        assert (res[~touched] == 0x5A5A5A5A).all(), (order, plain)


# ------------------------------------------------------------------ whole files

COMPRESS, SILENT, RAW = 0, 1, 2


def gapped(nch, n, bits, seed):
    """programme-like material with 3152 samples of digital silence from sample 2048 on and 2100 samples of full-scale white
    noise behind them: COMPRESS blocks that use the long-term filter, a SILENT block and a RAW block in one short file.
    (The silence starts on the 1024-sample grid of the partition search: at 3000 the one-channel file below has no SILENT block.)"""
    pcm = W.music_like(nch, n, bits, seed=seed)
    pcm[:, 2048:5200] = 0
    pcm[:, 5200:7300] = W.gen("white", nch, 2100, bits, seed=seed)
    return np.ascontiguousarray(pcm)


def two_files(order):
    """[(parameters, samples)]: one channel of 16 bits whose last block is one sample shorter than the order, two channels of
    24 bits mid/side whose last block is one sample longer than 2048 + order"""
    n1, n2 = 2 * 4096 + order - 1, 8192 + 2048 + order + 1
    return [(S.make_params(1, 16, 48000, order, 3, 8, 0, 1, 4096, cap=CAP(1, 4096)), gapped(1, n1, 16, order)),
            (S.make_params(2, 24, 48000, order, 3, 16, 1, 1, 8192, cap=CAP(2, 8192)), gapped(2, n2, 24, order))]


def assert_all_block_kinds(oracle, p, pcm):
    ret, _, to = oracle.encode_trace(p, pcm)
    assert ret == 0
    nb = to.num_blocks
    kinds = to.blk_type[:nb]
    assert (kinds == SILENT).any() and (kinds == RAW).any()
    assert (to.pitch[:nb][kinds == COMPRESS] >= 3).any()


@pytest.mark.parametrize("order", [49, 51, 52, 53, 64, 65, 100, 128, 255])
def test_encode_at_order(oracle, hip, order):
    for p, pcm in two_files(order):
        assert_all_block_kinds(oracle, p, pcm)
        assert_same_as_oracle(oracle, hip, p, pcm)


def encode(hip, p, pcm, **options):
    """one whole-file encode on a fresh handle; returns the bytes and what the handle reports about the routes it took"""
    enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    try:
        for k, v in options.items():
            enc.set_option(k, v)
        enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
        enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method, p.window_type, p.max_block_samples)
        data = enc.encode_whole(pcm)
        if options.get("stream"):
            return data, None                                # the pieces were analysed on worker lanes: nothing to read on this handle
        rerun, host_planned, exact_search, device_plan, _, device_ltm = enc.last_counters()
        cert_on, redone = enc.last_block_cert()
        report = {"tile_sums": exact_search, "device_plan": device_plan, "device_ltm": device_ltm, "block_cert": cert_on,
                  "redone": redone, "ltm_cert": enc.last_ltm_cert(), "verify": enc.last_verify(), "trace": enc.trace(False)}
        return data, report
    finally:
        enc.close()


@pytest.mark.parametrize("order", [51, 52, 64, 255])
def test_tail_of_exactly_order_samples(oracle, hip, order):
    """A last super-frame of exactly `order` samples.  The reference leaves the autocorrelation's lag `order` unwritten there
    and its recursion consumes what the super-frame before left in the scratch (src/SLAPredictor.c:344-346): the reference
    never returns, and the oracle, which keeps that scratch too, gives the whole file up with FAILED_TO_CALCULATE_COEF -- there
    are no oracle bytes of the whole file to compare with.  The library takes zero for the unwritten lag,
    which is what the oracle does on a fresh scratch; blocks are independent, so its bytes must be the oracle's block for the
    first 4096 samples followed by the oracle's block for the last `order` samples encoded as a range of their own, and the
    file must decode to the input"""
    n = 4096 + order
    pcm = W.music_like(1, n, 16, seed=order)
    p = S.make_params(1, 16, 48000, order, 3, 8, 0, 1, 4096, cap=CAP(1, 4096))
    assert oracle.encode_whole(p, pcm)[0] == 6
    ret, head, to = oracle.encode_trace(p, np.ascontiguousarray(pcm[:, :4096]))
    assert ret == 0 and to.num_blocks == 1
    ret, tail = oracle.encode_range(p, np.ascontiguousarray(pcm[:, 4096:]), to.offset_lshift)
    assert ret == 0
    got, rep = encode(hip, p, pcm, stream=0)
    tr = rep["trace"]
    assert tr.num_blocks == 2 and list(tr.blk_nsmpl[:2]) == [4096, order] and tr.offset_lshift == to.offset_lshift
    assert got[43:] == head[43:] + tail[43:]
    rd, dec, hdr = oracle.decode_whole(p, got, n)
    assert rd == 0 and np.array_equal(dec, pcm) and hdr[9] == 2


def test_capacity_equal_to_order(oracle, hip):
    order = 255
    pcm = gapped(1, 2 * 4096 + order - 1, 16, order)
    p = S.make_params(1, 16, 48000, order, 3, 8, 0, 1, 4096, cap=(1, 4096, 255, 3, 8))
    assert_all_block_kinds(oracle, p, pcm)
    assert_same_as_oracle(oracle, hip, p, pcm)


ROUTES = [{}, {"block_cert": 0}, {"search_exact": 0}, {"device_plan": 0}, {"lpc_blocks_chains": 1}, {"chunks": 3},
          {"chunks": 3, "single_tail": 0}, {"device_ltm": 0}, {"stream": 1, "stream_piece": 1024, "stream_lanes": 2}, {"verify": 1},
          {"fuse_lattice": 1}, {"lattice_plain": 1}]


@pytest.mark.parametrize("order", [51, 52, 64, 200])
def test_routes_agree_at_order(oracle, hip, order):
    """every switch of the handle that picks another route through the analysis: the oracle's bytes each time, and the
    handle's own report says that the route in question ran"""
    nch, n = 2, 5 * 4096 + 777
    pcm = W.music_like(nch, n, 16, seed=order)
    p = S.make_params(nch, 16, 48000, order, 3, 8, 1, 1, 4096, cap=CAP(nch, 4096))
    ret, want, to = oracle.encode_trace(p, pcm)
    assert ret == 0
    comp = to.blk_type[:to.num_blocks] == COMPRESS
    assert comp.any()
    for opts in ROUTES:
        if "fuse_lattice" in opts and order > 64:
            continue                                         # the fused lattice lives in k_lpc_blocks: orders up to 64
        got, rep = encode(hip, p, pcm, **dict({"stream": 0}, **opts))
        assert got == want, (order, opts)
        if rep is None:
            continue
        tr = rep["trace"]
        certified = int((tr.parcor_exact[:to.num_blocks][comp] == 0).sum())
        if order <= 51:
            assert rep["tile_sums"] == (0 if opts.get("search_exact") == 0 else 1), opts
            if opts.get("block_cert") == 0 or opts.get("lpc_blocks_chains") or opts.get("fuse_lattice"):
                assert rep["block_cert"] == 0 and certified == 0, opts
            else:
                assert rep["block_cert"] == 1 and certified > 0, opts
        else:
            assert rep["tile_sums"] == 0 and rep["block_cert"] == 0 and certified == 0, opts
        assert rep["device_plan"] == (0 if opts.get("device_plan") == 0 else 1), opts
        assert rep["device_ltm"] == (0 if opts.get("device_ltm") == 0 else 1), opts
        jobs, ltm_certified, ltm_fallback, _, audit_bad = rep["ltm_cert"]
        if opts.get("device_ltm") == 0:
            assert jobs == 0, opts
        else:
            assert jobs > 0 and ltm_certified + ltm_fallback == jobs and audit_bad == 0, opts
        compared, differed, _, blocks, bad_blocks = rep["verify"]
        if opts.get("verify"):
            assert compared == nch * n and differed == 0 and blocks == to.num_blocks and bad_blocks == 0
        else:
            assert compared == 0


def test_batch_and_device_routes_at_order_100(oracle, hip):
    """three clips through sla_hip_encode_batch and, from one padded device tensor, through sla_hip_encode_batch_device: the
    oracle's per-file bytes, which the HIP decoder turns back into the input"""
    import torch
    order, nch = 100, 2
    lens = [9000, 4096, 2049]
    p = S.make_params(nch, 16, 48000, order, 3, 8, 1, 1, 4096, cap=CAP(nch, 4096))
    clips = [W.music_like(nch, n, 16, seed=100 + i) for i, n in enumerate(lens)]
    want = []
    for pcm in clips:
        ret, data = oracle.encode_whole(p, pcm)
        assert ret == 0
        want.append((0, data))
    padded = np.zeros((len(clips), nch, max(lens)), np.int32)
    for i, pcm in enumerate(clips):
        padded[i, :, :lens[i]] = pcm
    enc = hip.Encoder(*CAP(nch, 4096))
    try:
        enc.set_wave_format(nch, 16, 48000)
        enc.set_encode_parameter(order, 3, 8, 1, 1, 4096)
        assert enc.encode_batch(clips) == want
        assert enc.encode_batch_tensor(torch.from_numpy(padded).cuda(), lens) == want
    finally:
        enc.close()
    dec = hip.Decoder(*CAP(nch, 4096))
    try:
        for (_, data), pcm in zip(want, clips):
            rc, back = dec.decode_whole(data, pcm.shape[1])
            assert rc == 0 and np.array_equal(back, pcm)
    finally:
        dec.close()
