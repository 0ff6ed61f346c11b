"""GPU tests of sla_hip_launch_lpc_far alone (run with -m gpu on an MI355X): the far-window LPC stage, sla_hip_launch_lpc's
semantics for windows of up to 65535 samples staged in global scratch slots (kernels/lpc_far.inc).

    * on windows both kernels take (up to 16384 samples) every output word equals sla_hip_launch_lpc's: the doubles as bit
      patterns, code, kint, rshift -- both forms, with and without mid/side, more groups than scratch slots;
    * above 16384 samples the oracle's LPC entry points decide (autocorr / parcor, the ones
      tests/test_gpu_parity.py::test_lpc_launcher_candidates compares with): block form at orders 1, 16, 48, 255, search form
      on the full 65-node candidate grid of a 65535-sample window and of a 16385-sample window;
    * slots of groups that are not in the launch keep a canary; the refusals launch nothing.

Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import waveforms as W

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 2
NO_WINDOW = 0xFFFFFFFF
SENTINEL = -7.25e100
CANARY = 77


class Group(C.Structure):                      # sla_hip_lpc_group
    _fields_ = [("pcm_off", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


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
    return None if t is None else C.c_void_p(t.data_ptr())


def launch(hip, far, pcm, ms, order, groups, cands, max_window, max_cands, nslots, pool=None, block=False, scratch_slots=3,
           num_groups=None, scratch="own"):
    """one launch of sla_hip_launch_lpc_far (far) or sla_hip_launch_lpc into buffers that hold a sentinel.  pcm: [planes][n]"""
    import torch
    L = hip.lib()
    pcm = np.ascontiguousarray(pcm, np.int32)
    d_pcm, d_g, d_c = _dev(pcm), _groups_dev(groups), _dev(np.array(cands, np.uint32).reshape(-1, 2))
    d_w = _dev(pool) if pool is not None else None
    d_out = torch.full((nslots * (order + 2),), SENTINEL, dtype=torch.float64, device="cuda")
    d_code = torch.full((nslots * (order + 1),), CANARY, dtype=torch.int32, device="cuda") if block else None
    d_kint = torch.full((nslots * (order + 1),), CANARY, dtype=torch.int32, device="cuda") if block else None
    d_rs = torch.full((nslots,), CANARY, dtype=torch.int32, device="cuda") if block else None
    d_scr = torch.zeros((scratch_slots * max_window,), dtype=torch.float64, device="cuda") if scratch == "own" else None
    ng = len(groups) if num_groups is None else num_groups
    torch.cuda.synchronize()
    if far:
        rc = L.sla_hip_launch_lpc_far(_p(d_pcm), C.c_uint64(pcm.shape[1]), ms, order, _p(d_g), ng, max_window, max_cands, _p(d_c), _p(d_w),
                                      _p(d_out), _p(d_code), _p(d_kint), _p(d_rs), _p(d_scr), scratch_slots, None)
    else:
        rc = L.sla_hip_launch_lpc(_p(d_pcm), C.c_uint64(pcm.shape[1]), ms, order, _p(d_g), ng, max_window, max_cands, _p(d_c), _p(d_w),
                                  _p(d_out), _p(d_code), _p(d_kint), _p(d_rs), None)
    torch.cuda.synchronize()
    left = {"out": d_out.cpu().numpy().reshape(nslots, order + 2)}
    if block:
        left.update(code=d_code.cpu().numpy().reshape(nslots, order + 1), kint=d_kint.cpu().numpy().reshape(nslots, order + 1),
                    rshift=d_rs.cpu().numpy())
    return rc, left


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype == np.float64:
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
        else:
            assert np.array_equal(a[k], b[k]), k


def lengths_for(order):
    return sorted({n for n in (1, 2, order - 1, order, order + 1, 3 * order, 3 * order + 1, 2048, 16383, 16384) if n >= 1})


@pytest.fixture(scope="module")
def stereo24():
    return W.music_like(2, 16384, 24, seed=21)


# ------------------------------------------------------------------ against the LDS kernel

@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("order", [1, 16, 32, 255])
def test_search_form_equals_the_lds_kernel(hip, stereo24, order, ms):
    """one group per channel with a candidate of every length of the list, somewhere in a 16384-sample window; two groups over
    one scratch slot"""
    lens = lengths_for(order)
    cands = [((7 * i * 131) % (16384 - n + 1), n) for i, n in enumerate(lens)]
    groups = [Group(0, 16384, ch, NO_WINDOW, 8, 0, len(cands), 1 + ch * len(cands), 0) for ch in range(2)]
    nslots = 2 * len(cands) + 2
    rc_l, lds = launch(hip, False, stereo24, ms, order, groups, cands, 16384, len(cands), nslots)
    rc_f, far = launch(hip, True, stereo24, ms, order, groups, cands, 16384, len(cands), nslots, scratch_slots=1)
    assert rc_l == 0 and rc_f == 0
    same(lds, far)
    assert (far["out"][0] == SENTINEL).all() and (far["out"][-1] == SENTINEL).all()


@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("order", [1, 16, 32, 255])
def test_block_form_equals_the_lds_kernel(oracle, hip, stereo24, order, ms):
    """a windowed group per (length, channel), blocks somewhere in the planes: doubles, codes, lattice coefficients and shifts;
    twenty or so groups over three scratch slots"""
    lens = lengths_for(order)
    pool, woff = [], {}
    for n in lens:
        woff[n] = sum(len(w) for w in pool)
        pool.append(oracle.window(1, n))
    pool = np.concatenate(pool)
    groups, cands = [], []
    for i, n in enumerate(lens):
        for ch in range(2):
            g = len(groups)
            groups.append(Group((i * 977) % (16384 - n + 1), n, ch, woff[n], 8, g, 1, 1 + g, 0))
            cands.append((0, n))
    nslots = len(groups) + 2
    rc_l, lds = launch(hip, False, stereo24, ms, order, groups, cands, 16384, 1, nslots, pool=pool, block=True)
    rc_f, far = launch(hip, True, stereo24, ms, order, groups, cands, 16384, 1, nslots, pool=pool, block=True, scratch_slots=3)
    assert rc_l == 0 and rc_f == 0
    same(lds, far)
    for k in ("code", "kint"):
        assert (far[k][0] == CANARY).all() and (far[k][-1] == CANARY).all()
    assert far["rshift"][0] == CANARY and far["rshift"][-1] == CANARY and (far["out"][0] == SENTINEL).all()


# ------------------------------------------------------------------ above 16384 samples: the oracle

LONG = (16385, 40000, 65534, 65535)


def families(n, seed):
    """(name, int32 samples left-justified, bits): music-like 16-bit, full-scale 32-bit alternating signs, all zero, non-zero only
    in the last sample"""
    alt = np.where(np.arange(n) % 2 == 0, 2 ** 31 - 1, -2 ** 31).astype(np.int64).astype(np.int32)
    last = np.zeros(n, np.int32)
    last[-1] = 12345 << 16
    return [("music16", W.music_like(1, n, 16, seed=seed)[0], 16), ("alternating32", alt, 32), ("zero", np.zeros(n, np.int32), 16),
            ("last_sample", last, 16)]


def quantise(par, rshift):
    """reference src/SLAEncoder.c:567-589 on the oracle's PARCOR doubles"""
    code, kint = np.zeros(len(par), np.int64), np.zeros(len(par), np.int64)
    for o in range(1, len(par)):
        q = 16 if o < 4 else 8
        lim = 1 << (q - 1)
        kq = par[o] * lim
        rk = np.floor(kq + 0.5) if kq >= 0 else -np.floor(-kq + 0.5)
        c = int(min(max(rk, -lim), lim - 1))
        code[o] = c
        kint[o] = (c << (16 - q)) >> rshift            # (Python's shift of a negative integer is arithmetic, as the int32's)
    return code.astype(np.int32), kint.astype(np.int32)


@pytest.fixture(scope="module")
def long_blocks_input(oracle):
    """the sixteen windows (four lengths x four families) back to back in one plane, their window tables, and per window the
    pre-emphasised windowed doubles the reference analyses"""
    plane, pool, items = [], [], []
    woff = {}
    for n in LONG:
        woff[n] = sum(len(w) for w in pool)
        pool.append(oracle.window(1, n))
    for n in LONG:
        for name, x, bits in families(n, seed=n % 97):
            off = sum(len(p) for p in plane)
            plane.append(x)
            xs = oracle.preemph_f64(x.astype(np.float64) * 2.0 ** -31 * pool[LONG.index(n)])
            rshift = max(oracle.bitwidth(x >> (32 - bits)) - 16, 0)
            items.append((name, n, off, woff[n], 32 - bits, xs, rshift))
    return np.concatenate(plane)[None, :], np.concatenate(pool), items


@pytest.mark.parametrize("order", [1, 16, 48, 255])
def test_block_form_above_16384_against_the_oracle(oracle, hip, long_blocks_input, order):
    pcm, pool, items = long_blocks_input
    groups = [Group(off, n, 0, wo, shift, g, 1, 1 + g, 0) for g, (_, n, off, wo, shift, _, _) in enumerate(items)]
    cands = [(0, it[1]) for it in items]
    nslots = len(groups) + 2
    rc, far = launch(hip, True, pcm, 0, order, groups, cands, 65535, 1, nslots, pool=pool, block=True, scratch_slots=5)
    assert rc == 0
    for g, (name, n, _, _, _, xs, rshift) in enumerate(items):
        r0 = oracle.autocorr(xs, 1)[0]
        ret, par = oracle.parcor(xs, order)
        assert ret == 0, (name, n)
        code, kint = quantise(par, rshift)
        o = far["out"][1 + g]
        assert o[0].hex() == r0.hex(), (name, n)
        assert np.array_equal(o[1:].view(np.uint64), par.view(np.uint64)), (name, n)
        assert np.array_equal(far["code"][1 + g], code) and np.array_equal(far["kint"][1 + g], kint), (name, n)
        assert far["rshift"][1 + g] == rshift, (name, n)
        if name == "zero":
            assert r0 < np.finfo(np.float32).eps and not par.any()
    assert (far["out"][0] == SENTINEL).all() and (far["out"][-1] == SENTINEL).all()
    assert far["rshift"][0] == CANARY and far["rshift"][-1] == CANARY and (far["code"][-1] == CANARY).all()


def grid(window):
    """the candidates of the encoder's partition search on one super-frame: every pair of 1024-sample nodes whose clipped
    length is at least the minimum block (reference src/SLAPredictor.c:1615-1630)"""
    nodes = (window + 1023) // 1024 + 1
    out = []
    for p in range(nodes):
        for q in range(p + 1, nodes):
            n = min((q - p) * 1024, window - p * 1024)
            if n >= min(2048, window):
                out.append((p * 1024, n))
    return out


@pytest.mark.parametrize("window,order,family", [(65535, 4, 0), (65535, 4, 1), (65535, 4, 3), (16385, 16, 0), (16385, 16, 2)])
def test_search_form_on_the_full_candidate_grid_against_the_oracle(oracle, hip, window, order, family):
    """every candidate of a super-frame in one group; a second group that is NOT in the launch keeps its slots"""
    name, x, _ = families(window, seed=5)[family]
    cands = grid(window)
    assert len(cands) == (2015 if window == 65535 else 135)
    groups = [Group(0, window, 0, NO_WINDOW, 0, 0, len(cands), 1, 0), Group(0, window, 0, NO_WINDOW, 0, 0, 3, 1 + len(cands), 0)]
    nslots = len(cands) + 5
    rc, far = launch(hip, True, x[None, :], 0, order, groups, cands, window, len(cands), nslots, scratch_slots=1, num_groups=1)
    assert rc == 0
    xf = x.astype(np.float64) * 2.0 ** -31
    for i, (s, n) in enumerate(cands):
        xs = np.ascontiguousarray(xf[s:s + n])
        r0 = oracle.autocorr(xs, 1)[0]
        ret, par = oracle.parcor(xs, order)
        assert ret == 0
        assert far["out"][1 + i, 0].hex() == r0.hex(), (name, s, n)
        assert np.array_equal(far["out"][1 + i, 1:].view(np.uint64), par.view(np.uint64)), (name, s, n)
    assert (far["out"][0] == SENTINEL).all() and (far["out"][1 + len(cands):] == SENTINEL).all()


# ------------------------------------------------------------------ refusals

def test_refusals_launch_nothing(oracle, hip, stereo24):
    n, order = 4096, 8
    pcm = stereo24[:, :n]
    groups, cands, pool = [Group(0, n, 0, 0, 8, 0, 1, 0, 0)], [(0, n)], oracle.window(1, n)
    ok = dict(pcm=pcm, ms=0, order=order, groups=groups, cands=cands, max_window=n, max_cands=1, nslots=1, pool=pool, block=True)

    def refused(**kw):
        a = dict(ok, **kw)
        rc, left = launch(hip, True, a.pop("pcm"), a.pop("ms"), a.pop("order"), a.pop("groups"), a.pop("cands"), a.pop("max_window"),
                          a.pop("max_cands"), a.pop("nslots"), **a)
        assert rc == INVALID_ARGUMENT, kw
        assert (left["out"] == SENTINEL).all() and all((left[k] == CANARY).all() for k in left if k != "out"), kw

    rc, left = launch(hip, True, ok["pcm"], 0, order, groups, cands, n, 1, 1, pool=pool, block=True)
    assert rc == 0 and (left["rshift"] != CANARY).all()
    refused(order=0)
    refused(order=256)
    refused(max_window=65536)
    refused(scratch=None)                         # block form without scratch
    refused(scratch_slots=0)
    refused(max_cands=2)                          # block form: one candidate per group
    refused(pool=None)                            # block form: the window tables
    refused(block=False, pool=None, scratch=None)   # the search form stages through the scratch as well
    # NULL pointers, and max_window 0 (the scratch of the helper would be empty: sized by hand)
    import torch
    L = hip.lib()
    d = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    p = _p(d)
    for bad in range(4):
        args = [p, p, p, p]                        # d_pcm, d_groups, d_cands, d_out
        args[bad] = None
        rc = L.sla_hip_launch_lpc_far(args[0], C.c_uint64(n), 0, order, args[1], 1, n, 1, args[2], None, args[3], None, None, None, p, 1, None)
        assert rc == INVALID_ARGUMENT, bad
    assert L.sla_hip_launch_lpc_far(p, C.c_uint64(n), 0, order, p, 1, 0, 1, p, None, p, None, None, None, p, 1, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_lpc_far(p, C.c_uint64(n), 0, order, p, 1, n, 1, p, None, p, p, None, None, p, 1, None) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any()
