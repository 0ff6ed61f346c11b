"""GPU tests of sla_hip_launch_search_far and sla_hip_launch_lpc_far_rerun alone (run with -m gpu on an MI355X): the tile-sum
search for windows of up to 65535 samples (64 tiles; kernels/search_far.inc, the tile kernels of kernels/search.inc with a
stride of SLA_HIP_XTILES_FAR) and the rerun of the groups it flags.

    * every output word equals the far chains' (sla_hip_launch_lpc_far, search form, itself pinned to the oracle by
      tests/test_gpu_lpc_far.py) on the full candidate grid -- 2015 candidates at 65535 samples, several finish workgroups per
      group -- beside a group of three candidates, at one order per instantiation of the tile and finish kernels, mono and
      mid/side, on full-range 16-bit operands at a pcm_off that is no multiple of 4;
    * the oracle's autocorr / parcor on the full grids of 65535 (order 4) and 16385 (order 16);
    * on a 16384-sample window: sla_hip_launch_search_exact's output with cert_safety 0, and its tile sums;
    * the limit is strict; flagged groups carry NaN in r[0] of every candidate and nothing else; the rerun redoes exactly the
      flagged groups -- one of them flagged in its first slot only -- and counts them;
    * slots of groups that are not in the launch keep a sentinel; the refusals launch nothing.

Every comparison is exact equality."""
import ctypes as C
import math

import numpy as np
import pytest

import longsearchmodel as M
import waveforms as W

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 2
EXCEED_HANDLE_CAPACITY = 3
NO_WINDOW = 0xFFFFFFFF
SENTINEL = -7.25e100
XTILES, XTILES_FAR = 16, 64


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


def limit16(ms):
    """the encoder's limit for 16-bit material at exact_bits 53: 2^53 units^2, unit 2^(16 - 31 - ms)"""
    return 2.0 ** (53 + 2 * (16 - 31 - ms))


class Bench:
    """the device buffers of one set of groups; every launcher writes into `out`, which starts as sentinels"""

    def __init__(self, hip, pcm, ms, order, groups, cands, max_window, max_cands, nslots, num_groups=None):
        import torch
        self.L, self.ms, self.order = hip.lib(), ms, order
        self.pcm = np.ascontiguousarray(pcm, np.int32)
        self.d_pcm, self.d_g, self.d_c = _dev(self.pcm), _groups_dev(groups), _dev(np.array(cands, np.uint32).reshape(-1, 2))
        self.ng = len(groups) if num_groups is None else num_groups
        self.max_window, self.max_cands, self.nslots = max_window, max_cands, nslots
        self.lags = self.L.sla_hip_search_exact_lags(order)
        self.fresh()

    def fresh(self):
        import torch
        self.out = torch.full((self.nslots * (self.order + 2),), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

    def left(self):
        import torch
        torch.cuda.synchronize()
        return self.out.cpu().numpy().reshape(self.nslots, self.order + 2)

    def tiles(self, stride):
        import torch
        n = max(self.ng, 1) * stride * 2 * max(self.lags, 12)
        return torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")

    def search_far(self, limit, **kw):
        a = dict(pcm=_p(self.d_pcm), groups=_p(self.d_g), cands=_p(self.d_c), out=_p(self.out), order=self.order,
                 max_window=self.max_window, max_cands=self.max_cands)
        self.ts = self.tiles(XTILES_FAR)
        a["ts"] = _p(self.ts)
        a.update(kw)
        rc = self.L.sla_hip_launch_search_far(a["pcm"], self.pcm.shape[1], self.ms, a["order"], a["groups"], self.ng, a["max_window"],
                                              a["max_cands"], a["cands"], a["ts"], a["out"], limit, None)
        return rc

    def search_exact(self, limit):
        self.ts = self.tiles(XTILES)
        return self.L.sla_hip_launch_search_exact(_p(self.d_pcm), C.c_uint64(self.pcm.shape[1]), self.ms, self.order, _p(self.d_g), self.ng,
                                                  self.max_window, self.max_cands, _p(self.d_c), _p(self.ts), _p(self.out),
                                                  C.c_double(limit), C.c_double(0.0), None, None)

    def chains(self, scratch_slots=2):
        import torch
        scr = torch.zeros((scratch_slots * self.max_window,), dtype=torch.float64, device="cuda")
        return self.L.sla_hip_launch_lpc_far(_p(self.d_pcm), C.c_uint64(self.pcm.shape[1]), self.ms, self.order, _p(self.d_g), self.ng,
                                             self.max_window, self.max_cands, _p(self.d_c), None, _p(self.out), None, None, None,
                                             _p(scr), scratch_slots, None)

    def rerun(self, scratch_slots=2):
        import torch
        scr = torch.zeros((scratch_slots * self.max_window,), dtype=torch.float64, device="cuda")
        cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
        rc = self.L.sla_hip_launch_lpc_far_rerun(_p(self.d_pcm), self.pcm.shape[1], self.ms, self.order, _p(self.d_g), self.ng,
                                                 self.max_window, self.max_cands, _p(self.d_c), _p(self.out), _p(scr), scratch_slots,
                                                 _p(cnt), None)
        torch.cuda.synchronize()
        return rc, int(cnt.cpu()[0])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def full16(nch, n, seed):
    """full-range 16-bit samples, left-justified, every other one (at random) at an extreme.  Two channels: the second is the
    first's complement (-l - 1) at three samples of four, so that side = l - r comes close to twice the full scale there --
    |side| < 2 in the search's unit, an energy of up to 4 x the length, is what the limit of 16-bit material has to admit --
    and independent of it at the others, where mid is more than a constant"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(nch, n), dtype=np.int64)
    x = np.where(rng.random((nch, n)) < 0.5, np.where(rng.integers(0, 2, size=(nch, n)) == 0, -32768, 32767), x)
    if nch == 2:
        x[1] = np.where(rng.random(n) < 0.75, -x[0] - 1, x[1])
    return (x << 16).astype(np.int32)


def small_cands(window):
    return [(0, min(2048, window)), (1024, window - 1024), (0, window)]


def layout(window, nch, pcm_off):
    """per channel: a group with the full grid and a group with three candidates; one more group that is NOT in the launch.
    Slot 0 and the last slot belong to nobody."""
    cands = M.grid(window)
    small = small_cands(window)
    groups, slot = [], 1
    for ch in range(nch):
        groups.append(Group(pcm_off, window, ch, NO_WINDOW, 16, 0, len(cands), slot, 0))
        slot += len(cands)
        groups.append(Group(pcm_off, window, ch, NO_WINDOW, 16, len(cands), len(small), slot, 0))
        slot += len(small)
    groups.append(Group(pcm_off, window, 0, NO_WINDOW, 16, len(cands), len(small), slot, 0))
    launched = slot
    slot += len(small)
    return cands + small, groups, slot + 1, launched, len(cands)


# ------------------------------------------------------------------ bit for bit against the far chains

# one order per instantiation: 12; 20/20; 20/17; 36/36; 36/33; 52/52; 52/49; 52/52 -- 65535 and 16385 at each, the other windows at 16 and 48
ORDERS = (4, 13, 16, 20, 32, 40, 48, 51)
SHAPES = [(w, o) for o in ORDERS for w in (65535, 16385)] + [(w, o) for o in (16, 48) for w in (17408, 17413, 32769)]


def against_chains(hip, window, order, nch, ms, pcm_off):
    cands, groups, nslots, launched, ngrid = layout(window, nch, pcm_off)
    pcm = full16(nch, pcm_off + window + 7, seed=window % 1000 + order)
    b = Bench(hip, pcm, ms, order, groups, cands, window, ngrid, nslots, num_groups=len(groups) - 1)
    assert b.search_far(limit16(ms)) == 0
    far = b.left()
    b.fresh()
    assert b.chains() == 0
    ref = b.left()
    assert not np.isnan(ref[1:launched]).any()
    assert np.array_equal(bits(far), bits(ref))
    assert (far[0] == SENTINEL).all() and (far[launched:] == SENTINEL).all()      # before, not in the launch, after
    return b, far


@pytest.mark.parametrize("window,order", SHAPES)
def test_mono_equals_the_far_chains(hip, window, order):
    if window == 65535:
        assert len(M.grid(window)) == 2015            # eight finish workgroups for one group
    against_chains(hip, window, order, 1, 0, 3)


@pytest.mark.parametrize("window,order", [(65535, 16), (16385, 48), (17413, 16), (32769, 48), (16385, 4)])
def test_mid_side_equals_the_far_chains_on_both_channels(hip, window, order):
    b, far = against_chains(hip, window, order, 2, 1, 5)
    # the energy of the side channel is near the top of what 4 x the window admits
    ntiles = (window + 1023) // 1024
    ts = b.ts.cpu().numpy().reshape(-1, XTILES_FAR, 2, b.lags)
    side = ts[2, :ntiles, 0, 0].sum()                # group 2: channel 1, full grid
    assert 2.0 * window < side < 4.0 * window


# ------------------------------------------------------------------ the oracle

@pytest.mark.parametrize("window,order", [(65535, 4), (16385, 16)])
def test_full_grid_against_the_oracle(oracle, hip, window, order):
    x = W.music_like(1, window, 16, seed=5)[0]
    cands = M.grid(window)
    groups = [Group(0, window, 0, NO_WINDOW, 16, 0, len(cands), 1, 0), Group(0, window, 0, NO_WINDOW, 16, 0, 3, 1 + len(cands), 0)]
    b = Bench(hip, x[None, :], 0, order, groups, cands, window, len(cands), len(cands) + 5, num_groups=1)
    assert b.search_far(limit16(0)) == 0
    far = b.left()
    xf = x.astype(np.float64) * 2.0 ** -31
    for i, (s, n) in enumerate(cands):
        xs = np.ascontiguousarray(xf[s:s + n])
        r0 = oracle.autocorr(xs, 1)[0]
        ret, par = oracle.parcor(xs, order)
        assert ret == 0
        assert far[1 + i, 0].hex() == r0.hex(), (s, n)
        assert np.array_equal(bits(far[1 + i, 1:]), bits(par)), (s, n)
    assert (far[0] == SENTINEL).all() and (far[1 + len(cands):] == SENTINEL).all()


# ------------------------------------------------------------------ sla_hip_launch_search_exact

@pytest.mark.parametrize("order,ms", [(16, 0), (51, 1), (4, 1)])
def test_a_16384_sample_window_equals_search_exact(hip, order, ms):
    window, nch = 16384, 1 + ms
    cands, groups, nslots, launched, ngrid = layout(window, nch, 3)
    pcm = full16(nch, window + 16, seed=order)
    b = Bench(hip, pcm, ms, order, groups, cands, window, ngrid, nslots, num_groups=len(groups) - 1)
    assert b.search_far(limit16(ms)) == 0
    far, far_ts = b.left(), b.ts.cpu().numpy().reshape(-1, XTILES_FAR, 2, b.lags)
    b.fresh()
    assert b.search_exact(limit16(ms)) == 0
    ex, ex_ts = b.left(), b.ts.cpu().numpy().reshape(-1, XTILES, 2, b.lags)
    assert np.array_equal(bits(far), bits(ex))
    # the tile sums both define: 16 tiles, the lags up to the order, P and X
    assert np.array_equal(bits(far_ts[:b.ng, :XTILES, :, :order + 1]), bits(ex_ts[:b.ng, :, :, :order + 1]))
    assert (far_ts[:b.ng, XTILES:] == SENTINEL).all() and (far_ts[b.ng:] == SENTINEL).all()


# ------------------------------------------------------------------ the limit and the rerun

def constant_magnitude(n, k, seed):
    rng = np.random.default_rng(seed)
    return (np.where(rng.integers(0, 2, size=n) == 0, -k, k).astype(np.int64) << 16).astype(np.int32)


@pytest.fixture(scope="module")
def limit_bench(hip):
    """three mono groups back to back in one plane: magnitudes 1000 and 1200 (E1 < E2), and a third like the first"""
    order = 8
    n1, n2, n3, k1, k2 = 17000, 20000, 20000, 1000, 1200
    plane = np.concatenate([constant_magnitude(n1, k1, 1), constant_magnitude(n2, k2, 2), constant_magnitude(n3, k1, 3)])
    e1, e2 = n1 * k1 * k1, n2 * k2 * k2                      # in units^2 of 2^-30: exact integers below 2^53
    E1, E2 = float(e1) * 2.0 ** -30, float(e2) * 2.0 ** -30
    assert e1 < e2 < 2 ** 53 and n3 * k1 * k1 < e2 and n3 * k1 * k1 > e1
    cands, groups, slot = [], [], 1
    for off, n in ((0, n1), (n1, n2), (n1 + n2, n3)):
        g = M.grid(n)
        groups.append(Group(off, n, 0, NO_WINDOW, 16, len(cands), len(g), slot, 0))
        cands += g
        slot += len(g)
    assert groups[2].cand_count > 2 * 64                     # the third group's finish lanes spread over several workgroups
    b = Bench(hip, plane[None, :], 0, order, groups, cands, 20000, max(g.cand_count for g in groups), slot + 1)
    b.chains(scratch_slots=2)
    return b, groups, E1, E2, b.left()


def slots_of(g):
    return slice(g.slot_first, g.slot_first + g.cand_count)


def flagged_only(rows):
    return np.isnan(rows[:, 0]).all() and (rows[:, 1:] == SENTINEL).all()


def test_the_limit_is_strict(limit_bench):
    b, groups, E1, E2, ref = limit_bench
    g1, g2, g3 = (slots_of(g) for g in groups)
    b.fresh()
    assert b.search_far(E2) == 0
    out = b.left()
    assert np.array_equal(bits(out[g1]), bits(ref[g1])) and flagged_only(out[g2]) and np.array_equal(bits(out[g3]), bits(ref[g3]))
    b.fresh()
    assert b.search_far(math.nextafter(E2, math.inf)) == 0
    assert np.array_equal(bits(b.left()), bits(ref))
    b.fresh()
    assert b.search_far(E1) == 0
    out = b.left()
    assert flagged_only(out[g1]) and flagged_only(out[g2]) and flagged_only(out[g3])
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all()


def test_the_rerun_redoes_the_flagged_groups_and_counts_them(limit_bench):
    import torch
    b, groups, E1, E2, ref = limit_bench
    g1, g2, g3 = (slots_of(g) for g in groups)
    b.fresh()
    assert b.search_far(E2) == 0
    # the third group: sentinels everywhere but NaN in r[0] of its FIRST slot -- the word the finish kernel's first workgroup of
    # the group rewrites while its other workgroups may not have started
    rows = b.out.view(b.nslots, b.order + 2)
    rows[g3] = SENTINEL
    rows[groups[2].slot_first, 0] = float("nan")
    torch.cuda.synchronize()
    before = b.left().copy()
    rc, count = b.rerun(scratch_slots=2)
    assert rc == 0 and count == 2
    after = b.left()
    assert np.array_equal(bits(after[g1]), bits(before[g1])) and np.array_equal(bits(before[g1]), bits(ref[g1]))
    assert np.array_equal(bits(after[g2]), bits(ref[g2]))
    assert np.array_equal(bits(after[g3]), bits(ref[g3]))
    assert (after[0] == SENTINEL).all() and (after[-1] == SENTINEL).all()
    # nothing flagged: nothing changes, nothing is counted
    rc, count = b.rerun(scratch_slots=1)
    assert rc == 0 and count == 0 and np.array_equal(bits(b.left()), bits(after))


# ------------------------------------------------------------------ refusals

def test_refusals_launch_nothing(hip):
    window, order = 4096, 8
    cands = M.grid(window)
    groups = [Group(0, window, 0, NO_WINDOW, 16, 0, len(cands), 0, 0)]
    b = Bench(hip, full16(1, window, seed=1), 0, order, groups, cands, window, len(cands), len(cands))
    assert b.search_far(limit16(0)) == 0 and not (b.left() == SENTINEL).any()

    def refused(code, **kw):
        b.fresh()
        assert b.search_far(limit16(0), **kw) == code, kw
        assert (b.left() == SENTINEL).all(), kw
        if kw.get("ts", 1) is not None:
            assert (b.ts.cpu().numpy() == SENTINEL).all(), kw

    refused(EXCEED_HANDLE_CAPACITY, order=52)
    refused(EXCEED_HANDLE_CAPACITY, max_window=65536)
    refused(INVALID_ARGUMENT, max_window=0)
    refused(INVALID_ARGUMENT, max_cands=0)
    for name in ("pcm", "groups", "cands", "ts", "out"):
        refused(INVALID_ARGUMENT, **{name: None})
    # no groups: success, nothing written
    b.fresh()
    b.ng = 0
    assert b.search_far(limit16(0)) == 0 and (b.left() == SENTINEL).all()
