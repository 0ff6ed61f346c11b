"""The launchers of the search beside the prepass (option "search_early", include/sla_hip.h), called directly with real work:
sla_hip_launch_prepass_early on a capped grid (max_workgroups: the waves of k_prepass walk on through the file) with
k_prepass_done behind it, and sla_hip_launch_search_exact_early / _plan_early / _expand_early, whose kernels read a cancel
flag at their start and, behind the stream wait, take the file's offset_lshift from a device word.

  B1  the capped prepass against tests/prepassmodel.py: OR word, zero-word count, mask, and the two early words
  B2  a cancelled chain writes nothing; the same buffers with the flag down give the plain launchers' results
  B3  the shift word is applied exactly: exact_limit x 4^L, int_shift + L
  B4  the real order on two streams, no preset words: a file with offset_lshift 3, and the same file with silence

Everything compared is exact: integers, bit patterns of doubles.  Every buffer carries sentinels behind (and, where a
cancelled kernel must not write, in) what the call may write.  No test waits on a word in memory."""
import ctypes as C

import numpy as np
import pytest

import planmodel as P
import prepassmodel as M
import sla_amd
import waveforms as W

pytestmark = pytest.mark.gpu

SENT32 = 0xDEADBEEF
SENT64 = 0xDEADBEEFCAFEF00D
SLOT_SENT = -7.25e100
INT32_MIN = -2 ** 31
NOT_LIVE = 0xFFFFFFFF
NO_WINDOW = 0xFFFFFFFF
XTILE, XTILES, NODES = 1024, 16, 17
MARGIN = 512                     # samples in front of and behind what the search reads: inside the allocation

vp, u32, u64, f64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double


class Group(C.Structure):                                       # sla_hip_lpc_group
    _fields_ = [("pcm_off", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


class Extra(C.Structure):                                       # sla_hip_launch_extra
    _fields_ = [("d_span", vp), ("d_group_count", vp), ("clear_ptr", vp * 3), ("clear_words", u32 * 3), ("d_rice_init", vp)]


@pytest.fixture(scope="module")
def L():
    import torch
    torch.cuda.init()
    lib = sla_amd.lib()
    lib.sla_hip_launch_prepass_early.argtypes = [vp, u64, u32, u32, u32, u32, vp, vp, vp, u32, vp]
    lib.sla_hip_launch_search_exact_early.argtypes = [vp, u64, u32, u32, vp, u32, u32, u32, vp, vp, vp, f64, f64, vp, vp, vp, vp, vp]
    lib.sla_hip_launch_plan_early.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.sla_hip_launch_expand_early.argtypes = [vp, u32, vp, vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, u32, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def done(L):
    """an event that is recorded and complete"""
    import torch
    ev = torch.cuda.Event()
    ev.record()
    torch.cuda.synchronize()
    assert ev.query()
    return ev


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(values):
    """device words from unsigned 32-bit values"""
    return _dev(np.array(values, np.uint32).view(np.int32))


def _filled(count, value=SENT32):
    return _words(np.full(count, value, np.uint32))


def _host(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _groups_dev(groups):
    import torch
    return torch.frombuffer(bytearray(b"".join(bytes(g) for g in groups)), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _same(got, want, what):
    for name in want:
        assert np.array_equal(got[name], want[name]), (what, name)


# ---- B1: the capped prepass ----------------------------------------------------------------------------------------------

SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 12289, 70001)     # 12289: four workgroups, the last wave of a
                                                                                 # capped grid starts in a partial round


def _positions(n):
    pos = {0, 63, 64, n - 1}
    for b in range(1024, n + 1, 1024):                          # both sides of every 1024 (and so every 4096) boundary
        pos |= {b - 1, b}
    return sorted(p for p in pos if 0 <= p < n)


def _dense(nch, n, bits, lshift, seed=0):
    """every sample of every channel an odd multiple of 2^(32 - bits + lshift): that bit set, nothing below it"""
    half = 1 << (bits - lshift - 1)                             # odd k in [-half, half)
    rng = np.random.default_rng(1000 * bits + 10 * lshift + nch + seed)
    k = (rng.integers(-half, half, (nch, n), dtype=np.int64) | 1) if half > 1 else np.full((nch, n), -1, np.int64)
    return (k << (32 - bits + lshift)).astype(np.int32)


def _planes(nch, n, bits, ms, variant):
    """int32 [nch, n].  "crafted": one sample per listed position, its kind cycling; "last": one sample at n - 1 only;
    "zero": nothing; ("dense", L): see _dense; "wide": dense(0) and one sample with a bit below the declared unit"""
    shift = 32 - bits
    if isinstance(variant, tuple):
        return _dense(nch, n, bits, variant[1])
    if variant == "wide":
        pcm = _dense(nch, n, bits, 0)
        pcm[nch - 1, n // 3] |= np.int32(1 << (n % shift))      # on a capped grid: in a round that is not its wave's last
        return pcm
    pcm = np.zeros((nch, n), np.int64)
    if variant == "last" and n:
        pcm[nch - 1, n - 1] = 1 << shift
    if variant == "crafted":
        kinds = ["one", "minus"] + (["below"] if shift else []) + (["l=-r", "l=1", "l=r=1", "l=r=-1"] if ms else [])
        kinds += ["l=r=min"] if ms and bits == 32 else []
        for i, p in enumerate(_positions(n)):
            kind = kinds[i % len(kinds)]
            ch = nch - 1 if i % 3 else i % nch                  # mostly the last channel only (the generic path's last read)
            if kind == "one":
                pcm[ch, p] = 1 << shift
            elif kind == "minus":
                pcm[ch, p] = -1 << shift
            elif kind == "below":                               # only bits below the shift: the OR word sees them, the mask not
                pcm[ch, p] = (1 << shift) - 1 if i % 2 else 1
            elif kind == "l=-r":
                pcm[0, p], pcm[1, p] = 3 << shift, -3 << shift
            elif kind == "l=1":
                pcm[0, p] = 1 << shift
            elif kind == "l=r=1":
                pcm[0, p] = pcm[1, p] = 1 << shift
            elif kind == "l=r=-1":
                pcm[0, p] = pcm[1, p] = -1 << shift
            elif kind == "l=r=min":                             # mid and side both wrap to zero: silent, as the oracle has it
                pcm[0, p] = pcm[1, p] = INT32_MIN
    return pcm.astype(np.int32)


def _groups_needed(n):
    return ((n + 63) // 64 + 63) // 64                          # workgroups of four waves of 16 mask words


def _caps(n):
    """max_workgroups: 0 (no limit) and what lies around the number the file needs"""
    nb = _groups_needed(n)
    out = [0]
    for v in (1, 2, 3, 5, nb - 1, nb, nb + 1):
        if v >= 1 and v not in out:
            out.append(v)
    return out


def _upload(pcm):
    nch, n = pcm.shape
    stride = n + 37
    planes = np.full((nch, stride), 0x7FFFFFFF, np.int32)       # poison behind every plane
    planes[:, n::2] = -1
    planes[:, :n] = pcm
    return _dev(planes), stride


def _run_prepass(L, d_pcm, stride, pcm, bits, ms, cap, want, flag=0):
    """one sla_hip_launch_prepass_early; want = the model's (or, mask, zero words).  Returns the two early words."""
    nch, n = pcm.shape
    nwords = (n + 63) // 64
    mask_len = (nwords + 15) // 16 * 16 + 16
    d_or = _filled(4)
    d_nz = _dev(np.full(mask_len, SENT64, np.uint64).view(np.int64))
    d_early = _words([flag, SENT32, SENT32, SENT32])
    _sync()
    rc = L.sla_hip_launch_prepass_early(_p(d_pcm), stride, nch, n, bits, ms, _p(d_or), _p(d_nz), _p(d_early), cap, None)
    assert rc == 0
    _sync()
    orw, nz, early = _host(d_or), _host(d_nz), _host(d_early)
    want_or, want_mask, want_zero = want
    where = (nch, n, bits, ms, cap)
    assert orw.tolist() == [want_or, want_zero, SENT32, SENT32], where
    assert np.array_equal(nz[:nwords], want_mask), where
    assert (nz[nwords:] == SENT64).all(), where                  # nothing behind ceil(n / 64) words
    assert early[2:].tolist() == [SENT32, SENT32], where
    return int(early[0]), int(early[1])


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
@pytest.mark.parametrize("nch,ms", [(1, 0), (2, 0), (2, 1), (3, 0), (8, 0)])
def test_capped_prepass(L, nch, ms, bits):
    variants = ["crafted", "last", "zero"] + [("dense", s) for s in (0, 1, 3, bits - 1)] + (["wide"] if bits < 32 else [])
    capped = capped_with_zero_words = 0
    for n in SIZES:
        for variant in variants:
            if variant == "wide" and n == 0:
                continue                                        # (no sample to widen)
            pcm = _planes(nch, n, bits, ms, variant)
            want = M.prepass(pcm, bits, ms)[:3]
            done = M.prepass_done(want[0], want[2], bits)
            if isinstance(variant, tuple) and n:
                # dense material: no zero word, the flag stays down, the shift is the file's.  The one exception is arithmetic,
                # not the kernels': bit 31 alone is INT32_MIN, and at 32 bits with mid/side L = R = INT32_MIN wraps to silence
                if ms and bits == 32 and variant[1] == 31:
                    assert done == (1, 31)
                else:
                    assert want[2] == 0 and done == (0, variant[1]), (variant, n)
            if variant == "wide":
                assert want[2] == 0 and done == (1, 0)
            d_pcm, stride = _upload(pcm)
            for cap in _caps(n):
                got = _run_prepass(L, d_pcm, stride, pcm, bits, ms, cap, want)
                assert got == done, (nch, n, bits, ms, variant, cap, got, done)
                if cap and cap < _groups_needed(n):
                    capped += 1
                    capped_with_zero_words += 1 if want[2] else 0
    # the capped calls are the point: waves that walk on, and carry zero words across their rounds
    assert capped > 0 and capped_with_zero_words > 0, (capped, capped_with_zero_words)
    # nothing here clears the flag: a raised one stays raised, the shift is stored all the same
    pcm = _planes(nch, 12289, bits, ms, ("dense", 0))
    want = M.prepass(pcm, bits, ms)[:3]
    d_pcm, stride = _upload(pcm)
    assert _run_prepass(L, d_pcm, stride, pcm, bits, ms, 1, want, flag=1) == (1, 0)


# ---- the three launchers behind the prepass, each as a job: fixed inputs, fresh output buffers per run ---------------------

class SearchJob:
    def __init__(self, planes, ms, order, cases, cands_of, max_cands, int_shift):
        """planes: int32 [channels, MARGIN + .. + MARGIN]; cases: (first sample, samples, channel) per group; cands_of(samples) ->
        [(start, len)], one table per distinct length"""
        self.ms, self.order, self.max_cands = ms, order, max_cands
        self.d_pcm, self.stride = _dev(planes), planes.shape[1]
        table, first, groups, slots = [], {}, [], 0
        for off, n, ch in cases:
            if n not in first:
                first[n] = len(table)
                table += cands_of(n)
            nc = len(cands_of(n))
            groups.append(Group(off, n, ch, NO_WINDOW, int_shift, first[n], nc, slots, 0))
            slots += nc
        self.groups, self.num_groups, self.slots = groups, len(groups), slots
        self.max_window = max(n for _, n, _ in cases)
        self.d_groups, self.d_cands = _groups_dev(groups), _dev(np.array(table, np.uint32))
        self.lags = 0

    def buffers(self, L):
        import torch
        self.lags = L.sla_hip_search_exact_lags(self.order)
        assert self.lags
        return {"tile_sums": torch.full((self.num_groups * XTILES * 2 * self.lags + 8,), SLOT_SENT, dtype=torch.float64, device="cuda"),
                "out": torch.full((self.slots * (self.order + 2) + 8,), SLOT_SENT, dtype=torch.float64, device="cuda"),
                "any_exact": _filled(4), "cleared": _filled(8)}

    def _args(self, b, limit, cert, stream):
        extra = Extra()
        extra.clear_ptr[0], extra.clear_words[0] = b["cleared"].data_ptr(), 5
        return [_p(self.d_pcm, 4 * MARGIN), u64(self.stride), self.ms, self.order, _p(self.d_groups), self.num_groups, self.max_window,
                self.max_cands, _p(self.d_cands), _p(b["tile_sums"]), _p(b["out"]), f64(limit), f64(cert), _p(b["any_exact"]),
                vp(stream), C.byref(extra)], extra

    def plain(self, L, b, limit, cert, stream=None):
        args, extra = self._args(b, limit, cert, stream)
        assert L.sla_hip_launch_search_exact_x(*args) == 0

    def early(self, L, b, limit, cert, d_early, event, stream=None):
        args, extra = self._args(b, limit, cert, stream)
        args[-1] = C.cast(C.pointer(extra), vp)
        assert L.sla_hip_launch_search_exact_early(*args, _p(d_early), vp(event.cuda_event)) == 0


class PlanJob:
    def __init__(self, nch, order, bps, d_groups, d_cands, num_sf, d_lpc=None):
        self.nch, self.order, self.bps, self.d_groups, self.d_cands, self.num_sf, self.d_lpc = nch, order, bps, d_groups, d_cands, num_sf, d_lpc

    def buffers(self, lpc=None):
        """lpc: the candidates' slots (host doubles) where the job does not run behind a search"""
        b = {"parts": _filled(self.num_sf * NODES + 8), "num_parts": _filled(self.num_sf + 8), "status": _filled(self.num_sf + 8)}
        if lpc is not None:
            b["out"] = _dev(lpc)
        return b

    def _args(self, b, stream):
        return [_p(self.d_groups), self.num_sf, self.nch, self.order, self.bps, _p(self.d_cands), _p(b["out"]), _p(b["parts"]),
                _p(b["num_parts"]), _p(b["status"]), vp(stream)]

    def plain(self, L, b, stream=None):
        assert L.sla_hip_launch_plan(*self._args(b, stream)) == 0

    def early(self, L, b, d_early, stream=None):
        assert L.sla_hip_launch_plan_early(*self._args(b, stream), _p(d_early)) == 0


class ExpandJob:
    SEQUENCE = 0x51A7E

    def __init__(self, frames, nch, win_len, win_off, capacity):
        """frames: (start, window, live row or NOT_LIVE)"""
        self.nch, self.capacity, self.num_sf, self.num_win = nch, capacity, len(frames), len(win_len)
        self.d_frames = _words([w for s, n, live in frames for w in (s, n, live, 0)])
        self.d_win_len, self.d_win_off = _words(win_len), _words(win_off)

    def buffers(self):
        g = self.capacity + 4
        return {"run": _words([0, 0, 0, 0] + [SENT32] * 4), "prefix": _filled(2 * self.num_sf + 8), "groups": _filled(10 * g),
                "cands": _filled(2 * g), "acf_jobs": _filled(4 * g), "counts": _filled(8)}

    def _args(self, b, plan, int_shift, d_mask, stream):
        return [_p(self.d_frames), self.num_sf, _p(plan["parts"]), _p(plan["num_parts"]), _p(plan["status"]), self.nch, int_shift,
                _p(self.d_win_len), _p(self.d_win_off), self.num_win, _p(b["run"]), _p(b["prefix"]), _p(b["groups"]), _p(b["cands"]),
                _p(b["acf_jobs"]), self.capacity, _p(b["counts"]), self.SEQUENCE, _p(d_mask), vp(stream)]

    def plain(self, L, b, plan, int_shift, d_mask, stream=None):
        assert L.sla_hip_launch_expand_masked(*self._args(b, plan, int_shift, d_mask, stream)) == 0

    def early(self, L, b, plan, int_shift, d_mask, d_early, stream=None):
        assert L.sla_hip_launch_expand_early(*self._args(b, plan, int_shift, d_mask, stream), _p(d_early)) == 0


def _read(b):
    _sync()
    return {k: _host(t).copy() for k, t in b.items()}


# ---- B2 / B3: the search ---------------------------------------------------------------------------------------------------

LENGTHS = (35, 1025, 4096)
OFFSETS = (1, 4099)
PLANE16 = MARGIN + max(OFFSETS) + max(LENGTHS) + MARGIN


@pytest.fixture(scope="module")
def noise16():
    """two planes of 16-bit noise, left-justified in int32, never zero"""
    q = np.random.default_rng(7).integers(-32768, 32768, (2, PLANE16), dtype=np.int64)
    q[q == 0] = 1
    return (q << 16).astype(np.int32)


def _search16(noise16, order, ms):
    cases = [(off, n, ch) for n in LENGTHS for off in OFFSETS for ch in range(2 if ms else 1)]
    return SearchJob(noise16, ms, order, cases, lambda n: [(0, n)], 1, 16)


# (limit of offset_lshift 0, cert_safety): certificate + k_search_finish<., 2>; k_search_finish<., 1> + <., 2>; <., 0>.
# |x| < 1 in the search's unit (side: < 2): the 35-sample windows stay below 2^7, the others lie above it
FORMS = {"cert": (2.0 ** 7, 64.0), "flag": (2.0 ** 7, 0.0), "all_exact": (2.0 ** 23, 64.0)}


@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("order", [8, 16, 18, 20, 32, 48, 51])     # k_acf_tiles<3>; k_acf_tiles_lds<5, 17>, <5, 20>, <9, 36>, <9, 33>, <13, 49>, <13, 52>
def test_cancelled_search_writes_nothing(L, done, noise16, order, ms):
    job = _search16(noise16, order, ms)
    for form, (limit, cert) in FORMS.items():
        assert (limit >= 4 * job.max_window) == (form == "all_exact")
        b = job.buffers(L)
        before = _read(b)
        d_early = _words([1, 0, SENT32, SENT32])
        job.early(L, b, limit, cert, d_early, done)
        got = _read(b)
        what = (order, ms, form)
        _same(got, {k: before[k] for k in ("tile_sums", "out")}, what)
        # clear_words runs before the flag is read: the words it names are zero or as they were
        assert got["any_exact"][0] in (0, SENT32) and (got["any_exact"][1:] == SENT32).all(), what
        assert np.isin(got["cleared"][:5], (0, SENT32)).all() and (got["cleared"][5:] == SENT32).all(), what
        assert _host(d_early).tolist() == [1, 0, SENT32, SENT32]
        # the same buffers, the flag down: what the plain launcher leaves in fresh ones
        d_early = _words([0, 0, SENT32, SENT32])
        job.early(L, b, limit, cert, d_early, done)
        got = _read(b)
        fresh = job.buffers(L)
        job.plain(L, fresh, limit, cert)
        want = _read(fresh)
        _same(got, want, what)
        assert (want["cleared"][:5] == 0).all() and (want["cleared"][5:] == SENT32).all()
        out = want["out"].view(np.float64)[:job.slots * (order + 2)].reshape(job.slots, order + 2)
        assert not (out[:, 0].view(np.uint64) == np.float64(SLOT_SENT).view(np.uint64)).any(), what       # every slot was written
        small = np.array([g.num_samples == 35 for g in job.groups])
        if form == "flag":                                      # both kinds of groups: flagged above the limit, exact below
            assert np.isnan(out[~small, 0]).all() and not np.isnan(out[small, 0]).any(), what
        if form == "cert":                                      # a width in parcor[0] above the limit, 0 below
            assert (out[~small, 1] > 0).all() and (out[small, 1] == 0).all(), what
        if form == "all_exact":
            assert (out[:, 1] == 0).all() and not np.isnan(out[:, 0]).any(), what


GRADED_GROUPS, GRADED_WINDOW = 16, 4096


@pytest.fixture(scope="module")
def graded():
    """one plane of 24-bit noise, 16 windows of 4096 samples, each half as loud as the one before"""
    rng = np.random.default_rng(24)
    n = GRADED_GROUPS * GRADED_WINDOW
    plane = np.zeros((1, MARGIN + n + MARGIN), np.int64)
    for i in range(GRADED_GROUPS):
        amp = 1 << (23 - i)
        plane[0, MARGIN + i * GRADED_WINDOW:MARGIN + (i + 1) * GRADED_WINDOW] = rng.integers(-amp, amp, GRADED_WINDOW)
    plane[0, :MARGIN] = rng.integers(-2 ** 23, 2 ** 23, MARGIN)
    plane[0, -MARGIN:] = rng.integers(-2 ** 23, 2 ** 23, MARGIN)
    return (plane << 8).astype(np.int32)


@pytest.mark.parametrize("place", ["between", "under"])
@pytest.mark.parametrize("cert", [64.0, 0.0])
def test_search_scales_its_limit_by_the_shift_word(L, done, graded, cert, place):
    """sla_hip_launch_search_exact_early(limit X) with the shift word s against sla_hip_launch_search_exact_x(limit X * 4^s).
    X "between": some windows lie below X and some above, and every tested shift moves more of them below.  X "under": no
    window lies below X itself, so that only the scaled limit makes the certificate's kernel raise the word without which the
    kernel of the exact windows returns at once (with windows below X that kernel rewrites whatever a certificate with the
    unscaled limit had left in their slots: the unscaled certificate would not show)."""
    order = 32
    job = SearchJob(graded, 0, order, [(i * GRADED_WINDOW, GRADED_WINDOW, 0) for i in range(GRADED_GROUPS)], lambda n: [(0, n)], 1, 8)

    def slots(words):
        return words["out"].view(np.float64)[:job.slots * (order + 2)].reshape(job.slots, order + 2)

    b = job.buffers(L)
    job.plain(L, b, 2.0 ** 40, cert)                             # every window below the limit: r[0] of the whole window
    r0 = slots(_read(b))[:, 0]
    assert np.isfinite(r0).all() and (r0 > 0).all()
    order_r0 = np.sort(r0)
    # between the fourth and the fifth quietest window / half the quietest one
    x = float(np.sqrt(order_r0[3] * order_r0[4])) if place == "between" else float(order_r0[0]) / 2
    shifts = (0, 1, 3, 8)
    below = [int((r0 < x * 4.0 ** s).sum()) for s in shifts]
    assert (0 < below[0] < GRADED_GROUPS) if place == "between" else (below[0] == 0), below
    assert all(b1 > b0 for b0, b1 in zip(below, below[1:])) and below[-1] < GRADED_GROUPS, below
    assert x * 4.0 ** shifts[-1] < 4 * GRADED_WINDOW            # never the launch form of "every window is exact"
    plain_x = None
    for s, want_exact in zip(shifts, below):
        fresh = job.buffers(L)
        job.plain(L, fresh, x * 4.0 ** s, cert)
        want = _read(fresh)
        b = job.buffers(L)
        job.early(L, b, x, cert, _words([0, s, SENT32, SENT32]), done)
        got = _read(b)
        _same(got, want, (cert, place, s))
        exact = (slots(got)[:, 1] == 0) & ~np.isnan(slots(got)[:, 0])        # neither certified (a width) nor flagged
        assert int(exact.sum()) == want_exact, (cert, place, s, exact, below)
        assert int(got["any_exact"][0]) == (1 if want_exact else 0), (cert, place, s)
        if s == 0:
            plain_x = want
        else:                                                   # the limit matters on this material: without the scaling, other slots
            assert not np.array_equal(plain_x["out"], got["out"]), (cert, place, s)


# ---- B2 / B3: the plan -----------------------------------------------------------------------------------------------------

def _plan_of_table(t):
    """one table of the model as sla_hip_launch_plan's arguments, at non-zero slot_first / cand_first"""
    O2, nc = t.order + 2, len(t.cands)
    cands = [(7, 3)] * 3 + t.cands + [(7, 3)]
    groups = [Group(0, t.window, 0, NO_WINDOW, 32 - t.bps, 3, nc, 5, 0)]
    groups += [Group(0, 1024, ch, NO_WINDOW, 0, 0, 1, 0, 0) for ch in range(1, t.nch)]
    lpc = np.ascontiguousarray(np.concatenate([np.full((5, O2), SLOT_SENT), t.slots.reshape(t.nch * nc, O2), np.full((4, O2), SLOT_SENT)]))
    return PlanJob(t.nch, t.order, t.bps, _groups_dev(groups), _dev(np.array(cands, np.uint32)), 1), lpc


def test_cancelled_plan_writes_nothing_and_a_live_one_is_the_plain_plan(L):
    t = P.first_separated(11, 8192, 2, 32, 24)
    model = P.host_decide(t)
    assert model == P.hp_decide(t)
    job, lpc = _plan_of_table(t)
    b = job.buffers(lpc)
    before = _read(b)
    job.early(L, b, _words([1, 0]))
    _same(_read(b), before, "cancelled")
    fresh = job.buffers(lpc)
    job.plain(L, fresh)
    want = _read(fresh)
    assert want["status"][0] == 0 and want["parts"][:int(want["num_parts"][0])].tolist() == model      # the anchor: the model's partition
    assert (want["parts"][len(model):] == SENT32).all() and np.array_equal(want["out"], before["out"])
    for words in ([0, 0], [0, 5]):                              # the shift word is none of the plan's business
        job.early(L, b, _words(words))
        _same(_read(b), want, words)
        b = job.buffers(lpc)


# ---- B2 / B3: the block tables ----------------------------------------------------------------------------------------------

FRAMES = [(0, 4096, 0), (4096, 4096, 1), (8192, 4096, NOT_LIVE), (12288, 4096, 2)]
PARTITIONS = [[4096], [2048, 2048], [1024, 1024, 2048]]
WIN_LEN, WIN_OFF = [512, 2048, 4096, 1024], [7, 1000, 5000, 9000]       # (one length nobody asks for)
CHANNELS = 2


def _crafted_run():
    """three live super-frames with hand-written partitions and a SILENT one between them; the mask says the same"""
    parts = np.full(3 * NODES + 8, SENT32, np.uint32)
    for row, p in enumerate(PARTITIONS):
        parts[row * NODES:row * NODES + len(p)] = p
    plan = {"parts": _words(parts), "num_parts": _words([len(p) for p in PARTITIONS] + [SENT32] * 4), "status": _words([0, 0, 0] + [SENT32] * 4)}
    mask = np.full(16384 // 64, 2 ** 64 - 1, np.uint64)
    mask[8192 // 64:12288 // 64] = 0
    return ExpandJob(FRAMES, CHANNELS, WIN_LEN, WIN_OFF, 12), plan, _dev(mask.view(np.int64))


def _expected_tables(int_shift):
    """the header's words for the crafted run: 7 blocks, 12 groups; per (block, channel) d_groups, d_cands, d_acf_jobs"""
    groups, cands, jobs, block = [], [], [], 0
    for start, window, live in FRAMES:
        if live == NOT_LIVE:
            block += 1
            continue
        at = start
        for ln in PARTITIONS[live]:
            for ch in range(CHANNELS):
                g = len(groups)
                groups.append([at, 0, ln, ch, WIN_OFF[WIN_LEN.index(ln)], int_shift, g, 1, block * CHANNELS + ch, 0])
                cands.append([0, ln])
                jobs.append([at, 0, ln, ch])
            at += ln
            block += 1
    assert block == 7 and len(groups) == 12
    return np.array(groups, np.uint32), np.array(cands, np.uint32), np.array(jobs, np.uint32)


def _check_tables(got, int_shift, what):
    groups, cands, jobs = _expected_tables(int_shift)
    assert got["counts"].tolist() == [7, 12, 1, ExpandJob.SEQUENCE] + [SENT32] * 4, what
    assert np.array_equal(got["groups"][:120].reshape(12, 10), groups), what
    assert (got["groups"][:120].reshape(12, 10)[:, 5] == int_shift).all(), what
    assert np.array_equal(got["cands"][:24].reshape(12, 2), cands), what
    assert np.array_equal(got["acf_jobs"][:48].reshape(12, 4), jobs), what
    assert (got["groups"][120:] == SENT32).all() and (got["cands"][24:] == SENT32).all() and (got["acf_jobs"][48:] == SENT32).all(), what
    assert got["run"][:3].tolist() == [7, 12, 0] and (got["run"][4:] == SENT32).all() and (got["prefix"][8:] == SENT32).all(), what


def test_cancelled_expand_writes_nothing(L):
    job, plan, d_mask = _crafted_run()
    b = job.buffers()
    before = _read(b)
    job.early(L, b, plan, 8, d_mask, _words([1, 0]))
    _same(_read(b), before, "cancelled")                        # d_run, d_prefix, the three tables, all four count words
    job.early(L, b, plan, 8, d_mask, _words([0, 0]))
    got = _read(b)
    fresh = job.buffers()
    job.plain(L, fresh, plan, 8, d_mask)
    want = _read(fresh)
    _check_tables(want, 8, "plain")                             # the anchor: what the header says of the plain launcher
    _same(got, want, "live")


@pytest.mark.parametrize("int_shift,lshift", [(8, 0), (8, 3), (16, 15), (8, 23)])       # the last one reaches 31, the launcher's limit
def test_expand_adds_the_shift_word(L, int_shift, lshift):
    job, plan, d_mask = _crafted_run()
    b = job.buffers()
    job.early(L, b, plan, int_shift, d_mask, _words([0, lshift]))
    got = _read(b)
    fresh = job.buffers()
    job.plain(L, fresh, plan, int_shift + lshift, d_mask)
    want = _read(fresh)
    _check_tables(want, int_shift + lshift, "plain")
    _same(got, want, (int_shift, lshift))
    assert (got["groups"][:120].reshape(12, 10)[:, 5] == int_shift + lshift).all()


# ---- B4: the real order, two streams, no preset words -----------------------------------------------------------------------

FILE_N, FILE_BITS, FILE_ORDER, FILE_LSHIFT = 5 * 4096 + 1000, 24, 32, 3


def _file(silence):
    """dense(3) material that the planner can decide: music, every sample an odd multiple of 2^(32 - 24 + 3)"""
    unit = 32 - FILE_BITS + FILE_LSHIFT
    pcm = ((W.music_like(2, FILE_N, FILE_BITS, seed=41) >> unit) << unit) | np.int32(1 << unit)
    if silence:
        pcm[:, 6000:11000] = 0
    return pcm


@pytest.mark.parametrize("silence", [False, True])
def test_chain_on_two_streams(L, silence):
    import torch
    pcm = _file(silence)
    want_or, want_mask, want_zero, _ = M.prepass(pcm, FILE_BITS, 1)
    assert M.prepass_done(want_or, want_zero, FILE_BITS) == ((1, FILE_LSHIFT) if silence else (0, FILE_LSHIFT))
    rng = np.random.default_rng(4)
    planes = rng.integers(-2 ** 31, 2 ** 31, (2, MARGIN + FILE_N + MARGIN), dtype=np.int64).astype(np.int32)
    planes[:, MARGIN:MARGIN + FILE_N] = pcm
    frames = [(s, min(4096, FILE_N - s), i) for i, s in enumerate(range(0, FILE_N, 4096))]
    search = SearchJob(planes, 1, FILE_ORDER, [(s, n, ch) for s, n, _ in frames for ch in range(2)], P.full_lattice, 10, 32 - FILE_BITS)
    plan = PlanJob(2, FILE_ORDER, FILE_BITS, search.d_groups, search.d_cands, len(frames))
    lengths = [1024, 2048, 3072, 4096, 1000]
    expand = ExpandJob(frames, 2, lengths, [100 * i + 3 for i in range(len(lengths))], 2 * 4 * len(frames))
    limit0 = 2.0 ** (53 + 2 * ((32 - FILE_BITS) - 31 - 1))       # the encoder's exactness limit at offset_lshift 0, mid/side
    nwords = (FILE_N + 63) // 64

    # the plain launchers, one stream, the true shift
    sb, pb, eb = search.buffers(L), plan.buffers(), expand.buffers()
    pb["out"] = sb["out"]
    d_mask = _dev(np.concatenate([want_mask, np.zeros(16, np.uint64)]).view(np.int64))
    _sync()
    search.plain(L, sb, limit0 * 4.0 ** FILE_LSHIFT, 64.0)
    plan.plain(L, pb)
    expand.plain(L, eb, pb, 32 - FILE_BITS + FILE_LSHIFT, d_mask)
    want = {"search": _read(sb), "plan": _read(pb), "expand": _read(eb)}
    if not silence:                                             # a chain worth comparing: tables were written, with the file's shift
        assert want["expand"]["counts"][2] == 1 and want["expand"]["counts"][1] >= 2 * len(frames), want["expand"]["counts"]
        ngroups = int(want["expand"]["counts"][1])
        assert (want["expand"]["groups"][:10 * ngroups].reshape(ngroups, 10)[:, 5] == 32 - FILE_BITS + FILE_LSHIFT).all()

    # the prepass on stream A, capped to one workgroup; the chain on stream B behind an event
    sb, pb, eb = search.buffers(L), plan.buffers(), expand.buffers()
    pb["out"] = sb["out"]
    before = {"search": _read(sb), "plan": _read(pb), "expand": _read(eb)}
    d_or = _filled(4)
    d_nz = _dev(np.full(nwords + 16, SENT64, np.uint64).view(np.int64))
    d_early = _words([0, SENT32, SENT32, SENT32])
    a, bs, ev = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Event()
    _sync()
    assert _groups_needed(FILE_N) > 1
    rc = L.sla_hip_launch_prepass_early(_p(search.d_pcm, 4 * MARGIN), search.stride, 2, FILE_N, FILE_BITS, 1, _p(d_or), _p(d_nz), _p(d_early), 1,
                                        a.cuda_stream)
    assert rc == 0
    ev.record(a)
    search.early(L, sb, limit0, 64.0, d_early, ev, bs.cuda_stream)
    plan.early(L, pb, d_early, bs.cuda_stream)
    expand.early(L, eb, pb, 32 - FILE_BITS, d_nz, d_early, bs.cuda_stream)
    got = {"search": _read(sb), "plan": _read(pb), "expand": _read(eb)}
    assert _host(d_or).tolist() == [want_or, want_zero, SENT32, SENT32]
    assert np.array_equal(_host(d_nz)[:nwords], want_mask) and (_host(d_nz)[nwords:] == SENT64).all()
    assert _host(d_early).tolist() == [int(silence), FILE_LSHIFT, SENT32, SENT32]
    if not silence:
        for stage in want:
            _same(got[stage], want[stage], stage)
    else:                                                       # behind the wait nothing ran; the tile sums race the flag by design
        _same(got["search"], {"out": before["search"]["out"]}, "search")
        _same(got["plan"], before["plan"], "plan")
        _same(got["expand"], before["expand"], "expand")
