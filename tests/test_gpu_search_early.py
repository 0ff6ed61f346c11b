"""Search beside the prepass (option "search_early", include/sla_hip.h): a single file whose predecessor on the handle had no
silence starts its search chain while the prepass still runs; the chain takes offset_lshift from a device word, and a prepass
that finds silence (or an OR word of 0) cancels it on the device, after which the host launches the search again.

Every case: the packed image with the option on, the same with it off, and the oracle's encode, byte for byte -- and the
counters say which way the file went (sla_hip_last_search_early: started early, starts, cancelled starts).

Files of 5 x 4096 + 1000 samples (six super-frames, a ragged last one); the case of a silent last super-frame shorter than
127 samples needs a file that ends in one: 5 x 4096 + 100.  The prepass of such a file needs six workgroups: option
"early_prepass_groups" 1 and 2 both cap its grid (its waves walk on), and change neither a byte nor a counter.

Reference: offset_lshift src/SLAEncoder.c:425-455, the super-frame hop over silence src/SLAEncoder.c:846-869, 392-408."""
import numpy as np
import pytest

import slalibs as S
import waveforms as W

pytestmark = pytest.mark.gpu

N = 5 * 4096 + 1000
N_SHORT_TAIL = 5 * 4096 + 100

SHAPES = {
    # nch, bits, order, mid/side, max_block
    "stereo24": (2, 24, 32, 1, 4096),
    "mono16": (1, 16, 16, 0, 4096),
    "three16": (3, 16, 16, 0, 4096),                            # three channels: the prepass's generic channel path beside a search
}


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _params(shape):
    nch, bits, order, ms, maxb = SHAPES[shape]
    return S.make_params(nch, bits, 48000, order, 1, 8, ms, 1, maxb)


def _plain(shape, n, seed):
    """no silence, offset_lshift 0: every sample has the lowest bit of the file's unit set"""
    nch, bits = SHAPES[shape][:2]
    return W.music_like(nch, n, bits, seed=seed) | np.int32(1 << (32 - bits))


def _zero_words(pcm):
    """aligned 64-sample words in which every channel is zero (what the prepass counts; a partial last word counts too)"""
    any_nz = (pcm != 0).any(axis=0)
    pad = (-len(any_nz)) % 64
    return int((~np.pad(any_nz, (0, pad)).reshape(-1, 64).any(axis=1)).sum())


def _case(shape, name):
    """(the file, whether a search started beside its prepass has to be cancelled)"""
    nch, bits = SHAPES[shape][:2]
    n = N_SHORT_TAIL if name == "silent_short_tail" else N
    pcm = _plain(shape, n, seed=300 + len(name))
    if name == "plain":
        assert _zero_words(pcm) == 0
        return pcm, False
    if name == "zeros_at_start":
        pcm[:, :3000] = 0
        return pcm, True
    if name == "zeros_across_superframes":
        pcm[:, 4096 * 2 - 1500:4096 * 2 + 1700] = 0             # begins in super-frame 1, ends in super-frame 2
        return pcm, True
    if name == "silent_short_tail":
        pcm[:, 5 * 4096:] = 0                                   # the last super-frame: 100 samples, all zero
        assert _zero_words(pcm[:, :5 * 4096]) == 0              # ... and no all-zero word before it
        return pcm, True
    if name == "all_zero":
        pcm[:] = 0
        return pcm, True
    if name in LSHIFTS:
        unit = 32 - bits + LSHIFTS[name]
        pcm = ((pcm >> unit) << unit) | np.int32(1 << unit)     # (lshift3:) multiples of 8 in the file's unit, bit 3 always set
        assert _zero_words(pcm) == 0
        return pcm, False
    raise AssertionError(name)


def _encoder(hip, p, early, groups=0):
    enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    enc.set_option("stream", 0)
    enc.set_option("search_early", early)
    if groups:
        enc.set_option("early_prepass_groups", groups)
    enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
    enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method, p.window_type, p.max_block_samples)
    return enc


@pytest.fixture(scope="module")
def warm(oracle):
    """per (shape, length): a file without silence and the oracle's bytes for it -- what every handle encodes first, so that
    the file under test has a predecessor without silence"""
    made = {}

    def get(shape, n):
        if (shape, n) not in made:
            pcm = _plain(shape, n, seed=7)
            ret, want = oracle.encode_whole(_params(shape), pcm)
            assert ret == 0
            made[(shape, n)] = (pcm, want)
        return made[(shape, n)]
    return get


LSHIFTS = {"lshift1": 1, "lshift3": 3, "lshift8": 8}
CASES = ["plain", "zeros_at_start", "zeros_across_superframes", "silent_short_tail", "all_zero", "lshift3", "lshift1", "lshift8"]
# (shape, early_prepass_groups): every shape with the default cap, which no file here reaches; stereo24 also with caps that bind
RUNS = [pytest.param(shape, 0, id=shape) for shape in sorted(SHAPES)]
RUNS += [pytest.param("stereo24", g, id="stereo24-groups%d" % g) for g in (1, 2)]


@pytest.mark.parametrize("shape,groups", RUNS)
@pytest.mark.parametrize("name", CASES)
def test_early_search_gives_the_same_bytes(oracle, hip, warm, shape, groups, name):
    p = _params(shape)
    pcm, cancelled = _case(shape, name)
    ret, want = oracle.encode_whole(p, pcm)
    assert ret == 0                                             # the reference alone encodes the input
    first, first_want = warm(shape, pcm.shape[1])
    got = {}
    for early in (1, 0):
        enc = _encoder(hip, p, early, groups)
        try:
            assert enc.encode_whole(first) == first_want
            assert enc.last_search_early() == (0, 0, 0, 0)      # a fresh handle has no predecessor to go by
            got[early] = enc.encode_whole(pcm)
            assert enc.last_search_early() == ((1, 1, int(cancelled), 0) if early else (0, 0, 0, 0))
            # and the handle is fit for the next file, whichever way this one went
            assert enc.encode_whole(first) == first_want
            assert enc.last_search_early()[2] == (int(cancelled) if early else 0)
        finally:
            enc.close()
    assert got[1] == got[0]
    assert got[1] == want
    if name in LSHIFTS:
        assert got[1] != first_want and len(got[1]) < len(first_want)      # (lshift3: three bits per sample less to code)
        assert got[1][24] == LSHIFTS[name]                      # offset_lshift in the file header (tests/slastream.py)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_wide_samples_cancel_the_start_and_are_refused_as_ever(hip, warm, shape):
    """one sample with a bit below the declared unit set: the prepass beside the search finds the file wider than declared and
    calls the start off on the device; the handle answers with the result code it gives without the option, counts one start
    and one cancelled start, and encodes the next file as if nothing had happened"""
    nch, bits = SHAPES[shape][:2]
    p = _params(shape)
    pcm = _plain(shape, N, seed=311)
    pcm[nch - 1, N // 2] |= np.int32(1 << (32 - bits - 1))
    assert _zero_words(pcm) == 0
    first, first_want = warm(shape, N)
    codes = {}
    for early in (1, 0):
        enc = _encoder(hip, p, early)
        try:
            assert enc.encode_whole(first) == first_want
            assert enc.last_search_early() == (0, 0, 0, 0)
            with pytest.raises(hip.SlaError) as refused:
                enc.encode_whole(pcm)
            codes[early] = refused.value.code
            assert enc.last_search_early() == ((1, 1, 1, 0) if early else (0, 0, 0, 0))
            assert enc.encode_whole(first) == first_want
            assert enc.last_search_early()[2] == early
            assert enc.encode_whole(first) == first_want        # ... and so is the handle's next start beside a prepass
            assert enc.last_search_early() == ((1, 2, 1, 0) if early else (0, 0, 0, 0))
        finally:
            enc.close()
    assert codes[1] == codes[0] != 0


def test_one_handle_through_every_route(oracle, hip):
    """no silence (tables uploaded), no silence (early), silence (early, cancelled), no silence (not early: the last file had
    silence), no silence (early), another length (early on tables just uploaded), the first length again -- the bytes are the
    oracle's each time, the cancelled-start counter rises at the third file only, and the flag that cancelled it does not
    cancel a later one"""
    shape = "stereo24"
    p = _params(shape)
    plan = [(N, False, 0), (N, False, 1), (N, True, 1), (N, False, 0), (N, False, 1), (N + 4096 + 333, False, 1), (N, False, 1)]
    enc = _encoder(hip, p, 1)
    try:
        starts = 0
        for i, (n, gap, early) in enumerate(plan):
            pcm = _plain(shape, n, seed=50 + i)
            if gap:
                pcm[:, 6000:11000] = 0
            ret, want = oracle.encode_whole(p, pcm)
            assert ret == 0
            assert enc.encode_whole(pcm) == want, i
            starts += early
            assert enc.last_search_early() == (early, starts, 1 if i >= 2 else 0, 0), i
        assert enc.last_expand()[3] >= 1                        # (the cancelled start is a wrong guess like any other)
    finally:
        enc.close()
