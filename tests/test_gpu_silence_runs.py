"""Option "silence_runs": input with silence is encoded without the prepass mask ever reaching the host -- the device lists
the zero runs that can matter (sla_hip_launch_zero_runs), the super-frame hop and the block types are decided from that list.
Bytes against the oracle, as in tests/test_gpu_expand.py; every case also asserts the route (Encoder.last_silence(): 1 = run
list, no mask bytes beyond the fixed tail words).

Reference: the hop over silence, src/SLAEncoder.c:392-408, 846-869; the block lengths a partition may choose,
src/SLAPredictor.c:1623-1630."""
import numpy as np
import pytest

import slalibs as S
import waveforms as W

pytestmark = pytest.mark.gpu

CAPACITY = 1024


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _encoder(hip, p, **options):
    enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    options.setdefault("stream", 0)
    options.setdefault("silence_runs", CAPACITY)
    for k, v in options.items():
        enc.set_option(k, v)
    enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
    enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method, p.window_type, p.max_block_samples)
    return enc


def _loud(nch, n, bits, seed):
    """music without a single all-zero sample: every zero of a case is one the case put there"""
    pcm = W.music_like(nch, n, bits, seed=seed)
    quiet = ~(pcm != 0).any(axis=0)
    pcm[0, quiet] = 1 << (32 - bits)
    return pcm


def _lead_in(nch, bits, maxb, rng):
    pcm = _loud(nch, 60001, bits, 1)
    pcm[:, :3000] = 0
    return pcm


def _pauses(nch, bits, maxb, rng):
    pcm = _loud(nch, 80000, bits, 2)
    for at, ln in ((5001, 2047), (20003, 2048), (41007, 2049), (60011, 2047), (70001, 2049)):
        pcm[:, at:at + ln] = 0
    return pcm


def _inner_blocks(nch, bits, maxb, rng):
    """the construction of test_silent_blocks_inside_searched_superframes (tests/test_gpu_expand.py): zero runs that do not
    begin where a super-frame begins make all-zero blocks inside searched super-frames"""
    nsf = min(12, 98000 // maxb)
    n = maxb * nsf + int(rng.integers(1, maxb))
    pcm = _loud(nch, n, bits, 3)
    for k in range(nsf):
        lo, kind = k * maxb, k % 6
        if kind == 1:
            pcm[:, lo + maxb // 2:lo + maxb] = 0
        elif kind == 2:
            pcm[:, lo + 1024:lo + 1024 + 2048] = 0
        elif kind == 3:
            pcm[:, lo + 1:lo + maxb] = 0
        elif kind == 4:
            s0 = lo + int(rng.integers(1, maxb // 2))
            pcm[:, s0:lo + maxb + int(rng.integers(0, 3000))] = 0
    return pcm


def _last_77(nch, bits, maxb, rng):
    pcm = _loud(nch, maxb * 11 + 77, bits, 4)
    pcm[:, maxb * 11:] = 0
    return pcm


def _last_40(nch, bits, maxb, rng):
    """... and one that no all-zero mask word betrays at all: only the list's tail run does"""
    pcm = _loud(nch, maxb * 11 + 40, bits, 5)
    pcm[:, maxb * 11:] = 0
    return pcm


def _trailing_500(nch, bits, maxb, rng):
    pcm = _loud(nch, 50000, bits, 6)
    pcm[:, -500:] = 0
    return pcm


def _all_zero(nch, bits, maxb, rng):
    return np.zeros((nch, 40000), np.int32)


CASES = [
    # maker, nch, bits, order, ms, maxb
    (_lead_in, 2, 16, 16, 1, 4096),                # (mid/side)
    (_lead_in, 1, 24, 8, 0, 16384),
    (_pauses, 1, 16, 8, 0, 4096),
    (_pauses, 2, 24, 12, 0, 8192),
    (_inner_blocks, 2, 16, 12, 1, 4096),
    (_inner_blocks, 1, 16, 8, 0, 8192),
    (_last_77, 1, 16, 16, 0, 4096),
    (_last_40, 2, 16, 8, 1, 4096),
    (_trailing_500, 2, 16, 10, 0, 4096),
    (_all_zero, 2, 16, 16, 1, 4096),
]


@pytest.mark.parametrize("maker,nch,bits,order,ms,maxb", CASES, ids=lambda v: v.__name__.strip("_") if callable(v) else str(v))
def test_single_files(oracle, hip, maker, nch, bits, order, ms, maxb):
    pcm = maker(nch, bits, maxb, np.random.default_rng(order + maxb))
    assert 40000 <= pcm.shape[1] <= 100000
    p = S.make_params(nch, bits, 48000, order, 1, 8, ms, 1, maxb)
    ret, want = oracle.encode_whole(p, pcm)
    assert ret == 0
    enc = _encoder(hip, p)
    try:
        got = enc.encode_whole(pcm)
        sil = enc.last_silence()
        assert got == want
        assert sil[0] == 1 and sil[1] >= 1 and sil[2] == CAPACITY and sil[3] == 0, sil
        # the same handle with the option off: the mask route, the same bytes
        enc.set_option("silence_runs", 0)
        assert enc.encode_whole(pcm) == want
        assert enc.last_silence()[1] == 0
        # host tables instead of the device's (plan_chunk alone numbers the blocks), several chunks
        enc.set_option("silence_runs", CAPACITY)
        enc.set_option("expand_silence", 0)
        enc.set_option("chunks", 3)
        assert enc.encode_whole(pcm) == want
        assert enc.last_silence()[0] == 1 and enc.last_silence()[3] == 0
    finally:
        enc.close()


def test_one_handle_silence_between_files_without(oracle, hip):
    """no silence, silence, no silence (twice) at one length: the bytes are right each time, the route is the list's only for
    the file with silence, and the kept search tables come back -- the file with silence drops them after serving as the
    guess, the next one rebuilds them, the one after reuses them (tests/test_gpu_expand.py::test_kept_search_tables)"""
    p = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096)
    enc = _encoder(hip, p)
    try:
        hits, routes = [], []
        for i, gap in enumerate([False, True, False, False]):
            pcm = _loud(2, 90000, 16, 40 + i)
            if gap:
                pcm[:, 30001:36000] = 0
            ret, want = oracle.encode_whole(p, pcm)
            assert ret == 0
            assert enc.encode_whole(pcm) == want
            hits.append(enc.last_expand()[2])
            routes.append(enc.last_silence()[0])
            assert enc.last_silence()[3] == 0
        assert routes == [0, 1, 0, 0]
        assert hits == [0, 1, 1, 2], hits
        assert enc.last_expand()[3] == 1                        # the guess "like the file before" was wrong once: at the silence
    finally:
        enc.close()


def test_overflow_takes_the_mask(oracle, hip):
    """three runs, a list of one: the count says so, the mask comes home as without the option, the bytes are the same"""
    p = S.make_params(1, 16, 48000, 8, 1, 8, 0, 1, 4096)
    pcm = _loud(1, 70000, 16, 8)
    for at in (3001, 30001, 55001):
        pcm[:, at:at + 2500] = 0
    ret, want = oracle.encode_whole(p, pcm)
    assert ret == 0
    enc = _encoder(hip, p, silence_runs=1)
    try:
        assert enc.encode_whole(pcm) == want
        sil = enc.last_silence()
        assert sil[0] == 2 and sil[1] == 3 and sil[2] == 1 and sil[3] > 0, sil
        enc.set_option("silence_runs", 3)
        assert enc.encode_whole(pcm) == want
        assert enc.last_silence() == (1, 3, 3, 0)
    finally:
        enc.close()


def test_with_verify(oracle, hip):
    p = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096)
    pcm = _pauses(2, 16, 4096, None)
    ret, want = oracle.encode_whole(p, pcm)
    assert ret == 0
    enc = _encoder(hip, p, verify=1)
    try:
        assert enc.encode_whole(pcm) == want
        assert enc.last_silence()[0] == 1 and enc.last_silence()[3] == 0
        ver = enc.last_verify()
        assert ver[0] > 0 and ver[1] == 0 and ver[3] > 0 and ver[4] == 0, ver
    finally:
        enc.close()


# ------------------------------------------------------------------ batches

def _clips(n_each, seed):
    """six clips, two with silence: a lead-in, and a zero tail behind a ragged end (the next clip starts in the gap's tile)"""
    lens = [n_each, n_each - 777, n_each + 4097, n_each // 2 + 13, n_each, n_each - 1]
    pcms = [_loud(2, n, 16, seed + i) for i, n in enumerate(lens)]
    pcms[1][:, :24000] = 0
    pcms[3][:, -3001:] = 0
    return pcms


def test_batch_of_six(oracle, hip):
    """sla_hip_encode_batch and sla_hip_encode_batch_device (one padded tensor): one clip with silence no longer brings every
    clip's mask home; bytes equal encode_whole of each clip and the oracle's"""
    import torch
    p = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096, cap=(2, 4096, 16, 1, 8))
    pcms = _clips(48000, 100)
    wants = []
    for pcm in pcms:
        ret, want = oracle.encode_whole(p, pcm)
        assert ret == 0
        wants.append(want)
    enc = _encoder(hip, p)
    try:
        got = enc.encode_batch(pcms)
        assert [rc for rc, _ in got] == [0] * 6
        assert [d for _, d in got] == wants
        sil = enc.last_silence()
        assert sil[0] == 1 and sil[1] >= 2 and sil[3] == 0, sil
        L = max(pcm.shape[1] for pcm in pcms) + 50
        x = torch.full((6, 2, L), 7 << 16, dtype=torch.int32)                   # padding that must not be read
        for b, pcm in enumerate(pcms):
            x[b, :, :pcm.shape[1]] = torch.from_numpy(pcm)
        got = enc.encode_batch_tensor(x.cuda(), lengths=[pcm.shape[1] for pcm in pcms])
        assert [rc for rc, _ in got] == [0] * 6
        assert [d for _, d in got] == wants
        sil = enc.last_silence()
        assert sil[0] == 1 and sil[1] >= 2 and sil[3] == 0, sil
        for pcm, want in zip(pcms, wants):
            assert enc.encode_whole(pcm) == want
        # a list of one entry: the batch's mask comes home as before
        enc.set_option("silence_runs", 1)
        got = enc.encode_batch(pcms)
        assert [d for _, d in got] == wants
        sil = enc.last_silence()
        assert sil[0] == 2 and sil[3] > 0, sil
        # no clip with silence: neither list nor mask
        enc.set_option("silence_runs", CAPACITY)
        clean = [pcms[0], pcms[2], pcms[4]]
        got = enc.encode_batch(clean)
        assert [d for _, d in got] == [wants[0], wants[2], wants[4]]
        assert enc.last_silence()[0] == 0 and enc.last_silence()[3] == 0
    finally:
        enc.close()


def test_batch_on_lanes(oracle, hip):
    """the smallest batch the worker lanes take (8 files, 16 Mi sample-channels), batch_lanes = 2: every lane runs its own
    prepass and list; the counters are summed into the caller's handle.  Bytes against encode_whole of each clip on a second
    handle without the option, and against the oracle for the two clips with silence and one without"""
    p = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096, cap=(2, 4096, 16, 1, 8))
    n = (16 << 20) // (2 * 8) + 1024
    pcms = [S.synth_pcm(2, n - 100 * i, 16, 48000, seed=500 + i) for i in range(8)]
    pcms[2][:, :24000] = 0
    pcms[6][:, -3001:] = 0
    assert len(pcms) >= 8 and sum(x.shape[1] for x in pcms) * 2 >= (16 << 20)
    enc = _encoder(hip, p, batch_lanes=2, stream=1)
    one = _encoder(hip, p, silence_runs=0)
    try:
        got = enc.encode_batch(pcms)
        assert [rc for rc, _ in got] == [0] * 8
        sil = enc.last_silence()
        assert sil[0] == 1 and sil[1] >= 2 and sil[3] == 0, sil
        for i, pcm in enumerate(pcms):
            assert got[i][1] == one.encode_whole(pcm), i
        for i in (2, 6, 7):
            ret, want = oracle.encode_whole(p, pcms[i])
            assert ret == 0 and got[i][1] == want, i
    finally:
        enc.close()
        one.close()
