"""GPU tests of the encoder with max_num_block_samples of 16385 to 65535 (run with -m gpu on an MI355X): every case of
tests/longenccases.py through the long-block routes (include/sla_hip.h, "Long blocks": the far-window LPC stage for the
search and the chosen blocks, host planner, exact long-term stage) must give the oracle's .sla bytes through each of the
four calls that take such parameters -- SLAEncoder_EncodeWhole, sla_hip_encode_batch, sla_hip_analyze_device + pack (host and
device), SLAEncoder_EncodeBlock -- and the oracle's trace; the bytes must decode to the PCM through the HIP decoder; every
other public encode route refuses such parameters before it launches anything and leaves the handle usable; a
capacity-65535 handle given ordinary parameters behaves as an ordinary handle.  Every comparison is exact equality.

The long-term stage of a capacity-65535 handle.  The reference sizes its FFT from the handle's capacity, and so does this
encoder; the certified long-term kernels (sla_hip_ltm_cert_supported) stop at 32768 points, so a handle of that capacity --
here as before long-block parameters existed -- takes the exact long-term route at EVERY parameter and sla_hip_last_ltm_cert
reports no certified job for it; the block stage's certificate does not depend on the capacity and is reported as taken."""
import numpy as np
import pytest

import longenccases as E
import slalibs as S
import slastream as SS
import waveforms as W
import wavmodel

pytestmark = pytest.mark.gpu

EXCEED_HANDLE_CAPACITY = 3
METHOD = lambda hip, ms: hip.CH_STEREO_MS if ms else hip.CH_NONE


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


@pytest.fixture(scope="module")
def enc(hip):
    e = hip.Encoder(*E.CAP, long_blocks=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dec(hip):
    d = hip.Decoder(*E.CAP, long_blocks=True)
    yield d
    d.close()


def setup(hip, e, c, max_block=None):
    e.set_wave_format(c.num_channels, c.bits, 48000)
    e.set_encode_parameter(c.order, c.ltm, c.lms, METHOD(hip, c.ms), hip.WINDOW_SIN, c.max_block if max_block is None else max_block)


def same_trace(tg, to):
    nb = to.num_blocks
    assert tg.num_blocks == nb and tg.offset_lshift == to.offset_lshift
    for f in ("blk_start", "blk_nsmpl", "blk_type", "blk_bytes"):
        assert np.array_equal(getattr(tg, f)[:nb], getattr(to, f)[:nb]), f
    comp = to.blk_type[:nb] == 0
    assert S.parcor_same(tg, to, nb, comp)
    for f in ("code", "kint", "rshift", "pitch", "rice_init"):
        assert np.array_equal(getattr(tg, f)[:nb][comp], getattr(to, f)[:nb][comp]), f
    used = (to.pitch[:nb] >= 3) & comp[:, None]
    assert np.array_equal(tg.ltm_coef[:nb][used], to.ltm_coef[:nb][used])
    for b in np.nonzero(comp)[0]:
        s, n = int(to.blk_start[b]), int(to.blk_nsmpl[b])
        assert np.array_equal(tg.res_final[:, s:s + n], to.res_final[:, s:s + n]), ("final", b)


# ------------------------------------------------------------------ the four calls

@pytest.mark.parametrize("name", E.NAMES)
def test_encode_whole_bytes_trace_routes_and_round_trip(hip, enc, dec, name):
    c = E.by_name()[name]
    setup(hip, enc, c)
    got = enc.encode_whole(c.pcm)
    assert got == c.data
    same_trace(enc.trace(), c.trace)
    # what ran: no tile sums, host plan, host tables, one chunk, no certificates, the mask, nothing beside the prepass
    cnt = enc.last_counters()
    assert cnt[0] == 0 and cnt[2] == 0 and cnt[3] == 0
    assert enc.last_expand()[:2] == (0, 1)
    assert enc.last_block_cert() == (0, 0) and enc.last_ltm_cert() == (0, 0, 0, 0, 0)
    assert enc.last_search_early()[0] == 0 and enc.last_silence()[0] in (0, 2)
    rc, back = dec.decode_whole(got, c.num_samples)
    assert rc == 0 and np.array_equal(back, c.pcm)


@pytest.mark.parametrize("name", E.NAMES)
def test_analyze_device_and_both_packs(hip, enc, name):
    import torch
    c = E.by_name()[name]
    setup(hip, enc, c)
    d = torch.from_numpy(c.pcm).cuda()
    torch.cuda.synchronize()
    enc.analyze_device(d.data_ptr(), c.num_samples, c.num_samples)
    cap = 8 * c.num_channels * c.num_samples + 65536
    assert enc.pack(cap, on_device=True) == c.data
    assert enc.pack(cap, on_device=False) == c.data


def test_encode_batch_of_long_block_files_and_an_ordinary_one(hip, oracle, enc):
    """two files with long blocks and a short one in one call: a batch shares its handle's parameters"""
    a = E.by_name()["stereo16_ms_140000_max65535"]
    setup(hip, enc, a)
    b_pcm = W.music_like(2, 70000, 16, seed=3)
    small = E.ordinary_pcm()
    want = [a.data]
    for pcm in (b_pcm, small):
        ret, data = oracle.encode_whole(a.params(), pcm)
        assert ret == 0
        want.append(data)
    assert SS.HEADER_SIZE < len(want[2]) and max(E_blocks(want[1])) == 65535
    got = enc.encode_batch([a.pcm, b_pcm, small])
    assert [rc for rc, _ in got] == [0, 0, 0]
    for i in range(3):
        assert got[i][1] == want[i], i


def E_blocks(data):
    import longblockcases as LB
    return LB.block_lengths(data)


@pytest.mark.parametrize("name", E.NAMES)
def test_encode_batch_of_one(hip, enc, name):
    c = E.by_name()[name]
    setup(hip, enc, c)
    got = enc.encode_batch([c.pcm])
    assert got[0][0] == 0 and got[0][1] == c.data


@pytest.mark.parametrize("name", ["mono24_order32_65535_max65535", "stereo24_16385_max16385"])
def test_encode_block(hip, enc, name):
    """one block of 65535 and one of 16385 samples: the block bytes of the oracle's one-block file"""
    c = E.by_name()[name]
    assert c.blocks() == [(c.num_samples, E.COMPRESS)] and c.trace.offset_lshift == 0
    setup(hip, enc, c)
    assert enc.encode_block(c.pcm) == c.data[SS.HEADER_SIZE:]


# ------------------------------------------------------------------ either / or: the routes that refuse

def refused(call):
    with pytest.raises(Exception) as ei:
        call()
    assert getattr(ei.value, "code", None) == EXCEED_HANDLE_CAPACITY, ei.value


def still_encodes_an_ordinary_file(hip, oracle, e):
    pcm = E.ordinary_pcm()
    e.set_wave_format(2, 16, 48000)
    e.set_encode_parameter(16, 3, 8, hip.CH_STEREO_MS, hip.WINDOW_SIN, 4096)
    ret, want = oracle.encode_whole(S.make_params(2, 16, 48000, 16, 3, 8, 1, 1, 4096, cap=E.CAP), pcm)
    assert ret == 0 and e.encode_whole(pcm) == want


ROUTES = ("batch_device", "batch_resident", "wav_batch", "wav_resident", "shard_analyze", "shard_analyze_no_silence",
          "analyze_batch_device", "pack_resident", "verify_last_image", "verify_whole", "verify_batch", "verify_block", "verify_analyze")


@pytest.mark.parametrize("route", ROUTES)
def test_routes_that_do_not_take_long_blocks_refuse_and_leave_the_handle_usable(hip, oracle, route):
    import torch
    pcm = W.music_like(2, 20000, 16, seed=70)
    e = hip.Encoder(*E.CAP, long_blocks=True)
    e.set_wave_format(2, 16, 48000)
    e.set_encode_parameter(16, 3, 8, hip.CH_STEREO_MS, hip.WINDOW_SIN, 20000)
    d = torch.from_numpy(pcm).cuda()
    out = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    wav = wavmodel.build_wav(pcm, 16, 48000)
    torch.cuda.synchronize()
    if route == "batch_device":
        refused(lambda: e.encode_batch_from([d], hip.PCM_S32_LEFT))
    elif route == "batch_resident":
        refused(lambda: e.encode_resident_from([d], hip.PCM_S32_LEFT, outs=[out]))
    elif route == "wav_batch":
        refused(lambda: e.encode_wav_batch([wav], capacities=[1 << 20]))
    elif route == "wav_resident":
        src = torch.from_numpy(np.frombuffer(wav, np.uint8).copy()).cuda()
        refused(lambda: e.encode_wav_resident([src], outs=[out]))
    elif route == "shard_analyze":
        refused(lambda: e.shard_analyze(d.data_ptr(), 20000, 20000, 0xFFFF0000))
    elif route == "shard_analyze_no_silence":
        refused(lambda: e.shard_analyze(d.data_ptr(), 20000, 20000, 0xFFFF0000, no_silence=True))
    elif route == "analyze_batch_device":
        refused(lambda: e.analyze_batch_device(d.data_ptr(), 20000, 20000, [0], [20000]))
    elif route == "pack_resident":
        e.analyze_device(d.data_ptr(), 20000, 20000)
        refused(lambda: e.pack_resident(out))
    elif route == "verify_last_image":
        e.encode_whole(pcm)                            # (leaves its image on the device)
        refused(lambda: e.verify_last_image(d.data_ptr(), 20000))
    else:
        e.set_option("verify", 1)
        if route == "verify_whole":
            refused(lambda: e.encode_whole(pcm))
        elif route == "verify_batch":
            refused(lambda: e.encode_batch([pcm]))
        elif route == "verify_block":
            refused(lambda: e.encode_block(pcm))
        else:
            refused(lambda: e.analyze_device(d.data_ptr(), 20000, 20000))
        e.set_option("verify", 0)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()
    still_encodes_an_ordinary_file(hip, oracle, e)
    e.close()


# ------------------------------------------------------------------ the same handle on ordinary parameters

@pytest.mark.parametrize("max_block", [4096, 16384])
def test_a_capacity_65535_handle_on_ordinary_parameters(hip, oracle, max_block):
    """after a long-block file on the same handle: ordinary parameters take the ordinary routes again -- the oracle's bytes for
    that capacity (the long-term FFT follows it), the same bytes as a capacity-16384 handle's oracle twin for this input, the
    certified block stage, device plan and device tables; the long-term report as the module's docstring says.  (A handle of
    its own: device-written block tables need the handle's list of window lengths to stay within 256 entries, and the module's
    shared handle has seen every length of every case by now.)"""
    enc = hip.Encoder(*E.CAP, long_blocks=True)
    c = E.by_name()["stereo24_16385_max16385"]
    setup(hip, enc, c)
    assert enc.encode_whole(c.pcm) == c.data
    pcm = W.music_like(2, 50000, 16, seed=80)
    twin = S.make_params(2, 16, 48000, 16, 3, 8, 1, 1, max_block, cap=E.CAP)
    small = S.make_params(2, 16, 48000, 16, 3, 8, 1, 1, max_block, cap=(8, 16384, 48, 5, 40))
    ret, want = oracle.encode_whole(twin, pcm)
    ret2, want2 = oracle.encode_whole(small, pcm)
    assert ret == 0 and ret2 == 0 and want[SS.HEADER_SIZE:] == want2[SS.HEADER_SIZE:]
    enc.set_wave_format(2, 16, 48000)
    enc.set_encode_parameter(16, 3, 8, hip.CH_STEREO_MS, hip.WINDOW_SIN, max_block)
    for _ in range(2):                                 # (the second file of a shape: kept tables, search beside the prepass)
        assert enc.encode_whole(pcm) == want
        cnt = enc.last_counters()
        assert cnt[2] == 1 and cnt[3] == 1             # tile sums, device plan
        assert enc.last_block_cert()[0] == 1
        assert enc.last_expand()[0] >= 1
        L = hip.lib()
        fft = 1
        while fft < 2 * E.CAP[1]:
            fft <<= 1
        jobs = enc.last_ltm_cert()[0]
        assert (jobs > 0) == bool(L.sla_hip_ltm_cert_supported(fft))
    assert enc.last_expand()[2] >= 1                   # served from kept tables
    enc.close()


# ------------------------------------------------------------------ the Python guard

def test_python_guard(hip):
    with pytest.raises(RuntimeError):
        hip.Encoder(max_num_block_samples=20000)
    for n in (16385, 65535):
        with pytest.raises(RuntimeError):
            hip.Encoder(8, n, 48, 5, 40)
    e = hip.Encoder(2, 20000, 16, 1, 8, long_blocks=True)
    e.set_wave_format(2, 16, 48000)
    with pytest.raises(hip.SlaError) as ei:
        e.set_encode_parameter(16, 1, 8, hip.CH_NONE, hip.WINDOW_SIN, 20001)       # above the handle's capacity
    assert ei.value.code == EXCEED_HANDLE_CAPACITY
    e.set_encode_parameter(16, 1, 8, hip.CH_NONE, hip.WINDOW_SIN, 20000)
    e.close()
