"""GPU tests of the encoder's option "long_tile_search" (run with -m gpu on an MI355X): with max_num_block_samples above
16384 and the option at 1 the partition search takes 64-tile sums (sla_hip_launch_search_far) and reruns the groups at or over
the exactness limit as far chains (sla_hip_launch_lpc_far_rerun).  The ten cases of tests/longenccases.py and the two 24-bit
ones of tests/longsearchcases.py must give the oracle's bytes and trace; sla_hip_last_counters reports the tile sums ([2] == 1)
and the number of groups rerun ([0]), which the integer model of tests/longsearchmodel.py predicts (tests/test_long_search_model.py
asserts its split on the CPU: none of the 16-bit groups, all of the loud 24-bit ones, the loud super-frame of the mixed file).
Orders above 51 keep the far chains; ordinary parameters do not consult the option.  Every comparison is exact equality."""
import numpy as np
import pytest

import longenccases as E
import longsearchcases as Q
import longsearchmodel as M
import slalibs as S
import waveforms as W
import test_gpu_long_enc as LE

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 2


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
    e.set_option("long_tile_search", 1)
    yield e
    e.close()


def case(name):
    return E.by_name()[name] if name in E.NAMES else Q.by_name()[name]


@pytest.mark.parametrize("name", E.NAMES + Q.NAMES)
def test_encode_whole_bytes_trace_and_reports(hip, enc, name):
    c = case(name)
    LE.setup(hip, enc, c)
    got = enc.encode_whole(c.pcm)
    assert got == c.data
    LE.same_trace(enc.trace(), c.trace)
    over, groups = M.flagged(c.pcm, c.max_block, c.ms)
    if c.bits == 16 or name == "stereo24_ms_quiet_70000_max65535":
        assert over == 0
    elif name in E.NAMES:
        assert over == groups > 0
    else:
        assert over == 2 and groups == 4
    cnt = enc.last_counters()
    assert cnt[2] == 1 and cnt[0] == over
    # everything else as the long route reports it
    assert cnt[3] == 0 and enc.last_expand()[:2] == (0, 1)
    assert enc.last_block_cert() == (0, 0) and enc.last_ltm_cert() == (0, 0, 0, 0, 0)
    assert enc.last_search_early()[0] == 0 and enc.last_silence()[0] in (0, 2)
    assert enc.last_timing()[1] > 0.0                       # the time is the search stage's


def test_exact_bits_1_reruns_every_group(hip):
    c = case("stereo16_ms_140000_max65535")
    e = hip.Encoder(*E.CAP, long_blocks=True)
    e.set_option("long_tile_search", 1)
    e.set_option("exact_bits", 1)
    LE.setup(hip, e, c)
    assert e.encode_whole(c.pcm) == c.data
    over, groups = M.flagged(c.pcm, c.max_block, c.ms, exact_bits=1)
    assert over == groups == 6
    assert e.last_counters()[0] == 6 and e.last_counters()[2] == 1
    e.close()


def test_analyze_device_and_both_packs(hip, enc):
    import torch
    c = case("stereo24_quiet_then_loud_85535_max65535")
    LE.setup(hip, enc, c)
    d = torch.from_numpy(c.pcm).cuda()
    torch.cuda.synchronize()
    enc.analyze_device(d.data_ptr(), c.num_samples, c.num_samples)
    assert enc.last_counters()[2] == 1 and enc.last_counters()[0] == 2
    cap = 8 * c.num_channels * c.num_samples + 65536
    assert enc.pack(cap, on_device=True) == c.data
    assert enc.pack(cap, on_device=False) == c.data


def test_encode_batch(hip, oracle, enc):
    a = case("stereo16_ms_70000_max32768")
    LE.setup(hip, enc, a)
    small = E.ordinary_pcm()
    ret, want = oracle.encode_whole(a.params(), small)
    assert ret == 0
    got = enc.encode_batch([a.pcm, small])
    assert [rc for rc, _ in got] == [0, 0]
    assert got[0][1] == a.data and got[1][1] == want
    assert enc.last_counters()[2] == 1 and enc.last_counters()[0] == 0


def test_order_64_keeps_the_far_chains(hip):
    """above 51 the tile kernels have no instantiation: the same route and the same bytes with the option on and off"""
    pcm = W.music_like(1, 20000, 16, seed=90)
    out = []
    for opt in (0, 1):
        e = hip.Encoder(*E.CAP, long_blocks=True)
        e.set_option("long_tile_search", opt)
        e.set_wave_format(1, 16, 48000)
        e.set_encode_parameter(64, 1, 8, hip.CH_NONE, hip.WINDOW_SIN, 65535)
        out.append(e.encode_whole(pcm))
        cnt = e.last_counters()
        assert cnt[2] == 0 and cnt[0] == 0
        e.close()
    assert out[0] == out[1] and len(out[0]) > 0


def reports(e):
    return (e.last_counters(), e.last_expand()[:2], e.last_block_cert(), e.last_ltm_cert(), e.last_search_early()[0], e.last_silence(),
            e.last_cert_audit())


def test_ordinary_parameters_do_not_consult_the_option(hip, oracle):
    pcm = W.music_like(2, 50000, 24, seed=80)
    ret, want = oracle.encode_whole(S.make_params(2, 24, 48000, 16, 3, 8, 1, 1, 4096, cap=E.CAP), pcm)
    assert ret == 0
    seen = []
    for opt in (0, 1):
        e = hip.Encoder(*E.CAP, long_blocks=True)
        e.set_option("long_tile_search", opt)
        e.set_wave_format(2, 24, 48000)
        e.set_encode_parameter(16, 3, 8, hip.CH_STEREO_MS, hip.WINDOW_SIN, 4096)
        assert e.encode_whole(pcm) == want
        seen.append(reports(e))
        e.close()
    assert seen[0] == seen[1]
    assert seen[0][0][2] == 1 and seen[0][0][3] == 1       # the ordinary route: tile sums of 16, device plan


def test_the_option_takes_0_and_1_only(hip, enc):
    for bad in (2, -1, 0.5):
        with pytest.raises(hip.SlaError) as ei:
            enc.set_option("long_tile_search", bad)
        assert ei.value.code == INVALID_ARGUMENT
    enc.set_option("long_tile_search", 0)
    enc.set_option("long_tile_search", 1)
