"""The crafted-stream catalogue (tests/crafted_catalogue.py) through the HIP decoders (run with -m gpu on an MI355X).

These are legal .sla streams that the project's encoder never writes: extreme PARCOR codes and shifts, unstable
lattices, full-scale and even long-term taps, pitch >= 256, Rice parameters whose `<< 8` wraps, Golomb moduli that
are not powers of two, gamma escapes, tiles of more than 64 bits per sample (the bit reader's far path), 4 / 12 / 20 /
32-bit formats and 33-bit RAW side channels.  tests/test_crafted_streams.py pins the oracle's decoder to the reference
on every one of them and checks that the catalogue reaches each of those branches.  Here every case must come out of
  * SLADecoder_DecodeWhole, with the CRC check on and off,
  * Decoder.decode_batch, all cases in one call between clean encoder-written files, and
  * the streaming decoder fed in small fragments
exactly as from the oracle's decoder: result code, sample count, samples.  Nothing here reads the reference."""
import numpy as np
import pytest

import crafted_catalogue as CC
import slalibs as S
import slastream as SS
import waveforms as W

pytestmark = pytest.mark.gpu

CASES = CC.catalogue()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


@pytest.fixture(scope="module")
def decoders(hip):
    on, off = hip.Decoder(*CC.CAP, enable_crc_check=1), hip.Decoder(*CC.CAP, enable_crc_check=0)
    yield on, off
    on.close()
    off.close()


def oracle_decode(oracle, data, capacity):
    return oracle.decode_whole(S.make_params(cap=CC.CAP), data, capacity)


def same(got, want):
    rg, g = got
    ro, w = want[0], want[1]
    return rg == ro and g.shape[1] == w.shape[1] and np.array_equal(g[:w.shape[0]], w[:g.shape[0]])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decode_whole(oracle, decoders, case):
    want = oracle_decode(oracle, case.data, case.num_samples)
    assert want[0] == 0
    for crc, dec in zip((1, 0), decoders):
        got = dec.decode_whole(case.data, case.num_samples)
        assert same(got, want), (case.name, "crc", crc, got[0], int(np.argmax((got[1] != want[1]).any(axis=0))) if got[1].shape == want[1].shape else got[1].shape)


def test_decode_batch_with_clean_files_between(oracle, hip):
    """all cases in one call, each between two encoder-written files, so that passes mix crafted and clean blocks"""
    clean = []
    for i, (nch, bits) in enumerate([(2, 16), (1, 24), (8, 16), (2, 32)]):
        pcm = W.music_like(nch, 9000 + 777 * i, min(bits, 24), seed=40 + i)
        p = S.make_params(nch, min(bits, 24), 48000, 16, 3, 8, 1 if nch == 2 else 0, 1, 4096)
        ret, data = oracle.encode_whole(p, pcm)
        assert ret == 0
        clean.append(data)
    datas = []
    for i, c in enumerate(CASES):
        datas += [clean[i % len(clean)], c.data]
    datas.append(clean[0])
    for crc in (1, 0):
        dec = hip.Decoder(*CC.CAP, enable_crc_check=crc)
        try:
            got = dec.decode_batch(datas)
        finally:
            dec.close()
        for i, (data, g) in enumerate(zip(datas, got)):
            nsmp = int.from_bytes(data[15:19], "big")
            want = oracle_decode(oracle, data, nsmp)
            assert want[0] == 0
            assert same(g, want), ("item", i, "crc", crc, g[0])


@pytest.mark.parametrize("chunk", [97, 1000])
def test_streaming_decoder_in_fragments(oracle, hip, chunk):
    """every case in 1000-byte fragments; the cases below 20 kB also in 97-byte ones (blocks split across many calls)"""
    for case in CASES:
        if chunk < 1000 and len(case.data) > 20000:
            continue
        want = oracle_decode(oracle, case.data, case.num_samples)
        rc, got, _ = hip.streaming_decode(case.data, feed=lambda i: chunk, max_bit_per_sample=32, capacity=CC.CAP)
        assert rc == want[0] == 0, (case.name, rc)
        assert np.array_equal(got, want[1]), case.name


def test_lms_orders_off_the_list_are_refused_like_the_oracle(oracle, decoders):
    """header LMS orders other than 4 / 8 / 16 / 32: FAILED_TO_SYNTHESIZE, as from the oracle (tests/test_crafted_streams.py
    says why the reference is not followed there)"""
    rng = np.random.default_rng(5)
    for lms in (1, 2, 3, 6, 12, 24):
        f = SS.Format(1, 16, order=4, ntaps=1, lms=lms)
        data, _, _ = SS.write_file(f, [CC._comp(rng, f, 3000, bits=8, full=False)])
        want = oracle_decode(oracle, data, 3000)
        assert want[0] == 8
        for dec in decoders:
            assert same(dec.decode_whole(data, 3000), want), lms


# (case, blocks the call must hold at least): a one-channel case also with three blocks per wave
WAVE_SHARING = [("rice_over_64_bits_per_sample_1ch", 1025), ("rice_gamma_boundary_and_int32_extremes", 1025),
                ("rice_gamma_boundary_and_int32_extremes", 2049), ("lengths_lms4", 1025), ("lengths_lms4", 2049),
                ("format_32bit_ms_raw_33bit_side", 1025), ("format_8_channels", 1025)]


@pytest.mark.parametrize("name,blocks", WAVE_SHARING, ids=["%s-%d" % w for w in WAVE_SHARING])
def test_decode_batch_with_several_blocks_per_wave(oracle, hip, decoders, name, blocks):
    """the whole decoder where k_dec_bits gives a wave two or three blocks: one crafted file so many times in one call
    that its pass holds more than 1024 (2048) blocks.  One pass, so one k_dec_bits launch; every item must equal the
    oracle's decode of the file, with the CRC check on and off.
    (What this can see is limited: a block whose reader does not end where its size field says sends its file to the
    single-file path, one block per wave, which then decodes it correctly.  A k_dec_bits fault that moves used_bytes is
    therefore invisible from here; tests/test_gpu_dec_bits_lanes.py calls the launcher itself and sees it.)"""
    case = CC.by_name()[name]
    reps = -(-blocks // len(case.blocks))
    total = reps * len(case.blocks)
    assert total >= blocks
    lanes = hip.lib().sla_hip_dec_bits_lanes(total, case.fmt.num_channels)
    assert lanes >= 2 and (blocks < 2049 or lanes >= 3)
    want = oracle_decode(oracle, case.data, case.num_samples)
    assert want[0] == 0
    data = np.frombuffer(case.data, np.uint8)
    for crc, dec in zip((1, 0), decoders):
        got = dec.decode_batch([data] * reps)
        assert dec.last_timing()[5] == 1                       # all blocks went through one launch
        assert len(got) == reps
        bad = [i for i, g in enumerate(got) if not same(g, want)]
        assert not bad, (name, "crc", crc, "items", len(bad), "first", bad[0], got[bad[0]][0])
