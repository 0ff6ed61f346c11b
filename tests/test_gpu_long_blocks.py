"""Streams with blocks of more than 16384 samples through every route of the HIP decoder (run with -m gpu on an MI355X).

The files are those of tests/longblockcases.py: a crafted mono file [65535 compressed with long-term (1023, 5 taps), 2048 RAW,
40897 compressed with (1, 5 taps), 3000 SILENT, 16385 compressed], a crafted 24-bit mid/side stereo file [40000, 50000], a
crafted 8-channel file [20000], and two files from the oracle's encoder with blocks of 65535 and 32768 samples.  Through a
Decoder(8, 65535, 255, 5, 32, long_blocks=True) every route must give what the oracle gives (LB.expected; tests/test_long_blocks_model.py pins
that to the reference where the reference is defined): whole file with the CRC check on and off, batch between ordinary
files, device tensor, resident by the lane walk and by the wide walk, windows inside a long block / across its end / the whole
file, the block index and the windows decoded from it, salvage of clean and of damaged bytes, the streaming decoder in
1000-byte fragments, and WAV.  Nothing here reads the reference.
"""
import numpy as np
import pytest

import indexmodel as IM
import longblockcases as LB
import salvagemodel as SM

pytestmark = pytest.mark.gpu

CASES = LB.cases()
IDS = [c.name for c in CASES]
OK, EXCEED_HANDLE_CAPACITY, CORRUPT = 0, 3, 11


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


@pytest.fixture(scope="module")
def decoders(hip):
    on, off = hip.Decoder(*LB.CAP, enable_crc_check=1, long_blocks=True), hip.Decoder(*LB.CAP, enable_crc_check=0, long_blocks=True)
    yield on, off
    on.close()
    off.close()


def resident(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()


def first_bad(got, want):
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    bad = np.argwhere(got != want)
    return ("channel", int(bad[0][0]), "sample", int(bad[0][1]), "mismatches", len(bad)) if len(bad) else None


def windows_of(case):
    """(start, length): inside the first long block, across its end, across the file's end, the whole file"""
    lens = case.block_lengths
    k = next(i for i, n in enumerate(lens) if n > 16384)
    s0 = sum(lens[:k])
    return [(s0 + 1000, 3000), (s0 + lens[k] - 100, 300), (case.num_samples - 50, 200), (0, case.num_samples)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decode_whole(decoders, case):
    rc, want = LB.expected(case.name)
    assert rc == OK
    for crc, dec in zip((1, 0), decoders):
        got = dec.decode_whole(case.data, case.num_samples)
        assert got[0] == OK and got[1].shape[1] == case.num_samples, (case.name, "crc", crc, got[0], got[1].shape)
        assert np.array_equal(got[1], want), (case.name, "crc", crc, first_bad(got[1], want))


def test_decode_batch_between_ordinary_files(oracle, hip, decoders):
    import slalibs as S
    ordinary = LB.ordinary_files()
    datas = []
    for i, c in enumerate(CASES):
        datas += [ordinary[i % len(ordinary)], c.data]
    datas.append(ordinary[0])
    wants = []
    for i, d in enumerate(datas):
        if i % 2:
            wants.append(LB.expected(CASES[i // 2].name))
        else:
            rc, pcm, _ = oracle.decode_whole(S.make_params(cap=LB.CAP), d, int.from_bytes(d[15:19], "big"))
            wants.append((rc, pcm))
    for crc, dec in zip((1, 0), decoders):
        got = dec.decode_batch(datas)
        for i, (g, w) in enumerate(zip(got, wants)):
            assert g[0] == w[0] == OK and np.array_equal(g[1], w[1]), ("item", i, "crc", crc, g[0], first_bad(g[1], w[1]))


def check_padded(out, lens, codes, cases):
    """a padded [B][C][L] int32 tensor against the expected samples; rows and samples no file covers are zero"""
    host = out.cpu().numpy()
    assert codes == [OK] * len(cases) and lens == [c.num_samples for c in cases]
    for b, c in enumerate(cases):
        want = LB.expected(c.name)[1]
        assert np.array_equal(host[b, :c.num_channels, :c.num_samples], want), (c.name, first_bad(host[b, :c.num_channels, :c.num_samples], want))
        assert not host[b, c.num_channels:].any() and not host[b, :, c.num_samples:].any(), c.name


def test_decode_batch_tensor(decoders):
    import torch
    out, lens, codes = decoders[0].decode_batch_tensor([c.data for c in CASES], dtype=torch.int32)
    check_padded(out, lens, codes, CASES)


@pytest.mark.parametrize("walk", ["lane", "wide"])
def test_decode_resident_tensor(hip, walk):
    import torch
    srcs = [resident(c.data) for c in CASES]
    dec = hip.Decoder(*LB.CAP, long_blocks=True)
    try:
        if walk == "wide":
            dec.set_option("wide_walk", 1000)              # every file here is longer: all are walked by the whole device
        out, lens, codes = dec.decode_resident_tensor(srcs, dtype=torch.int32)
        wide, overflowed = dec.last_walk()[:2]
        assert (wide, overflowed) == ((len(CASES), 0) if walk == "wide" else (0, 0))
        check_padded(out, lens, codes, CASES)
    finally:
        dec.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_windows_index_and_indexed_windows(hip, decoders, case):
    import torch
    dec = decoders[0]
    src = resident(case.data)
    want = LB.expected(case.name)[1]
    model = IM.index_of(case.data)
    host_index = hip.Index.build(case.data)
    dev_index, = dec.index_resident([src])
    try:
        for x in (host_index, dev_index):
            rows = [(int(r["byte_off"]), int(r["byte_len"]), int(r["smp_off"]), int(r["num_samples"])) for r in x.blocks()]
            assert rows == model.rows and (x.stop, x.extent) == (model.stop, model.extent) == (OK, case.num_samples)
        assert host_index.to_bytes() == dev_index.to_bytes()
        for start, length in windows_of(case):
            n = min(length, case.num_samples - start)
            plan = IM.plan_window(model, start, length, LB.CAP[1])
            assert plan.stop == OK and plan.rows
            assert max(r[3] for r in plan.rows) > 16384 or start == case.num_samples - 50
            out, lens, codes = dec.decode_windows_tensor([src], [start], length, dtype=torch.int32)
            assert (codes, lens) == ([OK], [n]), (start, length, codes, lens)
            host = out.cpu().numpy()[0]
            assert np.array_equal(host[:, :n], want[:, start:start + n]), (start, length, first_bad(host[:, :n], want[:, start:start + n]))
            assert not host[:, n:].any()
            for x in (host_index, dev_index):
                out, outcomes = dec.decode_windows_indexed([src], [x], [start], length, dtype=torch.int32)
                torch.cuda.synchronize()
                assert [int(v) for v in outcomes.cpu().numpy()[0]] == [OK, n], (start, length)
                host = out.cpu().numpy()[0]
                assert np.array_equal(host[:, :n], want[:, start:start + n]), (start, length, first_bad(host[:, :n], want[:, start:start + n]))
                assert not host[:, n:].any()
    finally:
        host_index.close()
        dev_index.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_salvage_of_clean_bytes(decoders, case):
    import torch
    got, rep, ranges = decoders[0].salvage_resident_tensor(resident(case.data), dtype=torch.int32)
    want = LB.expected(case.name)[1]
    assert rep["result"] == OK and rep["mode"] == 1 and ranges == [] and rep["blocks_decoded"] == len(case.block_lengths)
    assert np.array_equal(got.cpu().numpy(), want), (case.name, first_bad(got.cpu().numpy(), want))


def test_salvage_with_a_byte_flipped_in_the_65535_sample_block(decoders):
    import torch
    case = LB.by_name()["mono_16bit_65535_2048raw_40897_3000silent_16385"]
    assert case.block_lengths[0] == 65535
    bad = bytearray(case.data)
    bad[case.offsets[0] + 20000] ^= 0x10                  # inside the first block's body: the chain stays whole, its CRC fails
    assert case.offsets[0] + 20000 < case.offsets[1]
    m = SM.salvage(bytes(bad), LB.CAP[1])
    assert (m.mode, m.lost) == (1, [(0, 65535, SM.CRC)])
    got, rep, ranges = decoders[0].salvage_resident_tensor(resident(bad), dtype=torch.int32)
    want = LB.expected(case.name)[1].copy()
    want[:, :65535] = 0
    assert rep["result"] == CORRUPT and rep["mode"] == 1 and ranges == [(0, 65535, "crc")]
    assert (rep["blocks_decoded"], rep["blocks_concealed"], rep["samples_lost"]) == (4, 1, 65535)
    host = got.cpu().numpy()
    assert not host[:, :65535].any()
    assert np.array_equal(host, want), first_bad(host, want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_streaming_decoder_in_1000_byte_fragments(hip, case):
    want = LB.expected(case.name)[1]
    rc, got, _ = hip.streaming_decode(case.data, feed=lambda i: 1000, max_bit_per_sample=32, capacity=LB.CAP)
    assert rc == OK and np.array_equal(got, want), (case.name, rc, first_bad(got, want))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decode_wav_batch_of_one_file(hip, decoders, case):
    (rc, wav), = decoders[0].decode_wav_batch([case.data])
    assert rc == OK
    code, info = hip.wav_info(wav)
    bits, lshift = case.data[23], case.data[24]
    assert code == OK and (info.num_channels, info.bits_per_sample, info.num_samples) == (case.num_channels, bits, case.num_samples)
    assert lshift == 0 and bits in (16, 24)
    want = (LB.expected(case.name)[1].astype(np.int64) >> (32 - bits)).T.reshape(-1)          # interleaved, right-justified
    body = np.frombuffer(wav, np.uint8)[info.data_off:info.data_off + info.data_bytes].reshape(-1, bits // 8).astype(np.int64)
    got = sum(body[:, k] << (8 * k) for k in range(bits // 8))
    got = np.where(got >> (bits - 1), got - (1 << bits), got)
    assert len(wav) == info.data_off + info.data_bytes and np.array_equal(got, want)


def test_an_ordinary_file_decodes_alike_on_both_capacities(hip, decoders):
    small = hip.Decoder(8, 16384, 255, 5, 32)
    try:
        for data in LB.ordinary_files():
            n = int.from_bytes(data[15:19], "big")
            a, b = small.decode_whole(data, n), decoders[0].decode_whole(data, n)
            assert a[0] == b[0] == OK and a[1].shape[1] == n and np.array_equal(a[1], b[1])
    finally:
        small.close()


def test_a_16384_handle_still_refuses_and_65536_is_no_capacity(oracle, hip):
    import torch
    import slalibs as S
    import slastream as SS
    case = LB.by_name()["encoded_70000_max32768"]
    small = hip.Decoder(8, 16384, 255, 5, 32)
    try:
        rc, got = small.decode_whole(case.data, case.num_samples)
        assert rc == EXCEED_HANDLE_CAPACITY and got.shape[1] == 0
        assert small.decode_batch([case.data])[0][0] == EXCEED_HANDLE_CAPACITY
        out, lens, codes = small.decode_resident_tensor([resident(case.data)], dtype=torch.int32)
        assert codes == [EXCEED_HANDLE_CAPACITY] and lens == [0] and not out.cpu().numpy().any()
    finally:
        small.close()
    with pytest.raises(RuntimeError):
        hip.Decoder(8, 65536, 255, 5, 32, long_blocks=True)
    for n in (16385, 32768, 65535):                    # the Python class wants the larger capacity asked for by name
        with pytest.raises(RuntimeError):
            hip.Decoder(8, n, 255, 5, 32)
    with pytest.raises(RuntimeError):
        hip.streaming_decode(case.data, capacity=(8, 65536, 255, 5, 32))
    # a block longer than the handle's capacity under a header that fits it: the walk ends there, the blocks before it stay
    mono = LB.by_name()["mono_16bit_65535_2048raw_40897_3000silent_16385"]
    hdr = bytearray(mono.data[:43])
    hdr[33:35] = (50000).to_bytes(2, "big")
    hdr[8:10] = SS.crc16(hdr[10:]).to_bytes(2, "big")
    data = bytes(hdr) + mono.data[43:]
    mid = hip.Decoder(8, 50000, 255, 5, 32, enable_crc_check=0, long_blocks=True)
    try:
        ro, want, _ = oracle.decode_whole(S.make_params(cap=(8, 50000, 255, 5, 32)), data, mono.num_samples)
        rc, got = mid.decode_whole(data, mono.num_samples)
        assert rc == ro == 4 and got.shape[1] == want.shape[1] == 0      # INSUFFICIENT_BUFFER_SIZE at the first block
    finally:
        mid.close()
