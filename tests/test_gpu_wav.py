"""GPU tests of the four WAV calls (Encoder.encode_wav_batch / encode_wav_resident, Decoder.decode_wav_batch /
decode_wav_resident; run with -m gpu on an MI355X).

Known answers: the reference's own test file under its tool's presets 0, 2 and 4 gives the recorded md5 sums and sizes and
decodes back to the file.  Against the oracle: WAV files built by tests/wavmodel.py from synthetic PCM of every depth, one to
three channels and lengths around the tile and block sizes -- with silence, with shared low zero bits, with an odd chunk
before `data`, with an extensible header -- encode to the bytes the oracle gives for the model's planes, one by one, in one
mixed batch, from device memory into buffers and into an arena; refusals are per item; the decode gives the canonical file
byte for byte or nothing."""
import hashlib
import os

import numpy as np
import pytest

import slalibs as S
import wavmodel as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_WAV = os.path.join(ROOT, "tests", "golden", "a.wav")
# the reference tool's presets 0, 2, 4 (parcor, longterm, lms, mid/side, window, max block: tests/test_gpu_parity.py) and
# what it makes of a.wav under them (recorded: tests/test_gpu_cli.py)
PRESETS = {0: (8, 1, 4, 0, 0, 4096), 2: (16, 1, 8, 1, 1, 12288), 4: (32, 3, 8, 1, 1, 16384)}
KNOWN = {0: ("48c60a59f94f70303be8207d7ea9dc03", 55982), 2: ("9739dfd1acd3eeaec7a3f4345ee8c4a4", 49454),
         4: ("9ad138cb6ad58ab8b074eae1132b3c28", 49450)}
OK, INVALID_ARGUMENT, EXCEED, BUF, DATA_SIZE, HEADER_FORMAT = 0, 2, 3, 4, 9, 10
PARAM = (8, 1, 4, 1, 1, 4096)              # mid/side requested: used only where a file has two channels
LENGTHS = [0, 1, 2047, 2048, 4097, 20000]
BYTE_SENTINEL = 0xC3


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def make_encoder(hip, param=PARAM, channels=8):
    po, lt, lm, ms, win, mb = param
    enc = hip.Encoder(channels, 16384, 48, 5, 40)
    enc.set_encode_parameter(po, lt, lm, ms, win, mb)
    return enc


def oracle_bytes(planes, bits, rate, param=PARAM):
    po, lt, lm, ms, win, mb = param
    p = S.make_params(planes.shape[0], bits, rate, po, lt, lm, ms if planes.shape[0] == 2 else 0, win, mb)
    ret, data = S.oracle().encode_whole(p, planes)
    assert ret == 0
    return data


def oracle_decode(sla, planes, bits, rate, param=PARAM):
    po, lt, lm, ms, win, mb = param
    nch, n = planes.shape
    p = S.make_params(nch, bits, rate, po, lt, lm, ms if nch == 2 else 0, win, mb)
    ret, out = S.oracle().decode_whole(p, sla, n)[:2]
    assert ret == 0
    return np.ascontiguousarray(out[:nch, :n])


class File:
    def __init__(self, name, planes, bits, rate, **how):
        self.name, self.planes, self.bits, self.rate = name, planes, bits, rate
        self.wav = W.build_wav(planes, bits, rate, **how)
        self.sla = oracle_bytes(planes, bits, rate)
        # What a decode gives back: the planes -- except at 32 bits, where the codec's 32-bit arithmetic wraps and the
        # reference's own decoder does not reproduce its encoder's input (the oracle's decode of the oracle's stream differs
        # from the planes in nearly every sample); there the reference is the oracle's decode.
        self.decoded = oracle_decode(self.sla, planes, bits, rate)
        self.lossless = bool(np.array_equal(self.decoded, planes))
        assert self.lossless or bits == 32, name
        self.canonical = W.canonical(self.decoded, bits, rate)


@pytest.fixture(scope="module")
def corpus():
    """the files of the tests and the oracle's answer to each, made once"""
    files = []
    for bits in (8, 16, 24, 32):
        for nch in (1, 2, 3):
            for i, n in enumerate(LENGTHS):
                pcm = S.synth_pcm(nch, max(n, 1), bits, 44100 + 100 * nch, seed=bits * 100 + nch * 10 + i)[:, :n]
                files.append(File("b%dc%dn%d" % (bits, nch, n), pcm, bits, 44100 + 100 * nch))
    pcm = S.synth_pcm(2, 12000, 16, 48000, seed=7)
    pcm[:, 4000:7000] = 0
    files.append(File("silence", pcm, 16, 48000))
    pcm = (S.synth_pcm(2, 9000, 24, 48000, seed=8) >> 11) << 11
    files.append(File("lshift3", pcm, 24, 48000))
    files.append(File("list", S.synth_pcm(2, 5001, 24, 48000, seed=9), 24, 48000, chunks_before_data=[(b"LIST", b"\7" * 27)]))
    files.append(File("extensible", S.synth_pcm(3, 5003, 24, 48000, seed=10), 24, 48000, extensible=True))
    return files


def on_device_at_odd_offsets(datas, gap=3):
    """the byte strings in one device buffer, each at an odd offset; (buffer, [views])"""
    import torch
    total = sum(len(d) + gap + 2 for d in datas) + 16
    host = np.full(total, BYTE_SENTINEL, np.uint8)
    spans, pos = [], 1
    for d in datas:
        pos |= 1
        host[pos:pos + len(d)] = np.frombuffer(d, np.uint8)
        spans.append((pos, len(d)))
        pos += len(d) + gap
    buf = torch.from_numpy(host).cuda()
    return buf, [buf[o:o + n] for o, n in spans]


# ------------------------------------------------------------------ known answers

@pytest.mark.parametrize("mode", sorted(KNOWN))
def test_known_answers_of_the_golden_file(hip, mode):
    wav = open(A_WAV, "rb").read()
    enc, dec = make_encoder(hip, PRESETS[mode]), hip.Decoder()
    try:
        (rc, sla), = enc.encode_wav_batch([wav])
        assert rc == OK
        assert (hashlib.md5(sla).hexdigest(), len(sla)) == KNOWN[mode]
        assert dec.decode_wav_batch([sla]) == [(OK, wav)]
    finally:
        enc.close(); dec.close()


# ------------------------------------------------------------------ against the oracle

@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_single_files_equal_the_oracle(hip, corpus, bits):
    enc = make_encoder(hip)
    try:
        for f in corpus:
            if f.bits != bits:
                continue
            assert enc.encode_wav_batch([f.wav]) == [(OK, f.sla)], f.name
    finally:
        enc.close()


def test_the_special_files_hold_what_they_are_meant_to(hip, corpus):
    by = {f.name: f for f in corpus}
    assert hip.decode_header(by["lshift3"].sla)[1].wave_format.offset_lshift == 3
    assert hip.decode_header(by["b16c1n20000"].sla)[1].wave_format.offset_lshift == 0
    assert len(by["b24c2n0"].sla) == 43                              # the empty data chunk: its header
    assert hip.wav_info(by["list"].wav)[1].data_off == 44 + 8 + 28   # the odd chunk and its pad byte
    assert hip.wav_info(by["extensible"].wav)[1].data_off == 44 + 24


def test_one_mixed_batch(hip, corpus):
    order = sorted(range(len(corpus)), key=lambda i: (i * 7) % len(corpus))      # the formats interleaved
    files = [corpus[i] for i in order]
    enc = make_encoder(hip)
    try:
        got = enc.encode_wav_batch([f.wav for f in files])
        for f, (rc, data) in zip(files, got):
            assert (rc, data) == (OK, f.sla), f.name
        # the handle's wave format is the last group's: the format that appeared last for the first time
        seen = []
        for f in files:
            if (f.planes.shape[0], f.bits, f.rate) not in seen:
                seen.append((f.planes.shape[0], f.bits, f.rate))
        last = next(f for f in files if (f.planes.shape[0], f.bits, f.rate) == seen[-1] and f.planes.shape[1] > 4000)
        enc.num_channels = last.planes.shape[0]
        # ... and the encode parameter is the caller's, mid/side still requested: a batch of the format the call left (no
        # set_wave_format here) runs with it when that format has two channels and is refused for the method otherwise
        if last.planes.shape[0] != 2:
            with pytest.raises(hip.SlaError) as err:
                enc.encode_batch([last.planes])
            assert err.value.code == 5                               # INVAILD_CHPROCESSMETHOD
            po, lt, lm, ms, win, mb = PARAM
            enc.set_encode_parameter(po, lt, lm, 0, win, mb)
        assert enc.encode_batch([last.planes]) == [(OK, last.sla)]
    finally:
        enc.close()


# ------------------------------------------------------------------ resident equals host

def test_resident_equals_host_in_buffers_and_in_an_arena(hip, corpus):
    import torch
    files = [f for f in corpus if f.planes.shape[1] in (0, 2047, 4097) or f.name in ("silence", "lshift3", "list", "extensible")]
    enc = make_encoder(hip)
    try:
        _, srcs = on_device_at_odd_offsets([f.wav for f in files])
        caps = [len(f.sla) + (5 if i % 2 else 0) for i, f in enumerate(files)]
        host = np.full(sum(caps) + 4 * len(caps) + 16, BYTE_SENTINEL, np.uint8)
        buf = torch.from_numpy(host).cuda()
        outs, offs, pos = [], [], 1
        for cap in caps:
            pos |= 1
            outs.append(buf[pos:pos + cap]); offs.append(pos)
            pos += cap + 3
        got = enc.encode_wav_resident(srcs, outs=outs)
        expect = host.copy()
        for f, o in zip(files, offs):
            expect[o:o + len(f.sla)] = np.frombuffer(f.sla, np.uint8)
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == [(OK, f.sla) for f in files]
        assert np.array_equal(buf.cpu().numpy(), expect)             # the files, and nothing between or behind them

        # the arena: one format (one group, one offset_lshift, one pass) lies in item order, back to back
        same = [f for f in files if (f.planes.shape[0], f.bits) == (2, 16) and f.name != "silence"]
        _, srcs = on_device_at_odd_offsets([f.wav for f in same])
        total = sum(len(f.sla) for f in same)
        arena = torch.from_numpy(np.full(total + 40, BYTE_SENTINEL, np.uint8)).cuda()
        got = enc.encode_wav_resident(srcs, arena=arena)
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == [(OK, f.sla) for f in same]
        assert arena.cpu().numpy().tobytes() == b"".join(f.sla for f in same) + bytes([BYTE_SENTINEL]) * 40
        # every format in one arena: every file delivered, the files tile [0, total) without gap or overlap
        _, srcs = on_device_at_odd_offsets([f.wav for f in files])
        total = sum(len(f.sla) for f in files)
        arena = torch.from_numpy(np.full(total + 40, BYTE_SENTINEL, np.uint8)).cuda()
        got = enc.encode_wav_resident(srcs, arena=arena)
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == [(OK, f.sla) for f in files]
        spans, pos = sorted((v.data_ptr() - arena.data_ptr(), v.numel()) for _, v in got), 0
        for o, n in spans:
            assert o == pos
            pos += n
        assert pos == total and arena[total:].cpu().numpy().tobytes() == bytes([BYTE_SENTINEL]) * 40
        # an arena that is too small for the last file of the group: the cursor stays, the others are delivered
        arena = torch.from_numpy(np.full(sum(len(f.sla) for f in same) - 1, BYTE_SENTINEL, np.uint8)).cuda()
        _, srcs = on_device_at_odd_offsets([f.wav for f in same])
        got = enc.encode_wav_resident(srcs, arena=arena)
        assert [rc for rc, _ in got] == [OK] * (len(same) - 1) + [BUF] and got[-1][1].numel() == 0
    finally:
        enc.close()


def test_probe_rounds_find_a_data_chunk_behind_a_long_chunk(hip):
    planes = S.synth_pcm(2, 5000, 16, 48000, seed=21)
    far = W.build_wav(planes, 16, 48000, chunks_before_data=[(b"JUNK", b"\1" * 10000)])
    farther = W.build_wav(planes, 16, 48000, chunks_before_fmt=[(b"JUNK", b"\1" * 5001)], chunks_before_data=[(b"LIST", b"\2" * 9999)])
    want = oracle_bytes(planes, 16, 48000)
    enc = make_encoder(hip)
    try:
        _, srcs = on_device_at_odd_offsets([far, W.build_wav(planes, 16, 48000), farther])
        import torch
        outs = [torch.empty(len(want), dtype=torch.uint8, device="cuda") for _ in srcs]
        got = enc.encode_wav_resident(srcs, outs=outs)
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == [(OK, want)] * 3
        assert enc.encode_wav_batch([far, farther]) == [(OK, want)] * 2
    finally:
        enc.close()


# ------------------------------------------------------------------ refusals

def test_refusals_are_per_item(hip, corpus):
    import torch
    good = next(f for f in corpus if f.name == "b16c2n4097")
    frames = W.frames_from_planes(good.planes, 16)
    nine = W.build_wav(S.synth_pcm(9, 100, 16, 48000, seed=3), 16, 48000)
    bad = [
        (b"RIFX" + good.wav[4:], HEADER_FORMAT),                                              # no signature
        (b"RIFF\0\0\0\0WAVE" + W.chunk(b"data", frames) + good.wav[12:36], HEADER_FORMAT),   # data before fmt
        (good.wav[:16] + b"\x0e" + good.wav[17:], HEADER_FORMAT),                             # fmt shorter than 16 bytes
        (good.wav[:20] + b"\x03" + good.wav[21:], HEADER_FORMAT),                             # format tag
        (good.wav[:34] + b"\x14" + good.wav[35:], HEADER_FORMAT),                             # bit depth
        (good.wav[:22] + b"\0\0" + good.wav[24:], HEADER_FORMAT),                             # zero channels
        (good.wav[:40], DATA_SIZE),                                                           # the chain runs off the end
        (W.build_wav(good.planes, 16, good.rate, data_size=len(frames) + 1), DATA_SIZE),      # data claims too much
        (nine, EXCEED),                                                                       # nine channels, handle of eight
    ]
    wavs, want = [], []
    for w, code in bad:
        wavs += [w, good.wav]
        want += [(code, b""), (OK, good.sla)]
    enc = make_encoder(hip)
    try:
        assert enc.encode_wav_batch(wavs) == want
        # a capacity one byte short: encode_batch's code
        caps = [len(good.sla) - 1, len(good.sla), 42]
        assert enc.encode_wav_batch([good.wav] * 3, capacities=caps) == [(BUF, b""), (OK, good.sla), (BUF, b"")]
        enc.set_wave_format(2, 16, good.rate)
        po, lt, lm, ms, win, mb = PARAM
        assert [rc for rc, _ in enc.encode_batch([good.planes] * 3, capacities=caps)] == [BUF, OK, BUF]
        # the resident call: the same per-item codes; a refused item's buffer keeps its sentinel
        _, srcs = on_device_at_odd_offsets(wavs)
        outs = [torch.from_numpy(np.full(len(good.sla) + 9, BYTE_SENTINEL, np.uint8)).cuda() for _ in wavs]
        got = enc.encode_wav_resident(srcs, outs=outs)
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == want
        for (code, _), out in zip(want, outs):
            tail = out.cpu().numpy()[len(good.sla) if code == OK else 0:]
            assert np.all(tail == BYTE_SENTINEL)
        # a host pointer as a resident source, and as a resident destination
        hostbuf = np.frombuffer(good.wav, np.uint8).copy()
        outs = [torch.from_numpy(np.full(len(good.sla), BYTE_SENTINEL, np.uint8)).cuda() for _ in range(3)]
        got = enc.encode_wav_resident([(hostbuf.ctypes.data, len(hostbuf)), srcs[1], (0, 10)], outs=outs)
        assert [rc for rc, _ in got] == [INVALID_ARGUMENT, OK, INVALID_ARGUMENT]
        assert got[1][1].cpu().numpy().tobytes() == good.sla
        assert np.all(outs[0].cpu().numpy() == BYTE_SENTINEL) and np.all(outs[2].cpu().numpy() == BYTE_SENTINEL)
        # NULL items with a count
        assert enc._lib.sla_hip_encode_wav_batch(enc._h, None, 1) == INVALID_ARGUMENT
        assert enc._lib.sla_hip_encode_wav_batch_resident(enc._h, None, 1, None, 0, None) == INVALID_ARGUMENT
    finally:
        enc.close()


# ------------------------------------------------------------------ decode to WAV

def test_decode_gives_the_canonical_file(hip, corpus):
    import torch
    dec = hip.Decoder()
    try:
        got = dec.decode_wav_batch([f.sla for f in corpus])
        for f, (rc, wav) in zip(corpus, got):
            assert (rc, wav) == (OK, f.canonical), f.name
        # resident: sources and destinations at odd offsets of sentinel-filled buffers
        _, srcs = on_device_at_odd_offsets([f.sla for f in corpus])
        sizes = [len(f.canonical) for f in corpus]
        host = np.full(sum(sizes) + 4 * len(sizes) + 16, BYTE_SENTINEL, np.uint8)
        buf = torch.from_numpy(host).cuda()
        outs, offs, pos = [], [], 1
        for n in sizes:
            pos |= 1
            outs.append(buf[pos:pos + n]); offs.append(pos)
            pos += n + 3
        got = dec.decode_wav_resident(srcs, outs=outs)
        expect = host.copy()
        for f, o in zip(corpus, offs):
            expect[o:o + len(f.canonical)] = np.frombuffer(f.canonical, np.uint8)
        assert [rc for rc, _ in got] == [OK] * len(corpus)
        assert np.array_equal(buf.cpu().numpy(), expect)
        # destinations allocated from the headers
        few = [f for f in corpus if f.planes.shape[1] == 2048]
        _, srcs = on_device_at_odd_offsets([f.sla for f in few])
        got = dec.decode_wav_resident(srcs)
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == [(OK, f.canonical) for f in few]
    finally:
        dec.close()


def test_decode_delivers_whole_files_or_nothing(hip, corpus):
    import torch
    a = next(f for f in corpus if f.name == "b16c2n20000")
    b = next(f for f in corpus if f.name == "b24c3n4097")
    broken = bytearray(a.sla)
    broken[len(broken) // 2] ^= 0x10                                 # one flipped bit in a block body
    broken = bytes(broken)
    enc = hip.Encoder(8, 16384, 48, 5, 40)
    enc.set_wave_format(1, 20, 48000)
    enc.set_encode_parameter(8, 1, 4, 0, 1, 4096)
    dec = hip.Decoder()
    try:
        (rc, twenty), = enc.encode_batch([S.synth_pcm(1, 3000, 20, 48000, seed=5)])
        assert rc == OK
        code = dec.decode_batch([broken])[0][0]
        assert code != OK
        assert dec.decode_wav_batch([a.sla, broken, b.sla, twenty]) == [(OK, a.canonical), (code, b""), (OK, b.canonical),
                                                                        (HEADER_FORMAT, b"")]
        _, srcs = on_device_at_odd_offsets([a.sla, broken, b.sla, twenty, a.sla])
        sizes = [len(a.canonical), len(a.canonical), len(b.canonical), 44 + 3000 * 3, len(a.canonical) - 1]
        outs = [torch.from_numpy(np.full(n + 6, BYTE_SENTINEL, np.uint8)).cuda()[3:3 + n] for n in sizes]
        got = dec.decode_wav_resident(srcs, outs=outs)
        assert [rc for rc, _ in got] == [OK, code, OK, HEADER_FORMAT, BUF]
        assert [v.cpu().numpy().tobytes() for _, v in got] == [a.canonical, b"", b.canonical, b"", b""]
        for k in (1, 3, 4):
            assert np.all(outs[k].cpu().numpy() == BYTE_SENTINEL)   # untouched
        # the host call with a capacity one byte short
        items = (hip.WavItem * 1)()
        src = np.frombuffer(a.sla, np.uint8)
        dst = np.full(len(a.canonical), BYTE_SENTINEL, np.uint8)
        items[0].src, items[0].src_size, items[0].dst, items[0].dst_capacity = src.ctypes.data, len(src), dst.ctypes.data, len(dst) - 1
        assert dec._lib.sla_hip_decode_wav_batch(dec._h, items, 1) == 0
        assert (items[0].result, items[0].output_size) == (BUF, 0) and np.all(dst == BYTE_SENTINEL)
        assert dec._lib.sla_hip_decode_wav_batch(dec._h, None, 1) == INVALID_ARGUMENT
        assert dec._lib.sla_hip_decode_wav_batch_resident(dec._h, None, 1, None) == INVALID_ARGUMENT
    finally:
        enc.close(); dec.close()


# ------------------------------------------------------------------ options

@pytest.mark.parametrize("option, value", [("verify", 1), ("silence_runs", 1024)])
def test_round_trip_with_options(hip, corpus, option, value):
    import torch
    files = [f for f in corpus if f.planes.shape[1] in (4097, 20000) or f.name in ("silence", "lshift3", "list", "extensible")]
    enc, dec = make_encoder(hip), hip.Decoder()
    try:
        enc.set_option(option, value)
        _, srcs = on_device_at_odd_offsets([f.wav for f in files])
        slas = enc.encode_wav_resident(srcs, outs=[torch.empty(len(f.sla) + 8, dtype=torch.uint8, device="cuda") for f in files])
        # verify decodes every stream on the device and compares it with the planes before the file is delivered: a file
        # the codec does not carry losslessly (File.lossless: the 32-bit ones) is refused with NG and nothing written, as on
        # every other route of the encoder; every other file is delivered
        ok = [f.lossless or option != "verify" for f in files]
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in slas] == [(OK, f.sla) if k else (1, b"") for f, k in zip(files, ok)]
        assert not all(ok) or option != "verify"
        kept = [(f, v) for f, (_, v), k in zip(files, slas, ok) if k]
        back = dec.decode_wav_resident([v for _, v in kept])
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in back] == [(OK, f.canonical) for f, _ in kept]
    finally:
        enc.close(); dec.close()
