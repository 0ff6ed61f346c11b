"""GPU tests of sla_hip_decode_batch_device (Decoder.decode_batch_into / decode_batch_tensor; run with -m gpu on an
MI355X): many .sla files in host memory decoded into caller-owned device tensors.

The reference for every item is Decoder.decode_batch of the same files on a second handle of the same configuration:
the same result code and sample count, and its left-justified samples converted as the format says -- S32_LEFT bit for
bit, F32 as np.float32(left) * 2**-31 compared through its bits, S16 and S32 as the numpy shifts.  Covered: every
format in planar, interleaved and padded-batch layouts; mixed formats over several passes; the crafted-stream
catalogue with the CRC check on and off; damaged files between good ones; guard bands around every destination; the
per-item argument refusals; ordering behind work queued on the caller's stream; handle reuse; a batch across the pass
cap; the empty call.  Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

import crafted_catalogue as CC
import slalibs as S
import test_gpu_decode_batch as TB
import waveforms as W

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, BUF = 0, 2, 4
S32_LEFT, S32, S16, F32 = range(4)
FORMATS = [S32_LEFT, S32, S16, F32]
FMT_IDS = ["s32_left", "s32", "s16", "f32"]
SENTINEL = -0x5A5A5A5B                       # bit pattern of every untouched int32 word (0xA5A5A5A5)


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def torch_dtype(fmt):
    import torch
    return {S32_LEFT: torch.int32, S32: torch.int32, S16: torch.int16, F32: torch.float32}[fmt]


def header(data):
    """(channels, bit_per_sample) the header gives, (0, 0) when it gives none"""
    b = np.frombuffer(bytes(data), np.uint8)
    import sla_amd
    rc, h = sla_amd.decode_header(b)
    return (h.wave_format.num_channels, h.wave_format.bit_per_sample) if rc in (0, 11) else (0, 0)


def convert(left, fmt, bps):
    """numpy form of the emit conversion of left-justified int32 samples"""
    left = np.asarray(left, np.int32)
    if fmt == S32_LEFT:
        return left
    if fmt == S32:
        return left >> np.int32((32 - bps) & 31)
    if fmt == S16:
        return (left >> np.int32(16)).astype(np.int16)
    return left.astype(np.float32) * np.float32(2.0 ** -31)


def bits_of(a):
    """comparable integer view (floats by their bits)"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def sentinel_like(fmt):
    return {S32_LEFT: SENTINEL, S32: SENTINEL, S16: -0x5A5B, F32: None}[fmt]


def alloc(shape, fmt):
    """a device tensor filled with the sentinel bit pattern"""
    import torch
    if fmt == F32:
        return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, sentinel_like(fmt), dtype=torch_dtype(fmt), device="cuda")


def sentinel_bits(fmt):
    return SENTINEL if fmt in (F32, S32_LEFT, S32) else -0x5A5B


def check_items(ref_got, got, outs, datas, fmt, zero_fill):
    """every item against decode_batch: code, count, samples; past the count zero (zero_fill) or the sentinel"""
    for i, ((rr, left), (rc, n), out) in enumerate(zip(ref_got, got, outs)):
        assert rc == rr, ("item", i, rc, rr)
        assert n == left.shape[1], ("item", i, n, left.shape)
        nch, bps = header(datas[i])
        o = bits_of(out.cpu().numpy())
        if n > 0:
            assert np.array_equal(o[:nch, :n], bits_of(convert(left[:nch], fmt, bps))), ("item", i)
        tail = o[:nch, n:]
        assert (tail == 0).all() if zero_fill else (tail == sentinel_bits(fmt)).all(), ("item", i, "tail")
        assert (o[nch:] == sentinel_bits(fmt)).all(), ("item", i, "rows past the header's channels")


def run_layout(hip, ref, dec, datas, caps, fmt, layout, zero_fill=True):
    ref_got = ref.decode_batch(datas, capacities=caps)
    outs = []
    for data, cap in zip(datas, caps):
        nch = max(header(data)[0], 1)
        if layout == "planar":
            outs.append(alloc((nch, cap), fmt))
        else:
            outs.append(alloc((cap, nch), fmt).t())
    got = dec.decode_batch_into(datas, outs, fmt, zero_fill=zero_fill)
    check_items(ref_got, got, outs, datas, fmt, zero_fill)
    return got


def pair(hip, cap=TB.HANDLE_CAP, crc=1):
    return hip.Decoder(*cap, enable_crc_check=crc), hip.Decoder(*cap, enable_crc_check=crc)


@pytest.fixture(scope="module")
def c4_clips(hip):
    lens = [480000 - 3001 * i - (i % 3) * 517 for i in range(6)]
    pcms = [S.synth_pcm(2, n, 16, 48000, seed=700 + i) for i, n in enumerate(lens)]
    return TB.encode_clips(hip, TB.C4, pcms), lens, pcms


# ------------------------------------------------------------------ every format x layout on C4-shaped clips

@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_c4_clips_every_format_and_layout(hip, c4_clips, fmt, layout):
    datas, lens, pcms = c4_clips
    caps = [n + 1000 for n in lens]                       # room past the end: the zero fill shows
    dec, ref = pair(hip)
    try:
        got = run_layout(hip, ref, dec, datas, caps, fmt, layout)
        assert all(rc == OK for rc, _ in got)
        t = dec.last_timing()
        assert t[5] == 1 and t[3] > 0                     # one pass; the emit stage took time
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_padded_batch_tensor(hip, c4_clips, fmt, layout):
    import torch
    datas, lens, pcms = c4_clips
    dtype, rj = torch_dtype(fmt), fmt == S32
    dec, ref = pair(hip)
    try:
        t, lengths, results = dec.decode_batch_tensor(datas, dtype=dtype, layout=layout, right_justify=rj)
        assert t.dtype == dtype and t.device.type == "cuda"
        L = max(lens)
        assert tuple(t.shape) == ((len(datas), 2, L) if layout == "planar" else (len(datas), L, 2))
        assert lengths == lens and results == [OK] * len(datas)
        host = t.cpu().numpy()
        for b, pcm in enumerate(pcms):
            o = host[b] if layout == "planar" else host[b].T
            assert np.array_equal(bits_of(o[:, :lens[b]]), bits_of(convert(pcm, fmt, 16))), b
            assert (bits_of(o[:, lens[b]:]) == 0).all(), b
        # a shorter length: INSUFFICIENT_BUFFER_SIZE where decode_batch gives it, the same prefix
        t2, lengths2, results2 = dec.decode_batch_tensor(datas, dtype=dtype, layout=layout, length=300000, right_justify=rj)
        want = ref.decode_batch(datas, capacities=[300000] * len(datas))
        assert results2 == [rc for rc, _ in want] and lengths2 == [o.shape[1] for _, o in want]
        assert all(rc == BUF for rc in results2)
    finally:
        dec.close(); ref.close()


def test_padded_batch_of_mixed_channel_counts_zeroes_the_missing_rows(oracle, hip):
    import torch
    files = TB._mixed_files(oracle)
    datas = [d for d, _ in files] + [b"", b"SL*\x01 not a header" + bytes(40)]
    dec, ref = pair(hip)
    try:
        t, lengths, results = dec.decode_batch_tensor(datas, dtype=torch.float32)
        want = ref.decode_batch(datas)
        assert results == [rc for rc, _ in want] and lengths == [o.shape[1] for _, o in want]
        host = t.cpu().numpy()
        assert host.shape == (len(datas), 8, max(pcm.shape[1] for _, pcm in files))
        for b, (rc, left) in enumerate(want):
            nch, bps = header(datas[b])
            assert np.array_equal(bits_of(host[b, :nch, :left.shape[1]]), bits_of(convert(left[:nch], F32, bps))), b
            assert (bits_of(host[b, :nch, left.shape[1]:]) == 0).all(), b
            assert (bits_of(host[b, nch:]) == 0).all(), b
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ mixed formats, crafted streams, damaged files

def _mixed_set(oracle):
    """1-8 channels, 8/16/24/32-bit (crafted 4/12/20/32-bit cases among them), mid/side and not: several passes"""
    datas = [d for d, _ in TB._mixed_files(oracle)]
    pick = [c for c in CC.catalogue() if c.fmt.bits in (4, 12, 20, 32) or c.fmt.num_channels in (3, 8)][:8]
    for i, c in enumerate(pick):
        datas.insert(2 * i + 1, c.data)
    p8 = S.make_params(2, 8, 48000, 8, 1, 8, 1, 1, 4096)
    ret, d8 = oracle.encode_whole(p8, W.music_like(2, 7001, 8, seed=61))
    assert ret == 0
    datas.insert(3, d8)
    return datas


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_mixed_formats_in_one_call(oracle, hip, fmt):
    datas = _mixed_set(oracle)
    caps = [int.from_bytes(bytes(d[15:19]), "big") + 17 * (i % 3) for i, d in enumerate(datas)]
    bits = {header(d)[1] for d in datas}
    assert {8, 16, 24, 32} <= bits
    dec, ref = pair(hip, CC.CAP)
    try:
        got = run_layout(hip, ref, dec, datas, caps, fmt, "planar")
        assert dec.last_timing()[5] >= 4
        got = run_layout(hip, ref, dec, datas, caps, fmt, "interleaved", zero_fill=False)
        assert all(rc == OK for rc, _ in got)
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("crc", [1, 0])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_crafted_catalogue(hip, crc, fmt):
    cases = CC.catalogue()
    assert len(cases) == 52
    datas = [c.data for c in cases]
    caps = [c.num_samples for c in cases]
    dec, ref = pair(hip, CC.CAP, crc)
    try:
        got = run_layout(hip, ref, dec, datas, caps, fmt, "planar")
        assert all(rc == OK for rc, _ in got)
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("crc", [1, 0])
@pytest.mark.parametrize("zero_fill", [True, False])
def test_damaged_files_between_good_ones(oracle, hip, crc, zero_fill):
    entries = TB._damaged_set(oracle, hip)
    good = [e for e in entries if e[0].startswith("good")]
    order = []
    for j, e in enumerate(e for e in entries if not e[0].startswith("good")):
        order += [good[j % len(good)], e]
    order.append(good[0])
    names = [e[0] for e in order]
    assert "size field disagrees" in names and "buffer too small" in names
    datas, caps = [e[1] for e in order], [e[2] for e in order]
    for fmt in (S32_LEFT, F32):
        dec, ref = pair(hip, crc=crc)
        try:
            got = run_layout(hip, ref, dec, datas, caps, fmt, "planar", zero_fill=zero_fill)
        finally:
            dec.close(); ref.close()
        codes = {n: rc for n, (rc, _) in zip(names, got)}
        assert codes["buffer too small"] == BUF and codes["no samples"] == OK


# ------------------------------------------------------------------ guard bands, argument refusals

@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_guard_bands(oracle, hip, fmt):
    """all items in one allocation, sentinel gaps between regions and past every capacity: only [0, n) changes
    without the zero fill, only [0, capacity) with it"""
    import torch
    entries = TB._damaged_set(oracle, hip)
    datas = [e[1] for e in entries]
    caps = [e[2] for e in entries]
    gap = 37
    layout, off = [], 64
    for k, (data, cap) in enumerate(zip(datas, caps)):
        nch = header(data)[0]
        cs = cap + gap                                     # planar, a gap after every channel
        if k % 2 == 0:                                     # every other region aligned for the kernel's wide stores
            cs += (-cs) % 4
            off += (-off) % 4
        layout.append((off, cs, nch))
        off += max(nch, 1) * cs + gap + 3
    total = off + 64
    dec, ref = pair(hip)
    try:
        ref_got = ref.decode_batch(datas, capacities=caps)
        for zero_fill in (False, True):
            base = alloc((total,), fmt)
            outs = [base[o:o + max(nch, 1) * cs].view(max(nch, 1), cs)[:, :cap] for (o, cs, nch), cap in zip(layout, caps)]
            got = dec.decode_batch_into(datas, outs, fmt, zero_fill=zero_fill)
            host = bits_of(base.cpu().numpy())
            expect = np.full(total, sentinel_bits(fmt), host.dtype)
            for (o, cs, nch), cap, (rc, n), (rr, left), data in zip(layout, caps, got, ref_got, datas):
                assert (rc, n) == (rr, left.shape[1])
                bps = header(data)[1]
                for c in range(nch):
                    if n > 0:
                        expect[o + c * cs:o + c * cs + n] = bits_of(convert(left[c], fmt, bps))
                    if zero_fill:
                        expect[o + c * cs + n:o + c * cs + cap] = 0
            bad = np.nonzero(host != expect)[0]
            assert bad.size == 0, ("zero_fill", zero_fill, bad[:10])
    finally:
        dec.close(); ref.close()


def test_argument_refusals_are_per_item(oracle, hip):
    import torch
    L = hip.lib()
    p, pcm, data, offs, tr = TB._stream(oracle, seed=50)
    data = bytes(data)
    n = pcm.shape[1]
    buf = np.frombuffer(data, np.uint8)
    outs = [alloc((2, n + 8), F32) for _ in range(6)]
    dec, _ = pair(hip)
    try:
        items = (hip.DecodeDeviceItem * 6)()
        for i in range(6):
            items[i].data = buf.ctypes.data_as(hip.u8p)
            items[i].data_size = len(buf)
            items[i].dst = outs[i].data_ptr()
            items[i].channel_stride = n + 8
            items[i].sample_stride = 1
            items[i].capacity = n
            items[i].output_num_samples = 12345
        items[1].dst = None                                # NULL dst
        items[2].sample_stride = 0                         # zero sample stride
        items[3].channel_stride = 0                        # zero channel stride on a stereo file
        items[4].dst = outs[4].data_ptr() + 2              # not aligned to the 4-byte element
        st = torch.cuda.current_stream().cuda_stream
        assert L.sla_hip_decode_batch_device(C.c_void_p(dec._h), items, 6, F32, hip.DEC_ZERO_FILL, C.c_void_p(st)) == 0
        torch.cuda.synchronize()
        want = bits_of(convert(pcm, F32, 16))
        for i in (0, 5):
            assert items[i].result == OK and items[i].output_num_samples == n
            assert np.array_equal(bits_of(outs[i].cpu().numpy()[:, :n]), want)
        for i in (1, 2, 3, 4):
            assert items[i].result == INVALID_ARGUMENT and items[i].output_num_samples == 0, i
            assert (bits_of(outs[i].cpu().numpy()) == SENTINEL).all(), i
        # the Python layer refuses mismatches before the library is called
        with pytest.raises(ValueError):
            dec.decode_batch_into([data], [alloc((2, n), S16)], F32)                         # dtype
        with pytest.raises(ValueError):
            dec.decode_batch_into([data], [alloc((1, n), F32)], F32)                         # too few rows
        with pytest.raises(ValueError):
            dec.decode_batch_into([data], [torch.zeros((2, n), dtype=torch.float32)], F32)   # host tensor
        with pytest.raises(ValueError):
            dec.decode_batch_into([data, data], [alloc((2, n), F32)], F32)                   # count
    finally:
        dec.close()


# ------------------------------------------------------------------ ordering, reuse, scale, empty

def test_waits_for_work_queued_on_the_callers_stream(hip, c4_clips):
    import torch
    datas, lens, pcms = c4_clips
    L = max(lens)
    dec, _ = pair(hip)
    try:
        side = torch.cuda.Stream()
        out = torch.empty((len(datas), 2, L), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(50_000_000)                  # the fills below start well after the call has begun
            for k in range(4):
                out.fill_(float(k + 1))
        got = dec.decode_batch_into(datas, [out[b] for b in range(len(datas))], F32, stream=side)
        side.synchronize()
        host = out.cpu().numpy()
        for b, pcm in enumerate(pcms):
            assert got[b] == (OK, lens[b])
            assert np.array_equal(bits_of(host[b, :, :lens[b]]), bits_of(convert(pcm, F32, 16))), b
            assert (host[b, :, lens[b]:] == 0).all(), b
    finally:
        dec.close()


def test_handle_reuse_across_device_host_and_whole(oracle, hip):
    import torch
    files = TB._mixed_files(oracle)
    datas, caps = [d for d, _ in files], [pcm.shape[1] for _, pcm in files]
    dec, ref = pair(hip)
    try:
        first = run_layout(hip, ref, dec, datas, caps, S32_LEFT, "planar")
        host = dec.decode_batch(datas, caps)
        for (data, pcm), cap, (rc, o) in zip(files, caps, host):
            assert rc == OK and np.array_equal(o, pcm)
            rw, ow = dec.decode_whole(data, cap)
            assert rw == OK and np.array_equal(ow, pcm)
        again = run_layout(hip, ref, dec, datas, caps, F32, "interleaved")
        assert first == again
        t, lengths, results = dec.decode_batch_tensor(datas, dtype=torch.int32)
        assert results == [OK] * len(files) and lengths == caps
    finally:
        dec.close(); ref.close()


def test_300_clips_cross_the_pass_cap(hip):
    import torch
    bases = [S.synth_pcm(2, 480000, 16, 48000, seed=300 + k) for k in range(4)]
    lens = [480000 - (i * 37) % 2000 for i in range(300)]
    pcms = [np.ascontiguousarray(bases[i % 4][:, :n]) for i, n in enumerate(lens)]
    datas = TB.encode_clips(hip, TB.C4, pcms)
    dec, _ = pair(hip)
    try:
        t, lengths, results = dec.decode_batch_tensor(datas, dtype=torch.float32)
        assert dec.last_timing()[5] >= 2
        assert results == [OK] * 300 and lengths == lens
        for b in range(0, 300, 10):
            chunk = t[b:b + 10].cpu().numpy()
            for k in range(chunk.shape[0]):
                i = b + k
                assert np.array_equal(bits_of(chunk[k, :, :lens[i]]), bits_of(convert(pcms[i], F32, 16))), i
                assert (chunk[k, :, lens[i]:] == 0).all(), i
    finally:
        dec.close()


def test_empty_call(hip):
    import torch
    dec, _ = pair(hip)
    try:
        assert dec.decode_batch_into([], [], F32) == []
        t, lengths, results = dec.decode_batch_tensor([])
        assert tuple(t.shape) == (0, 0, 0) and lengths == [] and results == []
        L = hip.lib()
        assert L.sla_hip_decode_batch_device(C.c_void_p(dec._h), None, 0, F32, 0, None) == 0
    finally:
        dec.close()
