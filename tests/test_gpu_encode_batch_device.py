"""GPU tests of sla_hip_encode_batch_device (Encoder.encode_batch_from / encode_batch_tensor; run with -m gpu on an
MI355X): many files whose PCM already lives in device tensors, encoded to .sla bytes without a host copy.

The reference for every item is Encoder.encode_batch on a second handle of the same settings, given the host planes of the
left-justified words the format's conversion makes (`left` of tests/pcmmodel.py: the numpy form of the table in include/sla_hip.h); some
items also against the oracle's encode.  Covered: C4-shaped clips in every format and layout (planar, interleaved, an
unaligned interleaved view, every other sample of a wider tensor, a padded batch with lengths); 8-channel 24-bit files;
round trips through decode_batch_tensor in every dtype; the F32 quantiser on crafted floats and a NaN; the S32 range; the
per-item argument refusals; ordering behind work queued on the caller's stream; handle reuse; a batch across the pass cap;
the empty call."""
import ctypes as C

import numpy as np
import pytest

import slalibs as S
import test_gpu_batch as GB
from pcmmodel import elements, left, wrap32

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CAPACITY, BUF, NOT_SET = 0, 2, 3, 4, 15
S32_LEFT, S32, S16, F32 = range(4)
FORMATS = [S32_LEFT, S32, S16, F32]
FMT_IDS = ["s32_left", "s32", "s16", "f32"]
C4 = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096, cap=(2, 4096, 16, 1, 8))
MONO16 = S.make_params(1, 16, 48000, 8, 1, 4, 0, 1, 4096)
MONO24 = S.make_params(1, 24, 48000, 8, 1, 4, 0, 1, 4096)
OCTO24 = S.make_params(8, 24, 96000, 48, 3, 8, 0, 1, 8192)


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def on_device(a, layout="planar"):
    """numpy [C][n] -> a device tensor view [C][n] in the given storage layout"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    nch, n = t.shape
    if layout == "planar":
        return t.cuda()
    if layout == "interleaved":                                     # [n][C] storage, passed as .T
        return t.t().contiguous().cuda().t()
    if layout == "interleaved_offset":                              # one frame in: not aligned for the wide loads
        buf = torch.zeros((n + 1, nch), dtype=t.dtype)
        buf[1:] = t.t()
        return buf.cuda()[1:].t()
    if layout == "every_other":                                     # every other sample of a wider tensor
        buf = torch.zeros((nch, 2 * n + 3), dtype=t.dtype)
        buf[:, 1:2 * n + 1:2] = t
        return buf.cuda()[:, 1:2 * n + 1:2]
    raise KeyError(layout)


def reference(hip, p, lefts, capacities=None):
    """encode_batch of host planes on a handle of its own; a None plane (a refused item) is (INVALID_ARGUMENT, b"")"""
    idx = [i for i, x in enumerate(lefts) if x is not None]
    ref = GB.make_encoder(hip, p)
    try:
        got = ref.encode_batch([lefts[i] for i in idx], capacities=None if capacities is None else [capacities[i] for i in idx])
    finally:
        ref.close()
    out = [(INVALID_ARGUMENT, b"")] * len(lefts)
    for i, g in zip(idx, got):
        out[i] = g
    return out


def encode_from(hip, p, srcs, fmt, **kw):
    enc = GB.make_encoder(hip, p)
    try:
        return enc.encode_batch_from(srcs, fmt, **kw)
    finally:
        enc.close()


@pytest.fixture(scope="module")
def c4_clips():
    lens = [480000, 300001, 4096, 4097, 2047, 99999]
    return [S.synth_pcm(2, n, 16, 48000, seed=800 + i) for i, n in enumerate(lens)]


@pytest.fixture(scope="module")
def c4_want(hip, c4_clips):
    want = reference(hip, C4, c4_clips)
    assert all(rc == OK for rc, _ in want)
    return want


# ------------------------------------------------------------------ C4 clips: every format x layout

@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("layout", ["planar", "interleaved", "interleaved_offset", "every_other"])
def test_c4_clips_every_format_and_layout(hip, c4_clips, c4_want, fmt, layout):
    import torch
    srcs = [on_device(elements(pcm, fmt, 16), layout) for pcm in c4_clips]
    keep = [s.clone() for s in srcs]
    got = encode_from(hip, C4, srcs, fmt)
    assert got == c4_want
    assert all(torch.equal(s, k) for s, k in zip(srcs, keep))         # the sources are never written


def test_c4_clips_against_the_oracle(oracle, hip, c4_clips, c4_want):
    got = encode_from(hip, C4, [on_device(elements(pcm, S16, 16)) for pcm in c4_clips], S16)
    for i, pcm in enumerate(c4_clips):
        ret, want = oracle.encode_whole(C4, pcm)
        assert ret == 0 and got[i] == (OK, want) == c4_want[i], i


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_padded_batch_tensor_with_lengths(hip, c4_clips, c4_want, fmt, layout):
    import torch
    lengths = [pcm.shape[1] for pcm in c4_clips]
    L, B = max(lengths) + 100, len(c4_clips)
    dtype = {S32_LEFT: torch.int32, S32: torch.int32, S16: torch.int16, F32: torch.float32}[fmt]
    x = torch.full((B, 2, L) if layout == "planar" else (B, L, 2), 7, dtype=dtype)      # padding that must not be read
    for b, pcm in enumerate(c4_clips):
        e = torch.from_numpy(elements(pcm, fmt, 16))
        if layout == "planar":
            x[b, :, :lengths[b]] = e
        else:
            x[b, :lengths[b], :] = e.t()
    enc = GB.make_encoder(hip, C4)
    try:
        got = enc.encode_batch_tensor(x.cuda(), lengths=lengths, layout=layout, right_justify=(fmt == S32))
    finally:
        enc.close()
    assert got == c4_want


@pytest.mark.parametrize("fmt", [S32_LEFT, S32, F32], ids=["s32_left", "s32", "f32"])
@pytest.mark.parametrize("layout", ["planar", "interleaved", "every_other"])
def test_eight_channel_24_bit_short_files(hip, fmt, layout):
    lens = [20000, 3000, 8193, 1, 0, 12288]
    pcms = [S.synth_pcm(8, max(n, 1), 24, 96000, seed=60 + i)[:, :n] for i, n in enumerate(lens)]
    got = encode_from(hip, OCTO24, [on_device(elements(pcm, fmt, 24), layout) for pcm in pcms], fmt)
    want = reference(hip, OCTO24, pcms)
    assert all(rc == OK for rc, _ in want)
    assert got == want


# ------------------------------------------------------------------ round trips through the device decode

@pytest.mark.parametrize("dtype_name,rj", [("float32", False), ("int16", False), ("int32", False), ("int32", True)],
                         ids=["f32", "s16", "s32_left", "s32"])
def test_round_trip_through_decode_batch_tensor(hip, dtype_name, rj):
    import torch
    pcms = [S.synth_pcm(2, 30000, 16, 48000, seed=5),
            np.zeros((2, 9000), np.int32),                                   # silence
            (S.synth_pcm(2, 20001, 16, 48000, seed=6) >> 17) << 17,          # all samples even: offset_lshift 1
            np.zeros((2, 0), np.int32),                                      # empty
            S.synth_pcm(2, 4097, 16, 48000, seed=7)]
    want = reference(hip, C4, pcms)
    assert all(rc == OK for rc, _ in want)
    datas = [d for _, d in want]
    dec = hip.Decoder(2, 4096, 16, 1, 8)
    enc = GB.make_encoder(hip, C4)
    try:
        if dtype_name == "float32":
            assert enc.encode_batch_tensor(*dec.decode_batch_tensor(datas)[:2]) == want
        for layout in ("planar", "interleaved"):
            t, lengths, results = dec.decode_batch_tensor(datas, dtype=getattr(torch, dtype_name), layout=layout, right_justify=rj)
            assert results == [OK] * len(datas)
            assert enc.encode_batch_tensor(t, lengths, layout=layout, right_justify=rj) == want, layout
    finally:
        dec.close(); enc.close()


# ------------------------------------------------------------------ what only the samples can refuse

def crafted_floats(bps):
    u = 2.0 ** -(bps - 1)                                   # one step of the grid
    f = np.float32
    vals = [0.0, -0.0, u, -3 * u, 0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, -2.5 * u, 1000.5 * u, -1001.5 * u,
            1 - u, 1 - u / 2, 1.0, -1.0, -1 - u / 2, -1 - u, float(np.nextafter(f(1), f(2))), 1.5, -1.5, 3.0e38, -3.0e38,
            np.inf, -np.inf, 1e-40, -1e-40, 1e-45, float(np.finfo(f).tiny), 0.25, -0.75]
    return np.array(vals, np.float32)


@pytest.mark.parametrize("bps", [16, 24])
def test_f32_quantiser_on_crafted_floats(hip, bps):
    p = MONO16 if bps == 16 else MONO24
    rng = np.random.default_rng(bps)
    base = crafted_floats(bps)
    music = elements(S.synth_pcm(1, 6000, bps, 48000, seed=bps), F32, bps)[0]
    a = np.concatenate([np.tile(base, 40), music])[None, :]
    b = np.concatenate([music, rng.permutation(np.tile(base, 25))])[None, :]
    nan = a.copy()
    nan[0, 1234] = np.nan
    files = [a, nan, b, music[None, :]]
    lefts = [left(x, F32, bps) for x in files]
    assert lefts[1] is None
    got = encode_from(hip, p, [on_device(x) for x in files], F32)
    want = reference(hip, p, lefts)
    assert [rc for rc, _ in got] == [OK, INVALID_ARGUMENT, OK, OK]
    assert got == want
    # the quantiser's grid: ties go to even, +-1 and beyond saturate
    q = lefts[0][0, :len(base)].astype(np.int64) >> (32 - bps)
    top = 1 << (bps - 1)
    assert list(q[:12]) == [0, 0, 1, -3, 0, 2, 2, 0, -2, -2, 1000, -1002]
    assert list(q[12:18]) == [top - 1, top - 1, top - 1, -top, -top, -top]
    assert list(q[23:25]) == [top - 1, -top]


@pytest.mark.parametrize("bps", [16, 24])
def test_s32_range(hip, bps):
    p = MONO16 if bps == 16 else MONO24
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    base = elements(S.synth_pcm(1, 5000, bps, 48000, seed=3), S32, bps)
    a = base.copy(); a[0, 100] = lo; a[0, 200] = hi               # the ends of the range: accepted
    b = base.copy(); b[0, 300] = hi + 1                           # 2^(bps-1): refused
    c = base.copy(); c[0, 4999] = lo - 1                          # refused
    files = [a, b, c, base]
    got = encode_from(hip, p, [on_device(x) for x in files], S32)
    assert [rc for rc, _ in got] == [OK, INVALID_ARGUMENT, INVALID_ARGUMENT, OK]
    assert got == reference(hip, p, [left(x, S32, bps) for x in files])


def test_s16_low_bits_on_an_8_bit_format(hip):
    p = S.make_params(1, 8, 48000, 4, 1, 4, 0, 1, 16384)
    good = elements(S.synth_pcm(1, 7000, 8, 48000, seed=4), S16, 16)          # the int16's low 8 bits are zero
    bad = good.copy()
    bad[0, 10] |= 1
    got = encode_from(hip, p, [on_device(good), on_device(bad)], S16)
    want = reference(hip, p, [left(good, S16, 8), left(bad, S16, 8)])
    assert [rc for rc, _ in want] == [OK, INVALID_ARGUMENT]
    assert got == want


# ------------------------------------------------------------------ argument refusals

def test_argument_refusals_are_per_item(hip):
    import torch
    L = hip.lib()
    n = 20000
    pcm = S.synth_pcm(2, n, 16, 48000, seed=11)
    good = on_device(pcm)
    keep = good.clone()
    host = np.ascontiguousarray(pcm)
    pinned = torch.from_numpy(pcm).pin_memory()
    K = 11
    bufs = [np.full(8 * 2 * n + 65536, 0xA5, np.uint8) for _ in range(K)]
    items = (hip.EncodeDeviceItem * K)()
    for i in range(K):
        items[i].src = good.data_ptr()
        items[i].channel_stride = good.stride(0)
        items[i].sample_stride = 1
        items[i].num_samples = n
        items[i].data = bufs[i].ctypes.data_as(hip.u8p)
        items[i].data_size = len(bufs[i])
        items[i].output_size = 12345
        items[i].result = -7
    items[1].src = host.ctypes.data                      # a numpy address
    items[2].src = pinned.data_ptr()                     # page-locked host memory
    items[3].src = good.data_ptr() + 2                   # not aligned to the 4-byte element
    items[4].sample_stride = 1 << 30                     # a region far past the end of its allocation
    items[5].sample_stride = 0
    items[6].channel_stride = 0                          # on a stereo handle
    items[7].data = None
    items[8].data_size = 10                              # too small for the header
    items[9].src = None                                  # NULL src with samples
    enc = GB.make_encoder(hip, C4)
    try:
        st = torch.cuda.current_stream().cuda_stream
        assert L.sla_hip_encode_batch_device(C.c_void_p(enc._h), items, K, S32_LEFT, C.c_void_p(st)) == 0
        want = reference(hip, C4, [pcm])[0]
        for i in (0, 10):
            assert (items[i].result, bufs[i][:items[i].output_size].tobytes()) == want, i
        for i in (1, 2, 3, 4, 5, 6, 7, 9):
            assert items[i].result == INVALID_ARGUMENT and items[i].output_size == 0, i
        assert items[8].result == BUF and items[8].output_size == 0
        for i in range(1, 10):
            assert (bufs[i] == 0xA5).all(), i
        assert torch.equal(good, keep)
        # the Python layer refuses mismatches before the library is called
        with pytest.raises(ValueError):
            enc.encode_batch_from([good], S16)                                   # dtype
        with pytest.raises(ValueError):
            enc.encode_batch_from([torch.from_numpy(host)], S32_LEFT)            # host tensor
        with pytest.raises(ValueError):
            enc.encode_batch_from([good[:1]], S32_LEFT)                          # too few rows
        with pytest.raises(ValueError):
            enc.encode_batch_from([host], S32_LEFT)                              # not a tensor
        with pytest.raises(ValueError):
            enc.encode_batch_from([good], 4)                                     # format
        with pytest.raises(ValueError):
            enc.encode_batch_tensor(good)                                        # not [B][C][L]
        with pytest.raises(ValueError):
            enc.encode_batch_tensor(good[None], lengths=[n + 1])                 # longer than L
    finally:
        enc.close()


def test_call_level_refusals_touch_no_item(hip):
    L = hip.lib()
    x = on_device(S.synth_pcm(2, 5000, 16, 48000, seed=12))
    items = (hip.EncodeDeviceItem * 2)()
    for i in range(2):
        items[i].src = x.data_ptr(); items[i].channel_stride = 5000; items[i].sample_stride = 1; items[i].num_samples = 5000
        items[i].output_size = 777; items[i].result = -7
    items[1].num_samples = (1 << 28) - 1023                    # above the pass cap
    enc = GB.make_encoder(hip, C4)
    raw = hip.Encoder()
    try:
        assert L.sla_hip_encode_batch_device(C.c_void_p(enc._h), items, 2, S16, None) == CAPACITY
        assert L.sla_hip_encode_batch_device(C.c_void_p(enc._h), items, 2, 4, None) == INVALID_ARGUMENT
        assert L.sla_hip_encode_batch_device(C.c_void_p(enc._h), None, 2, S16, None) == INVALID_ARGUMENT
        assert L.sla_hip_encode_batch_device(C.c_void_p(raw._h), items, 1, S32_LEFT, None) == NOT_SET
        assert all(it.result == -7 and it.output_size == 777 for it in items)
    finally:
        enc.close(); raw.close()


# ------------------------------------------------------------------ ordering, reuse, scale, empty

def test_waits_for_work_queued_on_the_callers_stream(hip, c4_clips, c4_want):
    import torch
    lengths = [pcm.shape[1] for pcm in c4_clips]
    real = torch.zeros((len(c4_clips), 2, max(lengths)), dtype=torch.int16)
    for b, pcm in enumerate(c4_clips):
        real[b, :, :lengths[b]] = torch.from_numpy(elements(pcm, S16, 16))
    real = real.cuda()
    x = torch.zeros_like(real)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)                    # the fills below start well after the call has begun
        for k in range(3):
            x.fill_(k + 1)
        x.copy_(real)
    enc = GB.make_encoder(hip, C4)
    try:
        got = enc.encode_batch_from([x[b][:, :lengths[b]] for b in range(len(lengths))], S16, stream=side)
    finally:
        enc.close()
    assert got == c4_want


def test_handle_reuse_across_device_whole_and_host_batch(hip, c4_clips, c4_want):
    srcs = [on_device(elements(pcm, S16, 16)) for pcm in c4_clips[:4]]
    fresh = GB.make_encoder(hip, C4)
    try:
        whole = fresh.encode_whole(c4_clips[1])
    finally:
        fresh.close()
    enc = GB.make_encoder(hip, C4)
    try:
        assert enc.encode_batch_from(srcs, S16) == c4_want[:4]
        assert enc.encode_whole(c4_clips[1]) == whole
        assert enc.encode_batch(c4_clips[:4]) == c4_want[:4]
        assert enc.encode_batch_from(srcs, S16) == c4_want[:4]
    finally:
        enc.close()


def test_600_mono_clips_cross_the_pass_cap(hip):
    import torch
    p = S.make_params(1, 16, 48000, 16, 1, 8, 0, 1, 4096, cap=(1, 4096, 16, 1, 8))
    n = 480000
    bases = [S.synth_pcm(1, n, 16, 48000, seed=900 + k) for k in range(4)]
    lengths = [n - (i * 37) % 2000 for i in range(600)]
    assert sum((m + 1023) // 1024 * 1024 for m in lengths) > (1 << 28)          # two passes
    b16 = torch.from_numpy(np.stack([elements(b, S16, 16)[0] for b in bases])).cuda()
    x = b16[torch.tensor([i % 4 for i in range(600)], device="cuda")].unsqueeze(1)   # int16 [600][1][n] on the device
    enc = GB.make_encoder(hip, p)
    try:
        got = enc.encode_batch_tensor(x, lengths=lengths)
    finally:
        enc.close()
    del x, b16
    want = reference(hip, p, [bases[i % 4][:, :lengths[i]] for i in range(600)])
    assert [rc for rc, _ in got] == [OK] * 600
    assert got == want


def test_empty_call(hip):
    import torch
    L = hip.lib()
    enc = GB.make_encoder(hip, C4)
    try:
        assert enc.encode_batch_from([], F32) == []
        assert enc.encode_batch_tensor(torch.empty((0, 2, 0), dtype=torch.float32, device="cuda")) == []
        assert L.sla_hip_encode_batch_device(C.c_void_p(enc._h), None, 0, F32, None) == 0
        # a batch of empty files only: 43-byte headers
        got = enc.encode_batch_tensor(torch.empty((3, 2, 0), dtype=torch.int16, device="cuda"))
        assert got == reference(hip, C4, [np.zeros((2, 0), np.int32)] * 3)
        assert all(len(d) == 43 for _, d in got)
    finally:
        enc.close()
