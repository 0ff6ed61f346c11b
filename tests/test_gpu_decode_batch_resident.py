"""GPU tests of sla_hip_decode_batch_resident (Decoder.decode_resident_into / decode_resident_tensor; run with -m gpu on
an MI355X): many .sla files whose bytes are in device memory decoded into caller-owned device tensors.

The reference for every item is Decoder.decode_batch_into of the same bytes in host memory on a second handle of the
same configuration, into destinations prepared the same way: the resident call must give the same result code, the same
sample count and the same bits of every destination, the sentinel or zero tail included.  Covered: every format in
planar and interleaved layouts on a ragged batch of short clips; mixed formats over several passes; the crafted-stream
catalogue with the CRC check on and off; damaged files between good ones, one that needs a resync among them; sources
as slices of one tensor at odd offsets and as separate allocations; the per-item source refusals; a source shorter than
its header; ordering behind work queued on the caller's stream; handle reuse; the padded-tensor call; the empty call.
Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

import crafted_catalogue as CC
import slalibs as S
import test_gpu_decode_batch as TB
import test_gpu_decode_batch_device as TD

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, BUF, DATA = 0, 2, 4, 9
S32_LEFT, S32, S16, F32 = range(4)
FORMATS, FMT_IDS = TD.FORMATS, TD.FMT_IDS


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def resident(datas, packed=True, lead=1):
    """the files in device memory: slices of one uint8 tensor at odd offsets (packed), or one allocation each.  An empty
    file is a (pointer, 0) pair: an empty tensor has no pointer.  -> (sources, what keeps them alive)"""
    import torch
    keep = [torch.from_numpy(np.frombuffer(bytes(d) or b"\0", np.uint8).copy()).cuda() for d in datas]
    if packed:
        # put together on the device, from one small upload per file
        offs, parts, pos = [], [], 0
        for t, d in zip(keep, datas):
            gap = lead if pos == 0 else (1 if pos % 2 == 0 else 2)       # every file starts at an odd offset
            parts += [torch.full((gap,), 0xEE, dtype=torch.uint8, device="cuda"), t[:len(d)]]
            offs.append(pos + gap)
            pos += gap + len(d)
        base = torch.cat(parts + [torch.full((16,), 0xEE, dtype=torch.uint8, device="cuda")])
        return [base[o:o + len(d)] if len(d) else (base.data_ptr() + o, 0) for d, o in zip(datas, offs)], base
    return [t if len(d) else (t.data_ptr(), 0) for t, d in zip(keep, datas)], keep


def outputs(datas, caps, fmt, layout):
    outs = []
    for data, cap in zip(datas, caps):
        nch = max(TD.header(data)[0], 1)
        outs.append(TD.alloc((nch, cap), fmt) if layout == "planar" else TD.alloc((cap, nch), fmt).t())
    return outs


def run_both(ref, dec, datas, caps, fmt, layout, zero_fill=True, packed=True):
    """the resident call against decode_batch_into of the same bytes in host memory: codes, counts, every bit"""
    srcs, keep = resident(datas, packed)
    want_outs, got_outs = outputs(datas, caps, fmt, layout), outputs(datas, caps, fmt, layout)
    want = ref.decode_batch_into(datas, want_outs, fmt, zero_fill=zero_fill)
    got = dec.decode_resident_into(srcs, got_outs, fmt, zero_fill=zero_fill)
    assert got == want
    for i, (a, b) in enumerate(zip(got_outs, want_outs)):
        assert np.array_equal(TD.bits_of(a.cpu().numpy()), TD.bits_of(b.cpu().numpy())), ("item", i, got[i])
    return got


@pytest.fixture(scope="module")
def clips(hip):
    """ten short stereo clips of the C4 shape, 1 to 8 blocks, ragged"""
    lens = [6000, 9001, 12345, 16384, 20000, 24577, 30000, 8193, 4096, 3000]
    pcms = [S.synth_pcm(2, n, 16, 48000, seed=900 + i) for i, n in enumerate(lens)]
    return TB.encode_clips(hip, TB.C4, pcms), lens, pcms


@pytest.fixture(scope="module")
def mixed(oracle):
    return TD._mixed_set(oracle)


@pytest.fixture(scope="module")
def damaged(oracle, hip):
    entries = TB._damaged_set(oracle, hip)
    good = [e for e in entries if e[0].startswith("good")]
    order = []
    for j, e in enumerate(e for e in entries if not e[0].startswith("good")):
        order += [good[j % len(good)], e]
    order.append(good[0])
    return order


# ------------------------------------------------------------------ formats, layouts, passes

@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_short_clips_every_format_and_layout(hip, clips, fmt, layout):
    datas, lens, pcms = clips
    caps = [n + 100 for n in lens]
    dec, ref = TD.pair(hip)
    try:
        got = run_both(ref, dec, datas, caps, fmt, layout)
        assert got == [(OK, n) for n in lens]
        t = dec.last_timing()
        assert t[5] == 1 and t[0] > 0 and t[1] > 0 and t[2] > 0 and t[3] > 0      # one pass: gather, walks, kernels, emit
        # the samples are the clips' (the reference call is itself checked against decode_batch elsewhere)
        if fmt == S32_LEFT and layout == "planar":
            srcs, keep = resident(datas)
            outs = outputs(datas, lens, fmt, layout)
            dec.decode_resident_into(srcs, outs, fmt)
            for o, pcm in zip(outs, pcms):
                assert np.array_equal(o.cpu().numpy(), pcm)
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_mixed_formats_take_several_passes(hip, mixed, fmt):
    datas = mixed
    caps = [int.from_bytes(bytes(d[15:19]), "big") + 17 * (i % 3) for i, d in enumerate(datas)]
    dec, ref = TD.pair(hip, CC.CAP)
    try:
        got = run_both(ref, dec, datas, caps, fmt, "planar")
        assert dec.last_timing()[5] >= 4 and dec.last_timing()[5] == ref.last_timing()[5]
        assert all(rc == OK for rc, _ in got)
        run_both(ref, dec, datas, [max(c - 40, 0) for c in caps], fmt, "interleaved", zero_fill=False)
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("crc", [1, 0])
@pytest.mark.parametrize("fmt", [S32_LEFT, F32], ids=["s32_left", "f32"])
def test_crafted_catalogue(hip, crc, fmt):
    cases = CC.catalogue()
    assert len(cases) == 52
    dec, ref = TD.pair(hip, CC.CAP, crc)
    try:
        got = run_both(ref, dec, [c.data for c in cases], [c.num_samples for c in cases], fmt, "planar")
        assert all(rc == OK for rc, _ in got)
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("crc", [1, 0])
@pytest.mark.parametrize("zero_fill", [True, False])
def test_damaged_files_between_good_ones(hip, damaged, crc, zero_fill):
    names = [e[0] for e in damaged]
    assert "size field disagrees" in names and "buffer too small" in names and "empty stream" in names
    datas, caps = [e[1] for e in damaged], [e[2] for e in damaged]
    for fmt in (S32_LEFT, F32):
        dec, ref = TD.pair(hip, crc=crc)
        try:
            got = run_both(ref, dec, datas, caps, fmt, "planar", zero_fill=zero_fill)
        finally:
            dec.close(); ref.close()
        codes = {n: rc for n, (rc, _) in zip(names, got)}
        assert codes["buffer too small"] == BUF and codes["no samples"] == OK and codes["empty stream"] == DATA


def test_slices_of_one_tensor_and_separate_allocations(hip, clips, damaged):
    datas = clips[0][:4] + [e[1] for e in damaged[:8]]
    caps = [n + 5 for n in clips[1][:4]] + [e[2] for e in damaged[:8]]
    dec, ref = TD.pair(hip)
    try:
        a = run_both(ref, dec, datas, caps, S16, "planar", packed=True)
        b = run_both(ref, dec, datas, caps, S16, "planar", packed=False)
        assert a == b
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ refusals

def test_source_refusals_are_per_item(hip, clips):
    import torch
    L = hip.lib()
    data, n = clips[0][2], clips[1][2]
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    dsrc = torch.from_numpy(buf).cuda()
    pinned = C.c_void_p()                                  # page-locked host memory of the test's own, freed below
    assert L.hipHostMalloc(C.byref(pinned), C.c_size_t(len(buf)), C.c_uint(0)) == 0
    C.memmove(pinned.value, buf.ctypes.data, len(buf))
    outs = [TD.alloc((2, n + 8), F32) for _ in range(7)]
    dec, ref = TD.pair(hip)
    try:
        items = (hip.DecodeDeviceItem * 7)()
        for i in range(7):
            items[i].data = C.cast(C.c_void_p(dsrc.data_ptr()), hip.u8p)
            items[i].data_size = len(buf)
            items[i].dst = outs[i].data_ptr()
            items[i].channel_stride = n + 8
            items[i].sample_stride = 1
            items[i].capacity = n
            items[i].output_num_samples = 12345
        items[1].data = None                                               # NULL source
        items[2].data = buf.ctypes.data_as(hip.u8p)                        # a host pointer
        items[3].data = C.cast(pinned, hip.u8p)                            # a page-locked host pointer
        items[4].data_size = 0xF0000000                                    # runs past its allocation
        items[5].dst = None                                                # a destination refusal of the device call
        st = torch.cuda.current_stream().cuda_stream
        assert L.sla_hip_decode_batch_resident(C.c_void_p(dec._h), items, 7, F32, hip.DEC_ZERO_FILL, C.c_void_p(st)) == 0
        torch.cuda.synchronize()
        want = TD.alloc((2, n + 8), F32)
        assert ref.decode_batch_into([data], [want[:, :n]], F32) == [(OK, n)]
        for i in (0, 6):
            assert items[i].result == OK and items[i].output_num_samples == n
            assert np.array_equal(TD.bits_of(outs[i].cpu().numpy()), TD.bits_of(want.cpu().numpy())), i
        for i in (1, 2, 3, 4, 5):
            assert items[i].result == INVALID_ARGUMENT and items[i].output_num_samples == 0, i
        for i in (1, 2, 3, 4):
            assert (TD.bits_of(outs[i].cpu().numpy()) == TD.SENTINEL).all(), i
        # sla_hip_resident_headers refuses the same sources, and tells the others' headers
        heads = dec.resident_headers([(dsrc.data_ptr(), len(buf)), (0, len(buf)), (buf.ctypes.data, len(buf)),
                                      (pinned.value, len(buf)), (dsrc.data_ptr(), 0xF0000000), (dsrc.data_ptr(), 20)])
        assert [rc for rc, _ in heads] == [OK, INVALID_ARGUMENT, INVALID_ARGUMENT, INVALID_ARGUMENT, INVALID_ARGUMENT, DATA]
        assert heads[0][1].num_samples == n and heads[0][1].wave_format.num_channels == 2
        # the Python layer refuses mismatches before the library is called
        with pytest.raises(ValueError):
            dec.decode_resident_into([dsrc], [TD.alloc((2, n), S16)], F32)                       # dtype
        with pytest.raises(ValueError):
            dec.decode_resident_into([dsrc], [TD.alloc((1, n), F32)], F32)                       # too few rows
        with pytest.raises(ValueError):
            dec.decode_resident_into([torch.from_numpy(buf)], [TD.alloc((2, n), F32)], F32)      # a host tensor
        with pytest.raises(ValueError):
            dec.decode_resident_into([dsrc[:2 * (len(buf) // 2)].view(torch.int16)], [TD.alloc((2, n), F32)], F32)     # not bytes
        with pytest.raises(ValueError):
            dec.decode_resident_into([dsrc, dsrc], [TD.alloc((2, n), F32)], F32)                 # count
    finally:
        dec.close(); ref.close()
        L.hipHostFree.argtypes = [C.c_void_p]
        assert L.hipHostFree(pinned) == 0


def test_a_source_shorter_than_its_header(hip, clips):
    datas = [clips[0][0], clips[0][1][:20], clips[0][1][:42], clips[0][1][:43], clips[0][1][:53], clips[0][3]]
    caps = [clips[1][0], 100, 100, 100, 100, clips[1][3]]
    dec, ref = TD.pair(hip)
    try:
        got = run_both(ref, dec, datas, caps, F32, "planar")
        assert [rc for rc, _ in got] == [OK, DATA, DATA, DATA, DATA, OK]
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ ordering, reuse, the padded tensor, empty

def test_waits_for_work_queued_on_the_callers_stream(hip, clips):
    """the sources are written by a copy queued on the caller's stream behind a long sleep: the call reads them after it"""
    import torch
    datas, lens, pcms = clips
    srcs, base = resident(datas)
    good = base.clone()
    dec, _ = TD.pair(hip)
    try:
        side = torch.cuda.Stream()
        outs = outputs(datas, lens, F32, "planar")
        base.fill_(0xFF)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(50_000_000)                  # the copy below starts well after the call has begun
            base.copy_(good)
        got = dec.decode_resident_into(srcs, outs, F32, stream=side)
        side.synchronize()
        assert got == [(OK, n) for n in lens]
        for o, pcm in zip(outs, pcms):
            assert np.array_equal(TD.bits_of(o.cpu().numpy()), TD.bits_of(TD.convert(pcm, F32, 16)))
    finally:
        dec.close()


def test_handle_reuse_alternating_resident_and_host_calls(oracle, hip, clips):
    files = TB._mixed_files(oracle)
    datas = [d for d, _ in files] + clips[0][:3]
    caps = [pcm.shape[1] for _, pcm in files] + clips[1][:3]
    dec, ref = TD.pair(hip)
    try:
        first = run_both(ref, dec, datas, caps, S32_LEFT, "planar")
        TD.run_layout(hip, ref, dec, datas, caps, F32, "interleaved")          # the host-bytes call on the same handle
        rw, ow = dec.decode_whole(datas[1], caps[1])
        assert rw == OK and np.array_equal(ow, files[1][1])
        again = run_both(ref, dec, datas[::-1], caps[::-1], S32_LEFT, "interleaved")
        assert again == first[::-1]
        host = dec.decode_batch(datas, caps)
        assert [(rc, o.shape[1]) for rc, o in host] == first
        assert run_both(ref, dec, datas, caps, S32, "planar", zero_fill=False) == first
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_resident_tensor_against_batch_tensor(oracle, hip, clips, layout):
    import torch
    files = TB._mixed_files(oracle)
    datas = clips[0][:4] + [d for d, _ in files] + [b"", b"SL*\x01 not a header" + bytes(40)]
    dec, ref = TD.pair(hip)
    try:
        for dtype, rj, length in ((torch.float32, False, None), (torch.int16, False, 7000), (torch.int32, True, None)):
            srcs, keep = resident(datas)
            want, wl, wr = ref.decode_batch_tensor(datas, dtype=dtype, layout=layout, length=length, right_justify=rj)
            got, gl, gr = dec.decode_resident_tensor(srcs, dtype=dtype, layout=layout, length=length, right_justify=rj)
            assert (gl, gr) == (wl, wr) and got.shape == want.shape and got.dtype == want.dtype
            assert np.array_equal(TD.bits_of(got.cpu().numpy()), TD.bits_of(want.cpu().numpy())), (dtype, rj, length)
    finally:
        dec.close(); ref.close()


def test_empty_call(hip):
    import torch
    dec, _ = TD.pair(hip)
    try:
        assert dec.decode_resident_into([], [], F32) == []
        assert dec.resident_headers([]) == []
        t, lengths, results = dec.decode_resident_tensor([])
        assert tuple(t.shape) == (0, 0, 0) and lengths == [] and results == []
        L = hip.lib()
        assert L.sla_hip_decode_batch_resident(C.c_void_p(dec._h), None, 0, F32, 0, None) == 0
        assert dec.last_timing() == [0.0] * 6
    finally:
        dec.close()


# ------------------------------------------------------------------ one pipeline behind every route

def _every_route(dec, datas, caps):
    """the batch through the host-source, the resident and the window route of ONE handle, windows being the whole clips
    -> per route (results, the bits of every destination, passes)"""
    srcs, keep = resident(datas)
    routes = []
    for route in ("host", "resident", "windows"):
        outs = [TD.alloc((2, cap), S32_LEFT) for cap in caps]
        if route == "host":
            got = dec.decode_batch_into(datas, outs, S32_LEFT)
        elif route == "resident":
            got = dec.decode_resident_into(srcs, outs, S32_LEFT)
        else:
            got = [g[:2] for g in dec.decode_windows_into(srcs, [0] * len(datas), outs, S32_LEFT)]
        routes.append((got, [TD.bits_of(o.cpu().numpy()) for o in outs], dec.last_timing()[5]))
    return routes, srcs, keep


def _same_on_every_route(routes):
    (want, want_bits, want_passes), others = routes[0], routes[1:]
    for got, bits, passes in others:
        assert got == want and passes == want_passes
        for i, (a, b) in enumerate(zip(bits, want_bits)):
            assert a.shape == b.shape and np.array_equal(a, b), ("item", i)
    return want, want_bits, want_passes


def test_same_samples_on_every_route_and_handle_reuse_across_routes(hip):
    """six short ragged clips in two formats (two passes), one with a header whose CRC fails (zero fill alone) and one whose
    destination is refused (an empty tensor has no pointer): the host-source, the resident and the window route, windows
    being the whole clips, deliver every item whole, refused or zero-filled -- the same bytes, codes and pass count on each.
    The handle then takes a smaller batch through each route, and one intact clip through the salvage call."""
    import torch
    other = S.make_params(2, 16, 48000, 8, 1, 8, 1, 1, 4096, cap=(2, 4096, 16, 1, 8))       # PARCOR order 8: another launch key
    lens = [2048, 5000, 9001, 12345, 16385, 20000]
    pcms = [S.synth_pcm(2, n, 16, 48000, seed=950 + i) for i, n in enumerate(lens)]
    even, odd = TB.encode_clips(hip, TB.C4, pcms[0::2]), TB.encode_clips(hip, other, pcms[1::2])
    datas = [bytearray((even if i % 2 == 0 else odd)[i // 2]) for i in range(6)]
    datas[1][20] ^= 0x04                                       # a header field changed, its CRC not: the fields are still delivered
    datas = [bytes(d) for d in datas]
    caps = list(lens)
    caps[4] = 0                                                # no destination at all: refused before anything is read
    dec = TB.make_decoder(hip)
    try:
        routes, srcs, keep = _every_route(dec, datas, caps)
        got, bits, passes = _same_on_every_route(routes)
        assert got == [(OK, 2048), (11, 0), (OK, 9001), (OK, 12345), (INVALID_ARGUMENT, 0), (OK, 20000)]
        assert passes == 2
        for i in (0, 2, 3, 5):
            assert np.array_equal(bits[i], pcms[i])
        assert bits[1].shape == (2, 5000) and not bits[1].any()
        # the same handle, a smaller batch: scratch and tables cut for the larger one
        small = [5, 0, 3]
        routes2, srcs2, keep2 = _every_route(dec, [datas[i] for i in small], [lens[i] for i in small])
        got2, bits2, passes2 = _same_on_every_route(routes2)
        assert got2 == [(OK, lens[i]) for i in small] and passes2 == 2
        for k, i in enumerate(small):
            assert np.array_equal(bits2[k], pcms[i])
        # and an intact clip through the salvage call of that handle
        t, rep, ranges = dec.salvage_resident_tensor(srcs[2], dtype=torch.int32)
        assert rep["result"] == OK and rep["mode"] == 1 and ranges == []
        assert np.array_equal(t.cpu().numpy(), bits[2])
    finally:
        dec.close()
