"""GPU tests of sla_hip_encode_batch_resident and sla_hip_pack_resident (Encoder.encode_resident_from /
encode_resident_tensor / pack_resident; run with -m gpu on an MI355X): device tensors encoded to .sla streams that stay in
device memory, in the items' own buffers or back to back in an arena.

The reference for every item is Encoder.encode_batch_from on a second handle of the same settings (host delivery of the same
sources).  Every destination is pre-filled with a per-byte pattern and compared as a whole, so a byte written outside a
file shows.  Covered: clip lengths around the tile and block sizes in every format and both modes; two offset_lshift groups
in one pass and the arena order they give; capacities in both modes; the argument refusals; round trips through
decode_resident_tensor; option verify; pack_resident; ordering behind the caller's stream; handle reuse; the empty call."""
import ctypes as C

import numpy as np
import pytest

import slalibs as S
import test_gpu_batch as GB
import test_gpu_encode_batch_device as ED
from test_gpu_encode_batch_device import C4, FMT_IDS, FORMATS, MONO24, OCTO24, F32, S16, S32, S32_LEFT, elements, on_device

pytestmark = pytest.mark.gpu

OK, NG, INVALID_ARGUMENT, BUF = 0, 1, 2, 4
MONO16_8 = S.make_params(1, 16, 48000, 8, 1, 4, 0, 1, 4096)              # mono 16-bit, PARCOR order 8
LENGTHS = [0, 1, 2047, 2048, 4096 + 17, 20000]
NONE = 2 ** 64 - 1


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def canary(n):
    """a per-byte pattern on the device and its host copy"""
    import torch
    a = ((np.arange(n, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8)
    return torch.from_numpy(a).cuda(), a


def clips(p, lengths, seed):
    nch, bps = p.num_channels, p.bits_per_sample
    return [S.synth_pcm(nch, max(n, 1), bps, p.sampling_rate, seed=seed + i)[:, :n] for i, n in enumerate(lengths)]


def odd_slices(buf, caps):
    """slices of buf of the given capacities at odd offsets, at least three bytes apart; (slices, offsets)"""
    outs, offs, pos = [], [], 1
    for cap in caps:
        pos |= 1
        outs.append(buf[pos:pos + cap]); offs.append(pos)
        pos += cap + 3
    assert pos <= buf.numel()
    return outs, offs


def check_per_buffer(hip, enc, srcs, fmt, want, slack=7):
    caps = [len(d) + (slack if i % 2 else 0) for i, (_, d) in enumerate(want)]      # exact fits and roomy ones
    buf, pat = canary(sum(caps) + 8 * len(caps) + 16)
    outs, offs = odd_slices(buf, caps)
    got = enc.encode_resident_from(srcs, fmt, outs=outs)
    expect = pat.copy()
    for (rc, d), o in zip(want, offs):
        expect[o:o + len(d)] = np.frombuffer(d, np.uint8)
    assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == want
    assert np.array_equal(buf.cpu().numpy(), expect)                 # the files, and nothing between or behind them
    for (rc, v), o in zip(got, offs):
        assert v.numel() == 0 or v.data_ptr() == buf.data_ptr() + o


def check_arena(hip, enc, srcs, fmt, want, extra=100):
    total = sum(len(d) for _, d in want)
    arena, pat = canary(total + extra)
    got = enc.encode_resident_from(srcs, fmt, arena=arena)
    assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == want
    spans = sorted((v.data_ptr() - arena.data_ptr(), v.numel()) for _, v in got if v.numel() > 0)
    pos = 0
    for o, n in spans:                                                # back to back from 0, no overlap, no padding
        assert o == pos
        pos += n
    assert pos == total
    assert np.array_equal(arena.cpu().numpy()[total:], pat[total:])  # nothing behind `used`
    return got


# ------------------------------------------------------------------ clip lengths x formats x modes

@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("p", [MONO16_8, C4], ids=["mono16", "c4"])
def test_clip_lengths_every_format_both_modes(hip, p, fmt):
    pcms = clips(p, LENGTHS, 300)
    srcs = [on_device(elements(pcm, fmt, p.bits_per_sample)) for pcm in pcms]
    want = ED.encode_from(hip, p, srcs, fmt)
    assert [rc for rc, _ in want] == [OK] * len(pcms) and len(want[0][1]) == 43      # the empty file: its header
    enc = GB.make_encoder(hip, p)
    try:
        check_per_buffer(hip, enc, srcs, fmt, want)
        check_arena(hip, enc, srcs, fmt, want)
    finally:
        enc.close()


def test_two_offset_lshift_groups_in_one_pass(hip):
    p = MONO24
    pcms = clips(p, [9000, 7001, 5000], 320)
    pcms[1] = (pcms[1] >> 16) << 16                                  # the low 8 of its 24 bits are zero: offset_lshift 8
    srcs = [on_device(pcm) for pcm in pcms]
    want = ED.encode_from(hip, p, srcs, S32_LEFT)
    assert [rc for rc, _ in want] == [OK] * 3
    assert [hip.decode_header(d)[1].wave_format.offset_lshift for _, d in want] == [0, 8, 0]
    enc = GB.make_encoder(hip, p)
    try:
        check_per_buffer(hip, enc, srcs, S32_LEFT, want)
        arena, _ = canary(sum(len(d) for _, d in want) + 50)
        got = enc.encode_resident_from(srcs, S32_LEFT, arena=arena)
        assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == want
        s = [len(d) for _, d in want]
        offs = [v.data_ptr() - arena.data_ptr() for _, v in got]
        assert offs == [0, s[0] + s[2], s[0]]                        # the group of file 0 (files 0 and 2), then file 1's
        check_arena(hip, enc, srcs, S32_LEFT, want)
    finally:
        enc.close()


# ------------------------------------------------------------------ capacities

def test_capacity_per_buffer(hip):
    pcms = clips(C4, [6000, 5000, 4097, 3000], 330)
    srcs = [on_device(elements(pcm, S16, 16)) for pcm in pcms]
    full = ED.encode_from(hip, C4, srcs, S16)
    caps = [len(full[0][1]), 42, len(full[2][1]) - 1, len(full[3][1]) + 5]
    want = ED.encode_from(hip, C4, srcs, S16, capacities=caps)       # the host call with the same room
    assert [rc for rc, _ in want] == [OK, BUF, BUF, OK]
    buf, pat = canary(sum(caps) + 64)
    outs, offs = odd_slices(buf, caps)
    enc = GB.make_encoder(hip, C4)
    try:
        got = enc.encode_resident_from(srcs, S16, outs=outs)
    finally:
        enc.close()
    assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == want
    expect = pat.copy()
    for i in (0, 3):
        expect[offs[i]:offs[i] + len(want[i][1])] = np.frombuffer(want[i][1], np.uint8)
    assert np.array_equal(buf.cpu().numpy(), expect)                 # the refused buffers are untouched


def raw_items(hip, enc, srcs, fmt):
    items = enc._device_items(srcs, fmt)
    for it in items:
        it.output_size = 777; it.result = -7
    return items


def test_capacity_arena(hip):
    import torch
    pcms = clips(C4, [6000, 5000, 4097, 0], 340)
    srcs = [on_device(elements(pcm, S16, 16)) for pcm in pcms]
    want = ED.encode_from(hip, C4, srcs, S16)
    s = [len(d) for _, d in want]
    assert s[3] == 43 and s[2] - 1 >= 43
    room = s[0] + s[1] + s[2] - 1                                    # one byte short for file 2; the empty file 3 still fits
    arena, pat = canary(room + 20)
    enc = GB.make_encoder(hip, C4)
    try:
        items = raw_items(hip, enc, srcs, S16)
        for it in items:
            it.data = C.cast(C.c_void_p(0x1234), hip.u8p); it.data_size = 1        # ignored on input
        st = torch.cuda.current_stream().cuda_stream
        assert hip.lib().sla_hip_encode_batch_resident(C.c_void_p(enc._h), items, 4, S16, C.c_void_p(arena.data_ptr()), room,
                                                       C.c_void_p(st)) == 0
    finally:
        enc.close()
    base = arena.data_ptr()
    where = [C.cast(it.data, C.c_void_p).value for it in items]
    assert [it.result for it in items] == [OK, OK, BUF, OK]
    assert [it.output_size for it in items] == [s[0], s[1], 0, 43]
    assert where == [base, base + s[0], None, base + s[0] + s[1]]
    used = s[0] + s[1] + 43
    got = arena.cpu().numpy()
    assert got[:used].tobytes() == want[0][1] + want[1][1] + want[3][1]
    assert np.array_equal(got[used:], pat[used:])


@pytest.mark.parametrize("verify", [0, 1])
def test_capacity_arena_single_file_too_small(hip, verify):
    """a group of one file without room is that file's result, not the call's: the call returns 0, nothing is written"""
    import torch
    pcm = clips(C4, [6000], 345)[0]
    src = on_device(elements(pcm, S16, 16))
    want = ED.encode_from(hip, C4, [src], S16)[0]
    enc = GB.make_encoder(hip, C4)
    try:
        enc.set_option("verify", verify)
        for room in (len(want[1]) - 1, 42, 0):
            arena, pat = canary(len(want[1]) + 20)
            items = raw_items(hip, enc, [src], S16)
            st = torch.cuda.current_stream().cuda_stream
            assert hip.lib().sla_hip_encode_batch_resident(C.c_void_p(enc._h), items, 1, S16, C.c_void_p(arena.data_ptr()), room,
                                                           C.c_void_p(st)) == 0
            assert (items[0].result, items[0].output_size, C.cast(items[0].data, C.c_void_p).value) == (BUF, 0, None), room
            assert np.array_equal(arena.cpu().numpy(), pat)
            assert enc.last_verify()[0] == 0                          # a file that is not delivered is not verified
        # the Python layer reports it per file too, and the handle goes on working
        x = src[None]
        a, offsets, sizes, results = enc.encode_resident_tensor(x, capacity=len(want[1]) - 1)
        assert (a.numel(), offsets, sizes, results) == (0, [0], [0], [BUF])
        a, offsets, sizes, results = enc.encode_resident_tensor(x, capacity=len(want[1]))
        assert (a.cpu().numpy().tobytes(), offsets, sizes, results) == (want[1], [0], [len(want[1])], [OK])
    finally:
        enc.close()


def test_capacity_arena_singleton_group_does_not_fit(hip):
    """two offset_lshift groups, the second one a single file the arena has no room for: the first group's files are
    delivered and reported, the singleton gets INSUFFICIENT_BUFFER_SIZE, and the groups behind it are still tried"""
    p = MONO24
    pcms = clips(p, [9000, 7001, 5000], 325)
    pcms[1] = (pcms[1] >> 16) << 16                                  # offset_lshift 8: a group of its own
    srcs = [on_device(pcm) for pcm in pcms]
    want = ED.encode_from(hip, p, srcs, S32_LEFT)
    s = [len(d) for _, d in want]
    assert [rc for rc, _ in want] == [OK] * 3
    enc = GB.make_encoder(hip, p)
    try:
        arena, pat = canary(s[0] + s[2] + 30)
        got = enc.encode_resident_from(srcs, S32_LEFT, arena=arena[:s[0] + s[2]])
        assert [rc for rc, _ in got] == [OK, BUF, OK] and got[1][1].numel() == 0
        assert [v.data_ptr() - arena.data_ptr() for _, v in got if v.numel()] == [0, s[0]]
        host = arena.cpu().numpy()
        assert host[:s[0] + s[2]].tobytes() == want[0][1] + want[2][1]
        assert np.array_equal(host[s[0] + s[2]:], pat[s[0] + s[2]:])
        # the singleton group first, and room for nothing but an empty file's header: that file is still placed, at 0
        order = [srcs[1], srcs[0], srcs[2][:, :0]]
        arena, pat = canary(43 + 30)
        got = enc.encode_resident_from(order, S32_LEFT, arena=arena[:43])
        assert [rc for rc, _ in got] == [BUF, BUF, OK]
        assert got[2][1].data_ptr() == arena.data_ptr() and got[2][1].numel() == 43
        assert got[2][1].cpu().numpy().tobytes() == ED.encode_from(hip, p, [srcs[2][:, :0]], S32_LEFT)[0][1]
        assert np.array_equal(arena.cpu().numpy()[43:], pat[43:])
    finally:
        enc.close()


# ------------------------------------------------------------------ refusals

def test_refusals(hip):
    import torch
    pcm = clips(C4, [5000], 350)[0]
    src = on_device(pcm)
    want = ED.encode_from(hip, C4, [src], S32_LEFT)[0]
    host = np.full(70000, 0xA5, np.uint8)
    buf, pat = canary(3 * 70000)
    enc = GB.make_encoder(hip, C4)
    try:
        L, st = hip.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        items = raw_items(hip, enc, [src] * 5, S32_LEFT)
        for i in range(5):
            items[i].data = C.cast(C.c_void_p(buf.data_ptr() + 1 + i * 35000), hip.u8p); items[i].data_size = 34000
        items[1].data = host.ctypes.data_as(hip.u8p)                 # host memory
        items[2].data_size = 0xFFFFFFFF                              # a range far past the end of its allocation
        items[3].data = None
        assert L.sla_hip_encode_batch_resident(C.c_void_p(enc._h), items, 5, S32_LEFT, None, 0, st) == 0
        assert [it.result for it in items] == [OK, INVALID_ARGUMENT, INVALID_ARGUMENT, INVALID_ARGUMENT, OK]
        assert [it.output_size for it in items] == [len(want[1]), 0, 0, 0, len(want[1])]
        expect = pat.copy()
        for i in (0, 4):
            expect[1 + i * 35000:1 + i * 35000 + len(want[1])] = np.frombuffer(want[1], np.uint8)
        assert np.array_equal(buf.cpu().numpy(), expect) and (host == 0xA5).all()
        # an arena in host memory, or reaching past its allocation: the call is refused and no item touched
        items = raw_items(hip, enc, [src] * 2, S32_LEFT)
        assert L.sla_hip_encode_batch_resident(C.c_void_p(enc._h), items, 2, S32_LEFT, host.ctypes.data_as(C.c_void_p), len(host),
                                               st) == INVALID_ARGUMENT
        assert L.sla_hip_encode_batch_resident(C.c_void_p(enc._h), items, 2, S32_LEFT, C.c_void_p(buf.data_ptr()), 1 << 40,
                                               st) == INVALID_ARGUMENT
        assert all(it.result == -7 and it.output_size == 777 for it in items)
        assert np.array_equal(buf.cpu().numpy(), expect) and (host == 0xA5).all()
        # the Python layer: exactly one of outs and arena, device tensors of bytes
        with pytest.raises(ValueError):
            enc.encode_resident_from([src], S32_LEFT)
        with pytest.raises(ValueError):
            enc.encode_resident_from([src], S32_LEFT, outs=[buf[:40000]], arena=buf)
        with pytest.raises(ValueError):
            enc.encode_resident_from([src], S32_LEFT, outs=[torch.from_numpy(host)])
        with pytest.raises(ValueError):
            enc.encode_resident_from([src], S32_LEFT, arena=buf[::2])
    finally:
        enc.close()


# ------------------------------------------------------------------ the closed loop on the device

@pytest.mark.parametrize("p,dtype_name,rj", [(C4, "int16", False), (C4, "float32", False), (OCTO24, "int32", False),
                                              (OCTO24, "int32", True), (OCTO24, "float32", False)],
                         ids=["c4_s16", "c4_f32", "octo24_s32_left", "octo24_s32", "octo24_f32"])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_round_trip_on_the_device(hip, p, dtype_name, rj, layout):
    import torch
    nch, bps = p.num_channels, p.bits_per_sample
    lengths = [9000, 0, 4097, 12288 + 5]
    fmt = {"int16": S16, "float32": F32, "int32": S32 if rj else S32_LEFT}[dtype_name]
    L, B = max(lengths) + 33, len(lengths)
    x = torch.zeros((B, nch, L), dtype=getattr(torch, dtype_name))
    for b, pcm in enumerate(clips(p, lengths, 360)):
        x[b, :, :lengths[b]] = torch.from_numpy(elements(pcm, fmt, bps))
    padded = x.clone()                                                # (x, zero behind every length, is what must come back)
    for b in range(B):
        padded[b, :, lengths[b]:] = 7                                 # padding that must not be read
    dev_in = (padded if layout == "planar" else padded.transpose(1, 2).contiguous()).cuda()
    enc = GB.make_encoder(hip, p)
    dec = hip.Decoder()
    try:
        a, offsets, sizes, results = enc.encode_resident_tensor(dev_in, lengths=lengths, layout=layout, right_justify=rj)
        assert results == [OK] * B and a.numel() == sum(sizes) and a.is_cuda
        assert offsets == [sum(sizes[:b]) for b in range(B)]          # one offset_lshift, one pass: item order
        back, lens, res = dec.decode_resident_tensor([a[o:o + s] for o, s in zip(offsets, sizes)], dtype=getattr(torch, dtype_name),
                                                     layout=layout, length=L, right_justify=rj)
    finally:
        enc.close(); dec.close()
    assert res == [OK] * B and lens == lengths
    back = back.cpu() if layout == "planar" else back.cpu().transpose(1, 2)
    assert torch.equal(back, x)


# ------------------------------------------------------------------ option verify, pack_resident

def test_verify_gives_the_same_bytes_and_counters(hip):
    pcms = clips(C4, [20000, 0, 4097, 6000], 370)
    srcs = [on_device(elements(pcm, S16, 16)) for pcm in pcms]
    want = ED.encode_from(hip, C4, srcs, S16)
    ref = GB.make_encoder(hip, C4)
    enc = GB.make_encoder(hip, C4)
    try:
        ref.set_option("verify", 1); enc.set_option("verify", 1)
        assert ref.encode_batch_from(srcs, S16) == want
        counters = ref.last_verify()
        assert counters[0] == 2 * sum(pcm.shape[1] for pcm in pcms) and counters[1] == 0 and counters[4] == 0
        check_per_buffer(hip, enc, srcs, S16, want)
        assert enc.last_verify() == counters
        check_arena(hip, enc, srcs, S16, want)
        assert enc.last_verify() == counters
        # an arena too small for file 0: the host call with that room does not verify it either
        s = [len(d) for _, d in want]
        arena, _ = canary(s[0] - 1)
        got = enc.encode_resident_from(srcs, S16, arena=arena)
        codes, room = [], s[0] - 1
        for size in s:                                               # the documented cursor
            codes.append(OK if size <= room else BUF)
            room -= size if size <= room else 0
        assert [rc for rc, _ in got] == codes and codes[0] == BUF and codes[1] == OK
        assert enc.last_verify()[0] == 2 * sum(pcm.shape[1] for pcm, rc in zip(pcms, codes) if rc == OK)
    finally:
        ref.close(); enc.close()


@pytest.mark.parametrize("verify", [0, 1])
def test_pack_resident(hip, verify):
    import torch
    p, n = C4, 3 * 4096 + 17
    pcm = clips(p, [n], 380)[0]
    d = on_device(pcm)
    enc = GB.make_encoder(hip, p)
    try:
        enc.set_option("verify", verify)
        enc.analyze_device(d.data_ptr(), n, n)
        want = enc.pack(8 * 2 * n + 65536, on_device=True)
        counters = enc.last_verify()
        enc.analyze_device(d.data_ptr(), n, n)
        buf, pat = canary(len(want) + 40)
        got = enc.pack_resident(buf[3:3 + len(want)])                # an exact fit at an odd address
        assert got.data_ptr() == buf.data_ptr() + 3 and got.cpu().numpy().tobytes() == want
        expect = pat.copy(); expect[3:3 + len(want)] = np.frombuffer(want, np.uint8)
        assert np.array_equal(buf.cpu().numpy(), expect)
        assert enc.last_verify() == counters
        nb = enc.trace(want_residuals=False).num_blocks
        assert enc.verify_last_image(d.data_ptr(), n) == (2 * n, 0, NONE, nb, 0)
        # one byte short, too small for a header, host memory: the code, and nothing written
        L, size = hip.lib(), C.c_uint32(55)
        assert L.sla_hip_pack_resident(C.c_void_p(enc._h), C.c_void_p(buf.data_ptr() + 3), len(want) - 1, C.byref(size)) == BUF
        assert L.sla_hip_pack_resident(C.c_void_p(enc._h), C.c_void_p(buf.data_ptr() + 3), 42, C.byref(size)) == BUF
        host = np.zeros(len(want), np.uint8)
        assert L.sla_hip_pack_resident(C.c_void_p(enc._h), host.ctypes.data_as(C.c_void_p), len(host), C.byref(size)) == INVALID_ARGUMENT
        assert size.value == 55 and not host.any() and np.array_equal(buf.cpu().numpy(), expect)
        with pytest.raises(ValueError):
            enc.pack_resident(torch.from_numpy(host))
    finally:
        enc.close()


# ------------------------------------------------------------------ ordering, reuse, empty

def test_waits_for_work_queued_on_the_callers_stream(hip):
    import torch
    pcms = clips(C4, [20000, 4097, 6000], 390)
    srcs = [on_device(elements(pcm, S16, 16)) for pcm in pcms]
    want = ED.encode_from(hip, C4, srcs, S16)
    total = sum(len(d) for _, d in want)
    arena = torch.full((total + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    enc = GB.make_encoder(hip, C4)
    try:
        with torch.cuda.stream(side):
            torch.cuda._sleep(50_000_000)                  # the zeroing below starts well after the call has begun
            arena.zero_()
        got = enc.encode_resident_from(srcs, S16, arena=arena, stream=side)
    finally:
        enc.close()
    torch.cuda.synchronize()
    assert [(rc, v.cpu().numpy().tobytes()) for rc, v in got] == want
    assert arena.cpu().numpy()[:total].tobytes() == b"".join(d for _, d in want) and not arena[total:].any()


def test_handle_reuse_resident_and_host_batches_alternate(hip):
    pcms = clips(C4, [20000, 4097, 2047, 6000], 400)
    srcs = [on_device(elements(pcm, S16, 16)) for pcm in pcms]
    want = ED.encode_from(hip, C4, srcs, S16)
    enc = GB.make_encoder(hip, C4)
    try:
        check_arena(hip, enc, srcs, S16, want)
        assert enc.encode_batch_from(srcs, S16) == want
        check_per_buffer(hip, enc, srcs[:2], S16, want[:2])
        assert enc.encode_batch(pcms) == want
        assert enc.encode_whole(pcms[0]) == want[0][1]
        check_arena(hip, enc, srcs[::-1], S16, want[::-1])
    finally:
        enc.close()


def test_empty_call(hip):
    import torch
    enc = GB.make_encoder(hip, C4)
    try:
        arena, pat = canary(64)
        assert enc.encode_resident_from([], F32, arena=arena) == []
        assert enc.encode_resident_from([], F32, outs=[]) == []
        assert hip.lib().sla_hip_encode_batch_resident(C.c_void_p(enc._h), None, 0, F32, None, 0, None) == 0
        a, offsets, sizes, results = enc.encode_resident_tensor(torch.empty((0, 2, 0), dtype=torch.float32, device="cuda"))
        assert (a.numel(), offsets, sizes, results) == (0, [], [], [])
        assert np.array_equal(arena.cpu().numpy(), pat)
    finally:
        enc.close()
