"""GPU tests of sla_hip_decode_windows_resident (Decoder.decode_windows_into / decode_windows_tensor /
block_index_resident; run with -m gpu on an MI355X): sample windows of .sla streams whose bytes are in device memory
decoded into caller-owned device tensors.

The reference for every window is a slice: Decoder.decode_resident_into of the same bytes on a second handle, in the same
format and layout, and [start, start + length) of it, clipped to the file.  The window must give the same bits, the
sentinel or zero tail included.  On encoder-made clips the samples are also compared with the source PCM.  What windows
do differently on purpose is tested as such: damage in a block the window does not need is not seen, damage in a needed
block fails the whole window, a hint skips the chain in front of it.  sla_hip_decoder_last_window_stats is held against
tests/windowmodel.py, which shows that only the window's blocks went through the kernels.
Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest

import crafted_catalogue as CC
import slalibs as S
import test_gpu_decode_batch as TB
import test_gpu_decode_batch_device as TD
import test_gpu_decode_batch_resident as TR
import walkmodel as WM
import windowmodel as WN

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, DATA, CORRUPT, SYNC_LOST = 0, 2, 9, 11, 12
S32_LEFT, S32, S16, F32 = range(4)
FORMATS, FMT_IDS = TD.FORMATS, TD.FMT_IDS
ALIGN = 64                       # DEC_BATCH_ALIGN: every item's plane region starts on a multiple of it


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def total_of(data):
    return WM.header_total(data) if len(data) >= 19 else 0


def blocks_of(data, cap_n=16384):
    """(byte_off, smp_off, num_samples) of every block of a clean file, from the model of the whole-file walk"""
    t = total_of(data)
    return [(r[0], r[2], r[3]) for r in WM.walk(data, t, t, cap_n).rows]


def win_out(nch, length, fmt, layout):
    """a sentinel-filled destination [nch][length]; a window of no samples still gets a pointer"""
    nch = max(nch, 1)
    if layout == "planar":
        return TD.alloc((nch, max(length, 1)), fmt)[:, :length]
    return TD.alloc((max(length, 1), nch), fmt)[:length].t()


def whole_files(ref, datas, srcs, fmt, layout):
    """[(result, samples, bits [nch][total])] of the whole-file resident decode on the second handle"""
    caps = [total_of(d) + 3 for d in datas]
    outs = TR.outputs(datas, caps, fmt, layout)
    got = ref.decode_resident_into(srcs, outs, fmt)
    return [(rc, n, TD.bits_of(o.cpu().numpy())) for (rc, n), o in zip(got, outs)]


def run_windows(dec, datas, srcs, wins, fmt, layout, zero_fill=True, hints=None):
    """wins: [(file, start, length)] -> (what the call returned, the destinations)"""
    outs = [win_out(TD.header(datas[i])[0], l, fmt, layout) for i, _, l in wins]
    got = dec.decode_windows_into([srcs[i] for i, _, _ in wins], [s for _, s, _ in wins], outs, fmt, zero_fill=zero_fill, hints=hints)
    return got, outs


def check_slices(datas, whole, wins, got, outs, fmt, zero_fill=True):
    """every window of a file whose whole decode is OK with all samples: code, count, the slice's bits, the tail, the
    rows past the header's channels"""
    checked = 0
    for w, (i, s, l) in enumerate(wins):
        rc, n, bits = whole[i]
        t = total_of(datas[i])
        if (rc, n) != (OK, t):
            continue
        nch = TD.header(datas[i])[0]
        o = TD.bits_of(outs[w].cpu().numpy())
        if s > t:
            assert got[w][:2] == (INVALID_ARGUMENT, 0), (w, i, s, l, got[w])
            assert (o == TD.sentinel_bits(fmt)).all(), (w, i, s, l)
            continue
        want_n = min(l, t - s)
        assert got[w][:2] == (OK, want_n), (w, i, s, l, got[w])
        assert np.array_equal(o[:nch, :want_n], bits[:nch, s:s + want_n]), (w, i, s, l)
        tail = o[:nch, want_n:]
        assert (tail == 0).all() if zero_fill else (tail == TD.sentinel_bits(fmt)).all(), (w, i, s, l, "tail")
        assert (o[nch:] == TD.sentinel_bits(fmt)).all(), (w, i, s, l, "rows past the header's channels")
        checked += 1
    return checked


def clip_windows(datas):
    wins = []
    for i, d in enumerate(datas):
        t = total_of(d)
        bl = blocks_of(d)
        wins += [(i, 0, t), (i, 0, 1), (i, t - 1, 1), (i, t - 100, 500), (i, t, 10), (i, t + 1, 10), (i, 5, 0), (i, t, 0)]
        wins += [(i, pos, n) for _, pos, n in bl]                                   # each block exactly
        wins += [(i, pos - 1, 2) for _, pos, _ in bl[1:]]                           # each boundary straddled by 2 samples
    return wins


@pytest.fixture(scope="module")
def clips(hip):
    """the ten ragged stereo clips of test_gpu_decode_batch_resident.py: 3000 to 30000 samples, 1 to 8 blocks"""
    lens = [6000, 9001, 12345, 16384, 20000, 24577, 30000, 8193, 4096, 3000]
    pcms = [S.synth_pcm(2, n, 16, 48000, seed=900 + i) for i, n in enumerate(lens)]
    datas = TB.encode_clips(hip, TB.C4, pcms)
    assert sorted({len(blocks_of(d)) for d in datas})[0] == 1 and max(len(blocks_of(d)) for d in datas) == 8
    return datas, lens, pcms


@pytest.fixture(scope="module")
def mixed(oracle):
    return TD._mixed_set(oracle)


# ------------------------------------------------------------------ formats, layouts, passes

@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_clip_windows_every_format_and_layout(hip, clips, fmt, layout):
    datas, lens, pcms = clips
    wins = clip_windows(datas)
    srcs, keep = TR.resident(datas)
    dec, ref = TD.pair(hip)
    try:
        whole = whole_files(ref, datas, srcs, fmt, layout)
        assert [(rc, n) for rc, n, _ in whole] == [(OK, n) for n in lens]
        got, outs = run_windows(dec, datas, srcs, wins, fmt, layout)
        assert check_slices(datas, whole, wins, got, outs, fmt) == len(wins) - len(datas)      # all but the start > total ones
        t = dec.last_timing()
        assert t[5] == 1 and t[0] > 0 and t[1] > 0 and t[2] > 0 and t[3] > 0      # one pass: gathers, walks, kernels, emit
        # without the zero fill the tails keep the sentinel
        some = wins[:24]
        got, outs = run_windows(dec, datas, srcs, some, fmt, layout, zero_fill=False)
        assert check_slices(datas, whole, some, got, outs, fmt, zero_fill=False) >= len(some) - 2
        if fmt == S32_LEFT and layout == "planar":
            got, outs = run_windows(dec, datas, srcs, wins, fmt, layout)
            for (i, s, l), (rc, n, _), o in zip(wins, got, outs):
                if rc == OK:
                    assert np.array_equal(o.cpu().numpy()[:, :n], pcms[i][:, s:s + n]), (i, s, l)
    finally:
        dec.close(); ref.close()


def test_overlapping_windows_of_one_source_in_one_call(hip, clips):
    datas, lens, pcms = clips
    srcs, keep = TR.resident(datas[6:7])
    wins = [(0, 4000, 5000), (0, 4000, 5000), (0, 4001, 4999), (0, 0, 30000), (0, 8191, 2), (0, 29999, 1), (0, 12000, 1)]
    dec, ref = TD.pair(hip)
    try:
        got, outs = run_windows(dec, datas[6:7], srcs, wins, S32_LEFT, "planar")
        for (_, s, l), (rc, n, _), o in zip(wins, got, outs):
            assert (rc, n) == (OK, l) and np.array_equal(o.cpu().numpy(), pcms[6][:, s:s + l]), (s, l)
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("fmt", [S32, F32], ids=["s32", "f32"])
def test_mixed_formats_take_several_passes(hip, mixed, fmt):
    datas = mixed
    wins = []
    for i, d in enumerate(datas):
        t = total_of(d)
        wins += [(i, 0, t), (i, t // 3, t // 2), (i, t // 2 + 1, t), (i, max(t - 7, 0), 7)]
        wins += [(i, pos - 1, 2) for _, pos, _ in blocks_of(d)[1:3]]
    srcs, keep = TR.resident(datas)
    dec, ref = TD.pair(hip, CC.CAP)
    try:
        whole = whole_files(ref, datas, srcs, fmt, "planar")
        assert all((rc, n) == (OK, total_of(d)) for (rc, n, _), d in zip(whole, datas))
        got, outs = run_windows(dec, datas, srcs, wins, fmt, "planar")
        assert check_slices(datas, whole, wins, got, outs, fmt) == len(wins)
        assert dec.last_timing()[5] >= 4 and dec.last_timing()[5] == ref.last_timing()[5]
        got, outs = run_windows(dec, datas, srcs, wins[::3], fmt, "interleaved", zero_fill=False)
        whole = whole_files(ref, datas, srcs, fmt, "interleaved")
        assert check_slices(datas, whole, wins[::3], got, outs, fmt, zero_fill=False) == len(wins[::3])
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("fmt,layout", [(S32_LEFT, "planar"), (F32, "interleaved")], ids=["s32_left-planar", "f32-interleaved"])
def test_crafted_catalogue(hip, fmt, layout):
    cases = CC.catalogue()
    assert len(cases) == 52
    datas = [c.data for c in cases]
    wins = []
    for i, d in enumerate(datas):
        t = total_of(d)
        wins += [(i, 0, t), (i, 1, max(t - 2, 0)), (i, t // 2, t), (i, t, 4)]
        wins += [(i, max(pos - 1, 0), 2) for _, pos, n in blocks_of(d) if n]
    srcs, keep = TR.resident(datas)
    dec, ref = TD.pair(hip, CC.CAP)
    try:
        whole = whole_files(ref, datas, srcs, fmt, layout)
        served = [(rc, n) == (OK, c.num_samples) for (rc, n, _), c in zip(whole, cases)]
        assert sum(served) >= 40                                   # a window equals the slice wherever the whole decode gives all
        got, outs = run_windows(dec, datas, srcs, wins, fmt, layout)
        assert check_slices(datas, whole, wins, got, outs, fmt) == sum(1 for i, _, _ in wins if served[i])
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ damage

def _flip(data, at, mask=0x10):
    d = bytearray(data)
    d[at] ^= mask
    return bytes(d)


def test_damage_is_seen_only_where_the_window_needs_the_bytes(hip, clips):
    datas, lens, pcms = clips
    data, pcm = datas[6], pcms[6]
    bl = blocks_of(data)
    assert len(bl) == 8
    body = _flip(data, bl[1][0] + 40)                             # a body bit of block 1
    nosync = _flip(data, bl[2][0], 0x01)                          # block 2 has lost its sync code
    cut = data[:bl[5][0] + 30]                                    # the file ends inside block 5
    files = [data, body, nosync, cut]
    srcs, keep = TR.resident(files)
    b3, b4, b5 = bl[3][1], bl[4][1], bl[5][1]
    wins = [(1, b3 + 10, 3000),                                   # the flipped bit lies in front of the window
            (1, bl[1][1] + 10, 3000),                             # ... in a block the window needs
            (1, 0, bl[1][1]),                                     # ... behind the window
            (2, b4 + 5, 2000),                                    # the lost sync lies in front of the window
            (2, 100, bl[1][1]),                                   # ... behind the window's end
            (3, 100, b4),                                         # the cut lies behind the window
            (3, b4 + 100, 6000)]                                  # the window runs across the cut
    dec, ref = TD.pair(hip)
    try:
        got, outs = run_windows(dec, files, srcs, wins, S32_LEFT, "planar")
        codes = [g[:2] for g in got]
        assert codes == [(OK, 3000), (CORRUPT, 0), (OK, bl[1][1]), (SYNC_LOST, 0), (OK, bl[1][1]), (OK, b4), (DATA, 0)]
        for (i, s, l), (rc, n, _), o in zip(wins, got, outs):
            o = o.cpu().numpy()
            assert np.array_equal(o[:, :n], pcm[:, s:s + n]) and (o[:, n:] == 0).all(), (i, s, l)
        # the same windows without the zero fill: a failed window writes nothing
        got, outs = run_windows(dec, files, srcs, wins, S32_LEFT, "planar", zero_fill=False)
        assert [g[:2] for g in got] == codes
        for (rc, n, _), o in zip(got, outs):
            assert (o.cpu().numpy()[:, n:] == TD.SENTINEL).all()
        # a hint behind the lost sync serves the window
        got, outs = run_windows(dec, files, srcs, [(2, b4 + 5, 2000)], S32_LEFT, "planar", hints=[(bl[3][0], bl[3][1])])
        assert got[0] == (OK, 2000, (bl[4][0], bl[4][1]))
        assert np.array_equal(outs[0].cpu().numpy(), pcm[:, b4 + 5:b4 + 2005])
        assert dec.last_window_stats()[:2] == (1, 1)
        assert b5 > b4
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ hints, the index, the counters

def test_hints_fed_back_and_the_block_index(hip, clips):
    import torch
    datas, lens, pcms = clips
    srcs, keep = TR.resident(datas)
    rng = np.random.default_rng(5)
    wins = [(i, int(rng.integers(0, n - 1000)), 1000) for i, n in enumerate(lens) for _ in range(3)]
    dec, ref = TD.pair(hip)
    try:
        first, outs1 = run_windows(dec, datas, srcs, wins, F32, "planar")
        skipped = dec.last_window_stats()[0]
        assert skipped > 0 and all(rc == OK for rc, _, _ in first)
        again, outs2 = run_windows(dec, datas, srcs, wins, F32, "planar", hints=[h for _, _, h in first])
        assert again == first and dec.last_window_stats()[0] == 0
        for a, b in zip(outs1, outs2):
            assert torch.equal(a, b)
        # the index: every block of every file, as the model of the whole-file walk has them
        index = dec.block_index_resident(srcs)
        for d, (byte_off, smp_off, stop) in zip(datas, index):
            bl = blocks_of(d)
            assert stop == OK and list(byte_off) == [b[0] for b in bl] and list(smp_off) == [b[1] for b in bl]
        starts = [s for _, s, _ in wins]
        plain, n1, r1 = dec.decode_windows_tensor([srcs[i] for i, _, _ in wins], starts, 1000)
        assert dec.last_window_stats()[0] == skipped
        hinted, n2, r2 = dec.decode_windows_tensor([srcs[i] for i, _, _ in wins], starts, 1000, index=[index[i] for i, _, _ in wins])
        assert dec.last_window_stats()[0] == 0 and (n1, r1) == (n2, r2) == ([1000] * len(wins), [OK] * len(wins))
        assert torch.equal(plain, hinted)
        for k, (i, s, _) in enumerate(wins):
            assert np.array_equal(TD.bits_of(plain[k].cpu().numpy()), TD.bits_of(TD.convert(pcms[i][:, s:s + 1000], F32, 16)))
        # the hints the call refuses, per item: nothing of the item is written
        bl = blocks_of(datas[6])
        hints = [(10, 0), (42, 0), (0, 5), (bl[2][0], 8193), None, (bl[1][0], bl[1][1])]
        got, outs = run_windows(dec, datas, srcs, [(6, 8192, 100)] * 6, F32, "planar", hints=hints)
        assert [g[:2] for g in got] == [(INVALID_ARGUMENT, 0)] * 4 + [(OK, 100)] * 2
        for o in outs[:4]:
            assert (TD.bits_of(o.cpu().numpy()) == TD.SENTINEL).all()
        assert torch.equal(outs[4], outs[5])
    finally:
        dec.close(); ref.close()


def test_window_stats_are_what_the_model_predicts(hip, clips):
    datas, lens, pcms = clips
    srcs, keep = TR.resident(datas)
    wins = [w for w in clip_windows(datas) if w[2] > 0 and w[1] < total_of(datas[w[0]])]
    bl6 = blocks_of(datas[6])
    hints = [None] * len(wins) + [(bl6[2][0], bl6[2][1])]
    wins = wins + [(6, 20000, 3000)]
    dec, ref = TD.pair(hip)
    try:
        got, outs = run_windows(dec, datas, srcs, wins, S16, "planar", hints=hints)
        models = [WN.walk(datas[i], total_of(datas[i]), s, l, TB.HANDLE_CAP[1], *(h or (0, 0))) for (i, s, l), h in zip(wins, hints)]
        assert all(m.stop == OK for m in models) and all(g[0] == OK for g in got)
        want = (sum(m.skipped for m in models), sum(m.num_blocks for m in models), sum(m.end_byte - m.first_byte for m in models),
                sum((m.end_sample - m.first_sample + ALIGN - 1) // ALIGN * ALIGN for m in models))
        assert dec.last_window_stats() == want
        assert [g[2] for g in got] == [(m.first_byte, m.first_sample) for m in models]
        # a one-sample window of an eight-block file costs one block, not eight
        got, outs = run_windows(dec, datas, srcs, [(6, 29999, 1)], S16, "planar")
        assert dec.last_window_stats()[:2] == (7, 1) and dec.last_window_stats()[2] == len(datas[6]) - bl6[7][0]
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ sources, destinations, ordering, reuse, empty

def test_separate_allocations_and_the_padded_tensor(hip, clips):
    import torch
    datas, lens, pcms = clips
    wins = clip_windows(datas)[::5]
    dec, ref = TD.pair(hip)
    try:
        srcs, keep = TR.resident(datas, packed=False)
        whole = whole_files(ref, datas, srcs, S16, "interleaved")
        got, outs = run_windows(dec, datas, srcs, wins, S16, "interleaved")
        assert check_slices(datas, whole, wins, got, outs, S16) >= len(wins) - len(datas)
        for layout in ("planar", "interleaved"):
            full, _, _ = ref.decode_resident_tensor(srcs, dtype=torch.float32, layout=layout)
            starts = [n // 2 for n in lens]
            t, ns, rs = dec.decode_windows_tensor(srcs, starts, 2000, layout=layout)
            assert rs == [OK] * 10 and ns == [min(2000, n - s) for n, s in zip(lens, starts)]
            for b, (s, n) in enumerate(zip(starts, ns)):
                a = t[b] if layout == "planar" else t[b].t()
                w = full[b] if layout == "planar" else full[b].t()
                assert torch.equal(a[:, :n], w[:, s:s + n]) and (a[:, n:] == 0).all()
    finally:
        dec.close(); ref.close()


def test_source_and_destination_refusals_are_per_item(hip, clips):
    import torch
    L = hip.lib()
    data, n = clips[0][2], clips[1][2]
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    dsrc = torch.from_numpy(buf).cuda()
    outs = [TD.alloc((2, 508), F32) for _ in range(8)]
    dec, ref = TD.pair(hip)
    try:
        items = (hip.DecodeWindowItem * 8)()
        for i in range(8):
            items[i].data = C.cast(C.c_void_p(dsrc.data_ptr()), hip.u8p)
            items[i].data_size = len(buf)
            items[i].dst = outs[i].data_ptr()
            items[i].channel_stride = 508
            items[i].sample_stride = 1
            items[i].start = 4000
            items[i].length = 500
            items[i].output_num_samples = 12345
        items[1].data = None                                               # NULL source
        items[2].data = buf.ctypes.data_as(hip.u8p)                        # a host pointer
        items[3].data_size = 0xF0000000                                    # runs past its allocation
        items[4].dst = None                                                # NULL destination
        items[5].sample_stride = 0
        items[6].channel_stride = 1 << 62                                  # the region's extent overflows
        st = torch.cuda.current_stream().cuda_stream
        assert L.sla_hip_decode_windows_resident(C.c_void_p(dec._h), items, 8, F32, hip.DEC_ZERO_FILL, C.c_void_p(st)) == 0
        torch.cuda.synchronize()
        want = TD.alloc((2, n), F32)
        assert ref.decode_resident_into([dsrc], [want], F32) == [(OK, n)]
        want = TD.bits_of(want.cpu().numpy())
        for i in (0, 7):
            assert items[i].result == OK and items[i].output_num_samples == 500
            o = TD.bits_of(outs[i].cpu().numpy())
            assert np.array_equal(o[:, :500], want[:, 4000:4500]) and (o[:, 500:] == TD.SENTINEL).all(), i
        for i in range(1, 7):
            assert items[i].result == INVALID_ARGUMENT and items[i].output_num_samples == 0, i
            assert (TD.bits_of(outs[i].cpu().numpy()) == TD.SENTINEL).all(), i
        with pytest.raises(ValueError):
            dec.decode_windows_into([dsrc], [0], [TD.alloc((2, 10), S16)], F32)                  # dtype
        with pytest.raises(ValueError):
            dec.decode_windows_into([dsrc], [0], [TD.alloc((1, 10), F32)], F32)                  # too few rows
        with pytest.raises(ValueError):
            dec.decode_windows_into([dsrc], [0, 1], [TD.alloc((2, 10), F32)], F32)               # count
        with pytest.raises(ValueError):
            dec.decode_windows_into([dsrc], [-1], [TD.alloc((2, 10), F32)], F32)                 # a negative start
    finally:
        dec.close(); ref.close()


def test_waits_for_work_queued_on_the_callers_stream(hip, clips):
    """the sources are written by a copy queued on the caller's stream behind a long sleep: the call reads them after it"""
    import torch
    datas, lens, pcms = clips
    srcs, base = TR.resident(datas)
    good = base.clone()
    dec, _ = TD.pair(hip)
    try:
        side = torch.cuda.Stream()
        starts = [n // 3 for n in lens]
        outs = [win_out(2, 1500, F32, "planar") for _ in datas]
        base.fill_(0xFF)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(50_000_000)                  # the copy below starts well after the call has begun
            base.copy_(good)
        got = dec.decode_windows_into(srcs, starts, outs, F32, stream=side)
        side.synchronize()
        assert [g[:2] for g in got] == [(OK, 1500)] * len(datas)
        for o, pcm, s in zip(outs, pcms, starts):
            assert np.array_equal(TD.bits_of(o.cpu().numpy()), TD.bits_of(TD.convert(pcm[:, s:s + 1500], F32, 16)))
    finally:
        dec.close()


def test_handle_reuse_interleaved_with_the_whole_file_call(hip, clips):
    datas, lens, pcms = clips
    srcs, keep = TR.resident(datas)
    wins = clip_windows(datas)[::7]
    dec, ref = TD.pair(hip)
    try:
        whole = whole_files(ref, datas, srcs, S32_LEFT, "planar")
        for _ in range(2):
            got, outs = run_windows(dec, datas, srcs, wins, S32_LEFT, "planar")
            assert check_slices(datas, whole, wins, got, outs, S32_LEFT) > 0
            mine = whole_files(dec, datas, srcs, S32_LEFT, "planar")             # the whole-file call on the same handle
            assert all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) for a, b in zip(mine, whole))
        rw, ow = dec.decode_whole(datas[1], lens[1])
        assert rw == OK and np.array_equal(ow, pcms[1])
        got, outs = run_windows(dec, datas, srcs, wins[::-1], F32, "interleaved")
        assert check_slices(datas, whole_files(ref, datas, srcs, F32, "interleaved"), wins[::-1], got, outs, F32) > 0
    finally:
        dec.close(); ref.close()


def test_empty_call(hip):
    dec, _ = TD.pair(hip)
    try:
        assert dec.decode_windows_into([], [], [], F32) == []
        t, ns, rs = dec.decode_windows_tensor([], [], 100)
        assert tuple(t.shape) == (0, 0, 100) and ns == [] and rs == []
        assert dec.block_index_resident([]) == []
        L = hip.lib()
        assert L.sla_hip_decode_windows_resident(C.c_void_p(dec._h), None, 0, F32, 0, None) == 0
        assert dec.last_timing() == [0.0] * 6 and dec.last_window_stats() == (0, 0, 0, 0)
    finally:
        dec.close()
