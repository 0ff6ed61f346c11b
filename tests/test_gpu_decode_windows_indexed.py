"""GPU tests of sla_hip_decode_windows_indexed (Index, Decoder.index_resident / decode_windows_indexed_into /
decode_windows_indexed; run with -m gpu on an MI355X): windows of resident .sla streams decoded from block indexes, queued on
the caller's stream with no host wait.

The yardstick is the synchronous call: Decoder.decode_windows_into of the same bytes, windows, format and flags on a second
handle.  Outcomes and every bit of the destinations -- sentinel rows past the header's channels included -- must be equal.
What the queued call does differently on purpose is tested as such: bytes that changed under an old index fail the window
with DETECT_DATA_CORRUPTION, an index of another size refuses its item, and the call returns while the caller's stream is
still busy.  Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest

import crafted_catalogue as CC
import test_gpu_decode_batch_device as TD
import test_gpu_decode_batch_resident as TR
import test_gpu_decode_windows as TW
from test_gpu_decode_windows import clips, hip, mixed          # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, DATA, CORRUPT, SYNC_LOST = 0, 2, 9, 11, 12
S32_LEFT, S32, S16, F32 = range(4)


def make_outs(datas, wins, fmt, layout, guard=1):
    """sentinel-filled destinations [nch][length] as views of [guard + nch + guard][length] tensors -> (views, whole tensors)"""
    views, wholes = [], []
    for i, _, l in wins:
        nch = max(TD.header(datas[i])[0], 1)
        if layout == "planar":
            whole = TD.alloc((nch + 2 * guard, max(l, 1)), fmt)[:, :l]
        else:
            whole = TD.alloc((max(l, 1), nch + 2 * guard), fmt)[:l].t()
        wholes.append(whole)
        views.append(whole[guard:guard + nch])
    return views, wholes


def queued(dec, datas, srcs, idx, wins, fmt, layout, zero_fill=True, stream=None):
    outs, wholes = make_outs(datas, wins, fmt, layout)
    oc = dec.decode_windows_indexed_into([srcs[i] for i, _, _ in wins], [idx[i] for i, _, _ in wins], [s for _, s, _ in wins], outs, fmt,
                                         zero_fill=zero_fill, stream=stream)
    return oc, wholes


def synchronous(ref, datas, srcs, wins, fmt, layout, zero_fill=True):
    outs, wholes = make_outs(datas, wins, fmt, layout)
    got = ref.decode_windows_into([srcs[i] for i, _, _ in wins], [s for _, s, _ in wins], outs, fmt, zero_fill=zero_fill)
    return [g[:2] for g in got], wholes


def same(oc, wholes, want, want_wholes, wins):
    """outcomes and every bit of the destinations, guard rows included, against the synchronous call's"""
    import torch
    torch.cuda.synchronize()
    got = [tuple(int(v) for v in r) for r in oc.cpu().numpy()]
    assert got == want, [(w, g, x) for w, g, x in zip(wins, got, want) if g != x][:5]
    for w, a, b in zip(wins, wholes, want_wholes):
        assert np.array_equal(TD.bits_of(a.cpu().numpy()), TD.bits_of(b.cpu().numpy())), w
    return got


def indexes(hip, datas):
    return [hip.Index.build(d) for d in datas]


# ------------------------------------------------------------------ equality with the synchronous call

@pytest.mark.parametrize("fmt", TD.FORMATS, ids=TD.FMT_IDS)
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_clip_windows_every_format_and_layout(hip, clips, fmt, layout):
    datas, lens, pcms = clips
    wins = TW.clip_windows(datas)
    srcs, keep = TR.resident(datas)
    idx = indexes(hip, datas)
    dec, ref = TD.pair(hip)
    try:
        for zero_fill in (True, False):
            want, want_wholes = synchronous(ref, datas, srcs, wins, fmt, layout, zero_fill)
            oc, wholes = queued(dec, datas, srcs, idx, wins, fmt, layout, zero_fill)
            got = same(oc, wholes, want, want_wholes, wins)
            assert sum(1 for g in got if g[0] == OK and g[1] > 0) >= len(wins) - 4 * len(datas)
            assert sum(1 for g in got if g[0] == INVALID_ARGUMENT) == len(datas)               # start > num_samples
        t = dec.last_timing()
        assert t[4] > 0 and t[:4] == [0.0] * 4 and t[5] == 0.0
        if fmt == S32_LEFT and layout == "planar":
            for (i, s, l), (rc, n), o in zip(wins, got, wholes):
                assert np.array_equal(o.cpu().numpy()[1:3, :n], pcms[i][:, s:s + n]), (i, s, l)
    finally:
        dec.close(); ref.close()


def test_the_same_source_in_many_items(hip, clips):
    datas, lens, pcms = clips
    srcs, keep = TR.resident(datas[6:7])
    idx = indexes(hip, datas[6:7])
    wins = [(0, 4000, 5000), (0, 4000, 5000), (0, 4001, 4999), (0, 0, 30000), (0, 8191, 2), (0, 29999, 1), (0, 12000, 1)] * 3
    dec, ref = TD.pair(hip)
    try:
        want, want_wholes = synchronous(ref, datas[6:7], srcs, wins, F32, "interleaved")
        oc, wholes = queued(dec, datas[6:7], srcs, idx, wins, F32, "interleaved")
        assert same(oc, wholes, want, want_wholes, wins) == [(OK, l) for _, _, l in wins]
    finally:
        dec.close(); ref.close()


@pytest.mark.parametrize("fmt", [S32, F32], ids=["s32", "f32"])
def test_mixed_launch_parameters_in_one_call(hip, mixed, fmt):
    datas = mixed + [b"", mixed[0][:30], b"XL*\x01" + mixed[0][4:]]             # and items that reach no pass
    wins = []
    for i, d in enumerate(datas):
        t = TW.total_of(d) if len(d) >= 43 else 0
        wins += [(i, 0, t), (i, t // 3, t // 2), (i, t // 2 + 1, t), (i, max(t - 7, 0), 7), (i, t, 3)]
        wins += [(i, pos - 1, 2) for _, pos, _ in TW.blocks_of(d)[1:3]] if len(d) >= 43 and d[:2] == b"SL" else []
    srcs, keep = TR.resident(datas)
    idx = indexes(hip, datas)
    dec, ref = TD.pair(hip, CC.CAP)
    try:
        for layout, zero_fill in (("planar", True), ("interleaved", False)):
            want, want_wholes = synchronous(ref, datas, srcs, wins, fmt, layout, zero_fill)
            oc, wholes = queued(dec, datas, srcs, idx, wins, fmt, layout, zero_fill)
            got = same(oc, wholes, want, want_wholes, wins)
            assert len({g[0] for g in got}) >= 3
        assert ref.last_timing()[5] >= 4
    finally:
        dec.close(); ref.close()


def test_separate_allocations_and_the_padded_tensor(hip, clips):
    import torch
    datas, lens, pcms = clips
    wins = TW.clip_windows(datas)[::5]
    dec, ref = TD.pair(hip)
    try:
        srcs, keep = TR.resident(datas, packed=False)
        idx = indexes(hip, datas)
        want, want_wholes = synchronous(ref, datas, srcs, wins, S16, "interleaved")
        oc, wholes = queued(dec, datas, srcs, idx, wins, S16, "interleaved")
        same(oc, wholes, want, want_wholes, wins)
        starts = [n // 2 for n in lens]
        starts[3] = lens[3] + 5                                          # one window refused outright: zeroed by its outcome
        for layout in ("planar", "interleaved"):
            for dtype in (torch.float32, torch.int16):
                t0, ns, rs = ref.decode_windows_tensor(srcs, starts, 2000, dtype=dtype, layout=layout)
                t1, oc = dec.decode_windows_indexed(srcs, idx, starts, 2000, dtype=dtype, layout=layout)
                torch.cuda.synchronize()
                assert t1.shape == t0.shape and torch.equal(t1, t0)
                assert [tuple(int(v) for v in r) for r in oc.cpu().numpy()] == list(zip(rs, ns)) and rs[3] == INVALID_ARGUMENT
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ the index from device bytes, the sidecar

def test_index_resident_is_the_host_index_and_survives_a_sidecar(hip, clips, tmp_path):
    datas, lens, pcms = clips
    datas = list(datas) + [datas[2][:len(datas[2]) // 2], b"", datas[0][:43], b"XL*\x01" + datas[1][4:]]
    srcs, keep = TR.resident(datas)
    host = [hip.Index.build(d).to_bytes() for d in datas]
    dec, ref = TD.pair(hip)
    try:
        assert [x.to_bytes() for x in dec.index_resident(srcs)] == host
        # the wide walk forced on one stream, then an overflow of its nodes that falls back to the lane
        dec.set_option("wide_walk", 1)
        assert dec.index_resident(srcs[6:7])[0].to_bytes() == host[6] and dec.last_walk()[:2] == (1, 0)
        dec.set_option("wide_walk_nodes", 2)
        assert dec.index_resident(srcs[6:7])[0].to_bytes() == host[6] and dec.last_walk()[:2] == (0, 1)
        dec.set_option("wide_walk_nodes", 0)
        assert [x.to_bytes() for x in dec.index_resident(srcs)] == host
        dec.set_option("wide_walk", hip.WIDE_WALK_DEFAULT)
        # a save / load round trip, and windows decoded from what was loaded
        loaded = []
        for k, x in enumerate(dec.index_resident(srcs)):
            path = tmp_path / ("%d.slax" % k)
            path.write_bytes(x.to_bytes())
            loaded.append(hip.Index.from_bytes(path.read_bytes()))
        assert [x.to_bytes() for x in loaded] == host
        wins = TW.clip_windows(datas[:10])[::9] + [(10, 0, 2000), (10, 100, lens[2]), (11, 0, 4), (12, 0, 4), (13, 0, 4)]
        want, want_wholes = synchronous(ref, datas, srcs, wins, F32, "planar")
        oc, wholes = queued(dec, datas, srcs, loaded, wins, F32, "planar")
        got = same(oc, wholes, want, want_wholes, wins)
        assert got[-5][0] == OK and got[-4][0] == DATA                   # the cut file: served in front of the cut, DATA across it
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ damage, stale indexes

def _poke(data, at, value=None, mask=0x10):
    d = bytearray(data)
    d[at] = d[at] ^ mask if value is None else value
    return bytes(d)


@pytest.mark.parametrize("crc", [1, 0])
def test_damage_and_stale_indexes(hip, clips, crc):
    datas, lens, pcms = clips
    data = datas[6]
    bl = TW.blocks_of(data)
    assert len(bl) == 8
    files = [data, _poke(data, bl[1][0] + 40), _poke(data, bl[2][0], 0x7F), _poke(data, bl[2][0] + 5, mask=0x04),
             _poke(data, bl[2][0] + 9, mask=0x01)]
    srcs, keep = TR.resident(files)
    old = [hip.Index.build(data)] * len(files)                        # the index of the bytes as they were
    b1, b2, b3 = bl[1][1], bl[2][1], bl[3][1]
    dec, ref = TD.pair(hip, crc=crc)
    try:
        # a flipped payload byte: the synchronous call's code where the window needs the block, not seen where it does not
        wins = [(1, b1 + 10, 3000), (1, b3 + 10, 3000), (1, 0, b1), (0, b1 + 10, 3000)]
        want, want_wholes = synchronous(ref, files, srcs, wins, S32_LEFT, "planar")
        oc, wholes = queued(dec, files, srcs, old, wins, S32_LEFT, "planar")
        got = same(oc, wholes, want, want_wholes, wins)
        assert got[1:] == [(OK, 3000), (OK, b1), (OK, 3000)]
        if crc:
            assert got[0] == (CORRUPT, 0) and (wholes[0].cpu().numpy()[1:3] == 0).all()
        # a destroyed sync code, a changed size field, a changed sample count in a needed block, under the OLD index:
        # DETECT_DATA_CORRUPTION, the zero fill, nothing outside the destination; in front of and behind the block, served
        for f in (2, 3, 4):
            wins = [(f, b2 - 5, 10), (f, b2 + 100, 50), (f, 0, b2), (f, b3, 1000)]
            for zero_fill in (True, False):
                oc, wholes = queued(dec, files, srcs, old, wins, F32, "interleaved", zero_fill)
                import torch
                torch.cuda.synchronize()
                assert [tuple(int(v) for v in r) for r in oc.cpu().numpy()] == [(CORRUPT, 0), (CORRUPT, 0), (OK, b2), (OK, 1000)], f
                for w, o in zip(wins, wholes):
                    o = TD.bits_of(o.cpu().numpy())
                    assert (o[0] == TD.SENTINEL).all() and (o[3] == TD.SENTINEL).all(), (f, w)
                for o in wholes[:2]:
                    o = TD.bits_of(o.cpu().numpy())[1:3]
                    assert (o == 0).all() if zero_fill else (o == TD.SENTINEL).all(), f
                for (_, s, l), o in zip(wins[2:], wholes[2:]):
                    assert np.array_equal(TD.bits_of(o.cpu().numpy())[1:3], TD.bits_of(TD.convert(pcms[6][:, s:s + l], F32, 16))), (f, s)
    finally:
        dec.close(); ref.close()


def test_an_index_of_another_size_refuses_its_item_alone(hip, clips):
    datas, lens, pcms = clips
    srcs, keep = TR.resident(datas[:3])
    idx = indexes(hip, datas[:3])
    wins = [(0, 100, 900), (1, 100, 900), (2, 100, 900), (1, 200, 50)]
    dec, ref = TD.pair(hip)
    try:
        outs, wholes = make_outs(datas, wins, S16, "planar")
        oc = dec.decode_windows_indexed_into([srcs[i] for i, _, _ in wins], [idx[0], idx[2], idx[2], None], [s for _, s, _ in wins], outs, S16)
        want, want_wholes = synchronous(ref, datas, srcs, wins, S16, "planar")
        import torch
        torch.cuda.synchronize()
        assert [tuple(int(v) for v in r) for r in oc.cpu().numpy()] == [(OK, 900), (INVALID_ARGUMENT, 0), (OK, 900), (INVALID_ARGUMENT, 0)]
        for k in (0, 2):
            assert torch.equal(wholes[k], want_wholes[k])
        for k in (1, 3):
            assert (wholes[k].cpu().numpy() == TD.sentinel_bits(S16)).all()
    finally:
        dec.close(); ref.close()


# ------------------------------------------------------------------ queued: no host wait, the ring, the drain

def _sleep_cycles(ms):
    """torch.cuda._sleep cycles for at least `ms` milliseconds, calibrated with events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    a.record(); torch.cuda._sleep(20_000_000); b.record()
    torch.cuda.synchronize()
    return int(20_000_000 * ms / max(a.elapsed_time(b), 1e-3)) + 1


def _behind_a_sleep(side, base, good, cycles):
    """`base` holds garbage; on `side`: a sleep of measured length, then the copy that writes the sources -> the two events"""
    import torch
    base.fill_(0xFF)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side); torch.cuda._sleep(cycles); e1.record(side)
        base.copy_(good)
    return e0, e1


def test_the_call_returns_while_the_callers_stream_is_busy(hip, clips):
    """After a warm-up call of the same shape, >= 200 ms of work are queued on a side stream in front of the copy that writes
    the sources.  The queued call must return with that stream still busy; the synchronous call, given the same, returns only
    once the stream has run dry -- which shows that the probe sees a wait when there is one."""
    import torch
    datas, lens, pcms = clips
    srcs, base = TR.resident(datas)
    good = base.clone()
    idx = indexes(hip, datas)
    wins = [(i, n // 3, 1500) for i, n in enumerate(lens)]
    dec, ref = TD.pair(hip)
    try:
        side = torch.cuda.Stream()
        cycles = _sleep_cycles(300)
        queued(dec, datas, srcs, idx, wins, F32, "planar", stream=side)                # the warm-up: buffers and slots grow here
        side.synchronize()
        outs, wholes = make_outs(datas, wins, F32, "planar")
        e0, e1 = _behind_a_sleep(side, base, good, cycles)
        oc = dec.decode_windows_indexed_into(srcs, idx, [s for _, s, _ in wins], outs, F32, stream=side)
        busy = not side.query()
        side.synchronize()
        assert e0.elapsed_time(e1) >= 200.0
        assert busy, "the call waited for the device"
        assert [tuple(int(v) for v in r) for r in oc.cpu().numpy()] == [(OK, 1500)] * len(wins)
        for o, pcm, (_, s, _) in zip(outs, pcms, wins):
            assert np.array_equal(TD.bits_of(o.cpu().numpy()), TD.bits_of(TD.convert(pcm[:, s:s + 1500], F32, 16)))
        # the control: the synchronous route in the same place has waited
        outs2, _ = make_outs(datas, wins, F32, "planar")
        ref.decode_windows_into(srcs, [s for _, s, _ in wins], outs2, F32, stream=side)
        side.synchronize()
        e0, e1 = _behind_a_sleep(side, base, good, cycles)
        got = ref.decode_windows_into(srcs, [s for _, s, _ in wins], outs2, F32, stream=side)
        assert side.query() and [g[:2] for g in got] == [(OK, 1500)] * len(wins)
        side.synchronize()
    finally:
        dec.close(); ref.close()


def test_twice_the_ring_depth_of_calls_behind_one_sleep(hip, clips):
    import torch
    datas, lens, pcms = clips
    srcs, base = TR.resident(datas)
    good = base.clone()
    idx = indexes(hip, datas)
    dec, ref = TD.pair(hip)
    try:
        side = torch.cuda.Stream()
        cycles = _sleep_cycles(200)
        calls = [[(i, (n // 11) * (k + 1) % (n - 700), 700 + k) for i, n in enumerate(lens)] for k in range(2 * hip.DEC_QUEUE_SLOTS)]
        queued(dec, datas, srcs, idx, calls[0], S32_LEFT, "planar", stream=side)
        side.synchronize()
        _behind_a_sleep(side, base, good, cycles)
        results = [queued(dec, datas, srcs, idx, wins, S32_LEFT, "planar", stream=side) for wins in calls]
        side.synchronize()
        for wins, (oc, wholes) in zip(calls, results):
            assert [tuple(int(v) for v in r) for r in oc.cpu().numpy()] == [(OK, l) for _, _, l in wins]
            for (i, s, l), o in zip(wins, wholes):
                assert np.array_equal(o.cpu().numpy()[1:3], pcms[i][:, s:s + l]), (i, s, l)
    finally:
        dec.close(); ref.close()


def test_other_calls_of_the_handle_drain_the_queue(hip, clips):
    import torch
    datas, lens, pcms = clips
    srcs, keep = TR.resident(datas)
    idx = indexes(hip, datas)
    wins = TW.clip_windows(datas)[::7]
    dec, ref = TD.pair(hip)
    try:
        want, want_wholes = synchronous(ref, datas, srcs, wins, S32_LEFT, "planar")
        for _ in range(2):
            oc, wholes = queued(dec, datas, srcs, idx, wins, S32_LEFT, "planar")
            mine, mine_wholes = synchronous(dec, datas, srcs, wins[::-1], S32_LEFT, "planar")       # the same handle, at once
            rw, ow = dec.decode_whole(datas[1], lens[1])
            oc2, wholes2 = queued(dec, datas, srcs, idx, wins, S32_LEFT, "planar")
            whole = TW.whole_files(dec, datas, srcs, S32_LEFT, "planar")
            assert rw == OK and np.array_equal(ow, pcms[1])
            assert all((rc, n) == (OK, t) and np.array_equal(b[:, :t], p) for (rc, n, b), t, p in zip(whole, lens, pcms))
            same(oc, wholes, want, want_wholes, wins)
            same(oc2, wholes2, want, want_wholes, wins)
            assert mine == want[::-1] and all(torch.equal(a, b) for a, b in zip(mine_wholes, want_wholes[::-1]))
    finally:
        dec.close(); ref.close()


def test_empty_call(hip):
    import torch
    dec, _ = TD.pair(hip)
    try:
        oc = dec.decode_windows_indexed_into([], [], [], [], F32)
        assert tuple(oc.shape) == (0, 2)
        t, oc = dec.decode_windows_indexed([], [], [], 100)
        assert tuple(t.shape) == (0, 0, 100) and tuple(oc.shape) == (0, 2)
        assert dec.index_resident([]) == []
        L = hip.lib()
        out = torch.zeros(2, dtype=torch.int32, device="cuda")
        assert L.sla_hip_decode_windows_indexed(C.c_void_p(dec._h), None, 0, F32, 0, C.c_void_p(out.data_ptr()), None) == 0
        assert dec.last_timing() == [0.0] * 6
        # outcomes that are not device memory: nothing queued
        host = np.zeros(4, np.int32)
        items = (hip.IndexedWindowItem * 1)()
        assert L.sla_hip_decode_windows_indexed(C.c_void_p(dec._h), items, 1, F32, 0, C.c_void_p(host.ctypes.data), None) == INVALID_ARGUMENT
        assert L.sla_hip_decode_windows_indexed(C.c_void_p(dec._h), items, 1, F32, 0, C.c_void_p(out.data_ptr() + 4), None) == INVALID_ARGUMENT
    finally:
        dec.close()
