"""GPU tests of sla_hip_salvage_resident and sla_hip_launch_dec_salvage_scan (Decoder.salvage_resident_tensor / salvage;
kernels/salvage.inc; run with -m gpu on an MI355X): one resident .sla stream decoded through damage.

The specification is tests/salvagemodel.py; the streams and the damage catalogue are tests/salvagecases.py: 16-bit mono,
16-bit stereo mid/side and 24-bit three-channel streams of 8 to 10 blocks of 2048 to 4096 samples from the oracle's
encoder, and hand-written RAW streams for the decoy, the embedded block and the undecodable block.  The expected PCM of a
case is the oracle's decode of the clean stream with the case's lost ranges zeroed (and the embedded block's samples
moved); all 32 bits are compared, and the report and the ranges with the model's.  Destinations lie between guard words,
sources between guard bytes that look like blocks, tables between sentinel rows.  Nothing here provokes a fault: damaged
input must give codes and silence, which values and guards show."""
import ctypes as C

import numpy as np
import pytest

import salvagecases as SC
import salvagemodel as SM
import test_gpu_decode_batch_device as TD
import walkmodel as WM

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, BUF, CORRUPT = 0, 2, 4, 11
S32_LEFT, S32, S16, F32 = range(4)
GUARD = b"\xff\xff\x00\x00\x00\x02\x00\x00" * 8       # what surrounds every source: sync codes with plausible size fields
PAD = 64                          # guard words in front of and behind a destination
SENT = 0x5A5B5C5D
SPARE = 3                         # sentinel rows in front of and behind a table's rows
BLOCK_DT = np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"), ("num_samples", "<u4"), ("flags", "<u4")])
REASON = {SM.CRC: "crc", SM.UNDECODABLE: "undecodable", SM.GAP: "gap"}


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


@pytest.fixture(scope="module")
def streams(oracle):
    """{shape: (clean bytes, clean PCM)} -- encoded and decoded once by the oracle, shared by every test"""
    return {shape: SC.oracle_stream(oracle, shape) for shape in SC.SHAPES}


def make_decoder(hip, crc=1):
    return hip.Decoder(8, SC.CAP_N, 48, 5, 32, crc)


def place(data, mis):
    """the stream at a 16-byte boundary plus mis, between guards -> (tensor, address)"""
    import torch
    host = np.frombuffer(GUARD + bytes(mis) + bytes(data) + GUARD, np.uint8).copy()
    host[len(GUARD):len(GUARD) + mis] = 0xFF
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + len(GUARD) + mis


def call(hip, dec, data, mis=0, capacity=None, fmt=S32_LEFT, range_capacity=16):
    """sla_hip_salvage_resident into a guarded planar int32 destination -> (code, report, ranges, samples [C][cap], guards ok)"""
    import torch
    nch, total = data[14], WM.header_total(data)
    cap = total if capacity is None else capacity
    buf, addr = place(data, mis)
    dst = torch.full((PAD + nch * cap + PAD,), SENT, dtype=torch.int32, device="cuda")
    rep, rng = hip.SalvageReport(), (hip.SalvageRange * max(range_capacity, 1))()
    rc = hip.lib().sla_hip_salvage_resident(dec._h, C.c_void_p(addr), len(data), C.c_void_p(dst.data_ptr() + 4 * PAD), cap, 1, cap, fmt,
                                            C.byref(rep), rng, range_capacity, None)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    guards = bool(np.all(out[:PAD] == SENT) and np.all(out[PAD + nch * cap:] == SENT))
    assert bytes(buf.cpu().numpy()[len(GUARD) + mis:len(GUARD) + mis + len(data)]) == bytes(data)      # the source is only read
    ranges = [(r.start, r.length, r.reason) for r in rng[:min(rep.num_ranges, range_capacity)]]
    return rc, rep, ranges, out[PAD:PAD + nch * cap].reshape(nch, cap), guards


def check_case(hip, dec, case, pcm, mis=0):
    name, data, mode, lost, patches, undec = case
    m = SM.salvage(data, SC.CAP_N, undec)
    assert (m.mode, m.lost) == (mode, lost), name
    rc, rep, ranges, out, guards = call(hip, dec, data, mis)
    assert guards, name
    assert rc == (CORRUPT if (m.lost or m.concealed) else OK), (name, rc)
    assert (rep.mode, rep.blocks_decoded, rep.blocks_concealed, rep.samples_lost, rep.num_ranges) \
        == (m.mode, m.decoded, m.concealed, m.samples_lost, len(m.lost)), name
    assert ranges == m.lost, (name, ranges, m.lost)
    if m.mode == 2:
        assert (rep.prefix_blocks, rep.suffix_blocks, rep.suffix_byte, rep.suffix_sample, rep.nodes, rep.sound_nodes) \
            == (m.prefix_blocks, m.suffix_blocks, m.suffix_byte, m.suffix_sample, m.nodes, m.sound_nodes), name
    else:
        assert (rep.prefix_blocks, rep.suffix_blocks, rep.suffix_byte, rep.suffix_sample, rep.nodes, rep.sound_nodes) == (0,) * 6, name
    want = SC.expected_pcm(pcm, lost, patches)
    assert np.array_equal(out, want), (name, np.nonzero(np.any(out != want, axis=0))[0][:8])
    return rep


# ------------------------------------------------------------------ the catalogue

@pytest.mark.parametrize("shape", list(SC.SHAPES))
def test_catalogue(hip, streams, shape):
    data, pcm = streams[shape]
    dec = make_decoder(hip)
    try:
        for k, case in enumerate(SC.catalogue(data)):
            check_case(hip, dec, case, pcm, mis=(5 * k + 1) % 16)
    finally:
        dec.close()


def test_clean_stream_equals_the_resident_decode_bit_for_bit(hip, streams):
    import torch
    for shape, (data, pcm) in streams.items():
        dec, ref = make_decoder(hip), make_decoder(hip)
        try:
            src = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
            for dtype in (torch.int32, torch.float32, torch.int16):
                got, rep, ranges = dec.salvage_resident_tensor(src, dtype=dtype)
                want, lens, codes = ref.decode_resident_tensor([src], dtype=dtype)
                assert codes == [OK] and lens == [pcm.shape[1]]
                assert np.array_equal(TD.bits_of(got.cpu().numpy()), TD.bits_of(want[0].cpu().numpy())), (shape, dtype)
                assert rep["result"] == OK and rep["mode"] == 1 and ranges == []
                assert {k: v for k, v in rep.items() if k not in ("mode", "blocks_decoded")} == {
                    k: 0 for k in rep if k not in ("mode", "blocks_decoded")}
                assert rep["blocks_decoded"] == len(SC.blocks_of(data))
            assert np.array_equal(dec.salvage(data, dtype=torch.int32)[0], pcm), shape
        finally:
            dec.close(); ref.close()


def test_hand_written_streams_decoy_embedded_block_and_undecodable_block(hip):
    dec = make_decoder(hip)
    try:
        for cases, pcm in SC.raw_cases():
            for k, case in enumerate(cases):
                check_case(hip, dec, case, pcm, mis=(3 * k + 2) % 16)
    finally:
        dec.close()


def test_crc_check_off_changes_nothing(hip, streams):
    """soundness is judged with the CRC whatever the handle's enable_crc_check says"""
    data, pcm = streams["mono16"]
    dec = make_decoder(hip, crc=0)
    try:
        cases = SC.catalogue(data)
        for case in (cases[0], cases[2], cases[4], cases[6], cases[9]):
            check_case(hip, dec, case, pcm, mis=7)
    finally:
        dec.close()


@pytest.mark.parametrize("mis", [1, 3, 7, 13, 15])
def test_odd_source_byte_offsets(hip, streams, mis):
    data, pcm = streams["stereo16ms"]
    dec = make_decoder(hip)
    try:
        cases = SC.catalogue(data)
        for case in (cases[2], cases[5], cases[10], cases[12]):
            check_case(hip, dec, case, pcm, mis=mis)
    finally:
        dec.close()


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("fmt", [S32_LEFT, S32, S16, F32], ids=["s32left", "s32", "s16", "f32"])
def test_every_output_format_and_both_layouts(hip, streams, fmt, layout):
    import torch
    for shape in ("stereo16ms", "three24"):
        data, pcm = streams[shape]
        name, bad, mode, lost, patches, undec = SC.catalogue(data)[6]            # a sync code destroyed
        dec = make_decoder(hip)
        try:
            src = torch.from_numpy(np.frombuffer(bad, np.uint8).copy()).cuda()
            got, rep, ranges = dec.salvage_resident_tensor(src, dtype=TD.torch_dtype(fmt), layout=layout, right_justify=(fmt == S32))
            want = TD.convert(SC.expected_pcm(pcm, lost, patches), fmt, data[23])
            got = got.cpu().numpy()
            assert got.shape == (want.shape if layout == "planar" else want.T.shape)
            assert np.array_equal(TD.bits_of(got if layout == "planar" else got.T), TD.bits_of(want)), (shape, fmt, layout)
            assert rep["result"] == CORRUPT and rep["mode"] == 2 and ranges == [(s, n, REASON[r]) for s, n, r in lost]
        finally:
            dec.close()


# ------------------------------------------------------------------ refusals, guards, capacities

def test_capacity_below_the_header_is_refused_and_nothing_is_written(hip, streams):
    data, pcm = streams["mono16"]
    total = pcm.shape[1]
    dec = make_decoder(hip)
    try:
        rc, rep, ranges, out, guards = call(hip, dec, data, capacity=total - 1)
        assert rc == BUF and guards and np.all(out == np.int32(SENT))
        assert bytes(rep) == bytes(48)
        # a larger destination: exactly [0, C) x [0, N) is written, the tail of every channel keeps the sentinel
        data2, pcm2 = streams["stereo16ms"]
        case = SC.catalogue(data2)[9]
        rc, rep, ranges, out, guards = call(hip, dec, case[1], capacity=pcm2.shape[1] + 37)
        assert rc == CORRUPT and guards
        assert np.array_equal(out[:, :pcm2.shape[1]], SC.expected_pcm(pcm2, case[3], case[4])) and np.all(out[:, pcm2.shape[1]:] == np.int32(SENT))
    finally:
        dec.close()


def test_refusals_leave_the_destination_alone(hip, streams):
    import torch
    data, pcm = streams["mono16"]
    dec = make_decoder(hip)
    try:
        L = hip.lib()
        buf, addr = place(data, 3)
        dst = torch.full((pcm.shape[1] + 2 * PAD,), SENT, dtype=torch.int32, device="cuda")
        rep, rng = hip.SalvageReport(), (hip.SalvageRange * 4)()
        host = np.frombuffer(data, np.uint8).copy()
        n = pcm.shape[1]
        F = lambda src, size, d, cap, fmt=0: L.sla_hip_salvage_resident(dec._h, C.c_void_p(src), size, C.c_void_p(d), cap, 1, cap, fmt,
                                                                        C.byref(rep), rng, 4, None)
        assert F(host.ctypes.data, len(data), dst.data_ptr() + 4 * PAD, n) == INVALID_ARGUMENT          # a host source
        assert F(addr, 0xF0000000, dst.data_ptr() + 4 * PAD, n) == INVALID_ARGUMENT                     # a source that runs past its allocation
        assert F(addr, len(data), dst.data_ptr() + 4 * PAD, 0xF0000000) == INVALID_ARGUMENT             # a destination that runs past its allocation
        assert F(addr, len(data), dst.data_ptr() + 4 * PAD + 2, n) == INVALID_ARGUMENT                  # misaligned for int32
        assert F(addr, 20, dst.data_ptr() + 4 * PAD, n) == 9                                            # INSUFFICIENT_DATA_SIZE: no header
        bad = bytearray(data); bad[0] = ord("X")
        b2, a2 = place(bytes(bad), 5)
        assert F(a2, len(data), dst.data_ptr() + 4 * PAD, n) == 10                                      # INVALID_HEADER_FORMAT
        torch.cuda.synchronize()
        assert bool(torch.all(dst == SENT))
    finally:
        dec.close()


def test_more_ranges_than_room(hip, streams):
    data, pcm = streams["mono16"]
    case = SC.catalogue(data)[4]                               # two flipped blocks: two ranges
    dec = make_decoder(hip)
    try:
        for room in (0, 1, 2):
            rc, rep, ranges, out, guards = call(hip, dec, case[1], range_capacity=room)
            assert rc == CORRUPT and rep.num_ranges == 2 and ranges == case[3][:room] and guards
            assert np.array_equal(out, SC.expected_pcm(pcm, case[3], case[4]))
    finally:
        dec.close()


def test_node_capacity_of_one_forces_the_repeat_and_the_wide_walk_agrees(hip, streams):
    data, pcm = streams["three24"]
    cases = SC.catalogue(data)
    dec = make_decoder(hip)
    try:
        dec.set_option("wide_walk_nodes", 1)
        for case in (cases[6], cases[12]):
            check_case(hip, dec, case, pcm, mis=9)
            assert dec.last_walk()[1] == 1                     # the scan overflowed once and was repeated
        dec.set_option("wide_walk_nodes", 0)
        dec.set_option("wide_walk", 1)                         # the count and the mode-1 rows through the wide walk
        for case in (cases[0], cases[2], cases[6], cases[11]):
            check_case(hip, dec, case, pcm, mis=4)
            assert dec.last_walk()[0] >= 1
    finally:
        dec.close()


# ------------------------------------------------------------------ the scan launcher on its own

class ScanRig:
    def __init__(self, hip, max_size, node_capacity, max_rows):
        import torch
        self.torch, self.L, self.hip = torch, hip.lib(), hip
        self.cap = node_capacity
        self.scratch = torch.empty(int(self.L.sla_hip_dec_salvage_scratch_bytes(max_size, node_capacity)), dtype=torch.uint8, device="cuda")
        assert self.scratch.data_ptr() % 16 == 0
        self.rows = max_rows + 2 * SPARE

    def tables(self):
        t = self.torch
        return tuple(t.full((self.rows * w,), 0xA5, dtype=t.uint8, device="cuda") for w in (24, 8, 4))

    def scan(self, data, nch, mis, write, max_rows=0, img_off=0, plane_off=0, node_capacity=None):
        t = self.torch
        buf, addr = place(data, mis)
        f = self.hip.DecWalkFile()
        f.src, f.img_off, f.data_size, f.total, f.capacity = addr, img_off, len(data), WM.header_total(data), 0
        f.first, f.max_rows, f.plane_off = SPARE, max_rows, plane_off
        res = t.full((48,), 0xA5, dtype=t.uint8, device="cuda")
        tabs = self.tables()
        p = lambda x: C.c_void_p(x.data_ptr())
        rc = self.L.sla_hip_launch_dec_salvage_scan(C.byref(f), nch, SC.CAP_N, p(res), *([p(x) for x in tabs] if write else [None] * 3),
                                                    node_capacity or self.cap, p(self.scratch), None)
        assert rc == 0
        t.cuda.synchronize()
        return tuple(int(v) for v in res.cpu().numpy().view("<u4")), tuple(x.cpu().numpy().tobytes() for x in tabs)

    def want_tables(self, m, data, max_rows, img_off, plane_off):
        blk = np.frombuffer(bytes([0xA5]) * (self.rows * 24), BLOCK_DT).copy()
        end = np.full(self.rows, 0xA5A5A5A5A5A5A5A5, "<u8")
        crc = np.full(self.rows, 0xA5A5A5A5, "<u4")
        for r in range(max_rows):
            if r < len(m.rows):
                off, blen, pos, n, flags, crcv = m.rows[r]
                blk[SPARE + r] = (img_off + off, blen, plane_off + pos, n, 0)
                crc[SPARE + r] = crcv
            else:
                blk[SPARE + r] = (img_off, 8, plane_off, 0, WM.HEADER_ONLY)
                crc[SPARE + r] = 0
            end[SPARE + r] = img_off + len(data)
        return blk.tobytes(), end.tobytes(), crc.tobytes()


def model_result(m, overflow=0):
    return (m.prefix_blocks, m.prefix_samples, m.prefix_end, m.suffix_byte, m.suffix_samples, m.suffix_blocks, m.nodes, m.sound_nodes,
            overflow, 0, 0, 0)


def test_scan_launcher_against_the_model(hip, streams):
    rig = ScanRig(hip, 1 << 18, 4096, 16)
    untouched = tuple(bytes([0xA5]) * (rig.rows * w) for w in (24, 8, 4))
    sets = [(SC.catalogue(data), data[14]) for data, pcm in streams.values()] + [(cases, 1) for cases, pcm in SC.raw_cases()]
    k = 0
    for cases, nch in sets:
        for name, data, mode, lost, patches, undec in cases:
            if mode != 2:
                continue
            k += 1
            m = SM.salvage(data, SC.CAP_N, undec)
            mis, img_off, plane_off = (7 * k + 3) % 16, 4096 * k, 64 * k
            got, tabs = rig.scan(data, nch, mis, write=False)
            assert got == model_result(m), (name, got, model_result(m))
            assert tabs == untouched, name
            got, tabs = rig.scan(data, nch, mis, write=True, max_rows=len(m.rows), img_off=img_off, plane_off=plane_off)
            assert got == model_result(m), name
            assert tabs == rig.want_tables(m, data, len(m.rows), img_off, plane_off), name
    assert k >= 30


def test_scan_respects_max_rows_and_reports_an_overflow_exactly(hip, streams):
    data, pcm = streams["mono16"]
    name, bad, mode, lost, patches, undec = SC.catalogue(data)[6]
    m = SM.salvage(bad, SC.CAP_N)
    rig = ScanRig(hip, 1 << 17, 4096, 16)
    assert m.prefix_blocks >= 2 and m.suffix_blocks >= 2
    for rows in (0, 1, m.prefix_blocks, m.prefix_blocks + 1, len(m.rows) - 1, len(m.rows) + 3):
        got, tabs = rig.scan(bad, 1, 5, write=True, max_rows=rows, img_off=512, plane_off=64)
        assert got == model_result(m), rows
        assert tabs == rig.want_tables(m, bad, rows, 512, 64), rows       # nothing at or behind first + max_rows
    # exactly as many nodes as the capacity: no overflow; one fewer, or 1: overflow, the count exact, empty rows only
    got, tabs = rig.scan(bad, 1, 5, write=False, node_capacity=m.nodes)
    assert got == model_result(m)
    empty = SM.Salvage(nodes=m.nodes)
    for cap in (m.nodes - 1, 1):
        got, tabs = rig.scan(bad, 1, 5, write=True, max_rows=4, node_capacity=cap)
        assert got == model_result(empty, overflow=1), cap
        assert tabs == rig.want_tables(empty, bad, 4, 0, 0), cap
    # a stream too short for a block
    got, tabs = rig.scan(bad[:50], 1, 5, write=True, max_rows=2)
    assert got == model_result(SM.Salvage()) and tabs == rig.want_tables(SM.Salvage(), bad[:50], 2, 0, 0)


def test_conceal_and_crc_launchers(hip):
    import torch
    L = hip.lib()
    stride, nch = 1000, 3
    planes = torch.arange(1, nch * stride + 1, dtype=torch.int32, device="cuda")
    entries = [(0, 5), (17, 300), (990, 50), (400, 0), (2000, 7)]          # the third is clipped to the stride, the last lies beyond it
    lst = torch.from_numpy(np.array(entries, "<u4").reshape(-1).view(np.uint8).copy()).cuda()
    assert L.sla_hip_launch_dec_conceal(C.c_void_p(planes.data_ptr()), stride, nch - 1, C.c_void_p(lst.data_ptr()), len(entries), 300, None) == 0
    torch.cuda.synchronize()
    want = np.arange(1, nch * stride + 1, dtype=np.int32).reshape(nch, stride)
    for s, n in entries:
        want[:nch - 1, s:min(s + n, stride)] = 0
    assert np.array_equal(planes.cpu().numpy().reshape(nch, stride), want)    # the third plane is not one of the two channels
    # the CRC pass: three blocks in an image, the second with a wrong stored CRC
    rng = np.random.default_rng(5)
    body = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (100, 8, 5000)]
    image, rows, crcf, pos = b"\x00" * 3, [], [], 3
    for k, b in enumerate(body):
        rows.append((pos, len(b), 0, 0, 0))
        crcf.append(SM.crc16(b[8:]) ^ (1 if k == 1 else 0))
        image += b
        pos += len(b)
    img = torch.from_numpy(np.frombuffer(image + b"\x00" * 16, np.uint8).copy()).cuda()
    blk = torch.from_numpy(np.array(rows, BLOCK_DT).view(np.uint8).copy()).cuda()
    cf = torch.from_numpy(np.array(crcf, "<u4").view(np.uint8).copy()).cuda()
    bad = torch.full((5,), 0x77, dtype=torch.int32, device="cuda")
    assert L.sla_hip_launch_salvage_crc(C.c_void_p(img.data_ptr()), C.c_void_p(blk.data_ptr()), C.c_void_p(cf.data_ptr()), 3,
                                        C.c_void_p(bad.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert bad.cpu().numpy().tolist() == [0, 1, 0, 0x77, 0x77]
    got = blk.cpu().numpy().view(BLOCK_DT)
    assert got["flags"].tolist() == [0, WM.HEADER_ONLY, 0] and got["byte_off"].tolist() == [r[0] for r in rows]
