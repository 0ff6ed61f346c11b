"""GPU tests of sla_hip_launch_dec_walk_wide (kernels/walk_wide.inc; run with -m gpu on an MI355X): the block table of one
stream, found and ranked by the whole device, against tests/walkmodel.py::walk and against sla_hip_launch_dec_walk run on
the same file in the same test -- results and the raw bytes of the three tables, which are sentinel-filled so that a
write outside [first, first + max_rows) shows.  The sources lie between sentinel bytes that look like blocks: a read
outside the stream would show as a node the model does not have."""
import ctypes as C

import numpy as np
import pytest

import walkmodel as WM
import widewalkcases as WC
import widewalkmodel as WW

pytestmark = pytest.mark.gpu

BLOCK_DT = np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"), ("num_samples", "<u4"), ("flags", "<u4")])
FILE_DT = np.dtype([("src", "<u8"), ("img_off", "<u8"), ("data_size", "<u4"), ("total", "<u4"), ("capacity", "<u4"),
                    ("first", "<u4"), ("max_rows", "<u4"), ("plane_off", "<u4")])
SPARE = 3                        # sentinel rows in front of and behind the file's rows
GUARD = b"\xff\xff\x00\x00\x00\x02\x00\x00" * 8       # what surrounds every source: sync codes with plausible size fields
INVALID = 2                      # SLA_APIRESULT_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


class Rig:
    """one scratch, one stream (the default), tables large enough for every case of a test"""

    def __init__(self, hip, max_size, node_capacity, max_rows):
        import torch
        self.torch, self.L = torch, hip.lib()
        self.cap = node_capacity
        self.scratch = torch.empty(WW.scratch_bytes(max_size, node_capacity), dtype=torch.uint8, device="cuda")
        assert self.scratch.data_ptr() % 16 == 0
        self.rows = max_rows + 2 * SPARE
        self.max_size = max_size

    def _tables(self):
        t = self.torch
        return (t.full((self.rows * 24,), 0xA5, dtype=t.uint8, device="cuda"), t.full((self.rows * 8,), 0xA5, dtype=t.uint8, device="cuda"),
                t.full((self.rows * 4,), 0xA5, dtype=t.uint8, device="cuda"))

    def place(self, data, mis):
        """the stream at a 16-byte boundary plus mis, between guards -> (tensor, address)"""
        host = np.frombuffer(GUARD + bytes(mis) + bytes(data) + GUARD, np.uint8).copy()
        host[len(GUARD):len(GUARD) + mis] = 0xFF
        buf = self.torch.from_numpy(host).cuda()
        assert buf.data_ptr() % 16 == 0
        return buf, buf.data_ptr() + len(GUARD) + mis

    def run(self, case, crc, mis=0, max_rows=None, img_off=0, plane_off=0, node_capacity=None):
        """count mode and write mode, wide and lane; -> (model, info of the write-mode wide walk)"""
        t, L = self.torch, self.L
        name, data, total, cap, cap_n = case
        assert len(data) <= self.max_size
        ncap = node_capacity or self.cap
        model = WW.wide_walk(data, total, cap, cap_n, crc, ncap)
        spec = WM.walk(data, total, cap, cap_n, crc)
        if not model.overflow:
            assert (model.rows, model.stop, model.extent) == (spec.rows, spec.stop, spec.extent), name
        want_res = (model.num_blocks, model.stop, model.extent, model.overflow)
        buf, addr = self.place(data, mis)
        rows = spec.num_blocks if max_rows is None else max_rows
        assert rows + 2 * SPARE <= self.rows
        ft = np.zeros(1, FILE_DT)
        ft[0] = (addr if len(data) else 0, img_off, len(data), total, cap, SPARE, rows, plane_off)
        host_file = (C.c_uint8 * 40).from_buffer_copy(ft.tobytes())
        d_ft = t.from_numpy(ft.view(np.uint8).copy()).cuda()
        p = lambda x: C.c_void_p(x.data_ptr())
        got = {}
        for mode in ("count", "write"):
            for walker in ("lane", "wide"):
                res = t.full((16,), 0xA5, dtype=t.uint8, device="cuda")
                blk, end, crcf = self._tables()
                tabs = (p(blk), p(end), p(crcf)) if mode == "write" else (None, None, None)
                if walker == "lane":
                    rc = L.sla_hip_launch_dec_walk(p(d_ft), 1, cap_n, crc, p(res), *tabs, None)
                else:
                    rc = L.sla_hip_launch_dec_walk_wide(host_file, cap_n, crc, p(res), *tabs, ncap, p(self.scratch), None)
                assert rc == 0, (name, mode, walker)
                t.cuda.synchronize()
                got[mode, walker] = (tuple(int(v) for v in res.cpu().numpy().view("<u4")), blk.cpu().numpy().tobytes(),
                                     end.cpu().numpy().tobytes(), crcf.cpu().numpy().tobytes())
            info = tuple(int(v) for v in self.scratch[:16].cpu().numpy().view("<u4"))
            assert got[mode, "wide"][0] == want_res, (name, mode, crc, got[mode, "wide"][0], want_res, info)
            if not model.overflow:
                assert got[mode, "lane"][0] == want_res, (name, mode)
                assert got[mode, "wide"][1:] == got[mode, "lane"][1:], (name, mode, crc, mis)
            if total != 0 and len(data) >= 54:
                assert info[0] == model.num_nodes, (name, mode, info, model.num_nodes)
        # the write-mode tables against the model, row by row
        want_blk = np.frombuffer(bytes([0xA5]) * (self.rows * 24), BLOCK_DT).copy()
        want_end = np.full(self.rows, 0xA5A5A5A5A5A5A5A5, "<u8")
        want_crc = np.full(self.rows, 0xA5A5A5A5, "<u4")
        for r in range(rows):
            if r < len(model.rows):
                off, blen, pos, n, flags, crcv = model.rows[r]
                want_blk[SPARE + r] = (img_off + off, blen, plane_off + pos, n, flags)
                want_crc[SPARE + r] = crcv
            else:
                want_blk[SPARE + r] = (img_off, 8, plane_off, 0, WM.HEADER_ONLY)
                want_crc[SPARE + r] = 0
            want_end[SPARE + r] = img_off + len(data)
        _, blk, end, crcf = got["write", "wide"]
        assert blk == want_blk.tobytes() and end == want_end.tobytes() and crcf == want_crc.tobytes(), (name, crc, mis)
        assert got["count", "wide"][1:] == (bytes([0xA5]) * (self.rows * 24), bytes([0xA5]) * (self.rows * 8), bytes([0xA5]) * (self.rows * 4))
        # the source is only read
        assert bytes(buf.cpu().numpy()[len(GUARD) + mis:len(GUARD) + mis + len(data)]) == bytes(data), name
        return model, info


@pytest.mark.parametrize("crc", [1, 0])
def test_round_boundaries(hip, crc):
    rig = Rig(hip, 1 << 16, 4096, 1100)
    for k, case in enumerate(WC.round_cases()):
        model, info = rig.run(case, crc, mis=(5 * k + 1) % 16, img_off=4096 * k, plane_off=64 * k)
        assert model.num_blocks == WC.ROUND_LENGTHS[k] and info[1] == WC.ROUND_LENGTHS[k]


def test_70000_blocks_take_more_than_16_rounds(hip):
    case = WC.long_case()
    rig = Rig(hip, len(case[1]), 70000, 70000)
    assert hip.lib().sla_hip_dec_wide_rounds(len(case[1]), 70000) == 17
    model, info = rig.run(case, 1, mis=9, img_off=1 << 33, plane_off=128)
    assert model.num_blocks == 70000 and info[:3] == (70000, 70000, 0xFFFFFFFF)


@pytest.mark.parametrize("crc", [1, 0])
def test_decoys(hip, crc):
    rig = Rig(hip, 1 << 16, 8192, 64)
    nodes = {}
    for k, case in enumerate(WC.decoy_cases()):
        model, info = rig.run(case, crc, mis=(3 * k + 2) % 16)
        nodes[case[0]] = (info[0], model.num_blocks)
    assert nodes["decoys that chain among themselves"] == (79, 40) and nodes["decoys that merge into the chain"] == (80, 40)
    assert nodes["a decoy chain longer than the real one"] == (183, 3)
    assert nodes["dense field, period 6"][0] > 4500 and nodes["dense field, period 8"][0] > 4500


@pytest.mark.parametrize("head", [0, 13])
def test_headers_across_chunk_word_and_tile_boundaries(hip, head):
    rig = Rig(hip, 1 << 15, 64, 8)
    for case in WC.tile_cases(head):
        model, _ = rig.run(case, 1, mis=head)
        assert model.num_blocks == 3 and model.stop == WM.OK


@pytest.mark.parametrize("mis", [0, 1, 3, 7, 13, 15])
def test_source_alignment_and_every_end_residue(hip, mis):
    """the stream's end at every residue of 16: a chain that ends at its last byte, and one cut inside its last header"""
    rig = Rig(hip, 1 << 12, 256, 16)
    for tail in range(16):
        data, offs = WC.chain([7, 8, 9, 10], [20, 21, 22, 1 + tail], seed=tail)
        model, _ = rig.run(("end %d" % tail, data, 34, 34, 4096), 1, mis=mis)
        assert model.num_blocks == 4 and model.stop == WM.OK
        model, _ = rig.run(("cut %d" % tail, data[:offs[3] + 10], 34, 34, 4096), 1, mis=mis)
        assert model.num_blocks == 3 and model.stop == WM.DATA


@pytest.mark.parametrize("crc", [1, 0])
def test_stops(hip, crc):
    rig = Rig(hip, 1 << 12, 256, 16)
    for k, case in enumerate(WC.stop_cases()):
        rig.run(case, crc, mis=(7 * k + 3) % 16, img_off=1000 + 4 * k, plane_off=64 + k)


def test_max_rows_smaller_and_larger_than_the_chain(hip):
    rig = Rig(hip, 1 << 12, 256, 16)
    case = WC.stop_cases()[0]
    for rows in (0, 1, 4, 6, 9):
        rig.run(case, 1, mis=5, max_rows=rows, img_off=512, plane_off=64)
    rig.run(WC.stop_cases()[12], 1, mis=5, max_rows=9)                   # a header-only row, then empty rows


def test_node_capacity_reached_and_exceeded(hip):
    rig = Rig(hip, 1 << 16, 8192, 64)
    for case in (WC.decoy_cases()[0], WC.decoy_cases()[4]):
        n = len(WW.nodes(case[1]))
        model, info = rig.run(case, 1, mis=4, node_capacity=n)
        assert model.overflow == 0 and info[0] == n
        for cap in (n - 1, 1):
            model, info = rig.run(case, 1, mis=4, node_capacity=cap, max_rows=5)
            assert model.overflow == WW.OVERFLOW and info[0] == n     # the count is exact beyond the capacity


def test_scratch_reuse_by_different_files(hip):
    """two files one after the other on one stream with one scratch, no wait in between: each gets its own table"""
    import torch
    rig = Rig(hip, 1 << 16, 8192, 64)
    L = hip.lib()
    cases = [WC.decoy_cases()[4], WC.stop_cases()[1], WC.decoy_cases()[2]]
    keep, res = [], []
    for k, (name, data, total, cap, cap_n) in enumerate(cases):
        buf, addr = rig.place(data, 3 + 4 * k)
        ft = np.zeros(1, FILE_DT)
        ft[0] = (addr, 0, len(data), total, cap, 0, 0, 0)
        r = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
        keep.append(buf); res.append(r)
        assert L.sla_hip_launch_dec_walk_wide((C.c_uint8 * 40).from_buffer_copy(ft.tobytes()), cap_n, 1, C.c_void_p(r.data_ptr()),
                                              None, None, None, 8192, C.c_void_p(rig.scratch.data_ptr()), None) == 0
    torch.cuda.synchronize()
    for (name, data, total, cap, cap_n), r in zip(cases, res):
        m = WM.walk(data, total, cap, cap_n, 1)
        assert tuple(int(v) for v in r.cpu().numpy().view("<u4")) == (m.num_blocks, m.stop, m.extent, 0), name


def test_refusals(hip):
    import torch
    L = hip.lib()
    name, data, total, cap, cap_n = WC.stop_cases()[0]
    rig = Rig(hip, 1 << 12, 256, 16)
    buf, addr = rig.place(data, 0)
    ft = np.zeros(1, FILE_DT)
    ft[0] = (addr, 0, len(data), total, cap, SPARE, 6, 0)
    f = (C.c_uint8 * 40).from_buffer_copy(ft.tobytes())
    res = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
    blk, end, crcf = rig._tables()
    p = lambda x: C.c_void_p(x.data_ptr())
    s = p(rig.scratch)
    W = L.sla_hip_launch_dec_walk_wide
    assert W(None, cap_n, 1, p(res), None, None, None, 256, s, None) == INVALID
    assert W(f, cap_n, 1, None, None, None, None, 256, s, None) == INVALID
    assert W(f, cap_n, 1, p(res), None, None, None, 256, None, None) == INVALID
    assert W(f, cap_n, 1, p(res), None, None, None, 0, s, None) == INVALID
    assert W(f, cap_n, 1, p(res), None, None, None, 256, C.c_void_p(rig.scratch.data_ptr() + 8), None) == INVALID
    for tabs in ((p(blk), None, None), (None, p(end), None), (None, None, p(crcf)), (p(blk), p(end), None), (p(blk), None, p(crcf))):
        assert W(f, cap_n, 1, p(res), *tabs, 256, s, None) == INVALID
    torch.cuda.synchronize()
    assert bytes(res.cpu().numpy()) == bytes([0xA5]) * 16                # nothing was launched
    assert blk.cpu().numpy().tobytes() == bytes([0xA5]) * (rig.rows * 24)
