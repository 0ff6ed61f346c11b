"""CPU-only checks of sla_hip_splice_plan (include/sla_hip.h; sla_amd/csrc/sla_splice.c), the layout rule of
sla_hip_splice_resident as a device-free function: on every cut and join of tests/splicemodel.py it gives the model's bytes,
counts and 43 header bytes; every refusal of the rule, each from an input that breaks one condition; and the new entry
points are exported by the library."""
import ctypes as C

import numpy as np
import pytest

import crafted_catalogue as CC
import sla_amd
import slastream as SS
import splicemodel as SM

CASES = SM.cases()
IDS = [name for name, _ in CASES]
OK, INVALID_ARGUMENT, CAPACITY, CHPROC, DATA, HEADER_FORMAT, SYNC_LOST = 0, 2, 3, 5, 9, 10, 12
SEG_DTYPE = np.dtype([("data", "<u8"), ("index", "<u8"), ("data_size", "<u4"), ("start", "<u4"), ("length", "<u4"), ("reserved", "<u4")])


@pytest.fixture(scope="module")
def L():
    import os
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


_index = {}


def index_of(case):
    if case.name not in _index:
        _index[case.name] = sla_amd.Index.build(case.data)
    return _index[case.name]


def plan(segs):
    return sla_amd.splice_plan([(None, index_of(c), s, l) for c, s, l in segs])


def reheader(data, edit):
    """the stream with edit(bytearray header) applied and a correct header CRC again"""
    d = bytearray(data)
    edit(d)
    d[8:10] = SS.crc16(d[10:43]).to_bytes(2, "big")
    return bytes(d)


def test_struct_sizes_and_symbols(L):
    assert C.sizeof(sla_amd.SpliceSegment) == SEG_DTYPE.itemsize == 32 and C.sizeof(sla_amd.SpliceItem) == 32
    assert C.sizeof(sla_amd.SpliceLayout) == 80
    assert (C.sizeof(sla_amd.SpliceCheck), C.sizeof(sla_amd.SpliceEdge), C.sizeof(sla_amd.SpliceCopy)) == (40, 24, 24)
    for name in ("sla_hip_splice_plan", "sla_hip_splice_resident", "sla_hip_launch_splice_edges", "sla_hip_launch_splice_copy",
                 "sla_hip_launch_splice_check"):
        assert hasattr(L, name), name


def test_the_check_entry_matches_the_headers_struct():
    """sla_hip_splice_check as include/sla_hip.h declares it: the fields in its order, pointers and uint64_t 8 bytes,
    uint32_t 4, no padding -- 40 bytes -- and sla_amd.SpliceCheck field for field at the same offsets"""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sla_hip.h")) as f:
        text = f.read()
    body = re.search(r"typedef struct sla_hip_splice_check \{(.*?)\} sla_hip_splice_check;", text, re.S).group(1)
    fields = re.findall(r"^\s*(const uint8_t\*|uint64_t|uint32_t)\s+(\w+);", body, re.M)
    assert [name for _, name in fields] == ["src", "plane_off", "byte_len", "num_samples", "verdict", "ordinal", "edge", "keep"]
    pos = 0
    for typ, name in fields:
        size = 4 if typ == "uint32_t" else 8
        assert pos % size == 0
        field = getattr(sla_amd.SpliceCheck, name)
        assert (field.offset, field.size) == (pos, size), name
        pos += size
    assert pos == C.sizeof(sla_amd.SpliceCheck) == 40 and len(sla_amd.SpliceCheck._fields_) == len(fields)
    assert int(re.search(r"#define SLA_HIP_SPLICE_NO_EDGE (0x[0-9A-Fa-f]+)u", text).group(1), 16) == sla_amd.SPLICE_NO_EDGE == SM.NO_EDGE


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_equals_the_model(L, case):
    _, segs = case
    m = SM.splice(list(segs))
    rc, lay = plan(segs)
    assert rc == m.rc == OK
    assert (lay.bytes, lay.num_samples, lay.num_blocks) == (len(m.data), m.num_samples, m.num_blocks)
    assert (lay.verbatim_bytes, lay.edge_blocks) == (m.verbatim_bytes, m.edge_blocks)
    assert (lay.max_block_size, lay.max_bit_per_second) == (m.max_block_size, m.max_bit_per_second)
    assert bytes(lay.header) == m.data[:43] + bytes(5)


def zero(lay):
    return bytes(lay) == bytes(C.sizeof(lay))


def test_refusals_of_arguments(L):
    A = SM.sources()["mono16"][0]
    item, keep = sla_amd._splice_item([(None, index_of(A), 0, 10)])
    lay = sla_amd.SpliceLayout()
    assert L.sla_hip_splice_plan(None, C.byref(lay)) == INVALID_ARGUMENT
    assert L.sla_hip_splice_plan(C.byref(item), None) == INVALID_ARGUMENT
    assert L.sla_hip_splice_plan(C.byref(item), C.byref(lay)) == OK and lay.num_samples == 10
    for segs in ([], [(None, None, 0, 10)], [(None, index_of(A), 0, 10), (None, None, 0, 0)],
                 [((0, len(A.data) + 1), index_of(A), 0, 10)], [((0, len(A.data) - 1), index_of(A), 0, 0)]):
        rc, lay = sla_amd.splice_plan(segs)
        assert rc == INVALID_ARGUMENT and zero(lay), segs
    item.num_segments = 0
    assert L.sla_hip_splice_plan(C.byref(item), C.byref(lay)) == INVALID_ARGUMENT
    item.num_segments, item.segments = 1, None
    assert L.sla_hip_splice_plan(C.byref(item), C.byref(lay)) == INVALID_ARGUMENT


def test_refusals_of_headers(L):
    A, B = SM.sources()["stereo16ms"][:2]
    xa = index_of(A)
    # a header DecodeHeader does not return OK for: a wrong CRC (fields delivered all the same), a wrong signature
    bad_crc = sla_amd.Index.build(A.data[:8] + bytes([A.data[8] ^ 1]) + A.data[9:])
    assert bad_crc.header_result == 11 and bad_crc.num_blocks == xa.num_blocks
    junk = sla_amd.Index.build(b"XL" + A.data[2:])
    for x in (bad_crc, junk):
        assert sla_amd.splice_plan([(None, x, 0, 10)])[0] == INVALID_ARGUMENT
        assert sla_amd.splice_plan([(None, xa, 0, 10), (None, x, 0, 0)])[0] == INVALID_ARGUMENT
    # every byte of the shared format, one at a time; the other header bytes may differ
    for k in [14] + list(range(19, 29)) + [33, 34]:
        other = sla_amd.Index.build(reheader(B.data, lambda d: d.__setitem__(k, d[k] ^ 1)))
        assert other.header_result == 0
        rc, lay = sla_amd.splice_plan([(None, xa, 0, 10), (None, other, 0, 0)])
        assert rc == INVALID_ARGUMENT and zero(lay), k
    for k in list(range(15, 19)) + list(range(29, 33)) + list(range(35, 43)):
        other = sla_amd.Index.build(reheader(B.data, lambda d: d.__setitem__(k, d[k] ^ 1)))
        rc, lay = sla_amd.splice_plan([(None, xa, 0, 10), (None, other, 0, 7)])
        assert rc == (OK if other.extent >= 7 else DATA), k
    # formats no RAW block can be written for
    M = SM.sources()["mono16"][0]
    for src, k, v, want in ((A, 14, 3, CHPROC), (A, 14, 0, CHPROC), (A, 23, 0, HEADER_FORMAT), (A, 23, 33, HEADER_FORMAT),
                            (A, 24, 16, HEADER_FORMAT), (M, 14, 0, HEADER_FORMAT), (M, 14, 9, HEADER_FORMAT), (M, 28, 1, CHPROC)):
        x = sla_amd.Index.build(reheader(src.data, lambda d: d.__setitem__(k, v)))
        assert x.header_result == 0
        rc, lay = sla_amd.splice_plan([(None, x, 0, 10)])
        assert rc == want and zero(lay), (k, v)


def test_refusals_past_the_extent(L):
    A = SM.sources()["eight24"][0]
    xa, N = index_of(A), A.num_samples
    assert sla_amd.splice_plan([(None, xa, 0, N)])[0] == OK
    assert sla_amd.splice_plan([(None, xa, N, 0)])[0] == OK and sla_amd.splice_plan([(None, xa, N + 5, 0)])[0] == OK
    for s, l in ((0, N + 1), (N, 1), (N - 1, 2), (0xFFFFFFFF, 0xFFFFFFFF), (1, 0xFFFFFFFF)):
        rc, lay = sla_amd.splice_plan([(None, xa, 0, 5), (None, xa, s, l)])
        assert rc == DATA and zero(lay), (s, l)
    cut = sla_amd.Index.build(A.data[:A.offsets[4] + 20])                  # the chain ends inside block 4
    lost = sla_amd.Index.build(A.data[:A.offsets[4]] + b"\x7f" + A.data[A.offsets[4] + 1:])
    ext = sum(b.n for b in A.blocks[:4])
    for x, stop in ((cut, DATA), (lost, SYNC_LOST)):
        assert (x.stop, x.extent) == (stop, ext)
        rc, lay = sla_amd.splice_plan([(None, x, 0, ext)])
        assert rc == OK and lay.num_blocks == 4 and lay.edge_blocks == 0
        assert sla_amd.splice_plan([(None, x, 0, ext + 1)])[0] == stop
        assert sla_amd.splice_plan([(None, x, ext, 1)])[0] == stop


def test_totals_beyond_32_bits(L):
    fmt = SS.Format(1, 16, max_block=16384)
    silent = SS.write_file(fmt, [SS.Block(SS.SILENT, 60000)] * 8)[0]          # samples overflow long before bytes
    loud = CC.by_name()["lengths_lms4"].data                                  # bytes overflow before samples
    for data, by_samples in ((silent, True), (loud, False)):
        x = sla_amd.Index.build(data)
        N, nb = x.extent, x.num_blocks
        fits = 0xFFFFFFFF // N if by_samples else (0xFFFFFFFF - 43) // (len(data) - 43)
        segs = np.zeros(fits + 1, SEG_DTYPE)
        segs["index"], segs["data_size"], segs["length"] = x.handle.value, len(data), N
        item, lay = sla_amd.SpliceItem(), sla_amd.SpliceLayout()
        item.segments = C.cast(segs.ctypes.data, C.POINTER(sla_amd.SpliceSegment))
        item.num_segments = fits
        assert L.sla_hip_splice_plan(C.byref(item), C.byref(lay)) == OK
        assert lay.num_samples == fits * N and lay.num_blocks == fits * nb and lay.edge_blocks == 0
        assert lay.bytes == 43 + fits * (len(data) - 43) == 43 + lay.verbatim_bytes
        item.num_segments = fits + 1
        assert L.sla_hip_splice_plan(C.byref(item), C.byref(lay)) == CAPACITY and zero(lay)
