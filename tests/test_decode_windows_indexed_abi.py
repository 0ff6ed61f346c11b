"""CPU-only checks of the ABI of the indexed window decode (sla_hip_decode_windows_indexed, sla_hip_launch_dec_judge and the
sla_hip_index_* entry points; include/sla_hip.h): the layouts of the item, outcome, judge and index structs, the header's
declarations, the exported symbols and Python methods, and the argument checks that return before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_decode_windows_indexed", "sla_hip_launch_dec_judge", "sla_hip_index_build", "sla_hip_index_build_resident",
         "sla_hip_index_info", "sla_hip_index_blocks", "sla_hip_index_destroy", "sla_hip_index_serialized_bytes",
         "sla_hip_index_serialize", "sla_hip_index_deserialize")
STRUCTS = (("sla_hip_indexed_window_item", "IndexedWindowItem"), ("sla_hip_window_outcome", "WindowOutcome"),
           ("sla_hip_dec_judge_item", "DecJudgeItem"), ("sla_hip_index_block", "IndexBlock"), ("sla_hip_dec_emit", "DecEmit"))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def _layout(S):
    return [(name, getattr(S, name).offset) for name, _ in S._fields_]


def test_struct_layouts():
    assert C.sizeof(sla_amd.IndexedWindowItem) == 56
    assert _layout(sla_amd.IndexedWindowItem) == [
        ("data", 0), ("dst", 8), ("channel_stride", 16), ("sample_stride", 24), ("index", 32), ("data_size", 40), ("start", 44),
        ("length", 48), ("reserved", 52)]
    assert C.sizeof(sla_amd.WindowOutcome) == 8
    assert _layout(sla_amd.WindowOutcome) == [("result", 0), ("output_num_samples", 4)]
    assert C.sizeof(sla_amd.DecJudgeItem) == 32
    assert _layout(sla_amd.DecJudgeItem) == [("first", 0), ("nb", 4), ("stop", 8), ("ok_samples", 12), ("outcome", 16), ("emit", 20),
                                             ("fill_end", 24), ("reserved", 28)]
    assert C.sizeof(sla_amd.IndexBlock) == 16 and sla_amd.INDEX_BLOCK_DTYPE.itemsize == 16
    assert [n for n, _ in sla_amd.IndexBlock._fields_] == list(sla_amd.INDEX_BLOCK_DTYPE.names)
    assert C.sizeof(sla_amd.DecEmit) == 56 and sla_amd.DecEmit.done.offset == 32 and sla_amd.DecEmit.fill_end.offset == 36
    assert C.sizeof(sla_amd.IndexSummary) == 24 + C.sizeof(sla_amd.SLAHeaderInfo) and sla_amd.IndexSummary.header.offset == 24
    # the synchronous call's item is as it was
    assert C.sizeof(sla_amd.DecodeWindowItem) == 72


def test_header_declares_the_structs_field_by_field():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name, py in STRUCTS:
        S = getattr(sla_amd, py)
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        fields = re.findall(r"(\w+);", body)
        assert fields == [f for f, _ in S._fields_], name
        widths = {"uint64_t": 8, "uint32_t": 4, "int32_t": 4}
        decls = re.findall(r"\s*([^;]*?\S)\s+(\w+);", body)
        assert [n for _, n in decls] == fields, name
        for (decl, _), (fname, ctype) in zip(decls, S._fields_):
            want = 8 if "*" in decl else widths[decl.split()[-1]]
            assert C.sizeof(ctype) == want, (name, fname, decl)


def test_header_declares_the_entry_points_and_states_the_contract():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    assert "THE HOST MAY WAIT in two places only" in text and "AN INDEX IS THE CALLER'S PROMISE" in text
    assert int(re.search(r"#define SLA_HIP_DEC_QUEUE_SLOTS (\d+)u", text).group(1)) == sla_amd.DEC_QUEUE_SLOTS
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "decode_windows_indexed" in open(os.path.join(ROOT, doc)).read(), doc


def test_symbols_are_exported_and_the_methods_exist(L):
    for name in NAMES:
        assert hasattr(L, name), name
    for name in ("index_resident", "decode_windows_indexed_into", "decode_windows_indexed", "block_index_resident", "decode_windows_tensor"):
        assert hasattr(sla_amd.Decoder, name), name
    for name in ("build", "from_bytes", "to_bytes", "blocks", "header", "header_result", "stop", "extent", "num_blocks"):
        assert hasattr(sla_amd.Index, name), name


def _items(n=2):
    items = (sla_amd.IndexedWindowItem * n)()
    for i in range(n):
        items[i].data = C.cast(C.c_void_p(0x2000), sla_amd.u8p)
        items[i].data_size = 64
        items[i].dst = 0x1000
        items[i].channel_stride = 16
        items[i].sample_stride = 1
        items[i].index = 0x3000
        items[i].start = 5
        items[i].length = 16
    return items


def test_call_level_errors_queue_nothing(L):
    items = _items()
    before = bytes(items)
    f = L.sla_hip_decode_windows_indexed
    out = C.c_void_p(0x4000)
    assert f(None, items, 2, sla_amd.PCM_F32, 0, out, None) == INVALID_ARGUMENT
    assert f(None, None, 0, sla_amd.PCM_F32, 0, out, None) == INVALID_ARGUMENT
    # NULL outcomes, a bad format, bad flags or NULL items with a count are refused before the handle is looked at: a
    # dangling handle value shows that nothing behind it is read
    bogus = C.c_void_p(0x10)
    assert f(bogus, items, 2, sla_amd.PCM_F32, 0, None, None) == INVALID_ARGUMENT
    assert f(bogus, items, 2, 4, 0, out, None) == INVALID_ARGUMENT
    assert f(bogus, items, 2, 0xFFFFFFFF, 0, out, None) == INVALID_ARGUMENT
    assert f(bogus, items, 2, sla_amd.PCM_S16, 2, out, None) == INVALID_ARGUMENT
    assert f(bogus, items, 2, sla_amd.PCM_S16, 0x80000001, out, None) == INVALID_ARGUMENT
    assert f(bogus, None, 3, sla_amd.PCM_S16, 0, out, None) == INVALID_ARGUMENT
    assert bytes(items) == before


def test_index_entry_points_refuse_null_arguments(L):
    h = C.c_void_p(0x55)
    a = np.zeros(64, np.uint8)
    assert L.sla_hip_index_build(None, 64, C.byref(h)) == INVALID_ARGUMENT
    assert L.sla_hip_index_build(a.ctypes.data, 64, None) == INVALID_ARGUMENT
    assert L.sla_hip_index_build_resident(None, a.ctypes.data, 64, None, C.byref(h)) == INVALID_ARGUMENT
    assert L.sla_hip_index_build_resident(C.c_void_p(0x10), None, 64, None, C.byref(h)) == INVALID_ARGUMENT
    assert L.sla_hip_index_build_resident(C.c_void_p(0x10), a.ctypes.data, 64, None, None) == INVALID_ARGUMENT
    assert L.sla_hip_index_info(None, C.byref(sla_amd.IndexSummary())) == INVALID_ARGUMENT
    assert L.sla_hip_index_blocks(None, 0, 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_index_serialized_bytes(None) == 0 and L.sla_hip_index_serialize(None, a.ctypes.data, 64) == 0
    L.sla_hip_index_destroy(None)
    x = sla_amd.Index.build(bytes(a))                     # 64 zero bytes: no header, no rows
    assert (x.header, x.header_result, x.num_blocks, x.stop, x.extent) == (None, 10, 0, 0, 0)
    assert L.sla_hip_index_info(x.handle, None) == INVALID_ARGUMENT
    assert L.sla_hip_index_serialize(x.handle, a.ctypes.data, 10) == 0               # too small: nothing written
    assert not a.any()


def test_judge_launcher_refuses_null_tables(L):
    a = np.zeros(256, np.uint8)
    p = a.ctypes.data
    judge = L.sla_hip_launch_dec_judge
    assert judge(p, 256, p, p, 1, None, 1, 1, 1, p, 1, p, 1, None) == INVALID_ARGUMENT      # no item table
    assert judge(p, 256, p, p, 1, p, 1, 1, 1, p, 1, None, 1, None) == INVALID_ARGUMENT      # no outcome table
    assert judge(p, 256, p, p, 1, p, 1, 1, 1, None, 1, p, 1, None) == INVALID_ARGUMENT      # emit entries without a table
    for tables in ((None, p, p), (p, None, p), (p, p, None)):
        assert judge(tables[0], 256, tables[1], tables[2], 1, p, 1, 1, 1, p, 1, p, 1, None) == INVALID_ARGUMENT, tables
