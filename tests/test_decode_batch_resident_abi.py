"""CPU-only checks of the resident batch decode ABI (sla_hip_decode_batch_resident, sla_hip_resident_headers,
sla_hip_launch_dec_walk, sla_hip_launch_dec_gather; include/sla_hip.h): the layouts of the two walk structs and of the
gather struct, the header's entry points, the exported symbols, and the argument checks that return before any device
work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_decode_batch_resident", "sla_hip_resident_headers", "sla_hip_launch_dec_walk", "sla_hip_launch_dec_gather")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def _layout(S):
    return [(name, getattr(S, name).offset) for name, _ in S._fields_]


def test_struct_layouts():
    assert C.sizeof(sla_amd.DecWalkFile) == 40
    assert _layout(sla_amd.DecWalkFile) == [("src", 0), ("img_off", 8), ("data_size", 16), ("total", 20), ("capacity", 24),
                                            ("first", 28), ("max_rows", 32), ("plane_off", 36)]
    assert C.sizeof(sla_amd.DecWalkResult) == 16
    assert _layout(sla_amd.DecWalkResult) == [("num_blocks", 0), ("stop", 4), ("extent", 8), ("reserved", 12)]
    assert C.sizeof(sla_amd.DecGather) == 24
    assert _layout(sla_amd.DecGather) == [("src", 0), ("dst_off", 8), ("bytes", 16), ("reserved", 20)]
    assert C.sizeof(sla_amd.DecodeDeviceItem) == 48                # the item struct is the device call's, unchanged


def test_header_declares_the_structs_field_by_field():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name, S in (("sla_hip_dec_walk_file", sla_amd.DecWalkFile), ("sla_hip_dec_walk_result", sla_amd.DecWalkResult),
                    ("sla_hip_dec_gather", sla_amd.DecGather)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        fields = re.findall(r"(\w+);", body)
        assert fields == [f for f, _ in S._fields_], name


def test_header_declares_the_resident_entry_points():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    for doc in ("README.md", "DESIGN.md"):
        assert "sla_hip_decode_batch_resident" in open(os.path.join(ROOT, doc)).read(), doc


def test_resident_symbols_are_exported(L):
    for name in NAMES:
        assert hasattr(L, name), name
    for name in ("decode_resident_into", "decode_resident_tensor", "resident_headers"):
        assert hasattr(sla_amd.Decoder, name), name


def _items(n=2):
    items = (sla_amd.DecodeDeviceItem * n)()
    for i in range(n):
        items[i].data = C.cast(C.c_void_p(0x2000), sla_amd.u8p)
        items[i].data_size = 64
        items[i].dst = 0x1000
        items[i].channel_stride = 16
        items[i].sample_stride = 1
        items[i].capacity = 16
        items[i].output_num_samples = 777
        items[i].result = -7
    return items


def _untouched(items):
    return all(it.result == -7 and it.output_num_samples == 777 for it in items)


def test_call_level_errors_leave_the_items_untouched(L):
    items = _items()
    f = L.sla_hip_decode_batch_resident
    assert f(None, items, 2, sla_amd.PCM_F32, 0, None) == INVALID_ARGUMENT
    assert _untouched(items)
    assert f(None, None, 0, sla_amd.PCM_F32, 0, None) == INVALID_ARGUMENT
    # a bad format, bad flags or NULL items with a count are refused before the handle is looked at: a dangling
    # handle value shows that nothing behind it is read
    bogus = C.c_void_p(0x10)
    assert f(bogus, items, 2, 4, 0, None) == INVALID_ARGUMENT
    assert f(bogus, items, 2, 0xFFFFFFFF, 0, None) == INVALID_ARGUMENT
    assert f(bogus, items, 2, sla_amd.PCM_S16, 2, None) == INVALID_ARGUMENT
    assert f(bogus, items, 2, sla_amd.PCM_S16, 0x80000001, None) == INVALID_ARGUMENT
    assert f(bogus, None, 3, sla_amd.PCM_S16, 0, None) == INVALID_ARGUMENT
    assert _untouched(items)


def test_resident_headers_refuses_null_arguments(L):
    f = L.sla_hip_resident_headers
    ptrs = (C.c_void_p * 1)(0x2000)
    sizes = (C.c_uint32 * 1)(64)
    hdrs = (sla_amd.SLAHeaderInfo * 1)()
    codes = (C.c_int32 * 1)(-7)
    assert f(None, ptrs, sizes, 1, hdrs, codes, None) == INVALID_ARGUMENT
    bogus = C.c_void_p(0x10)
    assert f(bogus, None, sizes, 1, hdrs, codes, None) == INVALID_ARGUMENT
    assert f(bogus, ptrs, None, 1, hdrs, codes, None) == INVALID_ARGUMENT
    assert f(bogus, ptrs, sizes, 1, None, codes, None) == INVALID_ARGUMENT
    assert f(bogus, ptrs, sizes, 1, hdrs, None, None) == INVALID_ARGUMENT
    assert codes[0] == -7


def test_launchers_refuse_null_tables(L):
    a = np.zeros(256, np.uint8)
    p = a.ctypes.data
    walk, gather = L.sla_hip_launch_dec_walk, L.sla_hip_launch_dec_gather
    assert walk(None, 1, 4096, 1, p, None, None, None, None) == INVALID_ARGUMENT          # no file table
    assert walk(p, 1, 4096, 1, None, None, None, None, None) == INVALID_ARGUMENT          # no result table
    assert walk(None, 0, 4096, 1, None, None, None, None, None) == INVALID_ARGUMENT
    for tables in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
        assert walk(p, 1, 4096, 1, p, *tables, None) == INVALID_ARGUMENT, tables             # write mode, a table missing
    assert gather(None, 1, 16, p, 256, None) == INVALID_ARGUMENT
    assert gather(p, 1, 16, None, 256, None) == INVALID_ARGUMENT
    assert gather(None, 0, 0, None, 0, None) == INVALID_ARGUMENT
