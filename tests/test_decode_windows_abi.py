"""CPU-only checks of the window decode ABI (sla_hip_decode_windows_resident, sla_hip_launch_dec_walk_window,
sla_hip_decoder_last_window_stats; include/sla_hip.h): the layouts of the item struct and of the two walk structs, the
header's declarations, the exported symbols and Python methods, and the argument checks that return before any device
work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_decode_windows_resident", "sla_hip_launch_dec_walk_window", "sla_hip_decoder_last_window_stats")
STRUCTS = (("sla_hip_dec_window_file", "DecWindowFile"), ("sla_hip_dec_window_result", "DecWindowResult"),
           ("sla_hip_decode_window_item", "DecodeWindowItem"))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def _layout(S):
    return [(name, getattr(S, name).offset) for name, _ in S._fields_]


def test_struct_layouts():
    assert C.sizeof(sla_amd.DecodeWindowItem) == 72
    assert _layout(sla_amd.DecodeWindowItem) == [
        ("data", 0), ("dst", 8), ("channel_stride", 16), ("sample_stride", 24), ("data_size", 32), ("start", 36), ("length", 40),
        ("seek_byte", 44), ("seek_sample", 48), ("output_num_samples", 52), ("result", 56), ("first_block_byte", 60),
        ("first_block_sample", 64), ("reserved", 68)]
    assert C.sizeof(sla_amd.DecWindowFile) == 64
    assert _layout(sla_amd.DecWindowFile) == [
        ("src", 0), ("img_off", 8), ("data_size", 16), ("total", 20), ("win_start", 24), ("win_len", 28), ("seek_byte", 32),
        ("seek_sample", 36), ("range_bytes", 40), ("base_byte", 44), ("base_sample", 48), ("plane_off", 52), ("first", 56),
        ("max_rows", 60)]
    assert C.sizeof(sla_amd.DecWindowResult) == 32
    assert _layout(sla_amd.DecWindowResult) == [
        ("num_blocks", 0), ("stop", 4), ("skipped", 8), ("first_byte", 12), ("first_sample", 16), ("end_byte", 20),
        ("end_sample", 24), ("reserved", 28)]
    # the walk structs of the whole-file walk are as they were
    assert C.sizeof(sla_amd.DecWalkFile) == 40 and C.sizeof(sla_amd.DecWalkResult) == 16


def test_header_declares_the_structs_field_by_field():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name, py in STRUCTS:
        S = getattr(sla_amd, py)
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        fields = re.findall(r"(\w+);", body)
        assert fields == [f for f, _ in S._fields_], name
        # every field is 4 or 8 bytes wide and the C types say the same
        widths = {"uint64_t": 8, "uint32_t": 4, "int32_t": 4}
        decls = re.findall(r"^\s*(\S.*?)\s+(\w+);", body, flags=re.M)
        assert [n for _, n in decls] == fields, name
        for (decl, _), (fname, ctype) in zip(decls, S._fields_):
            want = 8 if "*" in decl else widths[decl.split()[-1]]
            assert C.sizeof(ctype) == want, (name, fname, decl)


def test_header_declares_the_entry_points_and_says_what_windows_do_not_do():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    assert "NO RESYNC" in text and "NOT SEEN" in text
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "decode_windows" in open(os.path.join(ROOT, doc)).read(), doc


def test_symbols_are_exported_and_the_methods_exist(L):
    for name in NAMES:
        assert hasattr(L, name), name
    for name in ("decode_windows_into", "decode_windows_tensor", "block_index_resident", "last_window_stats"):
        assert hasattr(sla_amd.Decoder, name), name


def _items(n=2):
    items = (sla_amd.DecodeWindowItem * n)()
    for i in range(n):
        items[i].data = C.cast(C.c_void_p(0x2000), sla_amd.u8p)
        items[i].data_size = 64
        items[i].dst = 0x1000
        items[i].channel_stride = 16
        items[i].sample_stride = 1
        items[i].start = 5
        items[i].length = 16
        items[i].output_num_samples = 777
        items[i].result = -7
        items[i].first_block_byte = 555
        items[i].first_block_sample = 444
    return items


def _untouched(items):
    return all(it.result == -7 and it.output_num_samples == 777 and it.first_block_byte == 555 and it.first_block_sample == 444
               for it in items)


def test_call_level_errors_leave_the_items_untouched(L):
    items = _items()
    f = L.sla_hip_decode_windows_resident
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


def test_window_stats_refuses_null_arguments(L):
    c = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert L.sla_hip_decoder_last_window_stats(None, c) == INVALID_ARGUMENT
    assert L.sla_hip_decoder_last_window_stats(C.c_void_p(0x10), None) == INVALID_ARGUMENT
    assert list(c) == [9, 9, 9, 9]


def test_launcher_refuses_null_tables(L):
    a = np.zeros(256, np.uint8)
    p = a.ctypes.data
    walk = L.sla_hip_launch_dec_walk_window
    assert walk(None, 1, 4096, p, None, None, None, None) == INVALID_ARGUMENT          # no file table
    assert walk(p, 1, 4096, None, None, None, None, None) == INVALID_ARGUMENT          # no result table
    assert walk(None, 0, 4096, None, None, None, None, None) == INVALID_ARGUMENT
    for tables in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
        assert walk(p, 1, 4096, p, *tables, None) == INVALID_ARGUMENT, tables             # write mode, a table missing
