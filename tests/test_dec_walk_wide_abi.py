"""CPU-only checks of the wide walk's ABI (sla_hip_launch_dec_walk_wide, sla_hip_dec_wide_scratch_bytes,
sla_hip_dec_wide_rounds; sla_hip_decoder_set_option, sla_hip_decoder_last_walk): the symbols, the struct layouts the launcher
shares with the lane walk, the scratch macro against its Python copy, and the argument checks that return before any
device work."""
import ctypes as C
import os
import re

import pytest

import sla_amd
import widewalkmodel as WW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_launch_dec_walk_wide", "sla_hip_dec_wide_scratch_bytes", "sla_hip_dec_wide_rounds",
         "sla_hip_decoder_set_option", "sla_hip_decoder_last_walk")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def test_symbols_are_exported_declared_and_wrapped(L):
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read() + open(os.path.join(ROOT, "include", "SLADecoder.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, text), name
    for name in ("set_option", "last_walk", "block_index_resident"):
        assert hasattr(sla_amd.Decoder, name), name
    assert "SLA_HIP_DEC_WIDE_OVERFLOW 1u" in text and "SLA_HIP_DEC_WIDE_SCRATCH_BYTES(data_size, node_capacity)" in text
    assert "there is no second walker" not in text


def test_python_knows_the_default_threshold():
    text = open(os.path.join(ROOT, "sla_amd", "csrc", "sla_decoder.c")).read()
    m = re.search(r"#define DEC_WIDE_WALK_DEFAULT (\d+)u", text)
    assert m and int(m.group(1)) == sla_amd.WIDE_WALK_DEFAULT
    # the default follows from the recorded measurement: the smallest rung at which wide took at most half the lane's time
    import json
    rungs = json.load(open(os.path.join(ROOT, "profiles", "walk_wide.json")))["count_mode_walks"]
    pays = [r["stream_bytes"] for r in rungs if 2 * r["wide_ms"] <= r["lane_ms"]]
    assert pays and abs(pays[0] - sla_amd.WIDE_WALK_DEFAULT) <= pays[0] // 100


def test_struct_sizes_are_unchanged():
    assert C.sizeof(sla_amd.DecWalkFile) == 40 and C.sizeof(sla_amd.DecWalkResult) == 16
    assert [(n, getattr(sla_amd.DecWalkFile, n).offset) for n, _ in sla_amd.DecWalkFile._fields_] == [
        ("src", 0), ("img_off", 8), ("data_size", 16), ("total", 20), ("capacity", 24), ("first", 28), ("max_rows", 32), ("plane_off", 36)]
    assert [(n, getattr(sla_amd.DecWalkResult, n).offset) for n, _ in sla_amd.DecWalkResult._fields_] == [
        ("num_blocks", 0), ("stop", 4), ("extent", 8), ("reserved", 12)]
    assert C.sizeof(sla_amd.DecWideInfo) == 16
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    m = re.search(r"typedef struct sla_hip_dec_wide_info \{(.*?)\} sla_hip_dec_wide_info;", text, flags=re.S)
    assert re.findall(r"uint32_t (\w+);", m.group(1)) == [n for n, _ in sla_amd.DecWideInfo._fields_]


def test_scratch_macro_agrees_with_its_python_copy(L):
    for size in (0, 53, 54, 4096, 8176, 8177, 8178, 1 << 20, 82 * 1000 * 1000, 0xFFFFFFFF):
        for cap in (1, 2, 3, 4, 5, 1 << 16, 0xFFFFFFFF):
            got = L.sla_hip_dec_wide_scratch_bytes(size, cap)
            assert got == WW.scratch_bytes(size, cap) and got % 16 == 0, (size, cap)
            assert L.sla_hip_dec_wide_rounds(size, cap) == WW.rounds(size, cap), (size, cap)
    # the parts: 64 bytes of info words, 2048 bytes per tile of 8192 positions, 4 per tile (padded), 64 per node
    assert WW.scratch_bytes(54, 4) == 64 + 2048 + 16 + 256
    assert WW.scratch_bytes(8177, 4) == 64 + 2048 + 16 + 256 and WW.scratch_bytes(8178, 4) == 64 + 4096 + 16 + 256


def test_launcher_refuses_before_any_launch(L):
    f = sla_amd.DecWalkFile()
    f.src, f.data_size, f.total, f.capacity, f.max_rows = 0x7000, 4096, 100, 100, 4
    p, s = C.c_void_p(0x1000), C.c_void_p(0x2000)
    W = L.sla_hip_launch_dec_walk_wide
    assert W(None, 4096, 1, p, None, None, None, 64, s, None) == INVALID_ARGUMENT
    assert W(C.byref(f), 4096, 1, None, None, None, None, 64, s, None) == INVALID_ARGUMENT
    assert W(C.byref(f), 4096, 1, p, None, None, None, 64, None, None) == INVALID_ARGUMENT
    assert W(C.byref(f), 4096, 1, p, None, None, None, 0, s, None) == INVALID_ARGUMENT
    for off in (1, 4, 8, 15):
        assert W(C.byref(f), 4096, 1, p, None, None, None, 64, C.c_void_p(0x2000 + off), None) == INVALID_ARGUMENT
    for tabs in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
        assert W(C.byref(f), 4096, 1, p, *tabs, 64, s, None) == INVALID_ARGUMENT, tabs


def test_handle_calls_refuse_null_arguments(L):
    c = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert L.sla_hip_decoder_last_walk(None, c) == INVALID_ARGUMENT
    assert L.sla_hip_decoder_last_walk(C.c_void_p(0x10), None) == INVALID_ARGUMENT
    assert list(c) == [9, 9, 9, 9]
    assert L.sla_hip_decoder_set_option(None, b"wide_walk", 1.0) == INVALID_ARGUMENT
    assert L.sla_hip_decoder_set_option(C.c_void_p(0x10), None, 1.0) == INVALID_ARGUMENT
    # a value out of range is refused before the handle is touched: a dangling handle value shows it
    for bad in (-1.0, 0.5, 4294967296.0, float("nan"), float("inf")):
        assert L.sla_hip_decoder_set_option(C.c_void_p(0x10), b"wide_walk", bad) == INVALID_ARGUMENT
