"""CPU-only checks of the device-resident encode route (include/sla_hip.h): the emit table's layout, the three entry points
in the header, in EXPORTED_SYMBOLS and in the library, the sample-format constants the item struct is shared with, and the
refusals that return before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_encode_batch_resident", "sla_hip_pack_resident", "sla_hip_launch_enc_emit_batch")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def header_text():
    return open(os.path.join(ROOT, "include", "sla_hip.h")).read()


def test_emit_entry_is_72_bytes_with_the_documented_offsets():
    E = sla_amd.EncEmit
    assert C.sizeof(E) == 72
    assert [(n, getattr(E, n).offset, getattr(E, n).size) for n, _ in E._fields_] == \
        [("img_off", 0, 8), ("dst", 8, 8), ("bytes", 16, 4), ("header_bytes", 20, 4), ("header", 24, 48)]
    # the header's struct, field by field in the same order
    m = re.search(r"typedef struct sla_hip_enc_emit \{(.*?)\} sla_hip_enc_emit;", header_text(), re.S)
    assert m
    decl = re.findall(r"^\s*(\w+\*?)\s+(\w+)(?:\[(\d+)\])?;", m.group(1), re.M)
    assert decl == [("uint64_t", "img_off", ""), ("uint8_t*", "dst", ""), ("uint32_t", "bytes", ""),
                    ("uint32_t", "header_bytes", ""), ("uint8_t", "header", "48")]


def test_header_declares_the_entry_points():
    text = header_text()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    assert re.search(r"sla_hip_encode_batch_resident\(struct SLAEncoder\* encoder, sla_hip_encode_device_item\* items, "
                     r"uint32_t num_items,\s*uint32_t sample_format, uint8_t\* d_arena, uint64_t arena_bytes, "
                     r"sla_hip_stream_t stream\);", text)
    assert re.search(r"sla_hip_pack_resident\(struct SLAEncoder\* encoder, uint8_t\* d_data, uint32_t data_size, "
                     r"uint32_t\* output_size\);", text)


def test_entry_points_are_exported(L):
    for name in NAMES:
        assert hasattr(L, name), name
    for method in ("encode_resident_from", "encode_resident_tensor", "pack_resident"):
        assert hasattr(sla_amd.Encoder, method), method


def test_still_four_sample_formats():
    # the resident call shares sla_hip_encode_batch_device's item struct and formats: no new constant
    assert re.findall(r"^#define (SLA_HIP_PCM_\w+)", header_text(), re.M) == \
        ["SLA_HIP_PCM_S32_LEFT", "SLA_HIP_PCM_S32", "SLA_HIP_PCM_S16", "SLA_HIP_PCM_F32"]


def test_call_level_refusals_touch_no_item(L):
    items = (sla_amd.EncodeDeviceItem * 2)()
    for it in items:
        it.src = 0x1000; it.channel_stride = 64; it.sample_stride = 1; it.num_samples = 64
        it.data = C.cast(C.c_void_p(0x2000), sla_amd.u8p); it.data_size = 999
        it.output_size = 777; it.result = -7
    # a dangling handle value shows that nothing behind it is read when another argument already refuses the call
    bogus = C.c_void_p(0x10)
    for arena, size in ((None, 0), (C.c_void_p(0x3000), 4096)):
        assert L.sla_hip_encode_batch_resident(None, items, 2, 0, arena, size, None) == INVALID_ARGUMENT
        assert L.sla_hip_encode_batch_resident(bogus, None, 2, 0, arena, size, None) == INVALID_ARGUMENT
        assert L.sla_hip_encode_batch_resident(bogus, items, 2, 4, arena, size, None) == INVALID_ARGUMENT
    for it in items:
        assert (it.result, it.output_size, it.data_size, C.cast(it.data, C.c_void_p).value) == (-7, 777, 999, 0x2000)
    size = C.c_uint32(55)
    assert L.sla_hip_pack_resident(None, C.c_void_p(0x2000), 100, C.byref(size)) == INVALID_ARGUMENT
    assert size.value == 55


def test_emit_launcher_refuses_a_null_table_or_image(L):
    mem = np.zeros(256, np.uint8)
    p = mem.ctypes.data
    assert L.sla_hip_launch_enc_emit_batch(None, 1, 64, p, 256, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_enc_emit_batch(p, 1, 64, None, 256, None) == INVALID_ARGUMENT
    # the checks come first: an empty table with a missing argument is refused too, a good empty table launches nothing
    assert L.sla_hip_launch_enc_emit_batch(None, 0, 0, p, 256, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_enc_emit_batch(p, 0, 0, p, 256, None) == 0
    assert L.sla_hip_launch_enc_emit_batch(p, 3, 0, p, 256, None) == 0
    assert (mem == 0).all()
