"""CPU-only checks of the device-destination batch decode ABI (sla_hip_decode_batch_device, include/sla_hip.h): the
item struct's layout, the header's entry points, formats and flag, the exported symbols, and the call-level argument
checks that return before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_decode_batch_device", "sla_hip_launch_dec_emit_batch")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def test_decode_device_item_layout():
    D = sla_amd.DecodeDeviceItem
    assert C.sizeof(D) == 48
    assert [(name, getattr(D, name).offset) for name, _ in D._fields_] == [
        ("data", 0), ("dst", 8), ("channel_stride", 16), ("sample_stride", 24), ("data_size", 32), ("capacity", 36),
        ("output_num_samples", 40), ("result", 44)]


def test_header_declares_the_device_batch_entry_points():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    for name, value in (("SLA_HIP_PCM_S32_LEFT", 0), ("SLA_HIP_PCM_S32", 1), ("SLA_HIP_PCM_S16", 2), ("SLA_HIP_PCM_F32", 3),
                        ("SLA_HIP_DEC_ZERO_FILL", 1)):
        m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, text)
        assert m and int(m.group(1)) == value, name
    assert (sla_amd.PCM_S32_LEFT, sla_amd.PCM_S32, sla_amd.PCM_S16, sla_amd.PCM_F32, sla_amd.DEC_ZERO_FILL) == (0, 1, 2, 3, 1)
    assert re.search(r"typedef struct sla_hip_decode_device_item\b", text)


def test_device_batch_symbols_are_exported(L):
    for name in NAMES:
        assert hasattr(L, name), name


def _items(n=2):
    data = np.zeros(64, np.uint8)
    items = (sla_amd.DecodeDeviceItem * n)()
    for i in range(n):
        items[i].data = data.ctypes.data_as(sla_amd.u8p)
        items[i].data_size = len(data)
        items[i].dst = 0x1000
        items[i].channel_stride = 16
        items[i].sample_stride = 1
        items[i].capacity = 16
        items[i].output_num_samples = 777
        items[i].result = -7
    return data, items


def _untouched(items):
    return all(it.result == -7 and it.output_num_samples == 777 for it in items)


def test_call_level_errors_leave_the_items_untouched(L):
    data, items = _items()
    assert L.sla_hip_decode_batch_device(None, items, 2, sla_amd.PCM_F32, 0, None) == INVALID_ARGUMENT
    assert _untouched(items)
    assert L.sla_hip_decode_batch_device(None, None, 0, sla_amd.PCM_F32, 0, None) == INVALID_ARGUMENT
    # a bad format, bad flags or NULL items with a count are refused before the handle is looked at: a dangling
    # handle value shows that nothing behind it is read
    bogus = C.c_void_p(0x10)
    assert L.sla_hip_decode_batch_device(bogus, items, 2, 4, 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_decode_batch_device(bogus, items, 2, 0xFFFFFFFF, 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_decode_batch_device(bogus, items, 2, sla_amd.PCM_S16, 2, None) == INVALID_ARGUMENT
    assert L.sla_hip_decode_batch_device(bogus, items, 2, sla_amd.PCM_S16, 0x80000001, None) == INVALID_ARGUMENT
    assert L.sla_hip_decode_batch_device(bogus, None, 3, sla_amd.PCM_S16, 0, None) == INVALID_ARGUMENT
    assert _untouched(items)


def test_emit_launcher_rejects_null_pointers(L):
    table = np.zeros(64, np.uint8)
    planes = np.zeros(64, np.int32)
    assert L.sla_hip_launch_dec_emit_batch(None, 0, None, 0, 0, 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_dec_emit_batch(None, 16, table.ctypes.data, 1, 16, 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_dec_emit_batch(planes.ctypes.data, 16, None, 1, 16, 0, None) == INVALID_ARGUMENT
    # an unknown format is refused before any launch
    assert L.sla_hip_launch_dec_emit_batch(planes.ctypes.data, 16, table.ctypes.data, 1, 16, 4, None) == INVALID_ARGUMENT
