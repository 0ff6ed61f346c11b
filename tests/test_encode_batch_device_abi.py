"""CPU-only checks of the device-source batch encode ABI (sla_hip_encode_batch_device, include/sla_hip.h): the item
struct's layout, the header's entry points and table, the exported symbols, and the call-level argument checks that
return before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_encode_batch_device", "sla_hip_launch_enc_ingest_batch")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def test_encode_device_item_layout():
    E = sla_amd.EncodeDeviceItem
    assert C.sizeof(E) == 48
    assert [(name, getattr(E, name).offset) for name, _ in E._fields_] == [
        ("src", 0), ("channel_stride", 8), ("sample_stride", 16), ("data", 24), ("num_samples", 32), ("data_size", 36),
        ("output_size", 40), ("result", 44)]


def test_header_declares_the_device_encode_entry_points():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    assert re.search(r"typedef struct sla_hip_encode_device_item\b", text)
    assert re.search(r"typedef struct sla_hip_enc_ingest\b", text)
    # the formats are the decode side's, no new constants
    assert len(re.findall(r"#define\s+SLA_HIP_PCM_\w+", text)) == 4


def test_device_encode_symbols_are_exported(L):
    for name in NAMES:
        assert hasattr(L, name), name


def _items(n=2):
    out = np.zeros(64, np.uint8)
    items = (sla_amd.EncodeDeviceItem * n)()
    for i in range(n):
        items[i].src = 0x1000
        items[i].channel_stride = 16
        items[i].sample_stride = 1
        items[i].data = out.ctypes.data_as(sla_amd.u8p)
        items[i].data_size = len(out)
        items[i].num_samples = 16
        items[i].output_size = 777
        items[i].result = -7
    return out, items


def _untouched(items):
    return all(it.result == -7 and it.output_size == 777 for it in items)


def test_call_level_errors_leave_the_items_untouched(L):
    out, items = _items()
    assert L.sla_hip_encode_batch_device(None, items, 2, sla_amd.PCM_F32, None) == INVALID_ARGUMENT
    assert L.sla_hip_encode_batch_device(None, None, 0, sla_amd.PCM_F32, None) == INVALID_ARGUMENT
    assert _untouched(items)
    # a bad format or NULL items with a count are refused before the handle is looked at: a dangling handle value shows
    # that nothing behind it is read
    bogus = C.c_void_p(0x10)
    assert L.sla_hip_encode_batch_device(bogus, items, 2, 4, None) == INVALID_ARGUMENT
    assert L.sla_hip_encode_batch_device(bogus, items, 2, 0xFFFFFFFF, None) == INVALID_ARGUMENT
    assert L.sla_hip_encode_batch_device(bogus, None, 3, sla_amd.PCM_S16, None) == INVALID_ARGUMENT
    assert _untouched(items) and (out == 0).all()


def test_ingest_launcher_rejects_bad_arguments(L):
    table = np.zeros(64, np.uint8)
    planes = np.zeros(64, np.int32)
    err = np.zeros(4, np.uint32)
    t, p, e = table.ctypes.data, planes.ctypes.data, err.ctypes.data
    assert L.sla_hip_launch_enc_ingest_batch(None, 0, 0, 2, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_enc_ingest_batch(None, 1, 16, 2, 0, p, 16, e, None) == INVALID_ARGUMENT        # no table
    assert L.sla_hip_launch_enc_ingest_batch(t, 1, 16, 2, 0, None, 16, e, None) == INVALID_ARGUMENT        # no planes
    assert L.sla_hip_launch_enc_ingest_batch(t, 1, 16, 2, 0, p, 16, None, None) == INVALID_ARGUMENT        # no error words
    # an unknown format or channel count is refused before any launch
    assert L.sla_hip_launch_enc_ingest_batch(t, 1, 16, 2, 4, p, 16, e, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_enc_ingest_batch(t, 1, 16, 0, 0, p, 16, e, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_enc_ingest_batch(t, 1, 16, 9, 0, p, 16, e, None) == INVALID_ARGUMENT
    assert (planes == 0).all() and (err == 0).all()
