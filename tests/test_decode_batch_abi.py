"""CPU-only checks of the batch decode ABI (sla_hip_decode_batch, include/sla_hip.h): the item struct's layout, the
exported entry points, and the argument checks that return before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def test_decode_item_layout():
    D = sla_amd.DecodeItem
    assert C.sizeof(D) == 32
    assert [(name, getattr(D, name).offset) for name, _ in D._fields_] == [
        ("data", 0), ("data_size", 8), ("buffer_num_samples", 12), ("buffer", 16),
        ("output_num_samples", 24), ("result", 28)]


def test_header_declares_the_batch_entry_points():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in ("sla_hip_decode_batch", "sla_hip_launch_dec_bits_x", "sla_hip_launch_dec_finish_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    assert re.search(r"#define\s+SLA_HIP_DEC_BATCH_PASS\b", text)


def test_batch_symbols_are_exported(L):
    for name in ("sla_hip_decode_batch", "sla_hip_launch_dec_bits_x", "sla_hip_launch_dec_finish_batch"):
        assert hasattr(L, name), name


def test_null_decoder_and_null_items_are_rejected(L):
    data = np.zeros(64, np.uint8)
    out = np.zeros((1, 16), np.int32)
    ptrs = (sla_amd.i32p * 1)(out[0].ctypes.data_as(sla_amd.i32p))
    items = (sla_amd.DecodeItem * 1)()
    items[0].data = data.ctypes.data_as(sla_amd.u8p)
    items[0].data_size = len(data)
    items[0].buffer_num_samples = 16
    items[0].buffer = ptrs
    items[0].result = -7
    assert L.sla_hip_decode_batch(None, items, 1) == INVALID_ARGUMENT
    assert items[0].result == -7                 # nothing was touched
    assert L.sla_hip_decode_batch(None, None, 0) == INVALID_ARGUMENT


def test_launchers_reject_null_pointers(L):
    assert L.sla_hip_launch_dec_bits_x(None, 0, None, 0, 1, 16, 0, 0, 8, 1, 0, None, 0, None, None, None, None,
                                       None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_dec_finish_batch(None, 0, 1, None, 0, 0, None, None) == INVALID_ARGUMENT


def test_dec_bits_lanes_follow_the_rule(L):
    """blocks per wave of k_dec_bits (sla_hip_dec_bits_lanes, the function the launcher calls):
    ceil(num_blocks / 1024), at least 1, at most 64 // channels -- 3, 5, 6 and 7 channels do not divide 64"""
    caps = {1: 64, 2: 32, 3: 21, 4: 16, 5: 12, 6: 10, 7: 9, 8: 8}
    for nch in range(1, 9):
        assert caps[nch] == 64 // nch
        for nb in (1, 1024, 1025, 2048, 2049, 64512, 64513, 10 ** 6):
            want = min(max(-(-nb // 1024), 1), caps[nch])
            assert L.sla_hip_dec_bits_lanes(nb, nch) == want, (nb, nch)
    assert L.sla_hip_dec_bits_lanes(1024, 1) == 1 and L.sla_hip_dec_bits_lanes(1025, 1) == 2
    assert L.sla_hip_dec_bits_lanes(64512, 1) == 63 and L.sla_hip_dec_bits_lanes(64513, 1) == 64
    assert L.sla_hip_dec_bits_lanes(10 ** 6, 3) == 21 and L.sla_hip_dec_bits_lanes(10 ** 6, 7) == 9
