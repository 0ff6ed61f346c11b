"""CPU-only checks of the four launchers behind tests/test_gpu_dec_synth.py (sla_hip_launch_dec_lms, _dec_lattice,
_dec_deemphasis, _dec_finish; include/sla_hip.h): the argument checks that return before any device work, and the
empty launches that return 0 without one.  Every rejected call carries zero blocks or samples beside its one bad
argument, so that nothing could be launched even by a launcher that let it through; `stride < n` cannot be put that
way and is the one call with a sample count.  The pointers are host arrays: nothing reads them."""
import ctypes as C
import os

import numpy as np
import pytest

import sla_amd

INVALID_ARGUMENT = 2
u32, u64, i32, vp = C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


@pytest.fixture(scope="module")
def mem():
    """dummy planes / blocks / info / kint"""
    arrays = [np.zeros(64, np.int32) for _ in range(4)]
    return arrays, [vp(a.ctypes.data) for a in arrays]


def test_symbols_are_exported(L):
    for name in ("sla_hip_launch_dec_lms", "sla_hip_launch_dec_lattice", "sla_hip_launch_dec_deemphasis", "sla_hip_launch_dec_finish"):
        assert name in sla_amd.EXPORTED_SYMBOLS and hasattr(L, name), name


def test_lms_launcher_arguments(L, mem):
    planes, blocks, info, _ = mem[1]
    lms = lambda p, b, i, nb, nch, order: L.sla_hip_launch_dec_lms(p, u64(64), b, i, u32(nb), u32(nch), u32(order), None)
    assert lms(None, blocks, info, 0, 1, 4) == INVALID_ARGUMENT
    assert lms(planes, None, info, 0, 1, 4) == INVALID_ARGUMENT
    assert lms(planes, blocks, None, 0, 1, 4) == INVALID_ARGUMENT
    for nch in (0, 9):
        assert lms(planes, blocks, info, 0, nch, 4) == INVALID_ARGUMENT, nch
    for order in (0, 5, 64, 2, 12, 33):
        assert lms(planes, blocks, info, 0, 1, order) == INVALID_ARGUMENT, order
    for order in (4, 8, 16, 32):
        for nch in (1, 3, 8):
            assert lms(planes, blocks, info, 0, nch, order) == 0, (order, nch)


def test_lattice_launcher_arguments(L, mem):
    planes, blocks, info, kint = mem[1]
    lat = lambda p, b, i, k, nb, nch, order, de=1: L.sla_hip_launch_dec_lattice(p, u64(64), b, i, u32(nb), u32(nch), k, u32(order), u32(de), None)
    assert lat(None, blocks, info, kint, 0, 1, 16) == INVALID_ARGUMENT
    assert lat(planes, None, info, kint, 0, 1, 16) == INVALID_ARGUMENT
    assert lat(planes, blocks, None, kint, 0, 1, 16) == INVALID_ARGUMENT
    assert lat(planes, blocks, info, None, 0, 1, 16) == INVALID_ARGUMENT
    for nch in (0, 9):
        assert lat(planes, blocks, info, kint, 0, nch, 16) == INVALID_ARGUMENT, nch
    for order in (256, 257, 2 ** 31):
        assert lat(planes, blocks, info, kint, 0, 1, order) == INVALID_ARGUMENT, order
    for order in (0, 1, 16, 17, 64, 65, 129, 255):
        for de in (0, 1):
            assert lat(planes, blocks, info, kint, 0, 8, order, de) == 0, (order, de)


def test_deemphasis_launcher_arguments(L, mem):
    data = mem[1][0]
    de = lambda p, n, prev, shift: L.sla_hip_launch_dec_deemphasis(p, u32(n), i32(prev), u32(shift), None)
    assert de(None, 0, 0, 5) == INVALID_ARGUMENT
    for shift in (0, 31, 32, 2 ** 31):
        assert de(data, 0, 0, shift) == INVALID_ARGUMENT, shift
    for shift in (1, 5, 30):
        assert de(data, 0, -2 ** 31, shift) == 0, shift


def test_finish_launcher_arguments(L, mem):
    planes = mem[1][0]
    fin = lambda p, stride, nch, n, ms, shift: L.sla_hip_launch_dec_finish(p, u64(stride), u32(nch), u32(n), u32(ms), u32(shift), None)
    assert fin(None, 64, 1, 0, 0, 0) == INVALID_ARGUMENT
    for nch in (0, 9):
        assert fin(planes, 64, nch, 0, 0, 0) == INVALID_ARGUMENT, nch
    assert fin(planes, 64, 2, 0, 0, 32) == INVALID_ARGUMENT
    for nch in (1, 3, 8):
        assert fin(planes, 64, nch, 0, 1, 16) == INVALID_ARGUMENT, nch          # mid/side is for two channels
    assert fin(planes, 4, 1, 5, 0, 0) == INVALID_ARGUMENT                       # stride < n
    for nch, ms, shift in ((1, 0, 0), (2, 1, 31), (2, 0, 8), (8, 0, 16)):
        assert fin(planes, 64, nch, 0, ms, shift) == 0, (nch, ms, shift)
        assert fin(planes, 0, nch, 0, ms, shift) == 0                           # stride == n == 0
    assert (np.concatenate(mem[0]) == 0).all()                                  # and nothing wrote to the dummies
