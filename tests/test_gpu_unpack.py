"""GPU tests of sla_hip_launch_unpack16 and sla_hip_launch_unpack24 (k_unpack16, k_unpack24 of kernels/pack.inc; run with
-m gpu on an MI355X) called directly: counts around the 4-sample group a lane takes and around the 1024-sample workgroup,
the extremes of the input among the operands, the output sentinel-filled with guard words behind `count` and compared
whole."""
import ctypes as C

import numpy as np
import pytest

import pcmmodel as P

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 2
COUNTS = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4099, 3 * 1024 + 1]
GUARD = 8
SENTINEL = -0x5A5A5A5B


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def call(hip, name, d_in, d_out, count):
    """(the launchers have no argtypes: pointers and the 64-bit count are wrapped here)"""
    import torch
    rc = getattr(hip.lib(), name)(C.c_void_p(d_in), C.c_void_p(d_out), C.c_uint64(count), C.c_void_p(None))
    torch.cuda.synchronize()
    return rc


def samples16(count):
    rng = np.random.default_rng(16 + count)
    x = rng.integers(-32768, 32768, count, dtype=np.int64).astype(np.int16)
    edge = np.array([-32768, 32767, -1, 0, 1], np.int16)
    m = min(count, len(edge))
    x[:m] = edge[:m]
    x[count - m:] = edge[::-1][len(edge) - m:]                    # (the extremes again in the last group, whatever its size)
    return x


def bytes24(count):
    rng = np.random.default_rng(24 + count)
    raw = rng.integers(0, 256, 3 * count, dtype=np.int64).astype(np.uint8)
    top = np.array([0x00, 0x7F, 0x80, 0xFF], np.uint8)
    raw[2::3] = top[np.arange(count) % 4]                         # every third byte: the sample's sign byte
    if count > 5:
        raw[2::3][-5:] = top[[3, 2, 1, 0, 3]]                     # another phase against the group of four at the end
    return raw


@pytest.mark.parametrize("count", COUNTS)
def test_unpack16(hip, count):
    import torch
    x = samples16(count)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.full((count + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert d_in.data_ptr() % 8 == 0
    assert call(hip, "sla_hip_launch_unpack16", d_in.data_ptr(), d_out.data_ptr(), count) == 0
    want = np.full(count + GUARD, SENTINEL, np.int32)
    want[:count] = x.astype(np.int32) << 16
    got = d_out.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (count, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(d_in.cpu().numpy(), x)


@pytest.mark.parametrize("count", COUNTS)
def test_unpack24(hip, count):
    import torch
    raw = bytes24(count)
    d_in = torch.from_numpy(raw).cuda()
    d_out = torch.full((count + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert d_in.data_ptr() % 8 == 0
    assert call(hip, "sla_hip_launch_unpack24", d_in.data_ptr(), d_out.data_ptr(), count) == 0
    want = np.full(count + GUARD, SENTINEL, np.int32)
    want[:count] = P.unpack24_expect(raw, count)
    got = d_out.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (count, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(d_in.cpu().numpy(), raw)


@pytest.mark.parametrize("name", ["sla_hip_launch_unpack16", "sla_hip_launch_unpack24"])
def test_nothing_to_do_and_null_pointers(hip, name):
    import torch
    d_in = torch.full((64,), 0x11, dtype=torch.uint8, device="cuda")
    d_out = torch.full((16 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert call(hip, name, d_in.data_ptr(), d_out.data_ptr(), 0) == 0
    assert call(hip, name, None, d_out.data_ptr(), 16) == INVALID_ARGUMENT
    assert call(hip, name, d_in.data_ptr(), None, 16) == INVALID_ARGUMENT
    assert call(hip, name, None, None, 0) == INVALID_ARGUMENT
    assert (d_out.cpu().numpy() == SENTINEL).all() and (d_in.cpu().numpy() == 0x11).all()
    assert call(hip, name, d_in.data_ptr(), d_out.data_ptr(), 16) == 0              # the same buffers do get written
    assert (d_out.cpu().numpy()[:16] != SENTINEL).all() and (d_out.cpu().numpy()[16:] == SENTINEL).all()
