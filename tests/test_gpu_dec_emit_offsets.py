"""GPU tests of sla_hip_launch_dec_emit_batch (k_dec_emit_batch; run with -m gpu on an MI355X) called directly, at plane
offsets that are no multiple of 4 samples: a window decode emits every item from the window's first sample inside its
region, so the kernel's guarded 4-byte load path is the common one there.  Every format, every store shape (planar with
vector stores, planar with a channel stride that forbids them, interleaved stereo, mono), mid/side on and off, `done` no
multiple of 4, with and without a zero fill, all entries of a format in one launch, against a numpy model; the
destinations lie in one sentinel-filled tensor with guard bands that must stay as they were."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_decode_batch_device as TD

pytestmark = pytest.mark.gpu

EMIT_DT = np.dtype([("plane_off", "<u8"), ("channel_stride", "<u8"), ("sample_stride", "<u8"), ("dst", "<u8"), ("done", "<u4"),
                    ("fill_end", "<u4"), ("num_channels", "<u4"), ("mid_side", "<u4"), ("shift", "<u4"), ("bits_per_sample", "<u4")])
STRIDE = 8192                    # samples of a plane
GUARD = 8                        # sentinel elements between destinations


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _wrap(a):
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def model(planes, e):
    """left-justified int32 [C][done] of one entry: mid/side undone (two channels), shifted left; 32-bit wrap throughout"""
    src = planes[:e["C"], e["plane_off"]:e["plane_off"] + e["done"]].astype(np.int64)
    if e["ms"] and e["C"] == 2:
        mid = _wrap((src[0] << 1) | (src[1] & 1)).astype(np.int64)
        left = _wrap(mid + src[1]).astype(np.int64) >> 1
        right = _wrap(mid - src[1]).astype(np.int64) >> 1
        src = np.stack([left, right])
    return _wrap(src << e["shift"])


def entries():
    out = []
    k = 0
    for shape in ("planar", "planar_odd_stride", "interleaved", "mono"):
        for off in (0, 1, 2, 3):
            for done, fill in ((1, 0), (2, 7), (3, 0), (5, 5), (1021, 1030), (1027, 0), (2050, 2051), (0, 6)):
                C_ = {"planar": 2 + k % 2, "planar_odd_stride": 2, "interleaved": 2, "mono": 1}[shape]
                bps, lshift = ((16, 0), (24, 0), (16, 2))[k % 3]
                out.append({"shape": shape, "plane_off": 64 * (k % 50) + off, "done": done, "fill_end": fill, "C": C_,
                            "ms": (k // 2) % 2 if C_ == 2 else 0, "bps": bps, "shift": 32 - bps + lshift})
                k += 1
    return out


@pytest.mark.parametrize("fmt", TD.FORMATS, ids=TD.FMT_IDS)
def test_emit_at_plane_offsets_that_are_no_multiple_of_four(hip, fmt):
    import torch
    L = hip.lib()
    rng = np.random.default_rng(77)
    planes = np.stack([rng.integers(-(1 << 23), 1 << 23, STRIDE, dtype=np.int64) for _ in range(3)]).astype(np.int32)
    planes[:, ::3] >>= 8                                          # 16-bit values among the 24-bit ones
    es = entries()
    assert {e["plane_off"] % 4 for e in es} == {0, 1, 2, 3} and any(e["done"] % 4 for e in es)
    # destinations: element (c, i) at base + c * cs + i * ss, regions apart by a guard, the vector shapes 16-byte aligned
    pos = 16
    for e in es:
        lim = max(e["done"], e["fill_end"])
        if e["shape"] == "interleaved":
            e["cs"], e["ss"], span = 1, 2, 2 * lim
        elif e["shape"] == "planar_odd_stride":
            e["cs"], e["ss"] = lim + 1 + (lim % 2) * 2, 1              # never a multiple of 4 when it matters: see below
            while e["cs"] % 4 == 0:
                e["cs"] += 1
            span = e["cs"] * (e["C"] - 1) + lim
        else:
            e["cs"], e["ss"] = (lim + 3) // 4 * 4 + 4, 1
            span = e["cs"] * (e["C"] - 1) + lim
        pos = (pos + 7) // 8 * 8                                     # 16 bytes for int16, 32 for the 4-byte formats
        e["base"], e["span"] = pos, span
        pos += span + GUARD
    dst = TD.alloc((pos + 16,), fmt)
    esize = dst.element_size()
    table = np.zeros(len(es), EMIT_DT)
    for j, e in enumerate(es):
        table[j] = (e["plane_off"], e["cs"], e["ss"], dst.data_ptr() + e["base"] * esize, e["done"], e["fill_end"], e["C"], e["ms"],
                    e["shift"], e["bps"])
    d_planes = torch.from_numpy(planes).cuda()
    d_table = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_dec_emit_batch(C.c_void_p(d_planes.data_ptr()), STRIDE, C.c_void_p(d_table.data_ptr()), len(es),
                                         max(max(e["done"], e["fill_end"]) for e in es), fmt, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = TD.bits_of(dst.cpu().numpy())
    want = np.full(got.shape, TD.sentinel_bits(fmt), got.dtype)
    for e in es:
        vals = TD.bits_of(TD.convert(model(planes, e), fmt, e["bps"]))
        lim = max(e["done"], e["fill_end"])
        for c in range(e["C"]):
            at = e["base"] + c * e["cs"] + np.arange(lim) * e["ss"]
            want[at[:e["done"]]] = vals[c]
            want[at[e["done"]:]] = 0
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (fmt, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(d_planes.cpu().numpy(), planes)           # the planes are only read
