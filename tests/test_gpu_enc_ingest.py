"""GPU tests of sla_hip_launch_enc_ingest_batch (k_enc_ingest_batch; run with -m gpu on an MI355X) called directly, at the
shapes sla_hip_encode_batch_device never makes: plane regions that start off a 4-word boundary, plane strides and plane
bases that forbid the 16-byte stores, every bits_per_sample of the F32 quantiser and of the S32 range check, sources that
are misaligned for the vector loads.  One launch per (format, channel count, plane placement) with every load shape crossed
with lengths around the 4-sample run, the wave and the workgroup row; the planes are sentinel-filled and compared whole
against tests/pcmmodel.py -- the converted words, the zero gap [num_samples, fill_end) and every word outside the regions
--, the error words whole, and the source is read back unchanged.  A second group of files holds the refusals."""
import ctypes as C

import numpy as np
import pytest

import pcmmodel as P
from pcmmodel import F32, S16, S32, S32_LEFT
from test_gpu_encode_batch_device import crafted_floats

pytestmark = pytest.mark.gpu

FORMATS = [S32_LEFT, S32, S16, F32]
FMT_IDS = ["s32_left", "s32", "s16", "f32"]
INGEST_DT = np.dtype([("plane_off", "<u8"), ("channel_stride", "<u8"), ("sample_stride", "<u8"), ("src", "<u8"),
                      ("num_samples", "<u4"), ("fill_end", "<u4"), ("bits_per_sample", "<u4"), ("reserved", "<u4")])
assert INGEST_DT.itemsize == 48
SENTINEL = -0x5A5A5A5B                       # bit pattern of every untouched plane word (0xA5A5A5A5)
GAP = 2                                      # sentinel words between plane regions
PRESET = 0x100                               # a bit the kernel never sets: it must survive the OR
LENGTHS = [(0, 0), (0, 6), (1, 0), (2, 7), (3, 3), (4, 4), (5, 9), (63, 64), (64, 64), (65, 0), (1021, 1030), (1023, 1024),
           (1025, 1025), (1027, 0), (2050, 2051), (4099, 4100)]
DEPTHS = (1, 8, 16, 24, 32)
NANS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001)
VARIANTS = ("plane_off", "stride", "base")   # what keeps the plane stores from being 16-byte stores


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def bits_dtype(fmt):
    return np.int16 if fmt == S16 else np.int32


def shapes_of(fmt, nch):
    """(name, source offset in elements) of every load shape a launch of nch channels can hold"""
    per_word = 16 // np.dtype(P.DTYPES[fmt]).itemsize
    out = [("planar_vec", 0)] + [("planar_off", k) for k in (1, 2, 3)]
    if fmt == S16:
        out.append(("planar_vec", 4))                          # 8-byte aligned, in the middle of a 16-byte word
    if nch > 1:
        out += [("planar_cs%d" % k, 0) for k in (1, 2, 3)]
    if nch == 2:
        out += [("stereo", k) for k in range(per_word)]        # offset 0 takes the vector loads, the others the element loads
    if nch in (3, 8):
        out.append(("interleaved", 1))
    out.append(("every_other", 1))
    if nch == 1:
        out.append(("mono3", 2))
    return out


def strides_of(shape, n, nch):
    """(channel_stride, sample_stride, elements spanned) of a file of n samples"""
    pad = (n + 3) // 4 * 4 + 4
    if shape in ("planar_vec", "planar_off"):
        return pad, 1, pad * (nch - 1) + n
    if shape.startswith("planar_cs"):
        cs = pad + int(shape[-1])
        return cs, 1, cs * (nch - 1) + n
    if shape == "stereo":
        return 1, 2, 2 * n
    if shape == "interleaved":
        return 1, nch, n * nch
    if shape == "every_other":
        cs = 2 * n + 3
        return cs, 2, cs * (nch - 1) + 2 * n
    assert shape == "mono3" and nch == 1
    return 0, 3, 3 * n


def depth_of(fmt, k, flagged=False):
    if fmt == S16:
        return 16
    if fmt == S32_LEFT:
        return 24
    return DEPTHS[k % (4 if flagged and fmt == S32 else 5)]          # (nothing is out of range at 32 bits)


def fill_samples(fmt, bps, nch, n, rng):
    """[nch][n] elements: noise over the whole range, the extremes as the first two and the last two samples; floats also
    carry the crafted values and the quantiser's edges from sample 0 on and again up to the last sample"""
    if fmt == F32:
        x = rng.uniform(-1.1, 1.1, (nch, n)).astype(np.float32)
        big = np.finfo(np.float32).max
        special = np.concatenate([crafted_floats(bps), P.quantiser_edges(bps)])
        head = np.concatenate([np.array([-big, big], np.float32), special])
        tail = np.concatenate([special, np.array([big, -big], np.float32)])
        for c in range(nch):
            m = min(n, len(head))
            # (a file shorter than the list holds its start in the even channels and its end in the odd ones)
            if n >= 2 * len(head) or c % 2 == 0:
                x[c, :m] = head[:m]
            if n >= 2 * len(head) or c % 2 == 1:
                x[c, n - m:] = tail[len(tail) - m:]
        return x
    if fmt == S32:
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    else:
        info = np.iinfo(P.DTYPES[fmt])
        lo, hi = int(info.min), int(info.max)
    x = rng.integers(lo, hi + 1, (nch, n), dtype=np.int64)
    for k, v in ((0, lo), (1, hi), (n - 2, hi), (n - 1, lo)):
        if 0 <= k < n:
            x[:, k] = v
    return x.astype(P.DTYPES[fmt])


def offender_of(fmt, bps, k):
    if fmt == S32:
        return np.int32((1 << (bps - 1)) if k % 2 == 0 else -(1 << (bps - 1)) - 1)
    return np.array([NANS[k % 4]], np.uint32).view(np.float32)[0]


def clean_files(fmt, nch):
    out, k = [], 0
    for s, (shape, off) in enumerate(shapes_of(fmt, nch)):
        for n, fill in LENGTHS:
            out.append({"shape": shape, "off": off, "n": n, "fill": fill, "bps": depth_of(fmt, k), "bad": [],
                        "align": (k + s) % 4, "preset": PRESET if k % 5 == 2 else 0})
            k += 1
    return out


def flagged_files(fmt, nch):
    """files of one to four offending elements: at sample 0, at the last sample, inside the last run of fewer than 4, in the
    last channel only, in lane 63 of the first wave, and in the last wave of the second workgroup row"""
    if fmt not in (S32, F32):
        return []
    out, k = [], 0
    shapes = [sh for sh in shapes_of(fmt, nch) if sh in (("planar_vec", 0), ("planar_off", 1), ("planar_cs1", 0), ("stereo", 0),
                                                         ("stereo", 1), ("interleaved", 1), ("every_other", 1), ("mono3", 2))]
    for s, (shape, off) in enumerate(shapes):
        one_per_lane = shape in ("interleaved", "every_other", "mono3")
        # with max_samples 4100 the grid has 5 workgroup rows: row 1 holds samples 1024 .. 2047 where a lane takes four
        # samples (its last wave 1792 ..), and samples 256 .. 511 where a lane takes one (its last wave 448 ..)
        places = [("first", 5, 0, None), ("last", 1027, 1026, None), ("last_run", 1027, 1024, None), ("last_channel", 65, 33, nch - 1),
                  ("lane63", 1025, 4 * 63 + 3, None), ("row1_last_wave", 2050, 480 if one_per_lane else 2000, None)]
        for j, (_, n, at, ch) in enumerate(places):
            count = 1 + (s + j) % 4
            c = (k % nch) if ch is None else ch
            more = [i for i in dict.fromkeys((at + 1, 2, n // 2, at - 1)) if 0 <= i < n and i != at][:count - 1]
            out.append({"shape": shape, "off": off, "n": n, "fill": (0, n + 3)[k % 2], "bps": depth_of(fmt, k, True),
                        "bad": [(c, i) for i in [at] + more], "align": (k + s) % 4, "preset": PRESET if k % 5 == 2 else 0})
            k += 1
    return out


def lay_out(files, fmt, nch, variant, seed):
    """places every file's elements in one source buffer and its region in the planes; returns (src, table, stride): the
    table's src field holds ELEMENT offsets into src"""
    rng = np.random.default_rng(seed)
    per_word = 16 // np.dtype(P.DTYPES[fmt]).itemsize
    chunks, spos, ppos = [], 0, 4
    table = np.zeros(len(files), INGEST_DT)
    for j, f in enumerate(files):
        n, lim = f["n"], max(f["n"], f["fill"])
        cs, ss, span = strides_of(f["shape"], n, nch)
        x = fill_samples(fmt, f["bps"], nch, n, rng)
        for k, (c, i) in enumerate(f["bad"]):
            x[c, i] = offender_of(fmt, f["bps"], j + k)
        spos = (spos + per_word - 1) // per_word * per_word + f["off"]
        region = fill_samples(fmt, f["bps"], 1, span, rng)[0] if span else np.zeros(0, P.DTYPES[fmt])     # what lies between
        at = np.arange(nch)[:, None] * cs + np.arange(n)[None, :] * ss
        region[at] = x
        chunks.append((spos, region))
        ppos = (ppos + 3) // 4 * 4 + (f["align"] if variant == "plane_off" else 0)
        table[j] = (ppos, cs, ss, spos, n, f["fill"], f["bps"], 0)
        f["plane_off"], f["src_off"] = ppos, spos
        spos += span + 1
        ppos += lim + GAP
    src = np.zeros(spos + 2 * per_word, P.DTYPES[fmt])
    for at, region in chunks:
        src[at:at + len(region)] = region
    stride = (ppos + 8 + 3) // 4 * 4 + (1 if variant == "stride" else 0)
    return src, table, stride


def launch(hip, fmt, nch, src, table, stride, variant, presets, max_samples, num_files=None):
    """one launch over sentinel-filled planes; returns (rc, planes, error words, the source read back), the planes as the
    whole tensor (with variant "base" the kernel's planes start one word in)"""
    import torch
    L = hip.lib()
    shift = 1 if variant == "base" else 0
    bits = src.view(bits_dtype(fmt))
    d_src = torch.from_numpy(bits.copy()).cuda()
    if fmt == F32:
        d_src = d_src.view(torch.float32)                          # the same bits: NaN payloads and -0.0 stay as they are
    t = table.copy()
    t["src"] = np.uint64(d_src.data_ptr()) + t["src"] * np.uint64(src.dtype.itemsize)
    d_table = torch.from_numpy(t.view(np.uint8).copy()).cuda()
    d_planes = torch.full((nch * stride + 4 + shift,), SENTINEL, dtype=torch.int32, device="cuda")
    d_err = torch.from_numpy(np.asarray(presets, np.int32).copy()).cuda()
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_enc_ingest_batch(C.c_void_p(d_table.data_ptr()), len(table) if num_files is None else num_files, max_samples,
                                           nch, fmt, C.c_void_p(d_planes[shift:].data_ptr()), stride, C.c_void_p(d_err.data_ptr()), None)
    torch.cuda.synchronize()
    back = d_src.view(torch.int32 if fmt == F32 else d_src.dtype).cpu().numpy()
    return rc, d_planes.cpu().numpy(), d_err.cpu().numpy().view(np.uint32), back


def expectation(files, fmt, nch, src, table, stride, variant, words):
    """(planes, error bits, positions left out of the comparison) the launch should leave"""
    shift = 1 if variant == "base" else 0
    want = np.full(words, SENTINEL, np.int32)
    skip = np.zeros(words, bool)
    errs = np.zeros(len(files), np.uint32)
    for j, f in enumerate(files):
        e = {k: int(table[j][k]) for k in ("channel_stride", "sample_stride", "num_samples", "fill_end", "bits_per_sample")}
        e["src_off"] = f["src_off"]
        conv, err, bad = P.ingest_expect(src, e, fmt, nch)
        assert sorted(bad) == sorted(f["bad"]) and len(bad) <= 4, (j, bad, f["bad"])
        for c in range(nch):
            at = shift + c * stride + f["plane_off"]
            want[at:at + conv.shape[1]] = conv[c]
        for c, i in bad:
            skip[shift + c * stride + f["plane_off"] + i] = True
        errs[j] = err | f["preset"]
    return want, errs, skip


@pytest.mark.parametrize("nch", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_ingest_against_the_model(hip, variant, fmt, nch):
    clean = clean_files(fmt, nch)
    files = clean + flagged_files(fmt, nch)
    assert {f["align"] for f in clean} == {0, 1, 2, 3}
    if fmt in (S32, F32):
        assert {f["bps"] for f in clean} == set(DEPTHS) and len(files) > len(clean)
    src, table, stride = lay_out(files, fmt, nch, variant, 1000 * fmt + 10 * nch + VARIANTS.index(variant))
    if variant == "plane_off":
        assert {int(p) % 4 for p in table["plane_off"]} == {0, 1, 2, 3} and stride % 4 == 0
    else:
        assert not (table["plane_off"] % 4).any() and stride % 4 == (1 if variant == "stride" else 0)
    presets = np.array([f["preset"] for f in files], np.uint32)
    max_samples = max(max(f["n"], f["fill"]) for f in files)
    rc, got, got_err, back = launch(hip, fmt, nch, src, table, stride, variant, presets, max_samples)
    assert rc == 0
    want, want_err, skip = expectation(files, fmt, nch, src, table, stride, variant, len(got))
    assert skip.sum() == sum(len(f["bad"]) for f in files)
    bad = np.nonzero((got != want) & ~skip)[0]
    owner = [j for j, f in enumerate(files) if bad.size and f["plane_off"] <= (bad[0] - (variant == "base")) % stride]
    assert bad.size == 0, (variant, fmt, nch, "entry", owner[-1] if owner else None, files[owner[-1]] if owner else None,
                           bad[:8], got[bad[:8]], want[bad[:8]])
    wrong = np.nonzero(got_err != want_err)[0]
    assert wrong.size == 0, (variant, fmt, nch, "entry", wrong[:8], [files[j] for j in wrong[:2]], got_err[wrong[:8]], want_err[wrong[:8]])
    assert (want_err[:len(clean)] & 3 == 0).all()                   # every clean file proves "the error word stays 0"
    assert np.array_equal(back, src.view(bits_dtype(fmt)))          # the source is only read


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_an_empty_launch_writes_nothing(hip, fmt):
    files = [{"shape": "planar_vec", "off": 0, "n": 100, "fill": 120, "bps": depth_of(fmt, 2), "bad": [], "align": 0, "preset": 0}
             for _ in range(3)]
    src, table, stride = lay_out(files, fmt, 2, "plane_off", 5)
    presets = np.full(3, 0x55, np.uint32)
    for num_files, max_samples in ((0, 120), (3, 0), (0, 0)):
        rc, got, err, back = launch(hip, fmt, 2, src, table, stride, "plane_off", presets, max_samples, num_files=num_files)
        assert rc == 0
        assert (got == SENTINEL).all() and (err == 0x55).all() and np.array_equal(back, src.view(bits_dtype(fmt)))
    rc, got, err, _ = launch(hip, fmt, 2, src, table, stride, "plane_off", presets, 120)       # the same table does write
    assert rc == 0 and (got != SENTINEL).any() and (err == 0x55).all()
