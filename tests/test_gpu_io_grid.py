"""GPU tests of the grid-stride loops of the five sample I/O launchers (run with -m gpu on an MI355X):
sla_hip_launch_enc_ingest_batch, sla_hip_launch_dec_emit_batch, sla_hip_launch_dec_finish_batch,
sla_hip_launch_wav_ingest_batch and sla_hip_launch_wav_emit_batch.  Each caps its grid at 1024 workgroup rows in x and 65535
in y and walks what lies beyond with a stride, so each gets three tests: one workgroup row for long files (max_samples
understated as 1: every lane strides, in every load and store shape), one file that the honest grid cannot cover in one
sweep, and more entries than the grid has rows.  Destinations are sentinel-filled and compared whole.  The models are those
of the kernels' direct tests: `model` of test_gpu_dec_emit_offsets.py and `convert` of test_gpu_decode_batch_device.py,
tests/wavmodel.py and `finish` of test_gpu_wav_kernels.py, tests/pcmmodel.py.  The last test holds the content of
sla_hip_launch_dec_finish_batch against the model, which no other test calls with real arguments."""
import ctypes as C

import numpy as np
import pytest

import pcmmodel as P
import test_gpu_dec_emit_offsets as TO
import test_gpu_decode_batch_device as TD
import test_gpu_enc_ingest as TI
import test_gpu_wav_kernels as TW
import wavmodel as W
from pcmmodel import F32, S16, S32_LEFT

pytestmark = pytest.mark.gpu

LONG = [1, 255, 256, 257, 1023, 1025, 4099, 5000]      # samples of the files that one workgroup row has to walk
SWEEP = 1024 * 1024                                    # samples one sweep of the capped grid covers (4 per lane)
BIG = SWEEP + 1029
ROWS = 65535 + 70                                      # entries: 70 more than blockIdx.y can number
NAN_ENTRIES = (3, 65534, 65535, 65604)
SENTINEL = TD.SENTINEL

FILE_DT = np.dtype([("plane_off", "<u8"), ("out_off", "<u8"), ("num_samples", "<u4"), ("mid_side", "<u4"), ("shift", "<u4"),
                    ("reserved", "<u4")])
WAVIN_DT = np.dtype([("src", "<u8"), ("plane_off", "<u8"), ("num_samples", "<u4"), ("fill_end", "<u4")])
WAVEM_DT = np.dtype([("plane_off", "<u8"), ("dst", "<u8"), ("num_samples", "<u4"), ("mid_side", "<u4"), ("shift", "<u4"),
                     ("header_bytes", "<u4"), ("header", "u1", (48,))])
assert (FILE_DT.itemsize, WAVIN_DT.itemsize, WAVEM_DT.itemsize, TO.EMIT_DT.itemsize) == (32, 24, 80, 56)


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def up(a):
    """a numpy array (a table included) -> device"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).copy() if a.dtype.fields else a).cuda()


def full_range(shape, seed):
    return np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)


def differences(got, want):
    bad = np.nonzero(got != want)[0]
    return bad.size, bad[:8], got[bad[:8]], want[bad[:8]]


def per_entry(values, counts, total):
    """a value per entry -> a value per sample of entries that lie back to back in the planes"""
    out = np.zeros(total, np.int64)
    out[:int(counts.sum())] = np.repeat(values, counts)
    return out


def row_masks(n, lim, width):
    i = np.arange(width)[None, :]
    return i, i < n[:, None], (i >= n[:, None]) & (i < lim[:, None])


# ------------------------------------------------------------------ sla_hip_launch_enc_ingest_batch

@pytest.mark.parametrize("fmt", TI.FORMATS, ids=TI.FMT_IDS)
def test_enc_ingest_one_workgroup_row_walks_long_files(hip, fmt):
    files, k = [], 0
    for s, (shape, off) in enumerate(TI.shapes_of(fmt, 2)):
        for n in LONG:
            files.append({"shape": shape, "off": off, "n": n, "fill": n + k % 3, "bps": TI.depth_of(fmt, k), "bad": [],
                          "align": (k + s) % 4, "preset": 0})
            k += 1
    assert {f["shape"] for f in files} >= {"planar_vec", "planar_off", "planar_cs1", "stereo", "every_other"}
    src, table, stride = TI.lay_out(files, fmt, 2, "plane_off", 40 + fmt)
    rc, got, err, back = TI.launch(hip, fmt, 2, src, table, stride, "plane_off", np.zeros(len(files), np.uint32), 1)
    assert rc == 0
    want, want_err, skip = TI.expectation(files, fmt, 2, src, table, stride, "plane_off", len(got))
    assert not skip.any() and differences(got, want)[0] == 0, (fmt, differences(got, want))
    assert not err.any() and np.array_equal(back, src.view(TI.bits_dtype(fmt)))


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_enc_ingest_a_file_longer_than_one_sweep_of_the_grid(hip, layout):
    cs = (BIG + 3) // 4 * 4 + 4 if layout == "planar" else 1
    src = full_range(2 * cs if layout == "planar" else 2 * BIG, 50)
    table = np.zeros(1, TI.INGEST_DT)
    table[0] = (4, cs, 1 if layout == "planar" else 2, 0, BIG, BIG + 2, 32, 0)
    stride = (BIG + 2 + 4 + 8 + 3) // 4 * 4
    rc, got, err, back = TI.launch(hip, S32_LEFT, 2, src, table, stride, "plane_off", np.zeros(1, np.uint32), BIG + 2)
    assert rc == 0
    want = np.full(len(got), SENTINEL, np.int32)
    for c in range(2):
        want[c * stride + 4:c * stride + 4 + BIG] = src[c * cs:c * cs + BIG] if layout == "planar" else src[c::2]
        want[c * stride + 4 + BIG:c * stride + 4 + BIG + 2] = 0
    assert differences(got, want)[0] == 0, (layout, differences(got, want))
    assert not err.any() and np.array_equal(back, src)


def test_enc_ingest_more_entries_than_grid_rows(hip):
    """F32 mono files of k % 6 samples, a NaN in entries 3, 65534, 65535 and in the last one, 65604 -- which k % 6 would
    leave empty, so that entry alone has one sample; the error words are 2 there and 0 everywhere else"""
    k = np.arange(ROWS)
    n = k % 6
    n[ROWS - 1] = 1
    lim = n + k % 3
    rng = np.random.default_rng(51)
    src = rng.uniform(-1.1, 1.1, 7 * ROWS + 8).astype(np.float32)
    src_off, plane_off = 7 * k, 4 + 9 * k                           # (both at every alignment)
    for e in NAN_ENTRIES:
        assert n[e] > 0
        src[src_off[e] + n[e] - 1] = np.nan
    table = np.zeros(ROWS, TI.INGEST_DT)
    table["plane_off"], table["channel_stride"], table["sample_stride"], table["src"] = plane_off, 0, 1, src_off
    table["num_samples"], table["fill_end"], table["bits_per_sample"] = n, lim, 16
    stride = (4 + 9 * ROWS + 8 + 3) // 4 * 4
    rc, got, err, back = TI.launch(hip, F32, 1, src, table, stride, "plane_off", np.zeros(ROWS, np.uint32), 7)
    assert rc == 0
    conv = P.left(np.where(np.isnan(src), np.float32(0), src), F32, 16)
    i, inside, gap = row_masks(n, lim, 8)
    want = np.full(len(got), SENTINEL, np.int32)
    want[(plane_off[:, None] + i)[inside]] = conv[(src_off[:, None] + i)[inside]]
    want[(plane_off[:, None] + i)[gap]] = 0
    skip = np.zeros(len(got), bool)
    skip[[plane_off[e] + n[e] - 1 for e in NAN_ENTRIES]] = True
    bad = np.nonzero((got != want) & ~skip)[0]
    assert bad.size == 0, ("entry", (bad[:8] - 4) // 9, got[bad[:8]], want[bad[:8]])
    want_err = np.zeros(ROWS, np.uint32)
    want_err[list(NAN_ENTRIES)] = P.ERR_NAN
    assert np.array_equal(err, want_err), np.nonzero(err != want_err)[0][:8]
    assert np.array_equal(back, src.view(np.int32))


# ------------------------------------------------------------------ sla_hip_launch_dec_emit_batch

def dec_emit(hip, fmt, planes, table, dst_len, max_samples):
    """one launch; the table's dst field holds ELEMENT offsets into a sentinel-filled destination, returned as bits"""
    import torch
    dst = TD.alloc((dst_len,), fmt)
    t = table.copy()
    t["dst"] = np.uint64(dst.data_ptr()) + t["dst"] * np.uint64(dst.element_size())
    d_planes, d_table = up(planes), up(t)
    torch.cuda.synchronize()
    rc = hip.lib().sla_hip_launch_dec_emit_batch(C.c_void_p(d_planes.data_ptr()), planes.shape[1], C.c_void_p(d_table.data_ptr()),
                                                 len(table), max_samples, fmt, None)
    torch.cuda.synchronize()
    assert np.array_equal(d_planes.cpu().numpy(), planes)           # the planes are only read
    return rc, TD.bits_of(dst.cpu().numpy())


@pytest.mark.parametrize("fmt", TD.FORMATS, ids=TD.FMT_IDS)
def test_dec_emit_one_workgroup_row_walks_long_files(hip, fmt):
    planes = full_range((3, 8192), 60) >> 8
    planes[:, ::3] >>= 8
    es, k, pos = [], 0, 16
    for shape in ("planar", "planar_odd_stride", "interleaved", "mono"):
        for done in LONG:
            nch = {"planar": 2 + k % 2, "planar_odd_stride": 2, "interleaved": 2, "mono": 1}[shape]
            bps, lshift = ((16, 0), (24, 0), (16, 2))[k % 3]
            e = {"plane_off": 16 * (k % 50) + k % 4, "done": done, "fill_end": done + k % 3, "C": nch, "bps": bps,
                 "ms": (k // 2) % 2 if nch == 2 else 0, "shift": 32 - bps + lshift}
            lim = e["fill_end"]
            if shape == "interleaved":
                e["cs"], e["ss"], span = 1, 2, 2 * lim
            else:
                e["cs"], e["ss"] = (lim + 3) // 4 * 4 + 4 + (1 if shape == "planar_odd_stride" else 0), 1
                span = e["cs"] * (nch - 1) + lim
            pos = (pos + 7) // 8 * 8
            e["base"] = pos
            pos += span + TO.GUARD
            es.append(e)
            k += 1
    table = np.zeros(len(es), TO.EMIT_DT)
    for j, e in enumerate(es):
        table[j] = (e["plane_off"], e["cs"], e["ss"], e["base"], e["done"], e["fill_end"], e["C"], e["ms"], e["shift"], e["bps"])
    rc, got = dec_emit(hip, fmt, planes, table, pos + 16, 1)
    assert rc == 0
    want = np.full(got.shape, TD.sentinel_bits(fmt), got.dtype)
    for e in es:
        vals = TD.bits_of(TD.convert(TO.model(planes, e), fmt, e["bps"]))
        for c in range(e["C"]):
            at = e["base"] + c * e["cs"] + np.arange(e["fill_end"]) * e["ss"]
            want[at[:e["done"]]] = vals[c]
            want[at[e["done"]:]] = 0
    assert differences(got, want)[0] == 0, (fmt, differences(got, want))


@pytest.mark.parametrize("fmt", [S32_LEFT, S16], ids=["s32_left", "s16"])
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_dec_emit_a_file_longer_than_one_sweep_of_the_grid(hip, layout, fmt):
    planes = full_range((2, (BIG + 8 + 3) // 4 * 4), 61)                # (a stride that allows the 16-byte plane loads)
    cs, ss = ((BIG + 2 + 3) // 4 * 4 + 4, 1) if layout == "planar" else (1, 2)
    table = np.zeros(1, TO.EMIT_DT)
    table[0] = (4, cs, ss, 16, BIG, BIG + 2, 2, 1, 0, 16)
    rc, got = dec_emit(hip, fmt, planes, table, 16 + 2 * max(cs, BIG + 2) + 16, BIG + 2)
    assert rc == 0
    vals = TD.bits_of(TD.convert(TW.finish(planes[:, 4:4 + BIG], 1, 0), fmt, 16))
    want = np.full(got.shape, TD.sentinel_bits(fmt), got.dtype)
    for c in range(2):
        at = slice(16 + c * cs, 16 + c * cs + (BIG + 2) * ss, ss)
        want[at][:BIG] = vals[c]
        want[at][BIG:] = 0
    assert differences(got, want)[0] == 0, (layout, fmt, differences(got, want))


def test_dec_emit_more_entries_than_grid_rows(hip):
    k = np.arange(ROWS)
    n, ms, shift = k % 6, k % 2, 8 * (k % 3)
    lim = n + k % 3
    plane_off, base = 6 * k, 16 + 18 * k                            # (destinations 16-byte aligned and not)
    planes = full_range((2, 6 * ROWS + 8), 62)
    table = np.zeros(ROWS, TO.EMIT_DT)
    table["plane_off"], table["channel_stride"], table["sample_stride"], table["dst"] = plane_off, 8, 1, base
    table["done"], table["fill_end"], table["num_channels"], table["mid_side"], table["shift"], table["bits_per_sample"] = n, lim, 2, ms, shift, 16
    rc, got = dec_emit(hip, S32_LEFT, planes, table, 16 + 18 * ROWS + 16, 7)
    assert rc == 0
    six = np.full(ROWS, 6)
    sh, on = per_entry(shift, six, planes.shape[1]), per_entry(ms, six, planes.shape[1])
    fin = np.where(on != 0, TW.finish(planes, 1, sh), TW.finish(planes, 0, sh))
    for e in (0, 1, 2, 3, 4, 5, ROWS - 2, ROWS - 1):                  # the vectorised form against the entry model
        one = {"C": 2, "plane_off": int(plane_off[e]), "done": int(n[e]), "ms": int(ms[e]), "shift": int(shift[e])}
        assert np.array_equal(TO.model(planes, one), fin[:, plane_off[e]:plane_off[e] + n[e]]), e
    i, inside, gap = row_masks(n, lim, 8)
    want = np.full(got.shape, SENTINEL, np.int32)
    for c in range(2):
        want[(base[:, None] + 8 * c + i)[inside]] = fin[c][(plane_off[:, None] + i)[inside]]
        want[(base[:, None] + 8 * c + i)[gap]] = 0
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("entry", (bad[:8] - 16) // 18, got[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------ sla_hip_launch_dec_finish_batch

def dec_finish(hip, planes, nch, table, out_len, max_samples):
    import torch
    d_planes, d_table = up(planes), up(table)
    d_out = torch.full((out_len,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = hip.lib().sla_hip_launch_dec_finish_batch(C.c_void_p(d_planes.data_ptr()), planes.shape[1], nch, C.c_void_p(d_table.data_ptr()),
                                                   len(table), max_samples, C.c_void_p(d_out.data_ptr()), None)
    torch.cuda.synchronize()
    assert np.array_equal(d_planes.cpu().numpy(), planes)
    return rc, d_out.cpu().numpy()


def finish_entries(planes, nch, entries):
    """(table, expected output, its length) of entries (plane_off, n, mid_side, shift): packed [file][ch][n], three sentinel
    words between the files"""
    table = np.zeros(len(entries), FILE_DT)
    pos, parts = 3, []
    for j, (po, n, ms, shift) in enumerate(entries):
        table[j] = (po, pos, n, ms, shift, 0)
        parts.append((pos, TO.model(planes, {"C": nch, "plane_off": po, "done": n, "ms": ms, "shift": shift}).reshape(-1)))
        pos += nch * n + 3
    want = np.full(pos + 8, SENTINEL, np.int32)
    for at, vals in parts:
        want[at:at + len(vals)] = vals
    return table, want


MID_SIDE_OPERANDS = [(m, s) for m in (-2 ** 31, 2 ** 31 - 1, -1, 0, 1) for s in (1, 2, -1, -2, 2 ** 31 - 1, -2 ** 31, 0, 3)]


@pytest.mark.parametrize("nch", [1, 2, 3, 8])
def test_dec_finish_batch_against_the_model(hip, nch):
    """mid/side (two channels only: with three the flag is ignored), every shift, plane regions at every word alignment;
    mid words at the ends of int32 against odd and even side words: the 33-bit sum wraps as the reference's C does"""
    entries, pos, k = [], 0, 0
    planes = full_range((nch, 16384), 70 + nch)
    for n in (0, 1, 255, 256, 257, 1000):
        for shift in (0, 8, 16, 31):
            for ms in ((0, 1) if nch in (2, 3) else (0,)):
                po = (pos + 3) // 4 * 4 + k % 4
                m = min(n, len(MID_SIDE_OPERANDS))
                rot = MID_SIDE_OPERANDS[k % 40:] + MID_SIDE_OPERANDS[:k % 40]       # (a file of one sample sees another pair each)
                planes[0, po:po + m] = [a for a, _ in rot[:m]]
                if nch > 1:
                    planes[1, po:po + m] = [b for _, b in rot[:m]]
                entries.append((po, n, ms, shift))
                pos = po + n + 3
                k += 1
    assert pos <= planes.shape[1] and {e[0] % 4 for e in entries} == {0, 1, 2, 3}
    table, want = finish_entries(planes, nch, entries)
    rc, got = dec_finish(hip, planes, nch, table, len(want), 1000)
    assert rc == 0 and differences(got, want)[0] == 0, (nch, differences(got, want))
    if nch == 3:                                                      # ignored: the same words as without the flag
        off = [(po, n, 0, shift) for po, n, _, shift in entries]
        assert np.array_equal(finish_entries(planes, nch, off)[1], want)


@pytest.mark.parametrize("nch", [1, 2, 3])
def test_dec_finish_batch_one_workgroup_row_walks_long_files(hip, nch):
    planes = full_range((nch, 16384), 73 + nch)
    entries, pos = [], 0
    for k, n in enumerate(LONG):
        entries.append((pos + k % 4, n, k % 2, (0, 8, 16)[k % 3]))
        pos += n + 5
    table, want = finish_entries(planes, nch, entries)
    rc, got = dec_finish(hip, planes, nch, table, len(want), 1)
    assert rc == 0 and differences(got, want)[0] == 0, (nch, differences(got, want))


def test_dec_finish_batch_a_file_longer_than_one_sweep_of_the_grid(hip):
    n = 1024 * 256 + 77                                               # (a lane takes one sample: a sweep is 1024 x 256)
    planes = full_range((2, n + 8), 76)
    table = np.zeros(1, FILE_DT)
    table[0] = (3, 5, n, 1, 8, 0)
    rc, got = dec_finish(hip, planes, 2, table, 5 + 2 * n + 8, n)
    want = np.full(len(got), SENTINEL, np.int32)
    want[5:5 + 2 * n] = TW.finish(planes[:, 3:3 + n], 1, 8).reshape(-1)
    assert rc == 0 and differences(got, want)[0] == 0, differences(got, want)


def test_dec_finish_batch_more_entries_than_grid_rows(hip):
    k = np.arange(ROWS)
    n, ms, shift = k % 6, k % 2, 8 * (k % 3)
    plane_off, out_off = 6 * k, 3 + 13 * k
    planes = full_range((2, 6 * ROWS + 8), 77)
    table = np.zeros(ROWS, FILE_DT)
    table["plane_off"], table["out_off"], table["num_samples"], table["mid_side"], table["shift"] = plane_off, out_off, n, ms, shift
    rc, got = dec_finish(hip, planes, 2, table, 3 + 13 * ROWS + 8, 5)
    assert rc == 0
    six = np.full(ROWS, 6)
    sh, on = per_entry(shift, six, planes.shape[1]), per_entry(ms, six, planes.shape[1])
    fin = np.where(on != 0, TW.finish(planes, 1, sh), TW.finish(planes, 0, sh))
    for e in (0, 1, 2, 3, 4, 5, ROWS - 2, ROWS - 1):
        one = {"C": 2, "plane_off": int(plane_off[e]), "done": int(n[e]), "ms": int(ms[e]), "shift": int(shift[e])}
        assert np.array_equal(TO.model(planes, one), fin[:, plane_off[e]:plane_off[e] + n[e]]), e
    i, inside, _ = row_masks(n, n, 6)
    want = np.full(len(got), SENTINEL, np.int32)
    for c in range(2):
        want[(out_off[:, None] + c * n[:, None] + i)[inside]] = fin[c][(plane_off[:, None] + i)[inside]]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("entry", (bad[:8] - 3) // 13, got[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------ sla_hip_launch_wav_ingest_batch

def wav_ingest(hip, nch, B, src, table, stride, max_samples):
    """one launch; the table's src field holds BYTE offsets into src; returns (rc, the sentinel-filled planes)"""
    import torch
    d_src = up(src)
    t = table.copy()
    t["src"] = t["src"] + np.uint64(d_src.data_ptr())
    d_table = up(t)
    d_planes = torch.full((nch * stride + 4,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = hip.lib().sla_hip_launch_wav_ingest_batch(d_table.data_ptr(), len(table), max_samples, nch, B, d_planes.data_ptr(), stride, None)
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), src)
    return rc, d_planes.cpu().numpy()


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_wav_ingest_one_workgroup_row_walks_long_files(hip, B, nch):
    table = np.zeros(len(LONG), WAVIN_DT)
    chunks, pos, ppos = [], 0, 4
    for k, n in enumerate(LONG):
        raw = np.frombuffer(TW.frames_of(n, nch, B, 80 + 10 * B + nch + k), np.uint8)
        pos = (pos + 15) // 16 * 16 + (5 * k + B) % 16
        ppos = (ppos + 3) // 4 * 4 + (0, 0, 1, 3)[k % 4]              # (16-byte plane stores and guarded ones)
        table[k] = (pos, ppos, n, n + k % 3)
        chunks.append((pos, ppos, n, n + k % 3, raw))
        pos += len(raw)
        ppos += n + k % 3 + 2
    src = np.full(pos, TW.BYTE_SENTINEL, np.uint8)
    for at, _, _, _, raw in chunks:
        src[at:at + len(raw)] = raw
    stride = (ppos + 8 + 3) // 4 * 4
    rc, got = wav_ingest(hip, nch, B, src, table, stride, 1)
    assert rc == 0
    want = np.full(len(got), SENTINEL, np.int32)
    for _, po, n, lim, raw in chunks:
        conv = W.planes_from_frames(raw.tobytes(), nch, 8 * B)
        for c in range(nch):
            want[c * stride + po:c * stride + po + n] = conv[c]
            want[c * stride + po + n:c * stride + po + lim] = 0
    assert differences(got, want)[0] == 0, (B, nch, differences(got, want))


def test_wav_ingest_a_file_longer_than_one_sweep_of_the_grid(hip):
    nch, B = 2, 2
    src = np.random.default_rng(85).integers(0, 256, 6 + BIG * nch * B, dtype=np.int64).astype(np.uint8)
    table = np.zeros(1, WAVIN_DT)
    table[0] = (6, 4, BIG, BIG + 2)                                   # (the source 6 bytes into a 16-byte word)
    stride = (BIG + 2 + 4 + 8 + 3) // 4 * 4
    rc, got = wav_ingest(hip, nch, B, src, table, stride, BIG + 2)
    assert rc == 0
    conv = W.planes_from_frames(src[6:].tobytes(), nch, 8 * B)
    want = np.full(len(got), SENTINEL, np.int32)
    for c in range(nch):
        want[c * stride + 4:c * stride + 4 + BIG] = conv[c]
        want[c * stride + 4 + BIG:c * stride + 4 + BIG + 2] = 0
    assert differences(got, want)[0] == 0, differences(got, want)


def test_wav_ingest_more_entries_than_grid_rows(hip):
    nch, B = 2, 3
    k = np.arange(ROWS)
    n = k % 6
    lim = n + k % 3
    first = np.concatenate([[0], np.cumsum(n)[:-1]])                  # the files lie back to back: a frame index each
    src = np.random.default_rng(86).integers(0, 256, int(n.sum()) * nch * B, dtype=np.int64).astype(np.uint8)
    plane_off = 4 + 9 * k
    table = np.zeros(ROWS, WAVIN_DT)
    table["src"], table["plane_off"], table["num_samples"], table["fill_end"] = first * nch * B, plane_off, n, lim
    stride = (4 + 9 * ROWS + 8 + 3) // 4 * 4
    rc, got = wav_ingest(hip, nch, B, src, table, stride, 7)
    assert rc == 0
    conv = W.planes_from_frames(src.tobytes(), nch, 8 * B)          # frame after frame, whatever file it belongs to
    i, inside, gap = row_masks(n, lim, 8)
    want = np.full(len(got), SENTINEL, np.int32)
    for c in range(nch):
        want[c * stride + (plane_off[:, None] + i)[inside]] = conv[c][(first[:, None] + i)[inside]]
        want[c * stride + (plane_off[:, None] + i)[gap]] = 0
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("entry", (bad[:8] % stride - 4) // 9, got[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------ sla_hip_launch_wav_emit_batch

def wav_emit(hip, planes, table, dst_len, max_samples, nch, B, ms):
    """one launch; the table's dst field holds BYTE offsets into a sentinel-filled destination, which is returned"""
    import torch
    d_dst = torch.full((dst_len,), TW.BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
    t = table.copy()
    t["dst"] = t["dst"] + np.uint64(d_dst.data_ptr())
    d_planes, d_table = up(planes), up(t)
    torch.cuda.synchronize()
    rc = hip.lib().sla_hip_launch_wav_emit_batch(d_planes.data_ptr(), planes.shape[1], d_table.data_ptr(), len(table), max_samples, nch, B,
                                                 ms, None)
    torch.cuda.synchronize()
    assert np.array_equal(d_planes.cpu().numpy(), planes)
    return rc, d_dst.cpu().numpy()


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_wav_emit_one_workgroup_row_walks_long_files(hip, B, nch):
    for ms in ((0, 1) if nch == 2 else (0,)):
        planes = full_range((nch, sum(LONG) + 4 * len(LONG) + 8), 90 + 10 * B + nch)
        table = np.zeros(len(LONG), WAVEM_DT)
        pos, ppos, files = (3 * B + nch + 7 * ms) % 16, 0, []
        for k, n in enumerate(LONG):
            hb, shift = (0, 44)[k % 2], (0, 8, 16)[k % 3]
            header = W.header44(W.Info(nch, 8 * B, 44100 + k, n, 44, n * nch * B))
            ppos += (0, 1, 3, 2)[k % 4]
            table[k] = (ppos, pos, n, ms, shift, hb, np.frombuffer(header + bytes(4), np.uint8))
            body = W.frames_from_planes(TW.finish(planes[:, ppos:ppos + n], ms, shift), 8 * B)
            files.append((pos, (header if hb else b"") + body))
            pos += len(files[-1][1])                                  # back to back, no padding
            ppos += n
        rc, got = wav_emit(hip, planes, table, pos + 64, 1, nch, B, ms)
        assert rc == 0
        want = np.full(len(got), TW.BYTE_SENTINEL, np.uint8)
        for at, data in files:
            want[at:at + len(data)] = np.frombuffer(data, np.uint8)
        assert differences(got, want)[0] == 0, (B, nch, ms, differences(got, want))


def test_wav_emit_a_file_longer_than_one_sweep_of_the_grid(hip):
    """the grid is capped at 1024 x 256 lanes of 16 bytes: a destination of more than 4 MiB takes the grid-stride loop"""
    planes = full_range((1, BIG + 8), 95)
    header = W.header44(W.Info(1, 32, 48000, BIG, 44, 4 * BIG))
    table = np.zeros(1, WAVEM_DT)
    table[0] = (3, 5, BIG, 0, 0, 44, np.frombuffer(header + bytes(4), np.uint8))
    assert 44 + 4 * BIG > 4 << 20
    rc, got = wav_emit(hip, planes, table, 5 + 44 + 4 * BIG + 64, BIG, 1, 4, 0)
    assert rc == 0
    want = np.full(len(got), TW.BYTE_SENTINEL, np.uint8)
    want[5:49] = np.frombuffer(header, np.uint8)
    want[49:49 + 4 * BIG] = planes[0, 3:3 + BIG].astype("<i4").view(np.uint8)
    assert differences(got, want)[0] == 0, differences(got, want)


def test_wav_emit_more_entries_than_grid_rows(hip):
    nch, B = 2, 2
    k = np.arange(ROWS)
    n, ms, shift = k % 6, k % 2, 8 * (k % 3)
    first = np.concatenate([[0], np.cumsum(n)[:-1]])
    plane_off = 6 * k
    planes = full_range((2, 6 * ROWS + 8), 96)
    table = np.zeros(ROWS, WAVEM_DT)
    table["plane_off"], table["dst"], table["num_samples"] = plane_off, 9 + first * nch * B, n      # back to back, no headers
    table["mid_side"], table["shift"] = ms, shift
    total = int(n.sum()) * nch * B
    rc, got = wav_emit(hip, planes, table, 9 + total + 64, 5, nch, B, 1)
    assert rc == 0
    six = np.full(ROWS, 6)
    sh, on = per_entry(shift, six, planes.shape[1]), per_entry(ms, six, planes.shape[1])
    fin = np.where(on != 0, TW.finish(planes, 1, sh), TW.finish(planes, 0, sh))
    for e in (0, 1, 2, 3, 4, 5, ROWS - 2, ROWS - 1):
        assert np.array_equal(TW.finish(planes[:, plane_off[e]:plane_off[e] + n[e]], int(ms[e]), int(shift[e])),
                              fin[:, plane_off[e]:plane_off[e] + n[e]]), e
    i, inside, _ = row_masks(n, n, 6)
    kept = fin[:, (plane_off[:, None] + i)[inside]]                   # the samples of all files, in file order
    want = np.full(len(got), TW.BYTE_SENTINEL, np.uint8)
    want[9:9 + total] = np.frombuffer(W.frames_from_planes(kept, 8 * B), np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("entry", np.searchsorted(first * nch * B, bad[:8] - 9, side="right") - 1, got[bad[:8]], want[bad[:8]])
