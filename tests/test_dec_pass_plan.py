"""The batch decoder's pass arithmetic (sla_amd/csrc/sla_dec_plan.c: pure host code behind sla_hip_decode_batch and its
device, resident, window and salvage relatives) through ctypes, against the Python model written from the rules
(tests/decplanmodel.py) and against what the inline loops recorded before they became these functions
(tests/golden/dec_pass_plan.json).  The caps are parameters, so tiny ones make every cut happen."""
import ctypes as C
import json
import os

import pytest

import decplanmodel as M
import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 62


class Format(C.Structure):                                      # slai_dec_format
    _fields_ = [(n, C.c_uint32) for n in ("C", "total", "bps", "lshift", "order", "ntaps", "lms", "ms")]


class DecFile(C.Structure):                                     # slai_dec_file
    _fields_ = [("item", C.c_uint32), ("f", Format), ("bytes", C.c_uint32), ("first", C.c_uint32), ("nb", C.c_uint32),
                ("walk_err", C.c_int), ("extent", C.c_uint32), ("alone", C.c_int), ("wide", C.c_int),
                ("img_off", C.c_uint64), ("plane_off", C.c_uint64)]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    lib = sla_amd.lib()
    lib.slai_dec_cut.restype = C.c_uint32
    lib.slai_dec_cut.argtypes = [C.POINTER(DecFile), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    lib.slai_dec_layout.restype = None
    lib.slai_dec_layout.argtypes = [C.POINTER(DecFile), C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.slai_dec_pick_wide.restype = C.c_uint32
    lib.slai_dec_pick_wide.argtypes = [C.POINTER(DecFile), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.slai_dec_wide_capacity.restype = C.c_uint32
    lib.slai_dec_wide_capacity.argtypes = [C.c_uint32, C.c_uint32]
    lib.slai_dec_same_launch.argtypes = [C.POINTER(Format), C.POINTER(Format)]
    return lib


def mk(item=0, extent=1000, nbytes=1000, alone=0, nb=1, **fmt):
    f = dict(C=2, total=50000, bps=16, lshift=0, order=16, ntaps=1, lms=8, ms=1)
    f.update(fmt)
    return M.File(f, item=item, extent=extent, bytes=nbytes, alone=alone, nb=nb)


def table(files):
    """the files at exactly their number (one entry when there is none: ctypes has no empty array to point at)"""
    arr = (DecFile * max(len(files), 1))()
    for a, f in zip(arr, files):
        a.item, a.bytes, a.nb, a.extent, a.alone = f.item, f.bytes, f.nb, f.extent, f.alone
        for n, _ in Format._fields_:
            setattr(a.f, n, f[n])
    return arr


def c_order(L, files):
    """the files as the library's comparison orders them (every pair decided: no two files share an item)"""
    arr = table(files)
    cmp_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
    qsort = C.CDLL(None).qsort
    qsort.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, cmp_t]
    qsort(arr, len(files), C.sizeof(DecFile), cmp_t(lambda a, b: L.slai_dec_file_cmp(C.c_void_p(a), C.c_void_p(b))))
    return [arr[i].item for i in range(len(files))]


def c_passes(L, files, cap_s, cap_b):
    arr, n = table(files), sum(1 for f in files if not f.alone)
    out, p0 = [], 0
    while p0 < n:
        p1 = L.slai_dec_cut(arr, p0, n, cap_s, cap_b)
        assert p0 < p1 <= n
        out.append((p0, p1))
        p0 = p1
    return out


def c_layout(L, files):
    arr = table(files)
    img, span, nb = C.c_uint64(7), C.c_uint64(7), C.c_uint32(7)
    L.slai_dec_layout(arr, len(files), C.byref(img), C.byref(span), C.byref(nb))
    return [(arr[i].img_off, arr[i].plane_off) for i in range(len(files))], img.value, span.value, nb.value


def c_pick(L, files, threshold):
    pick = (C.c_uint32 * M.WIDE_MAX)(*([0xFFFFFFFF] * M.WIDE_MAX))
    n = L.slai_dec_pick_wide(table(files), len(files), threshold, pick)
    assert n <= M.WIDE_MAX and all(v == 0xFFFFFFFF for v in pick[n:])
    return list(pick[:n])


def cost(f):
    return (f.extent + 64) * f.C, f.bytes + 4


# ---- the cut -----------------------------------------------------------------------------------------------------------

def test_a_pass_at_the_cap_is_whole_and_one_above_is_cut(L):
    files = [mk(i, extent=1000 + 7 * i, nbytes=900 + i) for i in range(4)]
    smp, byt = (sum(c) for c in zip(*map(cost, files)))
    assert smp == sum((1000 + 7 * i + 64) * 2 for i in range(4)) and byt == sum(904 + i for i in range(4))   # both overheads counted
    assert c_passes(L, files, smp, byt) == [(0, 4)] == M.passes(files, smp, byt)
    assert c_passes(L, files, smp - 1, BIG) == [(0, 3), (3, 4)] == M.passes(files, smp - 1, BIG)
    assert c_passes(L, files, BIG, byt - 1) == [(0, 3), (3, 4)] == M.passes(files, BIG, byt - 1)
    # without the per-file 64 samples / 4 bytes these caps would hold all four
    assert c_passes(L, files, smp - 64 * 2 * 4, BIG) != [(0, 4)] and c_passes(L, files, BIG, byt - 4 * 4) != [(0, 4)]


def test_either_cap_binds_alone(L):
    files = [mk(i, extent=936, nbytes=96) for i in range(6)]            # 2000 sample-channels, 100 bytes each
    assert c_passes(L, files, 4000, BIG) == [(0, 2), (2, 4), (4, 6)] == M.passes(files, 4000, BIG)
    assert c_passes(L, files, BIG, 300) == [(0, 3), (3, 6)] == M.passes(files, BIG, 300)
    assert c_passes(L, files, 4000, 300) == [(0, 2), (2, 4), (4, 6)]
    assert c_passes(L, files, 8000, 300) == [(0, 3), (3, 6)]


def test_a_file_above_either_cap_is_a_pass_of_its_own(L):
    files = [mk(0, extent=100, nbytes=10), mk(1, extent=90000, nbytes=10), mk(2, extent=100, nbytes=90000), mk(3, extent=100, nbytes=10)]
    assert c_passes(L, files, 1000, 1000) == [(0, 1), (1, 2), (2, 3), (3, 4)] == M.passes(files, 1000, 1000)
    assert c_passes(L, [files[1]], 1, 1) == [(0, 1)]


@pytest.mark.parametrize("field", M.KEY)
def test_a_pass_ends_where_the_launch_key_changes(L, field):
    base = mk()
    other = {field: base[field] + 1}
    files = M.order([mk(0), mk(1), mk(2, **other), mk(3, **other), mk(4)])
    assert [f.item for f in files] == [0, 1, 4, 2, 3] == c_order(L, files[::-1])
    assert c_passes(L, files, BIG, BIG) == [(0, 3), (3, 5)] == M.passes(files, BIG, BIG)
    a, b = table([files[0]]), table([files[3]])
    assert L.slai_dec_same_launch(C.byref(a[0].f), C.byref(a[0].f)) == 1 and L.slai_dec_same_launch(C.byref(a[0].f), C.byref(b[0].f)) == 0


def test_total_is_no_part_of_the_key(L):
    files = [mk(0, total=5), mk(1, total=7)]
    assert c_passes(L, files, BIG, BIG) == [(0, 2)]


def test_alone_files_enter_no_pass(L):
    files = M.order([mk(0, alone=1), mk(1), mk(2, alone=1, C=1), mk(3), mk(4, alone=1)])
    assert [f.item for f in files] == [1, 3, 2, 0, 4] == c_order(L, files[::-1])        # alone last, then key, then item
    assert c_passes(L, files, BIG, BIG) == [(0, 2)] == M.passes(files, BIG, BIG)
    assert c_passes(L, [mk(0, alone=1)], BIG, BIG) == [] == M.passes([mk(0, alone=1)], BIG, BIG)


# ---- the layout --------------------------------------------------------------------------------------------------------

def test_layout_rounding(L):
    sizes, extents = (0, 1, 3, 4, 5), (0, 1, 63, 64, 65)
    files = [mk(i, nbytes=b, extent=e, nb=i % 3) for i, (b, e) in enumerate((b, e) for b in sizes for e in extents)]
    offs, img, span, nb = c_layout(L, files)
    assert (offs, img, span, nb) == M.layout(files)
    assert img == 5 * (0 + 4 + 4 + 4 + 8) and span == 5 * (0 + 64 + 64 + 64 + 128) and nb == sum(f.nb for f in files)
    for k, (io, po) in enumerate(offs):
        assert io % 4 == 0 and po % 64 == 0
        if k > 0:
            assert io >= offs[k - 1][0] + files[k - 1].bytes and po >= offs[k - 1][1] + files[k - 1].extent
    assert c_layout(L, [mk(0, nbytes=0, extent=0, nb=0)]) == ([(0, 0)], 0, 0, 0)       # span 0: the caller takes 1
    assert c_layout(L, []) == ([], 0, 0, 0)
    big = [mk(0, nbytes=0xFFFFFFFF, extent=0xFFFFFFFF), mk(1, nbytes=0xFFFFFFFF, extent=0xFFFFFFFF)]
    assert c_layout(L, big) == M.layout(big) and c_layout(L, big)[1] == 2 << 32          # 64-bit sums


# ---- the wide pick -----------------------------------------------------------------------------------------------------

def test_wide_pick(L):
    files = [mk(i, nbytes=b) for i, b in enumerate((500, 100, 900, 500, 99, 900, 300))]
    assert c_pick(L, files, 0) == [] == M.pick_wide(files, 0)
    assert c_pick(L, files, 100) == [2, 5, 0, 3, 6, 1] == M.pick_wide(files, 100)     # longest first, equal sizes in item order
    assert c_pick(L, files, 901) == []
    rev = files[::-1]                                                               # item order, not table order, breaks ties
    assert [rev[i].item for i in c_pick(L, rev, 100)] == [2, 5, 0, 3, 6, 1]
    for n in (M.WIDE_MAX - 1, M.WIDE_MAX, M.WIDE_MAX + 1, M.WIDE_MAX + 5):
        many = [mk(i, nbytes=1000 + (i * 7) % 5) for i in range(n)] + [mk(n, nbytes=10)]
        got = c_pick(L, many, 1000)
        assert got == M.pick_wide(many, 1000) and len(got) == min(n, M.WIDE_MAX)
        sizes = [many[i].bytes for i in got]
        assert sizes == sorted(sizes, reverse=True)
        assert min(sizes) >= max([f.bytes for i, f in enumerate(many[:n]) if i not in got], default=0)


def test_wide_capacity(L):
    for size in (0, 255, 256, (1 << 24) - 1, 1 << 24, (1 << 24) + 256, 82000000, 0xFFFFFFFF):
        assert L.slai_dec_wide_capacity(0, size) == max(1 << 16, size // 256) == M.wide_capacity(0, size)
        for opt in (1, 77, 0xFFFFFFFF):
            assert L.slai_dec_wide_capacity(opt, size) == opt


# ---- seeded batches: the model and the recording of the former inline loops ---------------------------------------------

def test_seeded_batches_against_the_model_and_the_recording(L):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "dec_pass_plan.json")))["batches"]
    batches = M.batches(200)
    assert len(golden) == len(batches) == 200
    cut_by = {"samples": 0, "bytes": 0, "key": 0}
    for (raw, cap_s, cap_b, thr), rec in zip(batches, golden):
        files = M.order(raw)
        assert c_order(L, raw) == [f.item for f in files]
        cuts = c_passes(L, files, cap_s, cap_b)
        assert cuts == M.passes(files, cap_s, cap_b)
        assert [b for _, b in cuts] == rec["ends"]
        # every file that is not alone in exactly one pass, the alone ones in none
        n = sum(1 for f in files if not f.alone)
        assert [i for a, b in cuts for i in range(a, b)] == list(range(n)) and all(f.alone for f in files[n:])
        for a, b in cuts:
            assert c_layout(L, files[a:b]) == M.layout(files[a:b])
            smp, byt = (sum(c) for c in zip(*map(cost, files[a:b])))
            assert b - a == 1 or (smp <= cap_s and byt <= cap_b)
            if b < n and M.key(files[b]) == M.key(files[a]):
                s1, b1 = cost(files[b])
                assert smp + s1 > cap_s or byt + b1 > cap_b
                cut_by["samples" if smp + s1 > cap_s else "bytes"] += 1
            elif b < n:
                cut_by["key"] += 1
        assert M.layout_sum(files, cuts) == rec["layout"]
        pick = c_pick(L, files, thr)
        assert pick == M.pick_wide(files, thr) and [files[i].item for i in pick] == rec["pick"]
    assert min(cut_by.values()) > 20, cut_by                   # (the batches exercise every reason for a cut)
