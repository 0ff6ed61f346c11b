"""CPU-only checks of the encoder's verification pass (option "verify", include/sla_hip.h): the header's entry points and
table, the exported symbols, the argument checks that return before any device work, and the host routine that turns the
pack table into the decoder's block table (slai_verify_tables, sla_amd/csrc/sla_verify.c -- pure host arithmetic)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_launch_verify_blocks", "sla_hip_last_verify", "sla_hip_verify_last_image")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def test_header_declares_the_verify_entry_points():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    assert re.search(r"typedef struct sla_hip_verify_expect\b", text)
    assert '"verify"' in text                                  # the option is documented with the others
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "verify" in open(os.path.join(ROOT, doc)).read(), doc


def test_verify_symbols_are_exported(L):
    for name in NAMES:
        assert hasattr(L, name), name
    assert hasattr(sla_amd.Encoder, "last_verify") and hasattr(sla_amd.Encoder, "verify_last_image")


def test_null_arguments_are_refused(L):
    c = (C.c_uint64 * 5)(*([7] * 5))
    # a dangling handle value shows that nothing behind it is read when another argument is NULL
    bogus = C.c_void_p(0x10)
    assert L.sla_hip_last_verify(None, c) == INVALID_ARGUMENT
    assert L.sla_hip_last_verify(bogus, None) == INVALID_ARGUMENT
    assert L.sla_hip_verify_last_image(None, C.c_void_p(0x1000), 16, c) == INVALID_ARGUMENT
    assert L.sla_hip_verify_last_image(bogus, None, 16, c) == INVALID_ARGUMENT
    assert L.sla_hip_verify_last_image(bogus, C.c_void_p(0x1000), 16, None) == INVALID_ARGUMENT
    assert list(c) == [7] * 5


def test_verify_launcher_rejects_bad_arguments(L):
    mem = np.zeros(256, np.uint8)
    rep = np.array([0, 2 ** 64 - 1, 0], np.uint64)
    p, r = mem.ctypes.data, rep.ctypes.data

    def launch(planes=p, source=p, blocks=p, info=p, expect=p, nb=1, nch=2, ms=0, shift=16, report=r):
        return L.sla_hip_launch_verify_blocks(planes, 64, source, 64, blocks, info, expect, None, nb, nch, ms, shift,
                                              None, 0, report, None)

    assert launch(planes=None) == INVALID_ARGUMENT
    assert launch(source=None) == INVALID_ARGUMENT
    assert launch(blocks=None) == INVALID_ARGUMENT
    assert launch(info=None) == INVALID_ARGUMENT
    assert launch(expect=None) == INVALID_ARGUMENT
    assert launch(report=None) == INVALID_ARGUMENT
    assert launch(nch=0) == INVALID_ARGUMENT
    assert launch(nch=9) == INVALID_ARGUMENT
    assert launch(nch=1, ms=1) == INVALID_ARGUMENT
    assert launch(nch=8, ms=1) == INVALID_ARGUMENT
    assert launch(shift=32) == INVALID_ARGUMENT
    # the checks come first: even an empty table with a bad argument is refused, and a good empty table launches nothing
    assert launch(nb=0, shift=32) == INVALID_ARGUMENT
    assert launch(nb=0) == 0
    assert (mem == 0).all() and list(rep) == [0, 2 ** 64 - 1, 0]


# ---- the table-building routine ------------------------------------------------------------------------------------

class PackBlock(C.Structure):                                   # sla_hip_pack_block
    _fields_ = [("blk_off", C.c_uint64), ("out_off", C.c_uint64), ("num_samples", C.c_uint32), ("type", C.c_uint32),
                ("header_off", C.c_uint32), ("header_bytes", C.c_uint32), ("out_bytes", C.c_uint32),
                ("raw_bits", C.c_uint32), ("golomb_m", C.c_uint32 * 8)]


class DecBlock(C.Structure):                                    # sla_hip_dec_block
    _fields_ = [("byte_off", C.c_uint64), ("byte_len", C.c_uint32), ("smp_off", C.c_uint32), ("num_samples", C.c_uint32),
                ("flags", C.c_uint32)]


class Expect(C.Structure):                                      # sla_hip_verify_expect
    _fields_ = [("type", C.c_uint32), ("bytes", C.c_uint32)]


class Seg(C.Structure):                                         # slai_verify_seg
    _fields_ = [("img_off", C.c_uint64), ("img_bytes", C.c_uint64), ("deliver", C.c_int)]


def _tables(L, files, deliver, channels=2, bare=False):
    """files: per file a list of (samples, type, bytes); laid out as pack_device_core does (1024-sample tiles, 43-byte
    headers).  Returns what slai_verify_tables wrote and the layout it was given."""
    pbs, segs, cur, pos = [], [], 0, 0
    for blocks in files:
        start = cur
        cur += 0 if bare else 43
        p = pos
        for n, t, nbytes in blocks:
            pbs.append((p, cur, n, t, nbytes))
            cur += nbytes
            p += n
        pos += -(-(p - pos) // 1024) * 1024
        segs.append((start, cur - start))
    pb = (PackBlock * max(len(pbs), 1))()
    for i, (p, o, n, t, nbytes) in enumerate(pbs):
        pb[i].blk_off, pb[i].out_off, pb[i].num_samples, pb[i].type, pb[i].out_bytes = p, o, n, t, nbytes
    sg = (Seg * max(len(segs), 1))()
    for i, (o, nbytes) in enumerate(segs):
        sg[i].img_off, sg[i].img_bytes, sg[i].deliver = o, nbytes, int(deliver[i])
    nb = len(pbs)
    db, end, ex, so = (DecBlock * (nb + 1))(), (C.c_uint64 * (nb + 1))(), (Expect * (nb + 1))(), (C.c_uint32 * (nb + 1))()
    compared, longest = C.c_uint64(99), C.c_uint32(99)
    L.slai_verify_tables.restype = C.c_uint32
    L.slai_verify_tables.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    got = L.slai_verify_tables(pb, nb, sg, len(segs), channels, db, end, ex, so, C.byref(compared), C.byref(longest))
    return got, db, end, ex, so, compared.value, longest.value, pbs, segs


def test_tables_of_a_batch_with_empty_and_undelivered_files(L):
    files = [[(2048, 0, 900), (17, 2, 80)], [], [(4096, 1, 11)], [(3000, 0, 700), (2500, 0, 600)], []]
    deliver = [1, 1, 1, 0, 1]
    got, db, end, ex, so, compared, longest, pbs, segs = _tables(L, files, deliver)
    want = [(f, b) for f, blocks in enumerate(files) for b in range(len(blocks)) if deliver[f]]
    assert got == len(want) == 3
    flat = [(f, blk) for f, blocks in enumerate(files) for blk in blocks]
    k = 0
    for i, (f, (n, t, nbytes)) in enumerate(flat):
        if not deliver[f]:
            continue
        assert (db[k].byte_off, db[k].byte_len, db[k].smp_off, db[k].num_samples, db[k].flags) == \
            (pbs[i][1], nbytes, pbs[i][0], n, 0)
        assert end[k] == segs[f][0] + segs[f][1]
        assert (ex[k].type, ex[k].bytes) == (t, nbytes)
        assert so[k] == f
        k += 1
    assert compared == 2 * (2048 + 17 + 4096) and longest == 4096


def test_tables_of_one_file_bare_piece_and_nothing(L):
    got, db, end, ex, so, compared, longest, pbs, segs = _tables(L, [[(2048, 0, 500), (2048, 0, 400), (5, 0, 30)]], [1], 1)
    assert got == 3 and [db[i].byte_off for i in range(3)] == [43, 543, 943] and list(end)[:3] == [973] * 3
    assert compared == 4101 and longest == 2048
    got, db, end, ex, so, compared, longest, pbs, segs = _tables(L, [[(2048, 0, 500), (100, 2, 40)]], [1], 8, bare=True)
    assert got == 2 and [db[i].byte_off for i in range(2)] == [0, 500] and list(end)[:2] == [540] * 2
    assert compared == 8 * 2148
    # files without blocks only, an undelivered single file, no file at all
    assert _tables(L, [[], [], []], [1, 1, 1])[0] == 0
    got, *_rest = _tables(L, [[(2048, 0, 500)]], [0])
    assert got == 0 and _rest[4] == 0 and _rest[5] == 0
    c, m = C.c_uint64(5), C.c_uint32(5)
    assert L.slai_verify_tables(None, 0, None, 0, 2, None, None, None, None, C.byref(c), C.byref(m)) == 0
    assert (c.value, m.value) == (0, 0)
