"""CPU-only checks of the salvage ABI (sla_hip_salvage_resident, sla_hip_launch_dec_salvage_scan,
sla_hip_dec_salvage_scratch_bytes, sla_hip_launch_salvage_crc, sla_hip_launch_dec_conceal): the symbols, the struct
layouts against the header's text, the Python face, the scratch macro against the function, the length cap against the
model, and every refusal that returns before any device work."""
import ctypes as C
import os
import re

import pytest

import salvagemodel as SM
import sla_amd
import widewalkmodel as WW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_salvage_resident", "sla_hip_launch_dec_salvage_scan", "sla_hip_dec_salvage_scratch_bytes",
         "sla_hip_launch_salvage_crc", "sla_hip_launch_dec_conceal")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def header_text():
    return open(os.path.join(ROOT, "include", "sla_hip.h")).read()


def test_symbols_are_exported_declared_and_wrapped(L):
    text = header_text()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, text), name
    for name in ("salvage_resident_tensor", "salvage"):
        assert callable(getattr(sla_amd.Decoder, name)), name
    for macro in ("SLA_HIP_SALVAGE_MAX_BLOCK_BYTES(C, n)", "SLA_HIP_DEC_SALVAGE_SCRATCH_BYTES(data_size, node_capacity)",
                  "SLA_HIP_SALVAGE_CRC         1u", "SLA_HIP_SALVAGE_UNDECODABLE 2u", "SLA_HIP_SALVAGE_GAP         3u"):
        assert macro in text, macro
    assert (sla_amd.SALVAGE_CRC, sla_amd.SALVAGE_UNDECODABLE, sla_amd.SALVAGE_GAP) == (SM.CRC, SM.UNDECODABLE, SM.GAP) == (1, 2, 3)


@pytest.mark.parametrize("ctype, cname, size", [(sla_amd.SalvageReport, "sla_hip_salvage_report", 48),
                                                (sla_amd.SalvageRange, "sla_hip_salvage_range", 12),
                                                (sla_amd.SalvageScan, "sla_hip_salvage_scan", 48),
                                                (sla_amd.DecConceal, "sla_hip_dec_conceal", 8)])
def test_struct_layouts_follow_the_header(ctype, cname, size):
    assert C.sizeof(ctype) == size
    m = re.search(r"typedef struct %s \{(.*?)\} %s;\s*/\* (\d+) bytes \*/" % (cname, cname), header_text(), flags=re.S)
    assert m and int(m.group(2)) == size
    fields = re.findall(r"uint32_t (\w+)(?:\[(\d+)\])?;", m.group(1))
    assert [n for n, _ in fields] == [n for n, _ in ctype._fields_]
    off = 0
    for (name, count), (pname, ptype) in zip(fields, ctype._fields_):
        assert getattr(ctype, pname).offset == off, name
        assert C.sizeof(ptype) == 4 * int(count or 1), name
        off += C.sizeof(ptype)
    assert off == size


def test_scratch_macro_is_the_function_and_extends_the_wide_walks(L):
    for size in (0, 53, 54, 4096, 8177, 8178, 1 << 20, 82 * 1000 * 1000, 0xFFFFFFFF):
        for cap in (1, 2, 3, 4, 5, 1 << 16, 0xFFFFFFFF):
            got = L.sla_hip_dec_salvage_scratch_bytes(size, cap)
            # the macro of the header, evaluated here: the wide walk's scratch, 64 bytes of words, 28 bytes per node
            assert got == WW.scratch_bytes(size, cap) + 64 + ((cap + 3) & ~3) * 28, (size, cap)
            assert got == L.sla_hip_dec_wide_scratch_bytes(size, cap) + 64 + ((cap + 3) & ~3) * 28 and got % 16 == 0
    m = re.search(r"#define SLA_HIP_DEC_SALVAGE_SCRATCH_BYTES\(data_size, node_capacity\) \\\n(.*)\n", header_text())
    assert m and "SLA_HIP_DEC_WIDE_SCRATCH_BYTES(data_size, node_capacity) + 64u" in m.group(1) and "* 28u" in m.group(1)


def test_length_cap_is_four_raw_blocks_of_32_bits():
    m = re.search(r"#define SLA_HIP_SALVAGE_MAX_BLOCK_BYTES\(C, n\) \((.*)\)\n", header_text())
    assert m
    expr = re.sub(r"\(uint32_t\)", "", m.group(1)).replace("u", "")
    for ch, n in ((1, 0), (1, 1), (2, 4096), (8, 65535), (3, 2)):
        want = 64 + 16 * ch * max(n, 1)
        assert SM.max_block_bytes(ch, n) == want
        assert eval(expr.replace("?", " and ").replace(":", " or "), {"C": ch, "n": n}) == want
        assert want >= 4 * (11 + 4 * ch * n)              # four times a RAW block of 32-bit samples with its header


def _file(src=0x7000, size=4096, total=100, rows=4):
    f = sla_amd.DecWalkFile()
    f.src, f.data_size, f.total, f.capacity, f.max_rows = src, size, total, total, rows
    return f


def test_scan_launcher_refuses_before_any_launch(L):
    f = _file()
    p, s = C.c_void_p(0x1000), C.c_void_p(0x2000)
    W = L.sla_hip_launch_dec_salvage_scan
    assert W(None, 2, 4096, p, None, None, None, 64, s, None) == INVALID_ARGUMENT
    assert W(C.byref(f), 2, 4096, None, None, None, None, 64, s, None) == INVALID_ARGUMENT
    assert W(C.byref(f), 2, 4096, p, None, None, None, 64, None, None) == INVALID_ARGUMENT
    assert W(C.byref(f), 2, 4096, p, None, None, None, 0, s, None) == INVALID_ARGUMENT             # zero node capacity
    for nch in (0, 9):
        assert W(C.byref(f), nch, 4096, p, None, None, None, 64, s, None) == INVALID_ARGUMENT
    for off in (1, 4, 8, 15):                                                                      # misaligned scratch
        assert W(C.byref(f), 2, 4096, p, None, None, None, 64, C.c_void_p(0x2000 + off), None) == INVALID_ARGUMENT
    for tabs in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
        assert W(C.byref(f), 2, 4096, p, *tabs, 64, s, None) == INVALID_ARGUMENT, tabs             # a missing table
    assert W(C.byref(_file(src=0)), 2, 4096, p, None, None, None, 64, s, None) == INVALID_ARGUMENT  # a NULL source that has to be read


def test_crc_and_conceal_launchers_refuse_before_any_launch(L):
    p = C.c_void_p(0x1000)
    K = L.sla_hip_launch_salvage_crc
    for args in ((None, p, p, 4, p), (p, None, p, 4, p), (p, p, None, 4, p), (p, p, p, 4, None)):
        assert K(*args, None) == INVALID_ARGUMENT
    assert K(p, p, p, 0, p, None) == 0                       # nothing to do: no launch
    Z = L.sla_hip_launch_dec_conceal
    assert Z(None, 64, 2, p, 1, 8, None) == INVALID_ARGUMENT
    assert Z(p, 64, 2, None, 1, 8, None) == INVALID_ARGUMENT
    for nch in (0, 9):
        assert Z(p, 64, nch, p, 1, 8, None) == INVALID_ARGUMENT
    assert Z(p, 64, 2, p, 0, 8, None) == 0 and Z(p, 64, 2, p, 3, 0, None) == 0


def test_salvage_call_refuses_null_pointers_and_unknown_formats(L):
    rep = sla_amd.SalvageReport()
    rng = (sla_amd.SalvageRange * 2)()
    for k in range(12):
        setattr(rep, sla_amd.SalvageReport._fields_[k][0], 9)
    h, p = C.c_void_p(0x10), C.c_void_p(0x1000)
    F = L.sla_hip_salvage_resident
    assert F(None, p, 100, p, 8, 1, 8, 0, C.byref(rep), rng, 2, None) == INVALID_ARGUMENT
    assert F(h, None, 100, p, 8, 1, 8, 0, C.byref(rep), rng, 2, None) == INVALID_ARGUMENT
    assert F(h, p, 100, None, 8, 1, 8, 0, C.byref(rep), rng, 2, None) == INVALID_ARGUMENT
    assert F(h, p, 100, p, 8, 1, 8, 0, None, rng, 2, None) == INVALID_ARGUMENT
    assert F(h, p, 100, p, 8, 1, 8, 4, C.byref(rep), rng, 2, None) == INVALID_ARGUMENT             # unknown format
    assert F(h, p, 100, p, 8, 1, 8, 0, C.byref(rep), None, 2, None) == INVALID_ARGUMENT            # room promised, none given
    # refused before the handle or the report is touched: a dangling handle value shows it
    assert all(getattr(rep, n) == 9 for n, _ in sla_amd.SalvageReport._fields_)
