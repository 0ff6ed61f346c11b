"""CPU-only checks of the block index (sla_hip_index, include/sla_hip.h; sla_amd/csrc/sla_dec_index.c) against
tests/indexmodel.py: the rows, stop code and extent sla_hip_index_build gives on the crafted catalogue, on the streams of
the golden vectors and on truncated and chain-broken variants; the sidecar format -- byte-stable round trips and every
refusal of the deserialiser, each with a blob that breaks one rule and carries a correct checksum; and the rows of a window
planned from an index, held against the window walk of the bytes (tests/windowmodel.py)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import crafted_catalogue as CC
import indexmodel as IM
import sla_amd
import walkmodel as WM
import windowmodel as WN

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID_ARGUMENT = 2
FIXED, HEAD = 32, 44                     # the blob: fixed fields, the header bytes, then 16 bytes per row and the CRC16


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    lib = sla_amd.lib()
    lib.slai_crc16.argtypes = [C.c_void_p, C.c_size_t]
    lib.slai_crc16.restype = C.c_uint32
    lib.slai_index_window.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)] * 4
    lib.slai_index_window.restype = None
    return lib


@pytest.fixture(scope="module")
def golden_streams():
    out = []
    for path in sorted(glob.glob(os.path.join(HERE, "golden", "*.npz"))):
        z = np.load(path)
        if "sla" in z.files:
            out.append((os.path.basename(path), z["sla"].tobytes()))
    assert len(out) >= 4
    return out


def rows_of(x):
    return [tuple(int(v) for v in r) for r in x.blocks()]


def same_as_model(x, data):
    m = IM.index_of(data)
    assert x.data_size == len(data)
    assert (x.header is not None) == m.has_header
    assert (x.stop, x.extent, x.num_blocks) == (m.stop, m.extent, len(m.rows))
    assert rows_of(x) == m.rows
    if m.has_header:
        assert x.header.num_samples == m.total
    return m


def seal(L, body):
    """body + the library's CRC16 of it, little-endian"""
    a = np.frombuffer(bytes(body), np.uint8)
    crc = L.slai_crc16(a.ctypes.data, len(a))
    return bytes(body) + bytes([crc & 0xFF, crc >> 8])


def reseal(L, blob, edit):
    """the blob with edit(bytearray body) applied and a correct checksum again"""
    body = bytearray(blob[:-2])
    body = edit(body) or body
    return seal(L, body)


def put32(b, at, v):
    b[at:at + 4] = int(v).to_bytes(4, "little")


def chain_stream(head, blocks):
    """a stream of chain headers only: `head` (43 bytes) and (num_samples, payload bytes) per block"""
    out = bytearray(head)
    for n, payload in blocks:
        out += b"\xff\xff" + (4 + payload).to_bytes(4, "big") + b"\x00\x00" + n.to_bytes(2, "big") + bytes(payload)
    return bytes(out)


def test_rows_on_the_crafted_catalogue(L):
    cases = CC.catalogue()
    assert len(cases) == 52
    for c in cases:
        x = sla_amd.Index.build(c.data)
        m = same_as_model(x, c.data)
        assert (m.stop, m.extent) == (WM.OK, c.num_samples), c.name
        assert [r[0] for r in m.rows] == list(c.offsets), c.name
        assert x.header_result == 0


def test_rows_on_the_golden_streams_and_their_damaged_variants(L, golden_streams):
    for name, data in golden_streams:
        x = sla_amd.Index.build(data)
        m = same_as_model(x, data)
        assert m.stop == WM.OK and m.extent == m.total and len(m.rows) >= 1, name
        offs = [r[0] for r in m.rows]
        k = len(offs) // 2
        variants = {
            "cut at a block": data[:offs[k]], "ten bytes of a block": data[:offs[k] + 10], "cut inside a block": data[:offs[k] + 30],
            "header only": data[:43], "short header": data[:20], "empty": b"",
            "sync lost": data[:offs[k]] + b"\x7f" + data[offs[k] + 1:],
            "size wraps": data[:offs[k] + 2] + b"\xff\xff\xff\xff" + data[offs[k] + 6:],
            "size past the end": data[:offs[k] + 2] + b"\x7f\xff\xff\xff" + data[offs[k] + 6:],
            "a block too many samples": data[:offs[-1] + 8] + b"\xff\xff" + data[offs[-1] + 10:],
            "bad signature": b"XL*\x01" + data[4:], "bad version": data[:10] + b"\x00\x00\x00\x02" + data[14:],
            "header crc": data[:20] + bytes([data[20] ^ 1]) + data[21:],
        }
        want_stop = {"cut at a block": WM.DATA, "ten bytes of a block": WM.DATA, "cut inside a block": WM.DATA, "sync lost": WM.SYNC_LOST,
                     "size wraps": WM.DATA, "size past the end": WM.DATA, "a block too many samples": WM.BUF}
        for what, d in variants.items():
            y = sla_amd.Index.build(d)
            mv = same_as_model(y, d)
            if what in want_stop and (k > 0 or what == "a block too many samples"):
                assert mv.stop == want_stop[what], (name, what)
            assert sla_amd.Index.from_bytes(y.to_bytes()).to_bytes() == y.to_bytes(), (name, what)
        assert sla_amd.Index.build(variants["header crc"]).header_result == 11
        assert sla_amd.Index.build(variants["bad version"]).header is None


def test_serialise_round_trip_is_byte_stable(L, golden_streams):
    for name, data in golden_streams + [(c.name, c.data) for c in CC.catalogue()[::5]]:
        x = sla_amd.Index.build(data)
        blob = x.to_bytes()
        assert len(blob) == FIXED + HEAD + 16 * x.num_blocks + 2 and blob[:4] == b"SLAX"
        assert blob == seal(L, blob[:-2])
        y = sla_amd.Index.from_bytes(blob)
        assert y.to_bytes() == blob and rows_of(y) == rows_of(x), name
        assert (y.data_size, y.stop, y.extent, y.header_result) == (x.data_size, x.stop, x.extent, x.header_result)
        assert bytes(y.header) == bytes(x.header)
        if x.num_blocks >= 3:
            assert rows_of(x)[1:3] == [tuple(int(v) for v in r) for r in x.blocks(1, 2)] and len(x.blocks(3, 0)) == 0
    with pytest.raises(sla_amd.SlaError):
        x.blocks(x.num_blocks, 1)


def test_every_refusal_of_the_deserialiser(L, golden_streams):
    data = max((d for _, d in golden_streams), key=lambda d: sla_amd.Index.build(d).num_blocks)
    x = sla_amd.Index.build(data)
    blob = x.to_bytes()
    nb = x.num_blocks
    assert nb >= 3
    R = FIXED + HEAD                                     # the first row
    rows = rows_of(x)

    def refused(b):
        h = C.c_void_p(0x77)
        a = np.frombuffer(bytes(b), np.uint8) if len(b) else np.zeros(1, np.uint8)
        rc = L.sla_hip_index_deserialize(a.ctypes.data, len(b), C.byref(h))
        return rc == INVALID_ARGUMENT and not h.value

    def grow_last_block(b, n=65536):
        """the last block gets n samples and the header a total that covers them (its CRC then fails: result 11)"""
        put32(b, R + 16 * (nb - 1) + 12, n)
        put32(b, 24, rows[-1][2] + n)
        b[FIXED + 15:FIXED + 19] = (rows[-1][2] + n).to_bytes(4, "big")
        put32(b, 16, 11)

    assert sla_amd.Index.from_bytes(reseal(L, blob, lambda b: None)).to_bytes() == blob      # the helper itself is sound
    assert sla_amd.Index.from_bytes(reseal(L, blob, lambda b: grow_last_block(b, 65535))).extent == rows[-1][2] + 65535
    cases = {
        "magic": reseal(L, blob, lambda b: b.__setitem__(0, ord("X"))),
        "version": reseal(L, blob, lambda b: put32(b, 4, 2)),
        "checksum": blob[:-1] + bytes([blob[-1] ^ 0x40]),
        "a flipped row bit under the old checksum": blob[:R + 1] + bytes([blob[R + 1] ^ 1]) + blob[R + 2:],
        "truncated by a row": seal(L, blob[:-18]),
        "truncated inside the fixed part": blob[:20],
        "empty": b"",
        "bytes not ascending": reseal(L, blob, lambda b: put32(b, R + 16, rows[0][0])),
        "rows that overlap by one byte": reseal(L, blob, lambda b: put32(b, R + 16, rows[1][0] - 1)),
        "a first row that spans the stream over the second": reseal(L, blob, lambda b: put32(b, R + 4, len(data) - rows[0][0])),
        "samples not cumulative": reseal(L, blob, lambda b: put32(b, R + 16 + 8, rows[1][2] + 1)),
        "first row not at sample 0": reseal(L, blob, lambda b: put32(b, R + 8, 1)),
        "byte_off below 43": reseal(L, blob, lambda b: put32(b, R, 42)),
        "byte_len below 11": reseal(L, blob, lambda b: put32(b, R + 4, 10)),
        "a row past data_size": reseal(L, blob, lambda b: put32(b, R + 16 * (nb - 1) + 4, rows[-1][1] + 1)),
        "a row that wraps 32 bits": reseal(L, blob, lambda b: put32(b, R + 16 * (nb - 1) + 4, 0xFFFFFFF0)),
        "num_samples above 65535": reseal(L, blob, grow_last_block),
        "extent not the rows' end": reseal(L, blob, lambda b: put32(b, 24, x.extent - 1)),
        "extent above the header's total": reseal(L, blob, lambda b: (put32(b, R + 16 * (nb - 1) + 12, rows[-1][3] + 1), put32(b, 24, x.extent + 1)) and None),
        "header result that the bytes do not give": reseal(L, blob, lambda b: put32(b, 16, 11)),
        "header bytes held": reseal(L, blob, lambda b: put32(b, 12, 40)),
    }
    for what, b in cases.items():
        assert refused(b), what
    assert L.sla_hip_index_deserialize(None, 10, C.byref(C.c_void_p())) == INVALID_ARGUMENT
    # the same edits that stay inside the rules are taken: the refusals above are the rules', not the helper's
    y = sla_amd.Index.from_bytes(reseal(L, blob, lambda b: put32(b, R + 16 * (nb - 1) + 4, rows[-1][1] - 1)))
    assert rows_of(y)[-1][1] == rows[-1][1] - 1


def test_an_index_records_a_block_longer_than_any_handle_decodes(L):
    head = bytearray(CC.catalogue()[0].data[:43])
    head[15:19] = (20000 + 300).to_bytes(4, "big")
    data = chain_stream(head, [(100, 40), (20000, 900), (0, 7), (200, 30)])
    x = sla_amd.Index.build(data)
    m = same_as_model(x, data)
    assert x.header_result == 11 and x.header.num_samples == 20300          # the header CRC no longer holds; the fields are delivered
    assert [r[3] for r in m.rows] == [100, 20000, 0, 200] and (m.stop, m.extent) == (WM.OK, 20300)
    assert sla_amd.Index.from_bytes(x.to_bytes()).to_bytes() == x.to_bytes()
    # a window that needs the long block ends there with INSUFFICIENT_BUFFER_SIZE on a handle of 16384; one behind it is served
    assert IM.plan_window(m, 50, 100, 16384).stop == WM.BUF and IM.plan_window(m, 50, 100, 16384).rows == [m.rows[0]]
    p = IM.plan_window(m, 20100, 500, 16384)
    assert (p.stop, p.rows) == (WM.OK, [m.rows[3]])


def test_the_shortest_block_of_the_walk_has_no_sidecar(L):
    """the walk keeps a block whose size field + 6 is 8 to 10 when 11 bytes are left; the builder follows it, the
    deserialiser's floor is 11 (include/sla_hip.h): such an index is built and read, its blob is refused"""
    head = bytearray(CC.catalogue()[0].data[:43])
    head[15:19] = (70000).to_bytes(4, "big")
    # (the sample count lies at bytes 8..9 of a block: for one of 8 or 9 bytes, in the next block's sync code)
    for size_field, count in ((2, 0xFFFF), (3, 0x00FF), (4, 100)):
        short = b"\xff\xff" + size_field.to_bytes(4, "big") + b"\x00\x00" + (100).to_bytes(2, "big")      # 10 bytes; size field + 6 < 11
        data = chain_stream(head, [(200, 30)]) + short[:size_field + 6] + chain_stream(b"", [(300, 25)])
        x = sla_amd.Index.build(data)
        m = same_as_model(x, data)
        assert [(r[1], r[3]) for r in m.rows] == [(40, 200), (size_field + 6, count), (35, 300)] and m.stop == WM.DATA
        blob = x.to_bytes()
        assert len(blob) == FIXED + HEAD + 16 * x.num_blocks + 2
        with pytest.raises(sla_amd.SlaError):
            sla_amd.Index.from_bytes(blob)


def test_mutated_blobs_never_yield_an_index_that_names_bytes_outside_its_rows_ranges(L, golden_streams):
    """blobs with a few changed bytes and a correct checksum again: whatever the deserialiser takes has rows inside
    [43, data_size) that ascend without overlap -- so the byte range of any run of rows holds each of them whole --, plans
    windows inside its rows and serialises to the blob it came from"""
    data = max((d for _, d in golden_streams), key=lambda d: sla_amd.Index.build(d).num_blocks)
    blob = sla_amd.Index.build(data).to_bytes()
    nb = sla_amd.Index.build(data).num_blocks
    rng = np.random.default_rng(7)
    taken = 0
    for it in range(3000):
        b = bytearray(blob[:-2])
        if it % 2:
            # a row's start moved and its length changed, by a little or by a lot
            at = FIXED + HEAD + 16 * int(rng.integers(0, nb))
            off, blen = int.from_bytes(b[at:at + 4], "little"), int.from_bytes(b[at + 4:at + 8], "little")
            d = int(rng.integers(-3, 40)) if it % 4 == 1 else int(rng.integers(-len(data), len(data)))
            put32(b, at, (off + d) & 0xFFFFFFFF)
            put32(b, at + 4, (blen - d + int(rng.integers(-2, 3)) * int(rng.integers(0, 2))) & 0xFFFFFFFF)
        else:
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(FIXED + HEAD - 4, len(b))) if it % 4 else int(rng.integers(0, len(b)))
                b[at] = b[at] ^ (1 << int(rng.integers(0, 8))) if rng.integers(0, 2) else int(rng.integers(0, 256))
        m = seal(L, b)
        try:
            y = sla_amd.Index.from_bytes(m)
        except sla_amd.SlaError:
            continue
        taken += 1
        rows = rows_of(y)
        end = 43
        for off, blen, _, n in rows:
            assert off >= end and blen >= 11 and off + blen <= y.data_size and n <= 65535
            end = off + blen
        assert y.to_bytes() == m
        total = y.header.num_samples
        for _ in range(4):
            s, l = int(rng.integers(0, total + 2)), int(rng.integers(0, total + 2))
            if s < min(s + l, total):
                got, stop = c_plan(L, y, total, s, l, 4096)
                assert all(r in rows for r in got)
    assert taken >= 300


def c_plan(L, x, total, start, length, cap):
    v = [C.c_uint32() for _ in range(4)]
    L.slai_index_window(x.handle, total, start, length, cap, *[C.byref(a) for a in v])
    row0, nrows, kept, stop = [a.value for a in v]
    rows = [r for r in rows_of(x)[row0:row0 + nrows] if r[3] != 0]
    assert len(rows) == kept
    return rows, stop


def test_planned_windows_are_the_window_walks(L, golden_streams):
    head = bytearray(CC.catalogue()[0].data[:43])
    head[15:19] = (9000).to_bytes(4, "big")
    streams = [d for _, d in golden_streams]
    streams.append(chain_stream(head, [(0, 3), (3000, 50), (0, 1), (0, 5), (2500, 20), (3000, 60), (500, 9)]))
    streams.append(streams[-1][:-40])                                   # the last block is cut
    streams.append(streams[0][:len(streams[0]) * 2 // 3])
    checked = 0
    for data in streams:
        x = sla_amd.Index.build(data)
        m = IM.index_of(data)
        t = m.total
        starts = sorted({0, 1, t // 3, t - 1, t} | {r[2] for r in m.rows} | {max(r[2] - 1, 0) for r in m.rows})
        for cap in (16384, 2600):
            for s in starts:
                for l in (1, 2, 2999, t, 0xFFFFFFFF):
                    w = WN.walk(data, t, s, l, cap)
                    p = IM.plan_window(m, s, l, cap)
                    assert (p.rows, p.stop) == ([r[:4] for r in w.rows], w.stop), (len(data), s, l, cap)
                    assert (p.first_byte, p.first_sample, p.end_byte, p.end_sample) == (w.first_byte, w.first_sample, w.end_byte, w.end_sample)
                    if s < min(s + l, t):
                        assert c_plan(L, x, t, s, l, cap) == (p.rows, p.stop), (len(data), s, l, cap)
                    checked += 1
    assert checked > 500
