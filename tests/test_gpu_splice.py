"""GPU tests of sla_hip_splice_resident (Decoder.splice_resident / cut_resident / join_resident; run with -m gpu on an
MI355X): new .sla streams cut and joined from resident ones without re-encoding.

The yardstick is tests/splicemodel.py, byte for byte: every cut and join of its catalogue in one call -- eight formats, so
eight passes -- in per-buffer mode at odd destination alignments between canaries and in arena mode; the outputs decoded by
decode_resident_tensor against decode_windows_tensor of the sources; an encoder-made stream; a cut inside a block of 65 535
samples; and the failures: each leaves its destination untouched while the other items of the call are delivered --
stale indexes, indexes forged through the sidecar format, items with two failures (the first in output order decides) and
40 items of one pass of which every third fails."""
import numpy as np
import pytest

import crafted_catalogue as CC
import longblockcases as LB
import slalibs as S
import slastream as SS
import splicemodel as SM
import test_gpu_decode_batch as TB
import test_gpu_decode_batch_resident as TR

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, BUF, DATA, CORRUPT = 0, 2, 4, 9, 11
CANARY = 0xA5


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


class Resident:
    """streams in device memory at odd offsets, and their indexes"""

    def __init__(self, hip, named):
        self.names = list(named)
        self.srcs, self.keep = TR.resident([named[k] for k in self.names])
        self.at = {k: (s, hip.Index.build(named[k])) for k, s in zip(self.names, self.srcs)}

    def segments(self, segs):
        return [(self.at[name][0], self.at[name][1], s, l) for name, s, l in segs]


@pytest.fixture(scope="module")
def crafted(hip):
    return Resident(hip, {c.name: c.data for files in SM.sources().values() for c in files})


def named(segs):
    return [(c.name, s, l) for c, s, l in segs]


def buffers(sizes, lead=1):
    """a canary buffer and one slice per size, every slice at an odd distance from the one before"""
    import torch
    offs, pos = [], lead
    for n in sizes:
        offs.append(pos)
        pos += n + (1 if (pos + n) % 2 == 0 else 2)
    buf = torch.full((pos + 64,), CANARY, dtype=torch.uint8, device="cuda")
    return buf, [buf[o:o + n] for o, n in zip(offs, sizes)], offs


def check_buffer(buf, offs, datas):
    """the delivered streams where they belong, canaries everywhere else (datas[i] None: nothing of item i written)"""
    want = np.full(buf.numel(), CANARY, np.uint8)
    for o, d in zip(offs, datas):
        if d is not None:
            want[o:o + len(d)] = np.frombuffer(d, np.uint8)
    got = buf.cpu().numpy()
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])


def test_every_model_case_per_buffer(hip, crafted):
    cases = SM.cases()
    models = [SM.splice(list(segs)) for _, segs in cases]
    buf, outs, offs = buffers([len(m.data) for m in models])
    dec = hip.Decoder(*CC.CAP)
    try:
        got = dec.splice_resident([crafted.segments(named(segs)) for _, segs in cases], outs=outs)
        assert dec.last_timing()[5] == len(SM.FORMATS)                   # one pass per format
    finally:
        dec.close()
    for (name, _), m, (rc, out) in zip(cases, models, got):
        assert rc == OK and out.numel() == len(m.data), name
        assert out.cpu().numpy().tobytes() == m.data, name
    check_buffer(buf, offs, [m.data for m in models])


def test_every_model_case_in_an_arena(hip, crafted):
    import torch
    cases = SM.cases()
    models = [SM.splice(list(segs)) for _, segs in cases]
    total = sum(len(m.data) for m in models)
    whole = torch.full((total + 3 + 64,), CANARY, dtype=torch.uint8, device="cuda")
    arena = whole[3:3 + total]
    dec = hip.Decoder(*CC.CAP)
    try:
        got = dec.splice_resident([crafted.segments(named(segs)) for _, segs in cases], arena=arena)
    finally:
        dec.close()
    spans = []
    for (name, _), m, (rc, out) in zip(cases, models, got):
        assert rc == OK and out.cpu().numpy().tobytes() == m.data, name
        spans.append((out.data_ptr() - arena.data_ptr(), len(m.data)))
    pos = 0
    for off, n in sorted(spans):                                          # back to back, no padding, the arena exactly full
        assert off == pos
        pos += n
    assert pos == total
    # items of one format lie in item order
    for fmt in SM.FORMATS:
        mine = [off for (name, _), (off, _) in zip(cases, spans) if name.startswith(fmt + "-")]
        assert mine == sorted(mine)
    host = whole.cpu().numpy()
    assert (host[:3] == CANARY).all() and (host[3 + total:] == CANARY).all()


def test_outputs_decode_to_the_windows_of_the_sources(hip, crafted):
    import torch
    picks = [c for c in SM.cases() if c[0].split("-")[1] in ("one_outside_at_both_ends", "join_three_with_cuts", "inside_one_raw_block")]
    dec = hip.Decoder(*CC.CAP)
    try:
        got = dec.splice_resident([crafted.segments(named(segs)) for _, segs in picks])
        for (name, segs), (rc, out) in zip(picks, got):
            assert rc == OK, name
            pcm, ns, rcs = dec.decode_resident_tensor([out], dtype=torch.int32)
            assert rcs == [OK] and ns == [sum(l for _, _, l in segs)], name
            parts = []
            for c, s, l in segs:
                if l:
                    w, n, r = dec.decode_windows_tensor([crafted.at[c.name][0]], [s], l, dtype=torch.int32)
                    assert r == [OK] and n == [l]
                    parts.append(w[0])
            assert torch.equal(pcm[0], torch.cat(parts, dim=1)), name
            assert np.array_equal(pcm[0].cpu().numpy(), SM.expected_pcm(list(segs))), name
    finally:
        dec.close()


def test_an_encoder_made_stream_cut_into_ten_windows(hip):
    import torch
    pcm = S.synth_pcm(2, 144000, 16, 48000, seed=4321)                    # 3 s, 16-bit stereo, blocks of up to 4096 samples
    data = TB.encode_clips(hip, TB.C4, [pcm])[0]
    res = Resident(hip, {"enc": data})
    src, x = res.at["enc"]
    assert x.extent == 144000 and x.num_blocks >= 36
    wins = [(0, 14400), (14400, 14400), (4096, 8192), (4095, 2), (100000, 44000), (143999, 1), (0, 144000), (7, 5000), (60000, 1), (33333, 66667)]
    dec = hip.Decoder(*TB.HANDLE_CAP)
    try:
        got = dec.splice_resident([[(src, x, s, l)] for s, l in wins])
        outs = [o for _, o in got]
        assert [rc for rc, _ in got] == [OK] * len(wins)
        for (s, l), out in zip(wins, outs):
            rc, lay = hip.splice_plan([(None, x, s, l)])
            assert rc == OK and lay.bytes == out.numel() and lay.edge_blocks <= 2
            assert bytes(lay.header)[:43] == out[:43].cpu().numpy().tobytes()
        dec_pcm, ns, rcs = dec.decode_resident_tensor(outs, dtype=torch.int32)
        assert rcs == [OK] * len(wins) and ns == [l for _, l in wins]
        for k, (s, l) in enumerate(wins):
            w, n, r = dec.decode_windows_tensor([src], [s], l, dtype=torch.int32)
            assert r == [OK] and torch.equal(dec_pcm[k, :, :l], w[0]), (s, l)
        whole = got[6][1].cpu().numpy().tobytes()
        assert whole[43:] == data[43:] and whole[15:19] == data[15:19] and whole[29:43] == data[29:43]      # a whole copy is the file
        rc, joined = dec.join_resident([outs[0], outs[1]], dec.index_resident([outs[0], outs[1]]))
        rc2, cut = dec.cut_resident(src, x, 0, 28800)
        assert rc == rc2 == OK
        a, _, _ = dec.decode_resident_tensor([joined], dtype=torch.int32)
        b, _, _ = dec.decode_resident_tensor([cut], dtype=torch.int32)
        assert torch.equal(a, b)
    finally:
        dec.close()


def test_a_cut_inside_a_block_of_65535_samples(hip):
    import torch
    c = LB.by_name()["encoded_140000_max65535"]
    res = Resident(hip, {"long": c.data})
    src, x = res.at["long"]
    assert [int(r["num_samples"]) for r in x.blocks()] == [65535, 65535, 8930]
    dec = hip.Decoder(*LB.CAP, long_blocks=True)
    try:
        wins = [(1000, 60000), (65000, 70000), (0, 140000), (131070 - 1, 3)]
        got = dec.splice_resident([[(src, x, s, l)] for s, l in wins])
        assert [rc for rc, _ in got] == [OK] * 4
        for (s, l), (_, out) in zip(wins, got):
            pcm, ns, rcs = dec.decode_resident_tensor([out], dtype=torch.int32)
            w, n, r = dec.decode_windows_tensor([src], [s], l, dtype=torch.int32)
            assert rcs == r == [OK] and ns == n == [l] and torch.equal(pcm, w), (s, l)
    finally:
        dec.close()


def flipped(data, at):
    return data[:at] + bytes([data[at] ^ 0x10]) + data[at + 1:]


def test_failures_leave_their_destination_untouched(hip):
    src = SM.sources()
    A, B, Cc = src["stereo16ms"]
    M = src["mono16"][0]
    hot_fmt = SS.Format(1, 16, order=8, ntaps=1, lms=8, max_block=2048)
    hot = SS.write_file(hot_fmt, [SS.Block(SS.COMPRESS, 100, [SS.Chan(0, [0] * 8, None, 0xFFFF, np.full(100, 1 << 20, np.int32))]),
                                  SS.Block(SS.SILENT, 50)])[0]
    offs = A.offsets
    ends = np.cumsum([b.n for b in A.blocks]).tolist()
    streams = {"A": A.data, "B": B.data, "M": M.data, "hot": hot,
               "A_chain": A.data[:offs[4] + 9] + bytes([A.data[offs[4] + 9] ^ 1]) + A.data[offs[4] + 10:],      # block 4: sample count
               "A_body": flipped(A.data, offs[4] + 40),                                                        # block 4: a body byte
               "A_type": A.data[:offs[2] + 10] + b"\x80" + A.data[offs[2] + 11:]}                               # the SILENT block 2: type RAW
    res = Resident(hip, streams)
    stale = {k: res.at["A"][1] for k in ("A_chain", "A_body", "A_type")}          # the index of the bytes before they changed
    N = A.num_samples

    def seg(name, s, l):
        return (res.at[name][0], stale.get(name, res.at[name][1]), s, l)

    good = [seg("A", 3, N - 5)]
    model_good = SM.splice([(A, 3, N - 5)]).data
    # (segments, result with enable_crc_check 1, result with 0, the stream delivered with 0 when that is not the model's)
    body_model = SM.splice([(A, 0, N)]).data
    body_copy = body_model[:offs[4] + 40] + bytes([body_model[offs[4] + 40] ^ 0x10]) + body_model[offs[4] + 41:]
    jobs = [
        ("clean", good, OK, OK, model_good),
        ("stale index, verbatim block", [seg("A_chain", 0, N)], CORRUPT, CORRUPT, None),
        ("stale index, edge block", [seg("A_chain", ends[3] + 1, 20)], CORRUPT, CORRUPT, None),
        ("flipped byte, verbatim block", [seg("A_body", 0, N)], CORRUPT, OK, body_copy),
        ("flipped byte, edge block", [seg("A_body", ends[3] + 1, 20)], CORRUPT, None, None),
        ("type bits of an 11-byte block", [seg("A_type", 0, N)], CORRUPT, CORRUPT, None),
        ("edge samples wider than the field", [seg("hot", 10, 50)], CORRUPT, CORRUPT, None),
        ("the same block copied whole", [seg("hot", 0, 150)], OK, OK, None),
        ("mismatched formats", [seg("A", 0, 10), seg("M", 0, 10)], INVALID_ARGUMENT, INVALID_ARGUMENT, None),
        ("past the extent", [seg("A", N - 1, 2)], DATA, DATA, None),
        ("clean again", good, OK, OK, model_good),
    ]
    sizes = [max(len(model_good), len(A.data)) + 100] * len(jobs)
    for crc in (1, 0):
        dec = hip.Decoder(*CC.CAP, enable_crc_check=crc)
        try:
            buf, outs, at = buffers(sizes)
            got = dec.splice_resident([j[1] for j in jobs], outs=outs)
            want_rc = [j[2] if crc else j[3] for j in jobs]
            datas = []
            for j, (rc, out), want in zip(jobs, got, want_rc):
                if want is None:                                         # a damaged edge without the CRC check: delivered or judged,
                    assert rc in (OK, CORRUPT), j[0]                      # whatever the damaged bytes decode to
                else:
                    assert rc == want, (j[0], crc, rc)
                datas.append(None if rc != OK else out.cpu().numpy().tobytes())
                if rc == OK and j[4] is not None:
                    assert datas[-1] == j[4], (j[0], crc)
            check_buffer(buf, at, datas)
            # a destination that is too small: per buffer, and an arena with room for one of two
            buf, outs, at = buffers([len(model_good), len(model_good) - 1, 42, len(model_good)])
            got = dec.splice_resident([good] * 4, outs=outs)
            assert [rc for rc, _ in got] == [OK, BUF, BUF, OK]
            check_buffer(buf, at, [model_good, None, None, model_good])
            buf, (arena,), at = buffers([2 * len(model_good) - 1])
            got = dec.splice_resident([good, [seg("A_chain", 0, N)], good, [seg("A", 0, 0)]], arena=arena)
            assert [rc for rc, _ in got] == [OK, CORRUPT, BUF, OK]
            empty = SM.splice([(A, 0, 0)]).data
            assert got[3][1].data_ptr() == arena.data_ptr() + len(model_good) and len(empty) == 43
            check_buffer(buf, at, [model_good + empty])
        finally:
            dec.close()


# ---- forged sidecars, several failures in one item, many items (tests/test_gpu_splice_check.py has the check kernel alone) ----

ROWS_AT = 76               # a sidecar: 32 bytes of fixed fields (num_blocks at 28), 44 of the header, 16 per row, the CRC16


def forged(hip, x, edit):
    """the index of x's sidecar with edit(rows) applied to its rows [[byte_off, byte_len, smp_off, num_samples]] and the
    checksum made right again: what a caller can hand in without ever having walked the stream"""
    import ctypes as C
    L = hip.lib()
    L.slai_crc16.argtypes = [C.c_void_p, C.c_size_t]
    L.slai_crc16.restype = C.c_uint32
    blob = x.to_bytes()
    rows = [[int(v) for v in r] for r in x.blocks()]
    assert len(blob) == ROWS_AT + 16 * len(rows) + 2
    edit(rows)
    body = bytearray(blob[:ROWS_AT])
    body[28:32] = len(rows).to_bytes(4, "little")
    for r in rows:
        body += b"".join(v.to_bytes(4, "little") for v in r)
    a = np.frombuffer(bytes(body), np.uint8)
    crc = int(L.slai_crc16(a.ctypes.data, len(a)))
    y = hip.Index.from_bytes(bytes(body) + bytes([crc & 0xFF, crc >> 8]))                 # the library accepts it
    assert [tuple(int(v) for v in r) for r in y.blocks()] == [tuple(r) for r in rows] and (y.extent, y.data_size) == (x.extent, x.data_size)
    return y


def count_flipped(data, off):
    """the block at `off` with another sample count in its chain header: an index made before fails on it, CRC check or not"""
    return data[:off + 9] + bytes([data[off + 9] ^ 1]) + data[off + 10:]


def test_forged_indexes_are_caught_on_the_device(hip):
    A = SM.sources()["stereo16ms"][0]
    assert [b.type for b in A.blocks[3:5]] == [SS.COMPRESS] * 2 and [b.type for b in A.blocks[7:9]] == [SS.COMPRESS] * 2
    ends = np.cumsum([b.n for b in A.blocks]).tolist()
    res = Resident(hip, {"A": A.data})
    src, honest = res.at["A"]
    assert honest.blocks()[8]["byte_len"] > 11

    def merge(rows):
        rows[3][1] += rows[4][1]
        rows[3][3] += rows[4][3]
        del rows[4]

    def move_a_sample(rows):
        rows[0][3] -= 1
        rows[1][2] -= 1
        rows[1][3] += 1

    def start_late(rows):
        rows[7][0] += 1
        rows[7][1] -= 1

    def claim_11_bytes(rows):
        rows[8][1] = 11

    # (the forgery, a cut that takes the forged rows verbatim, a cut that passes through them)
    forgeries = [(merge, (ends[2], ends[4] - ends[2]), (ends[2] + 10, 50)), (move_a_sample, (0, ends[1]), (10, 50)),
                 (start_late, (ends[6], ends[7] - ends[6]), (ends[6] + 5, 100)), (claim_11_bytes, (ends[6], ends[8] - ends[6]), (ends[7] + 2, 4))]
    jobs = []
    for edit, whole, through in forgeries:
        y = forged(hip, honest, edit)
        for s, l in (whole, through):
            rc, lay = hip.splice_plan([(None, y, s, l)])
            assert rc == OK and lay.edge_blocks == (0 if (s, l) == whole else 1), edit.__name__     # the layout rule has no objection
            jobs += [(edit.__name__, y, s, l, CORRUPT), (edit.__name__, honest, s, l, OK)]
    models = [SM.splice([(A, s, l)]).data for _, _, s, l, _ in jobs]
    for crc in (1, 0):
        dec = hip.Decoder(*CC.CAP, enable_crc_check=crc)
        try:
            buf, outs, at = buffers([len(m) + 40 for m in models])
            got = dec.splice_resident([[(src, x, s, l)] for _, x, s, l, _ in jobs], outs=outs)
            assert [rc for rc, _ in got] == [j[4] for j in jobs], crc
            check_buffer(buf, at, [m if j[4] == OK else None for j, m in zip(jobs, models)])
        finally:
            dec.close()


def test_the_first_failure_in_output_order_decides(hip):
    HEADER_FORMAT = 10
    A, B, Cc = SM.sources()["stereo16ms"]
    N, offs = A.num_samples, A.offsets
    assert A.blocks[0].type == A.blocks[10].type == SS.COMPRESS and len(A.blocks) == 11

    def type3(data, k):
        """block k with block type 3 and its CRC made right: the judge's INVALID_HEADER_FORMAT, not a corruption"""
        off, end = offs[k], (offs[k + 1] if k + 1 < len(offs) else len(data))
        d = bytearray(data)
        d[off + 10] |= 0xC0
        d[off + 6:off + 8] = SS.crc16(d[off + 8:end]).to_bytes(2, "big")
        return bytes(d)

    streams = {"A": A.data, "B": B.data, "C": Cc.data,
               "edge_then_verbatim": count_flipped(type3(A.data, 0), offs[4]), "verbatim_then_edge": count_flipped(type3(A.data, 10), offs[4]),
               "C_bad": count_flipped(Cc.data, Cc.offsets[2])}
    res = Resident(hip, streams)
    stale = {"edge_then_verbatim": "A", "verbatim_then_edge": "A", "C_bad": "C"}         # the indexes of the bytes before the damage

    def seg(name, s, l):
        return (res.at[name][0], res.at[stale.get(name, name)][1], s, l)

    two = [seg("A", 0, N), seg("B", 0, B.num_samples)]
    jobs = [([seg("edge_then_verbatim", 10, N - 10)], HEADER_FORMAT, None),             # block 0 is an edge: the judge's code
            ([seg("edge_then_verbatim", 0, N)], CORRUPT, None),                         # copied whole, a type of 3 is the decoder's to find
            ([seg("verbatim_then_edge", 0, N - 10)], CORRUPT, None),                    # block 4 comes before the edge block 10
            ([seg("verbatim_then_edge", ends_of(A)[4], N - 10 - ends_of(A)[4])], HEADER_FORMAT, None),
            (two + [seg("C_bad", 0, Cc.num_samples)], CORRUPT, None),
            (two, OK, SM.splice([(A, 0, N), (B, 0, B.num_samples)]).data),
            (two + [seg("C", 0, Cc.num_samples)], OK, SM.splice([(A, 0, N), (B, 0, B.num_samples), (Cc, 0, Cc.num_samples)]).data)]
    for crc in (1, 0):
        dec = hip.Decoder(*CC.CAP, enable_crc_check=crc)
        try:
            buf, outs, at = buffers([len(A.data) + len(B.data) + len(Cc.data) + 4096] * len(jobs))      # room for the RAW edges
            got = dec.splice_resident([j[0] for j in jobs], outs=outs)
            assert [rc for rc, _ in got] == [j[1] for j in jobs], crc
            check_buffer(buf, at, [j[2] for j in jobs])
        finally:
            dec.close()


def ends_of(case):
    return np.cumsum([b.n for b in case.blocks]).tolist()


def test_forty_items_every_third_one_failing(hip):
    """one format, one pass, about 300 entries of the check kernel: an item's failure is its own"""
    A = SM.sources()["mono16"][0]
    N, ends = A.num_samples, ends_of(A)
    damaged = {"bad%d" % k: count_flipped(A.data, A.offsets[k]) for k in range(len(A.blocks))}
    res = Resident(hip, dict(damaged, A=A.data))
    honest = res.at["A"][1]
    cuts = [(0, N), (3, N - 5), (10, 50), (ends[1], ends[6] - ends[1]), (ends[1] + 1, ends[6] - ends[1] - 2), (299, 1), (ends[5] + 3, 100)]
    items, models, want = [], [], []
    for i in range(40):
        if i % 3 == 0:
            k = (5 * (i // 3) + 1) % len(A.blocks)                    # the failing block's ordinal: 1, 6, 0, 5, 10, 4, ...
            items.append([(res.at["bad%d" % k][0], honest, 3, N - 5)])
            models.append(None)
            want.append(CORRUPT)
        else:
            s, l = cuts[i % len(cuts)]
            items.append([(res.at["A"][0], honest, s, l)])
            models.append(SM.splice([(A, s, l)]).data)
            want.append(OK)
    for crc in (1, 0):
        dec = hip.Decoder(*CC.CAP, enable_crc_check=crc)
        try:
            buf, outs, at = buffers([len(SM.splice([(A, 3, N - 5)]).data) + 64] * len(items))           # what a failed item would take
            got = dec.splice_resident(items, outs=outs)
            assert dec.last_timing()[5] == 1
            assert [rc for rc, _ in got] == want, crc
            for (rc, out), m in zip(got, models):
                assert m is None or out.cpu().numpy().tobytes() == m
            check_buffer(buf, at, models)
        finally:
            dec.close()
