"""Device-free checks of the layout rule of sla_hip_splice_resident as tests/splicemodel.py states it: on every cut and
join of its catalogue the model's stream, decoded by the oracle's decoder AND by the reference library, is the concatenated
source windows bit for bit; blocks inside a cut are the source's bytes; the header fields are what was emitted; and the
claim the SILENT rule rests on -- a block is 11 bytes long exactly when it is SILENT -- holds over the catalogue."""
import numpy as np
import pytest

import crafted_catalogue as CC
import indexmodel as IM
import slalibs as S
import slastream as SS
import splicemodel as SM

CASES = SM.cases()
IDS = [name for name, _ in CASES]


def params():
    return S.make_params(cap=CC.CAP)


def test_the_catalogue_covers_what_it_claims():
    fmts = list(SM.FORMATS.values())
    assert {f.num_channels for f in fmts} == {1, 2, 8} and {f.bits for f in fmts} == {8, 16, 24, 32}
    assert {f.lshift for f in fmts} == {0, 3} and {(f.num_channels, f.ms) for f in fmts} >= {(2, 0), (2, 1)}
    assert {sum(SS.raw_widths(f)) for f in fmts} >= {16, 33, 65, 192}
    for files in SM.sources().values():
        for c in files:
            assert {b.type for b in c.blocks} == {SS.COMPRESS, SS.SILENT, SS.RAW}
            assert all(1 <= b.n <= 300 for b in c.blocks)
    kinds = set()
    for _, segs in CASES:
        kinds |= {b[0] for b in SM.splice(list(segs)).blocks}
    assert kinds == {SM.VERBATIM, SM.SILENT, SM.RAW}


def test_eleven_bytes_means_silent():
    n = 0
    for c in list(CC.catalogue()) + [c for files in SM.sources().values() for c in files]:
        x = IM.index_of(c.data)
        assert len(x.rows) == len(c.blocks)
        for row, b in zip(x.rows, c.blocks):
            assert (row[1] == 11) == (b.type == SS.SILENT), c.name
            n += b.type == SS.SILENT
    assert n >= 60


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_stream_decodes_to_the_source_windows(oracle, ref, case):
    _, segs = case
    m = SM.splice(list(segs))
    want = SM.expected_pcm(list(segs))
    assert m.rc == SM.OK and m.num_samples == want.shape[1] == sum(l for _, _, l in segs)
    ro, do, _ = oracle.decode_whole(params(), m.data, m.num_samples)
    rr, dr, _ = ref.decode_whole(params(), m.data, m.num_samples)
    assert ro == rr == 0, (ro, rr)
    assert do.shape == dr.shape == want.shape
    assert np.array_equal(do, want) and np.array_equal(dr, want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_verbatim_blocks_and_header_fields(case):
    _, segs = case
    m = SM.splice(list(segs))
    fmt = segs[0][0].fmt
    x = IM.index_of(m.data)
    assert x.has_header and x.stop == SM.OK and x.extent == x.total == m.num_samples
    assert len(x.rows) == m.num_blocks == len(m.blocks)
    W = sum(SS.raw_widths(fmt))
    for row, (kind, s, src_row, off, length, a, n) in zip(x.rows, m.blocks):
        assert (row[0], row[1], row[3]) == (off, length, n)
        src = segs[s][0].data
        if kind == SM.VERBATIM:
            assert m.data[off:off + length] == src[src_row[0]:src_row[0] + src_row[1]] and n == src_row[3]
        else:
            assert n < src_row[3] and m.data[off + 10] >> 6 == (1 if kind == SM.SILENT else 2)
            assert length == (11 if kind == SM.SILENT else 11 + (n * W + 7) // 8)
            # never larger than its PCM at the file's depth (one bit per frame more under mid/side) and the 11 header bytes
            assert length <= 11 + (n * (fmt.num_channels * fmt.bits + fmt.ms) + 7) // 8
            assert SS.crc16(m.data[off + 8:off + length]) == int.from_bytes(m.data[off + 6:off + 8], "big")
    assert m.edge_blocks <= 2 * len(segs)
    sizes = [r[1] for r in x.rows]
    hdr = m.data[:43]
    assert hdr == SS.header_bytes(fmt, m.num_samples, len(sizes), max(sizes, default=0),
                                  max((((8 * b * fmt.rate) & SS.M32) // r[3] for b, r in zip(sizes, x.rows)), default=0))
    assert hdr[14] == segs[0][0].data[14] and hdr[19:29] == segs[0][0].data[19:29] and hdr[33:35] == segs[0][0].data[33:35]
    if m.num_samples == 0:
        assert m.data == hdr and m.num_blocks == 0


def test_model_refusals():
    src = SM.sources()
    A, B = src["mono16"][0], src["stereo8"][0]
    assert SM.splice([(A, 0, 10), (B, 0, 10)]).rc == SM.INVALID_ARGUMENT
    assert SM.splice([]).rc == SM.INVALID_ARGUMENT
    assert SM.splice([(A, A.num_samples - 5, 6)]).rc == SM.DATA
    assert SM.splice([(A, A.num_samples, 0)]).rc == SM.OK
