"""The model of one k_dec_bits launch (tests/decbitsmodel.py) and the files of tests/decbitscases.py, on the CPU.

The GPU tests of the entropy-decode kernel with several blocks per wave (tests/test_gpu_dec_bits_lanes.py) compare the
kernel with the writer's fields.  Here the oracle checks the other side of that comparison: the files are legal streams
(its decoder returns 0 on each), every compressed block's model samples are what its coder reads out of that block's
body bytes, used_bytes adds up to the file, and the planned sample ranges and canary gaps do not overlap."""
import numpy as np
import pytest

import crafted_catalogue as CC
import decbitscases as DC
import decbitsmodel as DM
import slalibs as S
import slastream as SS

CHANNELS = sorted(DC.FORMATS)
CASES = DC.launch_cases()


def _models(C):
    s = DC.suite(C)
    return s, (s.split, s.single)


@pytest.mark.parametrize("C", CHANNELS)
def test_files_are_legal_streams(oracle, C):
    _, models = _models(C)
    for m in models:
        for case in m.cases:
            rc, out, _ = oracle.decode_whole(S.make_params(cap=CC.CAP), case.data, case.num_samples)
            assert rc == 0 and out.shape == (C, case.num_samples), case.name


@pytest.mark.parametrize("C", CHANNELS)
def test_model_samples_are_what_the_oracle_coder_reads(oracle, C):
    """per compressed block: oracle.decode_residual of the block's own body bytes == the model's samples; and the
    header length the model computes from the fields is where that body starts"""
    s, models = _models(C)
    seen = 0
    for m in models:
        for it in m.items:
            blk = m.cases[it.file].blocks[it.block]
            want = m.pool[:, it.src:it.src + it.n]
            if blk.type != SS.COMPRESS:
                if blk.type == SS.SILENT:
                    assert not want.any() and it.byte_len == it.head == 11
                continue
            data = m.image[it.byte_off:it.byte_off + it.byte_len].tobytes()
            got = oracle.decode_residual(DM.residual_stream(m.fmt, blk, data), C, it.n, m.fmt.bits)
            assert np.array_equal(got, want), (m.cases[it.file].name, it.block)
            seen += 1
    assert seen == 2 * sum(b.type == SS.COMPRESS for b in s.menu.values())


@pytest.mark.parametrize("C", CHANNELS)
def test_used_bytes_sum_to_the_file(C):
    _, models = _models(C)
    for m in models:
        every = np.arange(len(m.items))
        la = m.launch(every, np.zeros(len(every), int), np.zeros(len(every), np.uint32))
        for f, case in enumerate(m.cases):
            mine = np.array([it.file == f for it in m.items])
            assert int(la.info[mine, 1].sum()) == len(case.data) - SS.HEADER_SIZE
            assert (la.ends[mine] == m.file_end[f]).all()
            assert m.file_off[f] % 4 == 0
            assert m.image[m.file_off[f]:m.file_end[f]].tobytes() == case.data
        covered = np.zeros(len(m.image), bool)
        for f in range(len(m.cases)):
            covered[m.file_off[f]:m.file_end[f]] = True
        assert not m.image[~covered].any()                     # the gaps between the files are zero
        assert not la.info[:, 3].any()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_planned_ranges_and_gaps_are_disjoint(case):
    s, model, plan, la = DC.build(case)
    assert len(la.blocks) == case.rows
    first, last, nxt = model.ranges(la)
    gap = nxt - last
    assert first[0] == 0 and (first[1:] == nxt[:-1]).all()    # in row order, nothing between a gap and the next row
    assert set(np.unique(gap)) <= set(DM.GAPS) and {0, 1, 3} == set(np.unique(gap))
    assert la.stride == nxt[-1] + DM.TAIL and la.stride < 8 << 20
    # what the model expects written is exactly the ranges of the rows that decode samples
    writes = np.zeros(la.stride, bool)
    for a, b, fl, cut in zip(first, last, la.blocks["flags"], la.cut):
        if not (fl & DM.HEADER_ONLY) and not cut:
            assert not writes[a:b].any()
            writes[a:b] = True
    canary = la.planes.view(np.uint32) == DM.CANARY
    assert canary[:, ~writes].all() and not (writes & la.free).any()
    assert (canary[:, writes].mean() < 0.01)                   # (a decoded sample may equal the canary by chance)
    assert la.cut.any() == case.cut and la.free.sum() == (la.blocks["num_samples"][la.cut]).sum()
    # rows and items agree
    n = np.array([it.n for it in model.items])
    assert (la.blocks["num_samples"] == n[la.item]).all()
    assert (la.blocks["byte_off"] + la.blocks["byte_len"] <= la.ends).all()


@pytest.mark.parametrize("C", CHANNELS)
def test_menu_reaches_the_rare_branches(C):
    """what the writer saw while it wrote the files: a tile of more than 64 bits per sample (the reader's far path),
    gamma escapes at quotients 15 / 16 / 17, Golomb moduli with and without a power of two, both coders; in the
    32-bit mid/side format a 33-bit RAW field and an initial parameter whose `<< 8` wraps"""
    s, models = _models(C)
    for m in models:
        st = SS.Stats()
        for case in m.cases:
            st.merge(case.stats)
        assert st.max_tile_bits_per_sample > 64
        assert st.gamma_escapes > 0 and {15, 16, 17} <= st.quotients
        mods = {g for ms in st.golomb_m for g in ms}
        assert any(g & (g - 1) == 0 for g in mods) and any(g & (g - 1) for g in mods) and max(mods) <= 8
        assert {"rice", "golomb"} == set(st.coder)
        if s.fmt.bits == 32:
            assert 33 in st.raw_widths and st.max_init >= 1 << 24
            raw = s.menu["raw70"].raw[1]
            assert (raw >> np.uint64(32)).any()
    far = s.menu["far"]
    assert far.n >= 200 and all(ch.init == 9 for ch in far.chans)
    assert sorted(b.n for b in s.menu.values() if b.type == SS.COMPRESS)[:5] == [1, 33, 63, 64, 65]
    assert max(b.n for b in s.menu.values()) <= 2100


@pytest.mark.parametrize("C", CHANNELS)
def test_files_decode_as_in_the_reference(oracle, ref, C):
    """the oracle's decoder, the yardstick of the whole-decoder tests, is the reference's on these files too"""
    _, models = _models(C)
    for m in models:
        for case in m.cases:
            ro, do, _ = oracle.decode_whole(S.make_params(cap=CC.CAP), case.data, case.num_samples)
            rr, dr, _ = ref.decode_whole(S.make_params(cap=CC.CAP), case.data, case.num_samples)
            assert ro == rr == 0 and np.array_equal(do, dr), case.name
