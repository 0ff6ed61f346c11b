"""CPU tests of tests/windowmodel.py, the specification of the window walk (k_dec_walk_window): on chains written with
tests/slastream.py the kept blocks are those of the whole-file walk (tests/walkmodel.py) that overlap the window, for
every window on a grid that hits every block boundary +-1; a hint at any block at or before the window gives the same
rows with fewer blocks passed over; and damage to the chain is seen exactly when it lies between where the walk starts
and the window's end.  No GPU, no reference tree."""
import pytest

import test_gpu_dec_walk as TW
import walkmodel as WM
import windowmodel as WN

M32 = 0xFFFFFFFF


def chain_only(data, total):
    """the whole-file walk with neither a capacity nor a block-size limit: every block up to the chain's own stop"""
    return WM.walk(data, total, M32, 0xFFFF, 0)


def expected(full, total, start, length, cap_n):
    """(rows, stop) a window must give, derived from the whole-file walk alone"""
    end = min(start + length, total)
    reached = sum(r[3] for r in full.rows)                      # the sample position at which the whole-file walk stopped
    rows = [r for r in full.rows if r[3] > 0 and r[2] + r[3] > start and r[2] < end]
    stop = full.stop if (full.stop != WM.OK and reached < end) else WM.OK
    for k, r in enumerate(rows):
        if r[3] > cap_n:
            return rows[:k], WM.BUF
    return rows, stop


def grid(bounds, total):
    pts = sorted({p for b in bounds for p in (b - 1, b, b + 1) if 0 <= p <= total + 2})
    return [(s, e - s) for s in pts for e in pts if e >= s]


def bounds_of(full, total):
    return sorted({0, total} | {r[2] for r in full.rows} | {r[2] + r[3] for r in full.rows})


def as_rows(w):
    return [(off, blen, pos, n) for off, blen, pos, n, _ in w.rows]


def check_window(data, total, start, length, cap_n, full, what):
    w = WN.walk(data, total, start, length, cap_n)
    rows, stop = expected(full, total, start, length, cap_n)
    assert as_rows(w) == [r[:4] for r in rows], (what, start, length)
    assert [r[4] for r in w.rows] == [r[5] for r in rows], (what, start, length)        # the stored CRC fields
    assert w.stop == stop, (what, start, length)
    if rows:
        assert (w.first_byte, w.first_sample) == (rows[0][0], rows[0][2])
        assert (w.end_byte, w.end_sample) == (rows[-1][0] + rows[-1][1], rows[-1][2] + rows[-1][3])
    else:
        assert (w.first_byte, w.first_sample, w.end_byte, w.end_sample) == (0, 0, 0, 0)
    return w


@pytest.mark.parametrize("lens", [[300, 200, 0, 500, 123], [0, 0, 77, 0], [0, 5, 0, 0, 9, 1, 0]])
def test_clean_chains_keep_exactly_the_overlapping_blocks(lens):
    data, _ = TW._chain(lens, seed=11)
    total = sum(lens)
    full = WM.walk(data, total, total, 4096)
    assert full.stop == WM.OK and sum(1 for r in full.rows if r[3]) == sum(1 for n in lens if n)
    for start, length in grid(bounds_of(full, total), total):
        w = check_window(data, total, start, length, 4096, full, lens)
        assert w.stop == WM.OK
        if start < total and length > 0:
            # the kept blocks cover the window; every other block the walk came by was passed over
            assert w.first_sample <= start and w.end_sample >= min(start + length, total)
            assert w.skipped == sum(1 for r in full.rows if r[0] < w.end_byte) - w.num_blocks
        elif start >= total:
            assert w.num_blocks == 0          # (the call answers start >= total and length == 0 without a walk)


def test_window_end_is_computed_in_64_bits():
    lens = [300, 200, 0, 500, 123]
    data, _ = TW._chain(lens, seed=11)
    total = sum(lens)
    w = WN.walk(data, total, 400, M32, 4096)
    assert w.stop == WM.OK and [r[2] for r in w.rows] == [300, 500, 1000] and w.skipped == 2
    assert WN.walk(data, total, M32, M32, 4096).num_blocks == 0


@pytest.mark.parametrize("lens", [[300, 200, 0, 500, 123], [0, 0, 77, 0]])
def test_a_hint_at_any_block_at_or_before_the_window_gives_the_same_rows(lens):
    data, _ = TW._chain(lens, seed=12)
    total = sum(lens)
    full = WM.walk(data, total, total, 4096)
    for start, length in grid(bounds_of(full, total), total):
        plain = WN.walk(data, total, start, length, 4096)
        for k, r in enumerate(full.rows):
            if r[2] > start:
                break
            w = WN.walk(data, total, start, length, 4096, seek_byte=r[0], seek_sample=r[2])
            assert (w.rows, w.stop) == (plain.rows, plain.stop), (start, length, k)
            if plain.num_blocks:
                assert w.skipped == plain.skipped - k, (start, length, k)
                assert (w.first_byte, w.first_sample, w.end_byte, w.end_sample) == \
                    (plain.first_byte, plain.first_sample, plain.end_byte, plain.end_sample)


def test_damage_is_seen_between_the_walks_start_and_the_windows_end():
    seen = set()
    for name, data, total, _, cap_n in TW._cases():
        full = chain_only(data, total)
        for start, length in grid(bounds_of(full, total), total):
            w = check_window(data, total, start, length, cap_n, full, name)
            seen.add((name, w.stop))
    stops = {}
    for name, stop in seen:
        stops.setdefault(name, set()).add(stop)
    # damage in front of the window gives its stop code, a window that ends in front of it is served
    for name in ("no sync at a later block", "size field 0xFFFFFFFF wraps", "size field below the CRC start",
                 "size field runs past the end", "the stream ends before total (off == data_size)"):
        assert WM.OK in stops[name] and len(stops[name]) == 2, (name, stops[name])
    assert stops["no sync at a later block"] == {WM.OK, WM.SYNC_LOST}
    assert stops["no sync at the first block"] == {WM.OK, WM.SYNC_LOST}          # OK: the empty windows alone
    assert stops["block larger than the handle's blocks"] == {WM.OK, WM.BUF}
    assert stops["clean, total reached at the last block"] == {WM.OK}


def test_an_oversized_block_is_passed_over_in_front_of_the_window_and_stops_the_walk_inside_it():
    name, data, total, _, cap_n = [c for c in TW._cases() if c[0] == "block larger than the handle's blocks"][0]
    assert cap_n == 499                                                         # block 3 has 500 samples, at [500, 1000)
    w = WN.walk(data, total, 1000, 50, cap_n)
    assert w.stop == WM.OK and [r[2] for r in w.rows] == [1000] and w.skipped == 4
    w = WN.walk(data, total, 999, 50, cap_n)
    assert w.stop == WM.BUF and w.num_blocks == 0 and w.skipped == 3
    w = WN.walk(data, total, 250, 300, cap_n)
    assert w.stop == WM.BUF and [r[2] for r in w.rows] == [0, 300]


def test_damage_behind_a_hint_is_not_seen():
    lens = [300, 200, 0, 500, 123]
    clean, offs = TW._chain(lens, seed=1)
    total = sum(lens)
    by = {c[0]: c for c in TW._cases()}
    for name, hint_block in (("no sync at the first block", 1), ("no sync at a later block", 4), ("size field 0xFFFFFFFF wraps", 2),
                             ("size field 0xFFFFFFFA wraps to 0", 3), ("size field below the CRC start", 4)):
        data = by[name][1]
        assert len(data) == len(clean) and data != clean
        full = WM.walk(clean, total, total, 4096)
        hint = full.rows[hint_block]
        start = hint[2] + 1
        assert WN.walk(data, total, start, 40, 4096).stop != WM.OK, name        # without the hint the damage is in the way
        w = WN.walk(data, total, start, 40, 4096, seek_byte=hint[0], seek_sample=hint[2])
        want = WN.walk(clean, total, start, 40, 4096, seek_byte=hint[0], seek_sample=hint[2])
        assert w.stop == WM.OK and w.rows == want.rows and w.num_blocks >= 1, name


def test_a_wrong_hint_stays_inside_the_stream():
    """a hint is the caller's promise; whatever it says, the model (like the kernel) looks at no byte outside the data"""
    lens = [300, 200, 0, 500, 123]
    data, offs = TW._chain(lens, seed=1)
    total = sum(lens)
    for seek in (43, 44, offs[1] + 3, len(data) - 11, len(data) - 10, len(data), len(data) + 1, M32):
        w = WN.walk(data, total, 600, 100, 4096, seek_byte=seek, seek_sample=100)
        for off, blen, pos, n, _ in w.rows:
            assert off + blen <= len(data) and n <= 4096
        if seek > len(data) - 11:
            assert w.stop == WM.DATA and w.num_blocks == 0


def test_table_rows_rebase_on_the_first_kept_block():
    lens = [300, 200, 0, 500, 123]
    data, _ = TW._chain(lens, seed=1)
    w = WN.walk(data, sum(lens), 450, 100, 4096)
    rows, end, crcs = WN.table_rows(w, img_off=4096, plane_off=640)
    assert [r[0] for r in rows] == [4096 + r[0] - w.first_byte for r in w.rows]
    assert rows[0][:1] == (4096,) and rows[0][2] == 640 and rows[1][2] == 640 + 200
    assert end == 4096 + w.end_byte - w.first_byte and len(crcs) == 2
