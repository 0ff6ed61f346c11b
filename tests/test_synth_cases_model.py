"""The tables of tests/synthcases.py held to account without a device: their shape, the conditions that keep
tests/test_gpu_dec_synth.py from passing on a kernel that does nothing or that never meets a hostile neighbour, the
oracle functions the expected planes come from against the reference (skipped where the reference library is not
built), and the two plain-integer models against the oracle's own loops.

Which waves can mix lengths is decided by the kernels' job numbering, j = block * C + ch with JPW = 64 / G jobs per
wave, not by the tables: a wave spans two blocks always for JPW > C, one time in three for JPW = 2 with C = 3, and never
where JPW divides C (8 channels at LMS order 4 and at PARCOR order 16: every wave is one block's channels, and the job
count is a multiple of JPW whatever the rows).  So the bars below are: three quarters of the waves that span blocks
hold two or more lengths; where every wave spans blocks that is also at least half of all waves; where none can, the
table says so and is held to the workgroup rule alone.
"""
import numpy as np
import pytest

import synthcases as SC
import tailmodel as TM

LMS_IDS = [SC.lms_name(*a) for a in SC.LMS_TABLES]
LAT_IDS = [SC.lattice_name(*a) for a in SC.LATTICE_TABLES]


def check_shape(t):
    nb, C = len(t.blocks), t.C
    off, n = t.blocks["smp_off"].astype(np.int64), t.blocks["num_samples"].astype(np.int64)
    assert len(t.jobs) == nb * C and t.planes.shape == t.want.shape == (C, t.stride)
    assert t.info.shape == (nb, 4) and not t.info[:, 1:].any() and set(t.info[:, 0].tolist()) == {0, 1, 2, 3}
    assert (t.body >= n).all() and ((t.body == n) | (n == 0)).all()
    # every block and its gap inside the stride, no two overlapping: the rows lie in the planes in row order
    assert off[0] == 0 and np.array_equal(off[1:], (off + t.body + SC.GAP)[:-1])
    assert off[-1] + t.body[-1] + SC.GAP + SC.TAIL == t.stride
    covered = np.zeros(t.stride, bool)
    for r in range(nb):
        covered[off[r]:off[r] + t.body[r]] = True
    assert (t.planes[:, ~covered] == SC.CANARY).all() and (t.want[:, ~covered] == SC.CANARY).all()
    assert (~covered).sum() == nb * SC.GAP + SC.TAIL
    # live words everywhere else, in the rows to be skipped too
    assert (t.planes[:, covered] != SC.CANARY).mean() > 0.99
    skipped = {"type 1": 0, "type 2": 0, "type 3": 0, "header only": 0, "empty": 0}
    for j, job in enumerate(t.jobs):
        r = job.row
        ch, a, b = t.region(j)
        assert (ch, job.n) == (j % C, int(n[r])) and a == off[r]
        typ, flags = int(t.info[r, 0]), int(t.blocks["flags"][r])
        assert job.live == (typ == 0 and flags == 0)
        whole = slice(a, a + int(t.body[r]))
        untouched = (not job.live) or job.n == 0 or (t.stage == "lms" and job.n < t.order)
        if untouched:
            assert np.array_equal(t.want[ch, whole], t.planes[ch, whole]), (t.name, j)
        if typ != 0:
            skipped["type %d" % typ] += 1
        elif flags:
            skipped["header only"] += 1
        elif job.n == 0 and t.body[r] > 0:
            skipped["empty"] += 1
        if not job.live or (job.n == 0 and t.body[r] > 0):
            x = t.planes[ch, whole].astype(np.int64)
            assert job.family == "full" and len(x) >= 40 and np.abs(x).max() > 2 ** 30     # live full-range samples
    assert all(v == C for v in skipped.values()), skipped
    if t.stage == "lattice":
        assert t.kint.shape == (nb * C, t.order + 1) and (t.kint[:, 0] == SC.KINT_UNREAD).all()
        if t.order:
            assert (t.kint[:, 1:] != 0).any(axis=1).all()                                 # live coefficients in every row


def check_not_vacuous(t):
    per_wg = 4 * t.jpw
    jobs = len(t.jobs)
    assert jobs > per_wg and jobs % per_wg != 0, (t.name, jobs)
    waves = t.waves
    if t.spans_blocks:
        assert jobs % t.jpw != 0, (t.name, jobs)
        spanning, mixed = t.spanning_waves(), t.mixed_waves()
        assert spanning >= len(waves) // 3 and 4 * mixed >= 3 * spanning, (t.name, len(waves), spanning, mixed)
        if t.jpw > t.C:
            assert 2 * mixed >= len(waves), (t.name, len(waves), mixed)
        assert t.waves_with_skipped_neighbour() >= 1, t.name
    elif t.jpw > 1:
        assert t.C % t.jpw == 0 and t.spanning_waves() == 0           # no table at this C could do otherwise
        # what such a table still offers a wave: neighbours of different operand families
        assert sum(len({j.family for j in w}) >= 2 for w in waves) * 2 >= len(waves)
    total = changed = 0
    for j, job in enumerate(t.jobs):
        counts = job.live and (job.n > t.order if t.stage == "lms" else (job.n >= 2 and t.order >= 1))
        if counts:
            ch, a, b = t.region(j)
            total += 1
            changed += not np.array_equal(t.want[ch, a:b], t.planes[ch, a:b])
    if t.stage == "lms" or t.order >= 1:
        assert total >= 40 and 4 * changed >= 3 * total, (t.name, changed, total)
    elif t.deemphasis:
        assert (t.want != t.planes).any()                             # order 0: the de-emphasis alone


def check_coverage(t, lengths):
    seen = {(job.n, job.family) for job in t.jobs if job.live}
    for n in lengths:
        for fam in TM.FAMILIES:
            assert (n, fam) in seen, (t.name, n, fam)
    if t.stage == "lattice":
        pairs = {(job.n, job.kind) for job in t.jobs if job.live}
        for n in lengths:
            for kind in SC.KINDS:
                assert (n, kind) in pairs, (t.name, n, kind)
        assert {(job.family, job.kind) for job in t.jobs if job.live} >= {(f, k) for f in TM.FAMILIES for k in SC.KINDS}


@pytest.mark.parametrize("order,C", SC.LMS_TABLES, ids=LMS_IDS)
def test_lms_table_is_sound(order, C):
    t = SC.lms_table(order, C)
    assert (t.G, t.jpw, t.kint) == (2 * order, 64 // (2 * order), None)
    g = 2 * order
    want_lengths = {0, 1, order - 1, order, order + 1, g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1, 3 * g + order + 1, 777}
    assert set(SC.lms_lengths(order)) == want_lengths
    check_shape(t)
    check_coverage(t, want_lengths)
    check_not_vacuous(t)
    # the expected planes are the oracle's, job by job
    import slalibs
    O = slalibs.oracle()
    for j in range(0, len(t.jobs), 7):
        job = t.jobs[j]
        ch, a, b = t.region(j)
        if job.live and job.n:
            assert np.array_equal(t.want[ch, a:b], O.lms_synth(t.planes[ch, a:b], order))


@pytest.mark.parametrize("order,deemphasis,C", SC.LATTICE_TABLES, ids=LAT_IDS)
def test_lattice_table_is_sound(order, deemphasis, C):
    t = SC.lattice_table(order, deemphasis, C)
    G, R = SC.lattice_shape(order)
    assert (t.G, t.jpw) == (G, 64 // G) and G * R >= order and (G * R == 16 or G * R // 2 < order)
    want_lengths = {0, 1, 15, 16, 17, G - 1, G, G + 1, 2 * G + 5, 300}
    assert set(SC.lattice_lengths(order)) == want_lengths
    check_shape(t)
    check_coverage(t, want_lengths)
    check_not_vacuous(t)
    import slalibs
    O = slalibs.oracle()
    for j in range(0, len(t.jobs), 7):
        job = t.jobs[j]
        ch, a, b = t.region(j)
        if job.live and job.n:
            y = O.lattice_synth(t.planes[ch, a:b], t.kint[j])
            assert np.array_equal(t.want[ch, a:b], O.deemph_i32(y) if deemphasis else y)


def test_the_tables_are_the_ones_asked_for():
    assert SC.LMS_TABLES == ((4, 1), (8, 1), (16, 1), (32, 1), (4, 3), (8, 3), (4, 8))
    lat = set(SC.LATTICE_TABLES)
    assert len(lat) == len(SC.LATTICE_TABLES)
    for order in (0, 1, 15, 16, 17, 32, 33, 64, 65, 128, 129, 255):
        assert (order, 0, 1) in lat and (order, 1, 1) in lat
    assert {SC.lattice_shape(o) for o, d, c in lat if c == 3} == {(16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}
    assert [(o, c) for o, d, c in lat if c == 8] == [(16, 8)]
    # the specialisation changes exactly where the launcher's thresholds lie
    assert [SC.lattice_shape(o) for o in (16, 17, 32, 33, 64, 65, 128, 129, 255)] == [
        (16, 1), (32, 1), (32, 1), (64, 1), (64, 1), (64, 2), (64, 2), (64, 4), (64, 4)]
    # tables are built once and frozen
    t = SC.lms_table(4, 1)
    assert t is SC.lms_table(4, 1)
    for a in (t.blocks, t.info, t.planes, t.want, SC.lattice_table(16, 1, 8).kint):
        assert not a.flags.writeable


def test_explain_names_the_job():
    t = SC.lattice_table(17, 0, 3)
    j = next(i for i, job in enumerate(t.jobs) if job.live and job.n == 300 and job.ch == 2)
    ch, a, b = t.region(j)
    got = t.want.copy()
    got[ch, a + 123] ^= 1
    said = SC.explain(t, got)
    job = t.jobs[j]
    for item in (t.name, "row", job.row, "n", 300, "channel", 2, "family", job.family, "kint", job.kind, "sample 123"):
        assert item in said, (item, said)
    got = t.want.copy()
    got[ch, b + 4] = 0
    assert "the gap behind it, word 4" in SC.explain(t, got)


# ---- the yardstick itself ----------------------------------------------------------------------------------------------

def test_lattice_oracle_equals_the_reference(oracle, ref):
    """every (order, coefficient kind, family) the tables use, at lengths 1, 17, 65 and 300"""
    cases = 0
    for order in SC.LATTICE_ORDERS:
        for kind in SC.KINDS:
            kint = SC.coefs(kind, order, seed=order)
            for fam in TM.FAMILIES:
                for n in SC.PIN_LENGTHS:
                    x = TM.family(fam, n, seed=order)
                    assert np.array_equal(oracle.lattice_synth(x, kint), ref.lattice_synth(x, kint)), (order, kind, fam, n)
                    cases += 1
    assert cases == 12 * 3 * 8 * 4


def test_lms_oracle_equals_the_reference(oracle, ref):
    """every (order, family, length) of the LMS tables with n >= 1"""
    cases = 0
    for order in sorted({o for o, c in SC.LMS_TABLES}):
        for fam in TM.FAMILIES:
            for n in SC.lms_lengths(order):
                if n >= 1:
                    x = TM.family(fam, n, seed=order)
                    assert np.array_equal(oracle.lms_synth(x, order), ref.lms_synth(x, order)), (order, fam, n)
                    cases += 1
    assert cases == 4 * 8 * 12


# ---- the two plain-integer models --------------------------------------------------------------------------------------

def test_deemphasis_model_equals_the_oracle(oracle):
    for fam in TM.FAMILIES:
        for n in (1, 2, 301):
            x = TM.family(fam, n)
            assert np.array_equal(SC.deemphasis(x, 0, 5), oracle.deemph_i32(x)), (fam, n)
    # by hand: y[-1] = -1, shift 1: numerator 1; -1 >> 1 = -1
    assert SC.deemphasis([10, 0, -2 ** 31], -1, 1).tolist() == [9, 4, -2 ** 31 + 2]
    # shift 30 on INT32_MIN: -2^31 * (2^30 - 1) wraps to -2^31, >> 30 = -2; then -2 * (2^30 - 1) = -2^31 + 2, >> 30 = -2
    assert SC.deemphasis([0, 0], -2 ** 31, 30).tolist() == [-2, -2]


def test_finish_model_on_hand_computed_values():
    """the loop at the end of the oracle's decoder (oracle/sla_oracle.c, slao_decode_whole): side = p1,
    mid = (p0 << 1) | (side & 1), left = (mid + side) >> 1, right = (mid - side) >> 1, every sum wrapping; then << shift.
    Columns: side odd, side even, both negative, mid << 1 wrapping, both INT32_MIN, both INT32_MAX"""
    p = np.array([[5, 5, -3, 2 ** 30, -2 ** 31, 2 ** 31 - 1],
                  [3, 2, -5, 1, -2 ** 31, 2 ** 31 - 1]], np.int64).astype(np.int32)
    left = [7, 6, -5, -(2 ** 30) + 1, -2 ** 30, 2 ** 30 - 1]
    right = [4, 4, 0, -2 ** 30, -2 ** 30, -2 ** 30]
    assert SC.finish(p, 1, 0).tolist() == [left, right]
    assert SC.finish(p, 1, 8).tolist() == [[1792, 1536, -1280, 256, 0, -256], [1024, 1024, 0, 0, 0, 0]]
    # shift 31 keeps the low bit alone, as the sign
    assert SC.finish(p, 1, 31).tolist() == [[-2 ** 31, 0, -2 ** 31, -2 ** 31, 0, -2 ** 31], [0] * 6]
    # without mid/side the planes are shifted and nothing else, any number of them
    q = np.array([[1], [-1], [0x12345]], np.int32)
    assert SC.finish(q, 0, 16).tolist() == [[65536], [-65536], [0x23450000]]
    assert SC.finish(q, 0, 0).tolist() == q.tolist() and SC.finish(q, 0, 31).tolist() == [[-2 ** 31], [-2 ** 31], [-2 ** 31]]
    assert SC.finish(q, 0, 16).dtype == np.int32 and SC.finish(p, 1, 0).shape == p.shape
