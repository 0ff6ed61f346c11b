"""Hand-made tables for the two synthesis kernels that pack several (block, channel) jobs into one wave, k_dec_lms<ORDER>
and k_dec_lattice<G, R> (sla_amd/csrc/sla_decode.hip), and plain-integer models of the two small kernels beside them,
k_dec_deemphasis and k_dec_finish (test infrastructure: numpy and the CPU oracle, no device).

A table is what one launch of sla_hip_launch_dec_lms / sla_hip_launch_dec_lattice gets: sla_hip_dec_block rows, their info
rows (type, 0, 0, 0), for the lattice the kint rows [(block * C + ch)][order + 1], and planes [C][stride] in which every
block is followed by GAP canary words and the plane ends in TAIL of them.  Job j = block * C + ch is what the kernels number:
k_dec_lms<ORDER> gives a job G = 2 * ORDER lanes, k_dec_lattice<G, R> gives it G lanes, so a wave holds JPW = 64 / G jobs
j = wave * JPW .. + JPW - 1 and a workgroup of four waves 4 * JPW.  The rows are shuffled, so that the jobs that share a wave
differ in length, operand family and coefficient kind, and rows the kernels must skip sit between live ones.

`want` comes from the oracle alone (slalibs.oracle(): lms_synth; lattice_synth, then deemph_i32), one call per job with zero
state.  tests/test_synth_cases_model.py holds the tables and the oracle to account; tests/test_gpu_dec_synth.py holds the
kernels against the tables.
"""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

import decbitsmodel as DM
import tailmodel as TM

BLOCK_DT, HEADER_ONLY = DM.BLOCK_DT, DM.HEADER_ONLY
CANARY = np.uint32(DM.CANARY).view(np.int32)
GAP = 19                           # canary words behind every block
TAIL = 64                          # and more of them at the end of every plane
EMPTY_BODY = 48                    # live words at the smp_off of a skipped row whose num_samples is 0
KINT_UNREAD = 0x7FFFFFFF           # kint[.][0]: no stage reads it
KINDS = ("q15", "alt", "full")     # coefficient kinds of a lattice job

LMS_TABLES = ((4, 1), (8, 1), (16, 1), (32, 1), (4, 3), (8, 3), (4, 8))                       # (order, C)
LATTICE_ORDERS = (0, 1, 15, 16, 17, 32, 33, 64, 65, 128, 129, 255)
LATTICE_TABLES = tuple((o, d, 1) for o in LATTICE_ORDERS for d in (0, 1)) + (
    (15, 1, 3), (17, 0, 3), (33, 1, 3), (65, 0, 3), (129, 1, 3),                              # one order per specialisation
    (16, 1, 8))                                                                               # (order, deemphasis, C)
PIN_LENGTHS = (1, 17, 65, 300)     # lengths at which the lattice yardstick is pinned to the reference


def lattice_shape(order):
    """(G, R) of the k_dec_lattice specialisation the launcher picks for a PARCOR order"""
    if order <= 16:
        return 16, 1
    if order <= 32:
        return 32, 1
    if order <= 64:
        return 64, 1
    return (64, 2) if order <= 128 else (64, 4)


def lms_lengths(order):
    g = 2 * order
    return tuple(sorted({0, 1, order - 1, order, order + 1, g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1, 3 * g + order + 1, 777}))


def lattice_lengths(order):
    g = lattice_shape(order)[0]
    return tuple(sorted({0, 1, 15, 16, 17, g - 1, g, g + 1, 2 * g + 5, 300}))


def coefs(kind, order, seed=0):
    """a job's kint row [order + 1]: the coefficients of stages 1..order behind the word nothing reads"""
    rng = np.random.default_rng(zlib.crc32(("kint/%s/%d/%d" % (kind, order, seed)).encode()))
    if kind == "q15":
        k = rng.integers(-32768, 32768, order, dtype=np.int64)
    elif kind == "alt":
        k = np.where(np.arange(order) % 2 == 0, -32768, 32767).astype(np.int64)
    elif kind == "full":
        k = rng.integers(TM.INT32_MIN, TM.INT32_MAX + 1, order, dtype=np.int64)
    else:
        raise KeyError(kind)
    return np.concatenate([[KINT_UNREAD], k]).astype(np.int32)


@dataclass(frozen=True)
class Job:
    row: int
    ch: int
    n: int                         # the row's num_samples
    family: str
    kind: str                      # coefficient kind ("" in an LMS table)
    live: bool                     # a compressed row without HEADER_ONLY: the kernel synthesises it


@dataclass
class Table:
    name: str
    stage: str                     # "lms" or "lattice"
    order: int
    deemphasis: int
    C: int
    G: int                         # lanes per job
    jpw: int                       # jobs per wave
    blocks: np.ndarray             # BLOCK_DT [rows]
    info: np.ndarray               # uint32 [rows][4]
    kint: np.ndarray               # int32 [rows * C][order + 1] (lattice), None (LMS)
    body: np.ndarray               # int64 [rows]: live words behind smp_off (num_samples, EMPTY_BODY for a skipped empty row)
    planes: np.ndarray             # int32 [C][stride]: the input
    want: np.ndarray               # int32 [C][stride]: the expected output
    jobs: tuple                    # Job per j = row * C + ch

    @property
    def stride(self):
        return self.planes.shape[1]

    @property
    def waves(self):
        """the jobs of every wave of the launch, as the kernels split them"""
        return [self.jobs[w:w + self.jpw] for w in range(0, len(self.jobs), self.jpw)]

    @property
    def spans_blocks(self):
        """whether a wave can hold jobs of two blocks at all: not when the C channels of a block fill whole waves"""
        return self.jpw > 1 and self.C % self.jpw != 0

    def spanning_waves(self):
        """waves that hold jobs of two or more blocks: all of them for jpw > C, one in three for jpw 2 and C 3"""
        return sum(len({j.row for j in w}) >= 2 for w in self.waves)

    def mixed_waves(self):
        return sum(len({j.n for j in w}) >= 2 for w in self.waves)

    def waves_with_skipped_neighbour(self):
        return sum(any(j.live and j.n > 0 for j in w) and any(not j.live for j in w) for w in self.waves)

    def region(self, j):
        """(channel, first word, end) of job j's samples in the planes"""
        job = self.jobs[j]
        first = int(self.blocks["smp_off"][job.row])
        return job.ch, first, first + job.n


def job_count_ok(jobs, C, jpw):
    """the launch spans two workgroups and ends inside a workgroup and, where a wave holds several jobs and the channel
    count lets it, inside a wave (jobs is a multiple of C: with C a multiple of jpw every wave is full)"""
    per_wg = 4 * jpw
    if jobs <= per_wg or jobs % per_wg == 0:
        return False
    return jpw == 1 or C % jpw == 0 or jobs % jpw != 0


def _rows(lengths, C, jpw, with_kinds, fillers):
    """(n, type, flags, body, [(family, kind)] * C) per row: every length with every family (and, for the lattice, the
    kinds in rotation, shifted per length so that the pairing of family and kind changes), rows short of C jobs and
    the job count filled up from the same lists; then the rows a kernel must leave alone"""
    fams = TM.FAMILIES
    rows = []
    for li, n in enumerate(lengths):
        mine = [(f, KINDS[(fi + li) % 3] if with_kinds else "") for fi, f in enumerate(fams)]
        for i in range(0, len(mine), C):
            part = mine[i:i + C]
            part += [(fams[(li + k) % len(fams)], KINDS[(li + k) % 3] if with_kinds else "") for k in range(C - len(part))]
            rows.append((n, 0, 0, n, part))
    skipped = 5
    extra = 0
    while extra < fillers or not job_count_ok((len(rows) + skipped) * C, C, jpw):
        n = lengths[len(lengths) - 1 - extra % (len(lengths) // 2)]          # from the longer half of the list
        live_fams = ("full", "minmax", "24bit", "ramp", "alt", "allmax")
        part = [(live_fams[(extra + k) % len(live_fams)], KINDS[(extra + k) % 3] if with_kinds else "") for k in range(C)]
        rows.append((n, 0, 0, n, part))
        extra += 1
    g = 64 // jpw
    kinds = [KINDS[k % 3] if with_kinds else "" for k in range(C)]
    full = lambda shift: [("full", kinds[(k + shift) % C]) for k in range(C)]
    rows.append((2 * g + 39, 1, 0, 2 * g + 39, full(0)))                     # SILENT
    rows.append((g + 43, 2, 0, g + 43, full(1)))                             # RAW
    rows.append((3 * g + 41, 3, 0, 3 * g + 41, full(2)))                     # not a block type
    rows.append((300, 0, HEADER_ONLY, 300, full(0)))                         # compressed, header only
    rows.append((0, 0, 0, EMPTY_BODY, full(1)))                              # compressed, no samples: live words behind it
    return rows


def _build(name, stage, order, deemphasis, C, G, lengths, fillers):
    import slalibs
    O = slalibs.oracle()
    jpw = 64 // G
    rows = _rows(lengths, C, jpw, stage == "lattice", fillers)
    tag = zlib.crc32(name.encode())
    perm = np.random.default_rng(tag).permutation(len(rows))
    rows = [rows[i] for i in perm]

    nb = len(rows)
    blocks = np.zeros(nb, BLOCK_DT)
    info = np.zeros((nb, 4), np.uint32)
    kint = np.zeros((nb * C, order + 1), np.int32) if stage == "lattice" else None
    body = np.array([r[3] for r in rows], np.int64)
    stride = int((body + GAP).sum()) + TAIL
    planes = np.full((C, stride), CANARY, np.int32)
    want = planes.copy()
    jobs, pos = [], 0
    for r, (n, typ, flags, words, chans) in enumerate(rows):
        blocks[r] = (0, 0, pos, n, flags)
        info[r] = (typ, 0, 0, 0)
        live = typ == 0 and flags == 0
        for ch, (fam, kind) in enumerate(chans):
            j = r * C + ch
            x = TM.family(fam, words, seed=tag % 100000 + j)
            planes[ch, pos:pos + words] = x
            y = x
            if stage == "lattice":
                kint[j] = coefs(kind, order, seed=tag % 100000 + j)
            if live and n > 0:
                if stage == "lms":
                    y = O.lms_synth(x, order)
                else:
                    y = O.lattice_synth(x, kint[j])
                    y = O.deemph_i32(y) if deemphasis else y
            want[ch, pos:pos + words] = y
            jobs.append(Job(r, ch, n, fam, kind, live))
        pos += words + GAP
    assert pos + TAIL == stride
    for a in (blocks, info, body, planes, want) + ((kint,) if kint is not None else ()):
        a.setflags(write=False)
    return Table(name, stage, order, deemphasis, C, G, jpw, blocks, info, kint, body, planes, want, tuple(jobs))


def lms_name(order, C):
    return "lms_o%d_c%d" % (order, C)


def lattice_name(order, deemphasis, C):
    return "lat_o%d_d%d_c%d" % (order, deemphasis, C)


# Jobs added beyond the job-count rule, so that three quarters of a table's jobs with more samples than taps come out
# different from what went in.  Three kinds of LMS job come out as they went in when the kernel is right: n = order + 1
# (the first prediction is made with all-zero coefficients), `allmin` (the steps are +-16, and every product of an even
# coefficient with -2^31 wraps to 0) and, at these lengths, `small` (steps of 0 or 1 against histories of at most 2 do
# not carry a prediction past 2^9).  They stay in: a value that leaks in from the neighbouring group shows on them first.
LMS_FILLER_JOBS = 64


@functools.lru_cache(maxsize=None)
def lms_table(order, C):
    return _build(lms_name(order, C), "lms", order, 0, C, 2 * order, lms_lengths(order), -(-LMS_FILLER_JOBS // C))


@functools.lru_cache(maxsize=None)
def lattice_table(order, deemphasis, C):
    return _build(lattice_name(order, deemphasis, C), "lattice", order, deemphasis, C, lattice_shape(order)[0],
                  lattice_lengths(order), 0)


def explain(t, got):
    """where the first difference lies: the row, its length, the channel, the job's operands, the sample or gap word"""
    ch, pos = (int(v) for v in np.argwhere(got != t.want)[0])
    r = int(np.searchsorted(t.blocks["smp_off"], pos, side="right")) - 1
    b = t.blocks[r]
    at = pos - int(b["smp_off"])
    job = t.jobs[r * t.C + ch]
    if at < int(b["num_samples"]):
        where = "sample %d" % at
    elif at < int(t.body[r]):
        where = "word %d behind an empty row" % at
    else:
        where = "the gap behind it, word %d" % (at - int(t.body[r]))
    return (t.name, "row", r, "n", int(b["num_samples"]), "type", int(t.info[r, 0]), "flags", int(b["flags"]), "channel", ch,
            "job", r * t.C + ch, "wave", (r * t.C + ch) // t.jpw, "family", job.family, "kint", job.kind, where,
            "got", int(got[ch, pos]), "want", int(t.want[ch, pos]), "mismatches", int((got != t.want).sum()))


# ---- the two small kernels, in plain integers ------------------------------------------------------------------------

def deemphasis(x, previous, shift):
    """k_dec_deemphasis: y[i] = x[i] + (wrap32(y[i-1] * (2^shift - 1)) >> shift), y[-1] = previous"""
    numer = (1 << shift) - 1
    y = int(previous)
    out = []
    for v in np.asarray(x).tolist():
        y = TM.wrap32(v + (TM.wrap32(y * numer) >> shift))
        out.append(y)
    return np.array(out, np.int64).astype(np.int32)


def finish(planes, mid_side, shift):
    """k_dec_finish: planes 0 / 1 from mid / side to left / right (the side's low bit is the mid's lost one), then
    every channel shifted left with wrap"""
    p = [[int(v) for v in row] for row in np.asarray(planes).tolist()]
    if mid_side:
        left, right = [], []
        for p0, side in zip(p[0], p[1]):
            mid = TM.wrap32((p0 << 1) | (side & 1))
            left.append(TM.wrap32(mid + side) >> 1)
            right.append(TM.wrap32(mid - side) >> 1)
        p[0], p[1] = left, right
    return np.array([[TM.wrap32(v << shift) for v in row] for row in p], np.int64).astype(np.int32).reshape(np.asarray(planes).shape)
