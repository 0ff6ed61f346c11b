"""The files and row plans of the k_dec_bits tests with several blocks per wave (test infrastructure, no device).

Per format one menu of blocks -- compressed blocks around the 64-sample tile edge, a far-path block whose every
sample costs more than 64 bits, a gamma-boundary block, Golomb blocks with a power-of-two modulus and without, int32's
extremes, RAW, SILENT, one long block -- written with tests/slastream.py into three files (and into one, for the launch
without per-row ends), and the row plans that replicate those few blocks into launches of 1025 to 64513 rows.
tests/test_dec_bits_model.py checks the files and the model (CPU), tests/test_gpu_dec_bits_lanes.py runs the launches.
"""
import functools
from dataclasses import dataclass

import numpy as np

import crafted_catalogue as CC
import decbitsmodel as DM
import slastream as SS

FORMATS = {
    1: SS.Format(1, 16, order=4, ntaps=1, lms=4),
    2: SS.Format(2, 32, order=8, ntaps=3, lms=8, ms=1),       # 33-bit RAW side fields, `init << 8` wraps
    3: SS.Format(3, 24, order=16, ntaps=5, lms=16),
    8: SS.Format(8, 24, order=16, ntaps=5, lms=16),
}
CAPS = {1: 64, 2: 32, 3: 21, 8: 8}                           # 64 // C: the most blocks a wave takes

# which file holds which block; the one-file image holds them all in this order
FILES = (("c1", "raw70", "c63", "silent1", "golomb_pow2", "long"),
         ("c64", "far", "silent300", "gamma", "c65"),
         ("golomb_other", "extremes", "c129", "wide_init"))
ONE_SAMPLE = ("c1", "silent1")
LONG_ROWS = ("long", "far")


def _menu(fmt):
    C = fmt.num_channels
    rng = np.random.default_rng(7000 + C)
    taps = [int(t) for t in rng.integers(-32768, 32768, fmt.ntaps)]
    m = {}
    for n in (1, 63, 64, 65, 129):
        m["c%d" % n] = CC._comp(rng, fmt, n, bits=10, rshift=n % 16, ltm=(40 + n, taps) if n & 1 else None)
    m["long"] = CC._comp(rng, fmt, 2000, bits=12, full=False)
    # every code k * 2^24 + m0 (crafted_catalogue: rice_over_64_bits_per_sample): both parameters stay where they are
    # and every sample costs a gamma escape of about 2 x 32 bits, far beyond the reader's 128-word window
    chans = []
    for _ in range(C):
        ks = rng.integers(1, 256, 200)
        codes = CC.adaptive_codes(9, 200, lambda i, m0, m1: (int(ks[i]) << 24) + m0)
        chans.append(SS.Chan(0, CC._codes(rng, fmt.order, False), None, 9, codes, folded=True))
    m["far"] = SS.Block(SS.COMPRESS, 200, chans)
    qs = [15, 16, 17, 1, 2, 16, 0, 17, 15, 300, 16]
    chans = []
    for c in range(C):
        codes = CC.adaptive_codes(5000, 66, lambda i, m0, m1: (m0 + m1 * (qs[(i + c) % len(qs)] - 1) + (i * 7919) % m1)
                                  if qs[(i + c) % len(qs)] else (i % m0))
        chans.append(SS.Chan(0, CC._codes(rng, fmt.order, False), None, 5000, codes, folded=True))
    m["gamma"] = SS.Block(SS.COMPRESS, 66, chans)
    m["golomb_pow2"] = SS.Block(SS.COMPRESS, 65, [CC._chan(rng, fmt, 65, res=rng.integers(-16, 16, 65).astype(np.int32), init=4,
                                                           full=False) for _ in range(C)])
    # a modulus that is no power of two; in the 32-bit format written as 2^24 + 5, which `init << 8` wraps to 5
    other = (1 << 24) + 5 if fmt.bits == 32 else 5
    m["golomb_other"] = SS.Block(SS.COMPRESS, 67, [CC._chan(rng, fmt, 67, res=rng.integers(-20, 20, 67).astype(np.int32),
                                                            init=other if c == 0 else 7, full=False) for c in range(C)])
    ext = np.array([-(1 << 31), (1 << 31) - 1, -1, 0, 1] * 13, np.int32)
    m["extremes"] = SS.Block(SS.COMPRESS, 65, [CC._chan(rng, fmt, 65, res=np.roll(ext, c), init=min(1 << 20, (1 << fmt.bits) - 1),
                                                        full=False) for c in range(C)])
    # the largest initial parameter the format can write (2^32 - 1 wraps to 0xFFFFFF00 in the 32-bit format)
    m["wide_init"] = SS.Block(SS.COMPRESS, 33, [CC._chan(rng, fmt, 33, bits=31, init=(1 << fmt.bits) - 1 if c == 0 else 1 << 12)
                                                for c in range(C)])
    m["raw70"] = CC._raw(rng, fmt, 70)
    m["silent1"] = SS.Block(SS.SILENT, 1)
    m["silent300"] = SS.Block(SS.SILENT, 300)
    return m


def _case(name, fmt, blocks):
    c = CC.Case(name, fmt, blocks)
    c.data, c.stats, c.offsets = SS.write_file(fmt, blocks)
    return c


@dataclass
class Suite:
    """the files of one format: three of them in one image, and all blocks in one file"""
    fmt: SS.Format
    menu: dict
    split: DM.Model
    single: DM.Model
    where: dict                   # (model, block name) -> item index


@functools.lru_cache(maxsize=None)
def suite(C):
    fmt = FORMATS[C]
    menu = _menu(fmt)
    split = DM.Model([_case("dec_bits_c%d_file%d" % (C, f), fmt, [menu[k] for k in names]) for f, names in enumerate(FILES)])
    names = [k for names in FILES for k in names]
    single = DM.Model([_case("dec_bits_c%d_one_file" % C, fmt, [menu[k] for k in names])])
    where = {}
    for f, fnames in enumerate(FILES):
        for b, k in enumerate(fnames):
            where[("split", k)] = split.index[(f, b)]
    for b, k in enumerate(names):
        where[("single", k)] = single.index[(0, b)]
    return Suite(fmt, menu, split, single, where)


# ---- row plans -------------------------------------------------------------------------------------------------

# (block, HEADER_ONLY, weight of the seeded draw): most rows stay at or below 65 samples, the long ones are rare
ROW_KINDS = (("c1", 0, 6.0), ("silent1", 0, 3.0), ("c63", 0, 1.0), ("c64", 0, 1.0), ("c65", 0, 1.0), ("c129", 0, 0.5),
             ("gamma", 0, 1.0), ("golomb_pow2", 0, 1.0), ("golomb_other", 0, 1.0), ("extremes", 0, 1.0), ("wide_init", 0, 1.0),
             ("raw70", 0, 1.0), ("silent300", 0, 0.2), ("far", 0, 0.15), ("long", 0, 0.02),
             ("c129", 1, 1.0), ("long", 1, 0.5))
# neighbours of five kinds: RAW, SILENT, Golomb, adaptive, HEADER_ONLY -- then one-sample rows and another Golomb
ADJACENT = (("raw70", 0), ("silent1", 0), ("golomb_other", 0), ("gamma", 0), ("c63", 1), ("c1", 0), ("golomb_pow2", 0),
            ("c65", 0), ("silent1", 0), ("c1", 0), ("extremes", 0))


@dataclass
class Plan:
    name: tuple                   # kind of each row: (block name, flags)
    gap: np.ndarray


def plan(kind, rows, lanes, seed):
    """the rows of one launch, as (block name, flags) and a gap each"""
    rng = np.random.default_rng(seed)
    if kind == "shuffle":
        w = np.array([k[2] for k in ROW_KINDS])
        pick = np.concatenate([np.arange(len(ROW_KINDS)), rng.choice(len(ROW_KINDS), rows - len(ROW_KINDS), p=w / w.sum())])
        rng.shuffle(pick)
        names = [ROW_KINDS[i][:2] for i in pick]
    elif kind == "dominated":
        # one-sample rows; in every fifth wave one lane holds the long block or the far-path block and decides alone
        # how many tiles the whole wave walks
        names = [(ONE_SAMPLE[r % 2], 0) for r in range(rows)]
        for w in range(0, rows // lanes, 5):
            names[w * lanes + (w // 5) % lanes] = (LONG_ROWS[(w // 5) % 2], 0)
    elif kind == "adjacent":
        # the pattern's length is coprime to every lane count in use, so it meets the waves at every alignment
        assert np.gcd(len(ADJACENT), lanes) == 1
        names = [ADJACENT[r % len(ADJACENT)] for r in range(rows)]
        for r in range(len(ADJACENT) * 40, rows - 8, len(ADJACENT) * 97):
            names[r + 5] = ("far", 0)
            names[r + 7] = ("long", 0)
    else:
        raise ValueError(kind)
    return Plan(tuple(names), rng.choice(DM.GAPS, rows))


@dataclass
class LaunchCase:
    id: str
    C: int
    lanes: int
    rows: int
    kind: str
    image: str                    # "split": three files, per-row ends; "single": one file, no ends
    cut: bool = False


def launch_cases():
    out = []
    for C in FORMATS:
        for L, kind in ((2, "shuffle"), (3, "dominated"), (CAPS[C], "adjacent")):
            out.append(LaunchCase("c%d_lanes%d_%s" % (C, L, kind), C, L, 1024 * (L - 1) + 1, kind, "split"))
        out.append(LaunchCase("c%d_lanes2_full_waves_cut" % C, C, 2, 2048, "shuffle", "split", cut=True))
        out.append(LaunchCase("c%d_lanes2_no_ends" % C, C, 2, 1025, "shuffle", "single"))
    return out


CUT_BLOCK = "long"                # the last block of file 0: its rows' stream ends in the middle of its body


def build(case):
    """(Suite, Model, Plan, decbitsmodel.Launch) of a LaunchCase"""
    s = suite(case.C)
    model = s.split if case.image == "split" else s.single
    p = plan(case.kind, case.rows, case.lanes, seed=case.C * 1000 + case.rows)
    item = np.array([s.where[(case.image, k)] for k, _ in p.name])
    flags = np.array([f for _, f in p.name], np.uint32)
    cut = None
    if case.cut:
        it = model.items[s.where[(case.image, CUT_BLOCK)]]
        assert it.byte_off + it.byte_len == it.end                    # the file's last block
        cut = {it.file: it.byte_off - model.file_off[it.file] + it.head + (it.byte_len - it.head) // 2}
        flags[[k == CUT_BLOCK for k, _ in p.name]] = 0                # a HEADER_ONLY row reads no body: nothing to cut
    return s, model, p, model.launch(item, p.gap, flags, cut)
