"""The layout rule of sla_hip_splice_resident (include/sla_hip.h) in plain Python (test infrastructure).

An output stream is the concatenation of segments (source stream, sample range).  Every block that lies whole inside a
segment is copied byte for byte; of a block the cut passes through, the samples that remain are written as a RAW block
(slastream.block_bytes) -- or as a SILENT block where the source block was 11 bytes long, which only a SILENT block is.
The header is slastream.header_bytes with the counts of what was emitted.

The coded values of a RAW block are the decoder's planes before its last step: right-justified, mid/side still folded.
The model builds them from the writer's fields through the oracle's unit functions (LMS -> lattice -> de-emphasis, as
tests/test_crafted_streams.py does), holds their finished form against the oracle's decode of the source, and asserts that
every one fits its channel's field -- a block whose samples do not is one the splice refuses -- so the catalogue below keeps
its amplitudes a few bits under the field width.

Sources: crafted files of short blocks (1 to 300 samples, tests/slastream.py): COMPRESS, RAW and SILENT blocks in mono,
stereo with and without mid/side and 8 channels, 8 / 16 / 24 / 32 bits, offset_lshift 0 and 3; three files per format
for the joins.  `cases()` lists the cuts every test of the splice runs.

`check_code` and `check_verdicts` are the rule of the check kernel (sla_hip_launch_splice_check) as the header states it,
entry by entry, in unbounded integers: the yardstick of tests/test_gpu_splice_check.py, held against the judge's model, the
RAW writer and the oracle's decoder by tests/test_splice_check_model.py.
"""
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import crafted_catalogue as CC
from decbitsmodel import kint_of, unfold
import indexmodel as IM
import slalibs as S
import slastream as SS

OK, INVALID_ARGUMENT, CAPACITY, BUFFER, DATA, CORRUPT = 0, 2, 3, 4, 9, 11
VERBATIM, SILENT, RAW = 0, 1, 2

FORMATS = {
    "mono16":        SS.Format(1, 16, order=8, ntaps=1, lms=8, max_block=2048),
    "stereo8":       SS.Format(2, 8, order=4, ntaps=1, lms=4, max_block=2048),
    "stereo16ms":    SS.Format(2, 16, order=8, ntaps=3, lms=8, ms=1, max_block=2048),
    "stereo32ms":    SS.Format(2, 32, order=4, ntaps=1, lms=4, ms=1, max_block=2048),
    "eight24":       SS.Format(8, 24, order=8, ntaps=1, lms=8, max_block=2048),
    "stereo24l3":    SS.Format(2, 24, order=8, ntaps=1, lms=16, lshift=3, max_block=2048),
    "mono32l3":      SS.Format(1, 32, order=4, ntaps=1, lms=32, lshift=3, max_block=2048),
    "stereo16msl3":  SS.Format(2, 16, order=8, ntaps=1, lms=8, ms=1, lshift=3, max_block=2048),
}
LENGTHS = ([300, 7, 64, 1, 129, 1, 300, 255, 8, 200, 64], [17, 300, 3, 100, 250], [1, 1, 299, 64, 65, 30])
KINDS = (["c", "r", "s", "c", "c", "s", "r", "c", "c", "s", "c"], ["r", "c", "s", "c", "r"], ["c", "s", "c", "r", "c", "c"])


def _raw(rng, fmt, n):
    """RAW codes: the whole field, or -- under mid/side, where left and right must fit the field too -- two bits less"""
    widths = SS.raw_widths(fmt)
    return SS.Block(SS.RAW, n, raw=[rng.integers(0, 1 << (min(w, 32) - (2 if fmt.ms else 0)), n, dtype=np.uint64) for w in widths])


@functools.lru_cache(maxsize=None)
def sources():
    """{format name: (Case, Case, Case)}"""
    out = {}
    for k, (name, fmt) in enumerate(FORMATS.items()):
        rng = np.random.default_rng(7000 + k)
        amp = max(fmt.bits - fmt.lshift - 12, 1)
        files = []
        for lens, kinds in zip(LENGTHS, KINDS):
            blocks = []
            for n, kind in zip(lens, kinds):
                if kind == "c":
                    blocks.append(CC._comp(rng, fmt, n, bits=amp, full=False))
                elif kind == "r":
                    blocks.append(_raw(rng, fmt, n))
                else:
                    blocks.append(SS.Block(SS.SILENT, n))
            c = CC.Case("%s_%d" % (name, len(files)), fmt, blocks)
            c.data, c.stats, c.offsets = SS.write_file(fmt, blocks)
            files.append(c)
        out[name] = tuple(files)
    return out


_planes = {}


def pcm_of(case):
    """the oracle's decode of a source: left-justified int32 [C][N]"""
    rc, got, _ = S.oracle().decode_whole(S.make_params(cap=CC.CAP), case.data, case.num_samples)
    assert rc == 0 and got.shape[1] == case.num_samples
    return got


def planes_of(case):
    """[C][N] int64: the decoder's planes before mid/side is undone and the samples are left-justified"""
    if case.name not in _planes:
        f, oracle = case.fmt, S.oracle()
        v = np.zeros((f.num_channels, case.num_samples), np.int64)
        pos = 0
        for b in case.blocks:
            if b.type == SS.RAW:
                for ch in range(f.num_channels):
                    v[ch, pos:pos + b.n] = unfold(b.raw[ch])
            elif b.type == SS.COMPRESS:
                for ch, c in enumerate(b.chans):
                    assert c.ltm is None and not c.folded
                    x = oracle.lattice_synth(oracle.lms_synth(np.asarray(c.res, np.int32), f.lms), kint_of(c))
                    v[ch, pos:pos + b.n] = oracle.deemph_i32(x)
            pos += b.n
        for ch, w in enumerate(SS.raw_widths(f)):
            assert w >= 32 or int(SS.fold_array(v[ch]).max(initial=0)) < (1 << w), (case.name, ch)
        # the decoder's last step on these planes gives the oracle's decode
        side = v[1] if f.ms else None
        mid = ((v[0] << 1) | (side & 1)) if f.ms else None
        lr = np.stack([(mid + side) >> 1, (mid - side) >> 1]) if f.ms else v
        assert np.array_equal(((lr << (32 - f.bits + f.lshift)) & SS.M32).astype(np.uint32).view(np.int32), pcm_of(case)), case.name
        _planes[case.name] = v
    return _planes[case.name]


@dataclass
class Spliced:
    rc: int = OK
    data: bytes = b""
    num_samples: int = 0
    num_blocks: int = 0
    max_block_size: int = 0
    max_bit_per_second: int = 0
    verbatim_bytes: int = 0
    edge_blocks: int = 0
    blocks: list = field(default_factory=list)       # (kind, segment, source row, out_off, out_len, first kept sample, samples)


def same_format(a, b):
    return (a.num_channels, a.bits, a.rate, a.lshift, a.order, a.ntaps, a.lms, a.ms, a.max_block) == \
           (b.num_channels, b.bits, b.rate, b.lshift, b.order, b.ntaps, b.lms, b.ms, b.max_block)


def splice(segments):
    """segments: [(Case, start, length)] -> Spliced"""
    out = Spliced()
    if not segments or any(not same_format(c.fmt, segments[0][0].fmt) for c, _, _ in segments):
        return Spliced(rc=INVALID_ARGUMENT)
    fmt = segments[0][0].fmt
    W = sum(SS.raw_widths(fmt))
    body, pos = [], SS.HEADER_SIZE
    for s, (case, start, length) in enumerate(segments):
        if length == 0:
            continue
        x = IM.index_of(case.data)
        if start + length > x.extent:
            return Spliced(rc=x.stop if x.stop != OK else DATA)
        for row in x.rows:
            off, blen, p0, n0 = row
            a, b = max(p0, start), min(p0 + n0, start + length)
            if n0 == 0 or a >= b:
                continue
            if b - a == n0:
                kind, bb = VERBATIM, case.data[off:off + blen]
                out.verbatim_bytes += blen
            elif blen == 11:
                kind, bb = SILENT, SS.block_bytes(fmt, SS.Block(SS.SILENT, b - a))
            else:
                planes = planes_of(case)
                kind = RAW
                bb = SS.block_bytes(fmt, SS.Block(SS.RAW, b - a, raw=[SS.fold_array(planes[ch][a:b]) for ch in range(fmt.num_channels)]))
                assert len(bb) == 11 + ((b - a) * W + 7) // 8
            out.edge_blocks += kind != VERBATIM
            out.blocks.append((kind, s, row, pos, len(bb), a, b - a))
            out.max_block_size = max(out.max_block_size, len(bb))
            out.max_bit_per_second = max(out.max_bit_per_second, ((8 * len(bb) * fmt.rate) & SS.M32) // (b - a))
            body.append(bb)
            pos += len(bb)
        out.num_samples += length
    out.num_blocks = len(body)
    if pos > SS.M32 or out.num_samples > SS.M32:
        return Spliced(rc=CAPACITY)
    out.data = SS.header_bytes(fmt, out.num_samples, out.num_blocks, out.max_block_size, out.max_bit_per_second) + b"".join(body)
    return out


def expected_pcm(segments):
    """the concatenated source windows, left-justified [C][sum of lengths]"""
    return np.concatenate([pcm_of(c)[:, s:s + l] for c, s, l in segments], axis=1)


# ---- the check kernel's rule (sla_hip_launch_splice_check), from the contract text of include/sla_hip.h -------------------
NG, NO_EDGE = 1, 0xFFFFFFFF
ALL_ONES = (1 << 64) - 1


@dataclass
class CheckEntry:
    """sla_hip_splice_check.  src: the block's first byte as an offset into `memory`, None for a NULL pointer"""
    src: Optional[int]
    byte_len: int
    num_samples: int
    verdict: int = 0
    ordinal: int = 0
    edge: int = NO_EDGE
    plane_off: int = 0
    keep: int = 0


def fits(s, w):
    """whether the sample s can be stored in a RAW field of w bits: the field holds the two's complement range of w bits"""
    return -(1 << (w - 1)) <= s < (1 << (w - 1))


def check_code(entry, memory, planes, stride, C, width, ms, outcomes, crc_check, crc16=SS.crc16):
    """the code of one entry, 0 when it is clean.  memory: the bytes entry.src counts in; planes: [C][stride] integers;
    outcomes: the result codes the judge left, one per edge block; crc16: SS.crc16, or a faster routine held against it"""
    if entry.src is None or entry.byte_len < 11:
        return CORRUPT                                               # 1.
    is_edge = entry.edge != NO_EDGE
    if is_edge:                                                      # 2. the tables, then the judge's word
        if entry.edge >= len(outcomes) or entry.plane_off > stride or entry.keep > stride - entry.plane_off:
            return NG
        if outcomes[entry.edge] != 0:
            return int(outcomes[entry.edge])
    h = bytes(memory[entry.src:entry.src + 11])                      # 3. the chain header against the row, and the type
    typ = h[10] >> 6
    if h[0:2] != b"\xff\xff" or (int.from_bytes(h[2:6], "big") + 6) % (1 << 32) != entry.byte_len:
        return CORRUPT
    if int.from_bytes(h[8:10], "big") != entry.num_samples or (typ == 1) != (entry.byte_len == 11):
        return CORRUPT
    if not is_edge:                                                  # 4.
        if crc_check and crc16(bytes(memory[entry.src + 8:entry.src + entry.byte_len])) != int.from_bytes(h[6:8], "big"):
            return CORRUPT
        return 0
    if typ != 1:                                                     # 5. what k_splice_edges would have to store
        for c in range(C):
            w = width + (1 if (ms and c == 1) else 0)
            if w >= 32:
                continue
            for s in planes[c][entry.plane_off:entry.plane_off + entry.keep]:
                if not fits(int(s), w):
                    return CORRUPT
    return 0


def check_verdicts(entries, initial_words, num_verdicts, memory, planes, stride, C, width, ms, outcomes, crc_check, crc16=SS.crc16):
    """the verdict buffer after one launch over `entries`: every failing entry whose word exists lowers it"""
    words = [int(w) for w in initial_words]
    for e in entries:
        code = check_code(e, memory, planes, stride, C, width, ms, outcomes, crc_check, crc16)
        if code != 0 and e.verdict < num_verdicts:
            words[e.verdict] = min(words[e.verdict], (e.ordinal << 8) | (code & 0xFF))
    return words


@functools.lru_cache(maxsize=None)
def cases():
    """((name, ((Case, start, length), ...)), ...): the cuts and joins of every test of the splice"""
    out = []
    for name, (A, B, Cc) in sources().items():
        N = A.num_samples
        ends = np.cumsum([b.n for b in A.blocks]).tolist()
        b2, b7 = ends[1], ends[6]                       # block boundaries: behind the RAW block of 7, behind the RAW block of 300
        cuts = {
            "whole": [(A, 0, N)], "from_0_to_a_boundary": [(A, 0, b2)], "boundary_to_the_end": [(A, b2, N - b2)],
            "boundary_to_boundary": [(A, b2, b7 - b2)],
            "one_inside_at_both_ends": [(A, b2 + 1, b7 - b2 - 2)], "one_outside_at_both_ends": [(A, b2 - 1, b7 - b2 + 2)],
            "inside_one_compress_block": [(A, 10, 50)], "inside_one_raw_block": [(A, ends[5] + 3, 100)],
            "inside_one_silent_block": [(A, ends[1] + 5, 20)], "one_sample": [(A, 299, 1)], "the_last_sample": [(A, N - 1, 1)],
            "from_0_inside_a_block": [(A, 0, 10)], "to_the_end_from_inside": [(A, N - 70, 70)], "nothing": [(A, 40, 0)],
            "join_two": [(A, 0, N), (B, 0, B.num_samples)],
            "join_three_with_cuts": [(A, 5, ends[0]), (B, 0, B.num_samples), (Cc, 1, Cc.num_samples - 2)],
            "join_with_an_empty_segment": [(B, 17, 300), (A, 3, 0), (Cc, 0, 2)],
            "the_same_block_twice": [(A, 20, 30), (A, 50, 30)],
        }
        out += [("%s-%s" % (name, k), tuple(v)) for k, v in cuts.items()]
    return tuple(out)
