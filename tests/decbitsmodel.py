"""What one launch of the entropy-decode kernel (k_dec_bits, sla_hip_launch_dec_bits_x) needs and must deliver, from
the writer's fields alone (test infrastructure, plain Python / numpy, no device).

A `Model` takes crafted files of one format (crafted_catalogue.Case: data, offsets, blocks, fmt), lays them out in one
image the way the host does -- every file at a 4-byte aligned offset, the gaps zero -- and knows of every block what
the kernel has to say about it: type, used_bytes, the sla_hip_dec_chan words, the kint rows and the samples (unfolded
residuals, unfolded RAW codes, or zeros).  None of that is decoded from the bytes: it is the list of fields the stream
was written from.  `Model.launch` turns a row plan -- (file, block) pairs in any order and any number of times, each
with a gap of canary words behind its samples and optionally SLA_HIP_DEC_HEADER_ONLY -- into the sla_hip_dec_block
table, the per-row file ends of the bounded launch and the expected outputs, replicated per row with numpy.

tests/test_dec_bits_model.py holds the model against the oracle; tests/test_gpu_dec_bits_lanes.py holds the kernel
against the model.
"""
from dataclasses import dataclass

import numpy as np

import slastream as SS

BLOCK_DT = np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"), ("num_samples", "<u4"), ("flags", "<u4")])
HEADER_ONLY = 1                   # SLA_HIP_DEC_HEADER_ONLY
CANARY = 0x5A5A5A5A
CHAN_WORDS = 8                    # sla_hip_dec_chan: pitch, ltm_coef[5], rice_init, reserved
GAPS = (0, 1, 3)
TAIL = 64                         # canary words behind the last row's samples


def unfold(codes):
    u = np.asarray(codes, np.uint64) & np.uint64(SS.M32)
    return ((u >> np.uint64(1)).astype(np.int64) ^ -(u & np.uint64(1)).astype(np.int64)).astype(np.int32)


def kint_of(chan):
    k = [0]
    for o, c in enumerate(chan.codes, start=1):
        q = 16 if o < 4 else 8
        v = SS.fold(c) & ((1 << q) - 1)
        s = (v >> 1) ^ -(v & 1)                                   # the code as read back from its q-bit field
        w = (s << (16 - q)) & SS.M32
        w = w - (1 << 32) if w >> 31 else w
        k.append(w >> chan.rshift)
    return np.array(k, np.int32)


def header_bits(fmt, blk):
    """bits from the sync code to the end of the block's parameters (the body starts at the next byte)"""
    bits = 16 + 32 + 16 + 16 + 2
    if blk.type == SS.COMPRESS:
        for ch in blk.chans:
            bits += 4 + sum(16 if o < 4 else 8 for o in range(1, fmt.order + 1)) + 1
            if ch.ltm is not None:
                bits += SS.LTM_PERIOD_BITS + 16 * fmt.ntaps
            bits += fmt.bits
    return bits


def header_bytes(fmt, blk):
    return (header_bits(fmt, blk) + 7) // 8


def chan_words(fmt, blk):
    """the sla_hip_dec_chan rows [C][8] of a compressed block: pitch, taps as `code << 16`, the initial parameter"""
    _, inits = SS.block_codes(fmt, blk)
    out = np.zeros((fmt.num_channels, CHAN_WORDS), np.uint32)
    for c, (ch, init) in enumerate(zip(blk.chans, inits)):
        if ch.ltm is not None:
            out[c, 0] = ch.ltm[0]
            for k, t in enumerate(ch.ltm[1][:5]):
                v = SS.fold(t) & 0xFFFF
                out[c, 1 + k] = (((v >> 1) ^ -(v & 1)) << 16) & SS.M32
        out[c, 6] = init & SS.M32
    return out


def block_samples(fmt, blk):
    """[C][n] int32: what the kernel leaves in the planes"""
    out = np.zeros((fmt.num_channels, blk.n), np.int32)
    if blk.type == SS.RAW:
        for c in range(fmt.num_channels):
            out[c] = unfold(blk.raw[c])
    elif blk.type == SS.COMPRESS:
        for c, ch in enumerate(blk.chans):
            out[c] = unfold(ch.res) if ch.folded else np.asarray(ch.res, np.int32)
    return out


def residual_stream(fmt, blk, block_data):
    """a compressed block's body in the form oracle.decode_residual reads: the initial parameters, aligned, the body"""
    _, inits = SS.block_codes(fmt, blk)
    w = SS.BitWriter()
    for i in inits:
        w.put(i, fmt.bits)
    w.align()
    return w.tobytes() + bytes(block_data[header_bytes(fmt, blk):])


@dataclass
class Item:
    """one block of one file, as the image holds it"""
    file: int
    block: int
    type: int
    n: int
    byte_off: int                 # in the image
    byte_len: int
    head: int                     # header_bytes
    end: int                      # byte end of its file in the image
    src: int                      # first sample in Model.pool


@dataclass
class Launch:
    blocks: np.ndarray            # BLOCK_DT [rows]
    ends: np.ndarray              # uint64 [rows]: the reader's end of stream (its file's end, or the cut)
    item: np.ndarray              # index into Model.items, per row
    stride: int
    info: np.ndarray              # uint32 [rows][4]: type, used_bytes, (crc: not the model's), overrun
    chan: np.ndarray              # uint32 [rows][C][8]
    kint: np.ndarray              # int32 [rows][C][order + 1]
    planes: np.ndarray            # int32 [C][stride], the canary where nothing may be written
    compressed: np.ndarray        # bool [rows]: chan / kint are compared
    cut: np.ndarray               # bool [rows]: the row's stream ends inside its body
    free: np.ndarray              # bool [stride]: sample positions a cut row may fill with anything


class Model:
    def __init__(self, cases):
        self.cases = list(cases)
        self.fmt = self.cases[0].fmt
        assert all(c.fmt == self.fmt for c in self.cases)
        C, order = self.fmt.num_channels, self.fmt.order
        parts, pos = [], 0
        self.file_off, self.file_end, self.items, self.index = [], [], [], {}
        pool, chans, kints, src = [], [], [], 0
        for f, case in enumerate(self.cases):
            pad = (-pos) % 4
            parts.append(bytes(pad))
            pos += pad
            self.file_off.append(pos)
            self.file_end.append(pos + len(case.data))
            offs = list(case.offsets) + [len(case.data)]
            for b, blk in enumerate(case.blocks):
                self.index[(f, b)] = len(self.items)
                self.items.append(Item(f, b, blk.type, blk.n, pos + offs[b], offs[b + 1] - offs[b],
                                       header_bytes(self.fmt, blk), pos + len(case.data), src))
                pool.append(block_samples(self.fmt, blk))
                src += blk.n
                if blk.type == SS.COMPRESS:
                    chans.append(chan_words(self.fmt, blk))
                    kints.append(np.stack([kint_of(ch) for ch in blk.chans]))
                else:
                    chans.append(np.zeros((C, CHAN_WORDS), np.uint32))
                    kints.append(np.zeros((C, order + 1), np.int32))
            parts.append(case.data)
            pos += len(case.data)
        parts.append(bytes((-pos) % 4))
        self.image = np.frombuffer(b"".join(parts), np.uint8)
        self.image_bytes = pos                                  # the last file's end: the unbounded launch's end of stream
        self.pool = np.concatenate(pool, axis=1)                # [C][samples of every block]
        self.chan = np.stack(chans)                             # [items][C][8]
        self.kint = np.stack(kints)                             # [items][C][order + 1]

    def launch(self, item, gap, flags, cut=None):
        """item / gap / flags: one entry per row (index into self.items, canary words behind the row's samples,
        sla_hip_dec_block.flags).  cut: {file: byte end inside the file}, the end its rows are given instead of the
        file's own; it has to lie inside the body of the one block of that file that reaches it."""
        it = self.items
        item, gap, flags = np.asarray(item, np.int64), np.asarray(gap, np.int64), np.asarray(flags, np.uint32)
        rows = len(item)
        assert set(np.unique(gap)) <= set(GAPS)
        col = lambda name: np.array([getattr(x, name) for x in it], np.int64)
        n, off, blen, typ, head, end, file = (col(k)[item] for k in ("n", "byte_off", "byte_len", "type", "head", "end", "file"))
        is_cut = np.zeros(rows, bool)
        for f, stop in (cut or {}).items():
            stop += self.file_off[f]
            mine = file == f
            assert not (mine & (off >= stop)).any(), "a row's block starts behind the cut"
            hit = mine & (off + blen > stop)
            assert (off[hit] + head[hit] < stop).all(), "the cut must lie inside the body"
            end = np.where(mine, stop, end)
            blen = np.where(hit, stop - off, blen)
            is_cut |= hit
        honly = (flags & HEADER_ONLY) != 0
        assert not (is_cut & honly).any()
        smp_off = np.cumsum(n + gap) - (n + gap)
        stride = int((n + gap).sum()) + TAIL
        assert stride < 1 << 32
        blocks = np.zeros(rows, BLOCK_DT)
        blocks["byte_off"], blocks["byte_len"], blocks["smp_off"], blocks["num_samples"], blocks["flags"] = off, blen, smp_off, n, flags
        info = np.zeros((rows, 4), np.uint32)
        info[:, 0] = typ
        info[:, 1] = np.where(honly, head, col("byte_len")[item])
        info[:, 3] = is_cut
        # the samples of every row that decodes them, replicated from the pool
        wn = np.where(honly | is_cut, 0, n)
        rep = np.repeat(np.arange(rows), wn)
        within = np.arange(int(wn.sum())) - np.repeat(np.cumsum(wn) - wn, wn)
        planes = np.full((self.fmt.num_channels, stride), CANARY, np.uint32).view(np.int32)
        planes[:, smp_off[rep] + within] = self.pool[:, col("src")[item][rep] + within]
        free = np.zeros(stride, bool)
        for r in np.flatnonzero(is_cut):
            free[smp_off[r]:smp_off[r] + n[r]] = True
        return Launch(blocks, end.astype(np.uint64), item, stride, info, self.chan[item], self.kint[item], planes,
                      typ == SS.COMPRESS, is_cut, free)

    def ranges(self, launch):
        """(first, end) of every row's sample range and of the gap behind it, in row order"""
        b = launch.blocks
        first = b["smp_off"].astype(np.int64)
        last = first + b["num_samples"]
        nxt = np.concatenate([first[1:], [launch.stride - TAIL]])
        return first, last, nxt
