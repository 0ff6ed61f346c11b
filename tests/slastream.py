"""An independent .sla stream writer (test infrastructure, plain Python / numpy).

The oracle's encoder (oracle/sla_oracle.c) only writes the field values its own analysis chooses.  This writer takes
every field explicitly -- per block its type and length; per channel of a compressed block the PARCOR shift and codes,
the long-term flag, pitch and taps, the initial Rice parameter and the residuals; per sample of a RAW block the coded
values -- and lays them out exactly as the format does (reference src/SLAEncoder.c:243-289 and :682-778, restated
in oracle/sla_oracle.c:1071-1097 and :1124-1245; the residual body after src/SLACoder.c, oracle/sla_oracle.c:843-960).
Nothing in it calls the oracle, so a stream it writes is a second opinion on the layout.

Besides the bytes it returns what each stream reaches in a decoder (`Stats`): the coder branch of every compressed
block, the Golomb moduli, the gamma escapes, the largest quotient, and the bits every 64-sample tile of every channel
costs, so that tests can assert the coverage they claim, and the body bits of every channel of every compressed block
(what the encoder's code-length pass must count).
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

HEADER_SIZE = 43
SYNC = 0xFFFF
LTM_PERIOD_BITS = 10
RICE_LOW_THRESHOLD = 8
QUOT_THRESHOLD = 16
TILE = 64
COMPRESS, SILENT, RAW = 0, 1, 2
M32 = 0xFFFFFFFF


def fold(v):
    """zig-zag fold of a signed 32-bit value (reference SLAUtility.h:37): s < 0 -> -2s-1, else 2s, modulo 2^32"""
    v = int(v) & M32
    u = (v << 1) & M32
    return (~u & M32) if (v >> 31) else u


def fold_array(a):
    a = np.asarray(a, np.int64) & M32
    u = (a << 1) & M32
    return np.where(a >> 31, ~u & M32, u).astype(np.uint64)


def crc16(data):
    """CRC16-IBM, reflected 0xA001, initial value 0 (reference src/SLAUtility.c:37-71)"""
    crc = 0
    for b in bytes(data):
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0xA001 if crc & 1 else crc >> 1
    return crc


def log2ceil(x):
    """ceil(log2(x)) for x >= 1, and 32 for x = 0 (the reference's 32 - nlz(x - 1) on uint32)"""
    return ((x - 1) & M32).bit_length()


def pow2ceil(x):
    return 1 << log2ceil(x)


class BitWriter:
    """MSB-first fields, collected as (value, width) and packed at the end with numpy"""

    def __init__(self):
        self.vals, self.widths, self.nbits = [], [], 0

    def put(self, val, nbits):
        if nbits <= 0:
            return
        self.vals.append(int(val) & ((1 << nbits) - 1) if nbits <= 64 else 0)
        self.widths.append(nbits)
        self.nbits += nbits

    def zeros(self, count):
        self.put(0, count)

    def align(self):
        if self.nbits & 7:
            self.put(0, 8 - (self.nbits & 7))

    def tobytes(self):
        if not self.widths:
            return b""
        w = np.array(self.widths, np.int64)
        v = np.array(self.vals, np.uint64)
        idx = np.repeat(np.arange(len(w)), w)
        start = np.cumsum(w) - w
        k = np.arange(self.nbits, dtype=np.int64) - start[idx]
        sh = np.minimum(w[idx] - 1 - k, 63).astype(np.uint64)
        bits = ((v[idx] >> sh) & np.uint64(1)).astype(np.uint8)
        return np.packbits(bits).tobytes()


# ---- the entropy coder (recursive Rice with 2 adaptive parameters; Golomb below the threshold) --------------------

def _rp_set(v):
    return (int(v) << 8) & M32                      # SLACODER_PARAMETER_SET in 32-bit arithmetic


def _rp_get(f):
    return max(((f + 128) >> 8) & M32, 1)


def _rp_rice(f):
    return pow2ceil(max((((f >> 1) + 128) >> 8) & M32, 1)) & M32


def _rp_update(f, code):
    return (119 * f + ((9 * ((code << 8) & M32)) & M32) + 64) >> 7


@dataclass
class Stats:
    """what a stream reaches in a decoder (filled by the writer)"""
    coder: List[str] = field(default_factory=list)              # per compressed block: "golomb" / "rice"
    golomb_m: List[List[int]] = field(default_factory=list)     # per Golomb block: the modulus of every channel
    gamma_escapes: int = 0
    max_quotient: int = 0
    quotients: set = field(default_factory=set)                  # unary quotients of the recursive-Rice tail
    max_tile_bits_per_sample: float = 0.0    # over every 64-sample tile of every block: its bits / (samples x channels)
    raw_widths: set = field(default_factory=set)
    max_init: int = 0
    chan_bits: List[List[int]] = field(default_factory=list)    # per compressed block: the body bits of every channel

    def merge(self, o):
        self.coder += o.coder
        self.golomb_m += o.golomb_m
        self.gamma_escapes += o.gamma_escapes
        self.max_quotient = max(self.max_quotient, o.max_quotient)
        self.quotients |= o.quotients
        self.max_tile_bits_per_sample = max(self.max_tile_bits_per_sample, o.max_tile_bits_per_sample)
        self.raw_widths |= o.raw_widths
        self.max_init = max(self.max_init, o.max_init)
        self.chan_bits += o.chan_bits


def _unary(w, q):
    w.zeros(q)
    w.put(1, 1)


def _golomb(w, m, val):
    quot, rest = val // m, val % m
    assert quot < (1 << 20), "a Golomb quotient this long makes a stream of megabytes"
    _unary(w, quot)
    if m & (m - 1) == 0:
        if m > 1:
            w.put(rest, log2ceil(m))
    else:
        b = log2ceil(m)
        cut = (1 << b) - m
        if rest < cut:
            w.put(rest, b - 1)
        else:
            w.put(rest + cut, b)
    return quot


def _gamma(w, val):
    if val == 0:
        w.put(1, 1)
        return
    nd = log2ceil(val + 2)
    w.zeros(nd - 1)
    w.put(val + 1, nd)


def _rrice(w, prm, val, st):
    m0 = _rp_rice(prm[0])
    if val < m0:
        _unary(w, 0)
        if m0 != 1:
            w.put(val & (m0 - 1), log2ceil(m0))
        prm[0] = _rp_update(prm[0], val)
        return
    prm[0] = _rp_update(prm[0], val)
    v = val - m0
    m = _rp_rice(prm[1])
    q = 1 + v // m
    st.quotients.add(min(q, 1 << 20))
    st.max_quotient = max(st.max_quotient, q)
    if q < QUOT_THRESHOLD:
        _unary(w, q)
    else:
        _unary(w, QUOT_THRESHOLD)
        _gamma(w, q - QUOT_THRESHOLD)
        st.gamma_escapes += 1
    if m != 1:
        w.put(v & (m - 1), log2ceil(m))
    prm[1] = _rp_update(prm[1], v)


def put_residuals(w, codes, inits, st=None):
    """the channel-interleaved body (reference src/SLACoder.c:429-467).  codes: [C][n] folded residuals (uint32),
    inits: the initial parameter of every channel as it stands in the stream"""
    st = st if st is not None else Stats()
    C = len(codes)
    n = len(codes[0]) if C else 0
    firsts = [_rp_set(i) for i in inits]
    avg = sum(_rp_get(f) for f in firsts) // C
    rice = avg > RICE_LOW_THRESHOLD
    st.coder.append("rice" if rice else "golomb")
    if not rice:
        st.golomb_m.append([_rp_get(f) for f in firsts])
    prm = [[f, f] for f in firsts]
    cols = [[int(x) for x in c] for c in codes]
    tile_bits = [0] * C
    total_bits = [0] * C
    st.chan_bits.append(total_bits)
    for s in range(n):
        for ch in range(C):
            before = w.nbits
            if rice:
                _rrice(w, prm[ch], cols[ch][s], st)
            else:
                _golomb(w, _rp_get(firsts[ch]), cols[ch][s])
            tile_bits[ch] += w.nbits - before
            total_bits[ch] += w.nbits - before
        if (s + 1) % TILE == 0 or s == n - 1:
            cnt = (s % TILE) + 1
            st.max_tile_bits_per_sample = max(st.max_tile_bits_per_sample, sum(tile_bits) / (cnt * C))
            tile_bits = [0] * C
    return st


# ---- blocks and files ------------------------------------------------------------------------------------------

@dataclass
class Chan:
    """one channel of a compressed block.  codes: PARCOR codes of orders 1..order (signed, 16-bit for orders 1-3,
    8-bit above; only their low bits reach the stream); ltm: None, or (pitch, [taps]) with signed 16-bit taps, one per
    long-term tap of the file header; init: the initial Rice parameter as written (its low `bps` bits; None: the mean
    of the folded residuals, as an encoder writes it); res: residuals
    (int32 values, or folded uint32 codes when `folded`)"""
    rshift: int
    codes: list
    ltm: Optional[tuple]
    init: Optional[int]
    res: np.ndarray
    folded: bool = False


@dataclass
class Block:
    type: int
    n: int
    chans: Optional[List[Chan]] = None       # COMPRESS
    raw: Optional[np.ndarray] = None         # RAW: [C][n] coded values (already folded, < 2^width)


def natural_init(codes):
    """the initial parameter an encoder would write for these folded residuals (mean, at least 1, src/SLACoder.c:361-385)"""
    return max(int(np.sum(np.asarray(codes, np.uint64), dtype=np.uint64)) // max(len(codes), 1), 1)


@dataclass
class Format:
    num_channels: int = 1
    bits: int = 16
    rate: int = 48000
    lshift: int = 0
    order: int = 8
    ntaps: int = 1
    lms: int = 8
    ms: int = 0
    window: int = 1
    max_block: int = 4096


def header_bytes(fmt, num_samples, num_blocks, max_block_size=0, max_bps=0):
    """43-byte big-endian file header with its CRC (reference src/SLAEncoder.c:243-289)"""
    d = bytearray(HEADER_SIZE)
    d[0:4] = b"SL*\x01"
    d[4:8] = (HEADER_SIZE - 8).to_bytes(4, "big")
    d[10:14] = (1).to_bytes(4, "big")
    d[14] = fmt.num_channels
    d[15:19] = int(num_samples).to_bytes(4, "big")
    d[19:23] = int(fmt.rate).to_bytes(4, "big")
    d[23], d[24], d[25], d[26], d[27], d[28] = fmt.bits, fmt.lshift, fmt.order, fmt.ntaps, fmt.lms, fmt.ms
    d[29:33] = int(num_blocks).to_bytes(4, "big")
    d[33:35] = int(fmt.max_block).to_bytes(2, "big")
    d[35:39] = int(max_block_size).to_bytes(4, "big")
    d[39:43] = int(max_bps).to_bytes(4, "big")
    d[8:10] = crc16(d[10:]).to_bytes(2, "big")
    return bytes(d)


def raw_widths(fmt):
    return [fmt.bits - fmt.lshift + (1 if (ch == 1 and fmt.ms == 1) else 0) for ch in range(fmt.num_channels)]


def block_codes(fmt, blk):
    """a compressed block's folded residuals [C][n] and the initial parameter of every channel as the stream holds it"""
    codes = [np.asarray(c.res, np.uint64) if c.folded else fold_array(c.res) for c in blk.chans]
    inits = [(natural_init(k) if c.init is None else int(c.init)) & ((1 << fmt.bits) - 1)
             for c, k in zip(blk.chans, codes)]
    return codes, inits


def block_bytes(fmt, blk, st=None):
    """one block: sync, size, CRC16, samples, type, parameters, body, each part byte-aligned as the format has it"""
    st = st if st is not None else Stats()
    codes, inits = [], []
    if blk.type == COMPRESS:
        codes, inits = block_codes(fmt, blk)
    w = BitWriter()
    w.put(SYNC, 16)
    w.put(0, 32)
    w.put(0, 16)
    w.put(blk.n, 16)
    w.put(blk.type, 2)
    if blk.type == COMPRESS:
        for ch, init in zip(blk.chans, inits):
            w.put(ch.rshift, 4)
            assert len(ch.codes) == fmt.order
            for o, c in enumerate(ch.codes, start=1):
                w.put(fold(c), 16 if o < 4 else 8)
            if ch.ltm is None:
                w.put(0, 1)
            else:
                pitch, taps = ch.ltm
                assert len(taps) == fmt.ntaps
                w.put(1, 1)
                w.put(pitch, LTM_PERIOD_BITS)
                for t in taps:
                    w.put(fold(t), 16)
            w.put(init, fmt.bits)
            st.max_init = max(st.max_init, init)
    w.align()
    if blk.type == RAW:
        widths = raw_widths(fmt)
        st.raw_widths |= set(widths)
        for s in range(blk.n):
            for ch in range(fmt.num_channels):
                w.put(int(blk.raw[ch][s]), widths[ch])
    elif blk.type == COMPRESS:
        put_residuals(w, codes, inits, st)
    w.align()
    out = bytearray(w.tobytes())
    out[2:6] = (len(out) - 6).to_bytes(4, "big")
    out[6:8] = crc16(out[8:]).to_bytes(2, "big")
    return bytes(out)


def write_file(fmt, blocks, num_samples=None):
    """(.sla bytes, Stats, byte offset of every block)"""
    st = Stats()
    body, offs, pos = [], [], HEADER_SIZE
    for b in blocks:
        bb = block_bytes(fmt, b, st)
        offs.append(pos)
        body.append(bb)
        pos += len(bb)
    total = sum(b.n for b in blocks) if num_samples is None else num_samples
    maxblk = max((len(b) for b in body), default=0)
    # the encoder's peak rate field, in its 32-bit arithmetic (src/SLAEncoder.c:900-905); no decoder reads it
    maxbps = max((((8 * len(bb) * fmt.rate) & M32) // b.n for bb, b in zip(body, blocks) if b.n), default=0)
    hdr = header_bytes(fmt, total, len(blocks), maxblk, maxbps)
    return hdr + b"".join(body), st, offs
