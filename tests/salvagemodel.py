"""Device-free statement of the salvage rule (test infrastructure): which blocks of a damaged .sla stream
sla_hip_salvage_resident decodes, where their samples go, and which sample ranges are lost.  It is the specification:
tests/test_salvage_model.py pins it to tests/walkmodel.py on undamaged streams and to a catalogue of damage,
tests/test_gpu_salvage.py holds the scan kernels (sla_amd/csrc/kernels/salvage.inc) and the call against it.

With S the stream's size and N, C from its header:
  node         tests/widewalkmodel.py::nodes -- 43 <= p, p + 11 <= S, FF FF at p, 8 <= size field + 6 (mod 2^32) <= S - p
  sound block  a node whose sample count n is <= max_block_samples, whose byte length is <= 64 + 16 * C * max(n, 1),
               and whose stored CRC16 equals the CRC16 of its bytes [8, length)
  mode 1       the plain walk (walkmodel.walk with capacity N) stops OK with extent N: every block of the chain keeps
               its position; one whose CRC differs is not decoded (a header-only row) and becomes silence, one that the
               decoder cannot decode becomes silence too
  mode 2       everything else: the PREFIX -- sound blocks from byte 43, sample 0, each starting where the one before
               ended, while s + n <= N -- ends at byte p0, sample s0; the SUFFIX is the chain of the smallest sound
               q >= p0 whose links (sound block to the sound block that starts exactly at its end) end exactly at byte S
               with a sample sum T <= N - s0, placed at sample N - T; [s0, N - T) is lost (without suffix [s0, N)).
A block that passes its CRC and still fails in the decoder (type > 2, reader overrun, a body that does not end where the
size field says) cannot be known here: the caller names such blocks by their byte position in `undecodable`.
"""
from dataclasses import dataclass, field

import numpy as np

import walkmodel as WM
import widewalkmodel as WW

CRC, UNDECODABLE, GAP = 1, 2, 3          # SLA_HIP_SALVAGE_CRC / _UNDECODABLE / _GAP: why a range is silent
NONE = 0xFFFFFFFF

_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xA001 if _c & 1 else _c >> 1
    _TABLE.append(_c)


def crc16(data):
    """CRC16-IBM, reflected 0xA001, start value 0 (the table walk of tests/slastream.py::crc16)"""
    crc = 0
    for b in bytes(data):
        crc = (crc >> 8) ^ _TABLE[(crc ^ b) & 0xFF]
    return crc


def max_block_bytes(channels, n):
    """SLA_HIP_SALVAGE_MAX_BLOCK_BYTES of include/sla_hip.h: four times a RAW block of 32-bit samples"""
    return 64 + 16 * channels * max(n, 1)


@dataclass
class Salvage:
    mode: int = 0
    rows: list = field(default_factory=list)     # (byte_off, byte_len, smp_off, num_samples, flags, crc_field), as walkmodel
    lost: list = field(default_factory=list)     # (start, length, reason), ascending, no empty range
    concealed: int = 0                           # rows that become silence
    prefix_blocks: int = 0                       # mode 2 from here on
    prefix_samples: int = 0                      # s0
    prefix_end: int = WM.HEADER_SIZE             # p0
    suffix_byte: int = 0                         # q, 0 when there is no suffix
    suffix_samples: int = 0                      # T
    suffix_blocks: int = 0
    nodes: int = 0
    sound_nodes: int = 0
    total: int = 0                               # N of the header

    @property
    def decoded(self):
        return len(self.rows) - self.concealed

    @property
    def samples_lost(self):
        return sum(length for _, length, _ in self.lost)

    @property
    def suffix_sample(self):
        return self.total - self.suffix_samples if self.suffix_byte else 0


def _node_fields(data, pos):
    d = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    bsize = ((((d[pos + 2] << 24) | (d[pos + 3] << 16) | (d[pos + 4] << 8) | d[pos + 5]) + 6) & WM.M32).astype(np.int64)
    n = ((d[pos + 8] << 8) | d[pos + 9]).astype(np.int64)
    crcf = ((d[pos + 6] << 8) | d[pos + 7]).astype(np.int64)
    return bsize, n, crcf


def sound_nodes(data, channels, max_block_samples):
    """-> (pos, bsize, n, crc field, sound flag) of every node, ascending"""
    data = bytes(data)
    pos = WW.nodes(data)
    if len(pos) == 0:
        z = np.zeros(0, np.int64)
        return pos, z, z, z, np.zeros(0, bool)
    bsize, n, crcf = _node_fields(data, pos)
    ok = np.zeros(len(pos), bool)
    for i in range(len(pos)):
        if n[i] <= max_block_samples and bsize[i] <= max_block_bytes(channels, int(n[i])):
            p = int(pos[i])
            ok[i] = crc16(data[p + WM.CRC_START:p + int(bsize[i])]) == crcf[i]
    return pos, bsize, n, crcf, ok


def salvage(data, max_block_samples, undecodable=()):
    """the rule, for a stream whose header is accepted"""
    data = bytes(data)
    size = len(data)
    channels, total = data[14], WM.header_total(data)
    r = Salvage(total=total)
    bad = set(undecodable)
    walk = WM.walk(data, total, total, max_block_samples, 1)
    if walk.stop == WM.OK and walk.extent == total:
        r.mode = 1
        for off, blen, smp, n, flags, crcf in walk.rows:
            reason = 0
            if crc16(data[off + WM.CRC_START:off + blen]) != crcf:
                reason, flags = CRC, WM.HEADER_ONLY
            elif off in bad:
                reason = UNDECODABLE
            r.rows.append((off, blen, smp, n, flags, crcf))
            if reason:
                r.concealed += 1
                if n:
                    r.lost.append((smp, n, reason))
        return r
    r.mode = 2
    pos, bsize, n, crcf, ok = sound_nodes(data, channels, max_block_samples)
    K = len(pos)
    r.nodes, r.sound_nodes = K, int(ok.sum())
    index = {int(p): i for i, p in enumerate(pos)}
    # the sound successor of every sound node, or none
    succ = [-1] * K
    for i in range(K):
        j = index.get(int(pos[i] + bsize[i]), -1)
        if ok[i] and j >= 0 and ok[j]:
            succ[i] = j
    # prefix
    p0, s0, rows = WM.HEADER_SIZE, 0, []
    i = index.get(WM.HEADER_SIZE, -1)
    if i >= 0 and not ok[i]:
        i = -1
    while i >= 0 and s0 + n[i] <= total:
        rows.append((int(pos[i]), int(bsize[i]), s0, int(n[i]), 0, int(crcf[i])))
        p0, s0 = int(pos[i] + bsize[i]), s0 + int(n[i])
        i = succ[i]
    r.prefix_blocks, r.prefix_samples, r.prefix_end = len(rows), s0, p0
    # every sound node's chain: where it ends and how many samples it carries (successors lie ahead: back to front)
    end, tsum = [0] * K, [0] * K
    for i in range(K - 1, -1, -1):
        if ok[i]:
            j = succ[i]
            end[i] = end[j] if j >= 0 else int(pos[i] + bsize[i])
            tsum[i] = int(n[i]) + (tsum[j] if j >= 0 else 0)
    q = next((i for i in range(K) if ok[i] and pos[i] >= p0 and end[i] == size and tsum[i] <= total - s0), -1)
    T = 0
    if q >= 0:
        T = tsum[q]
        r.suffix_byte, r.suffix_samples = int(pos[q]), T
        s, i = total - T, q
        while i >= 0:
            rows.append((int(pos[i]), int(bsize[i]), s, int(n[i]), 0, int(crcf[i])))
            s += int(n[i])
            i = succ[i]
            r.suffix_blocks += 1
    r.rows = rows
    for k, (off, blen, smp, cnt, flags, c) in enumerate(rows):
        if off in bad:
            r.concealed += 1
            if cnt:
                r.lost.append((smp, cnt, UNDECODABLE))
    if total - T > s0:
        r.lost.append((s0, total - T - s0, GAP))
    r.lost.sort()
    return r
