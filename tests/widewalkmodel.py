"""Device-free restatement of the wide walk (test infrastructure): the block table of one stream found the way
sla_hip_launch_dec_walk_wide finds it (sla_amd/csrc/kernels/walk_wide.inc) -- every byte position tested on its own for
"a block could start here", the successor table, pointer-doubling rounds that rank the path from byte 43, and the cut
where the lane walk would stop -- in numpy.  tests/test_wide_walk_model.py pins it to tests/walkmodel.py::walk, which is
the specification; tests/test_gpu_dec_walk_wide.py holds the kernels against both."""
import numpy as np

import walkmodel as WM

NONE = 0xFFFFFFFF
OVERFLOW = 1                     # SLA_HIP_DEC_WIDE_OVERFLOW


def _fields(data):
    d = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    return d, len(d)


def nodes(data):
    """positions p with 43 <= p, p + 11 <= len, FF FF at p and 8 <= (size field + 6 mod 2^32) <= len - p, ascending"""
    d, size = _fields(data)
    if size < WM.HEADER_SIZE + WM.MIN_BLOCK_HEADER:
        return np.zeros(0, np.int64)
    p = np.arange(WM.HEADER_SIZE, size - WM.MIN_BLOCK_HEADER + 1, dtype=np.int64)
    p = p[(d[p] == 0xFF) & (d[p + 1] == 0xFF)]
    bsize = (((d[p + 2] << 24) | (d[p + 3] << 16) | (d[p + 4] << 8) | d[p + 5]) + 6) & WM.M32
    return p[(bsize >= WM.CRC_START) & (bsize <= (size - p).astype(np.uint64))]


def rounds(data_size, node_capacity):
    """the doubling rounds the launcher issues (sla_hip_dec_wide_rounds): blocks are at least 8 bytes long and the
    last one starts at least 11 bytes before the end"""
    longest = 0 if data_size < 54 else (data_size - 54) // 8 + 1
    longest = min(longest, node_capacity)
    r = 0
    while (1 << r) < longest:
        r += 1
    return r


def scratch_bytes(data_size, node_capacity):
    """SLA_HIP_DEC_WIDE_SCRATCH_BYTES of include/sla_hip.h"""
    tiles = ((data_size + 46) // 32 + 255) // 256
    return 64 + tiles * 2048 + ((tiles * 4 + 15) & ~15) + ((node_capacity + 3) & ~3) * 64


def _stop_at(data, off):
    """the lane walk's stop code at a byte where no node is"""
    size = len(data)
    if off > size or size - off < WM.MIN_BLOCK_HEADER:
        return WM.DATA
    if data[off] != 0xFF or data[off + 1] != 0xFF:
        return WM.SYNC_LOST
    return WM.DATA


class WideWalk(WM.Walk):
    overflow = 0
    num_nodes = 0
    rounds = 0


def wide_walk(data, total, capacity, max_block_samples, crc_check=1, node_capacity=1 << 20):
    """-> WideWalk: rows, stop and extent as walkmodel.walk gives them, plus overflow, num_nodes and rounds"""
    data = bytes(data)
    d, size = _fields(data)
    w = WideWalk()
    if total == 0 or size < WM.HEADER_SIZE + WM.MIN_BLOCK_HEADER:
        w.stop = WM.OK if total == 0 else WM.DATA
        return w
    pos = nodes(data)
    w.num_nodes = N = len(pos)
    w.rounds = R = rounds(size, node_capacity)
    if N > node_capacity:
        w.overflow = OVERFLOW
        return w
    if N == 0 or pos[0] != WM.HEADER_SIZE:
        w.stop = _stop_at(data, WM.HEADER_SIZE)
        return w
    bsize = ((((d[pos + 2] << 24) | (d[pos + 3] << 16) | (d[pos + 4] << 8) | d[pos + 5]) + 6) & WM.M32).astype(np.int64)
    n = ((d[pos + 8] << 8) | d[pos + 9]).astype(np.int64)
    crcf = ((d[pos + 6] << 8) | d[pos + 7]).astype(np.int64)
    # the successor: the node at pos + bsize, or none (index N stands for none: a sink that points to itself)
    at = np.searchsorted(pos, pos + bsize)
    hit = (at < N) & (pos[np.minimum(at, N - 1)] == pos + bsize)
    succ = np.where(hit, at, N)
    jump = np.append(succ, N)
    ssum = np.append(n, 0)
    rank = np.full(N + 1, -1, np.int64)
    spos = np.zeros(N + 1, np.int64)
    rank[0] = 0
    for r in range(R):
        known = np.nonzero((rank[:N] >= 0) & (jump[:N] < N))[0]
        tgt = jump[known]
        assert np.all(rank[tgt] < 0) and len(np.unique(tgt)) == len(tgt)      # no two lanes write one slot
        new_rank, new_spos = rank.copy(), spos.copy()
        new_rank[tgt] = rank[known] + (1 << r)
        new_spos[tgt] = spos[known] + ssum[known]
        ssum = ssum + ssum[jump]
        jump = jump[jump]
        rank, spos = new_rank, new_spos
    ranked = np.nonzero(rank[:N] >= 0)[0]
    order = ranked[np.argsort(rank[ranked])]
    assert np.array_equal(rank[order], np.arange(len(order)))                 # the path is ranked without a gap
    path_len = len(order)
    assert succ[order[-1]] == N
    sp, pn = spos[order], n[order]
    ok = sp >= total
    buf = ~ok & ((sp > capacity) | (pn > capacity - sp) | (pn > max_block_samples))
    cut = np.nonzero(ok | buf)[0]
    if len(cut):
        kc = int(cut[0])
        is_buf = bool(buf[kc])
        nb = kc + (1 if is_buf and crc_check == 1 else 0)
        w.stop = WM.BUF if is_buf else WM.OK
        w.extent = int(sp[kc])
    else:
        kc, nb = -1, path_len
        last = order[-1]
        w.extent = int(sp[-1] + pn[-1])
        w.stop = WM.OK if w.extent >= total else _stop_at(data, int(pos[last] + bsize[last]))
    for k in range(nb):
        i = order[k]
        w.rows.append((int(pos[i]), int(bsize[i]), int(sp[k]), int(pn[k]), WM.HEADER_ONLY if k == kc else 0, int(crcf[i])))
    return w
