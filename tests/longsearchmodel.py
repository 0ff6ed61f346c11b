"""A model of the exactness limit of the long-block tile-sum search (option "long_tile_search", include/sla_hip.h:
sla_hip_launch_search_far): which (super-frame, channel) groups of a file lie under 2^exact_bits units^2 and which are flagged
and rerun as serial chains.  Exact integer arithmetic throughout.

The search analyses the un-windowed samples x = raw * 2^-31 (mid = (l + r) / 2, side = l - r with mid/side).  Every raw word is
a multiple of 2^ntz, ntz the trailing zeros of the OR of all input words, so in units of 2^(ntz - 31 - ms) every sample is an
integer: raw >> ntz without mid/side, (l + r) >> ntz and 2 (l - r) >> ntz with it.  A group is exact while its window's energy,
the sum of the squares of those integers, stays below 2^exact_bits (the encoder's limit, sla_encoder.c: search_launch).  The
device adds the same energy up in doubles; the two verdicts agree because every partial sum of integers below 2^53 is exact
and a partial sum that reaches 2^53 stays there (rounding is monotone and 2^53 is representable).

Super-frames as the encoder's table has them (reference src/SLAEncoder.c:846-869): from `pos`, a window of min(max_block,
remaining) samples; a run of all-zero samples at its start of at least min(2048, remaining) samples is one SILENT block and is
hopped, anything else is a searched super-frame of the whole window."""
import numpy as np

TILE = 1024
MIN_BLOCK = 2048


def ntz_of(pcm):
    word = int(np.bitwise_or.reduce(pcm.astype(np.int64).ravel() & 0xFFFFFFFF))
    assert word != 0
    return (word & -word).bit_length() - 1


def super_frames(pcm, max_block):
    """[(start, window)] of the searched super-frames"""
    n = pcm.shape[1]
    live = np.any(pcm != 0, axis=0)
    nz = np.nonzero(live)[0]
    out, pos = [], 0
    while pos < n:
        remain = n - pos
        window = min(max_block, remain)
        k = np.searchsorted(nz, pos)
        nxt = int(nz[k]) if k < len(nz) else n             # first non-zero sample at or behind pos
        run = min(nxt - pos, window)
        if run >= min(MIN_BLOCK, remain):
            pos += run
        else:
            out.append((pos, window))
            pos += window
    return out


def group_energies(pcm, max_block, ms):
    """[(start, window, channel, energy in units^2 as a Python integer)], in the order of the search's groups"""
    ntz = ntz_of(pcm)
    out = []
    for start, window in super_frames(pcm, max_block):
        seg = [[int(v) for v in pcm[ch, start:start + window]] for ch in range(pcm.shape[0])]
        if ms:
            assert len(seg) == 2
            chans = [[(l + r) >> ntz for l, r in zip(*seg)], [(2 * (l - r)) >> ntz for l, r in zip(*seg)]]
        else:
            chans = [[v >> ntz for v in s] for s in seg]
        for ch, s in enumerate(chans):
            out.append((start, window, ch, sum(v * v for v in s)))
    return out


def flagged(pcm, max_block, ms, exact_bits=53):
    """(number of groups at or over the limit, number of groups)"""
    e = group_energies(pcm, max_block, ms)
    return sum(1 for g in e if g[3] >= (1 << exact_bits)), len(e)


def grid(window):
    """the candidates of the partition search on one super-frame (reference src/SLAPredictor.c:1615-1630)"""
    nodes = (window + TILE - 1) // TILE + 1
    out = []
    for p in range(nodes):
        for q in range(p + 1, nodes):
            n = min((q - p) * TILE, window - p * TILE)
            if n >= min(MIN_BLOCK, window):
                out.append((p * TILE, n))
    return out
