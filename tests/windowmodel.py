"""Device-free restatement of the block-chain walk for a window of samples (test infrastructure).

sla_hip_decode_windows_resident delivers the samples [start, start + length) of a .sla stream, clipped to the file.
Blocks are independent, so the window needs exactly the blocks it overlaps and the 10-byte chain headers in front of
them; k_dec_walk_window of sla_amd/csrc/sla_decode.hip (sla_hip_launch_dec_walk_window) finds them, one file per lane.
This module is the specification of that walk, in Python, in the style of tests/walkmodel.py: the same three chain checks
in the same order and the same 32-bit arithmetic.  What differs from the whole-file walk: it may start at a hint
(seek_byte, seek_sample), it ends at the window's end, a block in front of the window is passed over without a row and
without any further check, and there is neither a capacity test nor a header-only row.  The sample position only grows
(it is not reduced modulo 2^32).  tests/test_window_model.py pins it to walkmodel.walk,
tests/test_gpu_dec_walk_window.py holds the kernel against it.
"""
from dataclasses import dataclass, field

from walkmodel import BUF, CRC_START, DATA, HEADER_SIZE, M32, MIN_BLOCK_HEADER, OK, SYNC, SYNC_LOST    # noqa: F401


@dataclass
class WindowWalk:
    rows: list = field(default_factory=list)     # kept blocks: (byte_off, byte_len, smp_off, num_samples, crc_field), file positions
    stop: int = OK
    skipped: int = 0                             # blocks passed over
    first_byte: int = 0                          # file position of the first kept block; 0, 0 when none was kept
    first_sample: int = 0
    end_byte: int = 0                            # file position behind the last kept block; 0, 0 when none was kept
    end_sample: int = 0

    @property
    def num_blocks(self):
        return len(self.rows)


def walk(data, total, win_start, win_len, max_block_samples, seek_byte=0, seek_sample=0):
    """the walk for the window [win_start, min(win_start + win_len, total)) of a file whose header says `total` samples"""
    data = bytes(data)
    size = len(data)
    w = WindowWalk()
    win_end = min(win_start + win_len, total)                    # in 64 bits: no wrap
    off, pos = (seek_byte, seek_sample) if seek_byte else (HEADER_SIZE, 0)
    while pos < win_end:
        if off > size:
            w.stop = DATA
            break
        left = size - off
        if left < MIN_BLOCK_HEADER:
            w.stop = DATA
            break
        p = data[off:off + 10]
        if int.from_bytes(p[0:2], "big") != SYNC:
            w.stop = SYNC_LOST
            break
        bsize = (int.from_bytes(p[2:6], "big") + 6) & M32          # wraps, as uint32 does
        n = int.from_bytes(p[8:10], "big")
        if bsize > left or bsize < CRC_START:
            w.stop = DATA
            break
        if n == 0 or pos + n <= win_start:                         # in front of the window: passed over, not looked at again
            w.skipped += 1
            off = (off + bsize) & M32
            pos += n
            continue
        if n > max_block_samples:                                  # not kept: windows have no header-only rows
            w.stop = BUF
            break
        if not w.rows:
            w.first_byte, w.first_sample = off, pos
        w.rows.append((off, bsize, pos, n, int.from_bytes(p[6:8], "big")))
        off = (off + bsize) & M32
        pos += n
        w.end_byte, w.end_sample = off, pos
    return w


def table_rows(w, img_off=0, plane_off=0):
    """the write-mode rows of a pass that gathered [first_byte, end_byte) to img_off and gave the file the plane region at
    plane_off from first_sample on: [(byte_off, byte_len, smp_off, num_samples, flags)], the block end, the CRC fields"""
    rows = [(img_off + off - w.first_byte, blen, plane_off + pos - w.first_sample, n, 0) for off, blen, pos, n, _ in w.rows]
    return rows, img_off + (w.end_byte - w.first_byte), [r[4] for r in w.rows]
