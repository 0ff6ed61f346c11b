"""Device-free restatement of the block-chain walk (test infrastructure).

The decoder follows a .sla file's chain of blocks -- sync code, size field, sample count: 10 bytes per block -- to lay
the blocks out as a table before any kernel decodes them.  On the host that is walk_chain() of
sla_amd/csrc/sla_decoder.c, on the device k_dec_walk of sla_amd/csrc/sla_decode.hip (sla_hip_launch_dec_walk); both
restate the reference's loop (src/SLADecoder.c:696-722) for a whole file: from byte 43, sample 0.  This module is the
third statement, in Python, with the same checks in the same order and the same 32-bit arithmetic;
tests/test_walk_model.py pins it to the oracle's encoder trace and to the crafted catalogue, tests/test_gpu_dec_walk.py
holds the kernel against it.
"""
from dataclasses import dataclass, field

HEADER_SIZE = 43
MIN_BLOCK_HEADER = 11            # SLA_MINIMUM_BLOCK_HEADER_SIZE
CRC_START = 8                    # the block's CRC16 covers [8, size field + 6)
SYNC = 0xFFFF
HEADER_ONLY = 1                  # SLA_HIP_DEC_HEADER_ONLY
M32 = 0xFFFFFFFF

OK, BUF, DATA, SYNC_LOST = 0, 4, 9, 12    # SLAApiResult: OK, INSUFFICIENT_BUFFER_SIZE, INSUFFICIENT_DATA_SIZE, FAILED_TO_FIND_SYNC_CODE


@dataclass
class Walk:
    rows: list = field(default_factory=list)     # (byte_off, byte_len, smp_off, num_samples, flags, crc_field)
    stop: int = OK
    extent: int = 0

    @property
    def num_blocks(self):
        return len(self.rows)


def walk(data, total, capacity, max_block_samples, crc_check=1):
    """the walk of a whole file: `total` is the header's num_samples, `capacity` the samples per channel of the
    destination, `max_block_samples` the handle's block capacity"""
    data = bytes(data)
    size = len(data)
    w = Walk()
    off, pos = HEADER_SIZE, 0
    while pos < total:
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
        flags = 0
        if n > ((capacity - pos) & M32) or n > max_block_samples:
            w.stop = BUF
            if crc_check != 1:
                break
            flags = HEADER_ONLY                                   # its CRC is still checked first: kept, header only
        w.rows.append((off, bsize, pos, n, flags, int.from_bytes(p[6:8], "big")))
        if flags:
            break
        w.extent = max(w.extent, pos + n)
        off += bsize
        pos += n
    return w


def header_total(data):
    """num_samples of the file header"""
    return int.from_bytes(bytes(data[15:19]), "big")
