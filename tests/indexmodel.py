"""Device-free model of the block index and of the windows decoded from it (test infrastructure).

sla_hip_index (include/sla_hip.h) is the block chain of one .sla stream kept on the host; sla_hip_decode_windows_indexed
lays a window's rows out from it without reading the stream, and k_dec_judge of sla_amd/csrc/kernels/judge.inc gives the
verdict on the device.  Three parts, each the specification of one of them:
  index_of     the rows of an index from bytes: tests/walkmodel.py's whole-file walk with capacity = the header's
               num_samples, no cap on the block length and no CRC rows.
  plan_window  the rows, the gather range and the stop code of a window, from an index alone; tests/windowmodel.py's walk
               over the same bytes gives the same (tests/test_index_model.py holds the two together).
  judge        the judge kernel's rule as a serial loop over an item's rows.
tests/test_index_model.py pins sla_hip_index_build to index_of, tests/test_gpu_dec_judge.py the kernel to judge.
"""
from dataclasses import dataclass, field

import walkmodel as WM
from walkmodel import BUF, DATA, HEADER_SIZE, OK

NG, SYNTH, HEADER_FORMAT, CORRUPT = 1, 8, 10, 11      # SLAApiResult: NG, FAILED_TO_SYNTHESIZE, INVALID_HEADER_FORMAT, DETECT_DATA_CORRUPTION
MAX_BLOCK_SAMPLES = 65535                              # the format's: a 16-bit field
NO_EMIT = 0xFFFFFFFF


@dataclass
class Index:
    data_size: int
    has_header: bool                             # DecodeHeader delivered fields (OK or DETECT_DATA_CORRUPTION)
    total: int = 0                               # the header's num_samples
    rows: list = field(default_factory=list)     # (byte_off, byte_len, smp_off, num_samples), file positions
    stop: int = OK
    extent: int = 0


def header_readable(data):
    """whether SLADecoder_DecodeHeader delivers the header's fields: 43 bytes, the signature, format version 1"""
    data = bytes(data[:HEADER_SIZE])
    return len(data) == HEADER_SIZE and data[:4] == b"SL*\x01" and int.from_bytes(data[10:14], "big") == 1


def index_of(data):
    data = bytes(data)
    x = Index(len(data), header_readable(data))
    if x.has_header:
        x.total = WM.header_total(data)
        w = WM.walk(data, x.total, x.total, MAX_BLOCK_SAMPLES, crc_check=0)
        x.rows = [r[:4] for r in w.rows]
        x.stop = w.stop
        x.extent = w.rows[-1][2] + w.rows[-1][3] if w.rows else 0
    return x


@dataclass
class Plan:
    rows: list = field(default_factory=list)     # the kept rows, file positions
    stop: int = OK
    first_byte: int = 0
    first_sample: int = 0
    end_byte: int = 0
    end_sample: int = 0


def plan_window(x, win_start, win_len, max_block_samples):
    """the window [win_start, min(win_start + win_len, total)) from the index: windowmodel.walk's rules over the rows; where
    the rows run out in front of the window's end, the index's stop code (DATA if that is OK) plays the walk's part"""
    p = Plan()
    win_end = min(win_start + win_len, x.total)
    i, pos = 0, 0
    while True:
        pos = x.rows[i][2] if i < len(x.rows) else x.extent
        if pos >= win_end:
            break
        if i == len(x.rows):
            p.stop = x.stop if x.stop != OK else DATA
            break
        off, blen, pos, n = x.rows[i]
        i += 1
        if n == 0 or pos + n <= win_start:
            continue
        if n > max_block_samples:
            p.stop = BUF
            break
        if not p.rows:
            p.first_byte, p.first_sample = off, pos
        p.rows.append((off, blen, pos, n))
        p.end_byte, p.end_sample = off + blen, pos + n
    return p


def judge_row(image, row, info, crc_check, lms_ok):
    """the code of one row, 0 when it is clean.  row: (byte_off, byte_len, smp_off, num_samples) in the pass image;
    info: (type, used_bytes, crc, overrun)"""
    off, blen, _, n = row[:4]
    typ, used, crc, overrun = info
    if off + 10 > len(image):
        return CORRUPT
    h = bytes(image[off:off + 10])
    if h[0:2] != b"\xff\xff" or (int.from_bytes(h[2:6], "big") + 6) & 0xFFFFFFFF != blen or int.from_bytes(h[8:10], "big") != n:
        return CORRUPT                                   # 1. the index is stale
    if crc_check and crc != int.from_bytes(h[6:8], "big"):
        return CORRUPT                                   # 2. the CRC
    if typ > 2:
        return HEADER_FORMAT                             # 3.
    if typ == 0 and not lms_ok:
        return SYNTH                                     # 4.
    if overrun or used != blen:
        return CORRUPT                                   # 5.
    return 0


def judge(image, rows, infos, items, crc_check, lms_ok, emit, num_outcomes):
    """items: [(first, nb, stop, ok_samples, outcome, emit, fill_end)]; emit: [[done, fill_end]], patched in place.
    Returns {outcome: (result, output_num_samples)}."""
    out = {}
    for first, nb, stop, ok_samples, outcome, e, fill_end in items:
        if first > len(rows) or nb > len(rows) - first:
            result = NG
        else:
            result = stop
            for r in range(first, first + nb):
                code = judge_row(image, rows[r], infos[r], crc_check, lms_ok)
                if code:
                    result = code
                    break
        if outcome < num_outcomes:
            out[outcome] = (result, ok_samples if result == OK else 0)
        if result != OK and e < len(emit):
            emit[e][0], emit[e][1] = 0, fill_end
    return out
