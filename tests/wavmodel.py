"""A device-free model of the library's WAV layer (include/sla_hip.h, "WAV files"): the RIFF/WAVE reader and the canonical
44-byte writer, and the sample maps between packed little-endian frames and planar left-justified int32 words.  Written
from the format and from the table in include/sla_hip.h; the tests hold sla_wav.c and the kernels of kernels/wav.inc
against it."""
import struct

import numpy as np

OK, INVALID_ARGUMENT, INSUFFICIENT_DATA_SIZE, INVALID_HEADER_FORMAT = 0, 2, 9, 10
HEADER_BYTES = 44


class Info:
    __slots__ = ("num_channels", "bits_per_sample", "sampling_rate", "num_samples", "data_off", "data_bytes")

    def __init__(self, num_channels=0, bits_per_sample=0, sampling_rate=0, num_samples=0, data_off=0, data_bytes=0):
        self.num_channels, self.bits_per_sample, self.sampling_rate = num_channels, bits_per_sample, sampling_rate
        self.num_samples, self.data_off, self.data_bytes = num_samples, data_off, data_bytes

    def fields(self):
        return tuple(getattr(self, k) for k in self.__slots__)


def frames_from_planes(planes, bits):
    """planar left-justified int32 [C][n] -> the bytes of the interleaved little-endian frames"""
    planes = np.asarray(planes, np.int32)
    inter = np.ascontiguousarray(planes.T)                       # [n][C]
    if bits == 8:
        return ((inter >> 24) + 128).astype(np.uint8).tobytes()
    if bits == 16:
        return (inter >> 16).astype("<i2").tobytes()
    if bits == 24:
        return (inter >> 8).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    assert bits == 32
    return inter.astype("<i4").tobytes()


def planes_from_frames(raw, num_channels, bits):
    """the bytes of interleaved little-endian frames -> planar left-justified int32 [C][n]"""
    raw = np.frombuffer(raw, np.uint8)
    B = bits // 8
    n = len(raw) // (B * num_channels)
    raw = raw[:n * B * num_channels]
    if bits == 8:
        a = (raw.astype(np.int32) - 128) << 24
    elif bits == 16:
        a = raw.view("<i2").astype(np.int32) << 16
    elif bits == 24:
        b = raw.reshape(-1, 3).astype(np.uint32)
        a = ((b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)).astype(np.uint32).view(np.int32)
    else:
        a = raw.view("<i4").astype(np.int32)
    return np.ascontiguousarray(a.reshape(n, num_channels).T)


def header44(info):
    """the canonical 44-byte header"""
    frame = info.num_channels * (info.bits_per_sample // 8)
    return (b"RIFF" + struct.pack("<I", (36 + info.data_bytes) & 0xFFFFFFFF) + b"WAVEfmt " + struct.pack("<I", 16)
            + struct.pack("<HHIIHH", 1, info.num_channels, info.sampling_rate, (info.sampling_rate * frame) & 0xFFFFFFFF,
                          frame & 0xFFFF, info.bits_per_sample)
            + b"data" + struct.pack("<I", info.data_bytes))


def chunk(cid, body):
    """one RIFF chunk, pad byte included"""
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def build_wav(planes, bits, rate, chunks_before_fmt=(), chunks_before_data=(), extensible=False, sub_format=1,
              valid_bits=None, data_size=None):
    """a WAV file of the planes; chunks_*: (id, body) pairs; extensible: a WAVE_FORMAT_EXTENSIBLE `fmt ` of 40 bytes;
    data_size: the size the data chunk claims (default: what it holds)"""
    planes = np.asarray(planes, np.int32)
    C = planes.shape[0]
    frames = frames_from_planes(planes, bits)
    frame = C * (bits // 8)
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else 1, C, rate, rate * frame, frame, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, 0)
        fmt += struct.pack("<H", sub_format) + bytes.fromhex("000000001000800000aa00389b71")
    body = b"WAVE"
    for cid, b in chunks_before_fmt:
        body += chunk(cid, b)
    body += chunk(b"fmt ", fmt)
    for cid, b in chunks_before_data:
        body += chunk(cid, b)
    body += b"data" + struct.pack("<I", len(frames) if data_size is None else data_size) + frames
    return b"RIFF" + struct.pack("<I", len(body)) + body


def canonical(planes, bits, rate):
    """the file the library's writer makes of the planes"""
    planes = np.asarray(planes, np.int32)
    frames = frames_from_planes(planes, bits)
    return header44(Info(planes.shape[0], bits, rate, planes.shape[1], HEADER_BYTES, len(frames))) + frames


def parse(data):
    """(result code, Info): the reader of include/sla_hip.h, the codes by its table"""
    data = bytes(data)
    size = len(data)
    if size < 12 or data[0:4] != b"RIFF" or data[8:12] != b"WAVE":
        return INVALID_HEADER_FORMAT, Info()
    pos, fmt = 12, None
    while True:
        if pos + 8 > size:
            return INSUFFICIENT_DATA_SIZE, Info()
        cid = data[pos:pos + 4]
        csize = struct.unpack_from("<I", data, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if csize < 16:
                return INVALID_HEADER_FORMAT, Info()
            if body + 16 > size:
                return INSUFFICIENT_DATA_SIZE, Info()
            tag, ch, rate, _, _, bits = struct.unpack_from("<HHIIHH", data, body)
            if tag == 0xFFFE:
                if csize < 40:
                    return INVALID_HEADER_FORMAT, Info()
                if body + 40 > size:
                    return INSUFFICIENT_DATA_SIZE, Info()
                cb, valid = struct.unpack_from("<HH", data, body + 16)
                sub = struct.unpack_from("<H", data, body + 24)[0]
                if cb < 22 or sub != 1 or valid != bits:
                    return INVALID_HEADER_FORMAT, Info()
            elif tag != 1:
                return INVALID_HEADER_FORMAT, Info()
            if bits not in (8, 16, 24, 32) or ch == 0:
                return INVALID_HEADER_FORMAT, Info()
            fmt = (ch, bits, rate)
        elif cid == b"data":
            if fmt is None:
                return INVALID_HEADER_FORMAT, Info()
            if body + csize > size:
                return INSUFFICIENT_DATA_SIZE, Info()
            frame = fmt[0] * (fmt[1] // 8)
            n = csize // frame
            return OK, Info(fmt[0], fmt[1], fmt[2], n, body, n * frame)
        pos = body + csize + (csize & 1)


def read(data):
    """(planes, bits, rate) of a file the reader accepts"""
    rc, info = parse(data)
    assert rc == OK, rc
    raw = bytes(data)[info.data_off:info.data_off + info.data_bytes]
    return planes_from_frames(raw, info.num_channels, info.bits_per_sample), info.bits_per_sample, info.sampling_rate
