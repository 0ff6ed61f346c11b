"""CPU-only checks of the WAV layer (include/sla_hip.h, "WAV files"): the model of tests/wavmodel.py against the reference's
own test file, sla_hip_wav_parse / sla_hip_wav_header against the model, the layout of the structs, the exported entry
points, and the argument checks that return before any device work."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import sla_amd
import slalibs as S
import wavmodel as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_WAV = os.path.join(ROOT, "tests", "golden", "a.wav")
ENTRY_POINTS = ("sla_hip_wav_parse", "sla_hip_wav_header", "sla_hip_launch_wav_ingest_batch", "sla_hip_launch_wav_emit_batch",
                "sla_hip_encode_wav_batch", "sla_hip_encode_wav_batch_resident", "sla_hip_decode_wav_batch",
                "sla_hip_decode_wav_batch_resident")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def planes_of(C_, n, bits, seed=1):
    rng = np.random.default_rng(seed)
    v = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(C_, n), dtype=np.int64)
    return (v << (32 - bits)).astype(np.int64).astype(np.uint32).view(np.int32) if bits < 32 else v.astype(np.int32)


def lib_parse(L, data):
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)          # (one spare byte: an empty file still has an address)
    info = sla_amd.WavInfo()
    rc = L.sla_hip_wav_parse(buf.ctypes.data, len(data), C.byref(info))
    return rc, (info.num_channels, info.bits_per_sample, info.sampling_rate, info.num_samples, info.data_off, info.data_bytes)


def same_as_model(L, data):
    want_rc, want = W.parse(data)
    rc, got = lib_parse(L, data)
    assert rc == want_rc, (rc, want_rc)
    assert got == want.fields()
    return rc


def test_model_reads_the_golden_file():
    data = open(A_WAV, "rb").read()
    planes, bits, rate = W.read(data)
    want, wbits, wrate = S.read_wav(A_WAV)
    assert (bits, rate) == (wbits, wrate)
    assert np.array_equal(planes, want)


def test_model_writer_reproduces_the_golden_file():
    data = open(A_WAV, "rb").read()
    planes, bits, rate = S.read_wav(A_WAV)
    assert W.canonical(planes, bits, rate) == data
    assert W.build_wav(planes, bits, rate) == data


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
@pytest.mark.parametrize("nch", [1, 2, 3, 8])
def test_parse_plain_files(L, bits, nch):
    data = W.build_wav(planes_of(nch, 7, bits), bits, 44100)
    assert same_as_model(L, data) == W.OK
    rc, got = lib_parse(L, data)
    assert got == (nch, bits, 44100, 7, 44, 7 * nch * bits // 8)
    planes, _, _ = W.read(data)
    assert np.array_equal(planes, planes_of(nch, 7, bits))


@pytest.mark.parametrize("before_fmt, before_data", [
    ([(b"JUNK", b"\1" * 10)], []), ([(b"JUNK", b"\1" * 11)], []), ([], [(b"LIST", b"\2" * 26)]), ([], [(b"LIST", b"\2" * 27)]),
    ([(b"bext", b"\3" * 5), (b"JUNK", b"")], [(b"LIST", b"\2" * 1), (b"fact", b"\4" * 4)])])
def test_parse_skips_other_chunks(L, before_fmt, before_data):
    planes = planes_of(2, 5, 24)
    data = W.build_wav(planes, 24, 48000, chunks_before_fmt=before_fmt, chunks_before_data=before_data)
    assert same_as_model(L, data) == W.OK
    got, _, _ = W.read(data)
    assert np.array_equal(got, planes)


def test_parse_extensible(L):
    planes = planes_of(2, 5, 24)
    assert same_as_model(L, W.build_wav(planes, 24, 96000, extensible=True)) == W.OK
    assert same_as_model(L, W.build_wav(planes, 24, 96000, extensible=True, sub_format=3)) == W.INVALID_HEADER_FORMAT
    assert same_as_model(L, W.build_wav(planes, 24, 96000, extensible=True, valid_bits=20)) == W.INVALID_HEADER_FORMAT


def test_parse_refusals(L):
    planes = planes_of(2, 5, 16)
    good = W.build_wav(planes, 16, 8000)
    # data before fmt
    frames = W.frames_from_planes(planes, 16)
    swapped = b"RIFF" + b"\0\0\0\0" + b"WAVE" + W.chunk(b"data", frames) + good[12:36]
    assert same_as_model(L, swapped) == W.INVALID_HEADER_FORMAT
    # a data size one byte too large
    assert same_as_model(L, W.build_wav(planes, 16, 8000, data_size=len(frames) + 1)) == W.INSUFFICIENT_DATA_SIZE
    # a data size that is no multiple of the frame: floored
    short = W.build_wav(planes, 16, 8000, data_size=len(frames) - 1)
    assert same_as_model(L, short) == W.OK
    assert lib_parse(L, short)[1][3:] == (4, 44, 16)
    # signature, fmt size, tag, depth, channels
    assert same_as_model(L, b"RIFX" + good[4:]) == W.INVALID_HEADER_FORMAT
    assert same_as_model(L, good[:8] + b"WAVX" + good[12:]) == W.INVALID_HEADER_FORMAT
    assert same_as_model(L, good[:16] + b"\x0e" + good[17:]) == W.INVALID_HEADER_FORMAT
    assert same_as_model(L, good[:20] + b"\x03" + good[21:]) == W.INVALID_HEADER_FORMAT
    assert same_as_model(L, good[:34] + b"\x14" + good[35:]) == W.INVALID_HEADER_FORMAT
    assert same_as_model(L, good[:22] + b"\0\0" + good[24:]) == W.INVALID_HEADER_FORMAT
    # NULL arguments
    info = sla_amd.WavInfo()
    buf = np.frombuffer(good, np.uint8)
    assert L.sla_hip_wav_parse(None, len(good), C.byref(info)) == W.INVALID_ARGUMENT
    assert L.sla_hip_wav_parse(buf.ctypes.data, len(good), None) == W.INVALID_ARGUMENT


def test_parse_every_prefix(L):
    data = W.build_wav(planes_of(2, 3, 24), 24, 48000, chunks_before_data=[(b"LIST", b"\5" * 9)])
    codes = [same_as_model(L, data[:k]) for k in range(len(data) + 1)]
    assert codes[-1] == W.OK and set(codes[:-1]) == {W.INVALID_HEADER_FORMAT, W.INSUFFICIENT_DATA_SIZE}
    # the same prefixes of an extensible file: the 40-byte fmt chunk is read only when all of it is there
    data = W.build_wav(planes_of(2, 3, 24), 24, 48000, extensible=True)
    codes = [same_as_model(L, data[:k]) for k in range(len(data) + 1)]
    assert codes[-1] == W.OK


@pytest.mark.parametrize("nch, bits, rate, n", [(1, 8, 48000, 240000), (2, 16, 44100, 1), (3, 24, 96000, 0), (8, 32, 192000, 12345)])
def test_header_equals_the_model(L, nch, bits, rate, n):
    info = sla_amd.WavInfo(nch, bits, rate, n, 44, n * nch * bits // 8)
    out = (C.c_uint8 * 44)()
    assert L.sla_hip_wav_header(C.byref(info), out) == 0
    want = W.header44(W.Info(nch, bits, rate, n, 44, n * nch * bits // 8))
    assert bytes(out) == want
    assert same_as_model(L, want + bytes(n * nch * bits // 8)) == W.OK
    assert L.sla_hip_wav_header(None, out) == W.INVALID_ARGUMENT
    assert L.sla_hip_wav_header(C.byref(info), None) == W.INVALID_ARGUMENT


def test_struct_layouts():
    # (the fields the header declares for sla_hip_wav_item -- two pointers and six 32-bit words -- take 40 bytes)
    def layout(T):
        return [(name, getattr(T, name).offset) for name, _ in T._fields_]
    assert C.sizeof(sla_amd.WavItem) == 40
    assert layout(sla_amd.WavItem) == [("src", 0), ("dst", 8), ("src_size", 16), ("dst_capacity", 20), ("output_size", 24),
                                       ("result", 28), ("num_samples", 32), ("reserved", 36)]
    assert C.sizeof(sla_amd.WavIngest) == 24
    assert layout(sla_amd.WavIngest) == [("src", 0), ("plane_off", 8), ("num_samples", 16), ("fill_end", 20)]
    assert C.sizeof(sla_amd.WavEmit) == 80
    assert layout(sla_amd.WavEmit) == [("plane_off", 0), ("dst", 8), ("num_samples", 16), ("mid_side", 20), ("shift", 24),
                                       ("header_bytes", 28), ("header", 32)]
    assert C.sizeof(sla_amd.WavInfo) == 24
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name, size in (("sla_hip_wav_item", 40), ("sla_hip_wav_ingest", 24), ("sla_hip_wav_emit", 80)):
        assert re.search(r"\}\s*%s;\s*/\*\s*%d bytes" % (name, size), text), name


def test_header_declares_and_library_exports_the_entry_points(L):
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    assert re.search(r"#define\s+SLA_HIP_WAV_HEADER_BYTES\s+44u", text)


def test_calls_refuse_null_handle_and_null_items(L):
    items = (sla_amd.WavItem * 1)()
    items[0].result = -7
    assert L.sla_hip_encode_wav_batch(None, items, 1) == W.INVALID_ARGUMENT
    assert L.sla_hip_encode_wav_batch_resident(None, items, 1, None, 0, None) == W.INVALID_ARGUMENT
    assert L.sla_hip_decode_wav_batch(None, items, 1) == W.INVALID_ARGUMENT
    assert L.sla_hip_decode_wav_batch_resident(None, items, 1, None) == W.INVALID_ARGUMENT
    assert items[0].result == -7                 # nothing was touched
    assert L.sla_hip_launch_wav_ingest_batch(None, 1, 1, 2, 2, None, 0, None) == W.INVALID_ARGUMENT
    assert L.sla_hip_launch_wav_emit_batch(None, 0, None, 1, 1, 2, 2, 0, None) == W.INVALID_ARGUMENT


def test_golden_file_is_what_the_tests_expect():
    assert hashlib.md5(open(A_WAV, "rb").read()).hexdigest() == hashlib.md5(W.canonical(*S.read_wav(A_WAV))).hexdigest()
