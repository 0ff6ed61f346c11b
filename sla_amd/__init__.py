"""sla_amd -- MI355X-native encode hot path of the SLA lossless audio codec.

The product is the C-ABI shared library ``sla_amd/libsla_hip.so`` (hand-written gfx950 kernels +
plain-C host, see include/*.h).  This package is only the thin ctypes face used by the tests,
bench.py and __graft_entry__: it mirrors the reference's encoder interface
(SLAEncoder_Create / SetWaveFormat / SetEncodeParameter / EncodeWhole / EncodeBlock, reference
src/include/public/SLAEncoder.h:28-53) and decoder interface (SLADecoder_Create / DecodeHeader /
DecodeWhole, src/include/public/SLADecoder.h:38-60) one to one.

There is no CPU fallback: loading fails loudly when the library has not been built, and
``Encoder()`` raises when no HIP device is usable.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SLA_HIP_LIB") or os.path.join(_HERE, "libsla_hip.so")     # SLA_HIP_LIB: A/B runs against another build

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)
f64p = C.POINTER(C.c_double)

(WINDOW_RECT, WINDOW_SIN, WINDOW_HANN, WINDOW_BLACKMAN, WINDOW_VORBIS) = range(5)
(CH_NONE, CH_STEREO_MS) = range(2)
BLOCK_COMPRESS, BLOCK_SILENT, BLOCK_RAW = 0, 1, 2

API_RESULT = ["OK", "NG", "INVALID_ARGUMENT", "EXCEED_HANDLE_CAPACITY", "INSUFFICIENT_BUFFER_SIZE",
              "INVAILD_CHPROCESSMETHOD", "FAILED_TO_CALCULATE_COEF", "FAILED_TO_PREDICT",
              "FAILED_TO_SYNTHESIZE", "INSUFFICIENT_DATA_SIZE", "INVALID_HEADER_FORMAT",
              "DETECT_DATA_CORRUPTION", "FAILED_TO_FIND_SYNC_CODE", "INVALID_WINDOWFUNCTION_TYPE",
              "NO_DATA_FRAGMENTS", "PARAMETER_NOT_SET"]


class SLAEncoderConfig(C.Structure):
    _fields_ = [("max_num_channels", C.c_uint32), ("max_num_block_samples", C.c_uint32),
                ("max_parcor_order", C.c_uint32), ("max_longterm_order", C.c_uint32),
                ("max_lms_order_per_filter", C.c_uint32), ("verpose_flag", C.c_uint8)]


class SLADecoderConfig(C.Structure):
    _fields_ = [("max_num_channels", C.c_uint32), ("max_num_block_samples", C.c_uint32),
                ("max_parcor_order", C.c_uint32), ("max_longterm_order", C.c_uint32),
                ("max_lms_order_per_filter", C.c_uint32), ("enable_crc_check", C.c_uint8),
                ("verpose_flag", C.c_uint8)]


class SLAStreamingDecoderConfig(C.Structure):
    _fields_ = [("core_config", SLADecoderConfig), ("decode_interval_hz", C.c_float), ("max_bit_per_sample", C.c_uint32)]


class SLAWaveFormat(C.Structure):
    _fields_ = [("num_channels", C.c_uint32), ("bit_per_sample", C.c_uint32),
                ("sampling_rate", C.c_uint32), ("offset_lshift", C.c_uint8)]


class SLAEncodeParameter(C.Structure):
    _fields_ = [("parcor_order", C.c_uint32), ("longterm_order", C.c_uint32),
                ("lms_order_per_filter", C.c_uint32), ("ch_process_method", C.c_int),
                ("window_function_type", C.c_int), ("max_num_block_samples", C.c_uint32)]


class SLAHeaderInfo(C.Structure):
    _fields_ = [("wave_format", SLAWaveFormat), ("encode_param", SLAEncodeParameter),
                ("num_samples", C.c_uint32), ("num_blocks", C.c_uint32),
                ("max_block_size", C.c_uint32), ("max_bit_per_second", C.c_uint32)]


class HipTrace(C.Structure):
    _fields_ = [
        ("max_blocks", C.c_uint32), ("order_stride", C.c_uint32),
        ("ltm_stride", C.c_uint32), ("sample_stride", C.c_uint32),
        ("num_blocks", C.c_uint32), ("offset_lshift", C.c_uint32),
        ("blk_start", u32p), ("blk_nsmpl", u32p), ("blk_type", u32p), ("blk_bytes", u32p),
        ("parcor", f64p), ("code", i32p), ("kint", i32p),
        ("rshift", u32p), ("pitch", u32p), ("ltm_coef", i32p), ("rice_init", u32p),
        ("res_lattice", i32p), ("res_final", i32p), ("parcor_exact", u32p)]


class BatchItem(C.Structure):
    _fields_ = [("input", C.POINTER(i32p)), ("num_samples", C.c_uint32), ("data_size", C.c_uint32),
                ("data", u8p), ("output_size", C.c_uint32), ("result", C.c_int32)]


class DecodeItem(C.Structure):
    """sla_hip_decode_item (include/sla_hip.h): one file of sla_hip_decode_batch"""
    _fields_ = [("data", u8p), ("data_size", C.c_uint32), ("buffer_num_samples", C.c_uint32),
                ("buffer", C.POINTER(i32p)), ("output_num_samples", C.c_uint32), ("result", C.c_int32)]


class DecodeDeviceItem(C.Structure):
    """sla_hip_decode_device_item (include/sla_hip.h): one file of sla_hip_decode_batch_device"""
    _fields_ = [("data", u8p), ("dst", C.c_void_p), ("channel_stride", C.c_uint64), ("sample_stride", C.c_uint64),
                ("data_size", C.c_uint32), ("capacity", C.c_uint32), ("output_num_samples", C.c_uint32),
                ("result", C.c_int32)]


class DecWalkFile(C.Structure):
    """sla_hip_dec_walk_file (include/sla_hip.h): one file of sla_hip_launch_dec_walk"""
    _fields_ = [("src", C.c_void_p), ("img_off", C.c_uint64), ("data_size", C.c_uint32), ("total", C.c_uint32),
                ("capacity", C.c_uint32), ("first", C.c_uint32), ("max_rows", C.c_uint32), ("plane_off", C.c_uint32)]


class DecWalkResult(C.Structure):
    """sla_hip_dec_walk_result (include/sla_hip.h): what the walk returns per file"""
    _fields_ = [("num_blocks", C.c_uint32), ("stop", C.c_uint32), ("extent", C.c_uint32), ("reserved", C.c_uint32)]


class DecWideInfo(C.Structure):
    """sla_hip_dec_wide_info (include/sla_hip.h): the first 16 bytes of the wide walk's scratch, once it has run"""
    _fields_ = [("nodes", C.c_uint32), ("path_len", C.c_uint32), ("cut", C.c_uint32), ("reserved", C.c_uint32)]


class DecGather(C.Structure):
    """sla_hip_dec_gather (include/sla_hip.h): one entry of sla_hip_launch_dec_gather"""
    _fields_ = [("src", C.c_void_p), ("dst_off", C.c_uint64), ("bytes", C.c_uint32), ("reserved", C.c_uint32)]


class DecWindowFile(C.Structure):
    """sla_hip_dec_window_file (include/sla_hip.h): one file of sla_hip_launch_dec_walk_window"""
    _fields_ = [("src", C.c_void_p), ("img_off", C.c_uint64), ("data_size", C.c_uint32), ("total", C.c_uint32),
                ("win_start", C.c_uint32), ("win_len", C.c_uint32), ("seek_byte", C.c_uint32), ("seek_sample", C.c_uint32),
                ("range_bytes", C.c_uint32), ("base_byte", C.c_uint32), ("base_sample", C.c_uint32), ("plane_off", C.c_uint32),
                ("first", C.c_uint32), ("max_rows", C.c_uint32)]


class DecWindowResult(C.Structure):
    """sla_hip_dec_window_result (include/sla_hip.h): what the window walk returns per file"""
    _fields_ = [("num_blocks", C.c_uint32), ("stop", C.c_uint32), ("skipped", C.c_uint32), ("first_byte", C.c_uint32),
                ("first_sample", C.c_uint32), ("end_byte", C.c_uint32), ("end_sample", C.c_uint32), ("reserved", C.c_uint32)]


class DecodeWindowItem(C.Structure):
    """sla_hip_decode_window_item (include/sla_hip.h): one window of sla_hip_decode_windows_resident"""
    _fields_ = [("data", u8p), ("dst", C.c_void_p), ("channel_stride", C.c_uint64), ("sample_stride", C.c_uint64),
                ("data_size", C.c_uint32), ("start", C.c_uint32), ("length", C.c_uint32), ("seek_byte", C.c_uint32),
                ("seek_sample", C.c_uint32), ("output_num_samples", C.c_uint32), ("result", C.c_int32),
                ("first_block_byte", C.c_uint32), ("first_block_sample", C.c_uint32), ("reserved", C.c_uint32)]


class IndexBlock(C.Structure):
    """sla_hip_index_block (include/sla_hip.h): one row of a block index, positions in the file"""
    _fields_ = [("byte_off", C.c_uint32), ("byte_len", C.c_uint32), ("smp_off", C.c_uint32), ("num_samples", C.c_uint32)]


class IndexSummary(C.Structure):
    """sla_hip_index_summary (include/sla_hip.h): what sla_hip_index_info returns"""
    _fields_ = [("data_size", C.c_uint32), ("header_bytes", C.c_uint32), ("header_result", C.c_int32), ("stop", C.c_uint32),
                ("extent", C.c_uint32), ("num_blocks", C.c_uint32), ("header", SLAHeaderInfo)]


class IndexedWindowItem(C.Structure):
    """sla_hip_indexed_window_item (include/sla_hip.h): one window of sla_hip_decode_windows_indexed"""
    _fields_ = [("data", u8p), ("dst", C.c_void_p), ("channel_stride", C.c_uint64), ("sample_stride", C.c_uint64),
                ("index", C.c_void_p), ("data_size", C.c_uint32), ("start", C.c_uint32), ("length", C.c_uint32),
                ("reserved", C.c_uint32)]


class WindowOutcome(C.Structure):
    """sla_hip_window_outcome (include/sla_hip.h): what sla_hip_decode_windows_indexed leaves per item, in device memory"""
    _fields_ = [("result", C.c_int32), ("output_num_samples", C.c_uint32)]


class SpliceSegment(C.Structure):
    """sla_hip_splice_segment (include/sla_hip.h): samples [start, start + length) of one resident stream"""
    _fields_ = [("data", C.c_void_p), ("index", C.c_void_p), ("data_size", C.c_uint32), ("start", C.c_uint32),
                ("length", C.c_uint32), ("reserved", C.c_uint32)]


class SpliceItem(C.Structure):
    """sla_hip_splice_item (include/sla_hip.h): one output stream of sla_hip_splice_resident"""
    _fields_ = [("segments", C.POINTER(SpliceSegment)), ("data", C.c_void_p), ("num_segments", C.c_uint32),
                ("data_size", C.c_uint32), ("output_size", C.c_uint32), ("result", C.c_int32)]


class SpliceLayout(C.Structure):
    """sla_hip_splice_layout (include/sla_hip.h): what sla_hip_splice_plan returns"""
    _fields_ = [("verbatim_bytes", C.c_uint64), ("bytes", C.c_uint32), ("num_samples", C.c_uint32), ("num_blocks", C.c_uint32),
                ("edge_blocks", C.c_uint32), ("max_block_size", C.c_uint32), ("max_bit_per_second", C.c_uint32),
                ("header", C.c_uint8 * 48)]


class SpliceCheck(C.Structure):
    """sla_hip_splice_check (include/sla_hip.h): one entry of sla_hip_launch_splice_check"""
    _fields_ = [("src", C.c_void_p), ("plane_off", C.c_uint64), ("byte_len", C.c_uint32), ("num_samples", C.c_uint32),
                ("verdict", C.c_uint32), ("ordinal", C.c_uint32), ("edge", C.c_uint32), ("keep", C.c_uint32)]


class SpliceEdge(C.Structure):
    """sla_hip_splice_edge (include/sla_hip.h): one entry of sla_hip_launch_splice_edges"""
    _fields_ = [("dst", C.c_void_p), ("plane_off", C.c_uint64), ("num_samples", C.c_uint32), ("silent", C.c_uint32)]


class SpliceCopy(C.Structure):
    """sla_hip_splice_copy (include/sla_hip.h): one entry of sla_hip_launch_splice_copy"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("bytes", C.c_uint32), ("reserved", C.c_uint32)]


SPLICE_NO_EDGE = 0xFFFFFFFF


class DecJudgeItem(C.Structure):
    """sla_hip_dec_judge_item (include/sla_hip.h): one item of sla_hip_launch_dec_judge"""
    _fields_ = [("first", C.c_uint32), ("nb", C.c_uint32), ("stop", C.c_uint32), ("ok_samples", C.c_uint32),
                ("outcome", C.c_uint32), ("emit", C.c_uint32), ("fill_end", C.c_uint32), ("reserved", C.c_uint32)]


class DecEmit(C.Structure):
    """sla_hip_dec_emit (include/sla_hip.h): one entry of sla_hip_launch_dec_emit_batch"""
    _fields_ = [("plane_off", C.c_uint64), ("channel_stride", C.c_uint64), ("sample_stride", C.c_uint64), ("dst", C.c_void_p),
                ("done", C.c_uint32), ("fill_end", C.c_uint32), ("num_channels", C.c_uint32), ("mid_side", C.c_uint32),
                ("shift", C.c_uint32), ("bits_per_sample", C.c_uint32)]


class EncodeDeviceItem(C.Structure):
    """sla_hip_encode_device_item (include/sla_hip.h): one file of sla_hip_encode_batch_device"""
    _fields_ = [("src", C.c_void_p), ("channel_stride", C.c_uint64), ("sample_stride", C.c_uint64), ("data", u8p),
                ("num_samples", C.c_uint32), ("data_size", C.c_uint32), ("output_size", C.c_uint32), ("result", C.c_int32)]


class EncEmit(C.Structure):
    """sla_hip_enc_emit (include/sla_hip.h): one entry of sla_hip_launch_enc_emit_batch"""
    _fields_ = [("img_off", C.c_uint64), ("dst", C.c_void_p), ("bytes", C.c_uint32), ("header_bytes", C.c_uint32),
                ("header", C.c_uint8 * 48)]


class WavInfo(C.Structure):
    """sla_hip_wav_info (include/sla_hip.h): what sla_hip_wav_parse finds in a RIFF/WAVE file"""
    _fields_ = [("num_channels", C.c_uint32), ("bits_per_sample", C.c_uint32), ("sampling_rate", C.c_uint32),
                ("num_samples", C.c_uint32), ("data_off", C.c_uint32), ("data_bytes", C.c_uint32)]


class WavItem(C.Structure):
    """sla_hip_wav_item (include/sla_hip.h): one file of the four WAV calls"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_size", C.c_uint32), ("dst_capacity", C.c_uint32),
                ("output_size", C.c_uint32), ("result", C.c_int32), ("num_samples", C.c_uint32), ("reserved", C.c_uint32)]


class WavIngest(C.Structure):
    """sla_hip_wav_ingest (include/sla_hip.h): one entry of sla_hip_launch_wav_ingest_batch"""
    _fields_ = [("src", C.c_void_p), ("plane_off", C.c_uint64), ("num_samples", C.c_uint32), ("fill_end", C.c_uint32)]


class WavEmit(C.Structure):
    """sla_hip_wav_emit (include/sla_hip.h): one entry of sla_hip_launch_wav_emit_batch"""
    _fields_ = [("plane_off", C.c_uint64), ("dst", C.c_void_p), ("num_samples", C.c_uint32), ("mid_side", C.c_uint32),
                ("shift", C.c_uint32), ("header_bytes", C.c_uint32), ("header", C.c_uint8 * 48)]


class SalvageReport(C.Structure):
    """sla_hip_salvage_report (include/sla_hip.h): what sla_hip_salvage_resident did"""
    _fields_ = [(n, C.c_uint32) for n in ("mode", "blocks_decoded", "blocks_concealed", "samples_lost", "num_ranges", "prefix_blocks",
                                           "suffix_blocks", "suffix_byte", "suffix_sample", "nodes", "sound_nodes", "reserved")]


class SalvageRange(C.Structure):
    """sla_hip_salvage_range (include/sla_hip.h): one silent range of a salvaged stream"""
    _fields_ = [("start", C.c_uint32), ("length", C.c_uint32), ("reason", C.c_uint32)]


class SalvageScan(C.Structure):
    """sla_hip_salvage_scan (include/sla_hip.h): what sla_hip_launch_dec_salvage_scan returns"""
    _fields_ = [(n, C.c_uint32) for n in ("prefix_blocks", "prefix_samples", "prefix_end", "suffix_byte", "suffix_samples",
                                           "suffix_blocks", "nodes", "sound_nodes", "overflow")] + [("reserved", C.c_uint32 * 3)]


class DecConceal(C.Structure):
    """sla_hip_dec_conceal (include/sla_hip.h): one entry of sla_hip_launch_dec_conceal"""
    _fields_ = [("smp_off", C.c_uint32), ("num_samples", C.c_uint32)]


class LaunchExtra(C.Structure):
    """sla_hip_launch_extra (include/sla_hip.h): optional extras of one launch of an `_x` launcher; all zero = none"""
    _fields_ = [("d_span", C.c_void_p), ("d_group_count", C.c_void_p), ("clear_ptr", C.c_void_p * 3),
                ("clear_words", C.c_uint32 * 3), ("d_rice_init", C.c_void_p)]


# sample formats of sla_hip_decode_batch_device / sla_hip_encode_batch_device, flag of the former
PCM_S32_LEFT, PCM_S32, PCM_S16, PCM_F32 = range(4)
DEC_ZERO_FILL = 1
DEC_QUEUE_SLOTS = 4              # SLA_HIP_DEC_QUEUE_SLOTS (include/sla_hip.h): the staging ring of sla_hip_decode_windows_indexed
# sla_hip_salvage_range.reason
SALVAGE_CRC, SALVAGE_UNDECODABLE, SALVAGE_GAP = 1, 2, 3
SALVAGE_REASON = {SALVAGE_CRC: "crc", SALVAGE_UNDECODABLE: "undecodable", SALVAGE_GAP: "gap"}


class SlaError(RuntimeError):
    def __init__(self, code, where):
        name = API_RESULT[code] if 0 <= code < len(API_RESULT) else ("hipError %d" % (-code))
        super().__init__("%s failed: %s (%d)" % (where, name, code))
        self.code = code


def build(verbose=False):
    """Compile sla_amd/libsla_hip.so in-tree (hipcc --offload-arch=gfx950 + gcc)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "all"]
    subprocess.run(cmd, check=True, stdout=None if verbose else subprocess.DEVNULL)


_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the HIP path has no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.SLAEncoder_Create.restype = C.c_void_p
        L.SLAEncoder_Create.argtypes = [C.POINTER(SLAEncoderConfig)]
        L.SLAEncoder_Destroy.argtypes = [C.c_void_p]
        L.SLAEncoder_Destroy.restype = None
        L.SLAEncoder_SetWaveFormat.argtypes = [C.c_void_p, C.POINTER(SLAWaveFormat)]
        L.SLAEncoder_SetEncodeParameter.argtypes = [C.c_void_p, C.POINTER(SLAEncodeParameter)]
        L.SLAEncoder_EncodeHeader.argtypes = [C.POINTER(SLAHeaderInfo), u8p, C.c_uint32]
        L.SLAEncoder_EncodeWhole.argtypes = [C.c_void_p, C.POINTER(i32p), C.c_uint32, u8p, C.c_uint32, u32p]
        L.SLAEncoder_EncodeBlock.argtypes = [C.c_void_p, C.POINTER(i32p), C.c_uint32, u8p, C.c_uint32, u32p]
        L.sla_hip_analyze_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                             C.POINTER(C.c_float)]
        L.sla_hip_pack.argtypes = [C.c_void_p, u8p, C.c_uint32, u32p]
        L.sla_hip_pack_device.argtypes = [C.c_void_p, u8p, C.c_uint32, u32p]
        L.sla_hip_get_trace.argtypes = [C.c_void_p, C.POINTER(HipTrace)]
        L.sla_hip_final_residual.restype = C.c_void_p
        L.sla_hip_final_residual.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.sla_hip_lattice_residual.restype = C.c_void_p
        L.sla_hip_lattice_residual.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.sla_hip_bind_residual_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.sla_hip_device_name.restype = C.c_char_p
        L.sla_hip_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.sla_hip_last_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.sla_hip_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.sla_hip_last_block_cert.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.sla_hip_last_cert_audit.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        if hasattr(L, "sla_hip_last_ltm_cert"):              # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_last_ltm_cert.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
            L.sla_hip_ltm_cert_eps_rel.restype = C.c_double
            L.sla_hip_ltm_cert_eps_rel.argtypes = [C.c_uint32, C.c_double]
            L.sla_hip_ltm_cert_supported.argtypes = [C.c_uint32]
        if hasattr(L, "sla_hip_launch_ltm_acf_int"):         # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_launch_ltm_acf_int.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                     C.c_void_p]
        if hasattr(L, "sla_hip_launch_acf_blocks"):          # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_launch_acf_blocks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "sla_hip_launch_search_far"):          # (SLA_HIP_LIB may name an older build in an A/B run)
            far = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]      # .. d_cands, d_tile_sums, d_out, exact_limit, stream
            L.sla_hip_launch_search_far.argtypes = far
            L.sla_hip_launch_search_far_x.argtypes = far + [C.c_void_p]
            L.sla_hip_launch_lpc_far_rerun.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.sla_hip_last_expand.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        if hasattr(L, "sla_hip_last_verify"):               # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_last_verify.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
            L.sla_hip_verify_last_image.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
            L.sla_hip_launch_verify_blocks.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                       C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        if hasattr(L, "sla_hip_last_silence"):               # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_last_silence.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
            L.sla_hip_launch_zero_runs.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                   C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "sla_hip_last_search_early"):          # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_last_search_early.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.sla_hip_search_exact_lags.restype = C.c_uint32
        L.sla_hip_encoder_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        L.sla_hip_shard_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, u32p, C.POINTER(C.c_uint64)]
        L.sla_hip_shard_bounds.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32, u32p]
        L.sla_hip_shard_scan_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, u32p, u32p]
        L.sla_hip_shard_analyze.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.sla_hip_shard_analyze_no_silence.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.sla_hip_shard_header.argtypes = [C.POINTER(u8p), C.c_uint32, u8p, C.c_uint32]
        L.sla_hip_encode_batch.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_uint32]
        L.sla_hip_analyze_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, u32p, u32p, C.c_uint32,
                                                   u32p, C.POINTER(C.c_float)]
        L.sla_hip_encode_batch_device.argtypes = [C.c_void_p, C.POINTER(EncodeDeviceItem), C.c_uint32, C.c_uint32, C.c_void_p]
        L.sla_hip_launch_enc_ingest_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                      C.c_uint64, C.c_void_p, C.c_void_p]
        L.SLADecoder_Create.restype = C.c_void_p
        L.SLADecoder_Create.argtypes = [C.POINTER(SLADecoderConfig)]
        L.SLADecoder_Destroy.argtypes = [C.c_void_p]
        L.SLADecoder_Destroy.restype = None
        L.SLADecoder_DecodeHeader.argtypes = [u8p, C.c_uint32, C.POINTER(SLAHeaderInfo)]
        L.SLADecoder_SetWaveFormat.argtypes = [C.c_void_p, C.POINTER(SLAWaveFormat)]
        L.SLADecoder_SetEncodeParameter.argtypes = [C.c_void_p, C.POINTER(SLAEncodeParameter)]
        L.SLADecoder_DecodeWhole.argtypes = [C.c_void_p, u8p, C.c_uint32, C.POINTER(i32p), C.c_uint32, u32p]
        L.sla_hip_decoder_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.SLAStreamingDecoder_Create.restype = C.c_void_p
        L.SLAStreamingDecoder_Create.argtypes = [C.POINTER(SLAStreamingDecoderConfig)]
        L.SLAStreamingDecoder_Destroy.argtypes = [C.c_void_p]
        L.SLAStreamingDecoder_Destroy.restype = None
        L.SLAStreamingDecoder_SetWaveFormat.argtypes = [C.c_void_p, C.POINTER(SLAWaveFormat)]
        L.SLAStreamingDecoder_SetEncodeParameter.argtypes = [C.c_void_p, C.POINTER(SLAEncodeParameter)]
        for name in ("EstimateMinimumNessesaryDataSize", "EstimateDecodableNumSamples", "GetOutputNumSamplesPerDecode",
                     "GetRemainDataSize"):
            getattr(L, "SLAStreamingDecoder_" + name).argtypes = [C.c_void_p, u32p]
        L.SLAStreamingDecoder_AppendDataFragment.argtypes = [C.c_void_p, u8p, C.c_uint32]
        L.SLAStreamingDecoder_CollectDataFragment.argtypes = [C.c_void_p, C.POINTER(u8p), u32p]
        L.SLAStreamingDecoder_Decode.argtypes = [C.c_void_p, C.POINTER(i32p), C.c_uint32, u32p]
        L.sla_hip_decode_device.argtypes = [C.c_void_p, u8p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, u32p]
        L.sla_hip_decode_batch.argtypes = [C.c_void_p, C.POINTER(DecodeItem), C.c_uint32]
        L.sla_hip_decode_batch_device.argtypes = [C.c_void_p, C.POINTER(DecodeDeviceItem), C.c_uint32, C.c_uint32,
                                                  C.c_uint32, C.c_void_p]
        L.sla_hip_launch_dec_emit_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32,
                                                    C.c_uint32, C.c_void_p]
        L.sla_hip_launch_dec_bits_x.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sla_hip_launch_dec_finish_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                      C.c_void_p, C.c_void_p]
        if hasattr(L, "sla_hip_dec_bits_lanes"):             # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_dec_bits_lanes.argtypes = [C.c_uint32, C.c_uint32]
            L.sla_hip_dec_bits_lanes.restype = C.c_uint32
        if hasattr(L, "sla_hip_dec_ltm_window"):             # (the same)
            L.sla_hip_dec_ltm_window.argtypes = []
            L.sla_hip_dec_ltm_window.restype = C.c_uint32
        if hasattr(L, "sla_hip_decode_batch_resident"):      # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_decode_batch_resident.argtypes = [C.c_void_p, C.POINTER(DecodeDeviceItem), C.c_uint32, C.c_uint32,
                                                        C.c_uint32, C.c_void_p]
            L.sla_hip_resident_headers.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), u32p, C.c_uint32,
                                                   C.POINTER(SLAHeaderInfo), i32p, C.c_void_p]
            L.sla_hip_launch_dec_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
            L.sla_hip_launch_dec_gather.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        if hasattr(L, "sla_hip_decode_windows_resident"):    # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_decode_windows_resident.argtypes = [C.c_void_p, C.POINTER(DecodeWindowItem), C.c_uint32, C.c_uint32,
                                                          C.c_uint32, C.c_void_p]
            L.sla_hip_launch_dec_walk_window.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p]
            L.sla_hip_decoder_last_window_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        if hasattr(L, "sla_hip_launch_dec_walk_wide"):       # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_launch_dec_walk_wide.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.sla_hip_dec_wide_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
            L.sla_hip_dec_wide_scratch_bytes.restype = C.c_uint64
            L.sla_hip_dec_wide_rounds.argtypes = [C.c_uint32, C.c_uint32]
            L.sla_hip_dec_wide_rounds.restype = C.c_uint32
            L.sla_hip_decoder_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
            L.sla_hip_decoder_last_walk.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        if hasattr(L, "sla_hip_encode_batch_resident"):      # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_encode_batch_resident.argtypes = [C.c_void_p, C.POINTER(EncodeDeviceItem), C.c_uint32, C.c_uint32,
                                                        C.c_void_p, C.c_uint64, C.c_void_p]
            L.sla_hip_pack_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, u32p]
            L.sla_hip_launch_enc_emit_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        if hasattr(L, "sla_hip_wav_parse"):                  # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_wav_parse.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(WavInfo)]
            L.sla_hip_wav_header.argtypes = [C.POINTER(WavInfo), u8p]
            L.sla_hip_launch_wav_ingest_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                          C.c_uint64, C.c_void_p]
            L.sla_hip_launch_wav_emit_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                        C.c_uint32, C.c_uint32, C.c_void_p]
            L.sla_hip_encode_wav_batch.argtypes = [C.c_void_p, C.POINTER(WavItem), C.c_uint32]
            L.sla_hip_encode_wav_batch_resident.argtypes = [C.c_void_p, C.POINTER(WavItem), C.c_uint32, C.c_void_p, C.c_uint64,
                                                            C.c_void_p]
            L.sla_hip_decode_wav_batch.argtypes = [C.c_void_p, C.POINTER(WavItem), C.c_uint32]
            L.sla_hip_decode_wav_batch_resident.argtypes = [C.c_void_p, C.POINTER(WavItem), C.c_uint32, C.c_void_p]
        if hasattr(L, "sla_hip_salvage_resident"):           # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_salvage_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                                   C.c_uint32, C.POINTER(SalvageReport), C.POINTER(SalvageRange), C.c_uint32,
                                                   C.c_void_p]
            L.sla_hip_launch_dec_salvage_scan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.sla_hip_dec_salvage_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
            L.sla_hip_dec_salvage_scratch_bytes.restype = C.c_uint64
            L.sla_hip_launch_salvage_crc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
            L.sla_hip_launch_dec_conceal.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        if hasattr(L, "sla_hip_decode_windows_indexed"):     # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_index_build.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
            L.sla_hip_index_build_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
            L.sla_hip_index_info.argtypes = [C.c_void_p, C.POINTER(IndexSummary)]
            L.sla_hip_index_blocks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.sla_hip_index_destroy.argtypes = [C.c_void_p]
            L.sla_hip_index_destroy.restype = None
            L.sla_hip_index_serialized_bytes.argtypes = [C.c_void_p]
            L.sla_hip_index_serialized_bytes.restype = C.c_uint64
            L.sla_hip_index_serialize.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
            L.sla_hip_index_serialize.restype = C.c_uint64
            L.sla_hip_index_deserialize.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
            L.sla_hip_decode_windows_indexed.argtypes = [C.c_void_p, C.POINTER(IndexedWindowItem), C.c_uint32, C.c_uint32,
                                                         C.c_uint32, C.c_void_p, C.c_void_p]
            L.sla_hip_launch_dec_judge.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                   C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        if hasattr(L, "sla_hip_splice_resident"):            # (SLA_HIP_LIB may name an older build in an A/B run)
            L.sla_hip_splice_plan.argtypes = [C.POINTER(SpliceItem), C.POINTER(SpliceLayout)]
            L.sla_hip_splice_resident.argtypes = [C.c_void_p, C.POINTER(SpliceItem), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
            L.sla_hip_launch_splice_check.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                                      C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
            L.sla_hip_launch_splice_edges.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                      C.c_uint32, C.c_void_p]
            L.sla_hip_launch_splice_copy.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib = L
    return _lib


def _splice_item(segments):
    """a SpliceItem (and the array it points to) of [(src, Index, start, length)]; src: None, a (ptr, size) pair or a 1-D uint8
    CUDA tensor; the segment's data_size is the source's, or the index's where there is no source"""
    segs = (SpliceSegment * max(len(segments), 1))()
    for k, (src, index, start, length) in enumerate(segments):
        if src is None:
            ptr, size = None, (index.data_size if index is not None else 0)
        elif isinstance(src, (tuple, list)):
            ptr, size = (int(src[0]) or None), int(src[1])
        else:
            if src.dim() != 1 or str(src.dtype) != "torch.uint8" or not src.is_contiguous() or src.device.type != "cuda":
                raise ValueError("segment %d: need a 1-D contiguous uint8 CUDA tensor or a (ptr, size) pair" % k)
            ptr, size = (src.data_ptr() or None), src.numel()
        if not (0 <= int(start) <= 0xFFFFFFFF and 0 <= int(length) <= 0xFFFFFFFF and 0 <= size <= 0xFFFFFFFF):
            raise ValueError("segment %d: start %d, length %d, %d bytes" % (k, start, length, size))
        segs[k].data, segs[k].index, segs[k].data_size = ptr, (index.handle if index is not None else None), size
        segs[k].start, segs[k].length = int(start), int(length)
    item = SpliceItem()
    item.segments = C.cast(segs, C.POINTER(SpliceSegment)) if len(segments) else None
    item.num_segments = len(segments)
    return item, segs


def splice_plan(segments):
    """(result code, SpliceLayout) of the output stream made of [(src, Index, start, length)] (sla_hip_splice_plan: the layout
    rule of Decoder.splice_resident, pure host code); src may be None, or a (ptr, size) pair that is never dereferenced"""
    item, keep = _splice_item(segments)
    lay = SpliceLayout()
    rc = lib().sla_hip_splice_plan(C.byref(item), C.byref(lay))
    return int(rc), lay


def wav_info(data):
    """(result code, WavInfo) of a RIFF/WAVE file in a bytes-like object (sla_hip_wav_parse)"""
    buf = np.frombuffer(data, np.uint8)
    info = WavInfo()
    rc = lib().sla_hip_wav_parse(buf.ctypes.data if len(buf) else C.cast(C.create_string_buffer(1), C.c_void_p), len(buf),
                                 C.byref(info))
    return int(rc), info


EXPORTED_SYMBOLS = [
    # include/SLAEncoder.h
    "SLAEncoder_Create", "SLAEncoder_Destroy", "SLAEncoder_SetWaveFormat", "SLAEncoder_SetEncodeParameter",
    "SLAEncoder_EncodeHeader", "SLAEncoder_EncodeBlock", "SLAEncoder_EncodeWhole",
    # include/sla_hip.h
    "sla_hip_launch_prepass", "sla_hip_launch_lpc", "sla_hip_launch_lattice", "sla_hip_launch_tail",
    "sla_hip_launch_ltm_acf", "sla_hip_launch_rice_len", "sla_hip_launch_rice_write", "sla_hip_pack_device", "sla_hip_launch_unpack16", "sla_hip_launch_unpack24",
    "sla_hip_analyze_device", "sla_hip_pack", "sla_hip_final_residual", "sla_hip_lattice_residual",
    "sla_hip_get_trace", "sla_hip_device_name", "sla_hip_last_timing", "sla_hip_launch_search_exact",
    "sla_hip_search_exact_lags", "sla_hip_launch_plan", "sla_hip_last_counters", "sla_hip_launch_lpc_rerun", "sla_hip_last_kernel_ms", "sla_hip_launch_lpc_blocks", "sla_hip_launch_lpc_blocks_cert", "sla_hip_last_block_cert", "sla_hip_last_cert_audit", "sla_hip_launch_batch_scan", "sla_hip_launch_lattice_groups_x", "sla_hip_launch_lpc_blocks_cert_x", "sla_hip_launch_lpc_blocks_x",
    "sla_hip_launch_lpc_x", "sla_hip_launch_ltm_acf_x", "sla_hip_launch_search_exact_x", "sla_hip_launch_tail_x", "sla_hip_last_expand", "sla_hip_launch_expand", "sla_hip_launch_expand_masked",
    "sla_hip_launch_lpc_f64", "sla_hip_launch_lattice_raw", "sla_hip_launch_tail_stages", "sla_hip_launch_emphasis_i32",
    "sla_hip_launch_emphasis_f64", "sla_hip_use_tuning", "sla_hip_launch_lattice_groups", "sla_hip_launch_ltm_solve",
    "sla_hip_launch_ltm_cert_x", "sla_hip_ltm_fast_twiddles", "sla_hip_ltm_cert_eps_rel", "sla_hip_ltm_cert_supported", "sla_hip_last_ltm_cert",
    "sla_hip_launch_ltm_acf_int", "sla_hip_launch_acf_blocks", "sla_hip_launch_lpc_far", "sla_hip_launch_lpc_far_x",
    "sla_hip_launch_search_far", "sla_hip_launch_search_far_x", "sla_hip_launch_lpc_far_rerun",
    "sla_hip_encoder_set_option", "sla_hip_shard_scan", "sla_hip_shard_scan_counts", "sla_hip_shard_bounds", "sla_hip_shard_analyze", "sla_hip_shard_analyze_no_silence", "sla_hip_shard_header",
    # include/SLAPredictor.h, include/SLACoder.h (per-call API of the reference, encode side)
    "SLALPCCalculator_Create", "SLALPCCalculator_Destroy", "SLALPCCalculator_CalculatePARCORCoefDouble",
    "SLALPCCalculator_EstimateCodeLength", "SLALPCSynthesizer_Create", "SLALPCSynthesizer_Destroy", "SLALPCSynthesizer_Reset",
    "SLALPCSynthesizer_PredictByParcorCoefInt32", "SLALongTermCalculator_Create", "SLALongTermCalculator_Destroy",
    "SLALongTermCalculator_CalculateCoef", "SLALongTermSynthesizer_Create", "SLALongTermSynthesizer_Destroy",
    "SLALongTermSynthesizer_Reset", "SLALongTermSynthesizer_PredictInt32", "SLALMSFilter_Create", "SLALMSFilter_Destroy",
    "SLALMSFilter_Reset", "SLALMSFilter_PredictInt32", "SLAOptimalEncodeEstimator_Create", "SLAOptimalEncodeEstimator_Destroy",
    "SLAOptimalEncodeEstimator_SearchOptimalBlockPartitions", "SLAOptimalEncodeEstimator_CalculateMaxNumPartitions",
    "SLAEmphasisFilter_Create", "SLAEmphasisFilter_Reset", "SLAEmphasisFilter_Destroy", "SLAEmphasisFilter_PreEmphasisInt32",
    "SLAEmphasisFilter_PreEmphasisDouble", "SLACoder_Create", "SLACoder_Destroy",
    "SLACoder_CalculateInitialRecursiveRiceParameter", "sla_hip_coder_initial_parameter", "sla_hip_bind_residual_planes",
    # include/SLADecoder.h + the decode-side launchers of include/sla_hip.h
    "SLADecoder_DecodeHeader", "SLADecoder_Create", "SLADecoder_Destroy", "SLADecoder_SetWaveFormat",
    "SLADecoder_SetEncodeParameter", "SLADecoder_DecodeWhole", "sla_hip_decoder_last_timing", "sla_hip_decode_device",
    "sla_hip_launch_dec_bits", "sla_hip_launch_dec_lms", "sla_hip_launch_dec_ltm", "sla_hip_launch_dec_lattice",
    "sla_hip_launch_dec_finish", "sla_hip_launch_prepass_tiles", "sla_hip_encode_batch", "sla_hip_analyze_batch_device",
    "SLAStreamingDecoder_Create", "SLAStreamingDecoder_Destroy", "SLAStreamingDecoder_SetWaveFormat",
    "SLAStreamingDecoder_SetEncodeParameter", "SLAStreamingDecoder_EstimateMinimumNessesaryDataSize",
    "SLAStreamingDecoder_EstimateDecodableNumSamples", "SLAStreamingDecoder_GetOutputNumSamplesPerDecode",
    "SLAStreamingDecoder_AppendDataFragment", "SLAStreamingDecoder_CollectDataFragment",
    "SLAStreamingDecoder_GetRemainDataSize", "SLAStreamingDecoder_Decode",
    # decode side of include/SLAPredictor.h
    "SLALPCSynthesizer_SynthesizeByParcorCoefInt32", "SLALongTermSynthesizer_SynthesizeInt32", "SLALMSFilter_SynthesizeInt32",
    "SLAEmphasisFilter_DeEmphasisInt32", "sla_hip_launch_dec_deemphasis",
    # batch decode (include/sla_hip.h)
    "sla_hip_decode_batch", "sla_hip_launch_dec_bits_x", "sla_hip_launch_dec_finish_batch", "sla_hip_dec_bits_lanes",
    "sla_hip_dec_ltm_window",
    # batch decode into device memory (include/sla_hip.h)
    "sla_hip_decode_batch_device", "sla_hip_launch_dec_emit_batch",
    # batch decode of streams that are in device memory (include/sla_hip.h)
    "sla_hip_decode_batch_resident", "sla_hip_resident_headers", "sla_hip_launch_dec_walk", "sla_hip_launch_dec_gather",
    # sample windows of streams that are in device memory (include/sla_hip.h)
    "sla_hip_decode_windows_resident", "sla_hip_launch_dec_walk_window", "sla_hip_decoder_last_window_stats",
    # the block table of one long resident stream, built by the whole device (include/sla_hip.h, include/SLADecoder.h)
    "sla_hip_launch_dec_walk_wide", "sla_hip_dec_wide_scratch_bytes", "sla_hip_dec_wide_rounds", "sla_hip_decoder_set_option",
    "sla_hip_decoder_last_walk",
    # batch encode from device memory (include/sla_hip.h)
    "sla_hip_encode_batch_device", "sla_hip_launch_enc_ingest_batch",
    # batch encode to .sla streams that stay in device memory (include/sla_hip.h)
    "sla_hip_encode_batch_resident", "sla_hip_pack_resident", "sla_hip_launch_enc_emit_batch",
    # verification of the encoded stream on the device (include/sla_hip.h)
    "sla_hip_launch_verify_blocks", "sla_hip_last_verify", "sla_hip_verify_last_image",
    # silence from a device-written run list (include/sla_hip.h)
    "sla_hip_launch_zero_runs", "sla_hip_last_silence",
    # search beside the prepass (option "search_early")
    "sla_hip_launch_prepass_early", "sla_hip_launch_search_exact_early", "sla_hip_launch_plan_early", "sla_hip_launch_expand_early",
    "sla_hip_last_search_early",
    # WAV files (include/sla_hip.h)
    "sla_hip_wav_parse", "sla_hip_wav_header", "sla_hip_launch_wav_ingest_batch", "sla_hip_launch_wav_emit_batch",
    "sla_hip_encode_wav_batch", "sla_hip_encode_wav_batch_resident", "sla_hip_decode_wav_batch",
    "sla_hip_decode_wav_batch_resident",
    # one resident stream decoded through damage (include/sla_hip.h)
    "sla_hip_salvage_resident", "sla_hip_launch_dec_salvage_scan", "sla_hip_dec_salvage_scratch_bytes",
    "sla_hip_launch_salvage_crc", "sla_hip_launch_dec_conceal",
    # block indexes and the windows decoded from them, queued (include/sla_hip.h)
    "sla_hip_index_build", "sla_hip_index_build_resident", "sla_hip_index_info", "sla_hip_index_blocks", "sla_hip_index_destroy",
    "sla_hip_index_serialized_bytes", "sla_hip_index_serialize", "sla_hip_index_deserialize", "sla_hip_launch_dec_judge",
    "sla_hip_decode_windows_indexed",
    # cutting and joining resident streams (include/sla_hip.h)
    "sla_hip_splice_plan", "sla_hip_splice_resident", "sla_hip_launch_splice_check", "sla_hip_launch_splice_edges",
    "sla_hip_launch_splice_copy",
]


class Trace:
    """numpy view of the per-block results of the last analysis (same fields as the oracle's trace)."""

    def __init__(self, num_channels, order, ltm_order, num_samples, max_blocks, want_residuals=True):
        Cn, O, L = num_channels, order + 1, max(ltm_order, 1)
        z = lambda shape, dt: np.zeros(shape, dtype=dt)
        self.blk_start = z(max_blocks, np.uint32)
        self.blk_nsmpl = z(max_blocks, np.uint32)
        self.blk_type = z(max_blocks, np.uint32)
        self.blk_bytes = z(max_blocks, np.uint32)
        self.parcor = z((max_blocks, Cn, O), np.float64)
        self.code = z((max_blocks, Cn, O), np.int32)
        self.kint = z((max_blocks, Cn, O), np.int32)
        self.rshift = z((max_blocks, Cn), np.uint32)
        self.pitch = z((max_blocks, Cn), np.uint32)
        self.ltm_coef = z((max_blocks, Cn, L), np.int32)
        self.rice_init = z((max_blocks, Cn), np.uint32)
        # 1 = parcor[] are the reference's doubles bit for bit, 0 = certified route (codes / decisions are the reference's)
        self.parcor_exact = z((max_blocks, Cn), np.uint32)
        ns = max(num_samples, 1)
        self.res_lattice = z((Cn, ns), np.int32) if want_residuals else None
        self.res_final = z((Cn, ns), np.int32) if want_residuals else None
        p = lambda a, t: a.ctypes.data_as(t)
        self.c = HipTrace(
            max_blocks, O, L, ns, 0, 0,
            p(self.blk_start, u32p), p(self.blk_nsmpl, u32p), p(self.blk_type, u32p), p(self.blk_bytes, u32p),
            p(self.parcor, f64p), p(self.code, i32p), p(self.kint, i32p), p(self.rshift, u32p),
            p(self.pitch, u32p), p(self.ltm_coef, i32p), p(self.rice_init, u32p),
            p(self.res_lattice, i32p) if want_residuals else None,
            p(self.res_final, i32p) if want_residuals else None,
            p(self.parcor_exact, u32p))

    @property
    def num_blocks(self):
        return int(self.c.num_blocks)

    @property
    def offset_lshift(self):
        return int(self.c.offset_lshift)


class Encoder:
    """Python face of ``struct SLAEncoder`` (reference src/include/public/SLAEncoder.h).

    max_num_block_samples: up to 16384 -- what the reference's tool writes, the default -- or, with long_blocks=True, up to
    65535, the longest block the format's 16-bit field can hold.  Encode parameters above 16384 take the long-block routes
    (include/sla_hip.h: the far-window LPC stage, host planner, exact long-term stage; slower per sample) and the handle's
    FFT and scratch grow with the capacity, which is why the larger capacity is asked for by name, as with Decoder."""

    LONG_BLOCKS_FROM = 16384      # capacities above this need long_blocks=True

    def __init__(self, max_num_channels=8, max_num_block_samples=16384, max_parcor_order=48,
                 max_longterm_order=5, max_lms_order_per_filter=40, long_blocks=False):
        if max_num_block_samples > self.LONG_BLOCKS_FROM and not long_blocks:
            raise RuntimeError("max_num_block_samples %d: capacities above %d (up to the format's 65535) need long_blocks=True"
                               % (max_num_block_samples, self.LONG_BLOCKS_FROM))
        self._lib = lib()
        cfg = SLAEncoderConfig(max_num_channels, max_num_block_samples, max_parcor_order,
                               max_longterm_order, max_lms_order_per_filter, 0)
        self._h = self._lib.SLAEncoder_Create(C.byref(cfg))
        if not self._h:
            raise RuntimeError("SLAEncoder_Create failed: no usable HIP device (libsla_hip has no CPU fallback)")
        dev = C.c_int(0)
        self._lib.hipGetDevice(C.byref(dev))
        self.device_index = dev.value             # the handle's stream lives on the device current at creation
        self.num_channels = 0
        self.order = 0
        self.ltm_order = 0
        self.num_samples = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.SLAEncoder_Destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, where):
        if rc != 0:
            raise SlaError(rc, where)

    def set_option(self, name, value):
        """sla_hip_encoder_set_option: layout knobs and route switches of this handle (include/sla_hip.h)"""
        self._check(self._lib.sla_hip_encoder_set_option(self._h, name.encode(), float(value)), "sla_hip_encoder_set_option(%s)" % name)

    def set_wave_format(self, num_channels, bit_per_sample, sampling_rate, offset_lshift=0):
        wf = SLAWaveFormat(num_channels, bit_per_sample, sampling_rate, offset_lshift)
        self._check(self._lib.SLAEncoder_SetWaveFormat(self._h, C.byref(wf)), "SLAEncoder_SetWaveFormat")
        self.num_channels = num_channels

    def set_encode_parameter(self, parcor_order, longterm_order, lms_order_per_filter,
                             ch_process_method=CH_NONE, window_function_type=WINDOW_SIN,
                             max_num_block_samples=4096):
        ep = SLAEncodeParameter(parcor_order, longterm_order, lms_order_per_filter, ch_process_method,
                                window_function_type, max_num_block_samples)
        self._check(self._lib.SLAEncoder_SetEncodeParameter(self._h, C.byref(ep)), "SLAEncoder_SetEncodeParameter")
        self.order, self.ltm_order = parcor_order, longterm_order

    @staticmethod
    def _planes(pcm):
        pcm = np.ascontiguousarray(pcm, np.int32)
        ptrs = (i32p * pcm.shape[0])(*[pcm[c].ctypes.data_as(i32p) for c in range(pcm.shape[0])])
        return pcm, ptrs

    def encode_whole(self, pcm, capacity=None, out=None):
        """planar left-justified int32 [C][N] on the host -> .sla bytes.  `out`: optional preallocated
        uint8 array to encode into (a view of it is returned instead of a bytes copy)"""
        pcm, ptrs = self._planes(pcm)
        n = pcm.shape[1]
        if out is None:
            cap = capacity if capacity is not None else 8 * pcm.shape[0] * n + 65536
            buf = np.zeros(cap, np.uint8)
        else:
            buf, cap = out, min(len(out), 0xFFFFFFF0)        # the API's sizes are 32-bit
        size = C.c_uint32(0)
        self._check(self._lib.SLAEncoder_EncodeWhole(self._h, ptrs, n, buf.ctypes.data_as(u8p), cap, C.byref(size)),
                    "SLAEncoder_EncodeWhole")
        self.num_samples = n
        return buf[:size.value] if out is not None else buf[:size.value].tobytes()

    def encode_batch(self, pcms, capacities=None, outs=None):
        """many files in one pass (sla_hip_encode_batch): list of planar int32 [C][n_i] -> list of (result, bytes).
        `outs`: optional preallocated uint8 arrays, one per file (views of them are returned instead of copies)"""
        keep, items = [], (BatchItem * len(pcms))()
        for i, pcm in enumerate(pcms):
            pcm, ptrs = self._planes(pcm)
            if outs is not None:
                buf, cap = outs[i], len(outs[i])
            else:
                cap = capacities[i] if capacities is not None else 8 * pcm.shape[0] * pcm.shape[1] + 65536
                buf = np.empty(cap, np.uint8)
            keep.append((pcm, ptrs, buf))
            items[i].input = ptrs
            items[i].num_samples = pcm.shape[1]
            items[i].data = buf.ctypes.data_as(u8p)
            items[i].data_size = cap
        self._check(self._lib.sla_hip_encode_batch(self._h, items, len(pcms)), "sla_hip_encode_batch")
        if outs is not None:
            return [(int(items[i].result), keep[i][2][:items[i].output_size]) for i in range(len(pcms))]
        return [(int(items[i].result), keep[i][2][:items[i].output_size].tobytes()) for i in range(len(pcms))]

    def encode_batch_from(self, srcs, sample_format, capacities=None, outs=None, stream=None):
        """many files whose PCM already lives in device tensors -> .sla bytes (sla_hip_encode_batch_device); returns
        [(result code, bytes)], each what encode_batch gives for the left-justified words the format's conversion makes
        (include/sla_hip.h).  srcs[i] is a 2-D torch tensor [channel][sample] on the handle's device with at least as many
        rows as the handle has channels; its strides become the item's (an interleaved [n][C] buffer is passed as its
        transpose .T), its length is the file's.  Its dtype must match sample_format: int32 for PCM_S32_LEFT and PCM_S32,
        int16 for PCM_S16, float32 for PCM_F32.  capacities / outs as in encode_batch.  stream: a torch.cuda.Stream, default
        the current one; the call is synchronous and never writes the tensors."""
        import torch
        if sample_format not in Decoder._FORMAT_DTYPE:
            raise ValueError("unknown sample format %r" % (sample_format,))
        if outs is not None and len(outs) != len(srcs):
            raise ValueError("%d outputs for %d files" % (len(outs), len(srcs)))
        items = self._device_items(srcs, sample_format)
        bufs = []
        for i, x in enumerate(srcs):
            n = x.shape[1]
            if outs is not None:
                buf, cap = outs[i], min(len(outs[i]), 0xFFFFFFFF)
            else:
                cap = capacities[i] if capacities is not None else 8 * self.num_channels * n + 65536
                buf = np.empty(cap, np.uint8)
            bufs.append(buf)
            items[i].data = buf.ctypes.data_as(u8p)
            items[i].data_size = cap
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        self._check(self._lib.sla_hip_encode_batch_device(self._h, items, len(srcs), sample_format, C.c_void_p(st.cuda_stream)),
                    "sla_hip_encode_batch_device")
        if outs is not None:
            return [(int(items[i].result), bufs[i][:items[i].output_size]) for i in range(len(srcs))]
        return [(int(items[i].result), bufs[i][:items[i].output_size].tobytes()) for i in range(len(srcs))]

    def _device_items(self, srcs, sample_format):
        """the source side of an EncodeDeviceItem array for 2-D device tensors [channel][sample] (encode_batch_from)"""
        import torch
        if sample_format not in Decoder._FORMAT_DTYPE:
            raise ValueError("unknown sample format %r" % (sample_format,))
        want = getattr(torch, Decoder._FORMAT_DTYPE[sample_format])
        items = (EncodeDeviceItem * len(srcs))()
        for i, x in enumerate(srcs):
            if not isinstance(x, torch.Tensor) or x.dim() != 2:
                raise ValueError("source %d: need a 2-D torch tensor [channel][sample]" % i)
            if x.dtype != want:
                raise ValueError("source %d: dtype %s, the format wants %s" % (i, x.dtype, want))
            if x.device.type != "cuda" or x.device.index != self.device_index:
                raise ValueError("source %d: on %s, the encoder's device is cuda:%d" % (i, x.device, self.device_index))
            if x.shape[0] < self.num_channels:
                raise ValueError("source %d: %d rows for %d channels" % (i, x.shape[0], self.num_channels))
            n = x.shape[1]
            if n > 0xFFFFFFFF or min(x.stride()) < 0:
                raise ValueError("source %d: unsupported shape %s / strides %s" % (i, tuple(x.shape), x.stride()))
            cs, ss = x.stride(0), x.stride(1)
            if n <= 1:                                  # strides that are never stepped along: any valid value
                ss = max(ss, 1)
                cs = max(cs, 1) if n == 0 else cs
            items[i].src = x.data_ptr() or None
            items[i].channel_stride = cs
            items[i].sample_stride = ss
            items[i].num_samples = n
        return items

    def encode_resident_from(self, srcs, sample_format, outs=None, arena=None, stream=None):
        """encode_batch_from with the .sla bytes delivered to device memory (sla_hip_encode_batch_resident): no byte of a
        file crosses the bus.  srcs, sample_format and stream as for encode_batch_from.  Exactly one of outs and arena:
        outs is a list of 1-D contiguous uint8 CUDA tensors, one per file (slices of a bigger tensor at any offset are
        fine), arena one such tensor in which the library places the delivered files back to back in delivery order
        (include/sla_hip.h).  Returns [(result code, uint8 tensor view of the file's bytes)], each what encode_batch_from
        gives with a host buffer of the same room; where nothing was delivered the view is empty."""
        import torch
        if (outs is None) == (arena is None):
            raise ValueError("exactly one of outs and arena")
        for i, t in enumerate(outs if outs is not None else [arena]):
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.uint8 or not t.is_contiguous() \
                    or t.device.type != "cuda" or t.device.index != self.device_index:
                raise ValueError("%s: need a 1-D contiguous uint8 tensor on cuda:%d"
                                 % ("arena" if outs is None else "output %d" % i, self.device_index))
        if outs is not None and len(outs) != len(srcs):
            raise ValueError("%d outputs for %d files" % (len(outs), len(srcs)))
        items = self._device_items(srcs, sample_format)
        if outs is not None:
            for i, t in enumerate(outs):
                items[i].data = C.cast(C.c_void_p(t.data_ptr() or None), u8p)
                items[i].data_size = min(t.numel(), 0xFFFFFFFF)
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        self._check(self._lib.sla_hip_encode_batch_resident(self._h, items, len(srcs), sample_format,
                                                            C.c_void_p(arena.data_ptr() or None) if arena is not None else None,
                                                            arena.numel() if arena is not None else 0, C.c_void_p(st.cuda_stream)),
                    "sla_hip_encode_batch_resident")
        got = []
        for i in range(len(srcs)):
            size = int(items[i].output_size)
            if outs is not None:
                view = outs[i][:size]
            else:
                off = (C.cast(items[i].data, C.c_void_p).value or arena.data_ptr()) - arena.data_ptr()
                view = arena[off:off + size]
            got.append((int(items[i].result), view))
        return got

    def encode_wav_batch(self, wavs, capacities=None):
        """many WAV files (bytes-like, host memory) -> [(result code, .sla bytes)] (sla_hip_encode_wav_batch): the data
        chunks cross the bus as they are, unpacking and de-interleaving run on the device.  Each file is what encode_batch
        on a handle of the file's wave format gives for its samples; files of different formats may share a call.  The
        default capacity is encode_batch's rule, 8 * C * n + 65536, from the file's own header."""
        n = len(wavs)
        items, keep = (WavItem * max(n, 1))(), []
        for i, w in enumerate(wavs):
            src = np.frombuffer(w, np.uint8)
            if capacities is not None:
                cap = capacities[i]
            else:
                rc, info = wav_info(w)
                cap = 8 * info.num_channels * info.num_samples + 65536
            buf = np.empty(min(cap, 0xFFFFFFFF), np.uint8)
            keep.append((src, buf))
            items[i].src = src.ctypes.data if len(src) else None
            items[i].src_size = len(src)
            items[i].dst = buf.ctypes.data
            items[i].dst_capacity = len(buf)
        self._check(self._lib.sla_hip_encode_wav_batch(self._h, items, n), "sla_hip_encode_wav_batch")
        return [(int(items[i].result), keep[i][1][:items[i].output_size].tobytes()) for i in range(n)]

    def encode_wav_resident(self, srcs, outs=None, arena=None, stream=None):
        """encode_wav_batch for WAV files whose bytes are in device memory, the .sla bytes delivered to device memory
        (sla_hip_encode_wav_batch_resident).  srcs[i] is a 1-D contiguous uint8 CUDA tensor (a slice at any offset is
        fine) or a (device pointer, bytes) pair; exactly one of outs and arena, as for encode_resident_from.  Returns
        [(result code, uint8 tensor view of the file's bytes)]; where nothing was delivered the view is empty."""
        import torch
        if (outs is None) == (arena is None):
            raise ValueError("exactly one of outs and arena")
        ps = Decoder._resident_sources(srcs)
        n = len(ps)
        if outs is not None and len(outs) != n:
            raise ValueError("%d outputs for %d files" % (len(outs), n))
        items = (WavItem * max(n, 1))()
        for i, (ptr, size) in enumerate(ps):
            items[i].src = ptr or None
            items[i].src_size = size
            if outs is not None:
                items[i].dst = outs[i].data_ptr() or None
                items[i].dst_capacity = min(outs[i].numel(), 0xFFFFFFFF)
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        self._check(self._lib.sla_hip_encode_wav_batch_resident(self._h, items, n,
                                                                C.c_void_p(arena.data_ptr() or None) if arena is not None else None,
                                                                arena.numel() if arena is not None else 0, C.c_void_p(st.cuda_stream)),
                    "sla_hip_encode_wav_batch_resident")
        got = []
        for i in range(n):
            size = int(items[i].output_size)
            if outs is not None:
                view = outs[i][:size]
            else:
                off = (items[i].dst or arena.data_ptr()) - arena.data_ptr()
                view = arena[off:off + size]
            got.append((int(items[i].result), view))
        return got

    def encode_batch_tensor(self, x, lengths=None, layout="planar", right_justify=False):
        """a padded batch in one device tensor -> .sla bytes, the mirror of Decoder.decode_batch_tensor: x is [B][C][L]
        (planar) or [B][L][C] (interleaved) on the handle's device, file b its first lengths[b] <= L samples (default L).
        The dtype picks the format: float32 -> PCM_F32, int16 -> PCM_S16, int32 -> PCM_S32_LEFT, or PCM_S32 with
        right_justify.  Returns encode_batch_from's [(result code, bytes)];
        enc.encode_batch_tensor(*dec.decode_batch_tensor(datas)[:2]) gives the files back."""
        srcs, fmt = self._tensor_sources(x, lengths, layout, right_justify)
        return self.encode_batch_from(srcs, fmt)

    @staticmethod
    def _tensor_sources(x, lengths, layout, right_justify):
        """(the per-file 2-D views, the sample format) of encode_batch_tensor's arguments"""
        import torch
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError("need a 3-D torch tensor [B][C][L] or [B][L][C]")
        if x.dtype == torch.float32:
            fmt = PCM_F32
        elif x.dtype == torch.int16:
            fmt = PCM_S16
        elif x.dtype == torch.int32:
            fmt = PCM_S32 if right_justify else PCM_S32_LEFT
        else:
            raise ValueError("dtype must be float32, int16 or int32, not %s" % (x.dtype,))
        if layout not in ("planar", "interleaved"):
            raise ValueError("layout must be 'planar' or 'interleaved', not %r" % (layout,))
        B, L = x.shape[0], (x.shape[2] if layout == "planar" else x.shape[1])
        lengths = [L] * B if lengths is None else [int(n) for n in lengths]
        if len(lengths) != B or any(n < 0 or n > L for n in lengths):
            raise ValueError("need %d lengths in [0, %d]" % (B, L))
        return [(x[b] if layout == "planar" else x[b].t())[:, :lengths[b]] for b in range(B)], fmt

    def encode_resident_tensor(self, x, lengths=None, layout="planar", right_justify=False, capacity=None):
        """encode_batch_tensor with the files left in device memory, the mirror of Decoder.decode_resident_tensor: one uint8
        arena of `capacity` bytes (default: the sum of 4 * C * n + 65536 over the files) is allocated on the handle's
        device and the files are placed in it back to back.  Returns (arena[:used], offsets, sizes, results), offsets and
        sizes Python lists (0 and 0 where nothing was delivered);
        dec.decode_resident_tensor([a[o:o + s] for o, s in zip(offsets, sizes)]) gives x back."""
        import torch
        srcs, fmt = self._tensor_sources(x, lengths, layout, right_justify)
        if capacity is None:
            capacity = sum(4 * self.num_channels * s.shape[1] + 65536 for s in srcs)
        arena = torch.empty(max(int(capacity), 1), dtype=torch.uint8, device=torch.device("cuda", self.device_index))
        got = self.encode_resident_from(srcs, fmt, arena=arena[:int(capacity)])
        base = arena.data_ptr()
        sizes = [int(v.numel()) for _, v in got]
        offsets = [(v.data_ptr() - base) if n > 0 else 0 for (_, v), n in zip(got, sizes)]
        used = max([o + n for o, n in zip(offsets, sizes)], default=0)
        return arena[:used], offsets, sizes, [rc for rc, _ in got]

    def encode_block(self, pcm, capacity=None):
        pcm, ptrs = self._planes(pcm)
        n = pcm.shape[1]
        cap = capacity if capacity is not None else 8 * pcm.shape[0] * n + 4096
        out = np.zeros(cap, np.uint8)
        size = C.c_uint32(0)
        self._check(self._lib.SLAEncoder_EncodeBlock(self._h, ptrs, n, out.ctypes.data_as(u8p), cap, C.byref(size)),
                    "SLAEncoder_EncodeBlock")
        self.num_samples = n
        return out[:size.value].tobytes()

    def analyze_device(self, device_ptr, plane_stride, num_samples, stream=None):
        """hot path on PCM already resident in HBM; returns the 12 stage timings [ms]"""
        timing = (C.c_float * 12)()
        self._check(self._lib.sla_hip_analyze_device(self._h, C.c_void_p(device_ptr), plane_stride, num_samples,
                                                     C.c_void_p(stream) if stream else None, timing),
                    "sla_hip_analyze_device")
        self.num_samples = num_samples
        return list(timing)

    def analyze_batch_device(self, device_ptr, plane_stride, span, starts, lens):
        """hot path on a batch of files resident in HBM (files at starts[i], multiples of 1024); returns
        (the 12 stage timings [ms], offset_lshift per file)"""
        st = np.ascontiguousarray(starts, np.uint32)
        ln = np.ascontiguousarray(lens, np.uint32)
        lsh = np.zeros(len(st), np.uint32)
        timing = (C.c_float * 12)()
        self._check(self._lib.sla_hip_analyze_batch_device(self._h, C.c_void_p(device_ptr), plane_stride, span,
                                                           st.ctypes.data_as(u32p), ln.ctypes.data_as(u32p), len(st),
                                                           lsh.ctypes.data_as(u32p), timing), "sla_hip_analyze_batch_device")
        self.num_samples = span
        return list(timing), lsh

    def shard_scan(self, device_ptr, plane_stride, num_samples):
        """sla_hip_shard_scan: (OR of every sample word, 1-bit 'not silent' mask as uint64 words) of a piece of a file"""
        orw = C.c_uint32(0)
        mask = np.zeros((num_samples + 63) // 64, np.uint64)
        self._check(self._lib.sla_hip_shard_scan(self._h, C.c_void_p(device_ptr), plane_stride, num_samples, C.byref(orw),
                                                 mask.ctypes.data_as(C.POINTER(C.c_uint64))), "sla_hip_shard_scan")
        return int(orw.value), mask

    def shard_scan_counts(self, device_ptr, plane_stride, num_samples):
        """sla_hip_shard_scan_counts: (OR of every sample word, number of all-zero 64-sample mask words) of a piece"""
        orw, zw = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.sla_hip_shard_scan_counts(self._h, C.c_void_p(device_ptr), plane_stride, num_samples,
                                                        C.byref(orw), C.byref(zw)), "sla_hip_shard_scan_counts")
        return int(orw.value), int(zw.value)

    def shard_analyze(self, device_ptr, plane_stride, num_samples, file_or_word, no_silence=False):
        """sla_hip_shard_analyze: the hot path on a range of a longer file whose OR word is `file_or_word`
        (no_silence: sla_hip_shard_analyze_no_silence -- the file's scan counted no all-zero mask word)"""
        timing = (C.c_float * 12)()
        fn = self._lib.sla_hip_shard_analyze_no_silence if (no_silence and file_or_word != 0) else self._lib.sla_hip_shard_analyze
        self._check(fn(self._h, C.c_void_p(device_ptr), plane_stride, num_samples,
                       C.c_uint32(file_or_word), timing), "sla_hip_shard_analyze")
        self.num_samples = num_samples
        return list(timing)

    def last_timing(self):
        """the 12 stage timings / counters of the last analysis (see include/sla_hip.h)"""
        timing = (C.c_float * 12)()
        self._check(self._lib.sla_hip_last_timing(self._h, timing), "sla_hip_last_timing")
        return list(timing)

    def last_kernel_ms(self):
        """on-device execution time [ms] of (k_lpc_blocks, k_lattice, k_ltm_acf, k_tail) in the last analysis"""
        k = (C.c_float * 4)()
        self._check(self._lib.sla_hip_last_kernel_ms(self._h, k), "sla_hip_last_kernel_ms")
        return list(k)

    def last_counters(self):
        """(search groups rerun as chains, super-frames planned on the host, exact search used, device plan enabled,
        k_tail launches, long-term solve on the device)"""
        c = (C.c_uint32 * 6)()
        self._check(self._lib.sla_hip_last_counters(self._h, c), "sla_hip_last_counters")
        return tuple(c)

    def last_expand(self):
        """(pipeline chunks whose block stage was launched from device-written tables, pipeline chunks, analyses of this
        handle served from kept search tables, searches launched on a wrong guess of the prepass result)"""
        c = (C.c_uint32 * 4)()
        self._check(self._lib.sla_hip_last_expand(self._h, c), "sla_hip_last_expand")
        return tuple(c)

    def last_block_cert(self):
        """(1 if the block stage took the certified route, (block, channel) pairs redone by the exact kernels)"""
        c = (C.c_uint32 * 2)()
        self._check(self._lib.sla_hip_last_block_cert(self._h, c), "sla_hip_last_block_cert")
        return tuple(c)

    def last_cert_audit(self):
        """option cert_audit: (certified pairs the exact kernels re-analysed and found equal, pairs they found different)"""
        c = (C.c_uint32 * 2)()
        self._check(self._lib.sla_hip_last_cert_audit(self._h, c), "sla_hip_last_cert_audit")
        return tuple(c)

    def last_ltm_cert(self):
        """certified long-term stage (option ltm_cert) in the last analysis: (jobs, certified, fallback, audit_ok, audit_bad)"""
        c = (C.c_uint32 * 5)()
        self._check(self._lib.sla_hip_last_ltm_cert(self._h, c), "sla_hip_last_ltm_cert")
        return tuple(c)

    def last_silence(self):
        """option "silence_runs": (route of the last analysis or batch call -- 0: nothing silent, no mask needed; 1: tables
        from the device's run list; 2: the mask was downloaded --, zero runs the device found, capacity of the list, mask
        bytes downloaded beyond the fixed tail words); a batch's passes and worker lanes are summed (the route: the maximum)"""
        c = (C.c_uint32 * 4)()
        self._check(self._lib.sla_hip_last_silence(self._h, c), "sla_hip_last_silence")
        return tuple(c)

    def last_search_early(self):
        """option "search_early": (1 if the last analysis started its search beside the prepass; analyses of this handle
        that did; those among them whose start was cancelled and whose search went out again; 0)"""
        c = (C.c_uint32 * 4)()
        self._check(self._lib.sla_hip_last_search_early(self._h, c), "sla_hip_last_search_early")
        return tuple(c)

    def last_verify(self):
        """option "verify": (sample-channels compared, sample-channels that differed, first differing position
        (sample << 3 | channel, or 2^64 - 1 when none), blocks decoded, bad blocks) of the last call that packed on the
        device; all zero when it did not verify (include/sla_hip.h)"""
        c = (C.c_uint64 * 5)()
        self._check(self._lib.sla_hip_last_verify(self._h, c), "sla_hip_last_verify")
        return tuple(int(v) for v in c)

    def verify_last_image(self, device_ptr, plane_stride):
        """sla_hip_verify_last_image: decode the image the last pack(on_device=True) / non-streamed encode_whole left on the
        device and compare it with the planes at device_ptr (planar left-justified int32 [C][plane_stride]); returns the
        five counters of last_verify.  Raises SlaError PARAMETER_NOT_SET when the handle holds no such image."""
        c = (C.c_uint64 * 5)()
        self._check(self._lib.sla_hip_verify_last_image(self._h, C.c_void_p(device_ptr), plane_stride, c),
                    "sla_hip_verify_last_image")
        return tuple(int(v) for v in c)

    def bind_residual_planes(self, lattice_ptr, final_ptr, plane_stride):
        self._check(self._lib.sla_hip_bind_residual_planes(self._h, C.c_void_p(lattice_ptr), C.c_void_p(final_ptr),
                                                           plane_stride), "sla_hip_bind_residual_planes")

    def pack(self, capacity, on_device=False):
        """bit-pack the analysed file: host threads (sla_hip_pack) or device kernels (sla_hip_pack_device)"""
        out = np.zeros(capacity, np.uint8)
        size = C.c_uint32(0)
        fn = self._lib.sla_hip_pack_device if on_device else self._lib.sla_hip_pack
        self._check(fn(self._h, out.ctypes.data_as(u8p), capacity, C.byref(size)), "sla_hip_pack")
        return out[:size.value].tobytes()

    def pack_resident(self, out):
        """sla_hip_pack_resident: pack(on_device=True) of the analysed file into `out`, a 1-D contiguous uint8 CUDA tensor
        on the handle's device (a slice at any offset is fine); returns the view of `out` that holds the file"""
        import torch
        if not isinstance(out, torch.Tensor) or out.dim() != 1 or out.dtype != torch.uint8 or not out.is_contiguous() \
                or out.device.type != "cuda" or out.device.index != self.device_index:
            raise ValueError("need a 1-D contiguous uint8 tensor on cuda:%d" % self.device_index)
        size = C.c_uint32(0)
        self._check(self._lib.sla_hip_pack_resident(self._h, C.c_void_p(out.data_ptr() or None), min(out.numel(), 0xFFFFFFFF),
                                                    C.byref(size)), "sla_hip_pack_resident")
        return out[:size.value]

    def trace(self, want_residuals=True, max_blocks=None):
        tr = Trace(self.num_channels, self.order, self.ltm_order, self.num_samples,
                   max_blocks if max_blocks is not None else self.num_samples // 1024 + 8, want_residuals)
        self._check(self._lib.sla_hip_get_trace(self._h, C.byref(tr.c)), "sla_hip_get_trace")
        return tr

    def final_residual_ptr(self):
        stride = C.c_uint64(0)
        return self._lib.sla_hip_final_residual(self._h, C.byref(stride)), stride.value


def shard_bounds(num_samples, max_num_block_samples, nz_mask, world):
    """sla_hip_shard_bounds: [bounds[r], bounds[r+1]) = the samples rank r of `world` encodes, every bound a super-frame
    start of the whole file's hop over silence runs.  Pure host arithmetic of the library (no GPU needed)."""
    bounds = np.zeros(world + 1, np.uint32)
    if nz_mask is None:            # no rank counted an all-zero mask word (shard_scan_counts): nothing is silent
        ptr = None
    else:
        mask = np.ascontiguousarray(nz_mask, np.uint64)
        if len(mask) < (num_samples + 63) // 64:
            raise ValueError("mask too short")
        ptr = mask.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = lib().sla_hip_shard_bounds(C.c_uint32(num_samples), C.c_uint32(max_num_block_samples),
                                    ptr, C.c_uint32(world), bounds.ctypes.data_as(u32p))
    if rc != 0:
        raise SlaError(rc, "sla_hip_shard_bounds")
    return [int(b) for b in bounds]


def shard_join(shard_images):
    """the per-rank .sla images (43-byte header + blocks each, in rank order) -> the file: sla_hip_shard_header over
    the shards' headers, then the blocks back to back"""
    shard_images = [img for img in shard_images if len(img) != 0]        # a rank without super-frames contributes nothing
    if not shard_images:
        raise ValueError("no shard produced an image")
    heads = [np.frombuffer(bytes(img[:43]), np.uint8).copy() for img in shard_images]
    if any(len(h) != 43 for h in heads):
        raise ValueError("shard image shorter than a header")
    ptrs = (u8p * len(heads))(*[h.ctypes.data_as(u8p) for h in heads])
    out = np.zeros(43, np.uint8)
    rc = lib().sla_hip_shard_header(ptrs, len(heads), out.ctypes.data_as(u8p), 43)
    if rc != 0:
        raise SlaError(rc, "sla_hip_shard_header")
    return out.tobytes() + b"".join(bytes(img[43:]) for img in shard_images)


INDEX_BLOCK_DTYPE = np.dtype([("byte_off", "<u4"), ("byte_len", "<u4"), ("smp_off", "<u4"), ("num_samples", "<u4")])


class Index:
    """the block index of one .sla stream (sla_hip_index, include/sla_hip.h): host memory, immutable.  Index.build(data)
    walks host bytes, Decoder.index_resident device bytes; to_bytes / from_bytes are the sidecar format."""

    def __init__(self, handle):
        self._lib = lib()
        self._h = handle
        info = IndexSummary()
        rc = self._lib.sla_hip_index_info(self._h, C.byref(info))
        if rc != 0:
            raise SlaError(rc, "sla_hip_index_info")
        self._info = info

    @classmethod
    def build(cls, data):
        """the index of a whole .sla stream in a bytes-like object (sla_hip_index_build: pure host code)"""
        buf = np.frombuffer(bytes(data), np.uint8)
        h = C.c_void_p()
        rc = lib().sla_hip_index_build(buf.ctypes.data if len(buf) else C.cast(C.create_string_buffer(1), C.c_void_p), len(buf),
                                       C.byref(h))
        if rc != 0:
            raise SlaError(rc, "sla_hip_index_build")
        return cls(h)

    @classmethod
    def from_bytes(cls, blob):
        """an index from to_bytes' blob (sla_hip_index_deserialize); SlaError INVALID_ARGUMENT for one it refuses"""
        buf = np.frombuffer(bytes(blob), np.uint8)
        h = C.c_void_p()
        rc = lib().sla_hip_index_deserialize(buf.ctypes.data if len(buf) else C.cast(C.create_string_buffer(1), C.c_void_p),
                                             len(buf), C.byref(h))
        if rc != 0:
            raise SlaError(rc, "sla_hip_index_deserialize")
        return cls(h)

    def to_bytes(self):
        n = int(self._lib.sla_hip_index_serialized_bytes(self._h))
        out = np.zeros(n, np.uint8)
        if int(self._lib.sla_hip_index_serialize(self._h, out.ctypes.data, n)) != n:
            raise SlaError(1, "sla_hip_index_serialize")
        return out.tobytes()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sla_hip_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def data_size(self):
        return int(self._info.data_size)

    @property
    def header(self):
        """the SLAHeaderInfo DecodeHeader delivered, None when it delivered none"""
        return self._info.header if self._info.header_result in (0, 11) else None

    @property
    def header_result(self):
        return int(self._info.header_result)

    @property
    def stop(self):
        return int(self._info.stop)

    @property
    def extent(self):
        return int(self._info.extent)

    @property
    def num_blocks(self):
        return int(self._info.num_blocks)

    def blocks(self, first=0, count=None):
        """rows [first, first + count) as a structured numpy array (INDEX_BLOCK_DTYPE)"""
        count = self.num_blocks - first if count is None else count
        out = np.zeros(max(count, 0), INDEX_BLOCK_DTYPE)
        rc = self._lib.sla_hip_index_blocks(self._h, first, count, out.ctypes.data if count > 0 else None)
        if rc != 0:
            raise SlaError(rc, "sla_hip_index_blocks")
        return out


WIDE_WALK_DEFAULT = 16000000     # the handle option "wide_walk" as SLADecoder_Create sets it (sla_decoder.c: DEC_WIDE_WALK_DEFAULT)


class Decoder:
    """Python face of ``struct SLADecoder`` (reference src/include/public/SLADecoder.h).

    max_num_block_samples: up to 16384 -- what the encoder and the reference's tool write, the default -- or, with
    long_blocks=True, up to 65535, the longest block the format's 16-bit field can hold (the reference's library writes such
    blocks when asked).  Every route decodes them; above 40896 the long-term synthesis of ALL blocks of the handle slides
    through a ring of LDS (sla_hip_launch_dec_ltm) instead of holding the block there whole, and the streaming buffers
    grow with the capacity, which is why the larger capacity is asked for by name: without long_blocks a capacity above
    16384 is refused as it always was."""

    LONG_BLOCKS_FROM = 16384      # capacities above this need long_blocks=True

    def __init__(self, max_num_channels=8, max_num_block_samples=16384, max_parcor_order=48,
                 max_longterm_order=5, max_lms_order_per_filter=32, enable_crc_check=1, long_blocks=False):
        if max_num_block_samples > self.LONG_BLOCKS_FROM and not long_blocks:
            raise RuntimeError("max_num_block_samples %d: capacities above %d (up to the format's 65535) need long_blocks=True"
                               % (max_num_block_samples, self.LONG_BLOCKS_FROM))
        self._lib = lib()
        cfg = SLADecoderConfig(max_num_channels, max_num_block_samples, max_parcor_order,
                               max_longterm_order, max_lms_order_per_filter, enable_crc_check, 0)
        self._h = self._lib.SLADecoder_Create(C.byref(cfg))
        if not self._h:
            raise RuntimeError("SLADecoder_Create failed: no usable HIP device or unsupported capacity "
                               "(libsla_hip has no CPU fallback)")
        dev = C.c_int(0)
        self._lib.hipGetDevice(C.byref(dev))
        self.device_index = dev.value             # the handle's stream lives on the device current at creation
        self.max_num_block_samples = max_num_block_samples
        self._wide_walk, self._wide_nodes, self._index_walk = WIDE_WALK_DEFAULT, 0, None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.SLADecoder_Destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_whole(self, data, capacity, num_channels=None):
        """.sla bytes -> (result code, planar left-justified int32 [C][n]); like the reference, samples of the
        blocks before a failing one are returned together with the error code"""
        buf = np.frombuffer(bytes(data), np.uint8)
        nch = num_channels if num_channels is not None else (int(buf[14]) if len(buf) > 14 else 1)
        out = np.zeros((max(nch, 1), max(capacity, 1)), np.int32)
        ptrs = (i32p * out.shape[0])(*[out[c].ctypes.data_as(i32p) for c in range(out.shape[0])])
        n = C.c_uint32(0)
        rc = self._lib.SLADecoder_DecodeWhole(self._h, buf.ctypes.data_as(u8p), len(buf), ptrs, capacity, C.byref(n))
        return rc, out[:, :n.value]

    def decode_batch(self, datas, capacities=None, outs=None):
        """many .sla files in one call (sla_hip_decode_batch) -> list of (result code, planar left-justified int32
        [C][n]), each exactly what decode_whole of that file alone returns.  The channel count comes from each header,
        the default capacity is its num_samples.  `outs`: optional preallocated int32 arrays [>= C][>= capacity], one
        per file (views of them are returned)"""
        items = (DecodeItem * len(datas))()
        keep = []
        for i, data in enumerate(datas):
            buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
            nch = int(buf[14]) if len(buf) > 14 else 1
            if capacities is not None:
                cap = int(capacities[i])
            else:
                cap = int.from_bytes(bytes(buf[15:19]), "big") if len(buf) >= 19 else 0
            out = outs[i] if outs is not None else np.empty((max(nch, 1), max(cap, 1)), np.int32)
            if out.shape[0] < nch or out.shape[1] < cap or out.dtype != np.int32 or not out[0].flags.c_contiguous:
                raise ValueError("output %d: need int32 rows of at least [%d][%d]" % (i, nch, cap))
            ptrs = (i32p * out.shape[0])(*[out[c].ctypes.data_as(i32p) for c in range(out.shape[0])])
            keep.append((buf, out, ptrs))
            items[i].data = buf.ctypes.data_as(u8p)
            items[i].data_size = len(buf)
            items[i].buffer_num_samples = cap
            items[i].buffer = ptrs
        self._check(self._lib.sla_hip_decode_batch(self._h, items, len(datas)), "sla_hip_decode_batch")
        return [(int(items[i].result), keep[i][1][:, :items[i].output_num_samples]) for i in range(len(datas))]

    def _check(self, rc, where):
        if rc != 0:
            raise SlaError(rc, where)

    _FORMAT_DTYPE = {PCM_S32_LEFT: "int32", PCM_S32: "int32", PCM_S16: "int16", PCM_F32: "float32"}

    def decode_batch_into(self, datas, outs, sample_format, zero_fill=True, stream=None):
        """many .sla files in host memory -> caller-owned device tensors (sla_hip_decode_batch_device); returns
        [(result code, samples)], each what decode_batch gives that file with capacity = the tensor's length.
        outs[i] is a 2-D torch tensor indexed [channel][sample] on the handle's device, with at least as many rows as
        the file's header has channels; its strides become the item's (an interleaved [n][C] buffer is passed as its
        transpose .T), its length is the capacity.  Its dtype must match sample_format: int32 for PCM_S32_LEFT and
        PCM_S32, int16 for PCM_S16, float32 for PCM_F32.  zero_fill: [n, capacity) of every channel is written zero.
        stream: a torch.cuda.Stream, default the current one; the call is synchronous."""
        import torch
        if sample_format not in self._FORMAT_DTYPE:
            raise ValueError("unknown sample format %r" % (sample_format,))
        if len(outs) != len(datas):
            raise ValueError("%d outputs for %d files" % (len(outs), len(datas)))
        want = getattr(torch, self._FORMAT_DTYPE[sample_format])
        items = (DecodeDeviceItem * len(datas))()
        keep = []
        for i, (data, out) in enumerate(zip(datas, outs)):
            buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
            if not isinstance(out, torch.Tensor) or out.dim() != 2:
                raise ValueError("output %d: need a 2-D torch tensor [channel][sample]" % i)
            if out.dtype != want:
                raise ValueError("output %d: dtype %s, the format wants %s" % (i, out.dtype, want))
            if out.device.type != "cuda" or out.device.index != self.device_index:
                raise ValueError("output %d: on %s, the decoder's device is cuda:%d" % (i, out.device, self.device_index))
            rc, h = decode_header(buf[:43])         # the header alone: no copy of the stream
            nch = h.wave_format.num_channels if rc in (0, 11) else 0
            if out.shape[0] < nch:
                raise ValueError("output %d: %d rows for a file of %d channels" % (i, out.shape[0], nch))
            if out.shape[1] > 0xFFFFFFFF or min(out.stride()) < 0 or (out.shape[1] > 1 and out.stride(1) == 0) \
                    or (nch > 1 and out.stride(0) == 0):
                raise ValueError("output %d: unsupported shape %s / strides %s" % (i, tuple(out.shape), out.stride()))
            keep.append(buf)
            items[i].data = buf.ctypes.data_as(u8p)
            items[i].data_size = len(buf)
            items[i].dst = out.data_ptr() or None
            items[i].channel_stride = out.stride(0)
            items[i].sample_stride = max(out.stride(1), 1)
            items[i].capacity = out.shape[1]
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        rc = self._lib.sla_hip_decode_batch_device(self._h, items, len(datas), sample_format,
                                                   DEC_ZERO_FILL if zero_fill else 0, C.c_void_p(st.cuda_stream))
        self._check(rc, "sla_hip_decode_batch_device")
        return [(int(items[i].result), int(items[i].output_num_samples)) for i in range(len(datas))]

    def decode_batch_tensor(self, datas, dtype=None, layout="planar", length=None, right_justify=False):
        """many .sla files -> one padded device tensor on the handle's device: [B][C][L] (planar) or [B][L][C]
        (interleaved), C the largest channel count among the headers, L `length` or the largest header num_samples.
        dtype float32 (default; sample * 2^-31), int16 (left-justified >> 16) or int32 (left-justified, or with
        right_justify the bit_per_sample-bit integer).  Returns (tensor, lengths, results); everything past a file's
        length, rows past its channel count and files that gave nothing are zero."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype == torch.float32:
            fmt = PCM_F32
        elif dtype == torch.int16:
            fmt = PCM_S16
        elif dtype == torch.int32:
            fmt = PCM_S32 if right_justify else PCM_S32_LEFT
        else:
            raise ValueError("dtype must be float32, int16 or int32, not %s" % (dtype,))
        if layout not in ("planar", "interleaved"):
            raise ValueError("layout must be 'planar' or 'interleaved', not %r" % (layout,))
        bufs = [d if isinstance(d, np.ndarray) else np.frombuffer(bytes(d), np.uint8) for d in datas]
        nchs, nsmp = [], []
        for buf in bufs:
            rc, h = decode_header(buf[:43])         # the header alone: no copy of the stream
            given = rc in (0, 11)                      # OK, or a header CRC failure: the fields are delivered
            nchs.append(h.wave_format.num_channels if given else 0)
            nsmp.append(h.num_samples if given else 0)
        B, Cn = len(bufs), max(nchs, default=0)
        L = int(length) if length is not None else max(nsmp, default=0)
        if L < 0 or L > 0xFFFFFFFF:
            raise ValueError("length %d out of range" % L)
        dev = torch.device("cuda", self.device_index)
        shape = (B, Cn, L) if layout == "planar" else (B, L, Cn)
        out = torch.empty(shape, dtype=dtype, device=dev)
        if out.numel() == 0:
            # nothing can be written: a one-element stand-in keeps the per-item pointers valid, the results are real
            scratch = torch.empty(1, dtype=dtype, device=dev)
            outs = [scratch.as_strided((Cn, L), (1, 1)) for _ in range(B)]
        else:
            outs = [out[b] if layout == "planar" else out[b].t() for b in range(B)]
        got = self.decode_batch_into(bufs, outs, fmt, zero_fill=True)
        # the zero fill covers [n, L) of the rows a header gave; what no header covers is zeroed here
        for b in range(B):
            if nchs[b] < Cn:
                if layout == "planar":
                    out[b, nchs[b]:].zero_()
                else:
                    out[b, :, nchs[b]:].zero_()
        return out, [n for _, n in got], [rc for rc, _ in got]

    def decode_wav_batch(self, slas):
        """many .sla streams (bytes-like, host memory) -> [(result code, WAV bytes)] (sla_hip_decode_wav_batch): canonical
        44-byte header and interleaved frames, packed on the device; capacities come from the streams' headers.  A file is
        delivered whole or not at all (empty bytes)."""
        n = len(slas)
        items, keep = (WavItem * max(n, 1))(), []
        for i, dat in enumerate(slas):
            src = np.frombuffer(dat, np.uint8)
            rc, h = decode_header(dat)
            cap = 44
            if rc == 0:
                cap = min(44 + h.num_samples * h.wave_format.num_channels * ((h.wave_format.bit_per_sample + 7) // 8), 0xFFFFFFFF)
            buf = np.empty(cap, np.uint8)
            keep.append((src, buf))
            items[i].src = src.ctypes.data if len(src) else None
            items[i].src_size = len(src)
            items[i].dst = buf.ctypes.data
            items[i].dst_capacity = cap
        self._check(self._lib.sla_hip_decode_wav_batch(self._h, items, n), "sla_hip_decode_wav_batch")
        return [(int(items[i].result), keep[i][1][:items[i].output_size].tobytes()) for i in range(n)]

    def decode_wav_resident(self, srcs, outs=None, stream=None):
        """decode_wav_batch for streams whose bytes are in device memory, the WAV files delivered to device memory
        (sla_hip_decode_wav_batch_resident).  srcs as for decode_resident_into; outs: 1-D contiguous uint8 CUDA tensors
        (slices at any offset are fine), allocated from resident_headers when None.  Returns [(result code, uint8 tensor
        view of the file's bytes)], empty where nothing was delivered."""
        import torch
        ps = self._resident_sources(srcs)
        n = len(ps)
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        if outs is None:
            outs = []
            for rc, h in self.resident_headers(ps, stream=st):
                size = 44 + h.num_samples * h.wave_format.num_channels * ((h.wave_format.bit_per_sample + 7) // 8) if rc == 0 else 44
                outs.append(torch.empty(min(size, 0xFFFFFFFF), dtype=torch.uint8, device="cuda:%d" % self.device_index))
        if len(outs) != n:
            raise ValueError("%d outputs for %d files" % (len(outs), n))
        items = (WavItem * max(n, 1))()
        for i, (ptr, size) in enumerate(ps):
            items[i].src = ptr or None
            items[i].src_size = size
            items[i].dst = outs[i].data_ptr() or None
            items[i].dst_capacity = min(outs[i].numel(), 0xFFFFFFFF)
        self._index_walk = None              # last_walk() speaks of this call from here on
        self._check(self._lib.sla_hip_decode_wav_batch_resident(self._h, items, n, C.c_void_p(st.cuda_stream)),
                    "sla_hip_decode_wav_batch_resident")
        return [(int(items[i].result), outs[i][:items[i].output_size]) for i in range(n)]

    @staticmethod
    def _resident_sources(srcs):
        """[(device pointer, bytes)] of 1-D contiguous uint8 CUDA tensors or (ptr, size) pairs"""
        out = []
        for i, s in enumerate(srcs):
            if isinstance(s, (tuple, list)):
                ptr, size = int(s[0] or 0), int(s[1])
            else:
                if s.dim() != 1 or str(s.dtype) != "torch.uint8" or not s.is_contiguous() or s.device.type != "cuda":
                    raise ValueError("source %d: need a 1-D contiguous uint8 CUDA tensor or a (ptr, size) pair" % i)
                ptr, size = s.data_ptr(), s.numel()
            if size < 0 or size > 0xFFFFFFFF:
                raise ValueError("source %d: %d bytes" % (i, size))
            out.append((ptr, size))
        return out

    def resident_headers(self, srcs, stream=None):
        """[(DecodeHeader's code, SLAHeaderInfo)] of streams that are in device memory (sla_hip_resident_headers); the
        code is INVALID_ARGUMENT for a source the resident decode refuses"""
        import torch
        ps = self._resident_sources(srcs)
        n = len(ps)
        ptrs = (C.c_void_p * max(n, 1))(*[p or None for p, _ in ps])
        sizes = (C.c_uint32 * max(n, 1))(*[s for _, s in ps])
        hdrs = (SLAHeaderInfo * max(n, 1))()
        codes = (C.c_int32 * max(n, 1))()
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        self._check(self._lib.sla_hip_resident_headers(self._h, ptrs, sizes, n, hdrs, codes, C.c_void_p(st.cuda_stream)),
                    "sla_hip_resident_headers")
        return [(int(codes[i]), hdrs[i]) for i in range(n)]

    def decode_resident_into(self, srcs, outs, sample_format, zero_fill=True, stream=None, _headers=None):
        """decode_batch_into for .sla streams whose bytes are in device memory (sla_hip_decode_batch_resident): no host
        copy of the streams, no staging, no upload.  srcs[i] is a 1-D contiguous uint8 CUDA tensor (a slice of a bigger
        one at any offset is fine) or a (device pointer, bytes) pair; outs, sample_format, zero_fill and stream as for
        decode_batch_into.  Returns [(result code, samples)], each what decode_batch_into gives the same bytes."""
        import torch
        if sample_format not in self._FORMAT_DTYPE:
            raise ValueError("unknown sample format %r" % (sample_format,))
        if len(outs) != len(srcs):
            raise ValueError("%d outputs for %d files" % (len(outs), len(srcs)))
        want = getattr(torch, self._FORMAT_DTYPE[sample_format])
        ps = self._resident_sources(srcs)
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        heads = _headers if _headers is not None else self.resident_headers(ps, stream=st)
        items = (DecodeDeviceItem * len(ps))()
        for i, ((ptr, size), out) in enumerate(zip(ps, outs)):
            if not isinstance(out, torch.Tensor) or out.dim() != 2:
                raise ValueError("output %d: need a 2-D torch tensor [channel][sample]" % i)
            if out.dtype != want:
                raise ValueError("output %d: dtype %s, the format wants %s" % (i, out.dtype, want))
            if out.device.type != "cuda" or out.device.index != self.device_index:
                raise ValueError("output %d: on %s, the decoder's device is cuda:%d" % (i, out.device, self.device_index))
            rc, h = heads[i]
            nch = h.wave_format.num_channels if rc in (0, 11) else 0
            if out.shape[0] < nch:
                raise ValueError("output %d: %d rows for a file of %d channels" % (i, out.shape[0], nch))
            if out.shape[1] > 0xFFFFFFFF or min(out.stride()) < 0 or (out.shape[1] > 1 and out.stride(1) == 0) \
                    or (nch > 1 and out.stride(0) == 0):
                raise ValueError("output %d: unsupported shape %s / strides %s" % (i, tuple(out.shape), out.stride()))
            items[i].data = C.cast(C.c_void_p(ptr or None), u8p)
            items[i].data_size = size
            items[i].dst = out.data_ptr() or None
            items[i].channel_stride = out.stride(0)
            items[i].sample_stride = max(out.stride(1), 1)
            items[i].capacity = out.shape[1]
        self._index_walk = None              # last_walk() speaks of this call from here on
        rc = self._lib.sla_hip_decode_batch_resident(self._h, items, len(ps), sample_format,
                                                     DEC_ZERO_FILL if zero_fill else 0, C.c_void_p(st.cuda_stream))
        self._check(rc, "sla_hip_decode_batch_resident")
        return [(int(items[i].result), int(items[i].output_num_samples)) for i in range(len(ps))]

    def decode_resident_tensor(self, srcs, dtype=None, layout="planar", length=None, right_justify=False):
        """decode_batch_tensor for .sla streams whose bytes are in device memory: the same padded tensor, lengths and
        results; the shapes come from the headers sla_hip_resident_headers brings home"""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype == torch.float32:
            fmt = PCM_F32
        elif dtype == torch.int16:
            fmt = PCM_S16
        elif dtype == torch.int32:
            fmt = PCM_S32 if right_justify else PCM_S32_LEFT
        else:
            raise ValueError("dtype must be float32, int16 or int32, not %s" % (dtype,))
        if layout not in ("planar", "interleaved"):
            raise ValueError("layout must be 'planar' or 'interleaved', not %r" % (layout,))
        ps = self._resident_sources(srcs)
        heads = self.resident_headers(ps) if ps else []
        given = [rc in (0, 11) for rc, _ in heads]         # OK, or a header CRC failure: the fields are delivered
        nchs = [h.wave_format.num_channels if g else 0 for g, (_, h) in zip(given, heads)]
        nsmp = [h.num_samples if g else 0 for g, (_, h) in zip(given, heads)]
        B, Cn = len(ps), max(nchs, default=0)
        L = int(length) if length is not None else max(nsmp, default=0)
        if L < 0 or L > 0xFFFFFFFF:
            raise ValueError("length %d out of range" % L)
        dev = torch.device("cuda", self.device_index)
        shape = (B, Cn, L) if layout == "planar" else (B, L, Cn)
        out = torch.empty(shape, dtype=dtype, device=dev)
        if out.numel() == 0:
            # nothing can be written: a one-element stand-in keeps the per-item pointers valid, the results are real
            scratch = torch.empty(1, dtype=dtype, device=dev)
            outs = [scratch.as_strided((Cn, L), (1, 1)) for _ in range(B)]
        else:
            outs = [out[b] if layout == "planar" else out[b].t() for b in range(B)]
        got = self.decode_resident_into(ps, outs, fmt, zero_fill=True, _headers=heads)
        # the zero fill covers [n, L) of the rows a header gave; what no header covers is zeroed here
        for b in range(B):
            if nchs[b] < Cn:
                if layout == "planar":
                    out[b, nchs[b]:].zero_()
                else:
                    out[b, :, nchs[b]:].zero_()
        return out, [n for _, n in got], [rc for rc, _ in got]

    def salvage_resident_tensor(self, src, dtype=None, layout="planar", right_justify=False, range_capacity=64):
        """one .sla stream whose bytes are in device memory decoded THROUGH damage (sla_hip_salvage_resident): all N samples
        of its header, each decoded or zero.  src as one source of decode_resident_into; dtype, layout and right_justify as
        for decode_resident_tensor.  Returns (tensor [C][N] or [N][C], report, ranges): report is a dict of the fields of
        sla_hip_salvage_report plus "result" (0 when nothing was concealed or lost, 11 = DETECT_DATA_CORRUPTION when
        something was), ranges the list of (start, length, reason) of the silent ranges, reason "crc", "undecodable" or
        "gap".  Raises SlaError for every other code: nothing was delivered then."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype == torch.float32:
            fmt = PCM_F32
        elif dtype == torch.int16:
            fmt = PCM_S16
        elif dtype == torch.int32:
            fmt = PCM_S32 if right_justify else PCM_S32_LEFT
        else:
            raise ValueError("dtype must be float32, int16 or int32, not %s" % (dtype,))
        if layout not in ("planar", "interleaved"):
            raise ValueError("layout must be 'planar' or 'interleaved', not %r" % (layout,))
        (ptr, size), = self._resident_sources([src])
        (rc, h), = self.resident_headers([(ptr, size)])
        if rc != 0:
            raise SlaError(rc, "sla_hip_salvage_resident (header)")
        nch, n = h.wave_format.num_channels, h.num_samples
        dev = torch.device("cuda", self.device_index)
        out = torch.empty((nch, n) if layout == "planar" else (n, nch), dtype=dtype, device=dev)
        view = out if layout == "planar" else out.t()
        # nothing can be written to an empty tensor: a one-element stand-in keeps the pointer valid, the result is real
        base = out if out.numel() else torch.empty(1, dtype=dtype, device=dev)
        report, ranges = SalvageReport(), (SalvageRange * max(range_capacity, 1))()
        while True:
            st = torch.cuda.current_stream(self.device_index)
            self._index_walk = None          # last_walk() speaks of this call from here on
            rc = self._lib.sla_hip_salvage_resident(self._h, C.c_void_p(ptr or None), size, C.c_void_p(base.data_ptr()),
                                                    view.stride(0), max(view.stride(1), 1), n, fmt, C.byref(report), ranges,
                                                    len(ranges), C.c_void_p(st.cuda_stream))
            if rc not in (0, 11):
                raise SlaError(rc, "sla_hip_salvage_resident")
            if report.num_ranges <= len(ranges):
                break
            ranges = (SalvageRange * report.num_ranges)()     # more silent ranges than room: once more with room for all
        rep = {name: int(getattr(report, name)) for name, _ in SalvageReport._fields_ if name != "reserved"}
        rep["result"] = rc
        return out, rep, [(int(r.start), int(r.length), SALVAGE_REASON.get(int(r.reason), int(r.reason)))
                          for r in ranges[:report.num_ranges]]

    def salvage(self, data, dtype=None, layout="planar", right_justify=False):
        """salvage_resident_tensor for a stream in host memory: the bytes are uploaded, the samples come back as a numpy
        array; -> (array, report, ranges)"""
        import torch
        buf = np.frombuffer(bytes(data), np.uint8)
        if len(buf) == 0:
            raise SlaError(9, "sla_hip_salvage_resident (header)")
        src = torch.from_numpy(buf.copy()).to(torch.device("cuda", self.device_index))
        out, rep, ranges = self.salvage_resident_tensor(src, dtype, layout, right_justify)
        return out.cpu().numpy(), rep, ranges

    def decode_windows_into(self, srcs, starts, outs, sample_format, zero_fill=True, hints=None, stream=None, _headers=None):
        """sample windows of .sla streams whose bytes are in device memory -> caller-owned device tensors
        (sla_hip_decode_windows_resident): window i is the samples [starts[i], starts[i] + outs[i].shape[1]) of srcs[i],
        clipped to the file, delivered whole or not at all; only the blocks it overlaps are gathered and decoded.  srcs,
        outs, sample_format, zero_fill and stream as for decode_resident_into; the same source may appear any number of
        times.  hints[i]: None or a (byte, sample) pair naming a block start at or before the window, such as an earlier
        call returned.  Returns [(result code, samples, (first_block_byte, first_block_sample))]."""
        import torch
        if sample_format not in self._FORMAT_DTYPE:
            raise ValueError("unknown sample format %r" % (sample_format,))
        if len(outs) != len(srcs) or len(starts) != len(srcs) or (hints is not None and len(hints) != len(srcs)):
            raise ValueError("%d sources, %d starts, %d outputs" % (len(srcs), len(starts), len(outs)))
        want = getattr(torch, self._FORMAT_DTYPE[sample_format])
        ps = self._resident_sources(srcs)
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        heads = _headers if _headers is not None else self.resident_headers(ps, stream=st)
        items = (DecodeWindowItem * max(len(ps), 1))()
        for i, ((ptr, size), out) in enumerate(zip(ps, outs)):
            if not isinstance(out, torch.Tensor) or out.dim() != 2:
                raise ValueError("output %d: need a 2-D torch tensor [channel][sample]" % i)
            if out.dtype != want:
                raise ValueError("output %d: dtype %s, the format wants %s" % (i, out.dtype, want))
            if out.device.type != "cuda" or out.device.index != self.device_index:
                raise ValueError("output %d: on %s, the decoder's device is cuda:%d" % (i, out.device, self.device_index))
            rc, h = heads[i]
            nch = h.wave_format.num_channels if rc in (0, 11) else 0
            if out.shape[0] < nch:
                raise ValueError("output %d: %d rows for a file of %d channels" % (i, out.shape[0], nch))
            if out.shape[1] > 0xFFFFFFFF or min(out.stride()) < 0 or (out.shape[1] > 1 and out.stride(1) == 0) \
                    or (nch > 1 and out.stride(0) == 0):
                raise ValueError("output %d: unsupported shape %s / strides %s" % (i, tuple(out.shape), out.stride()))
            start = int(starts[i])
            hint = hints[i] if hints is not None and hints[i] is not None else (0, 0)
            if not 0 <= start <= 0xFFFFFFFF or not 0 <= int(hint[0]) <= 0xFFFFFFFF or not 0 <= int(hint[1]) <= 0xFFFFFFFF:
                raise ValueError("window %d: start %d / hint %r out of range" % (i, start, hint))
            items[i].data = C.cast(C.c_void_p(ptr or None), u8p)
            items[i].data_size = size
            # a window of no samples is answered, not refused: an empty view still names its place in its storage
            items[i].dst = out.data_ptr() or (out.untyped_storage().data_ptr() + out.storage_offset() * out.element_size()) or None
            items[i].channel_stride = out.stride(0)
            items[i].sample_stride = max(out.stride(1), 1)
            items[i].start = start
            items[i].length = out.shape[1]
            items[i].seek_byte, items[i].seek_sample = int(hint[0]), int(hint[1])
        rc = self._lib.sla_hip_decode_windows_resident(self._h, items, len(ps), sample_format,
                                                       DEC_ZERO_FILL if zero_fill else 0, C.c_void_p(st.cuda_stream))
        self._check(rc, "sla_hip_decode_windows_resident")
        return [(int(items[i].result), int(items[i].output_num_samples),
                 (int(items[i].first_block_byte), int(items[i].first_block_sample))) for i in range(len(ps))]

    def decode_windows_tensor(self, srcs, starts, length, dtype=None, layout="planar", right_justify=False, index=None):
        """one window of `length` samples per source -> one device tensor on the handle's device: [B][C][length] (planar)
        or [B][length][C] (interleaved), C the largest channel count among the headers; dtype, layout and right_justify
        as for decode_resident_tensor.  Returns (tensor, samples, results); everything past a window's samples, rows past
        a file's channel count and windows that gave nothing are zero.  index: what block_index_resident(srcs) returned;
        every window's walk then starts at the last block at or before starts[i] instead of at the header."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype == torch.float32:
            fmt = PCM_F32
        elif dtype == torch.int16:
            fmt = PCM_S16
        elif dtype == torch.int32:
            fmt = PCM_S32 if right_justify else PCM_S32_LEFT
        else:
            raise ValueError("dtype must be float32, int16 or int32, not %s" % (dtype,))
        if layout not in ("planar", "interleaved"):
            raise ValueError("layout must be 'planar' or 'interleaved', not %r" % (layout,))
        ps = self._resident_sources(srcs)
        if len(starts) != len(ps) or (index is not None and len(index) != len(ps)):
            raise ValueError("%d sources, %d starts" % (len(ps), len(starts)))
        L = int(length)
        if L < 0 or L > 0xFFFFFFFF:
            raise ValueError("length %d out of range" % L)
        heads = self.resident_headers(ps) if ps else []
        nchs = [h.wave_format.num_channels if rc in (0, 11) else 0 for rc, h in heads]
        B, Cn = len(ps), max(nchs, default=0)
        hints = None
        if index is not None:
            hints = []
            for (byte_off, smp_off, _), start in zip(index, starts):
                k = int(np.searchsorted(smp_off, int(start), side="right")) - 1
                hints.append((int(byte_off[k]), int(smp_off[k])) if k >= 0 else None)
        dev = torch.device("cuda", self.device_index)
        shape = (B, Cn, L) if layout == "planar" else (B, L, Cn)
        out = torch.empty(shape, dtype=dtype, device=dev)
        if out.numel() == 0:
            # nothing can be written: a one-element stand-in keeps the per-item pointers valid, the results are real
            scratch = torch.empty(1, dtype=dtype, device=dev)
            outs = [scratch.as_strided((Cn, L), (1, 1)) for _ in range(B)]
        else:
            outs = [out[b] if layout == "planar" else out[b].t() for b in range(B)]
        got = self.decode_windows_into(ps, starts, outs, fmt, zero_fill=True, hints=hints, _headers=heads)
        # the zero fill covers the rows a header gave; rows no header covers, and windows refused outright, are zeroed here
        for b in range(B):
            if out.numel() and (nchs[b] < Cn or got[b][0] == 2):
                first = 0 if got[b][0] == 2 else nchs[b]
                if layout == "planar":
                    out[b, first:].zero_()
                else:
                    out[b, :, first:].zero_()
        return out, [n for _, n, _ in got], [rc for rc, _, _ in got]

    def index_resident(self, srcs, stream=None):
        """[Index] of .sla streams whose bytes are in device memory (sla_hip_index_build_resident): the header gather and
        the chain walk on the device, wide for streams of at least the option "wide_walk".  Each serialises to the bytes
        Index.build gives a host copy."""
        import torch
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        out = []
        self._index_walk = None              # last_walk() speaks of the last stream walked here
        for ptr, size in self._resident_sources(srcs):
            h = C.c_void_p()
            self._check(self._lib.sla_hip_index_build_resident(self._h, C.c_void_p(ptr or None), size, C.c_void_p(st.cuda_stream),
                                                               C.byref(h)), "sla_hip_index_build_resident")
            out.append(Index(h))
        return out

    def decode_windows_indexed_into(self, srcs, indexes, starts, outs, sample_format, zero_fill=True, stream=None):
        """decode_windows_into from block indexes, QUEUED (sla_hip_decode_windows_indexed): the call returns once its work
        is enqueued behind `stream`; work queued on `stream` afterwards sees outs and the outcomes written.  indexes[i] is
        the Index of srcs[i] (None refuses the item).  Returns an int32 device tensor [B][2]: (result code, samples) per
        window, what decode_windows_into returns for the same bytes.  Nothing here waits for the device."""
        import torch
        if sample_format not in self._FORMAT_DTYPE:
            raise ValueError("unknown sample format %r" % (sample_format,))
        if len(outs) != len(srcs) or len(starts) != len(srcs) or len(indexes) != len(srcs):
            raise ValueError("%d sources, %d indexes, %d starts, %d outputs" % (len(srcs), len(indexes), len(starts), len(outs)))
        want = getattr(torch, self._FORMAT_DTYPE[sample_format])
        ps = self._resident_sources(srcs)
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        items = (IndexedWindowItem * max(len(ps), 1))()
        for i, ((ptr, size), out) in enumerate(zip(ps, outs)):
            if not isinstance(out, torch.Tensor) or out.dim() != 2:
                raise ValueError("output %d: need a 2-D torch tensor [channel][sample]" % i)
            if out.dtype != want:
                raise ValueError("output %d: dtype %s, the format wants %s" % (i, out.dtype, want))
            if out.device.type != "cuda" or out.device.index != self.device_index:
                raise ValueError("output %d: on %s, the decoder's device is cuda:%d" % (i, out.device, self.device_index))
            x = indexes[i]
            nch = x.header.wave_format.num_channels if x is not None and x.header is not None and x.data_size == size else 0
            if out.shape[0] < nch:
                raise ValueError("output %d: %d rows for a file of %d channels" % (i, out.shape[0], nch))
            if out.shape[1] > 0xFFFFFFFF or min(out.stride()) < 0 or (out.shape[1] > 1 and out.stride(1) == 0) \
                    or (nch > 1 and out.stride(0) == 0):
                raise ValueError("output %d: unsupported shape %s / strides %s" % (i, tuple(out.shape), out.stride()))
            start = int(starts[i])
            if not 0 <= start <= 0xFFFFFFFF:
                raise ValueError("window %d: start %d out of range" % (i, start))
            items[i].data = C.cast(C.c_void_p(ptr or None), u8p)
            items[i].data_size = size
            items[i].index = x.handle if x is not None else None
            items[i].dst = out.data_ptr() or (out.untyped_storage().data_ptr() + out.storage_offset() * out.element_size()) or None
            items[i].channel_stride = out.stride(0)
            items[i].sample_stride = max(out.stride(1), 1)
            items[i].start = start
            items[i].length = out.shape[1]
        with torch.cuda.stream(st):
            outcomes = torch.empty((max(len(ps), 1), 2), dtype=torch.int32, device=torch.device("cuda", self.device_index))
        rc = self._lib.sla_hip_decode_windows_indexed(self._h, items, len(ps), sample_format, DEC_ZERO_FILL if zero_fill else 0,
                                                      C.c_void_p(outcomes.data_ptr()), C.c_void_p(st.cuda_stream))
        self._check(rc, "sla_hip_decode_windows_indexed")
        return outcomes[:len(ps)]

    def decode_windows_indexed(self, srcs, indexes, starts, length, dtype=None, layout="planar", right_justify=False):
        """decode_windows_tensor from block indexes, queued on the current stream: one window of `length` samples per
        source -> (tensor, outcomes); the tensor's shape is decode_windows_tensor's, from the indexes' headers, outcomes an
        int32 device tensor [B][2] of (result code, samples).  Rows no header covers, and windows refused outright, are
        zeroed by stream-ordered torch ops: nothing here waits for the device."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype == torch.float32:
            fmt = PCM_F32
        elif dtype == torch.int16:
            fmt = PCM_S16
        elif dtype == torch.int32:
            fmt = PCM_S32 if right_justify else PCM_S32_LEFT
        else:
            raise ValueError("dtype must be float32, int16 or int32, not %s" % (dtype,))
        if layout not in ("planar", "interleaved"):
            raise ValueError("layout must be 'planar' or 'interleaved', not %r" % (layout,))
        ps = self._resident_sources(srcs)
        if len(starts) != len(ps) or len(indexes) != len(ps):
            raise ValueError("%d sources, %d indexes, %d starts" % (len(ps), len(indexes), len(starts)))
        L = int(length)
        if L < 0 or L > 0xFFFFFFFF:
            raise ValueError("length %d out of range" % L)
        nchs = [x.header.wave_format.num_channels if x is not None and x.header is not None and x.data_size == size else 0
                for x, (_, size) in zip(indexes, ps)]
        B, Cn = len(ps), max(nchs, default=0)
        dev = torch.device("cuda", self.device_index)
        shape = (B, Cn, L) if layout == "planar" else (B, L, Cn)
        out = torch.empty(shape, dtype=dtype, device=dev)
        if out.numel() == 0:
            scratch = torch.empty(1, dtype=dtype, device=dev)
            outs = [scratch.as_strided((Cn, L), (1, 1)) for _ in range(B)]
        else:
            outs = [out[b] if layout == "planar" else out[b].t() for b in range(B)]
        outcomes = self.decode_windows_indexed_into(ps, indexes, starts, outs, fmt, zero_fill=True)
        if out.numel():
            # the zero fill covers the rows a header gave; rows no header covers are zeroed here, and a window refused
            # outright (INVALID_ARGUMENT: nothing of it was written) by a mask from its outcome, all on the stream
            for b in range(B):
                if nchs[b] < Cn:
                    (out[b, nchs[b]:] if layout == "planar" else out[b, :, nchs[b]:]).zero_()
            refused = (outcomes[:, 0] == 2).view(B, 1, 1)
            out.masked_fill_(refused, 0)
        return out, outcomes

    def splice_resident(self, outputs, outs=None, arena=None, stream=None):
        """new .sla streams from parts of resident ones, without re-encoding (sla_hip_splice_resident): outputs[i] is a list of
        segments (src, Index, start, length), src a 1-D uint8 CUDA tensor or a (ptr, size) pair; whole blocks are copied
        byte for byte, the blocks a cut passes through are decoded and stored as RAW (SILENT) blocks.  outs: one 1-D uint8
        CUDA tensor per output (its capacity), arena: one such tensor the streams are packed into back to back, neither:
        tensors of splice_plan's size.  Returns [(result code, uint8 tensor of the stream -- a view of outs[i] / the arena --
        or None)].  Synchronous."""
        import torch
        if outs is not None and arena is not None:
            raise ValueError("outs and arena exclude each other")
        n = len(outputs)
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        dev = torch.device("cuda", self.device_index)
        items = (SpliceItem * max(n, 1))()
        keep = []
        for i, segments in enumerate(outputs):
            item, segs = _splice_item(list(segments))
            keep.append(segs)
            items[i].segments, items[i].num_segments = item.segments, item.num_segments
        if arena is None:
            if outs is None:
                with torch.cuda.stream(st):
                    outs = [torch.empty(max(int(splice_plan(list(s))[1].bytes), 1), dtype=torch.uint8, device=dev) for s in outputs]
            if len(outs) != n:
                raise ValueError("%d outputs, %d destinations" % (n, len(outs)))
            for i, o in enumerate(outs):
                if o.dim() != 1 or o.dtype != torch.uint8 or not o.is_contiguous() or o.device != dev or o.numel() > 0xFFFFFFFF:
                    raise ValueError("destination %d: need a 1-D contiguous uint8 tensor on %s" % (i, dev))
                items[i].data, items[i].data_size = (o.data_ptr() or None), o.numel()
        elif arena.dim() != 1 or arena.dtype != torch.uint8 or not arena.is_contiguous() or arena.device != dev:
            raise ValueError("arena: need a 1-D contiguous uint8 tensor on %s" % dev)
        rc = self._lib.sla_hip_splice_resident(self._h, items, n, C.c_void_p(arena.data_ptr()) if arena is not None else None,
                                               arena.numel() if arena is not None else 0, C.c_void_p(st.cuda_stream))
        self._check(rc, "sla_hip_splice_resident")
        got = []
        for i in range(n):
            size = int(items[i].output_size)
            if items[i].result != 0:
                got.append((int(items[i].result), None))
            elif arena is not None:
                off = int(items[i].data) - arena.data_ptr()
                got.append((0, arena[off:off + size]))
            else:
                got.append((0, outs[i][:size]))
        return got

    def cut_resident(self, src, index, start, length):
        """samples [start, start + length) of one resident stream as a new stream: (result code, uint8 tensor or None)"""
        return self.splice_resident([[(src, index, start, length)]])[0]

    def join_resident(self, srcs, indexes):
        """whole resident streams of one format, one after the other, as one stream: (result code, uint8 tensor or None)"""
        return self.splice_resident([[(s, x, 0, x.extent) for s, x in zip(srcs, indexes)]])[0]

    def set_option(self, name, value):
        """a handle option (sla_hip_decoder_set_option): "wide_walk" -- resident streams of at least that many bytes have
        their block chain walked by the whole device, 0 = off, default WIDE_WALK_DEFAULT -- and "wide_walk_nodes", the node capacity of such a walk
        (0 = by stream size)"""
        self._check(self._lib.sla_hip_decoder_set_option(self._h, name.encode(), float(value)), "sla_hip_decoder_set_option")
        if name == "wide_walk":
            self._wide_walk = int(value)
        elif name == "wide_walk_nodes":
            self._wide_nodes = int(value)

    def last_walk(self):
        """(files walked wide, wide walks that overflowed and went to a lane, nodes found, doubling rounds launched), summed
        over the last resident decode (sla_hip_decoder_last_walk) or the last block_index_resident"""
        if self._index_walk is not None:
            return self._index_walk
        c = (C.c_uint64 * 4)()
        self._check(self._lib.sla_hip_decoder_last_walk(self._h, c), "sla_hip_decoder_last_walk")
        return tuple(int(v) for v in c)

    def block_index_resident(self, srcs, stream=None, wide=None):
        """the block chain of every resident stream, for hints: [(byte_off, smp_off, stop)] with the file position of
        every block's sync code and of its first sample as numpy uint32 arrays, and the walk's stop code (0: the chain
        reaches the header's num_samples).  Two launches of sla_hip_launch_dec_walk, count mode and write mode; a block
        larger than the handle's max_num_block_samples ends a file's index.  A caller keeps the index next to the bytes
        and hands it to decode_windows_tensor(index=...).
        wide: True walks every stream with sla_hip_launch_dec_walk_wide (the whole device on one file, for long files),
        False none, None those of at least the handle's "wide_walk" bytes (at most the 8 longest).  The index is the same
        either way; a wide walk whose nodes overflow the capacity falls back to the lane and shows in last_walk()."""
        import torch
        ps = self._resident_sources(srcs)
        nf = len(ps)
        if nf == 0:
            return []
        st = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        heads = self.resident_headers(ps, stream=st)
        dev = torch.device("cuda", self.device_index)
        table = (DecWalkFile * nf)()
        for i, ((ptr, size), (rc, h)) in enumerate(zip(ps, heads)):
            table[i].src = ptr or None
            table[i].data_size = size if rc in (0, 11) else 0
            table[i].total = h.num_samples if rc in (0, 11) else 0
            table[i].capacity = 0xFFFFFFFF
        sp = C.c_void_p(st.cuda_stream)

        def run(rows):
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            with torch.cuda.stream(st):
                d_tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
                d_res = torch.zeros(nf * C.sizeof(DecWalkResult), dtype=torch.uint8, device=dev)
                d_blk = torch.zeros(rows * 24, dtype=torch.uint8, device=dev) if rows else None
                d_end = torch.zeros(rows * 8, dtype=torch.uint8, device=dev) if rows else None
                d_crc = torch.zeros(rows * 4, dtype=torch.uint8, device=dev) if rows else None
                self._check(self._lib.sla_hip_launch_dec_walk(ptr(d_tab), nf, self.max_num_block_samples, 0, ptr(d_res), ptr(d_blk),
                                                              ptr(d_end), ptr(d_crc), sp), "sla_hip_launch_dec_walk")
                st.synchronize()
            res = np.frombuffer(d_res.cpu().numpy().tobytes(), np.uint32).reshape(nf, 4)
            blk = np.frombuffer(d_blk.cpu().numpy().tobytes(), np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"),
                                ("num_samples", "<u4"), ("flags", "<u4")])) if rows else None
            return res, blk

        # the streams that go wide: the lane launch sees them with total = 0, their wide launches come behind it
        threshold = self._wide_walk
        if wide is None:
            cand = [i for i in range(nf) if threshold and table[i].data_size >= threshold]
            cand = sorted(cand, key=lambda i: (-table[i].data_size, i))[:8]
        else:
            cand = list(range(nf)) if wide else []
        stats = [0, 0, 0, 0]
        ncap = lambda size: self._wide_nodes or max(1 << 16, size // 256)

        def run_wide(rows, which):
            """the lane launch with `which` blanked, then their wide launches; -> results, rows, the wide files' info"""
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            totals = {i: table[i].total for i in which}
            with torch.cuda.stream(st):
                for i in which:
                    table[i].total = 0
                d_tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
                for i in which:
                    table[i].total = totals[i]
                d_res = torch.zeros(nf * C.sizeof(DecWalkResult), dtype=torch.uint8, device=dev)
                d_blk = torch.zeros(rows * 24, dtype=torch.uint8, device=dev) if rows else None
                d_end = torch.zeros(rows * 8, dtype=torch.uint8, device=dev) if rows else None
                d_crc = torch.zeros(rows * 4, dtype=torch.uint8, device=dev) if rows else None
                need = max([self._lib.sla_hip_dec_wide_scratch_bytes(table[i].data_size, ncap(table[i].data_size)) for i in which] + [16])
                d_scr = torch.empty(need, dtype=torch.uint8, device=dev)
                d_inf = torch.zeros(max(len(which), 1) * 16, dtype=torch.uint8, device=dev)
                self._check(self._lib.sla_hip_launch_dec_walk(ptr(d_tab), nf, self.max_num_block_samples, 0, ptr(d_res), ptr(d_blk),
                                                              ptr(d_end), ptr(d_crc), sp), "sla_hip_launch_dec_walk")
                for k, i in enumerate(which):
                    size = table[i].data_size
                    self._check(self._lib.sla_hip_launch_dec_walk_wide(C.byref(table[i]), self.max_num_block_samples, 0,
                                                                       C.c_void_p(d_res.data_ptr() + 16 * i), ptr(d_blk), ptr(d_end),
                                                                       ptr(d_crc), ncap(size), ptr(d_scr), sp),
                                "sla_hip_launch_dec_walk_wide")
                    d_inf[16 * k:16 * k + 16].copy_(d_scr[:16])
                    stats[3] += int(self._lib.sla_hip_dec_wide_rounds(size, ncap(size)))
                st.synchronize()
            res = np.frombuffer(d_res.cpu().numpy().tobytes(), np.uint32).reshape(nf, 4).copy()
            blk = np.frombuffer(d_blk.cpu().numpy().tobytes(), np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"),
                                ("num_samples", "<u4"), ("flags", "<u4")])) if rows else None
            return res, blk, np.frombuffer(d_inf.cpu().numpy().tobytes(), np.uint32).reshape(-1, 4)

        if cand:
            res, _, info = run_wide(0, cand)
            stats[0] = len(cand)
            stats[2] = int(sum(int(info[k][0]) for k in range(len(cand))))
            over = [i for i in cand if int(res[i][3]) != 0]
            stats[1] = len(over)
            cand = [i for i in cand if i not in over]
            if over:                                     # more nodes than the capacity: those on lanes after all
                res_lane, _ = run(0)
                for i in over:
                    res[i] = res_lane[i]
        else:
            res, _ = run(0)
        first = 0
        for i in range(nf):
            table[i].first, table[i].max_rows = first, int(res[i][0])
            first += int(res[i][0])
        self._index_walk = tuple(stats)
        if first == 0:
            return [(np.zeros(0, np.uint32), np.zeros(0, np.uint32), int(res[i][1])) for i in range(nf)]
        if cand:
            res2, blk, _ = run_wide(first, cand)
            self._index_walk = tuple(stats)
        else:
            res2, blk = run(first)
        if not np.array_equal(res, res2):
            raise RuntimeError("block_index_resident: the streams changed during the call")
        out = []
        for i in range(nf):
            rows = blk[table[i].first:table[i].first + table[i].max_rows]
            out.append((rows["byte_off"].astype(np.uint32), rows["smp_off"].astype(np.uint32), int(res[i][1])))
        return out

    def last_window_stats(self):
        """(blocks passed over, blocks decoded, stream bytes gathered, plane samples per channel reserved), summed over the
        last decode_windows_into / decode_windows_tensor (sla_hip_decoder_last_window_stats)"""
        c = (C.c_uint64 * 4)()
        self._check(self._lib.sla_hip_decoder_last_window_stats(self._h, c), "sla_hip_decoder_last_window_stats")
        return tuple(int(v) for v in c)

    def decode_device(self, data, image_ptr, planes_ptr, plane_stride):
        """decode an image that already lives in device memory into device planes; returns (rc, samples)"""
        buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
        n = C.c_uint32(0)
        rc = self._lib.sla_hip_decode_device(self._h, buf.ctypes.data_as(u8p), C.c_void_p(image_ptr), len(buf),
                                             C.c_void_p(planes_ptr), plane_stride, C.byref(n))
        return rc, n.value

    def last_timing(self):
        """[ms] upload, block walk, kernels (stream events), download, total; number of kernel batches
        (after decode_batch: of passes; after decode_batch_into: [3] is the emit and zero-fill stage; after
        decode_resident_into: [0] the gathers, [1] the device walks and their copies)"""
        t = (C.c_float * 6)()
        self._lib.sla_hip_decoder_last_timing(self._h, t)
        return list(t)


def streaming_decode(data, decode_interval_hz=120.0, feed=None, max_bit_per_sample=24, crc=1,
                     capacity=(8, 16384, 48, 5, 40)):
    """Drive SLAStreamingDecoder_* the way the reference CLI does (src/main.c:277-420): header, then per call
    append the estimated number of bytes (or `feed(i)` bytes), decode, collect.  Returns (rc, pcm [C][n], calls).
    capacity: (channels, block samples <= 65535, PARCOR order, long-term taps, LMS order) of the handle."""
    L = lib()
    buf = np.frombuffer(bytes(data), np.uint8)
    h = SLAHeaderInfo()
    rc = L.SLADecoder_DecodeHeader(buf.ctypes.data_as(u8p), len(buf), C.byref(h))
    if rc != 0:
        return rc, None, 0
    cfg = SLAStreamingDecoderConfig(SLADecoderConfig(*capacity, crc, 0), decode_interval_hz, max_bit_per_sample)
    dec = L.SLAStreamingDecoder_Create(C.byref(cfg))
    if not dec:
        raise RuntimeError("SLAStreamingDecoder_Create failed")
    try:
        rc = L.SLAStreamingDecoder_SetWaveFormat(dec, C.byref(h.wave_format))
        if rc == 0:
            rc = L.SLAStreamingDecoder_SetEncodeParameter(dec, C.byref(h.encode_param))
        if rc != 0:
            return rc, None, 0
        nch, total = h.wave_format.num_channels, h.num_samples
        out = np.zeros((nch, max(total, 1)), np.int32)
        sample_pos, data_pos, calls = 0, 43, 0
        est, got = C.c_uint32(0), C.c_uint32(0)
        dummy_p, dummy_n = u8p(), C.c_uint32(0)
        while sample_pos < total:
            if feed is not None:
                want = int(feed(calls))
            elif sample_pos == 0 and calls == 0:
                want = h.max_block_size
            else:
                L.SLAStreamingDecoder_EstimateMinimumNessesaryDataSize(dec, C.byref(est))
                want = est.value
            put = min(want, len(buf) - data_pos)
            rc = L.SLAStreamingDecoder_AppendDataFragment(dec, buf[data_pos:].ctypes.data_as(u8p) if put > 0 else buf.ctypes.data_as(u8p), put)
            if rc != 0:
                return rc, out[:, :sample_pos], calls
            ptrs = (i32p * nch)(*[out[c, sample_pos:].ctypes.data_as(i32p) for c in range(nch)])
            rc = L.SLAStreamingDecoder_Decode(dec, ptrs, total - sample_pos, C.byref(got))
            calls += 1
            if rc == 9 and data_pos + put < len(buf):         # not even a block header yet: keep feeding
                rc, got.value = 0, 0
            if rc != 0:
                return rc, out[:, :sample_pos], calls
            L.SLAStreamingDecoder_CollectDataFragment(dec, C.byref(dummy_p), C.byref(dummy_n))
            data_pos += put
            sample_pos += got.value
            if got.value == 0 and put == 0 and data_pos >= len(buf):
                return 9, out[:, :sample_pos], calls          # the stream ended inside a block
        return 0, out[:, :total], calls
    finally:
        L.SLAStreamingDecoder_Destroy(dec)


def decode_header(data):
    """(result code, SLAHeaderInfo) of the first 43 bytes"""
    buf = np.frombuffer(bytes(data), np.uint8)
    h = SLAHeaderInfo()
    rc = lib().SLADecoder_DecodeHeader(buf.ctypes.data_as(u8p), len(buf), C.byref(h))
    return rc, h


def encode_header(num_channels, bits, rate, lshift, parcor, ltm, lms, chproc, window, max_block,
                  num_samples, num_blocks, max_block_size, max_bps):
    h = SLAHeaderInfo(SLAWaveFormat(num_channels, bits, rate, lshift),
                      SLAEncodeParameter(parcor, ltm, lms, chproc, window, max_block),
                      num_samples, num_blocks, max_block_size, max_bps)
    out = np.zeros(64, np.uint8)
    rc = lib().SLAEncoder_EncodeHeader(C.byref(h), out.ctypes.data_as(u8p), 64)
    if rc != 0:
        raise SlaError(rc, "SLAEncoder_EncodeHeader")
    return out[:43].tobytes()


def device_name():
    return lib().sla_hip_device_name().decode()
