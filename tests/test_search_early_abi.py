"""Checks of the search beside the prepass (option "search_early", include/sla_hip.h) that need no kernel: the header's entry
points, the exported symbols, the refusals that come before any device work.  Only the option check needs a handle, and a
handle needs a device: that one test is marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 2
NAMES = ("sla_hip_launch_prepass_early", "sla_hip_launch_search_exact_early", "sla_hip_launch_plan_early",
         "sla_hip_launch_expand_early", "sla_hip_last_search_early")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def _define(text, name):
    m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, text)
    assert m, name
    return int(m.group(1))


def test_header_declares_the_early_start():
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in sla_amd.EXPORTED_SYMBOLS, name
    # two words, the flag first: the encoder clears it together with the word in front of it
    assert (_define(text, "SLA_HIP_EARLY_CANCEL"), _define(text, "SLA_HIP_EARLY_LSHIFT"), _define(text, "SLA_HIP_EARLY_WORDS")) == (0, 1, 2)
    assert '"search_early"' in text and '"early_prepass_groups"' in text      # the options are documented with the others
    for doc in ("README.md", "DESIGN.md"):
        assert "search_early" in open(os.path.join(ROOT, doc)).read(), doc
    # the signatures that were there before are as they were
    assert re.search(r"int sla_hip_launch_prepass\(const int32_t\* d_pcm, uint64_t plane_stride, uint32_t num_channels,\s*"
                     r"uint32_t num_samples, uint32_t bits_per_sample, uint32_t mid_side,\s*"
                     r"uint32_t\* d_or_mask, uint64_t\* d_nz_mask, sla_hip_stream_t stream\);", text)
    assert re.search(r"int sla_hip_last_expand\(const struct SLAEncoder\* encoder, uint32_t\* counters\);", text)


def test_symbols_are_exported(L):
    for name in NAMES:
        assert hasattr(L, name), name
    assert hasattr(sla_amd.Encoder, "last_search_early")


def test_refusals_come_before_any_device_work(L):
    # dangling values: nothing behind them is touched when an argument is refused
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(12)]
    L.sla_hip_launch_prepass_early.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    assert L.sla_hip_launch_prepass_early(p[0], 100, 1, 100, 16, 0, p[1], p[2], None, 0, None) == INVALID_ARGUMENT      # no words
    assert L.sla_hip_launch_prepass_early(None, 100, 1, 100, 16, 0, p[1], p[2], p[3], 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_prepass_early(p[0], 100, 1, 100, 33, 0, p[1], p[2], p[3], 0, None) == INVALID_ARGUMENT
    assert L.sla_hip_launch_prepass_early(p[0], 99, 1, 100, 16, 0, p[1], p[2], p[3], 0, None) == INVALID_ARGUMENT       # stride < samples
    L.sla_hip_launch_search_exact_early.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                    C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def search(groups=8, early=p[6], done=p[7]):
        return L.sla_hip_launch_search_exact_early(p[0], 100000, 0, 16, p[1], groups, 4096, 10, p[2], p[3], p[4], 1.0, 64.0, p[5],
                                                   None, None, early, done)

    assert search(early=None) == INVALID_ARGUMENT
    assert search(done=None) == INVALID_ARGUMENT                # no event: nothing would order the chain behind the prepass
    assert search(groups=0) == INVALID_ARGUMENT                 # no launch, no wait queued
    c = (C.c_uint32 * 4)(*([7] * 4))
    L.sla_hip_last_search_early.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    assert L.sla_hip_last_search_early(None, c) == INVALID_ARGUMENT
    assert L.sla_hip_last_search_early(C.c_void_p(0x10), None) == INVALID_ARGUMENT
    assert list(c) == [7] * 4


@pytest.mark.gpu
def test_option_default_range_and_unknown_values():
    import torch
    torch.cuda.init()
    enc = sla_amd.Encoder(1, 4096, 16, 1, 8)
    try:
        assert enc.last_search_early() == (0, 0, 0, 0)
        for v in (-1, 2, 0.5, float("nan")):
            with pytest.raises(sla_amd.SlaError):
                enc.set_option("search_early", v)
        with pytest.raises(sla_amd.SlaError):
            enc.set_option("search_earlier", 1)
        for v in (1, 1 << 20, 0):                               # the cap on the early prepass's workgroups; 0 = automatic
            enc.set_option("early_prepass_groups", v)
        for v in (-1, (1 << 20) + 1, 1.5):
            with pytest.raises(sla_amd.SlaError):
                enc.set_option("early_prepass_groups", v)
        # the default is 1: the second file without silence starts early without anybody asking; 0 stops that, 1 brings it back
        enc.set_option("stream", 0)
        enc.set_wave_format(1, 16, 48000)
        enc.set_encode_parameter(16, 1, 8, 0, 1, 4096)
        rng = np.random.default_rng(5)
        pcm = ((rng.integers(-2000, 2000, size=(1, 3 * 4096 + 500), dtype=np.int64) | 1) << 16).astype(np.int32)
        first = enc.encode_whole(pcm)
        assert enc.last_search_early() == (0, 0, 0, 0)
        assert enc.encode_whole(pcm) == first
        assert enc.last_search_early() == (1, 1, 0, 0)
        enc.set_option("search_early", 0)
        assert enc.encode_whole(pcm) == first
        assert enc.last_search_early() == (0, 1, 0, 0)
        enc.set_option("search_early", 1)
        assert enc.encode_whole(pcm) == first
        assert enc.last_search_early() == (1, 2, 0, 0)
    finally:
        enc.close()
