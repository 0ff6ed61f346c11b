"""The two long-term synthesis kernels side by side, in one process (sla_hip_launch_dec_ltm picks by max_block_samples:
up to 40896 k_dec_ltm, the whole block in dynamic LDS; above, k_dec_ltm_far, a fixed 16 KiB ring).
 (a) identical job tables of 4096-, 16384- and 40896-sample blocks (two channels, 3 taps, pitches 20..256 as an analysis
     picks them), about 4 M samples each: k_dec_ltm asked for exactly the block's length of LDS, for a default handle's
     16384 samples (64 KiB) where the blocks fit, and for 40896 (the whole budget: one workgroup per CU); k_dec_ltm_far
     through max_block_samples = 40897.  The outputs of one run on a fresh copy must be equal.
 (b) Decoder.decode_resident_tensor of W.music_like(2, 140000, 16, seed=3) encoded by the oracle with blocks of up to 65535
     samples (handle capacity 65535: the ring kernel), against the same PCM encoded with blocks of up to 16384 on a default
     handle (k_dec_ltm, 64 KiB) and on the capacity-65535 handle.
Every step: 2 warm-ups, then the median of 5, under a time limit of its own.
usage: python tests/tools/bench_dec_ltm.py [out.json]"""
import ctypes as C
import json
import os
import signal
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch
torch.cuda.init()
import sla_amd
import decbitsmodel as DM
import slalibs as S
import waveforms as W

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dec_ltm_far.json")
WARM, REPS, STEP_LIMIT = 2, 5, 120
LDS_SAMPLES = (160 * 1024 - 256) // 4
CAP = (8, 65535, 255, 5, 32)


class StepTimeout(Exception):
    pass


def step(fn, limit=STEP_LIMIT):
    """fn() under a time limit of its own"""
    def on_alarm(signum, frame):
        raise StepTimeout("a step ran for more than %d s" % limit)
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(limit)
    try:
        return fn()
    finally:
        signal.alarm(0)


def median_ms(fn):
    """device time of fn() between two events on the current stream: 2 warm-ups, the median of 5"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t)), [round(x, 4) for x in t]


def wall_ms(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), [round(x, 3) for x in t]


L = sla_amd.lib()
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ptr = lambda t: C.c_void_p(t.data_ptr())
NTAPS, NCH = 3, 2

# ---- (a) the kernels on identical tables
kernels = []
for n, rows in ((4096, 512), (16384, 128), (40896, 52)):
    rng = np.random.default_rng(n)
    blocks = np.zeros(rows, DM.BLOCK_DT)
    blocks["smp_off"] = np.arange(rows) * n
    blocks["num_samples"] = n
    info = np.zeros((rows, 4), np.uint32)
    chan = np.zeros((rows, NCH, DM.CHAN_WORDS), np.uint32)
    chan[:, :, 0] = rng.integers(20, 257, (rows, NCH))
    chan[:, :, 1:1 + NTAPS] = (rng.integers(-9000, 9000, (rows, NCH, NTAPS)).astype(np.int64) << 16).astype(np.int32).view(np.uint32)
    x = rng.integers(-3000, 3000, (NCH, rows * n)).astype(np.int32)
    d_blk = torch.from_numpy(blocks.view(np.uint8).copy()).cuda()
    d_info = torch.from_numpy(info.view(np.int32).copy()).cuda()
    d_chan = torch.from_numpy(chan.view(np.int32).copy()).cuda()
    d_x = torch.from_numpy(x).cuda()
    d_work = d_x.clone()

    def run(mbs, planes=None):
        planes = d_work if planes is None else planes
        assert L.sla_hip_launch_dec_ltm(ptr(planes), C.c_uint64(rows * n), ptr(d_blk), ptr(d_info), ptr(d_chan), rows, NCH, NTAPS,
                                        mbs, sp) == 0

    asks = [("k_dec_ltm, LDS = the block", n)] + ([("k_dec_ltm, LDS of a default handle (16384 samples)", 16384)] if n <= 16384 else []) \
        + ([("k_dec_ltm, the whole LDS budget (40896 samples)", LDS_SAMPLES)] if n < LDS_SAMPLES else []) \
        + [("k_dec_ltm_far", LDS_SAMPLES + 1)]
    outs, row = [], {"block_samples": n, "blocks": rows, "channels": NCH, "taps": NTAPS, "runs": []}
    for name, mbs in asks:
        fresh = d_x.clone()
        run(mbs, fresh)
        torch.cuda.synchronize()
        outs.append(fresh)
        ms, all_ms = step(lambda: median_ms(lambda: run(mbs)))
        row["runs"].append({"kernel": name, "max_block_samples": mbs, "median_ms": round(ms, 4), "all_ms": all_ms,
                            "gsamples_per_s": round(NCH * rows * n / ms * 1e-6, 3)})
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and not torch.equal(outs[0], d_x)
    kernels.append(row)

# ---- (b) the resident decode of one file, long blocks against ordinary ones
pcm = W.music_like(2, 140000, 16, seed=3)
streams = {}
for max_block in (65535, 16384):
    ret, data = S.oracle().encode_whole(S.make_params(2, 16, 48000, 16, 3, 8, 1, 1, max_block, cap=CAP), pcm)
    assert ret == 0
    streams[max_block] = (data, torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda())
RES = ("gathers", "walks", "kernels", "emit", "total", "passes")
decodes, keep = [], {}
for max_block, capacity in ((65535, 65535), (16384, 16384), (16384, 65535)):
    dec = sla_amd.Decoder(8, capacity, 255, 5, 32, long_blocks=capacity > 16384)
    src = streams[max_block][1]

    def decode():
        t, lengths, results = dec.decode_resident_tensor([src], dtype=torch.int32)
        assert results == [0] and lengths == [140000]
        keep["t"] = t

    ms, all_ms = step(lambda: wall_ms(decode))
    assert np.array_equal(keep["t"].cpu().numpy()[0], pcm)                    # lossless: the PCM itself
    decodes.append({"stream_max_block_samples": max_block, "stream_bytes": len(streams[max_block][0]), "handle_capacity": capacity,
                    "long_term_kernel": "k_dec_ltm_far" if capacity > LDS_SAMPLES else "k_dec_ltm",
                    "median_ms": round(ms, 3), "all_ms": all_ms, "split_ms": dict(zip(RES, [round(v, 3) for v in dec.last_timing()]))})
    dec.close()

report = {"device": sla_amd.device_name(), "warmups": WARM, "reps": REPS, "window_samples": int(L.sla_hip_dec_ltm_window()),
          "kernels_on_identical_tables": kernels, "decode_resident_tensor_140000_samples": decodes, "all_results_equal": True}
print(json.dumps(report, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(report, fh, indent=1)
    fh.write("\n")
