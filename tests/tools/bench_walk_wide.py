"""The block-chain walk of ONE long resident stream, lane against wide, in one process: sla_hip_launch_dec_walk (one lane,
one dependent load per block) and sla_hip_launch_dec_walk_wide (the whole device: find, scan, pointer doubling) in count
mode on a stream of the long file of tests/tools/bench_decode_resident.py (48 kHz 16-bit stereo, order 16, MS,
4096-sample blocks) cut at block boundaries to a ladder of lengths -- about 0.25, 1, 4, 16 MB and the whole ten minutes,
82 MB -- then Decoder.decode_resident_tensor of the whole file with the handle option "wide_walk" off and on, and
Decoder.block_index_resident both ways.  Every step: 2 warm-ups, then the median of 5, under a time limit of its own;
every wide result must equal the lane's, which is the comparison: the lane walk in the same run.
The threshold the handle should default to is the smallest rung at which the wide walk takes at most half the lane walk's
time (half, not break-even: in a batch a file's lane walk runs beside the other files' for free, wide launches add up).
usage: python tests/tools/bench_walk_wide.py [out.json] [long_seconds]"""
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
import slalibs as S
import walkmodel as WM

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "walk_wide.json")
long_seconds = int(sys.argv[2]) if len(sys.argv) > 2 else 600
WARM, REPS, STEP_LIMIT = 2, 5, 120
LADDER_MB = (0.25, 1, 4, 16)


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


# ---- the stream
minute = S.synth_pcm(2, 60 * 48000, 16, 48000, seed=77)
long_pcm = np.ascontiguousarray(np.tile(minute, (1, (long_seconds + 59) // 60))[:, :long_seconds * 48000])
enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
enc.set_wave_format(2, 16, 48000)
enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
long_data = step(lambda: enc.encode_whole(long_pcm), 600)
enc.close()
total = long_pcm.shape[1]
chain = WM.walk(long_data, total, total, 4096)
assert chain.stop == 0 and chain.extent == total
host = np.zeros(len(long_data) + 33, np.uint8)
host[1:1 + len(long_data)] = np.frombuffer(long_data, np.uint8)           # at an odd offset, as a slice of a corpus is
corpus = torch.from_numpy(host).cuda()
L = sla_amd.lib()
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ptr = lambda t: C.c_void_p(t.data_ptr())

# ---- count-mode walks over the ladder
rungs = []
for mb in LADDER_MB:
    k = next((i for i, r in enumerate(chain.rows) if r[0] >= mb * 1e6), None)
    if k is not None and k < chain.num_blocks - 1:
        rungs.append((chain.rows[k][0], chain.rows[k][2], k))                # bytes, samples, blocks of the cut stream
rungs.append((len(long_data), total, chain.num_blocks))
ladder = []
for size, samples, blocks in rungs:
    cap = max(1 << 16, size // 256)
    f = sla_amd.DecWalkFile()
    f.src, f.data_size, f.total, f.capacity = corpus.data_ptr() + 1, size, samples, samples
    d_f = torch.frombuffer(bytearray(bytes(f)), dtype=torch.uint8).cuda()
    d_lane = torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_wide = torch.zeros(16, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(L.sla_hip_dec_wide_scratch_bytes(size, cap), dtype=torch.uint8, device="cuda")

    def lane():
        assert L.sla_hip_launch_dec_walk(ptr(d_f), 1, 4096, 1, ptr(d_lane), None, None, None, sp) == 0

    def wide():
        assert L.sla_hip_launch_dec_walk_wide(C.byref(f), 4096, 1, ptr(d_wide), None, None, None, cap, ptr(scratch), sp) == 0

    lane_ms, lane_all = step(lambda: median_ms(lane))
    wide_ms, wide_all = step(lambda: median_ms(wide))
    got_lane = [int(v) for v in d_lane.cpu().numpy().view("<u4")]
    got_wide = [int(v) for v in d_wide.cpu().numpy().view("<u4")]
    info = [int(v) for v in scratch[:16].cpu().numpy().view("<u4")]
    assert got_lane == [blocks, 0, samples, 0] and got_wide == got_lane, (size, got_lane, got_wide)
    ladder.append({"stream_bytes": size, "blocks": blocks, "nodes": info[0], "decoy_nodes": info[0] - blocks,
                   "rounds": int(L.sla_hip_dec_wide_rounds(size, cap)), "node_capacity": cap,
                   "lane_ms": round(lane_ms, 4), "wide_ms": round(wide_ms, 4), "lane_over_wide": round(lane_ms / wide_ms, 2),
                   "lane_us_per_block": round(1e3 * lane_ms / blocks, 3), "lane_all_ms": lane_all, "wide_all_ms": wide_all})
    del scratch
pays = [r["stream_bytes"] for r in ladder if 2 * r["wide_ms"] <= r["lane_ms"]]

# ---- the resident decode of the whole file, and its index, both ways
src = corpus[1:1 + len(long_data)]
dec = sla_amd.Decoder(2, 4096, 16, 1, 8)
keep = {}
RES = ("gathers", "walks", "kernels", "emit", "total", "passes")


def decode():
    t, lengths, results = dec.decode_resident_tensor([src], dtype=torch.float32)
    assert results == [0] and lengths == [total]
    keep["t"] = t


routes = {}
for name, threshold in (("lane", 0), ("wide", 1)):
    dec.set_option("wide_walk", threshold)
    ms, all_ms = step(lambda: wall_ms(decode), 300)
    routes["decode_" + name] = {"median_ms": round(ms, 2), "all_ms": all_ms, "split_ms": dict(zip(RES, dec.last_timing())),
                                "last_walk": list(dec.last_walk())}
    keep[name] = keep.pop("t")
assert torch.equal(keep["lane"].view(torch.int32), keep["wide"].view(torch.int32))
assert routes["decode_wide"]["last_walk"][:2] == [1, 0]
keep.clear()
index = {}
for name, wide in (("lane", False), ("wide", True)):
    ms, all_ms = step(lambda: wall_ms(lambda: keep.__setitem__("i", dec.block_index_resident([src], wide=wide))), 300)
    routes["index_" + name] = {"median_ms": round(ms, 2), "all_ms": all_ms, "last_walk": list(dec.last_walk())}
    index[name] = keep.pop("i")
assert all(np.array_equal(a, b) for a, b in zip(index["lane"][0][:2], index["wide"][0][:2])) and index["lane"][0][2] == index["wide"][0][2] == 0
assert len(index["lane"][0][0]) == chain.num_blocks
dec.close()

report = {"device": sla_amd.device_name(), "seconds": long_seconds, "warmups": WARM, "reps": REPS, "count_mode_walks": ladder,
          "smallest_rung_where_wide_takes_at_most_half": pays[0] if pays else None, **routes,
          "all_results_equal": True}
print(json.dumps(report, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(report, fh, indent=1)
    fh.write("\n")
