"""The far-window LPC stage beside the LDS kernel, and the encoder at maxima of 16384 and 65535, in one process.
 (a) sla_hip_launch_lpc_far against sla_hip_launch_lpc on the same 16384-sample windows (the longest both take), order 16:
     search form -- 32 groups (16 super-frames of a stereo file) with the 120 candidates of a 17-node grid each -- and block
     form -- 64 windowed groups of one candidate.  The outputs of both launchers must be equal, word for word.
 (b) SLAEncoder_EncodeWhole of one 120 s 16-bit stereo file (48 kHz) on a capacity-65535 handle at max_num_block_samples of
     16384 (the ordinary routes) and 65535 (the long-block routes): wall time, the stage timings of the analysis
     (sla_hip_last_timing: [1] search, [2] block LPC -- the two stages the far kernels serve --, [7] the whole analysis), file
     sizes.  Every repetition must give the same bytes, and the bytes must decode to the PCM.
Every step: 2 warm-ups, then the median of 5, under a time limit of its own.
usage: python tests/tools/bench_long_enc.py [out.json]"""
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "long_enc.json")
WARM, REPS, STEP_LIMIT = 2, 5, 240
CAP = (8, 65535, 255, 5, 32)
ORDER, WINDOW = 16, 16384


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


class Group(C.Structure):                      # sla_hip_lpc_group
    _fields_ = [("pcm_off", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


L = sla_amd.lib()
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
gdev = lambda gs: torch.frombuffer(bytearray(b"".join(bytes(g) for g in gs)), dtype=torch.uint8).cuda()

# ---- (a) the launchers on identical tables
frames = 16
pcm = S.synth_pcm(2, frames * WINDOW, 16, 48000)
d_pcm = dev(pcm)
nodes = WINDOW // 1024 + 1
grid = [(p * 1024, (q - p) * 1024) for p in range(nodes) for q in range(p + 2, nodes)]
tables = {
    "search": ([Group(f * WINDOW, WINDOW, ch, 0xFFFFFFFF, 16, 0, len(grid), (2 * f + ch) * len(grid), 0) for f in range(frames) for ch in range(2)],
               grid, len(grid), None),
    "block": ([Group((g // 2) % frames * WINDOW, WINDOW, g % 2, 0, 16, g, 1, g, 0) for g in range(64)], [(0, WINDOW)] * 64, 1,
              S.oracle().window(1, WINDOW)),
}
kernels = []
for form, (groups, cands, per_group, pool) in tables.items():
    nslots = len(groups) * per_group
    d_g, d_c, d_w = gdev(groups), dev(np.array(cands, np.uint32)), (dev(pool) if pool is not None else None)
    d_scr = torch.zeros(64 * WINDOW, dtype=torch.float64, device="cuda")
    block = pool is not None
    outs = {}

    def run(far, bufs):
        o, c, k, r = bufs
        if far:
            rc = L.sla_hip_launch_lpc_far(ptr(d_pcm), C.c_uint64(pcm.shape[1]), 1, ORDER, ptr(d_g), len(groups), WINDOW, per_group, ptr(d_c),
                                          ptr(d_w), ptr(o), ptr(c), ptr(k), ptr(r), ptr(d_scr), 64, sp)
        else:
            rc = L.sla_hip_launch_lpc(ptr(d_pcm), C.c_uint64(pcm.shape[1]), 1, ORDER, ptr(d_g), len(groups), WINDOW, per_group, ptr(d_c),
                                      ptr(d_w), ptr(o), ptr(c), ptr(k), ptr(r), sp)
        assert rc == 0, rc

    row = {"form": form, "window_samples": WINDOW, "order": ORDER, "groups": len(groups), "candidates_per_group": per_group, "mid_side": 1,
           "runs": []}
    for far in (False, True):
        bufs = (torch.zeros(nslots * (ORDER + 2), dtype=torch.float64, device="cuda"),
                torch.zeros(nslots * (ORDER + 1), dtype=torch.int32, device="cuda") if block else None,
                torch.zeros(nslots * (ORDER + 1), dtype=torch.int32, device="cuda") if block else None,
                torch.zeros(nslots, dtype=torch.int32, device="cuda") if block else None)
        ms, all_ms = step(lambda: median_ms(lambda: run(far, bufs)))
        torch.cuda.synchronize()
        outs[far] = [b.cpu().numpy().view(np.uint8) for b in bufs if b is not None]
        row["runs"].append({"launcher": "sla_hip_launch_lpc_far" if far else "sla_hip_launch_lpc", "median_ms": round(ms, 4), "all_ms": all_ms})
    assert all(np.array_equal(a, b) for a, b in zip(outs[False], outs[True])) and outs[True][0].any()
    row["far_over_lds"] = round(row["runs"][1]["median_ms"] / row["runs"][0]["median_ms"], 2)
    kernels.append(row)

# ---- (b) one 120 s stereo file at both maxima
SECONDS = 120
pcm = S.synth_pcm(2, SECONDS * 48000, 16, 48000)
enc = sla_amd.Encoder(*CAP, long_blocks=True)
dec = sla_amd.Decoder(*CAP, long_blocks=True)
enc.set_wave_format(2, 16, 48000)
encodes = []
for max_block in (16384, 65535):
    enc.set_encode_parameter(16, 3, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, max_block)
    seen, wall, timings = [], [], []

    def encode():
        t0 = time.perf_counter()
        seen.append(enc.encode_whole(pcm))
        wall.append((time.perf_counter() - t0) * 1e3)
        timings.append(enc.last_timing())

    step(lambda: [encode() for _ in range(WARM + REPS)], limit=600)
    assert all(s == seen[0] for s in seen)
    rc, back = dec.decode_whole(seen[0], pcm.shape[1])
    assert rc == 0 and np.array_equal(back, pcm)
    t = np.median(np.array(timings[WARM:]), axis=0)
    encodes.append({"max_num_block_samples": max_block, "seconds": SECONDS, "samples_per_channel": int(pcm.shape[1]), "file_bytes": len(seen[0]),
                    "encode_whole_median_ms": round(float(np.median(wall[WARM:])), 3), "encode_whole_all_ms": [round(x, 3) for x in wall[WARM:]],
                    "analysis_ms": round(float(t[7]), 3), "search_ms": round(float(t[1]), 3), "block_lpc_ms": round(float(t[2]), 3),
                    "lattice_ms": round(float(t[3]), 3), "long_term_ms": round(float(t[8]), 3), "tail_ms": round(float(t[4]), 3),
                    "search_and_block_lpc_share_of_analysis": round(float((t[1] + t[2]) / t[7]), 3) if t[7] > 0 else None,
                    "block_cert": enc.last_block_cert()[0], "device_plan": enc.last_counters()[3]})
enc.close()
dec.close()

report = {"device": sla_amd.device_name(), "warmups": WARM, "reps": REPS, "launchers_on_identical_tables": kernels,
          "encode_whole_120s_stereo_16bit": encodes, "all_results_equal": True}
print(json.dumps(report, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(report, fh, indent=1)
    fh.write("\n")
