"""The long-block partition search with 64-tile sums (option "long_tile_search") beside the far chains, in one process.
 (a) SLAEncoder_EncodeWhole of the 120 s 16-bit stereo file (48 kHz) of tests/tools/bench_long_enc.py at max_num_block_samples
     65535 with the option 0 and 1: wall time, the analysis and its search stage (sla_hip_last_timing [7], [1]), the groups rerun;
     and sla_hip_launch_search_far_x on its own over the same file's (super-frame, channel) groups: the whole launch between two
     events, k_search_finish_far by its execution span (extra->d_span), the tile sums as the difference.
 (b) the same for a 120 s 24-bit stereo file at ordinary loudness (waveforms.music_like), where every group is over the
     exactness limit and reruns as chains: what the tile sums cost where they are of no use.
Both routes must give the same bytes in every repetition, and the bytes must decode to the PCM.
Every step: 2 warm-ups, then the median of 5 (and the spread, max - min, of the 5), under a time limit of its own.
usage: python tests/tools/bench_long_search.py [out.json]"""
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
import waveforms as W
import longsearchmodel as M

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "long_search.json")
WARM, REPS, STEP_LIMIT = 2, 5, 240
CAP = (8, 65535, 255, 5, 32)
ORDER, MAXB, SECONDS = 16, 65535, 120


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


def med(v):
    return round(float(np.median(v)), 4)


def spread(v):
    return round(float(max(v) - min(v)), 4)


class Group(C.Structure):                      # sla_hip_lpc_group
    _fields_ = [("pcm_off", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "num_samples", "channel", "win_off", "int_shift", "cand_first", "cand_count", "slot_first", "pad_")]


class Extra(C.Structure):                      # sla_hip_launch_extra
    _fields_ = [("d_span", C.c_void_p), ("d_group_count", C.c_void_p), ("clear_ptr", C.c_void_p * 3), ("clear_words", C.c_uint32 * 3),
                ("d_rice_init", C.c_void_p)]


L = sla_amd.lib()
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
gdev = lambda gs: torch.frombuffer(bytearray(b"".join(bytes(g) for g in gs)), dtype=torch.uint8).cuda()


def encode_rows(pcm, bits):
    """the file through EncodeWhole with the option 0 and 1 on one handle each, alternating after the warm-ups"""
    encs, rows, seen = [], [], [[], []]
    for opt in (0, 1):
        e = sla_amd.Encoder(*CAP, long_blocks=True)
        e.set_option("long_tile_search", opt)
        e.set_wave_format(2, bits, 48000)
        e.set_encode_parameter(ORDER, 3, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, MAXB)
        encs.append(e)
    wall, timings = [[], []], [[], []]

    def encode(opt):
        t0 = time.perf_counter()
        seen[opt].append(encs[opt].encode_whole(pcm))
        wall[opt].append((time.perf_counter() - t0) * 1e3)
        timings[opt].append(encs[opt].last_timing())

    def run():
        for _ in range(WARM + REPS):
            encode(0)
            encode(1)
    step(run, limit=900)
    assert all(s == seen[0][0] for s in seen[0] + seen[1])          # the two routes: the same bytes, every time
    dec = sla_amd.Decoder(*CAP, long_blocks=True)
    rc, back = dec.decode_whole(seen[0][0], pcm.shape[1])
    dec.close()
    assert rc == 0 and np.array_equal(back, pcm)
    for opt in (0, 1):
        t = np.array(timings[opt][WARM:])
        cnt = encs[opt].last_counters()
        rows.append({"long_tile_search": opt, "file_bytes": len(seen[opt][0]),
                     "encode_whole_median_ms": med(wall[opt][WARM:]), "encode_whole_spread_ms": spread(wall[opt][WARM:]),
                     "analysis_median_ms": med(t[:, 7]), "analysis_spread_ms": spread(t[:, 7]),
                     "search_median_ms": med(t[:, 1]), "search_spread_ms": spread(t[:, 1]), "search_all_ms": [round(float(x), 4) for x in t[:, 1]],
                     "tile_sums_used": int(cnt[2]), "groups_rerun_as_chains": int(cnt[0])})
        encs[opt].close()
    return rows


def launcher_row(pcm, bits, ms):
    """sla_hip_launch_search_far_x alone over the file's groups, at the limit of exact_bits 53"""
    frames = M.super_frames(pcm, MAXB)
    cands, first = [], {}
    for _, w in frames:
        if w not in first:
            first[w] = (len(cands), len(M.grid(w)))
            cands += M.grid(w)
    groups, slot = [], 0
    for s, w in frames:
        for ch in range(2):
            groups.append(Group(s, w, ch, 0xFFFFFFFF, 32 - bits, first[w][0], first[w][1], slot, 0))
            slot += first[w][1]
    lags = L.sla_hip_search_exact_lags(ORDER)
    d_pcm, d_g, d_c = dev(pcm), gdev(groups), dev(np.array(cands, np.uint32))
    d_ts = torch.zeros(len(groups) * 64 * 2 * lags, dtype=torch.float64, device="cuda")
    d_out = torch.zeros(slot * (ORDER + 2), dtype=torch.float64, device="cuda")
    d_span = torch.zeros(2, dtype=torch.int64, device="cuda")
    x = Extra()
    x.d_span = d_span.data_ptr()
    limit = 2.0 ** (53 + 2 * (M.ntz_of(pcm) - 31 - ms))
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    whole, finish = [], []

    def run():
        for i in range(WARM + REPS):
            d_span.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = L.sla_hip_launch_search_far_x(ptr(d_pcm), pcm.shape[1], ms, ORDER, ptr(d_g), len(groups), MAXB, max(n for _, n in first.values()),
                                               ptr(d_c), ptr(d_ts), ptr(d_out), limit, sp, C.cast(C.byref(x), C.c_void_p))
            e1.record()
            e1.synchronize()
            assert rc == 0, rc
            if i >= WARM:
                s = d_span.cpu().numpy().view(np.uint64)
                whole.append(e0.elapsed_time(e1))
                finish.append(float(int(s[1]) - int(~s[0])) / 1e5)          # the device's constant 100 MHz clock
    step(run)
    flagged = int(torch.isnan(d_out.view(-1, ORDER + 2)[:, 0]).sum().item())
    return {"groups": len(groups), "candidate_slots": slot, "order": ORDER, "mid_side": ms, "flagged_slots": flagged,
            "launch_median_ms": med(whole), "launch_spread_ms": spread(whole),
            "finish_kernel_median_ms": med(finish), "finish_kernel_spread_ms": spread(finish),
            "tile_sums_median_ms": med([w - f for w, f in zip(whole, finish)])}


report = {"device": None, "warmups": WARM, "reps": REPS, "max_num_block_samples": MAXB, "order": ORDER, "seconds": SECONDS}
pcm16 = S.synth_pcm(2, SECONDS * 48000, 16, 48000)
report["a_stereo_16bit"] = {"encode_whole": encode_rows(pcm16, 16), "search_far_launcher": launcher_row(pcm16, 16, 1)}
pcm24 = W.music_like(2, SECONDS * 48000, 24, seed=7)
report["b_stereo_24bit_music_like"] = {"encode_whole": encode_rows(pcm24, 24), "search_far_launcher": launcher_row(pcm24, 24, 1)}
for key in ("a_stereo_16bit", "b_stereo_24bit_music_like"):
    off, on = report[key]["encode_whole"]
    report[key]["search_off_minus_on_ms"] = round(off["search_median_ms"] - on["search_median_ms"], 4)
    report[key]["three_spreads_ms"] = round(3 * max(off["search_spread_ms"], on["search_spread_ms"]), 4)
report["device"] = sla_amd.device_name()
report["all_results_equal"] = True
print(json.dumps(report, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(report, fh, indent=1)
    fh.write("\n")
