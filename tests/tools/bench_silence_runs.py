"""What option "silence_runs" buys on input with silence and costs on input without: the analysis
call on device-resident planes with the option 0 and 1024, interleaved in one process on two handles that differ in that
option only, after a warm-up of both; medians, minima and the spread of every arm, host clock around the call (which ends
with the stream idle) and the sum of the call's device-event stage times.

  C4   125 ten-second stereo clips (48 kHz 16-bit, MS, order 16, 4096-sample blocks), sla_hip_analyze_batch_device
         lead_in   25 of them begin with 0.5 s of digital silence
         clean     none does (no sample is zero in every channel over a whole mask word ... as the signal has it)
  C2   one ten-minute mono file (48 kHz 16-bit, order 16), sla_hip_analyze_device
         pauses    about 40 pauses of 0.1 .. 1 s
         clean     none

The library can be swapped with SLA_HIP_LIB (a build of the parent commit: `--off-only` then times the option-off arm alone,
since that build has no such option) for the claim "option 0 is the parent" in the same session.
usage: python tests/tools/bench_silence_runs.py [--reps R] [--clips N] [--off-only] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch
torch.cuda.init()
import sla_amd
import slalibs as S


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, clips = arg("--reps", 9), arg("--clips", 125)
off_only = "--off-only" in sys.argv
flags_with_value = ("--reps", "--clips")
rest = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags_with_value]
out_path = rest[0] if rest else None
ARMS = (0,) if off_only else (0, 1024)


def stats(t):
    t = sorted(t)
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
            "all_ms": [round(v, 4) for v in t]}


def ab(make, call):
    """call(enc) on an option-off and an option-on handle, alternating, after two warm-ups of each; the block tables of the
    arms must agree"""
    encs, tables = {}, {}
    for v in ARMS:
        encs[v] = make()
        if v:
            encs[v].set_option("silence_runs", v)
    for v in ARMS:
        call(encs[v]); call(encs[v])
        tr = encs[v].trace(want_residuals=False)
        nb = tr.num_blocks
        tables[v] = (nb, tr.blk_type[:nb].tobytes(), tr.blk_start[:nb].tobytes(), tr.blk_nsmpl[:nb].tobytes())
    wall, dev = {v: [] for v in ARMS}, {v: [] for v in ARMS}
    for _ in range(reps):
        for v in ARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            timing = call(encs[v])
            wall[v].append((time.perf_counter() - t0) * 1e3)
            dev[v].append(float(timing[7]))
    res = {"off": {"wall": stats(wall[0]), "call_ms": stats(dev[0])}}
    if len(ARMS) > 1:
        on = ARMS[1]
        assert tables[0] == tables[on], "the option changed the block table"
        res["on"] = {"wall": stats(wall[on]), "call_ms": stats(dev[on])}
        res["on_minus_off_wall_median_ms"] = round(res["on"]["wall"]["median_ms"] - res["off"]["wall"]["median_ms"], 4)
        res["off_spread_ms"] = round(res["off"]["wall"]["max_ms"] - res["off"]["wall"]["min_ms"], 4)
        res["silence_on"] = list(encs[on].last_silence())
    if hasattr(encs[0], "last_silence") and hasattr(sla_amd.lib(), "sla_hip_last_silence"):
        res["silence_off"] = list(encs[0].last_silence())
    res["blocks"] = tables[0][0]
    for e in encs.values():
        e.close()
    return res


report = {"device": sla_amd.device_name(), "library": sla_amd.LIB_PATH, "reps": reps}

# ---- C4: a batch of clips --------------------------------------------------------------------------------------------
n = 480000
base = []
for i in range(8):
    x = S.synth_pcm(2, n, 16, 48000, seed=100 + i)
    x[0, ~(x != 0).any(axis=0)] = 1 << 16                    # no accidental digital silence: the cases put it in
    base.append(x)
stride = (n + 1023) // 1024 * 1024
starts = [i * stride for i in range(clips)]
lens = [n] * clips
span = stride * clips


def planes_c4(lead_in):
    d = torch.zeros((2, span), dtype=torch.int32, device="cuda")
    for i in range(clips):
        d[:, starts[i]:starts[i] + n] = torch.from_numpy(base[i % 8]).cuda()
        if lead_in and i % 5 == 0:
            d[:, starts[i]:starts[i] + 24000] = 0
    torch.cuda.synchronize()
    return d


def make_c4():
    enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
    enc.set_wave_format(2, 16, 48000)
    enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
    enc.num_channels, enc.order, enc.ltm_order = 2, 16, 1
    return enc


c4 = {"clips": clips, "samples_per_clip": n, "mask_bytes": span // 8}
for name, lead in (("lead_in", True), ("clean", False)):
    d = planes_c4(lead)
    c4[name] = ab(make_c4, lambda enc: enc.analyze_batch_device(d.data_ptr(), span, span, starts, lens)[0])
    del d
report["C4"] = c4

# ---- C2: one long mono file ------------------------------------------------------------------------------------------
N = 600 * 48000
mono = S.synth_pcm(1, N, 16, 48000, seed=7)
mono[0, mono[0] == 0] = 1 << 16
rng = np.random.default_rng(11)
pauses = sorted(int(v) for v in rng.integers(48000, N - 96000, size=40))


def planes_c2(with_pauses):
    d = torch.from_numpy(mono).cuda()
    if with_pauses:
        for at in pauses:
            d[:, at:at + int(rng.integers(4800, 48001))] = 0
    torch.cuda.synchronize()
    return d


def make_c2():
    enc = sla_amd.Encoder(1, 4096, 16, 1, 8)
    enc.set_wave_format(1, 16, 48000)
    enc.set_encode_parameter(16, 1, 8, sla_amd.CH_NONE, sla_amd.WINDOW_SIN, 4096)
    enc.num_channels, enc.order, enc.ltm_order = 1, 16, 1
    return enc


c2 = {"samples": N, "mask_bytes": N // 8}
for name, p in (("pauses", True), ("clean", False)):
    d = planes_c2(p)
    c2[name] = ab(make_c2, lambda enc: enc.analyze_device(d.data_ptr(), N, N))
    del d
report["C2"] = c2

print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
