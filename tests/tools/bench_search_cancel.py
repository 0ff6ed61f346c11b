"""cost of a cancelled early start (option "search_early"): C3's synthetic signal, --seconds long, device
resident; file A as it is, file B with one second of zeros written over its start.  Calls alternate A, B, A, B ... on one
handle, so that every B follows a file without silence and starts its search beside the prepass -- which the prepass then
cancels.  Prints ms per call of A and of B (median, mean, max over --reps pairs), the prepass stage time and the counters.
Run it once per build (SLA_HIP_LIB names another libsla_hip.so) and compare the B rows: the new build may be slower there
by at most the parent's prepass time, which is all the work that can have been started in vain.

    python tests/tools/bench_search_cancel.py [--seconds 600] [--reps 8] [search_early=0 ...]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np
import torch
import bench as B
import sla_amd

args = sys.argv[1:]
seconds, reps = 600.0, 8
opts = []
while args:
    a = args.pop(0)
    if a == "--seconds":
        seconds = float(args.pop(0))
    elif a == "--reps":
        reps = int(args.pop(0))
    elif "=" in a:
        opts.append(a.split("="))
nch, bits, rate, _, order, ltm, lms, ms, win, maxb, cap = B.CONFIGS["C3"]
n = int(rate * seconds)
stride = (n + 63) // 64 * 64
plain = torch.zeros((nch, stride), dtype=torch.int32, device="cuda")
plain[:, :n] = B.synth_device(torch, nch, n, bits, rate, 0, n)
silent = plain.clone()
silent[:, :rate] = 0
enc = sla_amd.Encoder(*cap)
enc.set_wave_format(nch, bits, rate)
enc.set_encode_parameter(order, ltm, lms, ms, win, maxb)
for k, v in opts:
    enc.set_option(k, float(v))
d_lat = torch.zeros((nch, stride), dtype=torch.int32, device="cuda")
d_fin = torch.zeros((nch, stride), dtype=torch.int32, device="cuda")
enc.bind_residual_planes(d_lat.data_ptr(), d_fin.data_ptr(), stride)
torch.cuda.synchronize()
for _ in range(3):
    enc.analyze_device(plain.data_ptr(), stride, n)
    enc.analyze_device(silent.data_ptr(), stride, n)
t = {"plain": [], "silent": []}
prepass = {"plain": [], "silent": []}
for _ in range(reps):
    for name, buf in (("plain", plain), ("silent", silent)):
        t0 = time.perf_counter()
        tm = enc.analyze_device(buf.data_ptr(), stride, n)
        t[name].append((time.perf_counter() - t0) * 1e3)
        prepass[name].append(tm[0])
early = enc.last_search_early() if hasattr(sla_amd.lib(), "sla_hip_last_search_early") else None
for name in ("plain", "silent"):
    v = np.array(t[name])
    print("C3 %.0f s %s %-6s ms per call: median %.3f mean %.3f max %.3f; prepass stage %.3f ms; expand %s; early %s"
          % (seconds, opts, name, np.median(v), v.mean(), v.max(), float(np.median(prepass[name])), enc.last_expand(), early), flush=True)
