"""Encode side of BASELINE C4 from device memory: 125 ten-second stereo clips (48 kHz 16-bit, MS, order 16, 4096-sample
blocks) resident as one int16 [125][2][480000] device tensor, encoded to .sla bytes two ways:
  (a) what a user does without the device path: x.cpu().numpy(), << 16 to left-justified int32 planes, encode_batch (worker
      lanes on, the default);
  (b) encode_batch_tensor(x): sla_hip_encode_batch_device, the ingest kernel reading the tensor.
Each is repeated; the median is reported with its split -- (a) the device-to-host copy, the numpy conversion and
encode_batch, timed on the host; (b) the library's stamps of one more call on a handle created with SLA_HIP_TRACE=1
(ingest + prepass, analysis, pack + download) -- and (b) must equal (a) byte for byte for every clip.
usage: python tests/tools/bench_encode_batch_device.py [clips] [reps] [out.json] [--only-b]
(--only-b: path (b) alone, warm-up + reps, for a profiler run)"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch
torch.cuda.init()
import sla_amd
import slalibs as S

only_b = "--only-b" in sys.argv
args = [a for a in sys.argv[1:] if a != "--only-b"]
clips = int(args[0]) if len(args) > 0 else 125
reps = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else None
n = 480000
base = [(S.synth_pcm(2, n, 16, 48000, seed=100 + i) >> 16).astype(np.int16) for i in range(8)]
x = torch.empty((clips, 2, n), dtype=torch.int16, device="cuda")
for i in range(clips):
    x[i].copy_(torch.from_numpy(base[i % 8]))
torch.cuda.synchronize()


def make():
    enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
    enc.set_wave_format(2, 16, 48000)
    enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
    return enc


enc = make()
result, split = {}, {}


def via_host():
    t0 = time.perf_counter()
    h = x.cpu().numpy()
    t1 = time.perf_counter()
    planes = h.astype(np.int32) << 16
    t2 = time.perf_counter()
    res = enc.encode_batch([planes[i] for i in range(clips)])
    t3 = time.perf_counter()
    assert all(rc == 0 for rc, _ in res)
    result["a"] = res
    split["a"] = {"device_to_host": (t1 - t0) * 1e3, "numpy_convert": (t2 - t1) * 1e3, "encode_batch": (t3 - t2) * 1e3}


def via_device():
    res = enc.encode_batch_tensor(x)
    assert all(rc == 0 for rc, _ in res)
    result["b"] = res


def timed(fn, key):
    fn()                                                             # warm-up: device buffers, staging, code objects
    t, parts = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
        parts.append(split.get(key))
    k = int(np.argsort(t)[len(t) // 2])
    return float(np.median(t)), t, parts[k]


def traced_call():
    """one call of (b) on a handle created with SLA_HIP_TRACE=1; its stderr lines of the device batch"""
    os.environ["SLA_HIP_TRACE"] = "1"
    traced = make()
    del os.environ["SLA_HIP_TRACE"]
    traced.encode_batch_tensor(x)                                    # warm-up
    with tempfile.TemporaryFile(mode="w+") as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            traced.encode_batch_tensor(x)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        lines = [ln.strip() for ln in f if "encode_batch_device" in ln]
    traced.close()
    return lines


msamples = clips * n / 1e6
if only_b:
    b_ms, b_all, _ = timed(via_device, "b")
    print(json.dumps({"clips": clips, "b_median_ms": round(b_ms, 2), "b_all_ms": [round(v, 2) for v in b_all]}))
    enc.close()
    sys.exit(0)
a_ms, a_all, a_split = timed(via_host, "a")
a = result["a"]
b_ms, b_all, _ = timed(via_device, "b")
b = result["b"]
exact = len(a) == len(b) == clips and all(ra == rb for ra, rb in zip(a, b))
trace = traced_call()
report = {
    "device": sla_amd.device_name(), "clips": clips, "samples_per_clip": n, "channels": 2, "reps": reps,
    "tensor_bytes": clips * 2 * n * 2, "sla_bytes": sum(len(d) for _, d in b), "exact_b_equals_a": exact,
    "a_cpu_numpy_encode_batch": {
        "median_ms": round(a_ms, 2), "all_ms": [round(v, 2) for v in a_all], "msamples_per_s": round(msamples / (a_ms / 1e3), 1),
        "split_ms": {k: round(v, 2) for k, v in a_split.items()}},
    "b_encode_batch_tensor_s16": {
        "median_ms": round(b_ms, 2), "all_ms": [round(v, 2) for v in b_all], "msamples_per_s": round(msamples / (b_ms / 1e3), 1),
        "trace": trace},
    "speedup": round(a_ms / b_ms, 2),
}
print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
enc.close()
assert exact
