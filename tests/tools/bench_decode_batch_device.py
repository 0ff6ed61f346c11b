"""Decode side of BASELINE C4 into device memory: 125 ten-second stereo clips (48 kHz 16-bit, order 16, MS, 4096-sample
blocks) encoded with encode_batch, as tests/tools/bench_decode_batch.py builds them, then turned into one float32
[125][2][480000] device tensor two ways:
  (a) what a user does without the device path: decode_batch into pageable numpy planes, torch.from_numpy(...).cuda()
      and the float conversion (left * 2^-31);
  (b) decode_batch_tensor(float32): sla_hip_decode_batch_device, the emit kernel writing the tensor.
Each is repeated; the median is reported with the handle's last_timing split (upload, walk, kernels, download or emit,
total [ms]; passes), and (b) must equal (a) bit for bit.
usage: python tests/tools/bench_decode_batch_device.py [clips] [reps] [out.json]"""
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

clips = int(sys.argv[1]) if len(sys.argv) > 1 else 125
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None
n = 480000
base = [S.synth_pcm(2, n, 16, 48000, seed=100 + i) for i in range(8)]
pcms = [base[i % 8] for i in range(clips)]

enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
enc.set_wave_format(2, 16, 48000)
enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
res = enc.encode_batch(pcms)
enc.close()
assert all(rc == 0 for rc, _ in res)
datas = [np.frombuffer(d, np.uint8) for _, d in res]

dec = sla_amd.Decoder(2, 4096, 16, 1, 8)
host = np.zeros((clips, 2, n), np.int32)                             # pageable, touched once before timing
outs = [host[i] for i in range(clips)]
result = {}


def via_host():
    got = dec.decode_batch(datas, outs=outs)
    assert all(rc == 0 and o.shape[1] == n for rc, o in got)
    result["a"] = torch.from_numpy(host).cuda().float().mul_(2.0 ** -31)


def via_device():
    t, lengths, results = dec.decode_batch_tensor(datas, dtype=torch.float32)
    assert results == [0] * clips and lengths == [n] * clips
    result["b"] = t


def timed(fn):
    fn()                                                             # warm-up: device buffers, staging, code objects
    t, split = [], []
    for _ in range(reps):
        result.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
        split.append(dec.last_timing())
    k = int(np.argsort(t)[len(t) // 2])
    return float(np.median(t)), t, split[k]


a_ms, a_all, a_split = timed(via_host)
a = result["a"]
b_ms, b_all, b_split = timed(via_device)
b = result["b"]
exact = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
exact_pcm = all(np.array_equal(host[i], pcms[i]) for i in range(clips))
msamples = clips * n / 1e6
report = {
    "device": sla_amd.device_name(), "clips": clips, "samples_per_clip": n, "channels": 2, "reps": reps,
    "tensor_bytes": clips * 2 * n * 4, "exact_b_equals_a": exact, "exact_a_equals_pcm": exact_pcm,
    "a_decode_batch_numpy_upload_convert": {
        "median_ms": round(a_ms, 2), "all_ms": [round(x, 2) for x in a_all], "msamples_per_s": round(msamples / (a_ms / 1e3), 1),
        "decode_batch_split_ms": {"upload": a_split[0], "walk": a_split[1], "kernels": a_split[2], "download": a_split[3],
                                  "total": a_split[4], "passes": a_split[5]}},
    "b_decode_batch_tensor_f32": {
        "median_ms": round(b_ms, 2), "all_ms": [round(x, 2) for x in b_all], "msamples_per_s": round(msamples / (b_ms / 1e3), 1),
        "split_ms": {"upload": b_split[0], "walk": b_split[1], "kernels": b_split[2], "emit": b_split[3],
                     "total": b_split[4], "passes": b_split[5]}},
    "speedup": round(a_ms / b_ms, 2),
}
print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
dec.close()
assert exact and exact_pcm
