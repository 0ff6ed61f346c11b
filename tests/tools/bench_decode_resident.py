"""Decode side of BASELINE C4 from streams that are already in device memory: the 125 ten-second stereo clips of
tests/tools/bench_decode_batch_device.py (48 kHz 16-bit, order 16, MS, 4096-sample blocks), turned into one float32
[125][2][480000] device tensor two ways, in one process:
  (a) decode_batch_tensor(float32) from the bytes in host memory: sla_hip_decode_batch_device, the yardstick;
  (b) decode_resident_tensor(float32) from the same bytes resident on the device (slices of one uint8 tensor at odd
      offsets): sla_hip_decode_batch_resident -- no staging, no upload, a gather and two walks instead;
and (c) the resident call on ONE long file (default 600 s, about 7000 blocks), which puts a number on the serial walk.
Each is repeated; the median is reported with the handle's last_timing split, and (b) must equal (a) bit for bit.
usage: python tests/tools/bench_decode_resident.py [clips] [reps] [out.json] [long_seconds]"""
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
long_seconds = int(sys.argv[4]) if len(sys.argv) > 4 else 600
n = 480000
base = [S.synth_pcm(2, n, 16, 48000, seed=100 + i) for i in range(8)]
pcms = [base[i % 8] for i in range(clips)]
minute = S.synth_pcm(2, 60 * 48000, 16, 48000, seed=77)
long_pcm = np.ascontiguousarray(np.tile(minute, (1, (long_seconds + 59) // 60))[:, :long_seconds * 48000])

enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
enc.set_wave_format(2, 16, 48000)
enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
res = enc.encode_batch(pcms)
assert all(rc == 0 for rc, _ in res)
datas = [np.frombuffer(d, np.uint8) for _, d in res]
long_data = np.frombuffer(enc.encode_whole(long_pcm), np.uint8)
enc.close()


def resident(files):
    """the files as slices of one uint8 device tensor, each at an odd offset"""
    offs, pos = [], 1
    for d in files:
        offs.append(pos)
        pos += len(d) + (1 if (pos + len(d)) % 2 == 0 else 2)
    host = np.zeros(pos, np.uint8)
    for d, o in zip(files, offs):
        host[o:o + len(d)] = d
    dev = torch.from_numpy(host).cuda()
    return [dev[o:o + len(d)] for d, o in zip(files, offs)], dev


srcs, corpus = resident(datas)
long_srcs, long_corpus = resident([long_data])
dec = sla_amd.Decoder(2, 4096, 16, 1, 8)
result = {}


def from_host():
    t, lengths, results = dec.decode_batch_tensor(datas, dtype=torch.float32)
    assert results == [0] * clips and lengths == [n] * clips
    result["t"] = t


def from_device():
    t, lengths, results = dec.decode_resident_tensor(srcs, dtype=torch.float32)
    assert results == [0] * clips and lengths == [n] * clips
    result["t"] = t


def long_file():
    t, lengths, results = dec.decode_resident_tensor(long_srcs, dtype=torch.float32)
    assert results == [0] and lengths == [long_pcm.shape[1]]
    result["t"] = t


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


def entry(ms, all_ms, split, names, msamples):
    return {"median_ms": round(ms, 2), "all_ms": [round(x, 2) for x in all_ms], "msamples_per_s": round(msamples / (ms / 1e3), 1),
            "split_ms": dict(zip(names, split))}


HOST = ("upload", "walk", "kernels", "emit", "total", "passes")
RES = ("gathers", "walks", "kernels", "emit", "total", "passes")
a_ms, a_all, a_split = timed(from_host)
a = result["t"]
b_ms, b_all, b_split = timed(from_device)
b = result["t"]
exact = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
exact_pcm = all(bool(torch.equal(b[i].cpu().view(torch.int32), torch.from_numpy(
    (pcms[i].astype(np.float32) * np.float32(2.0 ** -31)).view(np.int32)))) for i in range(0, clips, 16))
del a, b
result.clear()
c_ms, c_all, c_split = timed(long_file)
c = result["t"]
exact_long = bool(torch.equal(c[0].cpu().view(torch.int32), torch.from_numpy(
    (long_pcm.astype(np.float32) * np.float32(2.0 ** -31)).view(np.int32))))
long_blocks = (long_pcm.shape[1] + 4095) // 4096
report = {
    "device": sla_amd.device_name(), "clips": clips, "samples_per_clip": n, "channels": 2, "reps": reps,
    "stream_bytes": int(sum(len(d) for d in datas)), "tensor_bytes": clips * 2 * n * 4,
    "exact_b_equals_a": exact, "exact_b_equals_pcm": exact_pcm,
    "a_decode_batch_tensor_f32_host_bytes": entry(a_ms, a_all, a_split, HOST, clips * n / 1e6),
    "b_decode_resident_tensor_f32": entry(b_ms, b_all, b_split, RES, clips * n / 1e6),
    "speedup_b_over_a": round(a_ms / b_ms, 2),
    "c_resident_one_long_file": dict(entry(c_ms, c_all, c_split, RES, long_pcm.shape[1] / 1e6), seconds=long_seconds,
                                     stream_bytes=int(len(long_data)), blocks=long_blocks,
                                     walks_us_per_block=round(1e3 * c_split[1] / (2 * long_blocks), 3), exact=exact_long),
}
print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
dec.close()
assert exact and exact_pcm and exact_long
