"""Decode side of BASELINE C4: 125 ten-second stereo clips (48 kHz 16-bit, order 16, MS, 4096-sample blocks) encoded
with encode_batch, then decoded (a) one SLADecoder_DecodeWhole per clip on one handle and (b) one sla_hip_decode_batch,
both into the same preallocated pageable numpy planes.  Each is repeated; the median is reported together with the
handle's last_timing split (upload, walk, kernels, download, total [ms]; batches / passes).
usage: python tests/tools/bench_decode_batch.py [clips] [reps]"""
import ctypes as C
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
total_bytes = sum(len(d) for d in datas)

dec = sla_amd.Decoder(2, 4096, 16, 1, 8)
L = sla_amd.lib()
outs = [np.zeros((2, n), np.int32) for _ in range(clips)]          # pageable, touched once before timing
ptrs = [(sla_amd.i32p * 2)(*[o[c].ctypes.data_as(sla_amd.i32p) for c in range(2)]) for o in outs]


def loop():
    got = C.c_uint32(0)
    for i in range(clips):
        rc = L.SLADecoder_DecodeWhole(dec._h, datas[i].ctypes.data_as(sla_amd.u8p), len(datas[i]), ptrs[i], n, C.byref(got))
        assert rc == 0 and got.value == n


def batch():
    got = dec.decode_batch(datas, outs=outs)
    assert all(rc == 0 and o.shape[1] == n for rc, o in got)


def timed(fn):
    fn()                                                             # warm-up: device buffers, staging, code objects
    t, split = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
        split.append(dec.last_timing())
    k = int(np.argsort(t)[len(t) // 2])
    return float(np.median(t)), t, split[k]


loop_ms, loop_all, loop_split = timed(loop)
ok_loop = all(np.array_equal(outs[i], pcms[i]) for i in range(clips))
for o in outs:
    o[:] = 0
batch_ms, batch_all, batch_split = timed(batch)
ok_batch = all(np.array_equal(outs[i], pcms[i]) for i in range(clips))
msamples = clips * n / 1e6
print(json.dumps({
    "device": sla_amd.device_name(), "clips": clips, "samples_per_clip": n, "channels": 2, "stream_bytes": total_bytes,
    "reps": reps, "exact": bool(ok_loop and ok_batch),
    "loop_decode_whole": {"median_ms": round(loop_ms, 2), "all_ms": [round(x, 2) for x in loop_all],
                          "msamples_per_s": round(msamples / (loop_ms / 1e3), 1),
                          "last_clip_split_ms": {"upload": loop_split[0], "walk": loop_split[1], "kernels": loop_split[2],
                                                 "download": loop_split[3], "total": loop_split[4], "batches": loop_split[5]}},
    "decode_batch": {"median_ms": round(batch_ms, 2), "all_ms": [round(x, 2) for x in batch_all],
                     "msamples_per_s": round(msamples / (batch_ms / 1e3), 1),
                     "split_ms": {"upload": batch_split[0], "walk": batch_split[1], "kernels": batch_split[2],
                                  "download": batch_split[3], "total": batch_split[4], "passes": batch_split[5]}},
    "speedup": round(loop_ms / batch_ms, 2),
}, indent=1))
dec.close()
