"""Random crops of streams that are in device memory: the 125 ten-second stereo clips of
tests/tools/bench_decode_resident.py (BASELINE C4: 48 kHz 16-bit, order 16, MS, 4096-sample blocks), one 48 000-sample
window of each with seeded starts, turned into one float32 [125][2][48000] device tensor two ways, in one process on one
handle:
  (a) decode_resident_tensor(float32) of the whole clips, then a slice per clip: the only way before;
  (b) decode_windows_tensor(float32) of the same windows: sla_hip_decode_windows_resident, only the blocks each window
      overlaps are gathered and decoded; (b) must equal (a) bit for bit;
and (c) ONE long mono file (BASELINE C2 shape, default 600 s, about 7000 blocks) with 64 one-second windows spread over
it, without and with index= (block_index_resident): the price of walking the chain from the header.
Each is repeated; the median is reported with the handle's last_timing split and last_window_stats.
usage: python tests/tools/bench_decode_windows.py [clips] [reps] [out.json] [long_seconds]"""
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
n, win = 480000, 48000
base = [S.synth_pcm(2, n, 16, 48000, seed=100 + i) for i in range(8)]
pcms = [base[i % 8] for i in range(clips)]
minute = S.synth_pcm(1, 60 * 48000, 16, 48000, seed=77)
long_pcm = np.ascontiguousarray(np.tile(minute, (1, (long_seconds + 59) // 60))[:, :long_seconds * 48000])
rng = np.random.default_rng(2024)
starts = [int(s) for s in rng.integers(0, n - win + 1, clips)]
long_windows = 64
long_starts = [int((k + 0.5) * (long_pcm.shape[1] - win) / long_windows) for k in range(long_windows)]

enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
enc.set_wave_format(2, 16, 48000)
enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
res = enc.encode_batch(pcms)
assert all(rc == 0 for rc, _ in res)
datas = [np.frombuffer(d, np.uint8) for _, d in res]
enc.set_wave_format(1, 16, 48000)
enc.set_encode_parameter(16, 1, 8, sla_amd.CH_NONE, sla_amd.WINDOW_SIN, 4096)
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


def whole_then_slice():
    t, lengths, results = dec.decode_resident_tensor(srcs, dtype=torch.float32)
    assert results == [0] * clips and lengths == [n] * clips
    result["t"] = torch.stack([t[b, :, s:s + win] for b, s in enumerate(starts)])


def windows():
    t, samples, results = dec.decode_windows_tensor(srcs, starts, win, dtype=torch.float32)
    assert results == [0] * clips and samples == [win] * clips
    result["t"] = t


long_index = dec.block_index_resident(long_srcs)
assert long_index[0][2] == 0


def long_plain():
    t, samples, results = dec.decode_windows_tensor(long_srcs * long_windows, long_starts, win, dtype=torch.float32)
    assert results == [0] * long_windows and samples == [win] * long_windows
    result["t"] = t


def long_indexed():
    t, samples, results = dec.decode_windows_tensor(long_srcs * long_windows, long_starts, win, dtype=torch.float32,
                                                    index=long_index * long_windows)
    assert results == [0] * long_windows and samples == [win] * long_windows
    result["t"] = t


def timed(fn):
    fn()                                                             # warm-up: device buffers, code objects
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


RES = ("gathers", "walks", "kernels", "emit", "total", "passes")
STATS = ("blocks_passed_over", "blocks_decoded", "bytes_gathered", "plane_samples_per_channel")


def entry(ms, all_ms, split, stats=None):
    e = {"median_ms": round(ms, 2), "all_ms": [round(x, 2) for x in all_ms], "split_ms": dict(zip(RES, split))}
    if stats is not None:
        e["window_stats"] = dict(zip(STATS, stats))
    return e


a_ms, a_all, a_split = timed(whole_then_slice)
a = result["t"]
b_ms, b_all, b_split = timed(windows)
b, b_stats = result["t"], dec.last_window_stats()
exact = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
exact_pcm = all(bool(torch.equal(b[i].cpu().view(torch.int32), torch.from_numpy(
    (pcms[i][:, starts[i]:starts[i] + win].astype(np.float32) * np.float32(2.0 ** -31)).view(np.int32)))) for i in range(0, clips, 16))
del a, b
result.clear()
c_ms, c_all, c_split = timed(long_plain)
c, c_stats = result["t"], dec.last_window_stats()
d_ms, d_all, d_split = timed(long_indexed)
d, d_stats = result["t"], dec.last_window_stats()
exact_long = bool(torch.equal(c.view(torch.int32), d.view(torch.int32))) and all(bool(torch.equal(
    d[k].cpu().view(torch.int32), torch.from_numpy((long_pcm[:, s:s + win].astype(np.float32) * np.float32(2.0 ** -31)).view(np.int32))))
    for k, s in enumerate(long_starts))
report = {
    "device": sla_amd.device_name(), "clips": clips, "samples_per_clip": n, "window_samples": win, "channels": 2, "reps": reps,
    "stream_bytes": int(sum(len(d_) for d_ in datas)), "tensor_bytes": clips * 2 * win * 4,
    "exact_b_equals_a": exact, "exact_b_equals_pcm": exact_pcm,
    "a_decode_resident_tensor_then_slice": entry(a_ms, a_all, a_split),
    "b_decode_windows_tensor": entry(b_ms, b_all, b_split, b_stats),
    "speedup_b_over_a": round(a_ms / b_ms, 2),
    "c_long_file_64_windows_from_the_header": dict(entry(c_ms, c_all, c_split, c_stats), seconds=long_seconds,
                                                   stream_bytes=int(len(long_data)), blocks=int(len(long_index[0][0]))),
    "d_long_file_64_windows_with_index": entry(d_ms, d_all, d_split, d_stats),
    "exact_long": exact_long,
}
print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
dec.close()
assert exact and exact_pcm and exact_long
