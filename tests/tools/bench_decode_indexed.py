"""Windows from block indexes, queued, against the synchronous window call with index hints: the two workloads of
tests/tools/bench_decode_windows.py in one process --
  clips : one 48 000-sample window of each of 125 ten-second stereo clips (BASELINE C4), seeded starts;
  long  : 64 one-second windows spread over ONE ten-minute mono file (about 7000 blocks);
each into one float32 device tensor, by
  sync    decode_windows_tensor(index=block_index_resident(...)): sla_hip_decode_windows_resident with seek hints;
  queued  decode_windows_indexed(indexes=index_resident(...)):    sla_hip_decode_windows_indexed.
For both, per repetition: (a) the host time spent inside the call, (b) the time until the caller's stream has finished
(the call, then torch.cuda.synchronize()).  2 warm-ups, median of 5, outputs compared equal bit for bit.
usage: python tests/tools/bench_decode_indexed.py [clips] [reps] [out.json] [long_seconds]"""
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
WARMUPS = 2
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
hints = dec.block_index_resident(srcs)
long_hints = dec.block_index_resident(long_srcs)
idx = dec.index_resident(srcs)
long_idx = dec.index_resident(long_srcs)
assert all(x.stop == 0 for x in idx + long_idx)
assert [x.to_bytes() for x in idx] == [sla_amd.Index.build(d.tobytes()).to_bytes() for d in datas]
result = {}


def sync_clips():
    t, samples, results = dec.decode_windows_tensor(srcs, starts, win, dtype=torch.float32, index=hints)
    result["t"], result["ok"] = t, (results == [0] * clips and samples == [win] * clips)


def queued_clips():
    result["t"], result["oc"] = dec.decode_windows_indexed(srcs, idx, starts, win, dtype=torch.float32)


def sync_long():
    t, samples, results = dec.decode_windows_tensor(long_srcs * long_windows, long_starts, win, dtype=torch.float32,
                                                    index=long_hints * long_windows)
    result["t"], result["ok"] = t, (results == [0] * long_windows and samples == [win] * long_windows)


def queued_long():
    result["t"], result["oc"] = dec.decode_windows_indexed(long_srcs * long_windows, long_idx * long_windows, long_starts, win,
                                                           dtype=torch.float32)


def timed(fn):
    """-> (median host ms inside the call, median ms until the stream has finished, all of both, the last output)"""
    for _ in range(WARMUPS):
        fn()
        torch.cuda.synchronize()
    host, done = [], []
    for _ in range(reps):
        result.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append((t1 - t0) * 1e3)
        done.append((t2 - t0) * 1e3)
        if "oc" in result:
            oc = result["oc"].cpu().numpy()
            result["ok"] = bool((oc[:, 0] == 0).all() and (oc[:, 1] == win).all())
        assert result["ok"]
    return {"host_ms_in_call": round(float(np.median(host)), 3), "ms_until_stream_done": round(float(np.median(done)), 3),
            "all_host_ms": [round(x, 3) for x in host], "all_done_ms": [round(x, 3) for x in done]}, result["t"]


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


sc, t_sc = timed(sync_clips)
qc, t_qc = timed(queued_clips)
exact_clips = same_bits(t_sc, t_qc) and all(bool(torch.equal(t_qc[i].cpu().view(torch.int32), torch.from_numpy(
    (pcms[i][:, starts[i]:starts[i] + win].astype(np.float32) * np.float32(2.0 ** -31)).view(np.int32)))) for i in range(0, clips, 16))
del t_sc, t_qc
result.clear()
sl, t_sl = timed(sync_long)
ql, t_ql = timed(queued_long)
exact_long = same_bits(t_sl, t_ql)
report = {
    "device": sla_amd.device_name(), "clips": clips, "samples_per_clip": n, "window_samples": win, "reps": reps, "warmups": WARMUPS,
    "ring_slots": sla_amd.DEC_QUEUE_SLOTS, "long_file": {"seconds": long_seconds, "stream_bytes": int(len(long_data)), "blocks": long_idx[0].num_blocks,
                                   "windows": long_windows},
    "clips_sync_decode_windows_tensor_with_hints": sc, "clips_queued_decode_windows_indexed": qc,
    "long_sync_decode_windows_tensor_with_hints": sl, "long_queued_decode_windows_indexed": ql,
    "exact_clips": exact_clips, "exact_long": exact_long,
}
print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
dec.close()
assert exact_clips and exact_long
