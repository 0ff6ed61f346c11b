"""Cutting one resident ten-minute file into 60 ten-second clips in one call, two routes in one process:
  splice    Decoder.splice_resident: whole blocks copied, the two blocks each cut passes through decoded and stored RAW;
  baseline  today's route: decode_windows_indexed into an int16 tensor, then Encoder.encode_resident_tensor.
The file is the ten-minute 16-bit stereo file of tests/tools/bench_walk_wide.py (profiles/walk_wide.json).  2 warm-ups,
median of 5 with the spread; the clips of both routes are decoded and compared for equality; recorded besides: the bytes of
both routes' outputs and the execution spans of k_splice_edges and k_splice_copy (sla_hip_decoder_last_timing).
usage: python tests/tools/bench_splice.py [reps] [out.json] [seconds]"""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None
seconds = int(sys.argv[3]) if len(sys.argv) > 3 else 600
WARMUPS = 2
clip = 10 * 48000
minute = S.synth_pcm(2, 60 * 48000, 16, 48000, seed=77)
pcm = np.ascontiguousarray(np.tile(minute, (1, (seconds + 59) // 60))[:, :seconds * 48000])
clips = pcm.shape[1] // clip
starts = [k * clip for k in range(clips)]

enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
enc.set_wave_format(2, 16, 48000)
enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
data = np.frombuffer(enc.encode_whole(pcm), np.uint8)
host = np.zeros(len(data) + 1, np.uint8)
host[1:] = data
corpus = torch.from_numpy(host).cuda()
src = corpus[1:]                                           # an odd address
dec = sla_amd.Decoder(2, 4096, 16, 1, 8)
index = dec.index_resident([src])[0]
assert index.stop == 0 and index.extent == pcm.shape[1]
plans = [sla_amd.splice_plan([(None, index, s, clip)])[1] for s in starts]
arena = torch.empty(sum(p.bytes for p in plans), dtype=torch.uint8, device="cuda")
result = {}


def splice():
    got = dec.splice_resident([[(src, index, s, clip)] for s in starts], arena=arena)
    assert all(rc == 0 for rc, _ in got)
    result["clips"] = [o for _, o in got]
    result["timing"] = dec.last_timing()


def baseline():
    x, oc = dec.decode_windows_indexed([src] * clips, [index] * clips, starts, clip, dtype=torch.int16)
    a, offs, sizes, rcs = enc.encode_resident_tensor(x)
    assert rcs == [0] * clips and bool((oc[:, 0] == 0).all())
    result["clips"] = [a[o:o + n] for o, n in zip(offs, sizes)]


def timed(fn):
    for _ in range(WARMUPS):
        fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_per_call": round(float(np.median(ms)), 3), "spread_ms": round(max(ms) - min(ms), 3), "all_ms": [round(v, 3) for v in ms]}


sp = timed(splice)
sp_clips, timing = result["clips"], result["timing"]
sp["output_bytes"] = int(sum(c.numel() for c in sp_clips))
sp["edge_blocks"] = int(sum(p.edge_blocks for p in plans))
sp["verbatim_bytes"] = int(sum(p.verbatim_bytes for p in plans))
sp["k_splice_edges_ms"], sp["k_splice_copy_ms"] = round(timing[2], 4), round(timing[3], 4)
a, na, ra = dec.decode_resident_tensor(sp_clips, dtype=torch.int16)
bl = timed(baseline)
bl_clips = result["clips"]
bl["output_bytes"] = int(sum(c.numel() for c in bl_clips))
b, nb, rb = dec.decode_resident_tensor(bl_clips, dtype=torch.int16)
equal = bool(torch.equal(a, b)) and na == nb == [clip] * clips and ra == rb == [0] * clips
equal = equal and bool(np.array_equal(a[0].cpu().numpy().astype(np.int32) << 16, pcm[:, :clip]))
gap, spread = bl["ms_per_call"] - sp["ms_per_call"], max(sp["spread_ms"], bl["spread_ms"])
report = {"device": sla_amd.device_name(), "file": {"seconds": seconds, "stream_bytes": int(len(data)), "blocks": index.num_blocks},
          "clips": clips, "samples_per_clip": clip, "reps": reps, "warmups": WARMUPS, "splice_resident": sp,
          "baseline_decode_windows_indexed_then_encode_resident_tensor": bl, "outputs_decode_equal": equal,
          "faster_by_more_than_three_spreads": bool(gap > 3 * spread)}
print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
dec.close()
enc.close()
assert equal
