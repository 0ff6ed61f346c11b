"""What decoding through damage costs, in one process: Decoder.salvage_resident_tensor against Decoder.decode_resident_tensor
-- the yardstick -- on the long file of tests/tools/bench_decode_resident.py (48 kHz 16-bit stereo, order 16, MS,
4096-sample blocks, ten minutes) in device memory:
  clean    the undamaged stream through both calls (mode 1, nothing concealed; the outputs must be equal bit for bit)
  mode 1   a copy with one body byte flipped in a block in the middle: the chain is intact, that block is silence
  mode 2   a copy with the sync code of a block in the middle destroyed: the chain is broken, the salvage scan runs twice
Every figure: 2 warm-ups, then the median of 5 wall-clock times around the synchronous call, each step under a time limit of
its own.  The damaged outputs must equal the clean one with the damaged block's samples zeroed.
usage: python tests/tools/bench_salvage.py [out.json] [long_seconds]"""
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
import walkmodel as WM

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "salvage.json")
long_seconds = int(sys.argv[2]) if len(sys.argv) > 2 else 600
WARM, REPS, STEP_LIMIT = 2, 5, 300


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


def wall_ms(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), [round(x, 3) for x in t]


# ---- the stream and its two damaged copies
minute = S.synth_pcm(2, 60 * 48000, 16, 48000, seed=77)
long_pcm = np.ascontiguousarray(np.tile(minute, (1, (long_seconds + 59) // 60))[:, :long_seconds * 48000])
enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
enc.set_wave_format(2, 16, 48000)
enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
clean = step(lambda: enc.encode_whole(long_pcm), 600)
enc.close()
total = long_pcm.shape[1]
chain = WM.walk(clean, total, total, 4096)
assert chain.stop == 0 and chain.extent == total
off, blen, smp, n, _, _ = chain.rows[chain.num_blocks // 2]
flipped = bytearray(clean)
flipped[off + blen // 2] ^= 0x55
broken = bytearray(clean)
broken[off] = 0x00


def resident(data):
    host = np.zeros(len(data) + 33, np.uint8)
    host[1:1 + len(data)] = np.frombuffer(bytes(data), np.uint8)           # at an odd offset, as a slice of a corpus is
    return torch.from_numpy(host).cuda()[1:1 + len(data)]


dec = sla_amd.Decoder(2, 4096, 16, 1, 8)
keep = {}
RES = ("gathers", "walks", "kernels", "emit", "total", "passes")


def decode(src):
    t, lengths, results = dec.decode_resident_tensor([src], dtype=torch.float32)
    assert results == [0] and lengths == [total]
    keep["t"] = t[0]


def salvage(src):
    keep["t"], keep["report"], keep["ranges"] = dec.salvage_resident_tensor(src, dtype=torch.float32)


src = resident(clean)
routes = {}
ms, all_ms = step(lambda: wall_ms(lambda: decode(src)))
routes["decode_resident_clean"] = {"median_ms": round(ms, 2), "all_ms": all_ms, "split_ms": dict(zip(RES, dec.last_timing()))}
want = keep.pop("t")
ms, all_ms = step(lambda: wall_ms(lambda: salvage(src)))
routes["salvage_clean"] = {"median_ms": round(ms, 2), "all_ms": all_ms, "split_ms": dict(zip(RES, dec.last_timing())),
                           "report": keep["report"], "ranges": keep["ranges"]}
assert keep["report"]["result"] == 0 and keep["report"]["mode"] == 1 and keep["ranges"] == []
assert torch.equal(keep.pop("t").view(torch.int32), want.view(torch.int32))
want = want.clone()
want[:, smp:smp + n] = 0
for name, data, mode, reason in (("salvage_mode1_one_block_flipped", flipped, 1, "crc"), ("salvage_mode2_one_sync_destroyed", broken, 2, "gap")):
    del src
    src = resident(data)
    ms, all_ms = step(lambda: wall_ms(lambda: salvage(src)))
    routes[name] = {"median_ms": round(ms, 2), "all_ms": all_ms, "split_ms": dict(zip(RES, dec.last_timing())),
                    "last_walk": list(dec.last_walk()), "report": keep["report"], "ranges": keep["ranges"]}
    assert keep["report"]["result"] == 11 and keep["report"]["mode"] == mode and keep["ranges"] == [(smp, n, reason)], keep["report"]
    assert torch.equal(keep.pop("t").view(torch.int32), want.view(torch.int32)), name
dec.close()

base = routes["decode_resident_clean"]["median_ms"]
report = {"device": sla_amd.device_name(), "seconds": long_seconds, "stream_bytes": len(clean), "blocks": chain.num_blocks,
          "warmups": WARM, "reps": REPS, **routes,
          "over_decode_resident": {k: round(v["median_ms"] / base, 3) for k, v in routes.items() if k != "decode_resident_clean"},
          "all_results_equal": True}
print(json.dumps(report, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(report, fh, indent=1)
    fh.write("\n")
