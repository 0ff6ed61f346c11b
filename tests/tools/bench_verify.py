"""What option "verify" costs: the same encode call with verify 0 and 1, interleaved in one process
on two handles that differ in that option only, after a warm-up of both; medians, minima and the spread of every arm.

  C4  125 ten-second stereo clips (48 kHz 16-bit, MS, order 16, 4096-sample blocks)
        host    encode_batch of left-justified int32 planes in pageable host memory (worker lanes on, the default)
        tensor  encode_batch_tensor of one int16 [125][2][480000] device tensor (no upload: the device-side cost)
  C3  one full-length stereo file (3600 s, 48 kHz 24-bit, MS, order 32, 3 long-term taps, LMS 8; ten minutes of
      synthetic signal, repeated), EncodeWhole
        pinned    from page-locked planes into a page-locked buffer
        pageable  from pageable planes

The yardstick of the device side is the decoder's own kernel time for the same files in the same run
(Decoder.decode_batch / decode_whole, then last_timing()[2]): the pass launches those four kernels plus one streaming
compare, so tensor(on) - tensor(off) should be about that time plus the compare and one small table upload.

The library can be swapped with SLA_HIP_LIB (a build of the parent commit: `--off-only` then times the verify-off arm
alone, since that build has no such option), for the claim "option off costs nothing" in the same session.
usage: python tests/tools/bench_verify.py [--reps R] [--clips N] [--seconds S] [--off-only] [--skip-c3] [out.json]"""
import hashlib
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


reps, clips, seconds = arg("--reps", 7), arg("--clips", 125), arg("--seconds", 3600)
off_only, skip_c3 = "--off-only" in sys.argv, "--skip-c3" in sys.argv
flags_with_value = ("--reps", "--clips", "--seconds")
rest = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags_with_value]
out_path = rest[0] if rest else None
ARMS = (0,) if off_only else (0, 1)


def stats(t):
    t = sorted(t)
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3),
            "all_ms": [round(v, 3) for v in t]}


def ab(make, call, digest=lambda r: r):
    """call(enc) on a verify-off and a verify-on handle, alternating, after one warm-up of each (whose results, through
    `digest`, must agree between the arms)"""
    encs = {}
    for v in ARMS:
        encs[v] = make()
        if v:
            encs[v].set_option("verify", 1)
    out, times, ctr = {}, {v: [] for v in ARMS}, None
    for v in ARMS:
        out[v] = digest(call(encs[v]))
    for _ in range(reps):
        for v in ARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(encs[v])
            times[v].append((time.perf_counter() - t0) * 1e3)
    if 1 in ARMS:
        ctr = encs[1].last_verify()
        assert out[0] == out[1], "verify changed a byte or a result"
        assert ctr[1] == 0 and ctr[4] == 0 and ctr[0] > 0, ctr
    for e in encs.values():
        e.close()
    res = {"off": stats(times[0])}
    if 1 in ARMS:
        res["on"] = stats(times[1])
        res["on_minus_off_median_ms"] = round(res["on"]["median_ms"] - res["off"]["median_ms"], 3)
        res["compared_sample_channels"] = ctr[0]
        res["blocks"] = ctr[3]
    return res, out[0]


report = {"device": sla_amd.device_name(), "library": sla_amd.LIB_PATH, "reps": reps}

# ---- C4 ----------------------------------------------------------------------------------------------------------
n = 480000
base = [S.synth_pcm(2, n, 16, 48000, seed=100 + i) for i in range(8)]
planes = [base[i % 8] for i in range(clips)]
x = torch.empty((clips, 2, n), dtype=torch.int16, device="cuda")
for i in range(clips):
    x[i].copy_(torch.from_numpy((base[i % 8] >> 16).astype(np.int16)))
torch.cuda.synchronize()


def make_c4():
    enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
    enc.set_wave_format(2, 16, 48000)
    enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
    return enc


c4 = {"clips": clips, "samples_per_clip": n}
c4["host"], files = ab(make_c4, lambda enc: enc.encode_batch(planes))
c4["tensor"], files_t = ab(make_c4, lambda enc: enc.encode_batch_tensor(x))
assert files == files_t
dec = sla_amd.Decoder(2, 4096, 16, 1, 8)
datas = [np.frombuffer(d, np.uint8) for _, d in files]
outs = [np.empty((2, n), np.int32) for _ in range(clips)]
dec.decode_batch(datas, outs=outs)
kern = []
for _ in range(reps):
    dec.decode_batch(datas, outs=outs)
    kern.append(dec.last_timing()[2])
dec.close()
c4["decoder_kernels"] = stats(kern)
if 1 in ARMS:
    c4["tensor_on_minus_off_over_decoder_kernels"] = round(c4["tensor"]["on_minus_off_median_ms"] / c4["decoder_kernels"]["median_ms"], 3)
    c4["host_on_minus_off_over_tensor_on_minus_off"] = round(c4["host"]["on_minus_off_median_ms"] / max(c4["tensor"]["on_minus_off_median_ms"], 1e-9), 3)
report["C4"] = c4
del x, planes, outs

# ---- C3 ----------------------------------------------------------------------------------------------------------
if not skip_c3:
    N = seconds * 48000
    unit = S.synth_pcm(2, min(N, 600 * 48000), 24, 48000, seed=7)
    pcm = np.ascontiguousarray(np.tile(unit, (1, -(-N // unit.shape[1])))[:, :N])
    cap = 4 * 2 * N + 65536
    pinned_in = torch.from_numpy(pcm).pin_memory()
    pinned_out = torch.empty(cap, dtype=torch.uint8).pin_memory()
    page_out = np.zeros(cap, np.uint8)

    def make_c3():
        enc = sla_amd.Encoder(2, 4096, 32, 3, 8)
        enc.set_wave_format(2, 24, 48000)
        enc.set_encode_parameter(32, 3, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
        return enc

    c3 = {"seconds": seconds, "samples": N}
    pin_np, pout_np = pinned_in.numpy(), pinned_out.numpy()
    md5 = lambda view: (len(view), hashlib.md5(view).hexdigest())
    c3["pinned"], whole = ab(make_c3, lambda enc: enc.encode_whole(pin_np, out=pout_np), md5)
    c3["pageable"], whole_p = ab(make_c3, lambda enc: enc.encode_whole(pcm, out=page_out), md5)
    assert whole == whole_p
    c3["sla_bytes"] = whole[0]
    dec = sla_amd.Decoder(2, 4096, 32, 3, 8)
    data = page_out[:whole[0]]
    kern = []
    for k in range(3):
        dec.decode_whole(data, N)
        if k > 0:
            kern.append(dec.last_timing()[2])
    dec.close()
    c3["decoder_kernels"] = stats(kern)
    report["C3"] = c3

print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
