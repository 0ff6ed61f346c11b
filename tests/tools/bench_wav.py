"""What the WAV calls cost against today's public route on the same bytes (DESIGN sections 4a, 4b).  One process, one encoder
and one decoder handle per workload, the legs interleaved after a warm-up of each; medians, minima and the spread.

Workloads: c4 = 125 ten-second 48 kHz 16-bit stereo clips (C4's parameters); c3 = one 240 s 48 kHz 24-bit stereo file
(C3's parameters); mono8 = one 60 s 48 kHz 8-bit mono file (C4's parameters, no mid/side).

  enc_wav        Encoder.encode_wav_batch: WAV bytes in host memory -> .sla bytes in host memory
  enc_numpy      today's route: the RIFF chunks parsed and the samples de-interleaved and widened with numpy as
                 tests/slalibs.py::read_wav does it, then Encoder.encode_batch of the planes
  enc_resident   Encoder.encode_wav_resident: WAV bytes in device memory -> .sla bytes in a device arena
  dec_wav        Decoder.decode_wav_batch: .sla bytes in host memory -> WAV bytes in host memory
  dec_numpy      today's route: Decoder.decode_batch, then shift, interleave and pack behind a 44-byte header with numpy
  dec_resident   Decoder.decode_wav_resident of the arena's streams -> WAV bytes in device memory

Every route must give the same bytes: checked before anything is timed.
usage: python tests/tools/bench_wav.py [--steps K] [--warmup W] [--clips N] [--only c4|c3|mono8] [out.json]"""
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
import wavmodel as W


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


steps, warmup, clips = max(arg("--steps", 5), 5), max(arg("--warmup", 2), 1), arg("--clips", 125)
only = arg("--only", None, str)
flags_with_value = ("--steps", "--warmup", "--clips", "--only")
rest = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags_with_value]
out_path = rest[0] if rest else None


def stats(t):
    t = sorted(t)
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3),
            "all_ms": [round(v, 3) for v in t]}


def numpy_read(wav):
    """the host work of today's route: chunk walk, de-interleave, widen (tests/slalibs.py::read_wav on bytes)"""
    rc, info = W.parse(wav)
    raw = np.frombuffer(wav, np.uint8, info.data_bytes, info.data_off)
    return W.planes_from_frames(raw, info.num_channels, info.bits_per_sample)


def numpy_write(planes, bits, rate):
    return W.canonical(planes, bits, rate)


def workload(name):
    if name == "c4":
        base = [S.synth_pcm(2, 480000, 16, 48000, seed=100 + i) for i in range(8)]
        return [base[i % 8] for i in range(clips)], 16, 48000, (2, 4096, 16, 1, 8), (16, 1, 8, 1, 1, 4096)
    if name == "c3":
        return [S.synth_pcm(2, 240 * 48000, 24, 48000, seed=300)], 24, 48000, (2, 4096, 32, 3, 8), (32, 3, 8, 1, 1, 4096)
    return [S.synth_pcm(1, 60 * 48000, 8, 48000, seed=800)], 8, 48000, (1, 4096, 16, 1, 8), (16, 1, 8, 0, 1, 4096)


report = {"device": sla_amd.device_name(), "steps": steps, "warmup": warmup, "workloads": {}}
for name in ("c4", "c3", "mono8"):
    if only is not None and only != name:
        continue
    pcms, bits, rate, cap, param = workload(name)
    nch = pcms[0].shape[0]
    wavs = [W.build_wav(p, bits, rate) for p in pcms]
    enc = sla_amd.Encoder(*cap)
    enc.set_wave_format(nch, bits, rate)
    enc.set_encode_parameter(*param)
    dec = sla_amd.Decoder(*cap)
    d_wavs = [torch.from_numpy(np.frombuffer(w, np.uint8).copy()).cuda() for w in wavs]
    arena = torch.empty(2 * sum(len(w) for w in wavs) + 65536 * len(wavs), dtype=torch.uint8, device="cuda")

    def enc_wav():
        return [d for _, d in enc.encode_wav_batch(wavs)]

    def enc_numpy():
        enc.set_wave_format(nch, bits, rate)
        return [d for _, d in enc.encode_batch([numpy_read(w) for w in wavs])]

    def enc_resident():
        return [v for _, v in enc.encode_wav_resident(d_wavs, arena=arena)]

    # ---- the routes agree ----
    slas = enc_wav()
    assert slas == enc_numpy(), "encode_wav_batch and numpy + encode_batch differ"
    views = enc_resident()
    assert [v.cpu().numpy().tobytes() for v in views] == slas, "encode_wav_resident differs"
    d_outs = [torch.empty(len(w), dtype=torch.uint8, device="cuda") for w in wavs]

    def dec_wav():
        return [d for _, d in dec.decode_wav_batch(slas)]

    def dec_numpy():
        return [numpy_write(p, bits, rate) for _, p in dec.decode_batch(slas)]

    def dec_resident():
        return [v for _, v in dec.decode_wav_resident(views, outs=d_outs)]

    assert dec_wav() == wavs and dec_numpy() == wavs, "the decode routes do not give the files back"
    assert [v.cpu().numpy().tobytes() for v in dec_resident()] == wavs, "decode_wav_resident differs"

    legs = {"enc_wav": enc_wav, "enc_numpy": enc_numpy, "enc_resident": enc_resident, "dec_wav": dec_wav,
            "dec_numpy": dec_numpy, "dec_resident": dec_resident}
    times = {k: [] for k in legs}
    for it in range(warmup + steps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    samples = sum(p.shape[0] * p.shape[1] for p in pcms)
    res = {"files": len(wavs), "channels": nch, "bits": bits, "samples": samples, "wav_bytes": sum(len(w) for w in wavs),
           "sla_bytes": sum(len(s) for s in slas)}
    for k in legs:
        res[k] = stats(times[k])
        res[k]["gsamples_per_s"] = round(samples / res[k]["median_ms"] / 1e6, 3)
    report["workloads"][name] = res
    print(name, {k: res[k]["median_ms"] for k in legs}, flush=True)
    enc.close(); dec.close()
    del d_wavs, arena, views, d_outs

print(json.dumps(report))
if out_path:
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
