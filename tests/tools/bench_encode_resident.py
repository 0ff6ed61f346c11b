"""What it costs to leave the .sla streams on the device: 125 C4 clips (ten seconds of 48 kHz 16-bit
stereo, MS, order 16, 4096-sample blocks) in one int16 [125][2][480000] device tensor, one process, one encoder handle and
one decoder handle, the legs interleaved after a warm-up of each; medians, minima and the spread of every leg.

  tensor        Encoder.encode_batch_tensor: the files come home into host buffers
  resident      Encoder.encode_resident_tensor: the files stay in a device arena (k_enc_emit)
  trip_host     encode_batch_tensor -> Decoder.decode_batch_tensor (bytes down, bytes up again)
  trip_resident encode_resident_tensor -> Decoder.decode_resident_tensor (no .sla byte in host memory)
  emit_kernel   sla_hip_launch_enc_emit_batch alone, between two stream events: the 125 files of the run, copied out of
                an image that holds them back to back (as the pack image does) with their headers from the table.  This is
                a reconstruction of the driver's launch -- the run's arena copied into a fresh image, header bytes zeroed,
                the table made here -- not the launch inside sla_hip_encode_batch_resident: same kernel, files and sizes

The resident route must give the host route's bytes, and both round trips the input: checked before anything is timed.
usage: python tests/tools/bench_encode_resident.py [--steps K] [--warmup W] [--clips N] [out.json]"""
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


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


steps, warmup, clips = max(arg("--steps", 10), 10), max(arg("--warmup", 3), 3), arg("--clips", 125)
flags_with_value = ("--steps", "--warmup", "--clips")
rest = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags_with_value]
out_path = rest[0] if rest else None


def stats(t):
    t = sorted(t)
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3),
            "all_ms": [round(v, 3) for v in t]}


n = 480000
base = [S.synth_pcm(2, n, 16, 48000, seed=100 + i) for i in range(8)]
x = torch.empty((clips, 2, n), dtype=torch.int16, device="cuda")
for i in range(clips):
    x[i].copy_(torch.from_numpy((base[i % 8] >> 16).astype(np.int16)))
torch.cuda.synchronize()

enc = sla_amd.Encoder(2, 4096, 16, 1, 8)
enc.set_wave_format(2, 16, 48000)
enc.set_encode_parameter(16, 1, 8, sla_amd.CH_STEREO_MS, sla_amd.WINDOW_SIN, 4096)
dec = sla_amd.Decoder(2, 4096, 16, 1, 8)


def leg_tensor():
    return enc.encode_batch_tensor(x)


def leg_resident():
    return enc.encode_resident_tensor(x)


def leg_trip_host():
    files = enc.encode_batch_tensor(x)
    return dec.decode_batch_tensor([np.frombuffer(d, np.uint8) for _, d in files], dtype=torch.int16)


def leg_trip_resident():
    a, offsets, sizes, _ = enc.encode_resident_tensor(x)
    return dec.decode_resident_tensor([a[o:o + s] for o, s in zip(offsets, sizes)], dtype=torch.int16)


# ---- the routes agree, the loops close ----------------------------------------------------------------------------
files = leg_tensor()
arena, offsets, sizes, results = leg_resident()
assert results == [rc for rc, _ in files] == [0] * clips
host_arena = arena.cpu().numpy()
assert all(host_arena[o:o + s].tobytes() == d for (o, s), (_, d) in zip(zip(offsets, sizes), files)), "resident bytes differ"
for leg in (leg_trip_host, leg_trip_resident):
    back, lens, res = leg()
    assert res == [0] * clips and lens == [n] * clips and torch.equal(back, x), leg.__name__
    del back

# ---- the emit kernel alone ----------------------------------------------------------------------------------------
table = (sla_amd.EncEmit * clips)()
image = torch.zeros(arena.numel() + 16, dtype=torch.uint8, device="cuda")      # (room for the last aligned 16-byte load)
image[:arena.numel()] = arena
dest = torch.zeros_like(arena)
for k, (o, s) in enumerate(zip(offsets, sizes)):
    table[k].img_off, table[k].dst, table[k].bytes, table[k].header_bytes = o, dest.data_ptr() + o, s, 43
    C.memmove(table[k].header, host_arena[o:o + 43].ctypes.data, 43)
    image[o:o + 43] = 0                                   # as the packer leaves the header bytes
d_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()


def leg_emit():
    st = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(st)
    rc = sla_amd.lib().sla_hip_launch_enc_emit_batch(d_table.data_ptr(), clips, max(sizes), image.data_ptr(), arena.numel(),
                                                     C.c_void_p(st.cuda_stream))
    t1.record(st)
    t1.synchronize()
    assert rc == 0
    return t0.elapsed_time(t1)


leg_emit()
assert torch.equal(dest, arena), "the emit kernel alone differs"

# ---- timing -------------------------------------------------------------------------------------------------------
legs = {"tensor": leg_tensor, "resident": leg_resident, "trip_host": leg_trip_host, "trip_resident": leg_trip_resident}
times = {name: [] for name in legs}
emit_ms = []
for step in range(warmup + steps):
    for name, leg in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leg()
        torch.cuda.synchronize()
        if step >= warmup:
            times[name].append((time.perf_counter() - t0) * 1e3)
    ms = leg_emit()
    if step >= warmup:
        emit_ms.append(ms)
enc.close(); dec.close()

report = {"device": sla_amd.device_name(), "clips": clips, "samples_per_clip": n, "steps": steps, "warmup": warmup,
          "sla_bytes": int(sum(sizes))}
for name in legs:
    report[name] = stats(times[name])
report["emit_kernel"] = stats(emit_ms)
report["emit_kernel"]["gb_per_s_read_plus_written"] = round(2 * sum(sizes) / (report["emit_kernel"]["median_ms"] * 1e-3) / 1e9, 1)
report["resident_over_tensor"] = round(report["resident"]["median_ms"] / report["tensor"]["median_ms"], 3)
report["trip_resident_over_trip_host"] = round(report["trip_resident"]["median_ms"] / report["trip_host"]["median_ms"], 3)
print(json.dumps(report, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
