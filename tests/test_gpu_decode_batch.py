"""GPU tests of sla_hip_decode_batch (many .sla files in one call; run with -m gpu on an MI355X).

Every item of a batch must carry exactly what SLADecoder_DecodeWhole of that file alone returns -- result code,
sample count, samples (those before a failing block included) -- checked against the CPU oracle's decoder
(oracle/sla_oracle.c: slao_decode_whole) and against Decoder.decode_whole on the same handle: clean clips of the
C4 shape, mixed formats that take several passes, damaged files between good ones with the CRC check on and off,
the bounded bit reader on its own, handle reuse, and a round trip that crosses the pass cap.
Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

import slalibs as S
import waveforms as W

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CAPACITY, BUF, DATA, HDRFMT, CORRUPT, SYNC = 0, 2, 3, 4, 9, 10, 11, 12
HANDLE_CAP = (8, 8192, 32, 3, 32)          # channels, block samples, PARCOR order, long-term order, LMS order


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def make_decoder(hip, crc=1, cap=HANDLE_CAP):
    return hip.Decoder(*cap, enable_crc_check=crc)


def dec_params(cap=HANDLE_CAP):
    """oracle parameters of a decode on a handle of capacity `cap` (the format comes from each file's header)"""
    return S.make_params(cap=cap)


def check_batch(oracle, dec, datas, caps, crc=1, clean=None):
    """decode_batch of `datas` == decode_whole of each file on the same handle, and == the oracle's decode where the
    oracle applies (it always checks CRCs: with crc=0 only the files marked clean are compared with it)"""
    got = dec.decode_batch(datas, capacities=caps)
    dec.batch_timing = dec.last_timing()          # decode_whole below replaces the handle's timing
    assert len(got) == len(datas)
    p = dec_params()
    for i, (data, cap, (rc, out)) in enumerate(zip(datas, caps, got)):
        rw, want_w = dec.decode_whole(data, cap)
        assert rc == rw, ("item", i, rc, rw)
        assert out.shape[1] == want_w.shape[1], ("item", i, out.shape, want_w.shape)
        n = min(out.shape[0], want_w.shape[0])
        assert np.array_equal(out[:n], want_w[:n]), ("item", i)
        if crc == 1 or (clean is not None and clean[i]):
            ro, want_o, _ = oracle.decode_whole(p, data, cap)
            assert rc == ro, ("item", i, rc, ro)
            assert out.shape[1] == want_o.shape[1], ("item", i)
            n = min(out.shape[0], want_o.shape[0])
            assert np.array_equal(out[:n], want_o[:n]), ("item", i)
    return got


def encode_clips(hip, p, pcms):
    enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    try:
        enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
        enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method, p.window_type,
                                 p.max_block_samples)
        res = enc.encode_batch(pcms)
    finally:
        enc.close()
    assert all(rc == 0 for rc, _ in res)
    return [d for _, d in res]


C4 = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096, cap=(2, 4096, 16, 1, 8))


# ------------------------------------------------------------------ clean batches

def test_c4_shaped_batch_with_ragged_lengths(oracle, hip):
    """16 ten-second stereo 16-bit MS clips (order 16, 4096-sample blocks), lengths ragged around 480 000"""
    lens = [480000 - 3001 * i - (i % 3) * 517 for i in range(16)]
    pcms = [S.synth_pcm(2, n, 16, 48000, seed=100 + i) for i, n in enumerate(lens)]
    datas = encode_clips(hip, C4, pcms)
    dec = make_decoder(hip)
    try:
        got = check_batch(oracle, dec, datas, lens)
        for pcm, (rc, out) in zip(pcms, got):
            assert rc == OK and np.array_equal(out, pcm)
        assert dec.batch_timing[5] == 1
    finally:
        dec.close()


def _mixed_files(oracle):
    """(data, pcm) of five formats, item order interleaved so that files of one pass are not neighbours"""
    specs = [
        (S.make_params(1, 16, 48000, 16, 1, 8, 0, 1, 4096), W.music_like(1, 30011, 16, seed=1)),
        (S.make_params(2, 24, 48000, 32, 3, 8, 1, 1, 4096), W.gen("sine", 2, 25000, 24, seed=2)),
        (S.make_params(8, 16, 48000, 8, 1, 4, 0, 1, 2048), W.gen("white", 8, 9000, 16, seed=3)),
        (S.make_params(1, 16, 48000, 16, 1, 8, 0, 1, 4096), W.gen("sine", 1, 20000, 16, lshift=0, seed=4)),
        (S.make_params(1, 16, 48000, 16, 1, 8, 0, 1, 4096), W.gen("sine", 1, 20000, 16, lshift=3, seed=5)),
        (S.make_params(2, 24, 48000, 32, 3, 8, 1, 1, 4096), W.gen("white", 2, 13003, 24, seed=6)),
        (S.make_params(1, 16, 48000, 16, 1, 8, 0, 1, 4096), W.gen("sine", 1, 17001, 16, lshift=3, seed=7)),
    ]
    out = []
    for p, pcm in specs:
        ret, data = oracle.encode_whole(p, pcm)
        assert ret == 0
        out.append((data, pcm))
    return out


def test_mixed_formats_take_several_passes(oracle, hip):
    files = _mixed_files(oracle)
    lshifts = {int(np.frombuffer(d, np.uint8)[24]) for d, _ in files}
    assert len(lshifts) >= 2                           # two offset_lshift values among the mono files
    dec = make_decoder(hip)
    try:
        got = check_batch(oracle, dec, [d for d, _ in files], [pcm.shape[1] for _, pcm in files])
        for (_, pcm), (rc, out) in zip(files, got):
            assert rc == OK and np.array_equal(out, pcm)
        assert dec.batch_timing[5] >= 4                # mono/lshift 0, mono/lshift 3, stereo 24 MS, 8 channels
    finally:
        dec.close()


# ------------------------------------------------------------------ damaged files between good ones

def _stream(oracle, nch=2, n=30000, ms=1, seed=9):
    pcm = W.music_like(nch, n, 16, seed=seed)
    p = S.make_params(nch, 16, 48000, 16, 1, 8, ms if nch == 2 else 0, 1, 4096)
    ret, data, tr = oracle.encode_trace(p, pcm)
    assert ret == 0
    offs = np.concatenate(([43], 43 + np.cumsum(tr.blk_bytes[:tr.num_blocks]))).astype(int)
    return p, pcm, bytearray(data), offs, tr


def _damaged_set(oracle, hip):
    """list of (name, data, capacity, clean)"""
    entries = []
    good = [_stream(oracle, seed=20 + i) for i in range(3)]
    for i, (p, pcm, data, offs, tr) in enumerate(good):
        entries.append(("good%d" % i, bytes(data), pcm.shape[1], True))

    p, pcm, data, offs, tr = _stream(oracle, seed=31)
    data[offs[3] + 40] ^= 0x10
    entries.append(("corrupt block", bytes(data), pcm.shape[1], False))

    p, pcm, data, offs, tr = _stream(oracle, seed=32)
    entries.append(("truncated in a block", bytes(data[:offs[2] + 100]), pcm.shape[1], False))
    entries.append(("truncated at a block", bytes(data[:offs[4]]), pcm.shape[1], False))
    entries.append(("truncated in a block header", bytes(data[:offs[4] + 5]), pcm.shape[1], False))

    p, pcm, data, offs, tr = _stream(oracle, seed=33)
    data[offs[2]] = 0x7F
    entries.append(("lost sync", bytes(data), pcm.shape[1], False))

    # a size field one byte too large, CRC re-made: the reference resyncs where its reader stopped
    p, pcm, data, offs, tr = _stream(oracle, nch=1, ms=0, seed=34)
    k = 2
    size = int.from_bytes(data[offs[k] + 2:offs[k] + 6], "big") + 1
    data[offs[k] + 2:offs[k] + 6] = size.to_bytes(4, "big")
    crc = oracle.crc16(np.frombuffer(bytes(data[offs[k] + 8:offs[k] + 6 + size]), np.uint8))
    data[offs[k] + 6:offs[k] + 8] = int(crc).to_bytes(2, "big")
    entries.append(("size field disagrees", bytes(data), pcm.shape[1], False))

    p, pcm, data, offs, tr = _stream(oracle, seed=35)
    hdr = bytearray(data); hdr[20] ^= 1
    entries.append(("header CRC", bytes(hdr), pcm.shape[1], False))
    bad = bytearray(data); bad[0] = ord("X")
    entries.append(("header format", bytes(bad), pcm.shape[1], False))

    p, pcm, data, offs, tr = _stream(oracle, seed=36)
    entries.append(("buffer too small", bytes(data), int(tr.blk_start[3]) + 10, True))
    small = bytearray(data); small[offs[3] + 30] ^= 0x01
    entries.append(("buffer too small, damaged", bytes(small), int(tr.blk_start[3]) + 10, False))

    big = S.make_params(2, 16, 48000, 48, 1, 8, 1, 1, 4096)                   # PARCOR order 48 > the handle's 32
    ret, data = oracle.encode_whole(big, W.music_like(2, 9000, 16, seed=37))
    assert ret == 0
    entries.append(("capacity exceeded", data, 9000, True))

    entries.append(("empty stream", b"", 100, True))
    entries.append(("no samples", hip.encode_header(2, 16, 48000, 0, 16, 1, 8, 1, 1, 4096, 0, 0, 0, 0), 100, True))
    return entries


@pytest.mark.parametrize("crc", [1, 0])
def test_damaged_files_between_good_ones(oracle, hip, crc):
    entries = _damaged_set(oracle, hip)
    # good files around every damaged one, and a truncated file in the MIDDLE of its pass (its reader would otherwise
    # run into the next file's bytes)
    good = [e for e in entries if e[0].startswith("good")]
    order = []
    for j, e in enumerate(e for e in entries if not e[0].startswith("good")):
        order += [good[j % len(good)], e]
    order.append(good[0])
    dec = make_decoder(hip, crc)
    try:
        got = check_batch(oracle, dec, [e[1] for e in order], [e[2] for e in order], crc=crc, clean=[e[3] for e in order])
    finally:
        dec.close()
    codes = {e[0]: rc for e, (rc, _) in zip(order, got)}
    if crc == 1:
        assert codes["corrupt block"] == CORRUPT
        assert codes["header CRC"] == CORRUPT
        assert codes["buffer too small, damaged"] == CORRUPT
    assert codes["truncated in a block"] == DATA
    assert codes["lost sync"] == SYNC
    assert codes["header format"] == HDRFMT
    assert codes["buffer too small"] == BUF
    assert codes["capacity exceeded"] == CAPACITY
    assert codes["empty stream"] == DATA
    assert codes["no samples"] == OK
    assert all(rc == OK for (name, _, _, _), (rc, _) in zip(order, got) if name.startswith("good"))


# ------------------------------------------------------------------ the bounded reader on its own

BLOCK_DT = np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"), ("num_samples", "<u4"), ("flags", "<u4")])


def _blocks(offs, tr, byte_base, smp_base, data_len):
    nb = int(tr.num_blocks)
    t = np.zeros(nb, BLOCK_DT)
    for b in range(nb):
        if offs[b] + 11 > data_len:
            return t[:b]
        t[b] = (byte_base + offs[b], min(int(offs[b + 1]), data_len) - offs[b], smp_base + int(tr.blk_start[b]),
                int(tr.blk_nsmpl[b]), 0)
    return t


def _run_dec_bits(hip, torch, image, image_bytes, blocks, ends, nch, span):
    L = hip.lib()
    nb = len(blocks)
    d_img = torch.from_numpy(image.view(np.int32).copy()).cuda()
    d_blk = torch.from_numpy(blocks.view(np.uint8).copy()).cuda()
    d_end = torch.from_numpy(np.asarray(ends, np.int64)).cuda() if ends is not None else None
    d_info = torch.zeros(nb * 4, dtype=torch.int32, device="cuda")
    d_chan = torch.zeros(nb * nch * 8, dtype=torch.int32, device="cuda")
    d_kint = torch.zeros(nb * nch * 17, dtype=torch.int32, device="cuda")
    d_planes = torch.zeros(nch * span, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_dec_bits_x(C.c_void_p(d_img.data_ptr()), C.c_uint64(image_bytes), C.c_void_p(d_blk.data_ptr()), nb,
                                     nch, 16, 0, 1, 16, 1, 1, C.c_void_p(d_planes.data_ptr()), C.c_uint64(span),
                                     C.c_void_p(d_info.data_ptr()), C.c_void_p(d_chan.data_ptr()), C.c_void_p(d_kint.data_ptr()),
                                     None, C.c_void_p(d_end.data_ptr()) if d_end is not None else None)
    assert rc == 0
    torch.cuda.synchronize()
    return d_planes.cpu().numpy().reshape(nch, span), d_info.cpu().numpy().reshape(nb, 4)


def test_dec_bits_x_bounds_each_block_by_its_own_file(oracle, hip):
    """two images back to back, the first cut inside its block 3: with per-block ends every block decodes as in its own
    image (zeros past the cut), without them block 3 reads the second image's bytes"""
    import torch
    Cn = 2
    pa, pcma, da, offsa, tra = _stream(oracle, seed=41)
    pb, pcmb, db, offsb, trb = _stream(oracle, seed=42)
    cut = int(offsa[3]) + 200
    a = np.frombuffer(bytes(da[:cut]), np.uint8)
    b = np.frombuffer(bytes(db), np.uint8)
    pad4 = lambda x: np.concatenate([x, np.zeros((-len(x)) % 4 + 4, np.uint8)])
    ia, ib = pad4(a), pad4(b)
    span_a, span_b = pcma.shape[1] + 4096, pcmb.shape[1] + 4096
    ba = _blocks(offsa, tra, 0, 0, len(a))
    bb = _blocks(offsb, trb, 0, 0, len(b))
    assert len(ba) == 4                                 # blocks 0..2 whole, block 3 clipped at the cut
    alone_a = _run_dec_bits(hip, torch, ia, len(a), ba, None, Cn, span_a)
    alone_b = _run_dec_bits(hip, torch, ib, len(b), bb, None, Cn, span_b)

    base_b = len(a) + (-len(a)) % 4                    # 4-byte aligned, the gap zero
    img = np.zeros(base_b + len(ib), np.uint8)
    img[:len(a)] = a
    img[base_b:base_b + len(b)] = b
    bb2 = _blocks(offsb, trb, base_b, span_a, len(b))
    both = np.concatenate([ba, bb2])
    ends = [len(a)] * len(ba) + [base_b + len(b)] * len(bb2)
    planes, info = _run_dec_bits(hip, torch, img, img.nbytes, both, ends, Cn, span_a + span_b)
    assert np.array_equal(planes[:, :span_a], alone_a[0])
    assert np.array_equal(planes[:, span_a:], alone_b[0])
    assert np.array_equal(info[:len(ba)], alone_a[1])
    assert np.array_equal(info[len(ba):], alone_b[1])
    # the same launch without the ends lets block 3 of the first image run into the second image
    planes_u, info_u = _run_dec_bits(hip, torch, img, img.nbytes, both, None, Cn, span_a + span_b)
    assert np.array_equal(planes_u[:, span_a:], alone_b[0])
    assert not (np.array_equal(planes_u[:, :span_a], alone_a[0]) and np.array_equal(info_u[:len(ba)], alone_a[1]))


# ------------------------------------------------------------------ handle reuse, scale, arguments

def test_handle_reuse(oracle, hip):
    files = _mixed_files(oracle)
    datas, caps = [d for d, _ in files], [pcm.shape[1] for _, pcm in files]
    dec = make_decoder(hip)
    try:
        first = dec.decode_batch(datas, caps)
        for (data, pcm), cap in zip(files, caps):
            rc, out = dec.decode_whole(data, cap)
            assert rc == OK and np.array_equal(out, pcm)
        again = dec.decode_batch(datas, caps)
        for (r1, o1), (r2, o2), (_, pcm) in zip(first, again, files):
            assert r1 == r2 == OK and np.array_equal(o1, o2) and np.array_equal(o1, pcm)
    finally:
        dec.close()


def test_round_trip_of_300_clips_crosses_the_pass_cap(hip):
    """encode_batch of 300 ten-second stereo clips, one decode_batch: the input PCM exactly, in at least two passes
    (300 x 480 000 x 2 sample-channels > SLA_HIP_DEC_BATCH_PASS)"""
    bases = [S.synth_pcm(2, 480000, 16, 48000, seed=300 + k) for k in range(4)]
    lens = [480000 - (i * 37) % 2000 for i in range(300)]
    pcms = [np.ascontiguousarray(bases[i % 4][:, :n]) for i, n in enumerate(lens)]
    assert sum(lens) * 2 > (1 << 28)
    datas = encode_clips(hip, C4, pcms)
    dec = make_decoder(hip)
    try:
        got = dec.decode_batch(datas)
        assert dec.last_timing()[5] >= 2
    finally:
        dec.close()
    for i, (pcm, (rc, out)) in enumerate(zip(pcms, got)):
        assert rc == OK, (i, rc)
        assert np.array_equal(out, pcm), i


def test_argument_checks(oracle, hip):
    L = hip.lib()
    p, pcm, data, offs, tr = _stream(oracle, seed=50)
    data = bytes(data)
    dec = make_decoder(hip)
    try:
        assert L.sla_hip_decode_batch(None, (hip.DecodeItem * 1)(), 1) == INVALID_ARGUMENT
        assert L.sla_hip_decode_batch(C.c_void_p(dec._h), None, 1) == INVALID_ARGUMENT
        assert L.sla_hip_decode_batch(C.c_void_p(dec._h), None, 0) == 0
        assert dec.decode_batch([]) == []
        # NULL data / NULL planes in the middle of good files: the per-item code DecodeWhole gives, the others decode
        buf = np.frombuffer(data, np.uint8)
        out = np.zeros((3, 2, pcm.shape[1]), np.int32)
        items = (hip.DecodeItem * 3)()
        keep = []
        for i in range(3):
            ptrs = (hip.i32p * 2)(*[out[i, c].ctypes.data_as(hip.i32p) for c in range(2)])
            keep.append(ptrs)
            items[i].data = buf.ctypes.data_as(hip.u8p)
            items[i].data_size = len(buf)
            items[i].buffer_num_samples = pcm.shape[1]
            items[i].buffer = ptrs
            items[i].output_num_samples = 12345
        items[1].data = None
        items[2].buffer = None
        assert L.sla_hip_decode_batch(C.c_void_p(dec._h), items, 3) == 0
        assert items[0].result == OK and items[0].output_num_samples == pcm.shape[1]
        assert np.array_equal(out[0], pcm)
        assert items[1].result == INVALID_ARGUMENT and items[1].output_num_samples == 0
        assert items[2].result == INVALID_ARGUMENT and items[2].output_num_samples == 0
    finally:
        dec.close()
