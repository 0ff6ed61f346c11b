"""GPU tests of the encoder's verification pass (option "verify", include/sla_hip.h; run with -m gpu).

1. k_verify_blocks alone (sla_hip_launch_verify_blocks) on crafted planes, block tables and parser records against a
   numpy model: mid/side inverse, left shift, 32-bit compare, first position, per-segment sums, bad-block count.
2. sla_hip_verify_last_image: the image a device pack (or a non-streamed EncodeWhole) left on the device, against the
   original planes and against planes with one flipped bit.
3. verify = 1 changes no byte and no result on any route, and compares every sample of every delivered file.

Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

import slalibs as S
import waveforms as W
from test_oracle_golden import load_case

pytestmark = pytest.mark.gpu

NONE = 2 ** 64 - 1
HEADER_ONLY = 1
NG, INSUFFICIENT_BUFFER_SIZE, PARAMETER_NOT_SET = 1, 4, 15


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_encoder(hip, p):
    enc = hip.Encoder(p.cap_channels, p.cap_block_samples, p.cap_parcor_order, p.cap_longterm_order, p.cap_lms_order)
    enc.set_wave_format(p.num_channels, p.bits_per_sample, p.sampling_rate)
    enc.set_encode_parameter(p.parcor_order, p.longterm_order, p.lms_order, p.ch_process_method, p.window_type, p.max_block_samples)
    return enc


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------------------------------
DEC_BLOCK = np.dtype([("byte_off", "<u8"), ("byte_len", "<u4"), ("smp_off", "<u4"), ("num_samples", "<u4"), ("flags", "<u4")])
DEC_INFO = np.dtype([("type", "<u4"), ("used_bytes", "<u4"), ("crc", "<u4"), ("overrun", "<u4")])
EXPECT = np.dtype([("type", "<u4"), ("bytes", "<u4")])
assert DEC_BLOCK.itemsize == 24 and DEC_INFO.itemsize == 16 and EXPECT.itemsize == 8

LENGTHS = [1, 63, 64, 65, 255, 2048, 2048, 65]          # the seventh block is HEADER_ONLY
GAPS = [3, 0, 1, 0, 5, 0, 2, 0]                          # plane positions left out behind each block
HEADER_ONLY_BLOCK = 6


def layout(first):
    blocks = np.zeros(len(LENGTHS), DEC_BLOCK)
    pos, byte = first, 43
    for i, (n, gap) in enumerate(zip(LENGTHS, GAPS)):
        blocks[i] = (byte, 16 + i, pos, n, HEADER_ONLY if i == HEADER_ONLY_BLOCK else 0)
        pos += n + gap
        byte += 16 + i
    return blocks, pos, byte


def finish(dec, ms, shift):
    """the decoder's last stage on right-justified planes [C][n] (src/SLAUtility.c:415-433, src/SLADecoder.c:540-547)"""
    wrap = lambda v: ((v + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31          # int32 arithmetic wraps, as the reference's C does
    out = dec.astype(np.int64)
    if ms:
        side = out[1]
        mid = wrap((out[0] << 1) | (side & 1))
        out = np.stack([wrap(mid + side) >> 1, wrap(mid - side) >> 1])
    return ((out << shift) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def model(dec, src, blocks, info, expect, seg_of, nsegs, ms, shift, image):
    """the report words the kernel must produce: per segment [differing, first (position << 3 | channel), bad blocks]"""
    rep = np.zeros((nsegs, 3), np.uint64)
    rep[:, 1] = NONE
    for b, blk in enumerate(blocks):
        if blk["flags"] & HEADER_ONLY:
            continue
        sg = seg_of[b]
        lo, hi = int(blk["smp_off"]), int(blk["smp_off"]) + int(blk["num_samples"])
        diff = finish(dec[:, lo:hi], ms, shift) != src[:, lo:hi]
        ch, at = np.nonzero(diff)
        if len(ch):
            rep[sg, 0] += np.uint64(len(ch))
            rep[sg, 1] = min(int(rep[sg, 1]), int((((at + lo) << 3) | ch).min()))
        bad = info[b]["type"] != expect[b]["type"] or info[b]["used_bytes"] != expect[b]["bytes"] or info[b]["overrun"] != 0
        if image is not None:
            o = int(blk["byte_off"])
            bad = bad or ((int(image[o + 6]) << 8) | int(image[o + 7])) != info[b]["crc"]
        rep[sg, 2] += np.uint64(bool(bad))
    return rep


class Case:
    """planes, tables and records of one launch, host copies the model reads and the plants go into"""

    def __init__(self, nch, ms, shift, first, nsegs, seed, src_misaligned=False):
        rng = np.random.default_rng(seed)
        self.nch, self.ms, self.shift, self.nsegs = nch, ms, shift, nsegs
        self.blocks, span, nbytes = layout(first)
        nb = len(self.blocks)
        self.stride, self.sstride = span + 7, span + 13 + (0 if src_misaligned else 3)
        self.src_pad = 1 if src_misaligned else 0               # the source planes start one word into their allocation
        bits = 32 - shift
        self.dec = rng.integers(-(1 << (bits - 1)) + 1, (1 << (bits - 1)) - 1, (nch, self.stride), dtype=np.int64).astype(np.int32)
        # the source: what the decoded planes finish to inside the blocks, something else everywhere outside them, so that a
        # read outside a block's range (a gap, the padding behind the last block) would count
        self.src = rng.integers(-2 ** 31, 2 ** 31 - 1, (nch, self.sstride), dtype=np.int64).astype(np.int32)
        inside = np.zeros(self.stride, bool)
        for blk in self.blocks:
            lo, n = int(blk["smp_off"]), int(blk["num_samples"])
            self.src[:, lo:lo + n] = finish(self.dec[:, lo:lo + n], ms, shift)
            inside[lo:lo + n] = True
        self.gap = [int(g) for g in np.nonzero(~inside[:span])[0]]
        self.seg_of = (np.arange(nb) * nsegs // nb).astype(np.uint32)
        self.expect = np.zeros(nb, EXPECT)
        self.expect["type"] = rng.integers(0, 3, nb)
        self.expect["bytes"] = self.blocks["byte_len"]
        self.info = np.zeros(nb, DEC_INFO)
        self.info["type"], self.info["used_bytes"] = self.expect["type"], self.expect["bytes"]
        self.info["crc"] = rng.integers(0, 65536, nb)
        self.image = rng.integers(0, 256, (nbytes + 3) & ~3, dtype=np.int64).astype(np.uint8)
        for b, blk in enumerate(self.blocks):
            o = int(blk["byte_off"])
            self.image[o + 6], self.image[o + 7] = int(self.info["crc"][b]) >> 8, int(self.info["crc"][b]) & 255

    def run(self, hip, with_image=True, with_segments=True):
        import torch
        d_dec = dev(self.dec)
        d_src_buf = dev(np.concatenate([np.zeros(self.src_pad, np.int32), self.src.reshape(-1)]))
        d_blocks, d_info, d_expect = dev(self.blocks.view(np.uint8)), dev(self.info.view(np.uint8)), dev(self.expect.view(np.uint8))
        d_seg, d_image = dev(self.seg_of.view(np.int32)), dev(self.image)
        init = np.zeros((self.nsegs, 3), np.uint64)
        init[:, 1] = NONE
        d_rep = dev(init.view(np.int64))
        rc = hip.lib().sla_hip_launch_verify_blocks(
            d_dec.data_ptr(), self.stride, d_src_buf.data_ptr() + 4 * self.src_pad, self.sstride, d_blocks.data_ptr(),
            d_info.data_ptr(), d_expect.data_ptr(), d_seg.data_ptr() if with_segments else None, len(self.blocks), self.nch,
            self.ms, self.shift, d_image.data_ptr() if with_image else None, len(self.image), d_rep.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        got = d_rep.cpu().numpy().view(np.uint64)
        seg_of = self.seg_of if with_segments else np.zeros_like(self.seg_of)
        want = model(self.dec, self.src[:, :self.stride], self.blocks, self.info, self.expect, seg_of, self.nsegs, self.ms,
                     self.shift, self.image if with_image else None)
        return got, want

    def flip(self, ch, pos, bit):
        self.src[ch, pos] ^= np.int32(1 << bit) if bit < 31 else np.int32(-2 ** 31)


FORMATS = [(1, 0), (2, 0), (2, 1), (8, 0)]
SHIFTS = [0, 8, 16, 17]
FIRSTS = [0, 1, 67, 128]


def seam_positions(blk):
    """plane positions on either side of the seam between lane 63 and lane 64 of the block's workgroup (a lane takes the
    four positions of one 16-byte group), and the block's own samples 63 / 64"""
    lo, n = int(blk["smp_off"]), int(blk["num_samples"])
    base = lo & ~3
    return [q for q in (base + 4 * 63 + 3, base + 4 * 64, lo + 63, lo + 64) if lo <= q < lo + n]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("nch,ms", FORMATS)
def test_kernel_against_model(hip, nch, ms, shift):
    for first in FIRSTS:
        for nsegs in (2, 3):
            seed = 1000 * nch + 100 * ms + shift + 7 * first + nsegs
            c = Case(nch, ms, shift, first, nsegs, seed, src_misaligned=(first == 67))
            # clean: the words stay as the caller set them
            got, want = c.run(hip)
            assert (want == [0, NONE, 0]).all() and (got == want).all(), (first, nsegs)

            # differences in the last segment only: the last sample of the last block, in the last channel
            last = c.blocks[-1]
            c.flip(nch - 1, int(last["smp_off"]) + int(last["num_samples"]) - 1, 31)
            got, want = c.run(hip)
            assert want[-1, 0] == 1 and (want[:-1, 0] == 0).all() and (got == want).all(), (first, nsegs)

            # and in several: the first sample of the first block, the lane seam of the long block, a bit below `shift`,
            # a gap between two blocks and the inside of the HEADER_ONLY block (those two must not count)
            c.flip(0, int(c.blocks[0]["smp_off"]), 31 if shift == 0 else shift)
            planted = 2
            for q in seam_positions(c.blocks[5]):
                c.flip(q % nch, q, 30)
                planted += 1
            if shift > 0:
                c.flip(nch - 1, int(c.blocks[4]["smp_off"]) + 100, 0)           # the source's own low bits: they count
                planted += 1
            for q in c.gap:
                c.flip(0, q, 29)
            ho = c.blocks[HEADER_ONLY_BLOCK]
            c.flip(0, int(ho["smp_off"]) + 5, 29)
            got, want = c.run(hip)
            assert want[:, 0].sum() == planted and want[0, 1] == (int(c.blocks[0]["smp_off"]) << 3), (first, nsegs)
            assert (got == want).all(), (first, nsegs, got, want)
            # no segment table: everything is segment 0
            got, want = c.run(hip, with_segments=False)
            assert want[0, 0] == planted and (want[1:] == [0, NONE, 0]).all() and (got == want).all(), (first, nsegs)


def test_kernel_bad_blocks(hip):
    for nch, ms, shift, first, nsegs in [(2, 1, 16, 0, 2), (1, 0, 8, 67, 3), (8, 0, 0, 1, 3)]:
        c = Case(nch, ms, shift, first, nsegs, 99 + first)
        c.info["type"][0] = (c.info["type"][0] + 1) % 4                  # wrong type
        c.info["used_bytes"][2] += 1                                    # one byte too many
        c.info["used_bytes"][3] -= 1                                    # one too few
        c.info["overrun"][7] = 1
        c.info["type"][HEADER_ONLY_BLOCK] = 3                           # a HEADER_ONLY block is skipped altogether
        got, want = c.run(hip)
        assert want[:, 2].sum() == 4 and (want[:, 0] == 0).all() and (got == want).all()
        # the CRC16 field of the image against what the parser computed
        o = int(c.blocks[4]["byte_off"])
        c.image[o + 7] ^= 1
        got, want = c.run(hip)
        assert want[:, 2].sum() == 5 and (got == want).all()
        # without an image the field is not looked at; a block that fails two checks is still one bad block
        c.image[int(c.blocks[0]["byte_off"]) + 6] ^= 0x80
        got, want = c.run(hip, with_image=False)
        assert want[:, 2].sum() == 4 and (got == want).all()
        got, want = c.run(hip)
        assert want[:, 2].sum() == 5 and (got == want).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. sla_hip_verify_last_image
# ---------------------------------------------------------------------------------------------------------------------
N_SHORT = 3 * 4096 + 17


def small_files():
    """(name, params, planes): stereo mid/side 16-bit, 8 channels 24-bit, a file with silent blocks, one with RAW blocks"""
    p2 = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096)
    p8 = S.make_params(8, 24, 48000, 16, 1, 8, 0, 1, 4096)
    files = [("stereo_ms", p2, S.synth_pcm(2, N_SHORT, 16, 48000, seed=21)),
             ("eight_24", p8, W.music_like(8, N_SHORT, 24, seed=22))]
    for name, kind in (("c2_gaps", 1), ("raw_white", 2)):
        g, p, pcm = load_case(name)
        assert (g["blk_type"] == kind).any(), name               # the recorded reference run: SILENT / RAW blocks are there
        files.append((name, p, np.ascontiguousarray(pcm)))
    return files


FILES = small_files()


def block_types(enc):
    tr = enc.trace(want_residuals=False)
    return tr, [int(t) for t in tr.blk_type[:tr.num_blocks]]


@pytest.mark.parametrize("name,p,pcm", FILES, ids=[f[0] for f in FILES])
def test_verify_last_image(oracle, hip, name, p, pcm):
    import torch
    nch, n = pcm.shape
    enc = make_encoder(hip, p)
    try:
        d = dev(pcm)
        with pytest.raises(hip.SlaError) as err:                  # before any pack
            enc.verify_last_image(d.data_ptr(), n)
        assert err.value.code == PARAMETER_NOT_SET
        enc.analyze_device(d.data_ptr(), n, n)
        with pytest.raises(hip.SlaError) as err:                  # analysed, not packed
            enc.verify_last_image(d.data_ptr(), n)
        assert err.value.code == PARAMETER_NOT_SET
        data = enc.pack(8 * nch * n + 65536, on_device=True)
        ret, want = oracle.encode_whole(p, pcm)
        assert ret == 0 and data == want
        tr, types = block_types(enc)
        if name == "c2_gaps":
            assert 1 in types
        if name == "raw_white":
            assert 2 in types
        nb = tr.num_blocks
        assert enc.verify_last_image(d.data_ptr(), n) == (nch * n, 0, NONE, nb, 0)
        assert enc.last_verify() == (0, 0, 0, 0, 0)              # the option is off: the call on demand leaves this alone
        # the same planes at another stride, starting one word into their allocation (no 16-byte alignment)
        wide = torch.zeros(nch * (n + 5) + 1, dtype=torch.int32, device="cuda")
        view = wide[1:].view(nch, n + 5)
        view[:, :n] = d
        assert enc.verify_last_image(view.data_ptr(), n + 5) == (nch * n, 0, NONE, nb, 0)
        # one flipped bit: at both ends of the file and on both sides of every block boundary
        bounds = [int(s) for s in tr.blk_start[1:nb]]
        spots = [0, n - 1] + [b - 1 for b in bounds] + bounds
        low_bit = 32 - p.bits_per_sample                          # the lowest bit the format carries
        for k, s in enumerate(spots):
            ch = k % nch
            for bit in (low_bit + (k % 3), 0):                    # bit 0 lies below every sample: stray low bits count
                bad = d.clone()
                bad[ch, s] ^= (1 << bit)
                assert enc.verify_last_image(bad.data_ptr(), n) == (nch * n, 1, (s << 3) | ch, nb, 0), (s, ch, bit)
        # arguments
        L = hip.lib()
        c5 = (C.c_uint64 * 5)()
        assert L.sla_hip_verify_last_image(enc._h, None, n, c5) == 2
        assert L.sla_hip_verify_last_image(enc._h, C.c_void_p(d.data_ptr()), n - 1 if n > 1 else 0, c5) == 2      # stride too short
        host = np.zeros((nch, n), np.int32)
        assert L.sla_hip_verify_last_image(enc._h, C.c_void_p(host.ctypes.data), n, c5) == 2                        # not device memory
        if nch > 1:
            # a stride that carries the second channel past any allocation (the tensor may sit inside a larger pooled one)
            assert L.sla_hip_verify_last_image(enc._h, C.c_void_p(d.data_ptr()), 1 << 40, c5) == 2
        # a batch leaves no such image, a non-streamed EncodeWhole does
        enc.encode_batch([pcm, pcm[:, :n // 2]])
        with pytest.raises(hip.SlaError) as err:
            enc.verify_last_image(d.data_ptr(), n)
        assert err.value.code == PARAMETER_NOT_SET
        assert enc.encode_whole(pcm) == want
        assert enc.verify_last_image(d.data_ptr(), n) == (nch * n, 0, NONE, nb, 0)
        bad = d.clone()
        bad[nch - 1, n // 2] ^= -2 ** 31
        assert enc.verify_last_image(bad.data_ptr(), n) == (nch * n, 1, ((n // 2) << 3) | (nch - 1), nb, 0)
    finally:
        enc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. verify = 1 changes no byte and compares everything
# ---------------------------------------------------------------------------------------------------------------------
def both(hip, p, call, **options):
    """call(enc) with verify 0 and 1 on handles of the same options; returns (result off, result on, counters on)"""
    out = []
    for v in (0, 1):
        enc = make_encoder(hip, p)
        try:
            for k, val in options.items():
                enc.set_option(k, val)
            enc.set_option("verify", v)
            out.append(call(enc))
            out.append(enc.last_verify())
            if v == 1:                                            # switched off again: the next call reports nothing
                enc.set_option("verify", 0)
                assert enc.last_verify() == (0, 0, 0, 0, 0)
                assert call(enc) == out[-2]
                assert enc.last_verify() == (0, 0, 0, 0, 0)
        finally:
            enc.close()
    off, ctr_off, on, ctr_on = out
    assert ctr_off == (0, 0, 0, 0, 0)
    return off, on, ctr_on


def test_the_option_is_zero_or_one(hip):
    enc = make_encoder(hip, FILES[0][1])
    try:
        for bad in (2, -1, 0.5):
            with pytest.raises(hip.SlaError):
                enc.set_option("verify", bad)
        assert enc.last_verify() == (0, 0, 0, 0, 0)
    finally:
        enc.close()


@pytest.mark.parametrize("name,p,pcm", FILES, ids=[f[0] for f in FILES])
def test_encode_whole_verified(oracle, hip, name, p, pcm):
    off, on, ctr = both(hip, p, lambda enc: enc.encode_whole(pcm))
    ret, want = oracle.encode_whole(p, pcm)
    assert ret == 0 and off == want and on == want
    assert ctr[:3] == (pcm.size, 0, NONE) and ctr[3] > 0 and ctr[4] == 0


@pytest.mark.parametrize("lanes", [1, 3])
def test_streamed_encode_whole_verified(oracle, hip, lanes):
    p = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096)
    pcm = S.synth_pcm(2, 20011, 16, 48000, seed=31)
    off, on, ctr = both(hip, p, lambda enc: enc.encode_whole(pcm), stream_piece=1024, stream_lanes=lanes)
    ret, want = oracle.encode_whole(p, pcm)
    assert ret == 0 and off == want and on == want
    assert ctr[:3] == (pcm.size, 0, NONE) and ctr[3] > 0 and ctr[4] == 0
    # the call really ran on the lanes: the handle holds no image afterwards
    enc = make_encoder(hip, p)
    try:
        enc.set_option("stream_piece", 1024)
        enc.set_option("stream_lanes", lanes)
        enc.set_option("verify", 1)
        enc.encode_whole(pcm)
        with pytest.raises(hip.SlaError) as err:
            enc.trace()
        assert err.value.code == PARAMETER_NOT_SET
        with pytest.raises(hip.SlaError) as err:
            enc.verify_last_image(dev(pcm).data_ptr(), pcm.shape[1])
        assert err.value.code == PARAMETER_NOT_SET
    finally:
        enc.close()


def short_batch():
    p = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096)
    pcms = [S.synth_pcm(2, 9000, 16, 48000, seed=41), np.zeros((2, 0), np.int32), W.music_like(2, 12289, 16, seed=42),
            (W.music_like(2, 5000, 16, seed=43) >> 18) << 18, S.synth_pcm(2, 4097, 16, 48000, seed=44, gaps=True)]
    caps = [8 * 2 * x.shape[1] + 65536 for x in pcms]
    caps[2] = 1000                                               # too small: that file is not delivered
    return p, pcms, caps


def test_encode_batch_verified(oracle, hip):
    p, pcms, caps = short_batch()
    off, on, ctr = both(hip, p, lambda enc: enc.encode_batch(pcms, capacities=caps))
    assert off == on
    assert [rc for rc, _ in on] == [0, 0, INSUFFICIENT_BUFFER_SIZE, 0, 0]
    for i in (0, 1, 3, 4):
        assert on[i][1] == oracle.encode_whole(p, pcms[i])[1], i
    delivered = sum(x.size for i, x in enumerate(pcms) if i != 2)
    assert ctr[:3] == (delivered, 0, NONE) and ctr[3] > 0 and ctr[4] == 0


def test_encode_batch_tensor_verified(oracle, hip):
    import torch
    p, pcms, caps = short_batch()
    lens = [x.shape[1] for x in pcms]
    t = torch.zeros((len(pcms), 2, max(lens)), dtype=torch.int32, device="cuda")
    for i, pcm in enumerate(pcms):
        t[i, :, :lens[i]] = dev(pcm)
    off, on, ctr = both(hip, p, lambda enc: enc.encode_batch_tensor(t, lens))
    assert off == on and all(rc == 0 for rc, _ in on)
    for i, pcm in enumerate(pcms):
        assert on[i][1] == oracle.encode_whole(p, pcm)[1], i
    assert ctr[:3] == (sum(x.size for x in pcms), 0, NONE) and ctr[3] > 0 and ctr[4] == 0
    # with the too-small buffer (encode_batch_from takes capacities)
    srcs = [t[i, :, :lens[i]] for i in range(len(pcms))]
    off, on, ctr = both(hip, p, lambda enc: enc.encode_batch_from(srcs, hip.PCM_S32_LEFT, capacities=caps))
    assert off == on and [rc for rc, _ in on] == [0, 0, INSUFFICIENT_BUFFER_SIZE, 0, 0]
    assert ctr[:3] == (sum(x.size for i, x in enumerate(pcms) if i != 2), 0, NONE) and ctr[4] == 0


def test_big_batch_on_lanes_verified(oracle, hip):
    """the recipe of test_gpu_batch.py::test_big_batch_on_lanes: 18 stereo files, more than 16 Mi samples together"""
    p = S.make_params(2, 16, 48000, 16, 1, 8, 1, 1, 4096, cap=(2, 4096, 16, 1, 8))
    rng = np.random.default_rng(77)
    lens = [int(v) for v in rng.integers(500000, 800000, size=18)]
    lens[5] = 4097
    lens[11] = 0
    pcms = [S.synth_pcm(2, max(n, 1), 16, 48000, seed=300 + i) if i % 3 else W.music_like(2, max(n, 1), 16, seed=300 + i) for i, n in enumerate(lens)]
    pcms[11] = np.zeros((2, 0), np.int32)
    pcms[3][:, 100000:160000] = 0
    pcms[7] = (pcms[7] >> 18) << 18
    assert sum(lens) * 2 >= (16 << 20)
    caps = [8 * 2 * n + 65536 for n in lens]
    caps[9] = 1000
    got = {}
    for v in (0, 1):
        enc = make_encoder(hip, p)
        try:
            enc.set_option("batch_lanes", 4)
            enc.set_option("verify", v)
            got[v] = (enc.encode_batch(pcms, capacities=caps), enc.last_verify())
        finally:
            enc.close()
    assert got[0][0] == got[1][0] and got[0][1] == (0, 0, 0, 0, 0)
    assert [rc for rc, _ in got[1][0]] == [INSUFFICIENT_BUFFER_SIZE if i == 9 else 0 for i in range(18)]
    for i in (5, 11):
        assert got[1][0][i][1] == oracle.encode_whole(p, pcms[i])[1], i
    ctr = got[1][1]
    assert ctr[:3] == (sum(x.size for i, x in enumerate(pcms) if i != 9), 0, NONE) and ctr[3] > 0 and ctr[4] == 0
