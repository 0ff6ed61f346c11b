"""Streams and the damage catalogue of the salvage tests (test infrastructure, no GPU): tests/test_salvage_model.py pins
tests/salvagemodel.py with them, tests/test_gpu_salvage.py holds sla_hip_salvage_resident and the scan launcher against
the model on the same cases.

A case is (name, damaged bytes, mode, lost, patches, undecodable): `lost` the silent ranges (start, length, reason) worked
out HERE from the blocks the case damaged -- not by the model --, `patches` a list of (dst sample, src sample, length)
that says where samples of the clean PCM appear at another place (the embedded block), `undecodable` the byte positions
of blocks whose CRC holds and which no decoder can decode.  The expected PCM of a case is the clean PCM with the lost
ranges zeroed and the patches applied.
"""
import numpy as np

import salvagemodel as SM
import slalibs as S
import slastream as W
import walkmodel as WM

CAP_N = 4096                     # max_num_block_samples of the handles and of the model
CRC, UNDEC, GAP = SM.CRC, SM.UNDECODABLE, SM.GAP


def blocks_of(data):
    """(byte offset, byte length, first sample, samples) of every block of a clean stream"""
    total = WM.header_total(data)
    w = WM.walk(data, total, total, CAP_N, 1)
    assert w.stop == WM.OK and w.extent == total
    return [(off, blen, smp, n) for off, blen, smp, n, _, _ in w.rows]


# ---- streams ------------------------------------------------------------------------------------------------------

SHAPES = {
    # name: (channels, bits, mid/side, block samples, samples)
    "mono16": (1, 16, 0, 3000, 9 * 3000 + 2100),
    "stereo16ms": (2, 16, 1, 4096, 8 * 4096 + 2049),
    "three24": (3, 24, 0, 2048, 8 * 2048 + 2500),
}


def params_of(shape):
    nch, bits, ms, blk, n = SHAPES[shape]
    return S.make_params(nch, bits, 48000, 16, 1, 8, ms, 1, CAP_N, cap=(8, CAP_N, 48, 5, 32))


def oracle_stream(oracle, shape):
    """-> (clean bytes, clean PCM [C][N] left-justified): the oracle's encoder with fixed blocks, its own decode"""
    nch, bits, ms, blk, n = SHAPES[shape]
    p = params_of(shape)
    pcm = S.synth_pcm(nch, n, bits, 48000, seed=4100 + n)
    ret, data = oracle.encode_fixed_blocks(p, pcm, blk)
    assert ret == 0
    ret, dec, _ = oracle.decode_whole(p, data, n)
    assert ret == 0 and np.array_equal(dec, pcm)
    assert 8 <= len(blocks_of(data)) <= 10
    return data, dec


RAW_FMT = W.Format(num_channels=1, bits=16, order=8, ntaps=1, lms=8, ms=0, max_block=CAP_N)
RAW_LENS = [2048, 3000, 2100, 4096, 2500, 3500, 2048, 3333, 2222]


def _raw_block(samples):
    """a RAW block of a mono 16-bit file holding these right-justified samples"""
    return W.Block(W.RAW, len(samples), raw=[W.fold_array(samples)])


def raw_stream(decoy=False, embed=False, type3=None):
    """a mono 16-bit stream of RAW blocks written by tests/slastream.py -> (bytes, PCM [1][N], blocks).
    decoy: block 6's payload holds FF FF, a plausible size field and a wrong CRC.  embed: the tail of block 5's payload is a
    complete copy of block 2, which so ends exactly where block 5 ends.  type3: that block is written with block type 3."""
    rng = np.random.default_rng(77)
    smp = [rng.integers(-20000, 20000, n).astype(np.int64) for n in RAW_LENS]
    if decoy:
        # sync, size field 0x20 (+ 6 = 38 bytes, inside the block), CRC field, 16 samples -- as the words of ten bytes
        words = [0xFFFF, 0x0000, 0x0020, 0x1234, 0x0010]
        for k, wd in enumerate(words):
            u = wd                                  # the coded (folded) value: unfold it to get the sample
            smp[6][100 + k] = -((u + 1) >> 1) if (u & 1) else (u >> 1)
    blocks = [_raw_block(s) for s in smp]
    if embed:
        inner = W.block_bytes(RAW_FMT, blocks[2])
        assert len(inner) < 2 * RAW_LENS[5]
        payload = W.block_bytes(RAW_FMT, blocks[5])[11:]
        payload = payload[:len(payload) - len(inner)] + inner
        u = np.frombuffer(payload, ">u2").astype(np.int64)
        smp[5] = np.where(u & 1, -((u + 1) >> 1), u >> 1)
        blocks[5] = _raw_block(smp[5])
        assert W.block_bytes(RAW_FMT, blocks[5])[11:] == payload
    if type3 is not None:
        blocks[type3] = W.Block(3, RAW_LENS[type3])
    data, _, offs = W.write_file(RAW_FMT, blocks)
    pcm = (np.concatenate(smp) << 16).astype(np.int64).astype(np.int32)[None, :]
    return data, pcm, blocks


# ---- damage -------------------------------------------------------------------------------------------------------

def _flip(data, pos):
    d = bytearray(data)
    d[pos] ^= 0x55
    return bytes(d)


def _kill_sync(data, off):
    d = bytearray(data)
    d[off] = 0x00
    return bytes(d)


FILLER = bytes(((7 * i + 1) & 0x7F) for i in range(100))          # no FF in it


def catalogue(data):
    """the damage kinds of the issue on a clean stream of 8 to 10 blocks -> cases"""
    b = blocks_of(data)
    total = WM.header_total(data)
    last = len(b) - 1
    body = lambda k: b[k][0] + b[k][1] // 2
    rng_of = lambda k, why: (b[k][2], b[k][3], why)
    span = lambda k0, k1, why: (b[k0][2], b[k1][2] + b[k1][3] - b[k0][2], why)
    cases = [("clean", data, 1, [], [], ())]
    for k, name in ((0, "first"), (4, "middle"), (last, "last")):
        cases.append(("a body byte flipped in the %s block" % name, _flip(data, body(k)), 1, [rng_of(k, CRC)], [], ()))
    cases.append(("body bytes flipped in two blocks", _flip(_flip(data, body(2)), body(6)), 1, [rng_of(2, CRC), rng_of(6, CRC)], [], ()))
    d = bytearray(data)
    d[b[3][0] + 2:b[3][0] + 6] = (b[3][1] - 6 + 5).to_bytes(4, "big")
    cases.append(("a size field corrupted", bytes(d), 2, [rng_of(3, GAP)], [], ()))
    cases.append(("a sync code destroyed", _kill_sync(data, b[4][0]), 2, [rng_of(4, GAP)], [], ()))
    d = bytearray(data)
    d[b[5][0] + 8:b[5][0] + 10] = (b[5][3] - 7).to_bytes(2, "big")
    cases.append(("a sample count lowered", bytes(d), 2, [rng_of(5, GAP)], [], ()))
    d = bytearray(data)
    d[b[5][0] + 8:b[5][0] + 10] = (b[5][3] + 7).to_bytes(2, "big")
    cases.append(("a sample count raised", bytes(d), 2, [rng_of(5, GAP)], [], ()))
    cases.append(("100 bytes deleted inside a block", data[:body(3)] + data[body(3) + 100:], 2, [rng_of(3, GAP)], [], ()))
    cases.append(("100 bytes inserted inside a block", data[:body(6)] + FILLER + data[body(6):], 2, [rng_of(6, GAP)], [], ()))
    cases.append(("two breaks with good blocks between them", _kill_sync(_kill_sync(data, b[2][0]), b[6][0]), 2, [span(2, 6, GAP)], [], ()))
    cases.append(("truncated inside a block", data[:body(7)], 2, [(b[7][2], total - b[7][2], GAP)], [], ()))
    cases.append(("truncated inside the first block", data[:body(0)], 2, [(0, total, GAP)], [], ()))
    cases.append(("the first sync code destroyed", _kill_sync(data, b[0][0]), 2, [rng_of(0, GAP)], [], ()))
    cases.append(("the last sync code destroyed", _kill_sync(data, b[last][0]), 2, [rng_of(last, GAP)], [], ()))
    cases.append(("bytes appended behind the last block and a break", _kill_sync(data, b[4][0]) + FILLER[:9], 2,
                  [(b[4][2], total - b[4][2], GAP)], [], ()))
    return cases


def raw_cases():
    """the cases that need a hand-written stream -> [(cases, clean PCM)]"""
    out = []
    data, pcm, _ = raw_stream(decoy=True)
    b = blocks_of(data)
    out.append(([("a decoy in a payload, chain intact", data, 1, [], [], ()),
                 ("a decoy in a payload behind a break", _kill_sync(data, b[3][0]), 2, [(b[3][2], b[3][3], GAP)], [], ()),
                 ("a decoy in a payload in front of a break", _kill_sync(data, b[7][0]), 2, [(b[7][2], b[7][3], GAP)], [], ())], pcm))
    data, pcm, _ = raw_stream(embed=True)
    b = blocks_of(data)
    total = WM.header_total(data)
    d = bytearray(data)
    d[b[5][0] + 2:b[5][0] + 6] = (b[5][1] - 6 + 3).to_bytes(4, "big")
    # block 5 is not sound any more; the copy of block 2 in its payload is, and chains to the end: it becomes q, its samples
    # are delivered right-aligned with the suffix, the rest of block 5's range is the gap
    n2, n5 = b[2][3], b[5][3]
    out.append(([("an embedded valid block, chain intact", data, 1, [], [], ()),
                 ("an embedded valid block chained to the end is picked", bytes(d), 2, [(b[5][2], n5 - n2, GAP)],
                  [(b[5][2] + n5 - n2, b[2][2], n2)], ())], pcm))
    data, pcm, _ = raw_stream(type3=4)
    b = blocks_of(data)
    out.append(([("a block of type 3 whose CRC holds", data, 1, [(b[4][2], b[4][3], UNDEC)], [], (b[4][0],)),
                 ("a block of type 3 behind a break", _kill_sync(data, b[1][0]), 2, [(b[1][2], b[1][3], GAP), (b[4][2], b[4][3], UNDEC)], [],
                  (b[4][0],))], pcm))
    return out


def expected_pcm(pcm, lost, patches):
    out = pcm.copy()
    for dst, src, n in patches:
        out[:, dst:dst + n] = pcm[:, src:src + n]
    for start, length, _ in lost:
        out[:, start:start + length] = 0
    return out
