"""Hand-made block chains for the wide walk (test infrastructure, shared by tests/test_wide_walk_model.py and
tests/test_gpu_dec_walk_wide.py).  A walk reads only the ten header bytes of each block, so the chains here are those
bytes around bodies of filler: bodies stay below 0x80, so that a sync code is wherever a case puts one and nowhere else.
A case is (name, data, total, capacity, max_block_samples)."""
import numpy as np

HEADER = bytes([0x11]) * 43
TILE = 8192                      # bytes one workgroup of the find kernel covers (256 words of 32)


def blk(n, body=b"\x00", crc=0x1234):
    """one block: sync code, size field, CRC field, sample count, body (at least one byte: 11 bytes is the least)"""
    return b"\xff\xff" + (len(body) + 4).to_bytes(4, "big") + crc.to_bytes(2, "big") + n.to_bytes(2, "big") + bytes(body)


def filler(rng, size):
    return bytes(rng.integers(0, 0x80, size, dtype=np.uint8))


def chain(lens, bodies=None, seed=0):
    """(data, offsets) of a chain with the given sample counts; bodies: byte strings or sizes, default 1 to 24 bytes"""
    rng = np.random.default_rng(seed)
    out, offs = bytearray(HEADER), []
    for k, n in enumerate(lens):
        body = bodies[k] if bodies is not None else int(rng.integers(1, 25))
        if isinstance(body, int):
            body = filler(rng, body)
        offs.append(len(out))
        out += blk(n, body, crc=(0x0101 * (k + 1)) & 0xFFFF)
    return bytes(out), offs


def put(data, at, value, width):
    d = bytearray(data)
    d[at:at + width] = int(value).to_bytes(width, "big")
    return bytes(d)


ROUND_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025]


def round_cases():
    out = []
    for L in ROUND_LENGTHS:
        data, _ = chain([3] * L, seed=L)
        if L == 0:
            data += bytes([0x22]) * 20
        out.append(("chain of %d" % L, data, 3 * L if L else 5, 3 * L + 7, 4096))
    return out


def long_case():
    """70 000 eleven-byte blocks: more than 16 doubling rounds"""
    one = np.frombuffer(blk(1, b"\x05"), np.uint8)
    data = HEADER + np.tile(one, 70000).tobytes()
    return ("70000 eleven-byte blocks", data, 70000, 70000, 4096)


def decoy_cases():
    out = []
    rng = np.random.default_rng(7)
    # (a) a decoy in every body that points at the decoy of the next body: a second chain beside the real one
    bodies = []
    for k in range(40):
        b = bytearray(filler(rng, 40))
        b[5:11] = b"\xff\xff" + (50 - 6).to_bytes(4, "big")           # 50: the real blocks' size
        bodies.append(bytes(b))
    data, _ = chain([10] * 40, bodies)
    out.append(("decoys that chain among themselves", data, 400, 400, 4096))
    # (b) decoys that point at the next real block: two predecessors of one node
    bodies = []
    for k in range(40):
        b = bytearray(filler(rng, 40))
        b[7:13] = b"\xff\xff" + (50 - 17 - 6).to_bytes(4, "big")      # from body byte 7 (block byte 17) to the block's end
        bodies.append(bytes(b))
    data, _ = chain([10] * 40, bodies)
    out.append(("decoys that merge into the chain", data, 400, 400, 4096))
    # (c) three real blocks whose bodies hold chains of eleven-byte decoys, far more of them than real blocks
    body = b"".join(blk(9, b"\x01") for _ in range(60)) + b"\x00" * 13
    data, _ = chain([100, 100, 100], [body] * 3)
    out.append(("a decoy chain longer than the real one", data, 300, 300, 4096))
    # (d) dense fields: a sync code and a size field of 2 every six bytes; every eight, where each is the next one's
    #     predecessor
    for name, pat in (("dense field, period 6", b"\xff\xff\x00\x00\x00\x02"), ("dense field, period 8", b"\xff\xff\x00\x00\x00\x02\x00\x00")):
        data, _ = chain([20, 30, 40], [pat * 3000, pat * 1500 + b"\x00" * 3, 5])
        out.append((name, data, 90, 90, 4096))
    return out


def tile_cases(head):
    """a real block whose ten header bytes straddle a chunk, word or tile boundary of the find kernel, for a source
    that is `head` bytes off a 16-byte boundary: the block starts j bytes before the boundary, j = 1 .. 10"""
    out = []
    for bound in (TILE, TILE + 16, TILE + 32, 2 * TILE):
        for j in range(1, 11):
            at = bound - j - head                                      # file position of the straddling block
            first = at - 43 - 10                                       # body of the block in front of it
            data, offs = chain([5, 6, 7], [first, 30, 30], seed=bound + j)
            assert offs[1] == at
            out.append(("header %d bytes before %d" % (j, bound), data, 18, 18, 4096))
    return out


def stop_cases():
    lens = [300, 200, 0, 0, 500, 123]
    n = sum(lens)
    data, offs = chain(lens, seed=11)
    size5 = int.from_bytes(data[offs[5] + 2:offs[5] + 6], "big")
    out = [
        ("clean", data, n, n, 4096),
        ("lost sync at the second block", put(data, offs[1], 0xFF7F, 2), n, n, 4096),
        ("lost sync at the last block", put(data, offs[5], 0x7FFF, 2), n, n, 4096),
        ("size beyond the bytes left", put(data, offs[5] + 2, size5 + 1, 4), n, n, 4096),
        ("size ends at the end", data + b"\x00", n, n, 4096),
        ("ten bytes left", data + b"\xff\xff" + bytes(8), n + 50, n + 50, 4096),
        ("five bytes left", data + b"\xff\xff\x00\x00\x00", n + 50, n + 50, 4096),
        ("the stream ends before total", data, n + 50, n + 50, 4096),
        ("total reached mid-chain", data, 400, n, 4096),
        ("total reached at a block's first sample", data, 300, n, 4096),
        ("total reached in front of zero-sample blocks", data, 500, n, 4096),
        ("total larger than the chain", data, n + 1, n + 1, 4096),
        ("capacity stop", data, n, 300 + 200 + 499, 4096),
        ("capacity stop at the first block", data, n, 299, 4096),
        ("capacity zero", data, n, 0, 4096),
        ("block stop", data, n, n, 499),
        ("block stop at the first block", data, n, n, 200),
        ("header only", data[:43], n, n, 4096),
        ("shorter than its header", data[:20], n, n, 4096),
        ("no samples in the header", data, 0, n, 4096),
        ("no sync at byte 43", put(data, 43, 0xFFFE, 2), n, n, 4096),
        ("size field below the CRC start", put(data, offs[4] + 2, 1, 4), n, n, 4096),
        ("size field just at the CRC start", put(data, offs[4] + 2, 2, 4), n, n, 4096),
    ]
    for v in range(0xFFFFFFFA, 0x100000000):
        out.append(("size field %08X wraps" % v, put(data, offs[1] + 2, v, 4), n, n, 4096))
    zeros, _ = chain([0, 0, 0, 77, 0, 0], seed=12)
    out.append(("zero-sample blocks in a row", zeros, 77, 77, 4096))
    out.append(("zero-sample blocks only", chain([0, 0, 0], seed=13)[0], 77, 77, 4096))
    return out


def all_cases():
    out = round_cases() + [long_case()] + decoy_cases() + stop_cases()
    for head in (0, 13):
        out += tile_cases(head)
    return out
