"""numpy model of the prepass and of the per-file batch scan (include/sla_hip.h: sla_hip_launch_prepass,
sla_hip_launch_prepass_tiles, sla_hip_launch_batch_scan), written from their definitions and from what the oracle's encoder
calls silent: a sample is silent when every channel is zero after right-justify (arithmetic shift by 32 - bits) and, with
mid/side, after mid = (L + R) >> 1 and side = L - R in wrapping 32-bit arithmetic.  Nothing here is derived from the kernels."""
import numpy as np

import zerorunmodel as Z

TILE = 1024


def justified(pcm, bits, mid_side):
    """int32 [channels, n] left-justified input -> the integers the encoder looks at"""
    x = np.asarray(pcm, np.int32) >> np.int32(32 - bits)
    if mid_side:
        assert x.shape[0] == 2
        l, r = x[0].view(np.uint32), x[1].view(np.uint32)
        with np.errstate(over="ignore"):
            mid = (l + r).view(np.int32) >> np.int32(1)
            side = (l - r).view(np.int32)
        x = np.stack([mid, side])
    return x


def prepass(pcm, bits, mid_side):
    """pcm: int32 [channels, n] (the samples only, no stride).  Returns (or_word, mask words, zero-word count, tile words):
    the mask has ceil(n / 64) words, bits at or above n zero; the count includes a partial last word; the tile words are the
    ORs of the raw words per 1024 samples, padded with zeros to ceil(n / 4096) * 4"""
    pcm = np.asarray(pcm, np.int32)
    n = pcm.shape[1]
    raw = pcm.view(np.uint32)
    or_word = int(np.bitwise_or.reduce(raw, axis=None)) if n else 0
    if n == 0:
        return 0, np.zeros(0, np.uint64), 0, np.zeros(0, np.uint32)
    nz = (justified(pcm, bits, mid_side) != 0).any(axis=0)
    mask = Z.mask_words(nz)
    per_sample = np.bitwise_or.reduce(raw, axis=0)
    ntiles = (n + TILE - 1) // TILE
    padded = np.zeros(ntiles * TILE, np.uint32)
    padded[:n] = per_sample
    tiles = np.zeros((n + 4 * TILE - 1) // (4 * TILE) * 4, np.uint32)
    tiles[:ntiles] = np.bitwise_or.reduce(padded.reshape(ntiles, TILE), axis=1)
    return or_word, mask, int((mask == 0).sum()), tiles


def prepass_done(or_word, zero_words, bits):
    """the two words sla_hip_launch_prepass_early leaves for the kernels started beside the prepass (include/sla_hip.h):
    (cancel, lshift).  lshift is the reference's offset_lshift (src/SLAEncoder.c:425-455): 0 for an all-zero file, otherwise
    bits minus the dynamic range 32 - ntz(OR word) -- the number of always-zero bits above the declared unit 2^(32 - bits).
    The start is called off for an OR word of 0, for any all-zero mask word, and for samples wider than `bits` (a bit below
    the unit set: the reference asserts there); lshift is 0 in the first and the last of these."""
    or_word, zero_words, bits = int(or_word), int(zero_words), int(bits)
    assert 0 <= or_word < 2 ** 32 and zero_words >= 0 and 1 <= bits <= 32
    if or_word == 0:
        return 1, 0
    ntz = (or_word & -or_word).bit_length() - 1                 # trailing zeros
    if ntz < 32 - bits:                                         # wider than declared
        return 1, 0
    return (1 if zero_words else 0), ntz - (32 - bits)


def batch_scan(mask, tile_or, starts, lens, max_block):
    """the documented three words per file: OR of the file's own tile words, all-zero WHOLE mask words inside the file, and
    1 when the file's last super-frame has 1 .. 126 samples and all of them are zero"""
    bits = Z.mask_bits(mask, len(mask) * 64)
    info = np.zeros(3 * len(starts), np.uint32)
    for f, (s, n) in enumerate(zip(starts, lens)):
        assert s % TILE == 0
        t0 = s // TILE
        info[3 * f] = np.bitwise_or.reduce(tile_or[t0:t0 + (n + TILE - 1) // TILE]) if n else 0
        whole = bits[s:s + n // 64 * 64].reshape(-1, 64)
        info[3 * f + 1] = int((~whole.any(axis=1)).sum())
        rem = n % max_block if max_block else 0
        info[3 * f + 2] = int(1 <= rem < 127 and not bits[s + n - rem:s + n].any())
    return info
