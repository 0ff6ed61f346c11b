"""Legal .sla streams that the project's encoder never writes, pinned to the unmodified reference decoder (CPU).

tests/crafted_catalogue.py writes them field by field with tests/slastream.py: PARCOR codes at the ends of their fields,
every rshift, orders across the HIP decoder's lattice specialisations, unstable lattices; 1-5 long-term taps (2 and 4
included) at full scale, pitch 3 / 255 / 256 / the top of the reference's ring buffer, delay = n - 1 / n / n + 1, the flag
set with pitch 0; initial Rice parameters 0 / 1 / 8 / 9, channel averages of exactly 8 and 9 (Golomb with moduli up to
57), 2^16 / 2^24 - 1 / 2^24 / 2^32 - 1; quotients 15 / 16 / 17; residuals INT32_MIN / INT32_MAX / -1; tiles of more than
64 bits per sample; 4 / 12 / 20 / 32-bit formats with and without lshift and mid/side, 32-bit mid/side RAW blocks (a
33-bit side field); 1, 2, 3 and 8 channels; block lengths 1, LMS order - 1, LMS order, 63 / 64 / 65, 4097 and 16384 for
LMS orders 4 / 8 / 16 / 32.  For every case the oracle's decoder (the yardstick of the HIP decoder) and the reference
decoder give the same result code and the same samples.

Left out, because the reference is undefined there (those fields get only the "without harm" treatment of
tests/test_gpu_decoder.py::test_garbage_reaches_the_kernels_without_harm):
  * long-term taps outside the reference's ring buffer.  SLALongTermSynthesizer_Create (reference
    src/SLAPredictor.c:991) allocates 2 * (max taps + 256) words and ProcessCore (:1080) reads
    signal_buffer[buffer_pos + max_delay - 1 - j]: a pitch below ceil(taps / 2) indexes below the buffer, a pitch
    above max taps + 256 - taps / 2 beyond it.
  * reads of more than 32 bits that start with exactly one bit left in the reader's byte buffer.
    SLABitReader_GetBits (reference src/include/private/SLABitStream.h:241-243) shifts a 32-bit value by
    nbits - bit_count, which is 32 there (undefined in C; on x86 the top bit of the field lands in bit 0).  The only
    such field of a legal stream is the 33-bit side channel of a 32-bit mid/side RAW block; the catalogue keeps that
    field's top bit clear at those positions and sets it elsewhere.  (A gamma code wider than 32 bits is the other
    one; a quotient never needs it.)
  * LMS orders other than 4 / 8 / 16 / 32 in the file header.  The reference asserts a power of two of at least 4
    (src/SLAPredictor.c:1355-1356), but is built with -DNDEBUG: it then decodes orders 1, 2, 3, 6, 12 and 24 with a
    filter whose ring buffer it sizes for the handle's maximum (:1139), and crashes on order 0.  The oracle and the HIP
    decoder refuse such a stream with FAILED_TO_SYNTHESIZE (oracle/sla_oracle.c: lms_run); no encoder writes one, and
    following the reference would put an unasserted code path of it into both.  test_lms_orders_off_the_list pins
    that refusal on the oracle side.
"""
import numpy as np
import pytest

import crafted_catalogue as CC
from decbitsmodel import kint_of, unfold
import slalibs as S
import slastream as SS
import waveforms as W

CASES = CC.catalogue()
IDS = [c.name for c in CASES]


def params():
    return S.make_params(cap=CC.CAP)


def synthesis_chain(oracle, case):
    """the samples a decoder must produce, from the writer's fields through the oracle's unit functions:
    LMS -> long-term -> lattice -> de-emphasis, then mid/side and the left-justification"""
    f = case.fmt
    out = np.zeros((f.num_channels, case.num_samples), np.int32)
    pos = 0
    for b in case.blocks:
        buf = np.zeros((f.num_channels, b.n), np.int32)
        if b.type == SS.RAW:
            for ch in range(f.num_channels):
                buf[ch] = unfold(b.raw[ch])
        elif b.type == SS.COMPRESS:
            for ch, c in enumerate(b.chans):
                res = unfold(c.res) if c.folded else np.asarray(c.res, np.int32)
                x = oracle.lms_synth(res, f.lms)
                if c.ltm is not None and c.ltm[0] != 0:
                    taps = (np.array([SS.fold(t) for t in c.ltm[1]], np.int64))
                    taps = ((((taps >> 1) ^ -(taps & 1)) << 16) & SS.M32).astype(np.uint32).view(np.int32)
                    x = oracle.ltm_synth(x, c.ltm[0], taps)
                x = oracle.lattice_synth(x, kint_of(c))
                buf[ch] = oracle.deemph_i32(x)
        if f.ms:
            side = buf[1].astype(np.int64)
            mid = ((buf[0].astype(np.int64) << 1) | (side & 1))
            buf[0] = ((((mid + side) & SS.M32).astype(np.uint32).view(np.int32)).astype(np.int64) >> 1).astype(np.int32)
            buf[1] = ((((mid - side) & SS.M32).astype(np.uint32).view(np.int32)).astype(np.int64) >> 1).astype(np.int32)
        sh = 32 - f.bits + f.lshift
        out[:, pos:pos + b.n] = ((buf.astype(np.int64) << sh) & SS.M32).astype(np.uint32).view(np.int32)
        pos += b.n
    return out


# ------------------------------------------------------------------ the writer against the oracle's own writer

@pytest.mark.parametrize("bits", [8, 16, 24])
@pytest.mark.parametrize("nch", [1, 2, 5])
def test_writer_body_equals_the_oracle_coder(oracle, bits, nch):
    rng = np.random.default_rng(bits * 10 + nch)
    for scale in (0, 3, 9, 15):
        res = np.round(rng.standard_normal((nch, 1500)) * 2.0 ** scale).astype(np.int32)
        want = oracle.code_residual(res, bits)
        codes = [SS.fold_array(c) for c in res]
        inits = [SS.natural_init(c) for c in codes]
        w = SS.BitWriter()
        for i in inits:
            w.put(i, bits)
        w.align()
        SS.put_residuals(w, codes, inits)
        w.align()
        assert w.tobytes() == want, scale


@pytest.mark.parametrize("nch,bits,order,ltm,lms,ms", [(2, 16, 16, 3, 8, 1), (1, 24, 32, 5, 16, 0), (3, 8, 8, 1, 4, 0)])
def test_writer_file_equals_a_traced_encode(oracle, nch, bits, order, ltm, lms, ms):
    """the oracle encoder's fields, re-written by the independent writer, give the oracle encoder's bytes"""
    pcm = W.music_like(nch, 20000, bits, seed=order)
    pcm[:, :3000] = 0                                      # leading silence: a SILENT block
    p = S.make_params(nch, bits, 48000, order, ltm, lms, ms, 1, 4096)
    ret, data, tr = oracle.encode_trace(p, pcm)
    assert ret == 0
    fmt = SS.Format(nch, bits, 48000, tr.offset_lshift, order, ltm, lms, ms, 1, 4096)
    blocks = []
    for b in range(tr.num_blocks):
        s0, n, typ = int(tr.blk_start[b]), int(tr.blk_nsmpl[b]), int(tr.blk_type[b])
        if typ != SS.COMPRESS:
            assert typ == SS.SILENT
            blocks.append(SS.Block(SS.SILENT, n))
            continue
        chans = []
        for ch in range(nch):
            pitch = int(tr.pitch[b, ch])
            lt = (pitch, [int(t) >> 16 for t in tr.ltm_coef[b, ch, :ltm]]) if pitch >= 3 else None
            chans.append(SS.Chan(int(tr.rshift[b, ch]), [int(c) for c in tr.code[b, ch, 1:]], lt, int(tr.rice_init[b, ch]),
                                 tr.res_final[ch, s0:s0 + n]))
        blocks.append(SS.Block(SS.COMPRESS, n, chans))
    assert SS.SILENT in [b.type for b in blocks] and SS.COMPRESS in [b.type for b in blocks]
    mine, _, _ = SS.write_file(fmt, blocks)
    assert mine == data


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_crafted_stream_decodes_to_the_synthesis_chain(oracle, case):
    """the oracle's decoder on a crafted stream == the oracle's own unit functions on the writer's fields"""
    rc, got, _ = oracle.decode_whole(params(), case.data, case.num_samples)
    assert rc == 0
    assert np.array_equal(got, synthesis_chain(oracle, case))


# ------------------------------------------------------------------ pinned to the reference

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_crafted_stream_matches_the_reference(oracle, ref, case):
    ro, do, _ = oracle.decode_whole(params(), case.data, case.num_samples)
    rr, dr, _ = ref.decode_whole(params(), case.data, case.num_samples)
    assert ro == rr == 0, (ro, rr)
    assert do.shape == dr.shape and np.array_equal(do, dr)


def test_lms_orders_off_the_list(oracle):
    """see the module docstring: the oracle (and so the HIP decoder, tests/test_gpu_crafted_streams.py) refuses
    header LMS orders other than 4 / 8 / 16 / 32 (below the handle's capacity) with FAILED_TO_SYNTHESIZE"""
    rng = np.random.default_rng(5)
    for lms in (1, 2, 3, 6, 12, 24):
        f = SS.Format(1, 16, order=4, ntaps=1, lms=lms)
        data, _, _ = SS.write_file(f, [CC._comp(rng, f, 3000, bits=8, full=False)])
        assert oracle.decode_whole(params(), data, 3000)[0] == 8, lms


# ------------------------------------------------------------------ what the catalogue reaches

def lattice_products_wrap(x, kint):
    """does the synthesis lattice (oracle/sla_oracle.c: slao_lattice_synth) form a k * b product outside int32 on x?"""
    order = len(kint) - 1
    k = [int(v) for v in kint]
    bwd = [0] * (order + 1)

    def wrap(v):
        v &= SS.M32
        return v - (1 << 32) if v >> 31 else v

    for e in x:
        f = int(e)
        for m in range(order, 0, -1):
            for v in (bwd[m - 1],):
                if not -(1 << 31) <= k[m] * v < (1 << 31):
                    return True
            f = wrap(f + (wrap(k[m] * bwd[m - 1] + (1 << 14)) >> 15))
            if not -(1 << 31) <= k[m] * f < (1 << 31):
                return True
            bwd[m] = wrap(bwd[m - 1] - (wrap(k[m] * f + (1 << 14)) >> 15))
        bwd[0] = f
    return False


def test_catalogue_reaches_every_target(oracle):
    """the catalogue really contains what the kernels' rare branches need (so no GPU test of it is green by not
    running them): a tile of more than 64 bits per sample, Golomb moduli that are not powers of two, gamma escapes,
    quotients 15 / 16 / 17, initial parameters whose `<< 8` wraps, a lattice whose products wrap, pitch >= 256, even
    tap counts, a 33-bit RAW field with its top bit set, 4- and 32-bit formats and a 16384-sample block"""
    st = SS.Stats()
    for c in CASES:
        st.merge(c.stats)
    assert st.max_tile_bits_per_sample > 64
    assert any(m & (m - 1) and m > 8 for ms in st.golomb_m for m in ms)
    assert st.gamma_escapes > 0 and {15, 16, 17} <= st.quotients
    assert st.max_init >= 1 << 24
    assert 33 in st.raw_widths
    side = [b.raw[1] for b in CC.by_name()["format_32bit_ms_raw_33bit_side"].blocks if b.type == SS.RAW]
    assert any((s >> np.uint64(32)).any() for s in side)
    pitches = {(c.fmt.ntaps, ch.ltm[0]) for c in CASES for b in c.blocks if b.type == SS.COMPRESS
               for ch in b.chans if ch.ltm is not None}
    assert any(p >= 256 for _, p in pitches) and {2, 4} <= {t for t, _ in pitches}
    assert {c.fmt.bits for c in CASES} >= {4, 12, 20, 32} and {c.fmt.num_channels for c in CASES} >= {1, 2, 3, 8}
    assert max(b.n for c in CASES for b in c.blocks) == 16384
    case = CC.by_name()["parcor_wrapping_products"]
    ch = case.blocks[0].chans[0]
    assert lattice_products_wrap(oracle.lms_synth(np.asarray(ch.res, np.int32), case.fmt.lms)[:256], kint_of(ch))
