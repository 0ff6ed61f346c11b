"""The entropy-decode kernel with several blocks per wave (k_dec_bits through sla_hip_launch_dec_bits_x; run with
-m gpu on an MI355X).

The launcher gives a wave ceil(num_blocks / 1024) blocks, at most 64 // channels (sla_hip_dec_bits_lanes).  From two
blocks per wave on, the readers of one wave share fill_windows (an owner loop over shuffled window bases, stream lengths
and, in the bounded launch, ends of stream), walk to the tile count of the wave's longest block, diverge by block type,
and flush each other's LDS rows; the last workgroup has lanes without a block.  The crafted catalogue and the damage
tests never reach that shape: no crafted file has more than 16 blocks.

Here a few crafted blocks per format (tests/decbitscases.py: the 64-sample tile edge, the bit reader's far path, the
gamma boundary, Golomb moduli, int32's extremes, 33-bit RAW fields, SILENT, a 2000-sample block) are replicated into
launches of 1025 to 64513 rows -- 2, 3 and 64 // C blocks per wave, a partial last workgroup and a full one, shuffled,
with one long row among one-sample rows, with five kinds of row side by side, with SLA_HIP_DEC_HEADER_ONLY rows, with
per-row ends of stream and without, and with one file's stream cut inside a block.  Every output is compared exactly
with the writer's fields (tests/decbitsmodel.py, held against the oracle by tests/test_dec_bits_model.py), never with
another run of the kernel; all buffers start as 0x5A5A5A5A and every word no row owns must still hold that.

A row whose stream ends inside its body must report overrun and its written type, its header outputs must be right,
and it may fill its own sample range with anything.  Its samples are not compared: past the end the kernel's reader
gives up and reads zeros from then on, while the oracle's coder (oracle.decode_residual on a zero-padded body) ends each
zero run a few bytes past the end and goes on, so the two agree only up to the cut."""
import ctypes as C

import numpy as np
import pytest

import decbitscases as DC
import decbitsmodel as DM
import slastream as SS

CASES = DC.launch_cases()
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def _lanes(case):
    import os
    import sla_amd
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return int(sla_amd.lib().sla_hip_dec_bits_lanes(case.rows, case.C))


def _crcs(oracle, model, la):
    """oracle.crc16 of [8, byte_len) of every row, computed once per distinct (block, byte_len)"""
    key = la.blocks["byte_off"].astype(np.int64) * (1 << 32) + la.blocks["byte_len"]
    uniq, inv = np.unique(key, return_inverse=True)
    crc = np.zeros(len(uniq), np.uint32)
    for i, k in enumerate(uniq):
        off, blen = int(k) >> 32, int(k) & SS.M32
        crc[i] = oracle.crc16(model.image[off + 8:off + blen])
    return crc[inv]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dec_bits_with_several_blocks_per_wave(oracle, hip, case):
    import torch
    L = hip.lib()
    s, model, plan, la = DC.build(case)
    fmt = s.fmt
    Cn, rows, order = fmt.num_channels, case.rows, fmt.order
    assert L.sla_hip_dec_bits_lanes(rows, Cn) == case.lanes >= 2
    want_info = la.info.copy()
    want_info[:, 2] = _crcs(oracle, model, la)

    canary = lambda count: torch.full((count,), DM.CANARY, dtype=torch.int32, device="cuda")
    d_img = torch.from_numpy(model.image.view(np.int32).copy()).cuda()
    d_blk = torch.from_numpy(la.blocks.view(np.uint8).copy()).cuda()
    d_end = torch.from_numpy(la.ends.astype(np.int64)).cuda() if case.image == "split" else None
    d_planes, d_info = canary(Cn * la.stride), canary(rows * 4)
    d_chan, d_kint = canary(rows * Cn * DM.CHAN_WORDS), canary(rows * Cn * (order + 1))
    torch.cuda.synchronize()
    rc = L.sla_hip_launch_dec_bits_x(C.c_void_p(d_img.data_ptr()), C.c_uint64(model.image_bytes), C.c_void_p(d_blk.data_ptr()),
                                     rows, Cn, fmt.bits, fmt.lshift, fmt.ms, order, fmt.ntaps, 1,
                                     C.c_void_p(d_planes.data_ptr()), C.c_uint64(la.stride), C.c_void_p(d_info.data_ptr()),
                                     C.c_void_p(d_chan.data_ptr()), C.c_void_p(d_kint.data_ptr()), None,
                                     C.c_void_p(d_end.data_ptr()) if d_end is not None else None)
    assert rc == 0
    torch.cuda.synchronize()
    info = d_info.cpu().numpy().view(np.uint32).reshape(rows, 4)
    chan = d_chan.cpu().numpy().view(np.uint32).reshape(rows, Cn, DM.CHAN_WORDS)
    kint = d_kint.cpu().numpy().reshape(rows, Cn, order + 1)
    planes = d_planes.cpu().numpy().reshape(Cn, la.stride)

    def first_bad(ok):
        r = int(np.argmin(ok))
        return ("row", r, plan.name[r], "lane", r % case.lanes, "wave", [plan.name[i] for i in
                                                                       range(r - r % case.lanes, min(r - r % case.lanes + case.lanes, rows))][:8])

    # header outputs: type and overrun of every row, used_bytes of every row whose stream is whole, the CRC of [8, byte_len)
    for col, name in ((0, "type"), (3, "overrun"), (2, "crc")):
        ok = info[:, col] == want_info[:, col]
        assert ok.all(), (name, first_bad(ok), int(info[np.argmin(ok), col]), int(want_info[np.argmin(ok), col]))
    ok = (info[:, 1] == want_info[:, 1]) | la.cut
    assert ok.all(), ("used_bytes", first_bad(ok), int(info[np.argmin(ok), 1]), int(want_info[np.argmin(ok), 1]))
    assert la.cut.any() == case.cut and (info[la.cut, 3] == 1).all()
    comp = la.compressed
    ok = (chan == la.chan).all(axis=(1, 2)) | ~comp
    assert ok.all(), ("chan", first_bad(ok))
    ok = (kint == la.kint).all(axis=(1, 2)) | ~comp
    assert ok.all(), ("kint", first_bad(ok))
    assert (kint[comp][:, :, 0] == 0).all()

    # the planes: every row's samples, the canary in every gap, behind the last row and in the HEADER_ONLY rows' ranges
    # (the model's planes hold the canary there); a cut row's own range is free
    same = (planes == la.planes) | la.free[None, :]
    if not same.all():
        c, pos = np.argwhere(~same)[0]
        r = int(np.searchsorted(la.blocks["smp_off"], pos, side="right")) - 1
        b = la.blocks[r]
        where = "sample %d of its %d" % (pos - b["smp_off"], b["num_samples"]) if pos < int(b["smp_off"]) + int(b["num_samples"]) \
            else "the gap behind it"
        raise AssertionError(("planes", "channel", int(c), where, first_bad(np.arange(rows) != r),
                              int(planes[c, pos]), int(la.planes[c, pos]), "mismatches", int((~same).sum())))
    honly = (la.blocks["flags"] & DM.HEADER_ONLY) != 0
    assert (info[honly, 1] < la.blocks["byte_len"][honly]).all()         # they stopped behind the header


@pytest.mark.parametrize("C_", sorted(DC.FORMATS))
def test_every_wave_shape_is_exercised(C_):
    """from the row plans and the library's lane count: some wave of some launch of every format held two block types
    (and RAW, SILENT, Golomb, adaptive and HEADER_ONLY rows together), a far-path row beside a one-sample row, a long
    row alone among one-sample rows, a cut row beside an intact one, and a lane below `lanes` without a block"""
    seen = set()
    for case in (c for c in CASES if c.C == C_):
        lanes = _lanes(case)
        assert lanes == case.lanes >= 2
        s, model, plan, la = DC.build(case)
        types = la.info[:, 0]
        n = la.blocks["num_samples"]
        honly = (la.blocks["flags"] & DM.HEADER_ONLY) != 0
        golomb = np.array([k.startswith("golomb") for k, _ in plan.name])
        far = np.array([k == "far" for k, _ in plan.name])
        if case.rows % lanes:
            seen.add("not mine")
        if case.image == "single":
            seen.add("no ends")
        elif len(np.unique(la.ends)) >= 3:
            seen.add("ends of three files")
        for w0 in range(0, case.rows, lanes):
            w = slice(w0, min(w0 + lanes, case.rows))
            live = ~honly[w]
            if len(np.unique(types[w][live])) >= 2:
                seen.add("two types")
            if {0, 1, 2} <= set(types[w][live]) and golomb[w].any() and (~golomb[w] & (types[w] == 0) & live).any() and honly[w].any():
                seen.add("five kinds")
            if (far[w] & live).any() and (n[w][live] == 1).any():
                seen.add("far beside one sample")
            if lanes >= 3 and (n[w][live] > 128).sum() == 1 and (n[w][live] == 1).sum() == (w.stop - w.start) - 1:
                seen.add("dominated")
            if la.cut[w].any() and (~la.cut[w]).any():
                seen.add("cut beside intact")
    assert seen == {"not mine", "no ends", "ends of three files", "two types", "five kinds", "far beside one sample",
                    "dominated", "cut beside intact"}
