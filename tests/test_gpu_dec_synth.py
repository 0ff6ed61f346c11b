"""k_dec_lms<ORDER> and k_dec_lattice<G, R> alone, many jobs per wave, through sla_hip_launch_dec_lms and
sla_hip_launch_dec_lattice; k_dec_deemphasis and k_dec_finish through their launchers (run with -m gpu on an MI355X).

The two synthesis kernels give a (block, channel) job G lanes of a wave (G = 2 * ORDER for the LMS; 16, 32 or 64 for the
lattice), sum and shift across lanes with DPP, and run every group of a wave as long as its longest job.  The tables of
tests/synthcases.py put jobs of different lengths, operand families (tailmodel.FAMILIES: full-range, the ends of int32,
alternating, tiny, 24-bit, a steep ramp), coefficient kinds (random Q15, alternating -32768 / 32767, full-range int32) and
rows that must be skipped (SILENT, RAW, not a type, HEADER_ONLY, no samples -- all holding live samples and coefficients)
side by side in the waves, at 1, 3 and 8 channels, with a job count that ends inside a workgroup and, where the channel
count allows, inside a wave:
  LMS      orders 4, 8, 16, 32; every family at n = 0, 1, order - 1, order, order + 1, G - 1, G, G + 1, 2 G - 1, 2 G, 2 G + 1,
           3 G + order + 1, 777;
  lattice  orders 0, 1, 15, 16, 17, 32, 33, 64, 65, 128, 129, 255 (either side of every specialisation's limit), with and
           without the fused de-emphasis; n = 0, 1, 15, 16, 17, G - 1, G, G + 1, 2 G + 5, 300.
One launch per table; the whole plane array -- samples, the canary words behind every block and at the planes' end -- must
equal the oracle's (lms_synth; lattice_synth, then deemph_i32; per job, never another kernel run), and the block, info and
kint tables must come back unchanged.  tests/test_synth_cases_model.py checks on the CPU that the tables are what this
says and that the oracle's two functions equal the reference's on these operands.
"""
import ctypes as C

import numpy as np
import pytest

import synthcases as SC
import tailmodel as TM

CANARY = SC.CANARY
GUARD = 67                         # canary words around a de-emphasis buffer and behind every finished plane


@pytest.fixture(scope="module")
def hip():
    import torch
    torch.cuda.init()
    import sla_amd
    sla_amd.lib()
    return sla_amd


def launch(hip, t):
    import torch
    L = hip.lib()
    d_planes = torch.from_numpy(t.planes.copy()).cuda()
    d_blk = torch.from_numpy(t.blocks.view(np.uint8).copy()).cuda()
    d_info = torch.from_numpy(t.info.view(np.int32).copy()).cuda()
    d_kint = torch.from_numpy(t.kint.copy()).cuda() if t.kint is not None else None
    torch.cuda.synchronize()
    if t.stage == "lms":
        rc = L.sla_hip_launch_dec_lms(C.c_void_p(d_planes.data_ptr()), C.c_uint64(t.stride), C.c_void_p(d_blk.data_ptr()),
                                      C.c_void_p(d_info.data_ptr()), C.c_uint32(len(t.blocks)), C.c_uint32(t.C),
                                      C.c_uint32(t.order), None)
    else:
        rc = L.sla_hip_launch_dec_lattice(C.c_void_p(d_planes.data_ptr()), C.c_uint64(t.stride), C.c_void_p(d_blk.data_ptr()),
                                          C.c_void_p(d_info.data_ptr()), C.c_uint32(len(t.blocks)), C.c_uint32(t.C),
                                          C.c_void_p(d_kint.data_ptr()), C.c_uint32(t.order), C.c_uint32(t.deemphasis), None)
    assert rc == 0, (t.name, rc)
    torch.cuda.synchronize()
    # the tables came through untouched
    assert np.array_equal(d_blk.cpu().numpy(), t.blocks.view(np.uint8)), t.name
    assert np.array_equal(d_info.cpu().numpy().view(np.uint32), t.info), t.name
    if d_kint is not None:
        assert np.array_equal(d_kint.cpu().numpy(), t.kint), t.name
    return d_planes.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("order,nch", SC.LMS_TABLES, ids=[SC.lms_name(*a) for a in SC.LMS_TABLES])
def test_lms_table(hip, order, nch):
    t = SC.lms_table(order, nch)
    assert (t.want != t.planes).any() and len(t.jobs) > 4 * t.jpw
    got = launch(hip, t)
    assert np.array_equal(got, t.want), SC.explain(t, got)


@pytest.mark.gpu
@pytest.mark.parametrize("order,deemphasis,nch", SC.LATTICE_TABLES, ids=[SC.lattice_name(*a) for a in SC.LATTICE_TABLES])
def test_lattice_table(hip, order, deemphasis, nch):
    t = SC.lattice_table(order, deemphasis, nch)
    assert (t.want != t.planes).any() == bool(order or deemphasis) and len(t.jobs) > 4 * t.jpw
    got = launch(hip, t)
    assert np.array_equal(got, t.want), SC.explain(t, got)


@pytest.mark.gpu
def test_deemphasis_kernel(hip):
    """sla_hip_launch_dec_deemphasis at the ends of its shift range and of `previous`: every case has a stretch of one
    buffer to itself, canary words on both sides; expected is the plain-integer model"""
    import torch
    L = hip.lib()
    cases = [(shift, prev, fam, n) for shift in (1, 5, 16, 30) for prev in (0, -1, TM.INT32_MIN, TM.INT32_MAX)
             for fam in ("full", "allmin", "alt", "small") for n in (1, 2, 301)]
    total = sum(GUARD + n for _, _, _, n in cases) + GUARD
    buf = np.full(total, CANARY, np.int32)
    want = buf.copy()
    at, pos = [], GUARD
    for shift, prev, fam, n in cases:
        x = TM.family(fam, n, seed=shift)
        buf[pos:pos + n] = x
        want[pos:pos + n] = SC.deemphasis(x, prev, shift)
        at.append(pos)
        pos += n + GUARD
    assert pos == total and 2 * (want != buf).sum() > sum(n for _, _, _, n in cases)
    d = torch.from_numpy(buf.copy()).cuda()
    torch.cuda.synchronize()
    for (shift, prev, fam, n), p in zip(cases, at):
        rc = L.sla_hip_launch_dec_deemphasis(C.c_void_p(d.data_ptr() + 4 * p), C.c_uint32(n), C.c_int32(prev), C.c_uint32(shift), None)
        assert rc == 0, (shift, prev, fam, n, rc)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    for (shift, prev, fam, n), p in zip(cases, at):
        a, b = p - GUARD, p + n + GUARD
        if not np.array_equal(got[a:b], want[a:b]):
            i = int(np.argmax(got[a:b] != want[a:b])) - GUARD
            raise AssertionError(("shift", shift, "previous", prev, "family", fam, "n", n, "sample", i,
                                  "got", int(got[p + i]), "want", int(want[p + i])))
    assert np.array_equal(got, want)


FINISH_LAYOUTS = ((1, 0), (2, 0), (2, 1), (8, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("nch,mid_side", FINISH_LAYOUTS, ids=["c%d_ms%d" % a for a in FINISH_LAYOUTS])
def test_finish_kernel(hip, nch, mid_side):
    """sla_hip_launch_dec_finish on full-range planes: mid/side to left/right with the side's low bit as the mid's,
    wrapping sums, the left shift up to 31; n around the workgroup size, the words at and past n of every plane untouched"""
    import torch
    L = hip.lib()
    cases = [(shift, n, fam) for shift in (0, 8, 16, 31) for n in (1, 255, 256, 257, 1000) for fam in ("full", "minmax")]
    ins, wants = [], []
    for shift, n, fam in cases:
        p = np.full((nch, n + GUARD), CANARY, np.int32)
        for ch in range(nch):
            p[ch, :n] = TM.family(fam, n, seed=100 * shift + ch)
        w = p.copy()
        w[:, :n] = SC.finish(p[:, :n], mid_side, shift)
        ins.append(p)
        wants.append(w)
    flat = np.concatenate([p.ravel() for p in ins] + [np.full(GUARD, CANARY, np.int32)])
    d = torch.from_numpy(flat.copy()).cuda()
    torch.cuda.synchronize()
    pos = 0
    for (shift, n, fam), p in zip(cases, ins):
        rc = L.sla_hip_launch_dec_finish(C.c_void_p(d.data_ptr() + 4 * pos), C.c_uint64(n + GUARD), C.c_uint32(nch), C.c_uint32(n),
                                         C.c_uint32(mid_side), C.c_uint32(shift), None)
        assert rc == 0, (shift, n, fam, rc)
        pos += p.size
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    pos = 0
    for (shift, n, fam), p, w in zip(cases, ins, wants):
        g = got[pos:pos + p.size].reshape(p.shape)
        if not np.array_equal(g, w):
            ch, i = (int(v) for v in np.argwhere(g != w)[0])
            raise AssertionError(("channels", nch, "mid_side", mid_side, "shift", shift, "n", n, "family", fam, "channel", ch,
                                  "sample %d" % i if i < n else "word %d past n" % (i - n), "got", int(g[ch, i]), "want", int(w[ch, i])))
        pos += p.size
    assert (got[pos:] == CANARY).all()
