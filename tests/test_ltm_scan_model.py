"""The model of the long-term stage's exact route (ltmscanmodel.py) against the oracle, without a device: both constructions
of the autocorrelation give the same doubles, the serial scan picks the oracle's pitch and reports no candidate exactly
where the oracle fails because of the scan, and the catalogue reaches every corner of the scan -- lags 256 and 257
included -- at every transform size, so that tests/test_gpu_ltm_exact.py cannot pass by never getting there."""
import ctypes as C
import os

import numpy as np
import pytest

import ltmscanmodel as M
import sla_amd
import slalibs as S

f64p, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
SIZES = (4096, 8192, 16384, 32768)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    lib = sla_amd.lib()
    lib.slai_ltm_solve.argtypes = [f64p, C.c_uint32, u32p, f64p]
    lib.slai_ltm_solve.restype = C.c_int
    return lib


def host_solve(L, rec, ntaps):
    pitch, coef = C.c_uint32(0), np.zeros(5)
    rec = np.ascontiguousarray(rec)
    ret = L.slai_ltm_solve(rec.ctypes.data_as(f64p), ntaps, C.byref(pitch), coef.ctypes.data_as(f64p))
    return ret, pitch.value, coef[:ntaps]


def test_table_rows_reach_what_they_were_built_for(oracle):
    """the eight hand-checked blocks: the oracle's result and pitch, and what the model says the scan did"""
    want = {"comb256": (0, 256, "pseudo256_chosen"), "comb257": (0, 257, "pseudo257_chosen"),
            "comb255": (4, None, "pseudo_seen_no_candidate"), "sin256": (0, 256, "open256_chosen"),
            "cos4": (0, 4, "open256_seen"), "two_impulses": (0, 40, "start_is_downward_crossing"),
            "alternating": (0, 2, "chosen_eq_2"), "single_one": (4, None, "exact_zero_in_scan")}
    for fft_size in SIZES:
        for name, x in M.table_rows(fft_size):
            ret, pitch, _, ac = oracle.ltm_analyze(x, fft_size, 1, want_autocorr=True)
            chosen, ncand, flags = M.scan(ac)
            wret, wpitch, wflag = want[name]
            assert ret == wret and wflag in flags, (fft_size, name, ret, pitch, flags)
            if ret == 0:
                assert pitch == wpitch == chosen, (fft_size, name, pitch, chosen)
            else:
                assert chosen == 0 and "no_candidate" in flags
            if name == "cos4":
                assert ncand == 64 and "open256_chosen" not in flags
            if name == "two_impulses":
                assert ncand >= 40
            if name == "single_one":
                assert M.record(ac)[0] == 2.0 and not ac[1:258].any()      # live, every lag of the scan exactly zero: code 2, not 0


@pytest.mark.parametrize("fft_size", [1024, 2048, 4096, 8192, 16384, 32768, 131072])
def test_both_constructions_agree(oracle, fft_size):
    """reference_acf's second construction (for blocks the oracle refuses) gives the oracle's doubles where both apply"""
    for name, x in M.plain_blocks(fft_size):
        ret, _, _, ac = oracle.ltm_analyze(x, fft_size, 1, want_autocorr=True)
        assert ret in (0, 4)
        assert np.array_equal(M.acf_by_fft(oracle, x, fft_size).view(np.uint64), ac.view(np.uint64)), (fft_size, name)


@pytest.mark.parametrize("fft_size", SIZES)
def test_scan_model_is_the_oracles(oracle, L, fft_size):
    """every catalogue block: the model's lag is the oracle's pitch where the oracle succeeds; where it returns 4 the model
    either has no candidate or the host solve refuses the model's record (lag too close to the origin, singular system);
    no candidate in the model always means 4.  1, 3 and 5 taps outside the sweep, 3 taps on the sweep."""
    cases = M.prepared(fft_size)
    nplain = len(M.plain_blocks(fft_size))
    scan_failures = solve_failures = 0
    for i, c in enumerate(cases):
        for ntaps in ((1, 3, 5) if i < nplain else (3,)):
            ret, pitch, coef = oracle.ltm_analyze(c.x, fft_size, ntaps)
            assert ret in (0, 4), (c.name, ret)
            hret, hpitch, hcoef = host_solve(L, c.record, ntaps)
            if "silent" in c.flags:
                assert ret == 0 and pitch == 0 and c.chosen == 0 and c.record[0] == 0.0
            elif "no_candidate" in c.flags:
                assert ret == 4 and c.chosen == 0 and c.record[0] == 2.0 and hret == 4, (c.name, ntaps, ret)
                scan_failures += 1
            elif ret == 0:
                assert c.chosen == pitch and c.record[0] == 1.0, (c.name, ntaps, c.chosen, pitch)
                assert hret == 0 and hpitch == pitch and np.array_equal(hcoef.view(np.uint64), coef.view(np.uint64)), (c.name, ntaps)
            else:
                assert hret == 4, (c.name, ntaps, c.chosen)        # the scan found a lag, the solve refused it
                solve_failures += 1
    print("fft", fft_size, "blocks", len(cases), "no candidate", scan_failures, "solve refused", solve_failures)
    assert scan_failures > 0


@pytest.mark.parametrize("fft_size", SIZES)
def test_catalogue_reaches_every_corner(fft_size):
    """a condition on the inputs, not a measurement: every flag of the scan is raised by some block (an exact tie of the two
    largest candidates among them), and at least 200 of the 256 sweep lags (2 .. 257) are the chosen lag of some sweep block"""
    cases = M.prepared(fft_size)
    counts = M.flag_counts(cases)
    print("fft", fft_size, counts)
    missing = [f for f in M.FLAGS if counts[f] == 0]
    assert not missing, missing
    nplain = len(M.plain_blocks(fft_size))
    hit = {c.chosen for c in cases[nplain:]} & set(M.SWEEP_LAGS)
    print("sweep lags chosen:", len(hit), "missing", sorted(set(M.SWEEP_LAGS) - hit))
    assert len(hit) >= 200
    assert any(c.chosen == 256 for c in cases) and any(c.chosen == 257 for c in cases)


def test_record_conventions():
    """code 0 / 1 / 2, 0.0 below index 0, the window chosen - 2 .. chosen + 2"""
    ac = np.zeros(300)
    assert M.record(ac).tolist() == [0.0] * 12                                   # silent
    ac[0] = 1.0
    assert M.record(ac).tolist() == [2.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]      # no candidate: window -2 .. 2
    ac[:6] = [4.0, -1.0, 3.0, -2.0, 1.0, -1.0]
    chosen, ncand, flags = M.scan(ac)
    # (lag 2 starts a segment and is a downward crossing itself: the segment runs on to the next one, lag 4 -- one candidate)
    assert (chosen, ncand) == (2, 1) and {"chosen_eq_2", "start_is_downward_crossing"} <= flags
    assert M.record(ac).tolist() == [1.0, 2.0, 4.0, -1.0, 3.0, -2.0, 1.0, 4.0, -1.0, 3.0, -2.0, 1.0]
