"""CPU tests of tests/acfmodel.py, the device-free reference of tests/test_gpu_acf_error.py, and of the two budgets the
certificates rest on:

  * staged() is, bit for bit, what the oracle stages (scaling, mid/side, window, pre-emphasis);
  * exact_lag_sums() is the correctly rounded sum Python's integers and fractions give, on 32-bit full-scale material and
    on the tiny values at a sine window's edges, and its P_t / X_t split is the one test_gpu_acf_lags.py defines;
  * the roundings the reference's chain and k_acf_blocks take together fit k_blocks_finish's delta for every block length
    and lag, and those of the tile sums and their assembly fit the search certificate's constant;
  * the oracle's own serial sums lie within roundings_reference of the exact sums;
  * the checker rejects a sum that lost one product at a tile edge, or whose 256-sample boundary moved by one sample.

What the budgets showed when they were first counted (nothing had checked them before): the block stage's n + 64 is short
at lag 0 from n = 3585 on -- the reference's energy sum alone takes n roundings, k_acf_blocks 4 ceil(n / 256) + 6 -- and the
search's 48 left the chain of X out, short at 36, 49 and 52 live lags.  Both constants were raised to what the counts
require (kernels/blocks.inc acf_blocks_budget, kernels/search.inc SEARCH_ACF_ROUNDINGS).
"""
import ctypes as C
import os
import re
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

import acfmodel as A
import slalibs as S
import sla_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def oracle():
    return S.oracle()


G = namedtuple("G", "pcm_off num_samples channel int_shift")


# ------------------------------------------------------------------ staged()

@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("ms", [0, 1])
def test_staged_is_what_the_oracle_stages(oracle, ms, bits):
    n, off = 777, 5
    pcm = A.material("uniform", bits, n + 40, seed=3)
    pcm[:, off] = [-2 ** 31, 2 ** 31 - (1 << (32 - bits))]        # the widest sum and difference
    l, r = pcm[0, off:off + n] * 2.0 ** -31, pcm[1, off:off + n] * 2.0 ** -31
    for ch in (0, 1):
        plain = ((l + r) / 2 if ch == 0 else l - r) if ms else (l, r)[ch]          # oracle/sla_oracle.c stage_input
        g = G(off, n, ch, 32 - bits)
        assert np.array_equal(A.staged(pcm, g, None, ms).view(np.uint64), plain.view(np.uint64))
        for w in (np.ones(n), oracle.window(1, n)):
            want = oracle.preemph_f64(plain * w)
            assert np.array_equal(A.staged(pcm, g, w, ms).view(np.uint64), want.view(np.uint64)), (ms, bits, ch)


# ------------------------------------------------------------------ exact_lag_sums()

def _fraction_sums(x, order, tile):
    """the same sums in exact rational arithmetic, rounded once (float(Fraction) rounds correctly)"""
    f = [Fraction(float(v)) for v in x]
    n = len(f)
    nt = (n + tile - 1) // tile
    r = np.zeros(order + 1)
    P, X = np.zeros((nt, order + 1)), np.zeros((nt, order + 1))
    for lag in range(min(order, n - 1) + 1):
        prod = [f[m] * f[m + lag] for m in range(n - lag)]
        r[lag] = float(sum(prod, Fraction(0)))
        for t in range(nt):
            t0, t1 = t * tile, min((t + 1) * tile, n)
            h = min(t1, n - lag)
            P[t, lag] = float(sum(prod[t0:h], Fraction(0)))
            X[t, lag] = float(sum(prod[max(t0, t1 - lag):h], Fraction(0)))
    return r, P, X


def _pin_windows(oracle):
    full = A.material("uniform", 32, 400, seed=5)
    full[0, :8] = [-2 ** 31, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1]
    yield "32-bit full scale, plain", A.staged(full, G(0, 300, 0, 0), None, 0)
    yield "32-bit full scale, side", A.staged(full, G(3, 300, 1, 0), None, 1)
    w = oracle.window(1, 16384)
    dc = A.material("dc", 32, 16384)
    x = A.staged(dc, G(0, 16384, 0, 0), w, 0)
    yield "sine window, front edge", x[:300]
    yield "sine window, back edge", x[-300:]
    yield "sine window of 257 samples, mid", A.staged(full, G(1, 257, 0, 0), oracle.window(1, 257), 1)
    nyq = A.material("nyquist", 24, 300)
    yield "cancelling lags", A.staged(nyq, G(0, 300, 1, 8), None, 0)


def test_exact_lag_sums_are_the_rounded_rational_sums(oracle):
    for name, x in _pin_windows(oracle):
        got = A.exact_lag_sums(x, 51, tile=64)
        r, P, X = _fraction_sums(x, 51, 64)
        for a, b, what in ((got.r, r, "r"), (got.P, P, "P"), (got.X, X, "X")):
            assert np.array_equal((a + 0.0).view(np.uint64), (b + 0.0).view(np.uint64)), (name, what)
        assert np.all(got.S >= np.abs(got.r) * (1 - 1e-12)) and np.all(got.SX <= got.SP * (1 + 1e-12))
    x = A.staged(A.material("nyquist", 24, 301), G(0, 301, 1, 8), None, 0)
    assert np.all(A.exact_lag_sums(x, 7).r[1::2] == 0.0)          # +, +, -, -: an even number of products at an odd lag cancels completely


def test_a_subrange_is_the_window_cut_out(oracle):
    x = A.staged(A.material("coloured", 32, 700), G(0, 700, 0, 0), None, 0)
    a, b = A.exact_lag_sums(x, 20, 133, 650, tile=128), A.exact_lag_sums(x[133:650], 20, tile=128)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_the_split_is_the_one_the_tile_test_defines():
    """16-bit material: every sum is an integer below 2^53 / scale, so the integer sums of test_gpu_acf_lags._expected_tiles are
    the exact ones"""
    from test_gpu_acf_lags import _expected_tiles
    q = np.random.default_rng(11).integers(-32768, 32768, 2500, dtype=np.int64)
    for order in (15, 51):
        P, X = _expected_tiles(q, order, 2.0 ** -30)
        got = A.exact_lag_sums(q.astype(np.float64) * 2.0 ** -15, order)
        assert np.array_equal(got.P, P) and np.array_equal(got.X, X)
        assert np.array_equal(got.r, (P.sum(axis=0) - X[-1]))        # (exact: integers)


def test_two_prod_is_error_free():
    rng = np.random.default_rng(2)
    a = np.concatenate([rng.standard_normal(500), [2.0 - 2.0 ** -52, 2.0 ** -45 * 3, -(2.0 - 2.0 ** -31)]])
    b = np.concatenate([rng.standard_normal(500) * 1e-9, [2.0 - 2.0 ** -52, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -31]])
    p, e = A.two_prod(a, b)
    for x, y, pp, ee in zip(a, b, p, e):
        assert Fraction(float(x)) * Fraction(float(y)) == Fraction(float(pp)) + Fraction(float(ee))


# ------------------------------------------------------------------ the counts and the budgets

def test_counts_at_the_sizes_the_comments_name():
    assert [A.roundings_blocks(n) for n in (1, 256, 257, 4096, 16384)] == [10, 10, 14, 70, 262]
    assert A.roundings_tile(52, 52, 51, "P") == 22 and A.roundings_tile(12, 12, 11, "P") == 26
    assert A.roundings_tile(20, 17, 16, "X") == 6 and A.roundings_tile(36, 33, 32, "X") == 17 and A.roundings_tile(52, 49, 48, "X") == 48
    assert A.roundings_search(16) == 16
    assert A.roundings_reference(16384, 0) == 16384 and A.roundings_reference(5, 7) == 0
    # the chain of slao_autocorr, term by term: n = 10, lag = 2 -> groups = 2, 4 pair terms, leftovers 10 - 8 - 2 = 0
    assert A.chain_terms(10, 2) == (4, 0) and A.roundings_reference(10, 2) == 5
    assert A.chain_terms(10, 4) == (0, 6) and A.roundings_reference(10, 4) == 6
    assert [A.instantiation(o) for o in (8, 16, 18, 32, 31, 48, 51, 52)] == [(12, 12), (20, 17), (20, 20), (36, 33), (36, 36), (52, 49), (52, 52), None]


def test_chain_terms_cover_every_pair_once():
    for n in (1, 2, 7, 100, 153, 154, 1000):
        for lag in range(1, 52):
            pairs, left = A.chain_terms(n, lag)
            assert 2 * pairs + left == max(n - lag, 0), (n, lag)


def test_block_budget_covers_both_sums():
    """for every block length and lag: roundings of the reference's chain + roundings of k_acf_blocks <= what delta allows"""
    worst = 0
    for n in range(1, 16385):
        own, allowed = A.roundings_blocks(n), A.budget_blocks(n)
        for lag in range(52):
            need = A.roundings_reference(n, lag) + own
            assert need <= allowed, (n, lag, need, allowed)
            assert lag == 0 or 2 * (need - own) <= n + 2 * lag      # the chain of a lag >= 1: at most n / 2 + lag
            worst = max(worst, need - n)
    assert worst == 262                                            # lag 0 of the longest block: equality there


def test_n_plus_64_was_short_only_at_lag_0_of_long_blocks():
    """the constant delta used to carry: enough at every lag >= 1 and every n, at lag 0 exactly up to n = 3584"""
    for n in range(1, 16385):
        own = A.roundings_blocks(n)
        assert all(A.roundings_reference(n, lag) + own <= n + 64 for lag in range(1, 52)), n
        assert (A.roundings_reference(n, 0) + own <= n + 64) == (n <= 3584), n
        assert A.budget_blocks(n) == (n + 64 if n <= 3584 else n + own)


def test_the_kernels_carry_the_budgets():
    blocks = open(os.path.join(ROOT, "sla_amd", "csrc", "kernels", "blocks.inc")).read()
    assert re.search(r"own = 4u \* \(\(n \+ 255u\) / 256u\) \+ 6u;\s*return \(double\)n \+ \(double\)\(\(own > 64u\) \? own : 64u\);", blocks)
    assert "acf_blocks_budget(g.num_samples) * u * r[0]" in blocks
    search = open(os.path.join(ROOT, "sla_amd", "csrc", "kernels", "search.inc")).read()
    assert re.search(r"#define SEARCH_ACF_ROUNDINGS %d\.0\b" % A.SEARCH_BUDGET, search)
    assert search.count("(SEARCH_ACF_ROUNDINGS * u) *") == 2       # k_search_finish and k_search_cert


def test_search_budget_covers_the_tile_sums():
    """up to 16 tiles, every kernel of the search stage, every lag it serves: tile sum + assembly (+ half the chain of X, whose
    pairs carry at most half the window's energy) <= the certificate's constant; the 48 it used to be held up to 33 live lags"""
    worst = {}
    for order in range(1, 52):
        lags, top = A.instantiation(order)
        for nt in range(1, 17):
            for lag in range(order + 1):
                need = A.roundings_window(lags, top, lag, nt)
                assert need <= A.SEARCH_BUDGET, (order, nt, lag, need)
                worst[lags, top] = max(worst.get((lags, top), 0), need)
                # without X (a candidate that ends with its window: X is exactly 0) the old constant was enough
                assert A.roundings_tile(lags, top, lag, "P") + A.roundings_search(nt) <= 48
    assert worst == {(12, 12): 48, (20, 17): 41, (20, 20): 48, (36, 33): 47, (36, 36): 56, (52, 49): 62, (52, 52): 64}


# ------------------------------------------------------------------ the oracle's sums, and the checker

@pytest.fixture(scope="module")
def layout(oracle):
    lengths = (1, 3, 4, 5, 255, 256, 257, 1000, 4096)
    return A.block_layout({n: oracle.window(1, n) for n in lengths}, lengths)


def test_layout_starts_unaligned(layout):
    pcm, pool, cases = layout
    assert all(c.win_off % 2 == 1 for c in cases)
    assert sum(c.pcm_off % 4 == 3 for c in cases) >= len(cases) // 8 and sum(c.pcm_off % 2 == 1 for c in cases) >= len(cases) // 4
    assert {(c.kind, c.bits) for c in cases} == set(A.BLOCK_MATERIAL) and {c.window for c in cases} == {"rect", "sine"}
    for c in cases:                                                 # loud samples in front of and behind every block
        assert c.pcm_off >= 13 and c.pcm_off + c.num_samples + 32 <= pcm.shape[1]
        assert np.all(pcm[:, c.pcm_off - 4:c.pcm_off] != 0) or c.kind in ("uniform", "coloured")
        assert len(pool) >= c.win_off + c.num_samples


def test_oracle_sums_lie_within_their_count(oracle, layout):
    """slao_autocorr (the reference's chain order) against the exact sums: within roundings_reference * 2^-53 * S_lag on every
    material, window and length (16384 on one material: the count grows with n, the material does not matter to it)"""
    pcm, pool, cases = layout
    seen = 0
    for ms in (0, 1):
        for c in cases:
            x = A.staged(pcm, c, pool[c.win_off:c.win_off + c.num_samples], ms)
            ex = A.exact_lag_sums(x, 51, tiles=False)
            got = np.zeros(52)
            got[:min(52, c.num_samples)] = oracle.autocorr(x, 52)[:min(52, c.num_samples)]
            count = [A.roundings_reference(c.num_samples, lag) for lag in range(52)]
            ok = A.within(got, ex.r, ex.S, count)
            assert ok.all(), (ms, c, np.nonzero(~ok)[0])
            seen += int((got != ex.r).sum())
    assert seen > 1000                                              # (the material is in the rounded regime)
    x = A.staged(A.material("uniform", 32, 16400), G(3, 16384, 0, 0), oracle.window(1, 16384), 0)
    ex = A.exact_lag_sums(x, 51, tiles=False)
    assert A.within(oracle.autocorr(x, 52), ex.r, ex.S, [A.roundings_reference(16384, lag) for lag in range(52)]).all()


def test_checker_rejects_a_dropped_pair_and_a_shifted_boundary(oracle):
    """negative control: the exact sums of one block, minus ONE product at a 256-sample edge, and the sums of a block whose
    first tile took one sample more (x[256] doubled in, x[255]'s neighbour lost), both judged as the GPU test judges k_acf_blocks"""
    n = 4096
    pcm = A.material("coloured", 24, n + 16)
    x = A.staged(pcm, G(7, n, 0, 8), oracle.window(1, n), 0)
    ex = A.exact_lag_sums(x, 51, tiles=False)
    count = A.roundings_blocks(n)
    assert A.within(ex.r, ex.r, ex.S, count).all()
    assert A.within(oracle.autocorr(x, 52), ex.r, ex.S, [A.roundings_reference(n, lag) + 0 for lag in range(52)]).all()
    for lag in (1, 2, 51):
        dropped = ex.r.copy()
        dropped[lag] -= x[256] * x[256 - lag]                      # the pair that straddles the first tile edge
        ok = A.within(dropped, ex.r, ex.S, count)
        assert not ok[lag] and ok.sum() == 51
        assert A.ratio(dropped, ex.r, ex.S)[lag] > 1e6 * count
    y = x.copy()
    y[255] = x[256]                                                 # one sample across the boundary
    moved = A.exact_lag_sums(y, 51, tiles=False).r
    assert not A.within(moved, ex.r, ex.S, count)[:8].any()
    # and in the tile split of the search stage: P of the first tile without its last straddling pair
    sx = A.staged(pcm, G(7, 2049, 0, 8), None, 0)
    st = A.exact_lag_sums(sx, 51)
    lags, top = A.instantiation(51)
    P = st.P.copy()
    P[0, 1] -= sx[1023] * sx[1024]
    ok = A.within(P, st.P, st.SP, A.roundings_tile(lags, top, 0, "P"))
    assert not ok[0, 1] and ok.sum() == ok.size - 1


# ------------------------------------------------------------------ the launcher that shows r[] of the block stage

@pytest.fixture(scope="module")
def L():
    if not os.path.exists(sla_amd.LIB_PATH):
        sla_amd.build()
    return sla_amd.lib()


def test_acf_blocks_launcher_is_declared_and_refuses_before_any_device_work(L):
    text = open(os.path.join(ROOT, "include", "sla_hip.h")).read()
    assert re.search(r"\bsla_hip_launch_acf_blocks\s*\(", text)
    assert "sla_hip_launch_acf_blocks" in sla_amd.EXPORTED_SYMBOLS and hasattr(L, "sla_hip_launch_acf_blocks")
    # dangling values: nothing behind them is touched when an argument is refused
    pcm, groups, pool, out, rs = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))

    def launch(pcm=pcm, order=16, groups=groups, ng=4, pool=pool, out=out, rs=rs):
        return L.sla_hip_launch_acf_blocks(pcm, 100000, 0, order, groups, ng, pool, out, rs, None)

    for name in ("pcm", "groups", "pool", "out", "rs"):
        assert launch(**{name: None}) == 2, name                    # SLA_APIRESULT_INVALID_ARGUMENT
    assert launch(order=0) == 2
    assert [launch(order=o) for o in (52, 53, 64, 255)] == [3] * 4   # SLA_APIRESULT_EXCEED_HANDLE_CAPACITY
    assert launch(ng=0) == 0
