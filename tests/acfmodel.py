"""Device-free model of the autocorrelation sums behind the two certificates (kernels/search.inc, kernels/blocks.inc):

  * staged()          -- the doubles the kernels multiply, operation for operation (pinned to the oracle's staging);
  * exact_lag_sums()  -- the CORRECTLY ROUNDED sums of their products (error-free products, math.fsum), the sums of the
                         products' magnitudes S_lag, and the tile-wise P_t / X_t split of the search stage;
  * roundings_*()     -- how many roundings per lag each summation order takes, derived from the code (never from measurements);
  * budget_*()        -- the number of roundings the certificates' constants allow (what the kernels multiply 2^-53 with);
  * within()          -- the one checker of "sum is within `count` roundings of the exact sum" (GPU tests, oracle, negative control).

Error model (first order in u = 2^-53, the 1e-6 in within() pays for the higher orders): a sum of products that reaches its
value through a tree of roundings, where every product passes through at most `count` of them, differs from the exact sum by at
most count * u * S, S = sum |product|.  A rounding here is one rounded operation on the way of a product: its multiplication
(fused into the first addition or not), the addition a + b in a term c * (a + b), and every addition of a partial sum.
"""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -53
XTILE = 1024                    # SLA_HIP_XTILE: tile of the search stage
BTILE = 256                     # ACF_TILE: tile of acf_tile_fma (k_acf_blocks, sub-tile of k_acf_tiles_lds)
EMPH = 0.96875                  # 31 / 32


# ------------------------------------------------------------------ what the kernels multiply

def staged(pcm, group, window, ms):
    """The doubles of one analysis window.  pcm: int32 planes [channels][samples]; group: anything with pcm_off, num_samples
    and channel (sla_hip_lpc_group); window: None (the search stage: no window, no pre-emphasis) or the num_samples window
    values (block stage); ms: mid/side of planes 0 and 1 (channel 0 = mid, 1 = side).
      un-windowed  x = s * 2^-31; mid = (l + r) * 2^-32, side = (l - r) * 2^-31 (mid_f64 / side_f64: every step exact)
      windowed     y[s] = x[s] * w[s],  x[s] = y[s] - y[s-1] * 0.96875,  y[-1] = 0   (two roundings after the product)"""
    lo, n, ch = int(group.pcm_off), int(group.num_samples), int(group.channel)
    p = np.asarray(pcm)
    if ms:
        a, b = p[0, lo:lo + n].astype(np.float64), p[1, lo:lo + n].astype(np.float64)
        x = (a + b) * 2.0 ** -32 if ch == 0 else (a - b) * 2.0 ** -31
    else:
        x = p[ch, lo:lo + n].astype(np.float64) * 2.0 ** -31
    if window is None:
        return x
    y = x * np.asarray(window, np.float64)[:n]
    prev = np.concatenate(([0.0], y[:-1]))
    return y - prev * EMPH


def int_samples(pcm, group, ms):
    """the integer samples whose widest decides the quantiser's shift (right-justified by int_shift; mid = (L + R) >> 1, side = L - R)"""
    lo, n, ch, sh = int(group.pcm_off), int(group.num_samples), int(group.channel), int(group.int_shift)
    p = np.asarray(pcm).astype(np.int64)
    if not ms:
        return p[ch, lo:lo + n] >> sh
    li, ri = p[0, lo:lo + n] >> sh, p[1, lo:lo + n] >> sh
    wrap = lambda v: ((v + 2 ** 31) % 2 ** 32) - 2 ** 31
    return (wrap(li + ri) >> 1) if ch == 0 else wrap(li - ri)


# ------------------------------------------------------------------ exact sums

_SPLIT = 134217729.0            # 2^27 + 1


def two_prod(a, b):
    """a * b = p + e exactly (Veltkamp split, Dekker product; no overflow or underflow at the magnitudes of audio samples)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p = a * b
    t = a * _SPLIT
    ah = t - (t - a)
    al = a - ah
    t = b * _SPLIT
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _fsum(p, e, lo, hi):
    if hi <= lo:
        return 0.0
    return math.fsum(p[lo:hi].tolist() + e[lo:hi].tolist())


LagSums = namedtuple("LagSums", "r S P X SP SX")


def exact_lag_sums(x, order, lo=0, hi=None, tiles=True, tile=XTILE):
    """The window x[lo:hi], lags 0 .. order (a lag that no pair has: 0).  Returns
      r[lag]      the correctly rounded sum of x[m] x[m - lag] over the pairs inside the window
      S[lag]      sum |x[m] x[m - lag]| (a double sum of doubles: good to 1e-12, it only scales tolerances)
      P[t][lag]   the same for the pairs whose FIRST sample lies in tile t (1024 samples from lo on), correctly rounded
      X[t][lag]   the ones among them whose second sample lies beyond the tile
      SP, SX      their sums of magnitudes
    (tiles = False: r and S only; tile: another tile length, for pinning the split on short windows.)  Products are split error-free into two doubles and math.fsum adds both halves: every
    value is the double nearest to the real sum."""
    x = np.asarray(x, np.float64)
    hi = len(x) if hi is None else hi
    w = x[lo:hi]
    n = len(w)
    nt = (n + tile - 1) // tile if tiles else 0
    r, S = np.zeros(order + 1), np.zeros(order + 1)
    P, X, SP, SX = (np.zeros((nt, order + 1)) for _ in range(4))
    for lag in range(min(order, n - 1) + 1):
        p, e = two_prod(w[:n - lag], w[lag:])                    # indexed by the pair's first sample
        ap = np.abs(p)
        r[lag] = _fsum(p, e, 0, n - lag)
        S[lag] = ap.sum()
        for t in range(nt):
            t0, t1 = t * tile, min((t + 1) * tile, n)
            h = min(t1, n - lag)
            P[t, lag] = _fsum(p, e, t0, h)
            SP[t, lag] = ap[t0:h].sum() if h > t0 else 0.0
            l = max(t0, t1 - lag)
            X[t, lag] = _fsum(p, e, l, h)
            SX[t, lag] = ap[l:h].sum() if h > l else 0.0
    return LagSums(r, S, P, X, SP, SX)


def within(got, exact, S, count):
    """|got - exact| <= count * 2^-53 * S * (1 + 1e-6) + ulp(exact), element by element (a boolean array)"""
    got, exact, S = np.asarray(got, np.float64), np.asarray(exact, np.float64), np.asarray(S, np.float64)
    tol = np.asarray(count, np.float64) * U * S * (1.0 + 1e-6) + np.spacing(np.abs(exact))
    return np.abs(got - exact) <= tol


def ratio(got, exact, S):
    """the error in units of 2^-53 * S (0 where S is 0 and the sum is right): what the written record keeps"""
    got, exact, S = np.asarray(got, np.float64), np.asarray(exact, np.float64), np.asarray(S, np.float64)
    err = np.abs(got - exact)
    return np.where(S > 0.0, err / (U * np.where(S > 0.0, S, 1.0)), np.where(err > 0.0, np.inf, 0.0))


# ------------------------------------------------------------------ which kernel serves an order

def instantiation(order):
    """(LAGS, TOP) of the kernels the launchers pick for `order` (launch_acf_blocks and sla_hip_launch_search_exact_x in
    kernels/launchers.inc): lag blocks of four, 12 / 20 / 36 / 52 lags; the orders 16 / 32 / 48 keep order + 1 live lags"""
    nb = (order + 1 + 3) // 4
    lags = 12 if nb <= 3 else 20 if nb <= 5 else 36 if nb <= 9 else 52 if nb <= 13 else 0
    if lags == 0 or order < 1:
        return None
    return lags, (order + 1 if order in (16, 32, 48) else lags)


# ------------------------------------------------------------------ roundings per lag, read off the code

def roundings_blocks(N):
    """k_acf_blocks (kernels/search.inc, the kernel's loop `for (s0 = 0; s0 < N; s0 += ACF_TILE)` and acf_tile_fma above it).
      * acc[] is zeroed once in front of the loop over the 256-sample tiles and lives in registers across ALL tiles;
      * acf_tile_fma adds, per tile and live lag, the lane's four own samples: `for q in 0..3: acc[lag] = fma(own[q], P[..], acc[lag])`
        -- four dependent FMAs, one rounding each (the first one, onto +0.0, rounds the product): a lane's chain is
        4 * ceil(N / 256) roundings long; the 64 lanes' chains are independent, their |products| add up to S_lag;
      * acf_reduce_store -> wave_transpose_sum runs ONCE behind the loop: six transpose_steps, every value passes through one
        addition per step (also in the pieces of 32 / 16 / 4 / 1 values): 6 more, each on partial sums whose magnitudes add up to <= S_lag.
    4 * ceil(N / 256) + 6: 10 for a block of one tile, 70 at N = 4096, 262 at N = 16384."""
    return 4 * ((N + BTILE - 1) // BTILE) + 6 if N > 0 else 0


def roundings_tile(lags, top, lag, part="P", span=XTILE):
    """One tile (span <= 1024 samples of the window) of the search stage's tile sums, per lag.
    P, k_acf_tiles_lds (lags 20 / 36 / 52; kernels/search.inc, the loop `for (sub = 0; sub < nsub; sub++)`): acc[] lives across the
      tile's nsub = ceil(span / 256) sub-tiles, acf_tile_fma adds four FMAs per sub-tile, acf_reduce_store six additions:
      4 * ceil(span / 256) + 6 <= 22.
    P, k_acf_tiles<3> (12 lags; the loop `for (p = 0; p < PASSES; p++)`): a pass advances (64 - NB) * 4 = 244 samples and adds
      four FMAs per lag (`for q`), passes with s0 >= t1 are skipped, wave_transpose_sum<16> adds six: 4 * ceil(span / 244) + 6 <= 26.
    X (the pairs that straddle the tile's end; lag 0 has none):
      TOP = 17 / 33 (`if constexpr (TOP == 17 || TOP == 33)`): the lag's terms are dealt out over NP = 64 / (TOP - 1) lanes, CH =
        (TOP - 1) / NP terms each -- a chain of at most min(lag, CH) kept FMAs -- and log2(NP) cross-lane additions: min(lag, 4) + 2
        and min(lag, 16) + 1;
      every other kernel (`lane = lag`, both forms of the loop, and k_acf_tiles<3>): a chain of `lag` FMAs."""
    if part == "P":
        step = 244 if lags == 12 else BTILE
        return 4 * ((span + step - 1) // step) + 6 if span > 0 else 0
    if lag == 0:
        return 0
    if top in (17, 33) and lags != 12:
        w = top - 1
        np_, ch = 64 // w, w // (64 // w)
        return min(lag, ch) + (np_.bit_length() - 1)
    return lag


def roundings_search(ntiles):
    """k_search_finish / k_search_cert on top of the tile sums (kernels/search.inc, `for (t = ..; t <= tl; t++) sum += ts[..]`
    and `sum -= ts[.. + lags + lag]` in both kernels): the first P_t is added onto 0.0 (exact), every further tile is one
    rounded addition, the X of the last tile one rounded subtraction: (ntiles - 1) + 1."""
    return ntiles if ntiles > 0 else 0


def roundings_window(lags, top, lag, ntiles):
    """A candidate of ntiles tiles, in units of 2^-53 * E, E = the window's energy (sum of P_t[0]):
        |r - exact| <= u * ((roundings_tile(P) + roundings_search) * S_P + roundings_tile(X) * S_X)
    where S_P <= E (Cauchy-Schwarz) and S_X = sum_(j < lag) |x[t1 - lag + j] x[t1 + j]| <= sqrt(E_a E_b) <= (E_a + E_b) / 2 <= E / 2
    (E_a, E_b: the energies of the `lag` samples in front of and behind the candidate's end, disjoint parts of the window)."""
    return roundings_tile(lags, top, lag, "P") + roundings_search(ntiles) + (roundings_tile(lags, top, lag, "X") + 1) // 2


def chain_terms(n, lag):
    """(pair terms c * (a + b), leftover products) of the reference's chain for lag >= 1 (src/SLAPredictor.c, restated by
    chain_lag in kernels/lpc_chains.inc and slao_autocorr in oracle/sla_oracle.c)"""
    if lag >= n:
        return 0, 0
    grp = 1 + (n - 3 * lag) // (2 * lag) if 3 * lag < n else 0
    return grp * lag, n - 2 * grp * lag - lag


def roundings_reference(n, lag):
    """The reference's serial sums.  Lag 0: n squares, one rounding each, added one after the other onto 0.0 -- the first
    addition is exact, the first square then passes through n - 1 more: n.  Lag >= 1: T = pairs + leftovers terms; a pair term
    c * (a + b) carries two roundings (the addition, the product; |c (a + b)| <= |c a| + |c b|), a leftover one; the first term
    passes through T - 1 rounded additions: T + 1 with pair terms, T without."""
    if n <= 0 or lag >= n:
        return 0
    if lag == 0:
        return n
    pairs, left = chain_terms(n, lag)
    return pairs + left + (1 if pairs else 0)


# ------------------------------------------------------------------ what the certificates allow

def budget_blocks(n):
    """k_blocks_finish<P, true>: delta = budget * 2^-53 * r[0] covers the reference's sum AND k_acf_blocks' for every lag.
    Lag 0 is the tightest: the reference alone takes n.  n + 64 until k_acf_blocks needs more than 64 (N > 3584)."""
    return n + max(64, roundings_blocks(n))


SEARCH_BUDGET = 64              # k_search_finish / k_search_cert: delta = len * u * r0 + SEARCH_BUDGET * u * energy


# ------------------------------------------------------------------ material

def coloured(bits, seed, n):
    """two planes of coloured integer noise over a slow triangle (the recipe of tests/test_gpu_acf_lags.py::_coloured at any
    length; integer arithmetic only), left-justified in int32"""
    rng = np.random.default_rng(seed)
    a = 1 << (bits - 3)
    e = rng.integers(-a, a, (2, n + 2), dtype=np.int64)
    t = np.arange(n, dtype=np.int64)
    tri = np.abs((t * 37) % (4 * a) - 2 * a) - a
    q = (2 * e[:, 2:] + 3 * e[:, 1:-1] + e[:, :-2]) // 2 + np.stack([tri, -tri // 2])
    full = 1 << (bits - 1)
    q = np.clip(q, -full, full - 1)
    return (q << (32 - bits)).astype(np.int32)


MATERIALS = ("dc", "nyquist", "uniform", "coloured")


def material(kind, bits, n, seed=1):
    """two int32 planes of n samples, left-justified `bits`-bit material:
      dc        positive full scale on both planes (every product positive: the largest growth of the partial sums);
      nyquist   +full scale - 1 / -full scale alternating; the second plane +, +, -, - at full scale - 1, half that frequency,
                whose products at odd lags cancel completely (only a bound relative to S_lag holds there);
      uniform   uniform noise over the whole range;
      coloured  coloured()."""
    full = 1 << (bits - 1)
    if kind == "dc":
        q = np.full((2, n), full - 1, np.int64)
        q[1] -= full // 4
    elif kind == "nyquist":
        s = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int64)
        h = np.where(np.arange(n) % 4 < 2, 1, -1).astype(np.int64)
        q = np.stack([s * (full - 1), h * (full - 1)])
        q[0][s < 0] = -full
    elif kind == "uniform":
        q = np.random.default_rng(1000 * bits + seed).integers(-full, full, (2, n), dtype=np.int64)
    elif kind == "coloured":
        return coloured(bits, 1000 * bits + seed, n)
    else:
        raise ValueError(kind)
    return (q << (32 - bits)).astype(np.int32)


# ------------------------------------------------------------------ the cases of the block stage (CPU and GPU tests share them)

BLOCK_LENGTHS = (1, 3, 4, 5, 255, 256, 257, 1000, 4096, 16384)
BLOCK_MATERIAL = tuple((kind, bits) for kind in MATERIALS for bits in (24, 32))
Case = namedtuple("Case", "pcm_off num_samples channel win_off int_shift kind bits window")


def block_layout(sine, lengths=BLOCK_LENGTHS, materials=BLOCK_MATERIAL):
    """One PCM (two planes: every material in a segment of its own, back to back), one window pool and the cases of one launch:
    every material x length x window (rect, sine) x plane.  Starts step by 7 from 13 on inside a segment of odd length -- every
    residue mod 4, odd ones and 3 mod 4 among them, at every length -- and every block has loud samples in front of it and
    behind it; every window sits at an odd offset of the pool.  sine: {length: the oracle's sine window}."""
    ncase = len(lengths) * 2
    seg = 13 + 7 * ncase + max(lengths) + 64
    pcm = np.concatenate([material(kind, bits, seg) for kind, bits in materials], axis=1)
    pool, woff = [np.full(1, 0.5)], {}
    for wk in ("rect", "sine"):
        for n in lengths:
            woff[wk, n] = sum(len(w) for w in pool)
            pool.append(np.ones(n) if wk == "rect" else np.asarray(sine[n], np.float64))
            if n % 2:
                pool.append(np.full(1, 0.25))
    cases = []
    for mi, (kind, bits) in enumerate(materials):
        ci = 0
        for wk in ("rect", "sine"):
            for n in lengths:
                for ch in (0, 1):
                    cases.append(Case(mi * seg + 13 + 7 * ci, n, ch, woff[wk, n], 32 - bits, kind, bits, wk))
                ci += 1
    return pcm, np.concatenate(pool), cases
