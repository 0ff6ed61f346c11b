"""Device-free model of the long-term stage's exact route (k_ltm_acf / k_ltm_acf2 / k_ltm_acf2_list and the pitch scan of
acf_emit, sla_amd/csrc/kernels/longterm.inc): the reference's real-FFT autocorrelation from the oracle, the serial pitch
scan of src/SLAPredictor.c:866-924 with flags that say which of its corners an input reached, the 12-double record the
kernels hand to the solver, and a catalogue of residual blocks that reaches every corner (tests/test_ltm_scan_model.py
asserts that it does)."""
import functools

import numpy as np

MAX_PERIOD = 256                    # K_LTM_MAX_PERIOD: the scan walks the lags 1 .. 255, lags 256 and 257 are its two special cases
FLT_MIN = float(np.finfo(np.float32).tiny)
SWEEP_LAGS = range(2, 258)
FLAGS = ("open256_chosen", "open256_seen", "pseudo256_chosen", "pseudo257_chosen", "pseudo_seen_no_candidate",
         "start_is_downward_crossing", "chosen_eq_2", "exact_zero_in_scan", "no_candidate", "silent", "tied_top")


# ---- the autocorrelation ----------------------------------------------------------------------------------------------

def acf_by_fft(oracle, x, fft_size):
    """slao_ltm_analyze lines 601-610 from the oracle's FFT and numpy elementwise operations (every product and sum its own
    rounding): scale by 2^-31, forward real FFT, ac[0]^2, ac[1]^2, re re + im im, inverse.  Any len(x) <= fft_size."""
    x = np.ascontiguousarray(x, np.int32)
    assert 0 < len(x) <= fft_size
    d = np.zeros(fft_size)
    d[:len(x)] = x.astype(np.float64) * 2.0 ** -31
    d = oracle.fft(d, 1)
    p = np.zeros(fft_size)
    p[0] = d[0] * d[0]
    p[1] = d[1] * d[1]
    re, im = d[2::2], d[3::2]
    rr = re * re
    ii = im * im
    p[2::2] = rr + ii
    return oracle.fft(p, -1)


def reference_acf(oracle, x, fft_size):
    """the fft_size doubles of the reference's route: the oracle's own where it accepts the block (2 len(x) <= fft_size),
    the same sequence built from its FFT where it refuses (fft_size / 2 < len(x) <= fft_size)"""
    x = np.ascontiguousarray(x, np.int32)
    if 2 * len(x) <= fft_size:
        ret, _, _, ac = oracle.ltm_analyze(x, fft_size, 1, want_autocorr=True)
        assert ret in (0, 4)
        return ac
    return acf_by_fft(oracle, x, fft_size)


# ---- the scan ---------------------------------------------------------------------------------------------------------

def scan(ac):
    """(chosen lag, number of candidates, set of flags): the serial scan of slao_ltm_analyze lines 613-640.  chosen = 0:
    silent block or no candidate."""
    ac = [float(v) for v in ac[:MAX_PERIOD + 3]]
    flags = set()
    if abs(ac[0]) <= FLT_MIN:
        flags.add("silent")
        return 0, 0, flags
    if any(v == 0.0 for v in ac[1:MAX_PERIOD + 3]):
        flags.add("exact_zero_in_scan")
    cand = []                                                    # (lag, kind of segment it came from)
    i = 1
    while i < MAX_PERIOD:
        start = i
        while start < MAX_PERIOD and not (ac[start - 1] < 0.0 and ac[start] > 0.0):
            start += 1
        end = start + 1
        while end < MAX_PERIOD and not (ac[end] > 0.0 and ac[end + 1] < 0.0):
            end += 1
        if start == MAX_PERIOD:
            kind = "pseudo"                                      # no upward crossing left: lags 256 and 257 are inspected
        elif end == MAX_PERIOD:
            kind = "open"                                        # unterminated segment: [start, 256]
            flags.add("open256_seen")
        else:
            kind = "closed"
        if start < MAX_PERIOD and ac[start] > 0.0 and ac[start + 1] < 0.0:
            flags.add("start_is_downward_crossing")              # (the search for the end begins behind the start)
        best, best_val = 0, 0.0
        for j in range(start, end + 1):
            if ac[j] > ac[j - 1] and ac[j] > ac[j + 1] and ac[j] > best_val:
                best, best_val = j, ac[j]
        if best != 0:
            cand.append((best, kind))
        pseudo_seen = (kind == "pseudo")                         # (the last round of the loop, if any)
        i = end + 1
    if not cand:
        flags.add("no_candidate")
        if pseudo_seen:
            flags.add("pseudo_seen_no_candidate")
        return 0, 0, flags
    top = max(ac[j] for j, _ in cand)
    chosen, kind = next((j, k) for j, k in cand if ac[j] >= top)
    if sum(ac[j] == top for j, _ in cand) > 1:
        flags.add("tied_top")                                    # several segments attain the maximum: the first one wins
    if kind == "open" and chosen == 256:
        flags.add("open256_chosen")
    if kind == "pseudo":
        flags.add("pseudo256_chosen" if chosen == 256 else "pseudo257_chosen")
    if chosen == 2:
        flags.add("chosen_eq_2")
    return chosen, len(cand), flags


def record(ac):
    """the 12 doubles {code, chosen, ac[0..4], ac[chosen-2 .. chosen+2]} of the kernels: code 0 silent, 1 a candidate, 2 none;
    0.0 for an index below 0"""
    chosen, _, flags = scan(ac)
    code = 0.0 if "silent" in flags else (2.0 if "no_candidate" in flags else 1.0)
    mid = [float(ac[chosen + k - 2]) if chosen + k >= 2 else 0.0 for k in range(5)]
    return np.array([code, float(chosen)] + [float(v) for v in ac[:5]] + mid)


# ---- the blocks -------------------------------------------------------------------------------------------------------

def _i32(v):
    return np.ascontiguousarray(np.clip(np.rint(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64).astype(np.int32))


def table_rows(fft_size):
    """the eight blocks whose scans were checked by hand against the oracle: n = fft_size / 2 samples but for the last"""
    n = fft_size // 2
    t = np.arange(n)
    return [("comb256", _i32(1e5 + 3e6 * (t % 256 == 0))),                     # no upward crossing in 1 .. 255: pitch 256
            ("comb257", _i32(1e5 + 3e6 * (t % 257 == 0))),                     # the same: pitch 257
            ("comb255", _i32(1e5 + 3e6 * (t % 255 == 0))),                     # lags 256, 257 inspected, no local maximum
            ("sin256", _i32(1e6 * np.sin(2 * np.pi * t / 256))),               # one segment [192, 256], unterminated
            ("cos4", _i32(1e6 * np.cos(2 * np.pi * t / 4 + 0.3))),             # 64 candidates, the last segment unterminated
            ("two_impulses", _i32(1e6 * (t == 10) + 9e5 * (t == 50))),         # one-lag segments in rounding noise
            ("alternating", _i32(np.where(t % 2 == 0, -2.0 ** 31, 2.0 ** 31 - 1))),   # chosen 2: the record's window starts at lag 0
            ("single_one", np.ones(1, np.int32))]                              # lags 1 .. all exactly 0.0, ac[0] live: code 2


def plain_blocks(fft_size):
    """the catalogue without the lag sweep: the table rows, noise of three widths, ramp, DC, zeros, the shortest and the
    longest lengths, lengths around the last lag the scan reads, a pitched block"""
    n = fft_size // 2
    t = np.arange(n)
    rng = np.random.default_rng(fft_size)
    noise20 = lambda m: rng.integers(-2 ** 19, 2 ** 19, m).astype(np.int32)
    out = table_rows(fft_size)
    out += [("noise32", rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)),
            ("noise20", noise20(n)),
            ("noise_lsb", rng.integers(-1, 2, n).astype(np.int32)),
            ("ramp", _i32((t - n // 2) * 1000.0)),
            ("dc", np.full(n, 12345, np.int32)),
            ("zeros", np.zeros(n, np.int32))]
    out += [("len%d" % m, noise20(m)) for m in (1, 2, 3, 255, 256, 257, 258, 259, 300, n - 1, n)]
    out.append(("pitched", _i32(3e4 * rng.standard_normal(n) + 2e5 * np.sin(2 * np.pi * t / 97.3))))
    return out


def sweep_blocks(fft_size):
    """one block per lag d = 2 .. 257 in two families: a sine of period d, and two impulses d apart on 18-bit noise 40 dB
    below them; then two small families aimed at what the sweep reaches only by luck"""
    n = fft_size // 2
    t = np.arange(n)
    out = []
    for d in SWEEP_LAGS:
        out.append(("sin%d" % d, _i32(1e6 * np.sin(2 * np.pi * t / d + 0.3))))
    for d in SWEEP_LAGS:
        rng = np.random.default_rng(1000 * d + fft_size)
        x = rng.integers(-2 ** 17, 2 ** 17, n).astype(np.float64)
        p = 3 + (7 * d) % (n - 300)
        x[p] = x[p + d] = 100.0 * 2 ** 17
        out.append(("imp%d" % d, _i32(x)))
    # the same family eight more times at the lags around the end of the scan: whether lag 256 / 257 is reached depends on
    # the signs the noise leaves at the lags 254 .. 256
    for d in (254, 255, 256, 257):
        for k in range(8):
            rng = np.random.default_rng(100000 * (k + 1) + 1000 * d + fft_size)
            x = rng.integers(-2 ** 17, 2 ** 17, n).astype(np.float64)
            p = 3 + (7 * d + 131 * k) % (n - 300)
            x[p] = x[p + d] = 100.0 * 2 ** 17
            out.append(("late%d_%d" % (d, k), _i32(x)))
    # three equal impulses at p, p + a, p + a + b in silence: the lags a, b and a + b are equal in exact arithmetic, and in
    # about one block of ten the top two come out of the transform as equal doubles -- the first of them must win
    rng = np.random.default_rng(7 + fft_size)
    for k in range(48):
        a, b = (int(v) for v in rng.choice(np.arange(3, 126), 2, replace=False))
        x = np.zeros(n, np.int32)
        p = int(rng.integers(0, n - 300))
        x[[p, p + a, p + a + b]] = int(rng.choice([1, 3, 1000, 12345, 2 ** 20, 2 ** 30]))
        out.append(("tri%d" % k, x))
    return out


def catalogue(fft_size, sweep=True):
    """[(name, int32 block)]: every block at most fft_size / 2 samples"""
    return plain_blocks(fft_size) + (sweep_blocks(fft_size) if sweep else [])


class Case:
    """a catalogue block with its reference (all fft_size doubles only for the blocks outside the sweep)"""
    __slots__ = ("name", "x", "ac", "chosen", "ncand", "flags", "record")

    def __init__(self, name, x, ac, keep):
        self.name, self.x = name, x
        self.ac = ac if keep else None
        self.chosen, self.ncand, self.flags = scan(ac)
        self.record = record(ac)


@functools.lru_cache(maxsize=None)
def _prepared(fft_size, part):
    import slalibs as S
    oracle = S.oracle()
    blocks = plain_blocks(fft_size) if part == "plain" else sweep_blocks(fft_size)
    return tuple(Case(name, x, reference_acf(oracle, x, fft_size), part == "plain") for name, x in blocks)


def prepared(fft_size, sweep=True):
    """the catalogue with its references from the oracle, computed once per process and size; read-only"""
    return _prepared(fft_size, "plain") + (_prepared(fft_size, "sweep") if sweep else ())


def flag_counts(cases):
    return {f: sum(f in c.flags for c in cases) for f in FLAGS}
