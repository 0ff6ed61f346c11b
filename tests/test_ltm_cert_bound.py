"""The error bound of the long-term stage's certificate (include/sla_hip.h: sla_hip_ltm_cert_eps_rel) against what the
reference's own FFT autocorrelation really loses: the oracle's ltm_analyze(..., want_autocorr=True) -- the reference's
transform, twiddle recurrence included -- compared with the exact integer autocorrelation over the lags the stage can
read (0 .. 261).  The built-in eps must be >= 16 x the largest error seen (the block certificate's convention).  The
fast kernel's side of the same comparison runs on the GPU (tests/test_gpu_ltm_cert.py::test_fast_autocorrelation_error)."""
import ctypes as C
from fractions import Fraction

import numpy as np

import slalibs as S
import waveforms as W

LAGS = 262


def exact_acf(x, nlags):
    """integer autocorrelation: int64 numpy while every sum stays below 2^62 (residuals below 2^24, at most 2^14 terms),
    Python integers beyond that"""
    n = len(x)
    peak = int(np.abs(x).max()) if n else 0
    if peak < 2 ** 24 and n <= 2 ** 14:
        assert peak * peak * n < 2 ** 62
        x64 = x.astype(np.int64)
        return [int(np.dot(x64[:n - k], x64[k:])) if k < n else 0 for k in range(nlags)]
    xs = [int(v) for v in x]
    return [sum(xs[i] * xs[i + k] for i in range(n - k)) if k < n else 0 for k in range(nlags)]


def blocks():
    """>= 200 seeded blocks: lengths 2048 .. 16384, 16 and 24 bits, white / gauss / music_like, each also with a sine added"""
    out = []
    for n in (2048, 3000, 4096, 6000, 8192, 16384):
        for bits in (16, 24):
            for name in ("white", "gauss", "music"):
                for sine in (0, 1):
                    for seed in range(3):
                        if name == "music":
                            x = W.music_like(1, n, bits, seed=seed + 1)[0]
                        else:
                            x = W.gen(name, 1, n, bits, seed=seed)[0]
                        x = (x >> (32 - bits)).astype(np.int64)
                        if sine:
                            x = x + np.round(2 ** (bits - 3) * np.sin(2 * np.pi * np.arange(n) / (97.3 + seed))).astype(np.int64)
                        lim = 2 ** (bits - 1) - 1
                        out.append((n, bits, name, sine, np.clip(x, -lim, lim).astype(np.int32)))
    return out


def test_reference_error_is_inside_the_bound():
    import sla_amd
    L = sla_amd.lib()
    L.sla_hip_ltm_cert_eps_rel.restype = C.c_double
    L.sla_hip_ltm_cert_eps_rel.argtypes = [C.c_uint32, C.c_double]
    o = S.oracle()
    cases = blocks()
    assert len(cases) >= 200
    worst = {}
    for n, bits, name, sine, x in cases:
        F = 1 << (2 * n - 1).bit_length()                  # the reference's size for a capacity of n: roundup2(2 n)
        ret, _, _, ac = o.ltm_analyze(x, F, 3, want_autocorr=True)
        ex = exact_acf(x, LAGS)
        assert ex[0] > 0
        # the reference's inverse transform is unnormalised and its input scaled by 2^-31: ac[k] = F/2 * 2^-62 * r[k]
        err = max(abs(Fraction(float(ac[k])) - Fraction(ex[k] * (F // 2), 2 ** 62)) for k in range(LAGS))
        rel = float(err / Fraction(ex[0] * (F // 2), 2 ** 62))
        worst[F] = max(worst.get(F, 0.0), rel)
    for F in sorted(worst):
        eps_rel = L.sla_hip_ltm_cert_eps_rel(F, 16.0)
        print("F %5d: largest |r_ref - exact| / r[0] = %.3e, built-in eps / r[0] = %.3e (x %.0f)" % (F, worst[F], eps_rel, eps_rel / worst[F]))
        assert eps_rel >= 16.0 * worst[F]


def test_python_integer_path_agrees():
    rng = np.random.default_rng(1)
    x = rng.integers(-2 ** 23, 2 ** 23, 300).astype(np.int32)
    a = exact_acf(x, 8)
    xs = [int(v) for v in x]
    assert a == [sum(xs[i] * xs[i + k] for i in range(len(xs) - k)) for k in range(8)]
    big = (x.astype(np.int64) << 7)                        # beyond 2^24: the Python-integer path
    b = exact_acf(big, 8)
    assert b == [v << 14 for v in a]


def test_safety_may_only_be_widened():
    import sla_amd
    L = sla_amd.lib()
    L.sla_hip_ltm_cert_eps_rel.restype = C.c_double
    L.sla_hip_ltm_cert_eps_rel.argtypes = [C.c_uint32, C.c_double]
    assert L.sla_hip_ltm_cert_eps_rel(8192, 32.0) == 2.0 * L.sla_hip_ltm_cert_eps_rel(8192, 16.0)
    assert L.sla_hip_ltm_cert_supported(8192) == 1 and L.sla_hip_ltm_cert_supported(65536) == 0
