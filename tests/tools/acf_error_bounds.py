"""Writes the largest error of the autocorrelation kernels' sums that tests/test_gpu_acf_error.py observes, in units of
2^-53 * sum|products|, per kernel and window length, beside the number of roundings tests/acfmodel.py derives for it.
Runs that file's tests in this process (one device) and formats what its measured() kept.  The figures are measurements:
no assertion uses them.

Run:  python tests/tools/acf_error_bounds.py [--out profiles/acf_error_bounds.txt]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pytest  # noqa: E402


def derived(stage, kernel, what, n):
    import acfmodel as A
    if kernel == "oracle":
        return "%d .. %d" % (min(A.roundings_reference(n, lag) for lag in range(min(n, 52))), A.roundings_reference(n, 0))
    if stage == "block":
        return str(A.roundings_blocks(n))
    lags, top = (int(v) for v in kernel[kernel.index("<") + 1:-1].split(","))
    if what == "P":
        return str(A.roundings_tile(lags, top, 0, "P", min(n, A.XTILE)))
    if what == "X":
        return "<= %d" % A.roundings_tile(lags, top, top - 1, "X")
    return "48 (asserted), %d derived" % (A.roundings_tile(lags, top, 0, "P") + A.roundings_search((n + A.XTILE - 1) // A.XTILE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acf_error_bounds.txt"))
    args = ap.parse_args()
    rc = pytest.main(["-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_acf_error.py")])
    import test_gpu_acf_error as T
    import torch
    rows = sorted(T.measured().items())
    with open(args.out, "w") as f:
        f.write("# largest |sum - exact| / (2^-53 * sum|products|) seen by tests/test_gpu_acf_error.py (pytest exit code %d)\n" % int(rc))
        f.write("# device: %s.  Measurements; the tests assert the derived counts only.\n" % torch.cuda.get_device_properties(0).gcnArchName)
        f.write("# 'window / energy': the assembled r[] of a whole window in units of 2^-53 * sum of P_t[0]\n")
        f.write("%-8s %-26s %-16s %7s  %10s  %s\n" % ("stage", "kernel", "sum", "length", "measured", "derived roundings"))
        for (stage, kernel, what, n), v in rows:
            f.write("%-8s %-26s %-16s %7d  %10.3f  %s\n" % (stage, kernel, what, n, v, derived(stage, kernel, what, n)))
    print("wrote", args.out, "rows", len(rows))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
