"""Restatement of one row of the step health record (option "health" of include/m2t.h) in plain torch / NumPy fp64, on a tensor.

Plain helper module (CPU only, no pytest hooks), shared by tests/test_health_cpu.py and tests/test_gpu_health.py.  Counts, max and
min by comparison; the histogram from ``frexp`` of the fp32 value (not from its bit pattern, which is what the kernel reads); the sums
in NumPy's extended precision (x86 long double: a 64-bit significand, pairwise), whose own error is 2^-11 of the tolerance and less.
``sum_bounds`` is the tolerance of slots 4 and 5: the fp64 summation bound n * 2^-53 * sum |x| (Higham, Accuracy and Stability of
Numerical Algorithms, (4.4): any order of n - 1 fp64 additions; the squares are exact in fp64), derived, not measured.
"""
from __future__ import annotations

import numpy as np

SLOTS, BINS = 72, 64
EXACT_SLOTS = (0, 1, 2, 3, 6, 7) + tuple(range(8, SLOTS))
U = 2.0 ** -53


def _f32(t) -> np.ndarray:
    """Every element widened to fp32 exactly (bf16 -> fp32 is exact), flat."""
    if hasattr(t, "detach"):
        t = t.detach().float().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).reshape(-1)


def row(t) -> np.ndarray:
    """The 72 doubles of the row of tensor ``t``."""
    x32 = _f32(t)
    x = x32.astype(np.float64)
    out = np.zeros(SLOTS)
    finite = np.isfinite(x)
    nz = finite & (x != 0.0)
    a = np.abs(x[nz])
    out[0] = x.size
    out[1] = np.count_nonzero(~finite)
    out[2] = np.count_nonzero(np.isnan(x))
    out[3] = np.abs(x[finite]).max() if finite.any() else 0.0
    xl = x[finite].astype(np.longdouble)
    out[4] = float(xl.sum())
    out[5] = float((xl * xl).sum())
    out[6] = np.count_nonzero(finite & (x == 0.0))
    out[7] = a.min() if a.size else np.inf
    out[8] = out[6]
    out[8 + BINS - 1] = out[1]
    if a.size:
        # frexp: a = m * 2^e with m in [0.5, 1), so floor(log2 a) = e - 1; fp32 subnormals (below 2^-126) are far under the clamp
        _, e = np.frexp(a)
        bins = np.clip(e.astype(np.int64) - 1, -41, 20) + 42
        out[8:] += np.bincount(bins, minlength=BINS)
    return out


def sum_bounds(t):
    """(bound of slot 4, bound of slot 5) for any fp64 summation order of the finite elements of ``t``."""
    x = _f32(t).astype(np.float64)
    x = x[np.isfinite(x)]
    return x.size * U * np.abs(x).sum(), x.size * U * (x * x).sum()


def compare(got, t, what="") -> tuple:
    """Asserts a device / emulated row against the restatement; returns the two ratios error / bound of the sums (0 where the bound
    is 0 and the sums are equal)."""
    got = np.asarray(got, dtype=np.float64)
    want = row(t)
    for s in EXACT_SLOTS:
        assert got[s] == want[s], (what, "slot", s, got[s], want[s])
    ratios = []
    for s, bound in zip((4, 5), sum_bounds(t)):
        err = abs(got[s] - want[s])
        assert err <= bound, (what, "slot", s, got[s], want[s], err, bound)
        ratios.append(err / bound if bound > 0 else 0.0)
    return tuple(ratios)
