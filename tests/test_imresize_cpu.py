"""CPU tests (no GPU) of the bicubic resampler (include/m2t_resize.h, m2trans_amd/resize.py): the fp64 restatement the GPU tests
compare the kernels with (tests/imresize_ref.py) against torch's antialiased bicubic interpolation away from the borders and against
its anchors, the host-side filter taps against the restatement's tables, the third header against its signature table and the
library's symbols, and the tie margin of every x3 input the GPU tests use."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import imresize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, up) for s in R.SCALES for up in (False, True)]


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("s,up", CASES)
def test_reference_is_torch_antialiased_bicubic_in_the_interior_and_differs_at_the_borders(s, up):
    """fp64, 0 .. 255 data: <= 1e-11 absolute on the pixels at least 2 output pixels (down) / 2 s (up) from every border -- measured
    exactly 0 for x2 and x4 and <= 2e-12 for x3 --; at the borders torch renormalises the truncated filter where MATLAB mirrors, so
    the two MUST differ there (a mirror silently swapped for renormalisation would make them agree)."""
    rng = np.random.default_rng(1)
    h, w = (24, 30) if up else (24 * s, 36 * s)
    img = rng.integers(0, 256, size=(2, 3, h, w)).astype(np.float64)
    ref = R.imresize(img, s, up, axes=(2, 3))
    want = F.interpolate(torch.from_numpy(img), scale_factor=float(s) if up else 1.0 / s, mode="bicubic", antialias=True,
                         align_corners=False).numpy()
    assert ref.shape == want.shape == (2, 3, h * s if up else h // s, w * s if up else w // s)
    b = 2 * s if up else 2
    err = np.abs(ref - want)
    print(f"x{s} up={up}: interior {err[..., b:-b, b:-b].max():.3e}, whole image {err.max():.3e}")
    assert err[..., b:-b, b:-b].max() <= 1e-11
    border = err.copy()
    border[..., b:-b, b:-b] = 0.0
    assert border.max() > 1.0


@pytest.mark.parametrize("s,up", CASES)
def test_reference_anchors(s, up):
    n = 12 * s
    w, ind = R.contributions(n, s, up)
    assert ind.min() >= 0 and ind.max() < n
    sums = w.sum(axis=1)
    assert np.abs(sums - 1.0).max() <= 3e-16
    if s != 3:
        assert np.all(sums == 1.0) and np.all(w * 4096 == np.round(w * 4096))       # multiples of 2^-12: exact products and sums
    nonzero = {(2, False): 8, (3, False): 9, (4, False): 16}.get((s, up), 4)
    assert int((w != 0).sum(axis=1).max()) == nonzero
    # a constant image maps to the same constant, borders included
    const = np.full((n, 2 * n, 3), 77.0)
    out = R.imresize(const, s, up)
    assert np.abs(out - 77.0).max() <= (0.0 if s != 3 else 1e-13)
    # a linear ramp is reproduced in the interior: output i sits at u(i)
    yy, xx = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(2 * n, dtype=np.float64), indexing="ij")
    ramp = 3.0 * yy - 2.0 * xx + 11.0
    out = R.imresize(ramp, s, up)
    cy = (np.arange(out.shape[0]) + 0.5) / s - 0.5 if up else (np.arange(out.shape[0]) + 0.5) * s - 0.5
    cx = (np.arange(out.shape[1]) + 0.5) / s - 0.5 if up else (np.arange(out.shape[1]) + 0.5) * s - 0.5
    want = 3.0 * cy[:, None] - 2.0 * cx[None, :] + 11.0
    b = 2 * s if up else 2
    assert np.abs(out - want)[b:-b, b:-b].max() <= 1e-11
    assert np.abs(out - want).max() > 0.1                                            # ... and not at the mirrored borders


@pytest.mark.parametrize("s", R.SCALES)
def test_reference_mirror_reflects_a_short_axis_more_than_once(s):
    """Down on an axis of length s: one output whose 4 s taps fold several times through aux = [1:n, n:-1:1]; against numpy's
    symmetric padding applied repeatedly (each application at most one reflection)."""
    n = s
    a = np.arange(10, 10 + n, dtype=np.float64)
    w, raw = R.contributions(n, s, False, fold=False)
    _, ind = R.contributions(n, s, False)
    assert raw.min() < -n and raw.max() >= 2 * n                                     # more than one reflection on both sides
    padded, off = a, 0
    while off + raw.min() < 0 or off + raw.max() >= padded.size:
        k = padded.size
        padded, off = np.pad(padded, k, mode="symmetric"), off + k
    assert np.array_equal(a[ind], padded[off + raw])
    # the same on an up-scaling axis of length 1: every tap is the one pixel
    _, ind1 = R.contributions(1, s, True)
    assert np.all(ind1 == 0)


def test_quantiser_rounds_half_away_from_zero_and_saturates():
    v = np.array([-3.0, -0.5, -0.4999, 0.0, 0.5, 1.5, 2.5, 2.4999999, 254.5, 255.4, 255.5, 300.0])
    assert R.quantise(v).tolist() == [0, 0, 0, 0, 1, 2, 3, 2, 255, 255, 255, 255]
    assert np.trunc(-0.5) - 1 == -1 and R.tie_margin(np.array([1.25, 7.5001])) == pytest.approx(1e-4)


# ------------------------------------------------------------------------------------------------------------- the host taps
@pytest.mark.parametrize("s,up", CASES)
def test_filter_taps_equal_the_reference_table_row_of_an_interior_output(s, up):
    """resize.filter_taps (what the kernels receive) against the restatement's table rows of two interior cells (the first one and
    one further in): <= 1e-16 for x2 and x4 (in fact equal), <= 2 ulp of the weight for x3; the same taps are zero in both."""
    from m2trans_amd import resize as Z
    taps = Z.filter_taps(s, up)
    m0, nt = Z.FIRST_TAP[(s, up)], Z.NUM_TAPS[(s, up)]
    assert taps.shape == ((s if up else 1), nt) and taps.dtype == np.float64
    w, ind = R.contributions(12 * s, s, up, fold=False)
    for q in (2, 7):
        for p in range(taps.shape[0]):
            i, base = (q * s + p, q + m0) if up else (q, q * s + m0)
            row = dict(zip(ind[i].tolist(), w[i].tolist()))
            assert {k for k, v in row.items() if v != 0.0} == {base + t for t in range(nt) if taps[p, t] != 0.0}
            for t in range(nt):
                a, b = float(taps[p, t]), row.get(base + t, 0.0)
                assert abs(a - b) <= (1e-16 if s != 3 else 2 * np.spacing(abs(b))), (s, up, q, p, t, a, b)
    assert np.abs(taps.sum(axis=1) - 1.0).max() <= 3e-16
    if s != 3:
        assert np.all(taps.sum(axis=1) == 1.0) and np.all(taps * 4096 == np.round(taps * 4096))
    assert [int((taps != 0).sum(axis=1).max())] == [{(2, False): 8, (3, False): 9, (4, False): 16}.get((s, up), 4)]
    with pytest.raises(ValueError):
        Z.filter_taps(5, up)


# ------------------------------------------------------------------------------------------------------------- tie margin
@pytest.mark.parametrize("up", [False, True])
def test_the_x3_inputs_stay_off_the_rounding_ties(up):
    """x3 leaves about 1e-13 of fp64 freedom (its weights are not dyadic): every x3 input of the GPU tests keeps its pre-rounding
    values at least 1e-6 from a half-integer (the GPU tests assert it again on what they run).  x2 and x4 need no such condition --
    their sums are exact and a tie is resolved by the rounding rule -- and their inputs do contain exact ties, which is wanted."""
    margins = [R.tie_margin(v) for _, _, v in R.u8_cases(3, up)]
    if not up:
        margins += [R.tie_margin(v) for _, _, v, _ in R.dataset_images(3)]
    print(f"x3 up={up}: smallest distance to a half-integer {min(margins):.3e}")
    assert min(margins) >= 1e-6
    ties = sum(int((np.abs(v - np.floor(v) - 0.5) == 0).sum()) for s in (2, 4) for d in (False, True) for _, _, v in R.u8_cases(s, d))
    assert ties > 0
