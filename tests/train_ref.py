"""Restatements of the training-loop kernels (include/m2t_train.h) that the tests compare them with: the step meter as a Python
class doing sequential fp64 sums, and the preview strip as a numpy integer implementation of the header's definition."""
from __future__ import annotations

import math

import numpy as np


class RefMeter:
    """m2t_meter_reset / m2t_meter_update on the host.  A sample is a Python float (fp64), a numpy float32 / float64 scalar, or
    None for an absent column."""

    def __init__(self, n_cols: int, ring_rows: int):
        self.n_cols, self.ring_rows = n_cols, ring_rows
        self.reset()

    def reset(self):
        self.record = np.zeros((self.n_cols, 8), dtype=np.float64)
        self.record[:, 3] = math.inf
        self.record[:, 4] = -math.inf
        self.ring = np.full((self.ring_rows, self.n_cols + 1), np.nan, dtype=np.float32)

    def update(self, values, step: int):
        row = self.ring[step % self.ring_rows]
        row[0] = np.float32(step)
        for c, v in enumerate(values):
            if v is None:
                row[c + 1] = np.nan
                continue
            v = float(v)                                   # float32 -> float64 is exact
            r = self.record[c]
            if math.isfinite(v):
                r[0] = r[0] + v                            # one fp64 add per call, in call order
                r[1] += 1.0
                r[3] = v if v < r[3] else r[3]
                r[4] = v if v > r[4] else r[4]
            else:
                r[2] += 1.0
            r[5] = v
            with np.errstate(over="ignore"):
                row[c + 1] = np.float32(v)                 # round to nearest even


def quantise(x: np.ndarray, rgb_range: float) -> np.ndarray:
    """q(v) = trunc(min(max((255 v) / rgb_range, 0), 255)) in float32, NaN -> 0; int64 out."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.float32(255.0) * x.astype(np.float32)) / np.float32(rgb_range)
        t = np.where(t > 0, t, np.float32(0.0))
        t = np.where(t < 255, t, np.float32(255.0))
    return t.astype(np.int64)


def _taps(n_out: int, s: int, n_in: int):
    """Per destination index: the two clamped taps and their integer weights out of 2 s (half-pixel centres)."""
    t0, t1, w0, w1 = [], [], [], []
    for i in range(n_out):
        num = 2 * i + 1 - s
        i0 = num // (2 * s)                                # floor, also for a negative numerator
        f = num - 2 * s * i0
        t0.append(min(max(i0, 0), n_in - 1))
        t1.append(min(max(i0 + 1, 0), n_in - 1))
        w0.append(2 * s - f)
        w1.append(f)
    return np.array(t0), np.array(t1), np.array(w0, dtype=np.int64), np.array(w1, dtype=np.int64)


def upsample_quantised(q: np.ndarray, s: int) -> np.ndarray:
    """q int64 [3,h,w] -> int64 [3,h s,w s]: (sum of wy wx q + 2 s^2) // (4 s^2)."""
    _, h, w = q.shape
    y0, y1, wy0, wy1 = _taps(h * s, s, h)
    x0, x1, wx0, wx1 = _taps(w * s, s, w)
    wy0, wy1 = wy0[None, :, None], wy1[None, :, None]
    wx0, wx1 = wx0[None, None, :], wx1[None, None, :]
    acc = wy0 * (wx0 * q[:, y0][:, :, x0] + wx1 * q[:, y0][:, :, x1]) + wy1 * (wx0 * q[:, y1][:, :, x0] + wx1 * q[:, y1][:, :, x1])
    return (acc + 2 * s * s) // (4 * s * s)


def preview_strip(lr: np.ndarray, sr: np.ndarray, hr: np.ndarray, rgb_range: float) -> np.ndarray:
    """lr float32 [3,h,w], sr / hr float32 [3,h s,w s] -> uint8 [h s, 3 w s, 3]: upsampled LR | SR | HR."""
    s = sr.shape[1] // lr.shape[1]
    assert sr.shape == (3, lr.shape[1] * s, lr.shape[2] * s) and hr.shape == sr.shape
    left = upsample_quantised(quantise(lr, rgb_range), s)
    strip = np.concatenate([left, quantise(sr, rgb_range), quantise(hr, rgb_range)], axis=2)       # [3, h s, 3 w s]
    return np.ascontiguousarray(strip.transpose(1, 2, 0)).astype(np.uint8)
