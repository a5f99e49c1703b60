"""numpy fp64 restatement of option "local_norm" (include/m2t.h has the definition): local-window InstanceNorm statistics, the
Test-time Local Converter.  Written twice -- brute force per pixel, and by cumulative sums -- plus the gate the device's Xn is held
to, and one-line faults of the restatement that the gate must see (tests/test_local_norm_cpu.py).

Planes are (N, C, H, W) arrays on the padded plane.  Nothing here touches a device."""
import numpy as np

EPS = 1e-5
T_MIN, T_MAX = 8, 16384
FAULTS = ("start_half", "pads_swapped", "unbiased", "no_eps", "k_unclipped", "shift_col")


def window_start(y, k, n):
    """First row of the window of output row y on an axis of length n, k = min(T, n): a left pad of (k - 1) // 2, a right pad of
    k // 2, replicated edges -- i.e. clamp(y - (k - 1) // 2, 0, n - k)."""
    return min(max(y - (k - 1) // 2, 0), n - k)


def _starts(n, k, fault=None, axis="h"):
    left = k // 2 if fault in ("start_half", "pads_swapped") else (k - 1) // 2      # (the two faults are the same window)
    s = np.clip(np.arange(n) - left, 0, n - k)
    if fault == "shift_col" and axis == "w":
        s = np.clip(s + 1, 0, n - k)
    return s


def _finish(s1, s2, n, fault, T):
    if fault == "k_unclipped":               # the count of a T x T window although the plane clipped it
        n = float(T) * float(T)
    m = s1 / n
    v = np.maximum(s2 / n - m * m, 0.0)
    if fault == "unbiased":
        v = v * n / (n - 1.0)
    with np.errstate(divide="ignore"):
        r = 1.0 / np.sqrt(v + (0.0 if fault == "no_eps" else EPS))
    return m, v, r


def local_stats_brute(x, T, fault=None):
    """(m, v, r) per pixel, each window summed on its own."""
    x = np.asarray(x, dtype=np.float64)
    N, C, H, W = x.shape
    kh, kw = min(T, H), min(T, W)
    si, sj = _starts(H, kh, fault, "h"), _starts(W, kw, fault, "w")
    s1, s2 = np.empty_like(x), np.empty_like(x)
    xx = x * x
    for y in range(H):
        for c in range(W):
            s1[:, :, y, c] = x[:, :, si[y]:si[y] + kh, sj[c]:sj[c] + kw].sum(axis=(2, 3))
            s2[:, :, y, c] = xx[:, :, si[y]:si[y] + kh, sj[c]:sj[c] + kw].sum(axis=(2, 3))
    return _finish(s1, s2, float(kh * kw), fault, T)


def local_stats_cumsum(x, T, fault=None):
    """The same by an integral image (in extended precision, so that the difference of two prefixes loses nothing in fp64 terms)."""
    x = np.asarray(x, dtype=np.float64)
    N, C, H, W = x.shape
    kh, kw = min(T, H), min(T, W)
    si, sj = _starts(H, kh, fault, "h"), _starts(W, kw, fault, "w")

    def box(a):
        I = np.zeros((N, C, H + 1, W + 1), dtype=np.longdouble)
        I[:, :, 1:, 1:] = a.astype(np.longdouble).cumsum(axis=2).cumsum(axis=3)
        r0, r1, c0, c1 = si[:, None], si[:, None] + kh, sj[None, :], sj[None, :] + kw
        return (I[:, :, r1, c1] - I[:, :, r0, c1] - I[:, :, r1, c0] + I[:, :, r0, c0]).astype(np.float64)

    return _finish(box(x), box(x * x), float(kh * kw), fault, T)


def local_norm_exact(x, T, fault=None, stats=local_stats_cumsum):
    """(xn, m, r) in fp64 without the fp32 / output roundings: what the gate is centred on."""
    x = np.asarray(x, dtype=np.float64)
    m, _, r = stats(x, T, fault)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x - m) * r, m, r


def round_bf16(a):
    """fp32 -> bf16 -> fp32, round to nearest even."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def local_norm(x, T, dtype="fp32", fault=None, stats=local_stats_cumsum):
    """The definition to the letter: mean32 = fl32(m), rstd32 = fl32(r), xn = round_to_plan_dtype((fl32(x) - mean32) * rstd32) with
    the subtraction and the product as separate fp32 operations.  Returns float32."""
    x = np.asarray(x, dtype=np.float64)
    m, _, r = stats(x, T, fault)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x.astype(np.float32) - m.astype(np.float32)
        xn = d * r.astype(np.float32)
    return round_bf16(xn) if dtype == "bf16" else xn


def gate_bound(x, m, r, xn_exact, dtype):
    """Per element: 2^-22 (|x| + |m|) r -- the four fp32 roundings of mean, difference, rstd and product, doubled -- plus one rounding of
    the output type, 2^-24 (fp32) or 2^-8 (bf16) relative."""
    u = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -24
    return 2.0 ** -22 * (np.abs(x) + np.abs(m)) * r + u * np.abs(xn_exact)


def gate(xn_got, x, T, dtype):
    """Holds `xn_got` (the device's Xn, or a faulted restatement) against the restatement applied to x.  Returns (number of elements
    outside the bound, worst |error| / bound).  No element is excluded; a non-finite value counts as outside."""
    x = np.asarray(x, dtype=np.float64)
    ref, m, r = local_norm_exact(x, T)
    bound = gate_bound(x, m, r, ref, dtype)
    err = np.abs(np.asarray(xn_got, dtype=np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    bad = ~(err <= bound)
    return int(bad.sum()), float(np.nanmax(np.where(np.isfinite(ratio), ratio, np.inf)))


def stage_input(B, H0, W0, seed=0):
    """The test image [B, 3, H0, W0] in [0, 1]: a ramp plus noise plus a black half-plane, so that windows differ."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H0, 0:W0]
    ramp = (0.15 + 0.6 * (0.7 * yy / H0 + 0.3 * xx / W0))[None, None]
    img = ramp * np.array([1.0, 0.8, 0.6])[None, :, None, None] + 0.12 * rng.standard_normal((B, 3, H0, W0))
    img = np.clip(img, 0.0, 1.0)
    img[:, :, :, W0 // 2:] = 0.0
    return img.astype(np.float32)


def stage_plane(N, C, H, W, seed=0, dtype="fp32"):
    """A block input for the host-only tests, same construction on (N, C, H, W) with per-channel gains; representable in `dtype`."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (0.5 * yy / H - 0.2 * xx / W)[None, None]
    gain = (0.5 + rng.random((1, C, 1, 1)))
    a = (gain * ramp + 0.1 * rng.standard_normal((N, C, H, W)) + 0.3 * rng.standard_normal((1, C, 1, 1))).astype(np.float32)
    a[:, :, :, W // 2:] = 0.0
    return (round_bf16(a) if dtype == "bf16" else a).astype(np.float64)
