"""NumPy fp64 restatement of include/m2t_jpeg.h for the tests: the quantisation tables of a quality, the colour transform in the written
order, the 8 x 8 transform as explicit ordered sums (elementwise multiply, then add, eight terms from 0.0 with the index ascending --
no `@`, no einsum, whose order and contraction are not fixed), the quantiser, the way back.  Written from the definition, vectorised
over blocks (NumPy never fuses a multiply with an add), not from the kernel text.  T [8, 8] and recip [256] are arguments."""
import numpy as np

from tests import degrade_ref as R

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.full((8, 8), 99, dtype=np.int64)
CHROMA[0, :4], CHROMA[1, :4], CHROMA[2, :3], CHROMA[3, :2] = (17, 18, 24, 47), (18, 21, 26, 66), (24, 26, 56), (47, 66)


def quant_tables(quality):
    """(luminance [8, 8], chrominance [8, 8]) int64, natural order."""
    assert 1 <= quality <= 100
    S = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.minimum(np.maximum((base * S + 50) // 100, 1), 255) for base in (LUMA, CHROMA))


def _level(v):
    return np.minimum(np.maximum(np.rint(v), 0.0), 255.0)


def to_ycc(rgb):
    """uint8 [..., 3] -> Y, Cb, Cr as fp64 levels 0 .. 255."""
    r, g, b = (rgb[..., c].astype(np.float64) for c in range(3))
    y = _level((0.299 * r + 0.587 * g) + 0.114 * b)
    cb = _level(((128.0 - 0.168736 * r) - 0.331264 * g) + 0.5 * b)
    cr = _level(((128.0 + 0.5 * r) - 0.418688 * g) - 0.081312 * b)
    return y, cb, cr


def to_rgb(y, cb, cr):
    cb, cr = cb - 128.0, cr - 128.0
    r = _level(y + 1.402 * cr)
    g = _level((y - 0.344136 * cb) - 0.714136 * cr)
    b = _level(y + 1.772 * cb)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def plane_roundtrip(f, Q, T, recip):
    """f [by, bx, 8, 8] (plane - 128, block rows i, block columns j), Q [8, 8] -> plane' [by, bx, 8, 8] as levels 0 .. 255."""
    g = np.zeros_like(f)
    for j in range(8):                                          # g[i][v] = sum_j T[v][j] f[i][j]
        g = g + T[:, j][None, None, None, :] * f[:, :, :, j][:, :, :, None]
    F = np.zeros_like(f)
    for i in range(8):                                          # F[u][v] = sum_i T[u][i] g[i][v]
        F = F + T[:, i][None, None, :, None] * g[:, :, i, :][:, :, None, :]
    c = np.rint(F * recip[Q][None, None])
    d = c * Q.astype(np.float64)[None, None]
    h = np.zeros_like(f)
    for u in range(8):                                          # h[i][v] = sum_u T[u][i] d[u][v]
        h = h + T[u, :][None, None, :, None] * d[:, :, u, :][:, :, None, :]
    o = np.zeros_like(f)
    for v in range(8):                                          # o[i][j] = sum_v T[v][j] h[i][v]
        o = o + T[v, :][None, None, None, :] * h[:, :, :, v][:, :, :, None]
    return _level(o + 128.0)


def roundtrip(img, quality, T, recip):
    """uint8 [h, w, 3] -> uint8 [h, w, 3]; blocks anchored at (0, 0), a block that sticks out reads the edge pixel; quality 0 skips."""
    if quality == 0:
        return img.copy()
    h, w, _ = img.shape
    H8, W8 = -(-h // 8) * 8, -(-w // 8) * 8
    ys, xs = np.minimum(np.arange(H8), h - 1), np.minimum(np.arange(W8), w - 1)
    full = img[ys[:, None], xs[None, :], :]
    tables = quant_tables(quality)
    out = []
    for k, plane in enumerate(to_ycc(full)):
        f = (plane - 128.0).reshape(H8 // 8, 8, W8 // 8, 8).transpose(0, 2, 1, 3)
        p = plane_roundtrip(np.ascontiguousarray(f), tables[min(k, 1)], T, recip)
        out.append(p.transpose(0, 2, 1, 3).reshape(H8, W8))
    return np.ascontiguousarray(to_rgb(*out)[:h, :w])


# ------------------------------------------------------------------------------------------------------------- behind the degradation
def image_u8(hr, w, s, T, recip, quality, sigma_add=0.0, sigma_speckle=0.0, gray=True, noise_id=0, seed=33):
    return roundtrip(R.image_u8(hr, w, s, sigma_add, sigma_speckle, gray, noise_id, seed), quality, T, recip)


def patch_u8(hr, w, s, lp, lx, ly, flags, T, recip, quality, sigma_add=0.0, sigma_speckle=0.0, gray=True, noise_id=0, seed=33):
    """(LR uint8 [lp, lp, 3], HR uint8) after the flips: degrade in source orientation, the stage on the patch, then the flips."""
    q, _ = R.patch_u8(hr, w, s, lp, lx, ly, 0, sigma_add, sigma_speckle, gray, noise_id, seed)
    return R.flip(roundtrip(q, quality, T, recip), flags), R.flip(hr[ly * s:(ly + lp) * s, lx * s:(lx + lp) * s, :], flags)


def patches(hr_images, kernels, s, lp, items, T, recip, gray=True, seed=33):
    """items: (image index, lx, ly, flags, bank index, sigma_add, sigma_speckle, noise_id, quality) -> (lr, hr) float32 NCHW."""
    lr, hr = [], []
    for img, lx, ly, flags, index, sa, ss, nid, quality in items:
        a, b = patch_u8(hr_images[img], kernels[index], s, lp, lx, ly, flags, T, recip, quality, sa, ss, gray, nid, seed)
        lr.append(R.to_tensor(a))
        hr.append(R.to_tensor(b))
    return np.stack(lr), np.stack(hr)
