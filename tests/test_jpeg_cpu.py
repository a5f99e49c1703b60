"""CPU tests (no GPU) of the JPEG stage (include/m2t_jpeg.h, m2trans_amd/degrade.py): the C ABI table, the quantisation tables of the
library and of the restatement (tests/jpeg_ref.py) against the tables PIL writes, the constants against a 50-digit evaluation, the
restatement against a real JPEG round trip and its structure, the Degradation's new draws and keys, and the kernel text run on host
threads (tests/jpeg_emulate.cpp, built with AddressSanitizer and UBSan) against the restatement, byte for byte."""
import copy
import ctypes as C
import decimal
import io
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import degrade_ref as R
from tests import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def consts():
    from m2trans_amd.degrade import jpeg_constants
    c = jpeg_constants()
    assert c.dtype == np.float64 and c.shape == (320,)
    return c[:64].reshape(8, 8).copy(), c[64:].copy()


# ------------------------------------------------------------------------------------------------------------- C ABI
def _strip(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_descriptor_width_and_constant_count_are_the_headers_and_a_tap_keeps_its_two_roundings():
    from m2trans_amd import _lib, build as B
    assert int(re.search(r"#define M2T_DEGRADE_JPEG_DESC_COLS (\d+)", _strip("m2t_jpeg.h")).group(1)) == _lib.JPEG_DESC_COLS == 12
    assert int(re.search(r"#define M2T_JPEG_CONSTS (\d+)", _strip("m2t_jpeg.h")).group(1)) == _lib.JPEG_CONSTS == 320
    assert _lib.DEGRADE_DESC_COLS == 11
    assert "-ffp-contract=off" in B.FLAGS


# ------------------------------------------------------------------------------------------------------------- tables, constants
def _library_tables(quality):
    from m2trans_amd import _lib
    luma, chroma = (C.c_int * 64)(), (C.c_int * 64)()
    rc = _lib.load().m2t_jpeg_quant_tables(quality, luma, chroma)
    return rc, np.array(luma[:]).reshape(8, 8), np.array(chroma[:]).reshape(8, 8)


def test_quant_tables_of_library_and_restatement_are_the_ones_pil_writes():
    from PIL import Image
    img = Image.fromarray(np.random.RandomState(0).randint(0, 256, size=(16, 16, 3)).astype(np.uint8), "RGB")
    assert J.LUMA[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61]
    for quality in range(1, 101):
        buf = io.BytesIO()
        img.save(buf, "JPEG", quality=quality, subsampling=0)
        tables = Image.open(io.BytesIO(buf.getvalue())).quantization
        want = [np.array(tables[k]).reshape(8, 8) for k in (0, 1)]
        rc, luma, chroma = _library_tables(quality)
        assert rc == 0
        ref = J.quant_tables(quality)
        for got in ((luma, chroma), ref):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), quality
    for bad in (0, -1, 101):
        assert _library_tables(bad)[0] == -2
    from m2trans_amd import _lib
    assert _lib.load().m2t_jpeg_quant_tables(50, None, None) == -2


def _exact_cosines():
    """cos(k pi / 16), k = 0 .. 8, from the nested-square-root closed forms, as 50-digit decimals."""
    D = decimal.Decimal
    r2 = D(2).sqrt()
    half = D(1) / D(2)
    return [D(1), half * (2 + (2 + r2).sqrt()).sqrt(), half * (2 + r2).sqrt(), half * (2 + (2 - r2).sqrt()).sqrt(), half * r2,
            half * (2 - (2 - r2).sqrt()).sqrt(), half * (2 - r2).sqrt(), half * (2 - (2 + r2).sqrt()).sqrt(), D(0)]


def test_constants_are_within_one_ulp_of_the_closed_forms_and_orthonormal(consts):
    T, recip = consts
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        cos = _exact_cosines()
        c0 = (decimal.Decimal(1) / decimal.Decimal(8)).sqrt()
        worst = 0.0
        for u in range(8):
            for x in range(8):
                k = (2 * x + 1) * u % 32
                k = 32 - k if k > 16 else k
                exact = (c0 if u == 0 else decimal.Decimal(1) / 2) * (-cos[16 - k] if k > 8 else cos[k])
                err = abs(decimal.Decimal(float(T[u, x])) - exact)
                ulp = decimal.Decimal(float(np.spacing(abs(T[u, x]))))
                worst = max(worst, float(err / ulp))
                assert err <= ulp, (u, x, float(err / ulp))
    print(f"T: worst error {worst:.3f} ulp")
    ident = np.zeros((8, 8))
    for k in range(8):
        ident = ident + T[:, k][:, None] * T[:, k][None, :]
    assert float(np.abs(ident - np.eye(8)).max()) <= 1e-15
    assert recip[0] == 0.0 and np.array_equal(recip[1:], 1.0 / np.arange(1, 256))


# ------------------------------------------------------------------------------------------------------------- against real JPEG
def tissue(h, w, seed):
    """A synthetic grey "tissue" frame replicated to RGB: smooth structure times speckle, black outside a sector."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 110 + 60 * np.sin(xx / 5.0 + 0.3 * seed) * np.cos(yy / 7.0) + 30 * np.sin((xx + yy) / 3.0)
    img = base * (0.6 + 0.8 * rng.rand(h, w))
    ang = np.arctan2(xx - (w - 1) / 2.0, yy + 2.0)
    rad = np.hypot(xx - (w - 1) / 2.0, yy + 2.0)
    img[(np.abs(ang) > 0.6) | (rad > 0.95 * (h + 2))] = 0.0
    g = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, g, g], axis=2))


def _pil_roundtrip(img, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, "JPEG", quality=quality, subsampling=0)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))


@pytest.mark.parametrize("h,w", [(24, 24), (64, 48), (37, 53)])
def test_the_definition_is_close_to_a_real_jpeg_round_trip(consts, h, w):
    """mean |restatement - PIL| < 0.5 mean |PIL - source| at qualities 10, 30, 50, 75, 90: the definition is JPEG (libjpeg's integer
    DCT and colour tables differ in isolated coefficients; the mean is gated, not single pixels)."""
    T, recip = consts
    src = tissue(h, w, 7 * h + w)
    assert 0.1 < float((src[..., 0] == 0).mean()) < 0.9
    for quality in (10, 30, 50, 75, 90):
        real = _pil_roundtrip(src, quality).astype(np.float64)
        ours = J.roundtrip(src, quality, T, recip).astype(np.float64)
        loss = float(np.abs(real - src).mean())
        gap = float(np.abs(ours - real).mean())
        print(f"{h}x{w} q{quality}: ratio {gap / loss:.4f}, equal bytes {float((ours == real).mean()):.3f}, worst pixel "
              f"{int(np.abs(ours - real).max())}")
        assert loss > 0.0 and gap < 0.5 * loss, (quality, gap, loss)


# ------------------------------------------------------------------------------------------------------------- structure
def test_structure_of_the_restatement(consts):
    T, recip = consts
    flat = np.full((13, 19, 3), 93, dtype=np.uint8)
    assert np.array_equal(J.roundtrip(flat, 100, T, recip), flat)
    img = tissue(24, 32, 3)
    base = J.roundtrip(img, 50, T, recip)
    assert not np.array_equal(base, img)
    assert np.array_equal(base[..., 0], base[..., 1]) and np.array_equal(base[..., 0], base[..., 2])     # grey in, grey out
    poked = img.copy()
    poked[11, 20] = 255 - poked[11, 20]
    diff = np.argwhere((J.roundtrip(poked, 50, T, recip) != base).any(axis=2))
    assert len(diff) > 1 and (diff[:, 0] // 8 == 1).all() and (diff[:, 1] // 8 == 2).all()            # only its own 8 x 8 block
    out0 = J.roundtrip(img, 0, T, recip)
    assert np.array_equal(out0, img) and out0 is not img
    colour = np.random.RandomState(5).randint(0, 256, size=(9, 17, 3)).astype(np.uint8)
    a = J.roundtrip(colour, 90, T, recip)
    assert a.shape == colour.shape and a.dtype == np.uint8 and not np.array_equal(a[..., 0], a[..., 1])
    # a block that sticks out reads the edge pixel: the image padded by replication gives the same bytes inside
    padded = np.pad(colour, ((0, 7), (0, 7), (0, 0)), mode="edge")
    assert np.array_equal(J.roundtrip(padded, 30, T, recip)[:9, :17], J.roundtrip(colour, 30, T, recip))


# ------------------------------------------------------------------------------------------------------------- Degradation
def test_without_jpeg_the_draws_and_the_state_are_as_before():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.degrade import CONFIG_KEYS, Degradation
    D = Degradation(4, bank=8, noise=(1.0, 9.0), speckle=(0.0, 0.3), seed=5)
    _, rng = R.bank(4, M=8, seed=5)
    assert D.jpeg is None and D.jpeg_prob == 1.0
    want = []
    for n in range(5):
        index = rng.randrange(8)
        sa = rng.uniform(1.0, 9.0)
        want.append((index, sa, rng.uniform(0.0, 0.3), n))
    assert [D.draw() for _ in range(5)] == want
    assert set(D.get_state()) == {"random", "noise_id"} and D.get_state()["random"] == rng.getstate()
    with pytest.raises(M2TError, match="jpeg"):
        D.draw_jpeg()
    assert CONFIG_KEYS[:9] == ("bank", "sigma", "iso_prob", "ksize", "kernels", "noise", "speckle", "gray_noise", "seed")
    assert CONFIG_KEYS[9:] == ("jpeg", "jpeg_prob")


def test_draw_order_with_jpeg_is_pinned():
    from m2trans_amd.degrade import Degradation
    D = Degradation(4, bank=8, noise=(1.0, 9.0), speckle=(0.0, 0.3), seed=5, jpeg=(30, 95), jpeg_prob=0.5)
    _, rng = R.bank(4, M=8, seed=5)                             # the bank is the one without jpeg: the same draws before it
    assert np.array_equal(D.kernels, Degradation(4, bank=8, seed=5).kernels)
    before = random.getstate()
    got, want = [], []
    for n in range(40):
        got.append(D.draw() + (D.draw_jpeg(),))
        index = rng.randrange(8)
        sa = rng.uniform(1.0, 9.0)
        ss = rng.uniform(0.0, 0.3)
        apply = rng.random() < 0.5                             # two draws, always
        q = rng.randint(30, 95)
        want.append((index, sa, ss, n, q if apply else 0))
    assert got == want and random.getstate() == before
    qs = [g[4] for g in got]
    assert 0 in qs and any(q > 0 for q in qs) and all(q == 0 or 30 <= q <= 95 for q in qs)
    assert set(D.get_state()) == {"random", "noise_id"}
    E = copy.deepcopy(D)
    assert (E.draw(), E.draw_jpeg()) == (D.draw(), D.draw_jpeg())
    other = random.Random(3)
    twin = random.Random(3)
    state = D.get_state()
    q = D.draw_jpeg(other)                                     # a generator handed in (datas.Benchmark): the object's own stays put
    a, v = twin.random() < 0.5, twin.randint(30, 95)
    assert q == (v if a else 0) and D.get_state() == state
    assert all(Degradation(2, bank=1, jpeg=(77, 77)).draw_jpeg() == 77 for _ in range(3))
    assert all(Degradation(2, bank=1, jpeg=(1, 100), jpeg_prob=0.0).draw_jpeg() == 0 for _ in range(3))


def test_bad_jpeg_arguments_and_unknown_keys_are_named():
    from m2trans_amd import train as T
    from m2trans_amd._lib import M2TError
    from m2trans_amd.degrade import Degradation, from_config
    for bad in ((0, 50), (50, 101), (60, 50), (30.0, 95), (True, 95), 50, (30,), (30, 60, 90), "ab"):
        with pytest.raises(M2TError, match="jpeg must be"):
            Degradation(2, bank=1, jpeg=bad)
    for bad in (-0.1, 1.5, float("nan"), "1", None, True):
        with pytest.raises(M2TError, match="jpeg_prob"):
            Degradation(2, bank=1, jpeg=(30, 95), jpeg_prob=bad)
    assert Degradation(2, bank=1, jpeg=[1, 100], jpeg_prob=1).jpeg == (1, 100)
    base = {"scale": 4, "patch_size": 64, "batch_size": 2, "epochs": 1, "lr": 1e-4, "eta_min": 1e-6, "log_every": 1, "test_every": 1,
            "training_dataset": "folder", "train_hr_path": "somewhere"}
    r = T.resolve_config(dict(base, degradation={"bank": 4, "jpeg": [30, 95], "jpeg_prob": 0.8}))
    assert r["data"]["degradation"] == {"bank": 4, "jpeg": [30, 95], "jpeg_prob": 0.8}
    with pytest.raises(M2TError, match="jpg_prob"):
        T.resolve_config(dict(base, degradation={"bank": 4, "jpg_prob": 0.8}))
    D = from_config(4, {"bank": 4, "jpeg": [30, 95], "jpeg_prob": 0.8})
    assert D.jpeg == (30, 95) and D.jpeg_prob == 0.8
    with pytest.raises(M2TError, match="jpeg must be"):
        from_config(4, {"bank": 4, "jpeg": [95, 30]})


# ------------------------------------------------------------------------------------------------------------- host emulation
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++"), shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("jpeg") / "jpeg_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "tests", "emulate_hip"), "-I", os.path.join(ROOT, "m2trans_amd", "csrc"),
                    os.path.join(ROOT, "tests", "jpeg_emulate.cpp"), "-o", exe, "-lpthread"], check=True, capture_output=True)
    return exe


def _emulate(exe, tmp_path, consts, mode, hr, w, s, ly, lx, lh, lw, flags, gray, quality, noise_id, seed, sa, ss):
    H, W, _ = hr.shape
    T, recip = consts
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("12i", mode, H, W, s, w.shape[0], ly, lx, lh, lw, flags, int(gray), quality) + struct.pack("2Q", noise_id, seed)
                + struct.pack("2d", sa, ss) + np.concatenate([T.reshape(-1), recip]).tobytes()
                + np.ascontiguousarray(w, dtype=np.float64).tobytes() + np.ascontiguousarray(hr).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.uint8).reshape(lh, lw, 3)


def _hr(H, W, seed, colour):
    rng = np.random.RandomState(seed)
    if colour:
        return rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    g = rng.randint(0, 256, size=(H, W, 1)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g, 3, axis=2))


PATCH_CASES = [(s, K, lp, quality) for (s, K, lp) in ((2, 4, 8), (3, 7, 16), (4, 20, 24)) for quality in (1, 50, 100)]


@pytest.mark.parametrize("s,K,lp,quality", PATCH_CASES, ids=[f"x{s}-K{K}-lp{lp}-q{q}" for s, K, lp, q in PATCH_CASES])
def test_kernel_text_emulated_on_the_host_equals_the_restatement_patches(emulator, tmp_path, consts, s, K, lp, quality):
    """csrc/m2t_jpeg_tile.h on host threads under ASan / UBSan: lp = 8 (one block of a tile), 16 (one full tile), 24 (four tiles, three
    of them partial), all eight flag values (the transposed ones take the swapped walk), grey and colour HR, both noises: every byte."""
    T, recip = consts
    H = W = lp * s + 2 * s
    w = R.bank(s, M=2, K=K, seed=11)[0][1]
    nid, seed = (1 << 40) + 5, (7 << 32) + 33
    for flags in range(8):
        colour = flags % 2 == 1
        hr = _hr(H, W + (s if colour else 0), 100 * lp + flags, colour)
        ly, lx = (2, 1) if flags & 2 else (0, 0)
        lev = ((0.0, 0.0), (6.0, 0.0), (0.0, 0.2), (6.0, 0.2))[flags % 4]
        got = _emulate(emulator, tmp_path, consts, 0, hr, w, s, ly, lx, lp, lp, flags, not colour, quality, nid + flags, seed, *lev)
        want, _ = J.patch_u8(hr, w, s, lp, lx, ly, flags, T, recip, quality, lev[0], lev[1], not colour, nid + flags, seed)
        assert np.array_equal(got, want), (flags, int((got != want).sum()))
        assert not np.array_equal(want, R.patch_u8(hr, w, s, lp, lx, ly, flags, lev[0], lev[1], not colour, nid + flags, seed)[0]) or quality == 100


def test_kernel_text_emulated_quality_zero_is_the_degrade_tile(emulator, tmp_path, consts):
    hr = _hr(60, 64, 1, True)
    w = R.bank(2, M=1, K=6, seed=2)[0][0]
    for flags in (0, 5):
        got = _emulate(emulator, tmp_path, consts, 0, hr, w, 2, 1, 2, 24, 24, flags, False, 0, 9, 33, 5.0, 0.1)
        want, _ = R.patch_u8(hr, w, 2, 24, 2, 1, flags, 5.0, 0.1, False, 9, 33)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("lh,lw", [(13, 19), (33, 17)])
@pytest.mark.parametrize("quality", [1, 50, 100])
def test_kernel_text_emulated_whole_images(emulator, tmp_path, consts, lh, lw, quality):
    """Whole images whose size is no multiple of the block or the tile: the stage alone (grey and colour) and behind the degradation."""
    T, recip = consts
    one = np.zeros((2, 2))                                      # the stage alone does not read the kernel
    for colour in (False, True):
        img = _hr(lh, lw, lh + quality, colour)
        got = _emulate(emulator, tmp_path, consts, 2, img, one, 2, 0, 0, lh, lw, 0, True, quality, 0, 0, 0.0, 0.0)
        assert np.array_equal(got, J.roundtrip(img, quality, T, recip)), colour
    s = 3
    hr = _hr(lh * s + 2, lw * s + 1, lw, True)
    w = R.bank(s, M=1, K=7, seed=11)[0][0]
    got = _emulate(emulator, tmp_path, consts, 1, hr, w, s, 0, 0, lh, lw, 0, False, quality, 1 << 63, 33, 4.0, 0.15)
    assert np.array_equal(got, J.image_u8(hr, w, s, T, recip, quality, 4.0, 0.15, False, 1 << 63, 33))
