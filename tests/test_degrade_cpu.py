"""CPU tests (no GPU) of the LR synthesis beyond bicubic (include/m2t_degrade.h, m2trans_amd/degrade.py): the C ABI table, the fp64
restatement the GPU tests compare the kernels with (tests/degrade_ref.py) -- the generator's known answers, the bank, the tap
geometry, the folding, the variate's statistics -- the Degradation object, the train.py key, and the kernel text run on host threads
(tests/degrade_emulate.cpp, built with AddressSanitizer and UBSan) against the restatement, byte for byte."""
import copy
import ctypes as C
import os
import pickle
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import degrade_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- C ABI
def _strip(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_descriptor_width_is_the_headers_and_a_tap_keeps_its_two_roundings():
    from m2trans_amd import _lib, build as B
    assert int(re.search(r"#define M2T_DEGRADE_DESC_COLS (\d+)", _strip("m2t_degrade.h")).group(1)) == _lib.DEGRADE_DESC_COLS
    assert "-ffp-contract=off" in B.FLAGS                      # the multiply and the add of a tap are two roundings


# ------------------------------------------------------------------------------------------------------------- the restatement
def _words(s):
    return [int(x, 16) for x in s.split()]


@pytest.mark.parametrize("ctr,key,want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")], ids=["zero", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    out = R.philox4x32_10([np.array([w], dtype=np.uint64) for w in _words(ctr)], _words(key))
    assert [int(v[0]) for v in out] == _words(want)


def test_variate_is_exact_and_bounded():
    g = R.variate(np.arange(4096, dtype=np.uint64), 0, 0, 7, 33)
    assert g.dtype == np.float64 and float(np.abs(g).max()) < 6.0
    assert np.array_equal(g * 2.0 ** 33, np.rint(g * 2.0 ** 33))              # a multiple of 2^-33
    assert not np.array_equal(g, R.variate(np.arange(4096, dtype=np.uint64), 1, 0, 7, 33))
    assert not np.array_equal(g, R.variate(np.arange(4096, dtype=np.uint64), 0, 1, 7, 33))
    assert not np.array_equal(g, R.variate(np.arange(4096, dtype=np.uint64), 0, 0, 7 + (1 << 32), 33))
    assert not np.array_equal(g, R.variate(np.arange(4096, dtype=np.uint64), 0, 0, 7, 33 + (1 << 32)))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_bank_properties(s):
    from m2trans_amd.degrade import Degradation, default_ksize
    kernels, _ = R.bank(s, M=32)
    D = Degradation(s, bank=32)
    K = kernels.shape[1]
    assert K == D.ksize == default_ksize(s, 0.8 * s) == {2: 12, 3: 17, 4: 20}[s] and D.kernels.shape == kernels.shape
    assert float(np.abs(D.kernels - kernels).max()) <= 1e-14                    # two routes to Sigma^-1: a few ulp of the exponent
    for bank in (kernels, D.kernels):
        assert float(np.abs(bank.reshape(32, -1).sum(axis=1) - 1.0).max()) <= 1e-15 * K * K
        assert float(np.abs(bank - bank[:, ::-1, ::-1]).max()) <= 1e-15
    rng = random.Random(33)
    iso = []
    for _ in range(32):
        iso.append(rng.random() < 0.5)
        rng.uniform(0, 1)
        if not iso[-1]:
            rng.uniform(0, 1)
        rng.uniform(0, 1)
    assert any(iso) and not all(iso)
    for m in range(32):
        sym = float(np.abs(D.kernels[m] - D.kernels[m].T).max())
        assert sym <= 1e-15 if iso[m] else sym > 1e-6, (m, iso[m], sym)
    assert default_ksize(3, 0.1) == 3 and default_ksize(2, 0.1) == 2 and default_ksize(3, 10.0) == 21 and default_ksize(4, 10.0) == 20
    assert R.default_ksize(3, 0.1) == 3 and R.default_ksize(2, 0.1) == 2 and R.default_ksize(3, 10.0) == 21


def test_first_tap_centres_the_kernel_on_the_footprint_for_every_scale():
    for s in (2, 3, 4):
        for K in range(1 if s % 2 else 2, 22, 2):
            for X in (0, 1, 7):
                first = R.first_tap(s, X, K)
                assert first == s * X + (s - K) / 2
                # the centre of the K taps is the centre of the footprint s X .. s X + s - 1
                assert first + (K - 1) / 2 == s * X + (s - 1) / 2


def test_folding_is_symmetric_with_period_2n_and_repeats():
    N = 3
    want = {-10: 2, -9: 2, -8: 1, -7: 0, -6: 0, -5: 1, -4: 2, -3: 2, -2: 1, -1: 0, 0: 0, 1: 1, 2: 2, 3: 2, 4: 1, 5: 0, 6: 0, 7: 1, 8: 2,
            9: 2, 10: 1, 11: 0, 12: 0}
    assert set(want) == set(range(-10, N + 10))
    for i, w in want.items():
        assert R.fold(i, N) == w, i
        assert R.fold(i + 2 * N, N) == w
    assert [R.fold(i, 1) for i in range(-3, 4)] == [0] * 7


@pytest.mark.parametrize("noise_id", [0, 1, 12345678901])
def test_variate_statistics_of_the_restatement(noise_id):
    acc = np.full((64, 64, 3), 128.0)
    q = R.quantise(acc, 8.0, 0.0, True, noise_id, 33).astype(np.float64)
    assert np.array_equal(q[..., 0], q[..., 1]) and np.array_equal(q[..., 0], q[..., 2])       # gray: one variate per pixel
    mean, std = float(q[..., 0].mean()) - 128.0, float(q[..., 0].std())
    print(f"noise_id {noise_id}: mean {mean:+.2f}, standard deviation {std:.2f}")
    assert abs(mean) <= 0.5 and 7.5 <= std <= 8.5
    colour = R.quantise(acc, 8.0, 0.0, False, noise_id, 33)
    assert np.array_equal(colour[..., 0], q[..., 0].astype(np.uint8)) and not np.array_equal(colour[..., 0], colour[..., 1])


def test_restatement_identities():
    rng = np.random.RandomState(1)
    hr = rng.randint(0, 256, size=(12, 15, 3)).astype(np.uint8)
    delta = np.zeros((3, 3))
    delta[1, 1] = 1.0
    assert np.array_equal(R.image_u8(hr, delta, 3), hr[1::3, 1::3])
    flat = np.full((8, 12, 3), 77, dtype=np.uint8)
    k, _ = R.bank(4, M=1, K=20)
    assert np.array_equal(R.image_u8(flat, k[0], 4), np.full((2, 3, 3), 77, dtype=np.uint8))
    lr, hr_p = R.patch_u8(hr, delta, 3, 2, 1, 2, 5)
    assert np.array_equal(hr_p, R.flip(hr[6:12, 3:9], 5)) and np.array_equal(lr, R.flip(hr[1::3, 1::3][2:4, 1:3], 5))


# ------------------------------------------------------------------------------------------------------------- Degradation
def test_draw_order_state_and_the_global_generator():
    from m2trans_amd.degrade import Degradation
    D = Degradation(4, bank=8, noise=(1.0, 9.0), speckle=(0.0, 0.3), seed=5)
    _, rng = R.bank(4, M=8, seed=5)                             # the generator after the bank's draws
    before = random.getstate()
    np_before = np.random.get_state()[1].copy()
    got = [D.draw() for _ in range(5)]
    assert random.getstate() == before and np.array_equal(np.random.get_state()[1], np_before)
    want = []
    for n in range(5):
        index = rng.randrange(8)
        sa = rng.uniform(1.0, 9.0)
        want.append((index, sa, rng.uniform(0.0, 0.3), n))
    assert got == want
    state = pickle.loads(pickle.dumps(D.get_state()))
    nxt = [D.draw() for _ in range(3)]
    E = Degradation(4, bank=8, noise=(1.0, 9.0), speckle=(0.0, 0.3), seed=5)
    E.set_state(state)
    assert [E.draw() for _ in range(3)] == nxt and nxt[0][3] == 5
    F = copy.deepcopy(D)
    assert F.draw() == D.draw() and F.kernels is D.kernels
    # a user bank leaves the generator at its seed
    U = Degradation(3, kernels=np.full((2, 3, 3), 1.0 / 9.0), noise=(0, 0), speckle=(0, 0), seed=9)
    r9 = random.Random(9)
    assert U.draw() == (r9.randrange(2), r9.uniform(0, 0), r9.uniform(0, 0), 0) and len(U) == 2 and U.ksize == 3


def test_constructor_refuses_bad_arguments():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.degrade import Degradation
    ok3 = np.full((1, 3, 3), 1.0 / 9.0)
    nan = ok3.copy()
    nan[0, 0, 0] = float("nan")
    for kw in (dict(scale=5), dict(scale=1), dict(scale=3, kernels=np.full((1, 2, 2), 0.25)), dict(scale=2, kernels=ok3),
               dict(scale=3, kernels=np.full((1, 23, 23), 1.0 / 529)), dict(scale=2, kernels=np.full((1, 22, 22), 1.0 / 484)),
               dict(scale=3, kernels=nan), dict(scale=3, kernels=ok3 * (1 + 1e-11)), dict(scale=3, kernels=np.zeros((3, 3))),
               dict(scale=3, kernels=np.zeros((1, 3, 5))), dict(scale=3, ksize=4), dict(scale=2, ksize=3), dict(scale=4, ksize=22),
               dict(scale=2, bank=0), dict(scale=2, sigma=(0.0, 1.0)), dict(scale=2, sigma=(2.0, 1.0)), dict(scale=2, noise=(-1.0, 1.0)),
               dict(scale=2, speckle=(0.0, float("inf"))), dict(scale=2, noise=3.0), dict(scale=2, iso_prob=1.5), dict(scale=2, seed=-1)):
        with pytest.raises(M2TError):
            Degradation(**kw)
    assert Degradation(3, kernels=ok3 * (1 + 1e-13)).ksize == 3


def _cfg(**kw):
    base = {"scale": 4, "patch_size": 64, "batch_size": 2, "epochs": 1, "lr": 1e-4, "eta_min": 1e-6, "log_every": 1, "test_every": 1,
            "training_dataset": "folder", "train_hr_path": "somewhere"}
    base.update(kw)
    return base


def test_resolve_config_accepts_the_key_and_names_an_unknown_sub_key():
    from m2trans_amd import train as T
    from m2trans_amd._lib import M2TError
    assert "degradation" not in T.resolve_config(_cfg())["data"]
    r = T.resolve_config(_cfg(degradation={"bank": 16, "noise": [0, 5], "gray_noise": False}))
    assert r["data"]["degradation"] == {"bank": 16, "noise": [0, 5], "gray_noise": False}
    with pytest.raises(M2TError, match="blurr"):
        T.resolve_config(_cfg(degradation={"bank": 16, "blurr": 1}))
    with pytest.raises(M2TError, match="mapping"):
        T.resolve_config(_cfg(degradation=True))
    with pytest.raises(M2TError, match="data_add_noise"):
        T.resolve_config(_cfg(data_add_noise=True, degradation={}))
    from m2trans_amd.degrade import from_config
    D = from_config(4, {"bank": 4, "noise": [0, 5], "sigma": [0.5, 1.0], "seed": 7})
    assert len(D) == 4 and D.noise == (0.0, 5.0) and D.seed == 7 and D.ksize == 8 and from_config(4, None) is None


# ------------------------------------------------------------------------------------------------------------- host emulation
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++"), shutil.which("g++"))
                if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("degrade") / "degrade_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "tests", "emulate_hip"), "-I", os.path.join(ROOT, "m2trans_amd", "csrc"),
                    os.path.join(ROOT, "tests", "degrade_emulate.cpp"), "-o", exe, "-lpthread"], check=True, capture_output=True)
    return exe


def _emulate(exe, tmp_path, mode, hr, w, s, ly, lx, lh, lw, flags, gray, noise_id, seed, sa, ss):
    H, W, _ = hr.shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("11i", mode, H, W, s, w.shape[0], ly, lx, lh, lw, flags, int(gray)) + struct.pack("2Q", noise_id, seed)
                + struct.pack("2d", sa, ss) + np.ascontiguousarray(w, dtype=np.float64).tobytes() + np.ascontiguousarray(hr).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.uint8).reshape(lh, lw, 3)


def _kernels(s, K):
    return R.bank(s, M=3, K=K, seed=11)[0]


PATCH_CASES = [(s, K, corner, flags, lev, gray)
               for s in (2, 3, 4) for K in ((2 - s % 2), (21 if s % 2 else 20)) for corner in (0, 1)
               for flags, lev, gray in ((0, (0.0, 0.0), True), (3, (6.0, 0.0), True), (5, (0.0, 0.2), False), (6, (6.0, 0.2), True),
                                        (7, (6.0, 0.2), False))]


@pytest.mark.parametrize("s,K,corner,flags,lev,gray", PATCH_CASES,
                         ids=[f"x{s}-K{K}-{'far' if c else 'origin'}-f{f}-a{l[0]:g}-s{l[1]:g}-{'gray' if g else 'rgb'}" for s, K, c, f, l, g in PATCH_CASES])
def test_kernel_text_emulated_on_the_host_equals_the_restatement_patches(emulator, tmp_path, s, K, corner, flags, lev, gray):
    """csrc/m2t_degrade_tile.h on host threads under ASan / UBSan: the patches of the GPU test (HR 36 x 40, 36 x 39 at x3, lp = 8, both
    corners, so that the reflection is hit on all four sides with the largest K), every byte."""
    H, W, lp = 36, 39 if s == 3 else 40, 8
    hr = np.random.RandomState(s * 100 + K).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    w = _kernels(s, K)[1]
    ly, lx = (H // s - lp, W // s - lp) if corner else (0, 0)
    nid, seed = (1 << 40) + 5, (7 << 32) + 33
    got = _emulate(emulator, tmp_path, 0, hr, w, s, ly, lx, lp, lp, flags, gray, nid, seed, *lev)
    want, _ = R.patch_u8(hr, w, s, lp, lx, ly, flags, lev[0], lev[1], gray, nid, seed)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("s", [2, 4])
def test_kernel_text_emulated_multi_fold(emulator, tmp_path, s):
    """An image narrower than the kernel: HR 8 x 12, K = 20, lp = 2 -- the fold is applied more than once."""
    hr = np.random.RandomState(s).randint(0, 256, size=(8, 12, 3)).astype(np.uint8)
    w = _kernels(s, 20)[2]
    for ly, lx in ((0, 0), (8 // s - 2, 12 // s - 2)):
        got = _emulate(emulator, tmp_path, 0, hr, w, s, ly, lx, 2, 2, 4, True, 3, 33, 5.0, 0.1)
        want, _ = R.patch_u8(hr, w, s, 2, lx, ly, 4, 5.0, 0.1, True, 3, 33)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("s,lh,lw,extra", [(2, 13, 19, (1, 0)), (3, 33, 17, (2, 1)), (4, 13, 19, (0, 3)), (3, 13, 19, (0, 0))],
                         ids=["x2-13x19", "x3-33x17", "x4-13x19", "x3-13x19"])
def test_kernel_text_emulated_whole_image(emulator, tmp_path, s, lh, lw, extra):
    """Whole images whose LR size is no tile multiple, non-square, HR not a multiple of the scale: every byte."""
    hr = np.random.RandomState(lh + s).randint(0, 256, size=(lh * s + extra[0], lw * s + extra[1], 3)).astype(np.uint8)
    w = _kernels(s, 7 if s == 3 else 8)[0]
    for gray in (True, False):
        got = _emulate(emulator, tmp_path, 1, hr, w, s, 0, 0, lh, lw, 0, gray, 1 << 63, 33, 4.0, 0.15)
        want = R.image_u8(hr, w, s, 4.0, 0.15, gray, 1 << 63, 33)
        assert np.array_equal(got, want), int((got != want).sum())
