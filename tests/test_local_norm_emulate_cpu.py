"""CPU test (no GPU): the per-thread text of k_local_norm.hip (csrc/m2t_local_norm_tile.h) run on the host by the stand-alone program
tests/local_norm_emulate.cpp, built with -fsanitize=address,undefined and run as a program, against the restatement of
tests/local_norm_ref.py under the gate of the GPU stage test, at that test's planes and window sides.  X, the fp64 sums and Xn are heap
blocks of exactly their sizes there, so an index outside a region ends the program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import local_norm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tuple((2, 64, 64, T) for T in (24, 33, 64, 200)) + ((1, 64, 96, 80), (1, 32, 160, 8), (1, 160, 32, 150))


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    # (clang: the header uses ext_vector_type and __bf16, as the device build does)
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"), shutil.which("clang++")) if c and os.path.exists(c)), None)
    assert cxx, "no clang-based C++ compiler found"
    exe = str(tmp_path_factory.mktemp("local_norm") / "local_norm_emulate")
    subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "tests", "emulate_hip"), "-I", os.path.join(ROOT, "m2trans_amd", "csrc"),
                    os.path.join(ROOT, "tests", "local_norm_emulate.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def _emulate(exe, tmp_path, dtype, x, T):
    """x: (B, 64, H, W) -> the program's Xn, same shape."""
    B, _, H, W = x.shape
    p64 = np.ascontiguousarray(x.reshape(B, 4, 16, H, W).transpose(1, 0, 3, 4, 2), dtype=np.float32)      # [4][B][H][W][16]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("5i", 1 if dtype == "bf16" else 0, B, H, W, T) + p64.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.float32).reshape(4, B, H, W, 16)
    return out.transpose(1, 0, 4, 2, 3).reshape(B, 64, H, W)


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
@pytest.mark.parametrize("B,H,W,T", CASES)
def test_the_kernel_text_on_the_host_passes_the_gate(emulator, tmp_path, B, H, W, T, dtype):
    x = R.stage_plane(B, 64, H, W, seed=T, dtype=dtype)
    xn = _emulate(emulator, tmp_path, dtype, x, T)
    nbad, worst = R.gate(xn, x, T, dtype)
    assert nbad == 0, (nbad, worst)
    # the text differs from the definition "to the letter" only in the order of its fp64 sums: almost every element has its very bits
    same = float(np.mean(xn == R.local_norm(x, T, dtype)))
    assert same > 0.999, same


def test_black_is_exact_zero_and_a_constant_plane_too(emulator, tmp_path):
    for value in (0.0, 0.3359375):                                   # (the second: representable in bf16)
        x = np.full((1, 64, 64, 64), value)
        xn = _emulate(emulator, tmp_path, "bf16", x, 24)
        assert not xn.any() and not np.signbit(xn).any()
