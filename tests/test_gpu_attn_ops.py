"""-m gpu: the operator gate of the window attention.  m2t_window_attention_fwd / _bwd (bf16: k_attn_c16.hip at C = 16, k_attn_res.hip
at C = 64 / 256, halo_gather and rel_reduce of k_attn.hip; fp32: the chunked kernels of k_attn.hip) against the fp64 reference of
tests/attn_ref.py, whole tensor and per pixel class: bf16 within 3x the bf16 error budget (the CPU emulation of the kernels' own
rounding points), fp32 within 2e-5 (forward) / 5e-5 (backward) of own norm.  tests/test_attn_reference_cpu.py shows on the same
cells that this gate rejects eight one-line faults.

Geometries (B, h, w) -> windows:
    (1,  8,  8)   1   36 of the 100 keys are phantom; three idle waves in the C = 16 workgroup
    (1,  8, 16)   2   h < w
    (1, 16,  8)   2   h > w
    (3,  8, 24)   9   odd B; nwin % 4 = 1
    (1, 24, 24)   9   an interior window (a full ring of real halo keys); 4-covered pixels
    (2, 16, 24)  12   the case of tests/test_gpu_ops.py
    (1, 40, 56)  35   nwin % 4 = 3; rel_reduce with 2 windows per split and a short last split; the model's padded geometry
    (2, 32, 72)  72   3 windows per split
x value regimes randn / kzero / grid (attn_ref.make_inputs) x two seeds.  -s prints every cell's table."""
import pytest
import torch

from tests import attn_ref as A
from tests.gpu_util import nchw_to_nhwc, nhwc_to_nchw

pytestmark = pytest.mark.gpu

GUARD = 4096                 # bytes on either side of the backward scratch (a multiple of the 256-byte alignment the regions assume)
GUARD_BYTE = 0xA5
WORST = {}                   # (C, dt, tensor) -> (ratio, error, budget or tolerance, cell, class)


@pytest.fixture(scope="module")
def lib():
    from m2trans_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib


def _poisoned(shape, dtype):
    """0xFF bytes: NaN as bf16 and as fp32.  A kernel that leaves an element unwritten, or reads scratch it has not written, shows."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def _run_hip(lib, inp, dt):
    """forward and backward through the C ABI -> {tensor: float32 NCHW / [10][C/2] on the CPU}."""
    L = lib.load()
    code, tdt = (lib.F32, torch.float32) if dt == "fp32" else (lib.BF16, torch.bfloat16)
    B, Cc, h, w = inp["q"].shape
    st = lib.stream_ptr()
    qkv = nchw_to_nhwc(torch.cat((inp["q"], inp["k"], inp["v"]), dim=1).cuda()).to(tdt)
    gout = nchw_to_nhwc(inp["gout"].cuda()).to(tdt)
    assert torch.equal(nhwc_to_nchw(qkv.float()).cpu(), torch.cat((inp["q"], inp["k"], inp["v"]), dim=1)), "inputs are pre-rounded"
    rh, rw = inp["rel_h"].reshape(-1).cuda(), inp["rel_w"].reshape(-1).cuda()
    out = _poisoned((B, h, w, Cc), tdt)
    lib.check(L.m2t_window_attention_fwd(code, lib.ptr(qkv), lib.ptr(rh), lib.ptr(rw), lib.ptr(out), B, h, w, Cc, st),
              "m2t_window_attention_fwd")
    gq = _poisoned((B, h, w, 3 * Cc), tdt)
    grh, grw = _poisoned((10 * Cc // 2,), torch.float32), _poisoned((10 * Cc // 2,), torch.float32)
    nb = int(L.m2t_window_attention_bwd_scratch_bytes(code, B, h, w, Cc))
    buf = torch.empty(nb + 2 * GUARD, dtype=torch.uint8, device="cuda")
    buf.fill_(0xFF)
    buf[:GUARD].fill_(GUARD_BYTE)
    buf[GUARD + nb:].fill_(GUARD_BYTE)
    scratch = buf[GUARD:GUARD + nb]
    assert scratch.data_ptr() % 256 == 0
    lib.check(L.m2t_window_attention_bwd(code, lib.ptr(qkv), lib.ptr(rh), lib.ptr(rw), lib.ptr(gout), lib.ptr(gq), lib.ptr(grh),
                                         lib.ptr(grw), lib.ptr(scratch), B, h, w, Cc, st), "m2t_window_attention_bwd")
    torch.cuda.synchronize()
    # m2t_window_attention_bwd_scratch_bytes is exact: nothing is written outside the bytes it asks for (read-back of the bands)
    assert bool((buf[:GUARD] == GUARD_BYTE).all()), "the backward wrote in front of its scratch"
    assert bool((buf[GUARD + nb:] == GUARD_BYTE).all()), "the backward wrote behind the bytes m2t_window_attention_bwd_scratch_bytes asks for"
    g = nhwc_to_nchw(gq.float()).cpu()
    got = {"out": nhwc_to_nchw(out.float()).cpu(), "dq": g[:, :Cc], "dk": g[:, Cc:2 * Cc], "dv": g[:, 2 * Cc:],
           "drel_h": grh.cpu().view(10, Cc // 2), "drel_w": grw.cpu().view(10, Cc // 2)}
    for t, x in got.items():
        assert bool(torch.isfinite(x).all()), f"{t}: {int((~torch.isfinite(x)).sum())} elements not written (poison survives) or not finite"
    return got


@pytest.mark.parametrize("regime", A.REGIMES)
@pytest.mark.parametrize("geo", A.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("Cc", A.CHANNELS)
def test_window_attention_gate(lib, Cc, dt, geo, regime):
    failures = []
    for seed in A.SEEDS:
        cell = f"C{Cc} {dt} {'x'.join(map(str, geo))} {regime} seed {seed}"
        inp = A.make_inputs(Cc, *geo, regime, seed, dt)
        ref = A.reference(inp)
        got = _run_hip(lib, inp, dt)
        if dt == "bf16":
            bad, table = A.gate_bf16(got, ref, A.budget(inp, ref, Cc))
            print(f"\n  {cell}: error, bf16 budget, error / budget (gate {A.MARGIN:g})\n" + A.format_table(table))
            score = {k: (q, e, b) for k, (e, b, q) in table.items()}
        else:
            bad, table = A.gate_fp32(got, ref, A.reference(inp, torch.float32))
            print(f"\n  {cell}: error, tolerance, error / the float32 oracle's own error\n" + A.format_table(table, "x oracle32"))
            score = {k: (e / tol, e, tol) for k, (e, tol, _) in table.items()}
        for (t, c), (q, e, b) in score.items():
            if q > WORST.get((Cc, dt, t), (-1.0,))[0]:
                WORST[(Cc, dt, t)] = (q, e, b, cell, c)
        failures += [f"{cell}: {m}" for m in bad]
    assert not failures, "\n".join(failures)


def test_zz_worst_ratio_report():
    """Not a check: prints (with -s) the worst ratio per (C, dtype, tensor) of the cells run in this session and where it occurred
    -- bf16: error / budget; fp32: error / tolerance."""
    for (Cc, dt, t), (q, e, b, cell, c) in sorted(WORST.items()):
        print(f"  worst C{Cc:<3d} {dt} {t:7s} ratio {q:6.3f}  (error {e:.3e} / {b:.3e})  at {cell} [{c}]")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("Cc,h,w,why", [(16, 12, 16, "h % 8"), (64, 16, 20, "w % 8"), (32, 16, 16, "C"), (128, 8, 8, "C")])
def test_argument_errors_launch_nothing(lib, dt, Cc, h, w, why):
    """h % 8 != 0, w % 8 != 0 and C outside {16, 64, 256} are early returns of the dispatch: M2T_ERR_ARG, a message, and no launch --
    every output and the scratch keep their fill pattern.  (Buffers are sized for the dimensions rounded UP, never under-sized.)"""
    L = lib.load()
    code, tdt = (lib.F32, torch.float32) if dt == "fp32" else (lib.BF16, torch.bfloat16)
    B, hp, wp, Cp = 1, (h + 7) // 8 * 8, (w + 7) // 8 * 8, max(Cc, 64)
    st = lib.stream_ptr()
    qkv = torch.zeros(B, hp, wp, 3 * Cp, device="cuda", dtype=tdt)
    gout = torch.zeros(B, hp, wp, Cp, device="cuda", dtype=tdt)
    rh, rw = torch.zeros(10 * Cp // 2, device="cuda"), torch.zeros(10 * Cp // 2, device="cuda")

    def pattern(n):
        return torch.full((n,), GUARD_BYTE, dtype=torch.uint8, device="cuda")

    es = 4 if dt == "fp32" else 2
    out, gq = pattern(B * hp * wp * Cp * es), pattern(B * hp * wp * 3 * Cp * es)
    grh, grw = pattern(10 * Cp // 2 * 4), pattern(10 * Cp // 2 * 4)
    scratch = pattern(int(L.m2t_window_attention_bwd_scratch_bytes(code, B, hp, wp, 256)))
    rc = L.m2t_window_attention_fwd(code, lib.ptr(qkv), lib.ptr(rh), lib.ptr(rw), lib.ptr(out), B, h, w, Cc, st)
    assert rc == -2, (why, rc)                                           # M2T_ERR_ARG (include/m2t.h)
    assert L.m2t_last_error_string(), "no message"
    msg_f = L.m2t_last_error_string().decode()
    rc = L.m2t_window_attention_bwd(code, lib.ptr(qkv), lib.ptr(rh), lib.ptr(rw), lib.ptr(gout), lib.ptr(gq), lib.ptr(grh), lib.ptr(grw),
                                    lib.ptr(scratch), B, h, w, Cc, st)
    assert rc == -2, (why, rc)
    msg_b = L.m2t_last_error_string().decode()
    for msg in (msg_f, msg_b):
        assert ("multiples of 8" in msg) if why != "C" else ("16, 64 or 256" in msg), msg
    torch.cuda.synchronize()
    for name, t in (("out", out), ("gqkv", gq), ("grel_h", grh), ("grel_w", grw), ("scratch", scratch)):
        assert bool((t == GUARD_BYTE).all()), f"{name} was written although the call returned M2T_ERR_ARG"
    with pytest.raises(lib.M2TError):
        lib.check(rc, "m2t_window_attention_bwd")
