"""-m gpu: stage gate of the MedCLIP text tower (csrc/m2t_text.hip): every kernel against fp64, len up to 128.

One handle per dtype (max_seqs 4, max_len 128); the cases of tests/text_ref.py run on it in order, long ones first, so a short
call follows a long one on the same workspace.  Before every encode the activation part of the workspace (everything after the
packed weights and fused biases), `hidden_out` and `emb` are filled with 0xFF bytes (NaN in fp32 and bf16).

Every reference is TEACHER-FORCED: the fp64 stage of tests/text_ref.py applied to the DEVICE's own stage input, so an error is
charged to the stage that makes it.  The metric is the largest per-row relative L2 error over the n * len token rows.
  1. hs[0]            <- embed(ids)
  2. hs[l], l = 1..12 <- the whole layer on the device hs[l - 1]
  3. the last layer's chain out of the workspace (ws: / wsn:): QKV <- hs[11]; AO <- device QKV, mask; XM <- device AO, hs[11];
     MH <- device XM; Y <- device MH, XM; X <- device Y; X is bit-equal to hs[12]
  4. pooled <- device hs[1], hs[2], hs[12]; emb <- device pooled; | ||emb|| - 1 | < 1e-4
  5. every byte beyond the rows the call owns, in every region and in hidden_out, is still 0xFF; every owned element is finite
  6. the same call on a workspace filled with another byte gives the same bits in emb and hs

BOUNDS.  fp32: 2e-5 per stage (text_ref.FP32_TOL: the project's gate of an fp32 forward against fp64).  bf16: the device error
against fp64 is at most 3 x the error of the CPU emulation of that stage (text_ref, emu=True: bf16 round trips where the code
stores bf16) against fp64, on the same teacher-forced input.  `pooled` and `emb` are fp32 on a bf16 handle too and have no bf16
rounding point (their emulation error is zero), so they take the fp32 bound there.

WHAT BF16 CANNOT SEE.  The emulated attention stage sits at the error of one bf16 store (1.65e-3 whole-tensor, about 2.2e-3 on
the worst row), so 3 x that budget is about what ONE dropped key does among >= 100 attended keys (7.6e-3 on the worst row at
len 128, tests/test_text_ref_cpu.py): the bf16 run cannot be relied on to see it.  It does at `short`, where a key weighs 1 / 5
(5.5e-2).  The fp32 run of the same templated kernel, at 2e-5, carries that check at every length.
"""
import ctypes as C

import pytest
import torch

from tests import text_ref as R

pytestmark = pytest.mark.gpu

ACT = ("ids", "mask", "X", "XM", "Y", "QKV", "AO", "MH", "pooled")
WIDTH = {"ids": 1, "mask": 1, "X": R.H, "XM": R.H, "Y": R.H, "QKV": 3 * R.H, "AO": R.H, "MH": R.FF, "pooled": R.H}
GUARD = 4096


@pytest.fixture(scope="module")
def params():
    return R.make_params()


@pytest.fixture(scope="module")
def encoders(params):
    made = {}

    def get(dtype):
        if dtype not in made:
            from m2trans_amd import _lib
            from m2trans_amd.losses import TextEncoder
            enc = TextEncoder(4, 128, _lib.F32 if dtype == "fp32" else _lib.BF16, torch.device("cuda"))
            enc.load(params)
            made[dtype] = enc
        return made[dtype]
    return get


class Run:
    """one m2t_text_encode_ex on a workspace whose activation part, hidden_out and emb were filled with `fill` bytes"""

    def __init__(self, enc, dtype, ids, mask, fill):
        from m2trans_amd import _lib
        self.tdt, self.es = (torch.float32, 4) if dtype == "fp32" else (torch.bfloat16, 2)
        self.n, self.len = ids.shape
        self.rows = self.n * self.len
        self.off = {k: enc.query("ws:" + k) for k in ACT}
        self.cnt = {k: enc.query("wsn:" + k) for k in ACT}
        self.esz = {k: (4 if k in ("ids", "mask", "pooled") else self.es) for k in ACT}
        self.start = self.off["ids"]
        # the activation regions lie behind the packed weights and the fused biases, which must survive the fill
        assert enc.query("ws:packed") + enc.query("wsn:packed") * self.es <= enc.query("ws:fbias")
        assert enc.query("ws:fbias") + enc.query("wsn:fbias") * 4 <= self.start == min(self.off.values())
        enc.workspace[self.start:].fill_(fill)
        self.hs_bytes = 13 * self.rows * R.H * self.es
        hidden = torch.full((self.hs_bytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
        emb = torch.full((self.n * 512 * 4 + GUARD,), fill, dtype=torch.uint8, device="cuda")
        ip, mp = C.cast(ids.data_ptr(), C.POINTER(C.c_int)), C.cast(mask.data_ptr(), C.POINTER(C.c_int))
        _lib.check(_lib.load().m2t_text_encode_ex(enc.handle, ip, mp, self.n, self.len, _lib.ptr(emb), _lib.ptr(enc.workspace),
                                                  _lib.stream_ptr(), _lib.ptr(hidden)), "m2t_text_encode_ex")
        torch.cuda.synchronize()
        self.ws = enc.workspace[self.start:].cpu()
        self.hidden, self.emb_raw = hidden.cpu(), emb.cpu()
        self.hs = self.hidden[:self.hs_bytes].view(self.tdt).reshape(13, self.n, self.len, R.H)
        self.emb = self.emb_raw[:self.n * 512 * 4].view(torch.float32).reshape(self.n, 512)

    def owned(self, k):
        return (self.n if k == "pooled" else self.rows) * WIDTH[k] * self.esz[k]

    def region(self, k):
        o = self.off[k] - self.start
        t = self.ws[o:o + self.owned(k)].view(torch.int32 if k in ("ids", "mask") else torch.float32 if k == "pooled" else self.tdt)
        return t.reshape(self.n, R.H) if k == "pooled" else t.reshape(self.n, self.len, WIDTH[k]).squeeze(-1) if WIDTH[k] == 1 \
            else t.reshape(self.n, self.len, WIDTH[k])

    def untouched(self, fill):
        """names of the buffers in which a byte the call does not own lost the fill value"""
        keep = torch.ones(self.ws.numel(), dtype=torch.bool)
        for k in ACT:
            assert self.owned(k) <= self.cnt[k] * self.esz[k]
            keep[self.off[k] - self.start:self.off[k] - self.start + self.owned(k)] = False
        bad = []
        spoiled = torch.nonzero(keep & (self.ws != fill)).flatten()
        if len(spoiled):
            at = int(spoiled[0]) + self.start
            bad.append("workspace byte %d (region %s)" % (at, max((k for k in ACT if self.off[k] <= at), key=lambda k: self.off[k])))
        if not bool((self.hidden[self.hs_bytes:] == fill).all()):
            bad.append("hidden_out")
        if not bool((self.emb_raw[self.n * 512 * 4:] == fill).all()):
            bad.append("emb")
        return bad


CASE_IDS = [("fp32", c) for c in R.CASES] + [("bf16", c) for c in R.BF16_CASES]
_RUNS = {}                                      # (dtype, case) -> Run of the stage test, for the layer test of the same case


class Table:
    """(stage, error, budget) rows of one case; fp32: FP32_TOL; bf16: MARGIN x the emulation's error, FP32_TOL where nothing rounds"""

    def __init__(self, dtype, name):
        self.dtype, self.name, self.emu, self.rows = dtype, name, dtype == "bf16", []

    def check(self, tag, got, want, emulated=None):
        budget = R.FP32_TOL if emulated is None else R.MARGIN * R.row_err(emulated, want)
        self.rows.append((tag, R.row_err(got, want) if bool(torch.isfinite(got.float()).all()) else float("inf"), budget))

    def stage(self, tag, got, fn, *args):
        self.check(tag, got, fn(*args), fn(*args, emu=True) if self.emu else None)

    def over(self):
        for tag, err, budget in self.rows:
            print(f"{self.dtype:5s} {self.name:9s} {tag:9s} err {err:.3e} budget {budget:.3e}{'' if err <= budget else '   <-- OVER'}")
        return [(t, e, b) for t, e, b in self.rows if not e <= b]


@pytest.mark.parametrize("dtype,name", CASE_IDS, ids=[f"{d}-{c}" for d, c in CASE_IDS])
def test_text_stages_against_fp64(dtype, name, params, encoders):
    """checks 1 and 3 - 6 of the module docstring"""
    enc = encoders(dtype)
    ids, mask = R.case(name)
    run = _RUNS[dtype, name] = Run(enc, dtype, ids, mask, 0xFF)
    p, t = params, Table(dtype, name)
    hs = [h.to(torch.float64) for h in run.hs]
    dev = {k: run.region(k) for k in ACT}
    # 5. owned elements are finite (a NaN of the 0xFF fill read as data would show here and in the stages), the rest is untouched
    assert torch.equal(dev["ids"], ids) and torch.equal(dev["mask"], mask)
    not_finite = [k for k in ACT[2:] if not bool(torch.isfinite(dev[k].float()).all())]
    not_finite += ["hs"] if not bool(torch.isfinite(run.hs.float()).all()) else []
    not_finite += ["emb"] if not bool(torch.isfinite(run.emb).all()) else []
    spoiled = run.untouched(0xFF)
    # 1.
    t.stage("embed", hs[0], R.embed, ids, p)
    # 3. the last layer, stage by stage
    L = R.LAYERS - 1
    t.stage("qkv", dev["QKV"], R.qkv, hs[11], p, L)
    t.stage("attn", dev["AO"], R.attn, dev["QKV"], mask)
    t.stage("attn_out", dev["XM"], R.attn_out, dev["AO"], hs[11], p, L)
    t.stage("fc1", dev["MH"], R.fc1, dev["XM"], p, L)
    t.stage("fc2", dev["Y"], R.fc2, dev["MH"], dev["XM"], p, L)
    t.stage("ln_out", dev["X"], R.ln_out, dev["Y"], p, L)
    # 4. fp32 stages on either handle
    t.check("pool", dev["pooled"], R.pool(hs[1], hs[2], hs[12]))
    t.check("head", run.emb, R.head(dev["pooled"], p))
    over = t.over()
    norm_off = float((run.emb.norm(dim=1) - 1).abs().max())
    # 6. stale workspace: other bytes underneath, same bits out
    again = Run(enc, dtype, ids, mask, 0x5A)
    assert not not_finite, not_finite
    assert not spoiled, spoiled
    assert not again.untouched(0x5A)
    assert not over, over
    assert torch.equal(run.region("X").view(torch.uint8), run.hs[12].contiguous().view(torch.uint8)), "X is not hs[12]"
    assert norm_off < 1e-4, norm_off
    assert torch.equal(again.emb.view(torch.int32), run.emb.view(torch.int32)), "emb depends on stale workspace bytes"
    assert torch.equal(again.hidden[:run.hs_bytes], run.hidden[:run.hs_bytes]), "hidden states depend on stale workspace bytes"


@pytest.mark.parametrize("dtype,name", CASE_IDS, ids=[f"{d}-{c}" for d, c in CASE_IDS])
def test_text_layers_against_fp64(dtype, name, params, encoders):
    """check 2: hs[l] against the whole layer applied to the device hs[l - 1], l = 1..12 (the hidden states of the stage test's run).

    fp32, layer 1 is where this check found something: with the closed-form weights the first layer's scores reach +-303 (24 in
    the last layer), the softmax turns an ABSOLUTE score error into a relative one, and the 5.8e-7 of the fp32-accumulating q|k|v
    GEMM came out of the layer as 2.13e-5 (`max`), 2.70e-5 (`edge64`), 2.16e-5 (`allmasked`): over the bound, with every single
    stage inside it.  The fp32 handle now forms q|k|v with fp64 accumulation (text_qkv_f64acc_kernel): layer 1 measures at most
    6.6e-6, the qkv stage 2.7e-8.  DESIGN.md has the measurements."""
    if (dtype, name) not in _RUNS:
        ids, mask = R.case(name)
        _RUNS[dtype, name] = Run(encoders(dtype), dtype, ids, mask, 0xFF)
    run, mask, t = _RUNS[dtype, name], R.case(name)[1], Table(dtype, name)
    hs = [h.to(torch.float64) for h in run.hs]
    for l in range(1, 13):
        t.stage(f"layer{l}", hs[l], R.layer, hs[l - 1], mask, params, l - 1)
    over = t.over()
    assert not over, over


def test_encode_with_hidden_states_is_the_plain_encode(params, encoders):
    """TextEncoder.encode(..., hidden_states=True): same embedding bits as the plain call, hs of the documented shape and type"""
    enc = encoders("fp32")
    ids, mask = R.case("base")
    emb = enc.encode(ids, mask)
    emb2, hs = enc.encode(ids, mask, hidden_states=True)
    assert hs.shape == (13, 3, 19, R.H) and hs.dtype == torch.float32
    assert torch.equal(emb, emb2)
    assert R.row_err(hs[0].cpu(), R.embed(ids, params)) < R.FP32_TOL
