"""CPU test (no GPU): the stage reference of the text-tower gate (tests/text_ref.py) is the oracle, and the gate it feeds
(tests/test_gpu_text_stages.py) can see the faults a kernel of this tower would make.

  * composition: the fp64 stages chained = oracle.text_oracle.bert_hidden_states / encode_text evaluated in fp64, within 1e-12
    relative, on all eight cases of the gate -- `allmasked` pins the no-attended-key rule (uniform 1 / len) to the oracle;
  * discrimination: each emulated fault of text_ref.BUGS moves the stage metric, at the stage where the fault lives and on the
    teacher-forced inputs the GPU gate uses, by at least 5 x the fp32 bound on at least one case;
  * the bf16 emulation rounds where the code rounds: every stored tensor is bf16-representable, and the emulated attention stage
    sits at the bf16 store error (1.65e-3 whole-tensor, 2.2e-3 on the worst row), so one dropped key among >= 100 is about AT the
    bf16 budget, not safely above it -- it is at `short` -- which is why the fp32 run of the same templated kernel carries that check.
"""
import pytest
import torch

from oracle import text_oracle as T
from tests import text_ref as R


@pytest.fixture(scope="module")
def params():
    return R.make_params()


@pytest.fixture(scope="module")
def clean(params):
    """{case: (ids, mask, emb, hidden states)} of the fp64 stages, computed once"""
    out = {}
    for name in R.CASES:
        ids, mask = R.case(name)
        emb, hs = R.encode(ids, mask, params)
        out[name] = (ids, mask, emb, hs)
    return out


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name", R.CASES)
def test_fp64_stages_compose_to_the_oracle(name, params, clean):
    ids, mask, emb, hs = clean[name]
    p64 = R.F64View(params)
    want_hs = T.bert_hidden_states(ids.long(), mask.long(), p64)
    want = T.encode_text(ids.long(), mask.long(), p64)
    assert want.dtype == torch.float64 and all(h.dtype == torch.float64 for h in want_hs)
    assert len(hs) == len(want_hs) == 13
    for l in range(13):
        assert torch.isfinite(want_hs[l]).all()
        assert _rel(hs[l], want_hs[l]) < 1e-12, (l, _rel(hs[l], want_hs[l]))
        assert R.row_err(hs[l], want_hs[l]) < 1e-12, (l, R.row_err(hs[l], want_hs[l]))
    assert _rel(emb, want) < 1e-12


def test_cases_are_what_the_gate_says(clean):
    ids, mask = clean["max"][:2]
    assert 0 in ids and R.VOCAB - 1 in ids and mask[0, -3:].sum() == 0 and mask.sum() == 125
    assert clean["half+"][1][1, 64:].sum() == 0 and clean["half+"][1][0].all()
    m = clean["edge64"][1]
    assert m[1, :2].sum() == 0 and m[1, 10:13].sum() == 0 and m[1].sum() == 59 and m[0].all()
    assert clean["allmasked"][1][2].sum() == 0 and clean["allmasked"][1].sum() == 21
    for name, (n, ln) in R.SHAPES.items():
        assert tuple(clean[name][0].shape) == (n, ln)
    assert [c for c in R.CASES if c in R.BF16_CASES] == list(R.BF16_CASES)


def _bug_metric(bug, name, params, clean):
    """the stage metric of the GPU gate between the faulty and the clean stage, on the clean (teacher-forced) stage input"""
    ids, mask, _, hs = clean[name]
    b = (bug,)
    stage = R.BUG_STAGE[bug]
    if stage == "embed":
        return R.row_err(R.embed(ids, params, bugs=b), hs[0])
    if stage == "qkv":
        return R.row_err(R.qkv(hs[11], params, 11, bugs=b), R.qkv(hs[11], params, 11))
    if stage == "attn":
        q = R.qkv(hs[11], params, 11)
        return R.row_err(R.attn(q, mask, bugs=b), R.attn(q, mask))
    assert stage == "pool"
    return R.row_err(R.pool(hs[1], hs[2], hs[12], mask, b), R.pool(hs[1], hs[2], hs[12]))


@pytest.mark.parametrize("bug", R.BUGS)
def test_the_gate_discriminates(bug, params, clean):
    worst = {name: _bug_metric(bug, name, params, clean) for name in R.CASES}
    print(bug, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) >= 5 * R.FP32_TOL, worst


def test_one_dropped_key_after_a_whole_layer_is_above_the_fp32_bound(params, clean):
    """the smallest fault of the list, at the coarsest check that sees it (hs[12] from hs[11]), on the longest case"""
    ids, mask, _, hs = clean["max"]
    e = R.row_err(R.layer(hs[11], mask, params, 11, bugs=("last_key",)), hs[12])
    print(f"last_key, max, whole layer: {e:.2e}")
    assert e >= 5 * R.FP32_TOL, e


def test_bf16_emulation_rounds_at_the_stores(params, clean):
    ids, mask, _, hs = clean["half+"]
    x = R.bf16(hs[11])
    q = R.qkv(x, params, 11, emu=True)
    ao = R.attn(q, mask, emu=True)
    xm = R.attn_out(ao, x, params, 11, emu=True)
    mh = R.fc1(xm, params, 11, emu=True)
    y = R.fc2(mh, xm, params, 11, emu=True)
    for t in (R.embed(ids, params, emu=True), q, ao, xm, mh, y, R.ln_out(y, params, 11, emu=True)):
        assert torch.equal(R.bf16(t), t)
    ref = R.attn(q, mask)
    whole = _rel(ao, ref)
    print(f"bf16 attention emulation: whole-tensor {whole:.2e}, per-row {R.row_err(ao, ref):.2e}")
    assert 5e-4 < whole < 3e-3                              # a bf16 store: 2^-9 / sqrt(3) ~ 1.1e-3 .. 2^-8 / sqrt(3)
    # one dropped key among the 100 of sequence 0 is NOT safely above 3 x that budget (whole-tensor it is below it, per row it is
    # about at it: printed, not asserted); at `short`, where a key weighs 1 / 5, it is far above
    drop = R.row_err(R.attn(q, mask, bugs=("last_key",))[0], ref[0])
    print(f"one key of 100 dropped: per-row {drop:.2e} against a bf16 budget of {R.MARGIN * R.row_err(ao[0], ref[0]):.2e}")
    assert drop < 5 * R.MARGIN * R.row_err(ao[0], ref[0])
    ids, mask, _, hs = clean["short"]
    q = R.qkv(R.bf16(hs[11]), params, 11, emu=True)
    ref = R.attn(q, mask)
    assert R.row_err(R.attn(q, mask, bugs=("last_key",)), ref) > 5 * R.MARGIN * R.row_err(R.attn(q, mask, emu=True), ref)


def test_text_handle_answers_the_region_queries_and_the_null_argument_error_needs_no_device():
    """the text handle answers ws: / wsn: for every region the gate reads, and the null-argument error of m2t_text_encode_ex needs no
    device."""
    import ctypes as C
    from m2trans_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.m2t_text_create(C.byref(h), 4, 128, 0) == 0
    q = lambda k: lib.m2t_text_query(h, k.encode())
    offs = [q("ws:" + k) for k in ("packed", "fbias", "ids", "mask", "X", "XM", "Y", "QKV", "AO", "MH", "pooled")]
    assert offs == sorted(offs) and offs[0] == 0 and all(o % 256 == 0 for o in offs)
    assert [q("wsn:" + k) for k in ("X", "XM", "QKV", "MH", "pooled")] == [512 * 768, 512 * 768, 512 * 2304, 512 * 3072, 4 * 768]
    assert q("ws:nope") == -1 and q("packed:encoder.layer.0.qkv") == -1
    assert lib.m2t_text_encode_ex(h, None, None, 1, 1, None, None, None, None) == -2
    lib.m2t_text_destroy(h)
