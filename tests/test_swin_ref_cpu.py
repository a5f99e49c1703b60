"""CPU test (no GPU): the stage reference of the image-tower gate (tests/swin_ref.py) is the oracle, its hand-written VJPs are
autograd's, and the gate it feeds (tests/test_gpu_swin_stages.py) can see the faults a kernel of this tower would make.

  * composition: the fp64 stages chained = oracle.swin_oracle.encode_image in fp64, within 1e-12, and the gather permutation
    is the oracle's concat order exactly;
  * VJPs: every hand-written backward stage (emu=False) = torch.autograd of the fp64 forward stage, within 1e-10;
  * parameter sets: on the closed-form weights AND on the `peaked` set (query / key weights of stage s x PEAK[s]), torch float32 on the CPU
    against fp64, block by block and teacher-forced, stays within FP32_TOL / 4 -- so the fp32 bound of the GPU gate is
    reachable by a correct fp32 kernel on both; each PEAK[s] is the largest of swin_ref.PEAK_CANDIDATES that keeps this;
  * discrimination: each emulated fault of swin_ref.BUGS moves the stage metric (or, where stated, the branch metric), at the
    stage where the fault lives and on teacher-forced inputs, by at least 5 x the fp32 bound on at least one case; the ratio to
    the bf16 budget (MARGIN x the emulation's error) is printed per fault;
  * the bf16 emulation rounds where the code stores bf16.
"""
import pytest
import torch

from oracle import swin_oracle as S
from tests import swin_ref as R

SHIFTED = [(0, 1), (1, 1), (2, 1)]
PLAIN = [(0, 0), (3, 1)]


@pytest.fixture(scope="module")
def params():
    return {k: R.make_params(k) for k in ("closed", "peaked")}


@pytest.fixture(scope="module")
def clean(params):
    """{(set, case): (crops, emb, hidden states)} of the fp64 stages, computed once"""
    out = {}
    for kind, name in (("closed", "three"), ("closed", "one"), ("peaked", "three")):
        crops = R.crops_of(name)
        emb, hs = R.Ref(params[kind]).encode(crops)
        out[kind, name] = (crops, emb, hs)
    return out


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("kind,name", [("closed", "three"), ("peaked", "three"), ("closed", "one")])
def test_fp64_stages_compose_to_the_oracle(kind, name, params, clean):
    crops, emb, hs = clean[kind, name]
    p64 = {k: v.to(torch.float64) for k, v in params[kind].items()}
    cap = {}
    pooled = S.swin_pooled(crops.to(torch.float64), p64, cap)
    want = S.encode_image(crops.to(torch.float64), p64)
    assert want.dtype == torch.float64
    assert _rel(emb, want) < 1e-12
    assert _rel(hs["hnf"].mean(1), pooled) < 1e-12
    for s in range(3):
        assert R.row_err(R.scatter_perm(hs[f"m{s}"]), cap[f"stage{s}"]) < 1e-12, s
    assert R.row_err(hs["xf"], cap["stage3"]) < 1e-12


def test_gather_is_the_oracles_concat_order_and_scatter_inverts_it():
    x = torch.arange(2 * 28 * 28 * 8, dtype=torch.float64).reshape(2, 28 * 28, 8)
    v = x.view(2, 28, 28, 8)
    want = torch.cat([v[:, r::2, c::2, :] for c in range(2) for r in range(2)], dim=-1).view(2, -1, 32)     # oracle.patch_merge
    assert torch.equal(R.gather_perm(x), want)
    assert torch.equal(R.scatter_perm(R.gather_perm(x)), x)
    assert not torch.equal(R.gather_perm(x, bugs=("merge_order",)), want)


def test_cases_are_what_the_gate_says():
    assert [c for c in R.CASES if c in R.BF16_CASES] == list(R.BF16_CASES)
    for name, n in (("full", 4), ("three", 3), ("pair_edge", 3), ("one", 1)):
        a, b, crops = R.case(name)
        n_src = a.shape[0] + (0 if b is None else b.shape[0])
        assert len(crops) == n and tuple(R.crops_of(name).shape) == (n, 3, 224, 224)
        assert all(0 <= i < n_src and y + 224 <= a.shape[2] and x + 224 <= a.shape[3] for i, y, x in crops)
    a, b, crops = R.case("pair_edge")
    assert a.shape[0] == 1 and b.shape[0] == 2 and a.shape[3] % 2 == 1 and crops[0] == (2, 230 - 224, 241 - 224)
    # the ragged last tile of the 64-row fused MLP at stage 1: 784 n rows
    assert (784 * 1) % 64 == 16 and (784 * 3) % 64 == 48 and (3136 * 3) % 64 == 0


def _vjp_check(fwd, inputs, got_fn, tag):
    """autograd of fwd at inputs[0] under a fixed cotangent against the hand-written VJP"""
    x = inputs[0].clone().requires_grad_(True)
    y = fwd(x)
    g = torch.sin(torch.arange(y.numel(), dtype=torch.float64) * 0.37 + 0.2).reshape(y.shape)
    want, = torch.autograd.grad(y, x, g)
    got = got_fn(g)
    err = _rel(got, want)
    print(f"vjp {tag}: {err:.2e}")
    assert err < 1e-10, (tag, err)


def test_hand_written_vjps_are_autograd(params, clean):
    crops, emb, hs = clean["peaked", "three"]
    r = R.Ref(params["peaked"])
    one = {k: v[:1] for k, v in hs.items()}
    _vjp_check(r.head, [one["hnf"]], lambda g: r.head_bwd(one["hnf"], g), "head")
    _vjp_check(r.final_ln, [one["xf"]], lambda g: r.ln_bwd(one["xf"], g, "layernorm.weight"), "final_ln")
    for s, j in SHIFTED + PLAIN:
        k = f"s{s}b{j}."
        xin, qkv, xmid = one[k + "xin"], one[k + "qkv"], one[k + "xmid"]
        _vjp_check(lambda t: r.attn(t, s, j), [qkv], lambda g: r.attn_bwd(qkv, g, s, j), k + "attn")
        # the half-blocks as functions of the residual stream: the VJP takes the stashed qkv / gelu' as the device does
        _vjp_check(lambda t: r.attn_half(r.qkv(t, s, j), t, s, j), [xin], lambda g: r.attn_half_bwd(xin, qkv, g, s, j), k + "attn_half")
        _vjp_check(lambda t: r.mlp_half(t, s, j), [xmid], lambda g: r.mlp_half_bwd(xmid, r.gder(xmid, s, j), g, s, j), k + "mlp_half")
    for s in range(3):
        x = R.scatter_perm(one[f"m{s}"])
        _vjp_check(lambda t: r.merge(r.gather(t), s), [x], lambda g: r.merge_bwd(one[f"m{s}"], g, s), f"merge{s}")
    c1 = crops[:1].to(torch.float64)
    _vjp_check(lambda t: r.embed_ln(r.patch(t)), [c1], lambda g: r.embed_bwd(r.embed_ln_bwd(one["e0"], g)), "embed")


def _blockwise_fp32(p, hs):
    """worst row error of torch float32 against fp64 over the 12 blocks, each on the fp64 block input"""
    r64, r32 = R.Ref(p), R.Ref(p, dt=torch.float32)
    worst = {}
    for s, j in R.BLOCKS:
        x = hs[f"s{s}b{j}.xin"]
        worst[s, j] = R.row_err(r32.block(x, s, j), r64.block(x, s, j))
    return worst


@pytest.mark.parametrize("kind", ["closed", "peaked"])
def test_fp32_bound_is_reachable_on_both_parameter_sets(kind, params, clean):
    worst = _blockwise_fp32(params[kind], clean[kind, "three"][2])
    print(kind, {f"{s}.{j}": f"{v:.1e}" for (s, j), v in worst.items()})
    assert max(worst.values()) <= R.FP32_TOL / 4, worst


def test_fp32_stand_in_in_the_kernels_contraction_order(params, clean):
    """the branch metric of mlp_half under the two float32 contraction orders (blocked BLAS sums / one chain over K in steps of 4,
    as the fp32 gemm_nt epilogue kernels sum): the GPU gate's fp32 branch budget is MARGIN x the larger; both are far below what
    the seeded gelu_tanh fault does (5.4e-4)"""
    p, hs = params["closed"], clean["closed", "three"][2]
    r64, r32, rc = R.Ref(p), R.Ref(p, dt=torch.float32), R.Ref(p, dt=torch.float32, chain=True)
    for s, j in [(0, 0), (1, 1), (2, 5), (3, 0), (3, 1)]:
        x = hs[f"s{s}b{j}.xmid"].float()
        want = r64.mlp_half(x, s, j)
        blocked, chained = R.branch_err(r32.mlp_half(x, s, j), want, x), R.branch_err(rc.mlp_half(x, s, j), want, x)
        print(f"s{s}b{j} mlp_half branch, float32: blocked {blocked:.2e}  chained {chained:.2e}")
        assert R.row_err(rc.mlp_half(x, s, j), r32.mlp_half(x, s, j)) < R.FP32_TOL / 4          # the same function
        assert R.MARGIN * max(blocked, chained) < 5.4e-4 / 10


@pytest.mark.parametrize("s", [0, 1, 2])
def test_peak_factor_is_the_largest_candidate_that_keeps_the_condition(s, params):
    """the next candidate at stage s (earlier stages as chosen, later ones unscaled, as they were when it was picked) breaks it"""
    nxt = R.PEAK_CANDIDATES[R.PEAK_CANDIDATES.index(R.PEAK[s]) + 1]
    p = R.peaked(params["closed"], tuple(R.PEAK[:s]) + (nxt,) + (1.0,) * (3 - s))
    r64, r32 = R.Ref(p), R.Ref(p, dt=torch.float32)
    x = r64.embed_ln(r64.patch(R.crops_of("three")))
    for t in range(s):
        for j in range(R.DEPTHS[t]):
            x = r64.block(x, t, j)
        x = r64.merge(r64.gather(x), t)
    worst = 0.0
    for j in range(R.DEPTHS[s]):
        want = r64.block(x, s, j)
        worst = max(worst, R.row_err(r32.block(x, s, j), want))
        x = want
    print(f"stage {s}: factor {nxt} gives {worst:.2e}")
    assert worst > R.FP32_TOL / 4 and R.PEAK[3] == R.PEAK_CANDIDATES[-1]


def test_peaked_attention_is_selective(params, clean):
    """what the second set is for: with the closed-form weights attention is nearly uniform (a dropped or mis-masked key shows
    least); the peaked set's median largest probability per query is above 1 / 2 at every stage"""
    for kind, least in (("closed", 0.0), ("peaked", 0.5)):
        r, hs = R.Ref(params[kind]), clean[kind, "three"][2]
        out = {}
        for s, j in [(0, 0), (1, 1), (2, 1), (3, 1)]:
            q, k, v = r._split(hs[f"s{s}b{j}.qkv"], s, j)
            out[s, j] = float(torch.softmax(r._scores(q, k, s, j), -1).amax(-1).median())
        print(kind, "median of the largest probability per query:", {f"{s}.{j}": f"{v:.3f}" for (s, j), v in out.items()})
        assert min(out.values()) >= least, out


def _bug_metric(bug, kind, name, params, clean):
    """-> (stage metric, branch metric or None, bf16 budget of that metric): faulty against clean stage on the clean input"""
    p, hs = params[kind], clean[kind, name][2]
    ok, bad, emu = R.Ref(p), R.Ref(p, bugs=(bug,)), R.Ref(p, emu=True)
    stage = R.BUG_STAGE[bug]
    best = (0.0, None, 0.0)

    def keep(full, branch, budget):
        nonlocal best
        if (branch or full) / max(budget, 1e-300) >= (best[1] or best[0]) / max(best[2], 1e-300):
            best = (full, branch, budget)
    if stage == "attn_half":
        for s, j in (SHIFTED + PLAIN if bug in ("last_key", "rel_swap") else SHIFTED):
            q, x = hs[f"s{s}b{j}.qkv"], hs[f"s{s}b{j}.xin"]
            want = ok.attn_half(q, x, s, j)
            keep(R.row_err(bad.attn_half(q, x, s, j), want), R.branch_err(bad.attn_half(q, x, s, j), want, x),
                 R.MARGIN * R.branch_err(emu.attn_half(R.bf16(q), R.bf16(x), s, j), ok.attn_half(R.bf16(q), R.bf16(x), s, j), R.bf16(x)))
    elif stage == "mlp_half":
        for s, j in ([(1, 0), (1, 1)] if bug == "mlp_tail" else [(0, 0), (1, 1), (2, 3), (3, 1)]):
            x = hs[f"s{s}b{j}.xmid"]
            want = ok.mlp_half(x, s, j)
            keep(R.row_err(bad.mlp_half(x, s, j), want), R.branch_err(bad.mlp_half(x, s, j), want, x),
                 R.MARGIN * R.branch_err(emu.mlp_half(R.bf16(x), s, j), ok.mlp_half(R.bf16(x), s, j), R.bf16(x)))
    elif stage == "gather":
        x = R.scatter_perm(hs["m1"])
        keep(R.row_err(bad.gather(x), ok.gather(x)), None, 0.0)
    elif stage == "qkv":
        x = hs["s3b1.xin"]
        keep(R.row_err(bad.qkv(x, 3, 1), ok.qkv(x, 3, 1)), None, R.MARGIN * R.row_err(emu.qkv(R.bf16(x), 3, 1), ok.qkv(R.bf16(x), 3, 1)))
    elif stage == "gder":
        x = hs["s2b2.xmid"]
        keep(R.row_err(bad.gder(x, 2, 2), ok.gder(x, 2, 2)), None, R.MARGIN * R.row_err(emu.gder(R.bf16(x), 2, 2), ok.gder(R.bf16(x), 2, 2)))
    else:
        assert stage == "ln_bwd"
        g = torch.sin(torch.arange(512.0, dtype=torch.float64) * 0.7)[None].expand(hs["hnf"].shape[0], -1)
        gc = ok.head_bwd(hs["hnf"], g)
        want = ok.ln_bwd(hs["xf"], gc, "layernorm.weight")
        keep(R.row_err(bad.ln_bwd(hs["xf"], gc, "layernorm.weight"), want), None,
             R.MARGIN * R.row_err(emu.ln_bwd(R.bf16(hs["xf"]), emu.head_bwd(R.bf16(hs["hnf"]), g), "layernorm.weight"),
                                  ok.ln_bwd(R.bf16(hs["xf"]), emu.head_bwd(R.bf16(hs["hnf"]), g), "layernorm.weight")))
    return best


# faults the stage metric alone does not carry safely to 5 x FP32_TOL = 1e-4 (gelu_tanh: 9.9e-5 .. 1.1e-4 in the stage metric,
# 5.4e-4 in the branch metric): the GPU gate bounds the BRANCH metric of their stage (mlp_half)
BRANCH_ONLY = ("gelu_tanh",)


@pytest.mark.parametrize("bug", R.BUGS)
def test_the_gate_discriminates(bug, params, clean):
    rows = {(kind, name): _bug_metric(bug, kind, name, params, clean) for kind, name in clean}
    for (kind, name), (full, branch, budget) in rows.items():
        seen = branch if branch is not None else full
        print(f"{bug:12s} {kind:6s} {name:5s} stage {full:.2e}" + (f" branch {branch:.2e}" if branch is not None else "")
              + (f"  bf16 budget {budget:.2e} ratio {seen / budget:.1f}" if budget > 0 else "  (exact stage: no bf16 budget)"))
    worst_full = max(v[0] for v in rows.values())
    worst_branch = max((v[1] for v in rows.values() if v[1] is not None), default=0.0)
    if bug in BRANCH_ONLY:
        assert worst_branch >= 5 * R.FP32_TOL, rows
    else:
        assert worst_full >= 5 * R.FP32_TOL, rows


def test_bf16_emulation_rounds_at_the_stores(params, clean):
    crops, emb, hs = clean["closed", "three"]
    e = R.Ref(params["closed"], emu=True)
    s, j = 1, 1
    x = R.bf16(hs["s1b1.xin"])
    q = e.qkv(x, s, j)
    xm = e.attn_half(q, x, s, j)
    out = e.mlp_half(xm, s, j)
    g = torch.cos(torch.arange(x.numel(), dtype=torch.float64)).reshape(x.shape)
    stored = (e.patch(crops), e.embed_ln(hs["e0"]), q, e.attn(q, s, j), xm, e.mlp_hidden(xm, s, j), out, e.gder(xm, s, j), e.merge(hs["m1"], 1),
              e.final_ln(hs["xf"]), e.head_bwd(hs["hnf"], emb))
    for t in stored:
        assert torch.equal(R.bf16(t), t)
    # fp32 on the device, no rounding point: the head, the residual-stream gradient, the gather
    assert not torch.equal(R.bf16(e.head(hs["hnf"])), e.head(hs["hnf"]))
    assert not torch.equal(R.bf16(e.mlp_half_bwd(xm, e.gder(xm, s, j), g, s, j)), e.mlp_half_bwd(xm, e.gder(xm, s, j), g, s, j))
    assert torch.equal(e.gather(out), R.gather_perm(out))
    # the probabilities are rounded before P.V: the attention stage sits at about two bf16 stores, not one
    ref = R.Ref(params["closed"]).attn(q, s, j)
    whole = _rel(e.attn(q, s, j), ref)
    print(f"bf16 attention emulation: whole-tensor {whole:.2e}, per-row {R.row_err(e.attn(q, s, j), ref):.2e}")
    assert 5e-4 < whole < 4e-3


def test_swin_handle_answers_the_region_queries_and_the_wrappers_layouts_are_the_headers():
    """the handle answers wsn: / gws: / gwsn:; the wrappers' layouts are the header's (needs no device)"""
    import ctypes as C
    from m2trans_amd import _lib
    from m2trans_amd.losses import SwinEncoder
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.m2t_swin_create(C.byref(h), 4, 1) == 0
    q = lambda k: lib.m2t_swin_query(h, k.encode())
    offs = [q("ws:" + k) for k in ("packed", "fbias", "crops", "A0", "X", "Hn", "QKV", "AO", "MH", "emb")]
    assert offs == sorted(offs) and offs[0] == 0 and all(o % 256 == 0 for o in offs)
    tok = 4 * 3136 * 96
    assert [q("wsn:" + k) for k in ("A0", "X", "Hn", "QKV", "AO", "MH", "emb")] == [tok // 2, tok, tok, 3 * tok, tok, 4 * tok, 4 * 512]
    assert q("ws:nope") == -1 and q("wsn:nope") == -1
    assert q("gws:gR") == -1 and q("gwsn:gR") == -1                       # before any m2t_swin_grad_workspace_bytes
    total = lib.m2t_swin_grad_workspace_bytes(h, 2)
    g = 2 * 3136 * 96
    assert q("gwsn:gR") == g and q("gwsn:s1b0.qkv") == 3 * g // 2 and q("gwsn:s2b5.gder") == g and q("gwsn:xf") == 2 * 49 * 768
    assert 0 < q("gws:gR") < q("gws:e0") < q("gws:s0b0.xin") < q("gws:hnf") < q("gws:MD") < total and q("gws:nope") == -1
    assert q("gwsn:MD") == 4 * 3136 * 96 * 4
    # the layouts of the wrappers are the header's totals
    lay = SwinEncoder.hidden_layout(1)
    assert lay[-1][1] + 49 * 768 == 8053248 and [k for k, _, _ in lay][:4] == ["e0", "s0b0.xin", "s0b0.qkv", "s0b0.xmid"]
    tap = SwinEncoder.tap_layout(1)
    assert tap[-1][1] + 3136 * 96 == 3725568 and len(tap) == 1 + 24 + 3 + 1
    assert lib.m2t_swin_encode_ex(h, None, 1, None, 0, 224, 224, None, 1, None, None, None, None) == -2
    assert lib.m2t_swin_backward_ex(h, None, 1, None, None, None, None, None) == -2
    lib.m2t_swin_destroy(h)
