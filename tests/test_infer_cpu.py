"""CPU tests (no GPU) of the inference end (include/m2t_infer.h, m2trans_amd/infer.py): the ninth header against its signature table
and the library's symbols, the torch restatement the GPU tests compare the kernels with (tests/infer_ref.py) against itself, the
command line's parsing and name mapping, and the new keyword of metrics.evaluate."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from tests import infer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_argument_errors_need_no_device():
    """Every M2T_ERR_ARG of the header is decided on the host before any launch, so it is reported without a device too."""
    from m2trans_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(4096)                                     # never dereferenced: the checks come first
    assert lib.m2t_dihedral_pack(None, 3, 8, 8, one, one, None) == -2
    assert lib.m2t_dihedral_pack(one, 0, 8, 8, one, one, None) == -2
    assert lib.m2t_dihedral_merge(one, one, 65536, 8, 8, one, None, None) == -2
    assert lib.m2t_dihedral_merge(one, one, 3, 8, 16385, one, None, None) == -2
    assert lib.m2t_tensor_to_image_u8(one, 2, 8, 8, 1.0, one, None) == -2
    assert lib.m2t_tensor_to_image_u8(one, 3, 8, 8, 0.0, one, None) == -2
    assert b"m2t_tensor_to_image_u8" in lib.m2t_last_error_string()


# ------------------------------------------------------------------------------------------------------------- the restatement
def _distinct(*shape):
    n = 1
    for s in shape:
        n *= s
    return torch.arange(n, dtype=torch.float32).reshape(shape) * 0.37 + 1.0


def test_the_eight_views_are_eight_different_arrays_and_each_inverse_undoes_its_view():
    x = _distinct(2, 3, 5, 7)                                  # non-square, all entries distinct
    assert x.unique().numel() == x.numel()
    views = [R.view(x, k) for k in range(8)]
    for k, y in enumerate(views):
        assert tuple(y.shape) == ((2, 3, 5, 7) if k < 4 else (2, 3, 7, 5))
        assert torch.equal(R.inverse(y, k), x), k
    for k in range(8):
        for m in range(k + 1, 8):
            assert views[k].shape != views[m].shape or not torch.equal(views[k], views[m]), (k, m)
    # the definition, element by element, on one plane
    H, W = 5, 7
    p = x[1, 2]
    for k in range(8):
        t, v, h = k >> 2, (k >> 1) & 1, k & 1
        y = torch.empty(H, W)
        for i in range(H):
            for j in range(W):
                y[i, j] = p[H - 1 - i if v else i, W - 1 - j if h else j]
        assert torch.equal(views[k][1, 2], y.t() if t else y), k
    # a flip taken for the inverse of a transposed view is not one: the order "un-transpose, then the same flips" matters
    z = views[5]                                               # t = 1, h = 1
    wrong = z.flip(-1).transpose(-1, -2)
    assert not torch.equal(wrong, x)


def test_pack_places_view_k_of_image_n_at_batch_index_k_mod_4_times_n_plus_n():
    x = _distinct(2, 3, 4, 6)
    a, b = R.pack(x)
    assert tuple(a.shape) == (8, 3, 4, 6) and tuple(b.shape) == (8, 3, 6, 4)
    for k in range(8):
        for n in range(2):
            got = (a if k < 4 else b)[(k % 4) * 2 + n]
            assert torch.equal(got, R.view(x[n], k)), (k, n)
    U = R.unpack(a, b)
    assert len(U) == 8 and all(torch.equal(u, x) for u in U)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_the_restated_ensemble_of_the_equivariant_stub_is_the_stub_itself(s):
    g = torch.Generator().manual_seed(5 + s)
    for shape in ((2, 3, 5, 7), (1, 3, 6, 6)):
        x = torch.randn(*shape, generator=g)
        up = R.nearest_up(s)
        mean, var, spread = R.ensemble(up, x)
        assert tuple(mean.shape) == (shape[0], 3, shape[2] * s, shape[3] * s)
        assert torch.equal(mean, up(x))
        assert torch.equal(var, torch.zeros_like(var)) and torch.equal(spread, torch.zeros_like(spread))
    # a stub that is NOT equivariant (it shifts the image) has a positive spread: the zero above is not vacuous
    mean, var, _ = R.ensemble(lambda t: R.nearest_up(s)(t.roll(1, dims=-1)), x)
    assert float(var.max()) > 0.0


def test_export_rounds_like_save_image():
    # rgb_range 255: s = 1, every product exact -- below 0, a value that rounds down, exact .5 ties (up), above the range, NaN
    v = torch.tensor([-1.0, 0.0, 0.49, 0.5, 1.0, 1.5, 127.5, 254.5, 255.0, 300.0, float("nan")]).view(1, 1, -1)
    assert R.export_u8(v, 255.0).view(-1).tolist() == [0, 0, 0, 1, 1, 2, 128, 255, 255, 255, 0]
    assert R.export_u8(torch.tensor([-0.2, 0.0, 1.0, 1.7, float("nan")]).view(1, 1, -1)).view(-1).tolist() == [0, 0, 255, 255, 0]
    rgb = torch.rand(3, 4, 5, generator=torch.Generator().manual_seed(1))
    out = R.export_u8(rgb)
    assert tuple(out.shape) == (4, 5, 3) and out.dtype == torch.uint8
    assert torch.equal(out, (rgb * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0))


# ------------------------------------------------------------------------------------------------------------- CLI, evaluate
def test_cli_parses_its_arguments_and_maps_names():
    from m2trans_amd import infer
    base = ["--config", "c.yml", "--model_path", "m.pt", "--input", "in", "--output", "out"]
    a = infer.parse_args(base)
    assert (a.config, a.model_path, a.input, a.output) == ("c.yml", "m.pt", "in", "out")
    assert a.self_ensemble is False and a.spread is None and a.compute_dtype is None
    a = infer.parse_args(base + ["--self_ensemble", "--spread", "sp", "--compute_dtype", "bf16"])
    assert a.self_ensemble is True and a.spread == "sp" and a.compute_dtype == "bf16"
    for bad in (base[2:], base + ["--compute_dtype", "fp16"], base + ["--spread", "sp"]):      # --spread needs --self_ensemble
        with pytest.raises(SystemExit):
            infer.parse_args(bad)
    ns = infer.model_namespace({"scale": 4, "n_blocks": 8, "rgb_range": 1.0, "compute_dtype": "fp32"}, "bf16")
    assert ns.scale == 4 and ns.compute_dtype == "bf16"
    assert infer.model_namespace({"scale": 2}).scale == 2 and not hasattr(infer.model_namespace({"scale": 2}), "compute_dtype")
    assert infer.output_name("0001.jpg") == "0001.png" and infer.output_name("a/b/img.x4.PNG") == "img.x4.png"
    assert infer.output_names(["b.jpg", "a.png"]) == ["b.png", "a.png"]
    with pytest.raises(infer.M2TError):
        infer.output_names(["a.jpg", "a.png"])


def test_image_names_lists_the_images_of_a_folder_sorted(tmp_path):
    from m2trans_amd import infer
    for n in ("b.PNG", "a.jpg", "notes.txt", "c.bmp"):
        (tmp_path / n).write_bytes(b"")
    assert infer.image_names(tmp_path) == ["a.jpg", "b.PNG", "c.bmp"]


def test_evaluate_takes_self_ensemble_as_its_last_keyword():
    from m2trans_amd.metrics import evaluate
    params = list(inspect.signature(evaluate).parameters.values())
    assert params[-1].name == "self_ensemble" and params[-1].default is False
    assert [p.name for p in params[:-1]] == ["model", "pairs", "scale", "rgb_range", "with_gmsd", "with_fsim", "with_vif"]


def test_host_tensors_are_refused():
    from m2trans_amd import infer
    x = torch.zeros(1, 3, 4, 4)
    for call in (lambda: infer.dihedral_pack(x), lambda: infer.dihedral_merge(x.repeat(4, 1, 1, 1), x.repeat(4, 1, 1, 1)),
                 lambda: infer.self_ensemble(R.nearest_up(2), x), lambda: infer.to_uint8(x)):
        with pytest.raises(infer.M2TError):
            call()
