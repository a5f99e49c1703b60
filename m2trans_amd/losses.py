"""Drop-in for the reference's ``losses.SemanticLoss`` (losses.py:18-81) on MI355X.

Same constructor and call surface -- ``SemanticLoss(criterion='l1', N_patches=3)``,
``loss_clip(sr[i], hr[i], caption) -> Tensor[1]`` (train.py:78,205) -- but the MedCLIP image
tower (Swin-T 224 + Linear(768,512) + L2 norm) runs as hand-written gfx950 kernels behind the
C ABI (``m2t_swin_*``), and ``batch(sr, hr, captions)`` evaluates a whole batch with ONE encoder
launch sequence instead of the reference's B sequential B=1 calls, while drawing the patch
coordinates from the global torch CPU RNG in exactly the reference's order.

What the reference value really is (and what is reproduced): only the LAST patch's embeddings
survive the loop (losses.py:67-69), so for N_patches > 1 the value is
``|cos(E(sr_crop), T) - cos(E(hr_crop), T)| / N_patches`` on the last random 224x224 crop; the
bicubic 224x224 resize (losses.py:53-54) only matters for N_patches == 1.  Everything is
evaluated without gradient (losses.py:63): the term shifts the logged loss, not the update.

PARITY UNPINNED: the `medclip` package, its Swin/BERT checkpoints and tokenizer are not vendored
by the reference.  Weights are therefore injected (``load_state_dict`` with HF swin-tiny names,
4.24 or 5.x spelling, plus ``projection_head.weight``); text features are injected per caption
(``set_text_features``) or computed by the text tower built here (``load_text_encoder`` / ``load_medclip_state_dict``:
BERT-base forward + the MedCLIP head behind ``m2t_text_*``, with the reference's input_ids quirk of losses.py:65; the
tokenizer is a host callable) -- they are constants of the frozen text tower, cached per caption.  A caption with neither
RAISES (``synthetic_text=True`` opts into a deterministic hash stand-in for benchmarks).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import math
from typing import Dict, Iterable, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib
from ._lib import M2TError

_V5_TO_V4 = (
    ("attention.q_proj", "attention.self.query"), ("attention.k_proj", "attention.self.key"),
    ("attention.v_proj", "attention.self.value"), ("attention.o_proj", "attention.output.dense"),
    ("attention.relative_position_bias.relative_position_bias_table", "attention.self.relative_position_bias_table"),
    ("mlp.fc1", "intermediate.dense"), ("mlp.fc2", "output.dense"),
)


class _Tower(_lib.Handle):
    """A frozen tower behind ``m2t_<family>_*``: handle + parameter inventory + flat fp32 weights + workspace."""
    what = ""          # the tower in the "missing ... weights" message

    def __init__(self, dtype: int, device, *sizes: int):
        h = C.c_void_p()
        _lib.check(getattr(_lib.load(), f"m2t_{self.family}_create")(C.byref(h), *sizes, dtype), f"m2t_{self.family}_create")
        self.handle, self.dtype, self.device = h, dtype, device
        self.names, self.slots = self.inventory()
        self.flat = torch.zeros(self.query("num_params"), dtype=torch.float32, device=device)
        self.workspace = torch.empty(self.query("workspace_bytes"), dtype=torch.uint8, device=device)
        self.loaded = False

    def _store(self, k: str, v: torch.Tensor, short_ok: bool = False):
        """a state-dict tensor into its slot of ``flat`` (short_ok: one with fewer elements fills the front of the slot)"""
        o, n = self.slots[k]
        if v.numel() != n and not (short_ok and v.numel() < n):
            raise M2TError(f"shape mismatch for {k}: {tuple(v.shape)}")
        self.flat[o:o + v.numel()].copy_(v.reshape(-1).to(self.flat))

    def _load_weights(self, seen):
        """after the ``_store`` calls of a state dict: every tensor must have come, then the library packs them"""
        missing = [n for n in self.names if n not in seen]
        if missing:
            raise M2TError(f"missing {self.what} weights: {missing[:5]} ... ({len(missing)})")
        entry = f"m2t_{self.family}_load_weights"
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), entry)(self.handle, _lib.ptr(self.flat), _lib.ptr(self.workspace), _lib.stream_ptr()), entry)
        self.loaded = True


class SwinEncoder(_Tower):
    """m2t_swin handle + workspace + flat weights."""
    family, what = "swin", "Swin"

    def __init__(self, max_images: int, dtype: int, device):
        super().__init__(dtype, device, max_images)
        self.max_images = max_images
        self.grad_workspace = None         # allocated on the first encode_grad (differentiable SemanticLoss only)

    def load(self, state: Dict[str, torch.Tensor]):
        seen = set()
        for k, v in state.items():
            for a, b in _V5_TO_V4:
                k = k.replace(a, b)
            for prefix in ("vision_model.model.", "model.", "swin."):
                if k.startswith(prefix) and k[len(prefix):] in self.slots:
                    k = k[len(prefix):]
            if k in self.slots:
                self._store(k, v)
                seen.add(k)
        self._load_weights(seen)

    DEPTHS = (2, 2, 6, 2)

    @classmethod
    def hidden_layout(cls, n: int):
        """[(name, element offset, shape)] of ``hidden_out`` of m2t_swin_encode_ex for n crops (include/m2t_swin.h)"""
        out, off = [], 0

        def add(name, rows, width):
            nonlocal off
            out.append((name, off, (n, rows, width)))
            off += n * rows * width
        add("e0", 3136, 96)
        for s, depth in enumerate(cls.DEPTHS):
            t, c = 3136 >> (2 * s), 96 << s
            for j in range(depth):
                add(f"s{s}b{j}.xin", t, c)
                add(f"s{s}b{j}.qkv", t, 3 * c)
                add(f"s{s}b{j}.xmid", t, c)
            if s < 3:
                add(f"m{s}", t // 4, 4 * c)
        add("xf", 49, 768)
        add("hnf", 49, 768)
        return out

    @classmethod
    def tap_layout(cls, n_grad: int):
        """[(name, float offset, shape)] of ``grad_taps`` of m2t_swin_backward_ex for n_grad crops (include/m2t_swin.h)"""
        out, off = [], 0

        def add(name, rows, width):
            nonlocal off
            out.append((name, off, (n_grad, rows, width)))
            off += n_grad * rows * width
        add("xf", 49, 768)
        for s in (3, 2, 1, 0):
            t, c = 3136 >> (2 * s), 96 << s
            for j in reversed(range(cls.DEPTHS[s])):
                add(f"s{s}b{j}.xmid", t, c)
                add(f"s{s}b{j}.xin", t, c)
            if s > 0:
                add(f"s{s - 1}.out", 4 * t, c // 2)
        add("e0", 3136, 96)
        return out

    def encode(self, src: torch.Tensor, crops: Sequence[Sequence[int]], hidden_states: bool = False):
        """src [n_src,3,Hs,Ws] fp32 on the device; crops [(src index, row0, col0)] -> [n,512] unit-norm embeddings.
        hidden_states=True: -> (emb, {name: tensor [n, rows, width]} in the compute type, the names of ``hidden_layout``);
        the embedding is the plain call's, bit for bit (m2t_swin_encode_ex)."""
        if not self.loaded:
            raise M2TError("SwinEncoder: weights not loaded")
        src = src.contiguous().float()
        n = len(crops)
        arr = (C.c_int * (3 * n))(*[int(v) for c in crops for v in c])
        emb = torch.empty(n, 512, dtype=torch.float32, device=self.device)
        if hidden_states:
            lay = self.hidden_layout(n)
            total = lay[-1][1] + math.prod(lay[-1][2])
            hid = torch.empty(total, dtype=torch.float32 if self.dtype == _lib.F32 else torch.bfloat16, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().m2t_swin_encode_ex(self.handle, _lib.ptr(src), src.shape[0], None, 0, src.shape[2], src.shape[3], arr,
                                                          n, _lib.ptr(emb), _lib.ptr(self.workspace), _lib.stream_ptr(), _lib.ptr(hid)),
                           "m2t_swin_encode_ex")
            return emb, {k: hid[o:o + math.prod(shp)].view(shp) for k, o, shp in lay}
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().m2t_swin_encode(self.handle, _lib.ptr(src), src.shape[0], src.shape[2], src.shape[3], arr, n,
                                                   _lib.ptr(emb), _lib.ptr(self.workspace), _lib.stream_ptr()), "m2t_swin_encode")
        return emb

    def encode_pair(self, src_a: torch.Tensor, src_b: torch.Tensor, crops: Sequence[Sequence[int]]) -> torch.Tensor:
        """like ``encode`` with the sources in two tensors (index < len(src_a): src_a, else src_b): no concatenation"""
        if not self.loaded:
            raise M2TError("SwinEncoder: weights not loaded")
        src_a, src_b = src_a.contiguous().float(), src_b.contiguous().float()
        if tuple(src_a.shape[1:]) != tuple(src_b.shape[1:]):
            raise M2TError("SwinEncoder.encode_pair: the two source tensors must have the same image shape")
        n = len(crops)
        arr = (C.c_int * (3 * n))(*[int(v) for c in crops for v in c])
        emb = torch.empty(n, 512, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().m2t_swin_encode_pair(self.handle, _lib.ptr(src_a), src_a.shape[0], _lib.ptr(src_b), src_b.shape[0],
                                                        src_a.shape[2], src_a.shape[3], arr, n, _lib.ptr(emb), _lib.ptr(self.workspace),
                                                        _lib.stream_ptr()), "m2t_swin_encode_pair")
        return emb

    def encode_grad(self, src_a: torch.Tensor, src_b: Optional[torch.Tensor], crops: Sequence[Sequence[int]], n_grad: int) -> torch.Tensor:
        """``encode_pair`` that also keeps what ``backward`` needs for the first ``n_grad`` crops (src_b may be None)."""
        if not self.loaded:
            raise M2TError("SwinEncoder: weights not loaded")
        lib = _lib.load()
        if self.grad_workspace is None:
            self.grad_workspace = torch.empty(int(lib.m2t_swin_grad_workspace_bytes(self.handle, self.max_images // 2)),
                                              dtype=torch.uint8, device=self.device)
        if not 1 <= n_grad <= self.max_images // 2:
            raise M2TError(f"SwinEncoder.encode_grad: n_grad {n_grad} outside [1, {self.max_images // 2}]")
        src_a = src_a.contiguous().float()
        n_b = 0
        if src_b is not None:
            src_b = src_b.contiguous().float()
            n_b = src_b.shape[0]
        n = len(crops)
        arr = (C.c_int * (3 * n))(*[int(v) for c in crops for v in c])
        emb = torch.empty(n, 512, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.m2t_swin_encode_grad(self.handle, _lib.ptr(src_a), src_a.shape[0], _lib.ptr(src_b), n_b, src_a.shape[2],
                                                src_a.shape[3], arr, n, n_grad, _lib.ptr(emb), _lib.ptr(self.workspace),
                                                _lib.ptr(self.grad_workspace), _lib.stream_ptr()), "m2t_swin_encode_grad")
        return emb

    def backward(self, g_emb: torch.Tensor, n_grad: int, taps: bool = False):
        """vector-Jacobian product of the last ``encode_grad``: g_emb [n_grad,512] -> g_crops [n_grad,3,224,224] fp32.
        taps=True: -> (g_crops, {name: fp32 residual-stream gradient [n_grad, rows, width]}, the names of ``tap_layout``);
        g_crops is the plain call's, bit for bit (m2t_swin_backward_ex)."""
        g_emb = g_emb.contiguous().float()
        g = torch.empty(n_grad, 3, 224, 224, dtype=torch.float32, device=self.device)
        if taps:
            lay = self.tap_layout(n_grad)
            buf = torch.empty(lay[-1][1] + math.prod(lay[-1][2]), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().m2t_swin_backward_ex(self.handle, _lib.ptr(g_emb), n_grad, _lib.ptr(g), _lib.ptr(self.workspace),
                                                            _lib.ptr(self.grad_workspace), _lib.stream_ptr(), _lib.ptr(buf)),
                           "m2t_swin_backward_ex")
            return g, {k: buf[o:o + math.prod(shp)].view(shp) for k, o, shp in lay}
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().m2t_swin_backward(self.handle, _lib.ptr(g_emb), n_grad, _lib.ptr(g), _lib.ptr(self.workspace),
                                                     _lib.ptr(self.grad_workspace), _lib.stream_ptr()), "m2t_swin_backward")
        return g


class TextEncoder(_Tower):
    """m2t_text handle + workspace + flat weights: ``medmodel.encode_text`` (losses.py:65,74) = BERT-base -> mean of hidden
    states 1, 2, -1 -> Linear(768, 512) -> unit norm, as hand-written kernels behind ``m2t_text_*`` (csrc/m2t_text.hip)."""

    family, what = "text", "text-tower"

    def __init__(self, max_seqs: int, max_len: int, dtype: int, device):
        super().__init__(dtype, device, max_seqs, max_len)
        self.max_seqs, self.max_len = max_seqs, max_len

    def load(self, state: Dict[str, torch.Tensor]):
        """HF BertModel names (transformers 4.24), optionally behind the MedCLIP checkpoint's ``text_model.model.`` /
        ``text_model.`` prefixes (or ``bert.`` / ``model.``), plus ``projection_head.weight``; ``pooler.*``,
        ``embeddings.position_ids`` and anything else are ignored; a word-embedding table with fewer rows than the
        Bio_ClinicalBERT vocabulary fills the first rows."""
        seen = set()
        for k, v in state.items():
            for prefix in ("text_model.model.", "text_model.", "model.", "bert."):
                if k.startswith(prefix) and k[len(prefix):] in self.slots:
                    k = k[len(prefix):]
                    break
            if k not in self.slots:
                continue
            self._store(k, v, short_ok=k == "embeddings.word_embeddings.weight" and v.dim() == 2 and v.shape[1] == 768)
            seen.add(k)
        self._load_weights(seen)

    def encode(self, input_ids, attention_mask, hidden_states: bool = False):
        """input_ids, attention_mask: [n, len] integer arrays (host) -> [n,512] unit-norm embeddings on the device.
        ``hidden_states=True`` -> ``(emb, hs)``, hs [13, n, len, 768] in the handle's element type: BertModel's hidden_states."""
        if not self.loaded:
            raise M2TError("TextEncoder: weights not loaded")
        ids = torch.as_tensor(input_ids, dtype=torch.int32).reshape(-1, torch.as_tensor(input_ids).shape[-1]).contiguous().cpu()
        mask = torch.as_tensor(attention_mask, dtype=torch.int32).reshape(ids.shape).contiguous().cpu()
        n, ln = ids.shape
        emb = torch.empty(n, 512, dtype=torch.float32, device=self.device)
        ip, mp = C.cast(ids.data_ptr(), C.POINTER(C.c_int)), C.cast(mask.data_ptr(), C.POINTER(C.c_int))
        hs = None
        if hidden_states:
            hs = torch.empty(13, n, ln, 768, dtype=torch.float32 if self.dtype == _lib.F32 else torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().m2t_text_encode_ex(self.handle, ip, mp, n, ln, _lib.ptr(emb), _lib.ptr(self.workspace),
                                                      _lib.stream_ptr(), _lib.ptr(hs) if hidden_states else None),
                       "m2t_text_encode")
        return (emb, hs) if hidden_states else emb


def hash_text_feature(caption: str) -> torch.Tensor:
    """Deterministic stand-in for the frozen text tower (NOT the MedCLIP embedding)."""
    seed = int.from_bytes(hashlib.sha256(caption.encode("utf-8")).digest()[:8], "little") % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(512, generator=g)


class SemanticLoss(nn.Module):
    def __init__(self, criterion: str = "l1", N_patches: int = 3, device=None, compute_dtype: str = "fp32",
                 max_batch: int = 32, synthetic_text: bool = False, differentiable: bool = False):
        super().__init__()
        # differentiable=True (opt-in): batch() / __call__ return a tensor connected to `sr` (when sr.requires_grad), with the gradient
        # the paper's regulariser needs -- the reference's no_grad term (losses.py:63) taken out of no_grad.  The value, the RNG
        # consumption and the last-patch quirk are unchanged; the MedCLIP towers stay frozen (data gradient only).
        self.differentiable = bool(differentiable)
        # synthetic_text=True (benchmarks / tests with no MedCLIP weights): a caption without an injected text feature
        # gets a deterministic hash embedding.  The default is to RAISE: a silent stand-in behind a drop-in surface
        # would log a wrong regulariser value (the reference loads the real text tower itself, losses.py:22-23).
        self.synthetic_text = bool(synthetic_text)
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.N_patches = int(N_patches)
        self.compute_dtype = compute_dtype
        self.max_batch = int(max_batch)
        if self.differentiable and self.device.type != "cuda":
            raise M2TError("SemanticLoss(differentiable=True) needs a HIP device: the Swin-T data gradient has no CPU implementation")
        self._enc: Optional[SwinEncoder] = None
        self._state: Optional[Dict[str, torch.Tensor]] = None
        self._text: Dict[str, torch.Tensor] = {}
        self._text_dev = None
        self._tenc: Optional[TextEncoder] = None
        self._text_state: Optional[Dict[str, torch.Tensor]] = None
        self._by_count: Dict[int, torch.Tensor] = {}       # text feature per token count (see _text_feature)
        self.tokenizer = None                               # callable(caption) -> {'token_type_ids': [..], 'attention_mask': [..]}

    # ---- injected constants -----------------------------------------------------------------
    def load_image_encoder(self, state_dict: Dict[str, torch.Tensor]):
        """HF swin-tiny state dict (4.24 or 5.x names) + 'projection_head.weight' [512,768]."""
        self._state = {k: v.detach() for k, v in state_dict.items()}
        if self._enc is not None:
            self._enc.load(self._state)

    def load_text_encoder(self, state_dict: Dict[str, torch.Tensor], tokenizer=None):
        """The MedCLIP text tower: HF BertModel names (4.24) + 'projection_head.weight' [512,768] (see TextEncoder.load),
        and the tokenizer the reference builds with ``MedCLIPProcessor()`` (losses.py:25,64): any callable
        ``tokenizer(caption) -> mapping with 'token_type_ids' and 'attention_mask'`` (one sequence).  The tokenizer stays
        on the host; its vocabulary file ships with the checkpoint, not with this build."""
        self._text_state = {k: v.detach() for k, v in state_dict.items()}
        if tokenizer is not None:
            self.tokenizer = tokenizer
        self._tenc = None
        self._by_count.clear()

    def load_medclip_state_dict(self, state_dict: Dict[str, torch.Tensor], tokenizer=None):
        """A whole MedCLIPModel checkpoint (``vision_model.*`` / ``text_model.*`` / ``logit_scale``, the file
        pretrained/medclip-vit/readme.md:1-5 points at): both towers at once."""
        vis = {k[len("vision_model."):] if k.startswith("vision_model.projection_head") else k: v
               for k, v in state_dict.items() if k.startswith("vision_model.")}
        txt = {k: v for k, v in state_dict.items() if k.startswith("text_model.")}
        self.load_image_encoder(vis)
        self.load_text_encoder(txt, tokenizer)

    def _text_encoder(self) -> TextEncoder:
        if self._tenc is None:
            if self.device.type != "cuda":
                raise M2TError("SemanticLoss (MI355X build) needs a HIP device; there is no CPU fallback")
            code = _lib.F32 if self.compute_dtype in ("fp32", "float32") else _lib.BF16
            self._tenc = TextEncoder(1, 128, code, self.device)
            self._tenc.load(self._text_state)
        return self._tenc

    def set_text_features(self, table: Dict[str, torch.Tensor]):
        self._text.update({k: v.detach().float().reshape(512).cpu() for k, v in table.items()})
        self._text_dev = None

    def _encoder(self) -> SwinEncoder:
        if self.device.type != "cuda":
            raise M2TError("SemanticLoss (MI355X build) needs a HIP device; there is no CPU fallback")
        if self._enc is None:
            code = _lib.F32 if self.compute_dtype in ("fp32", "float32") else _lib.BF16
            self._enc = SwinEncoder(2 * self.max_batch, code, self.device)
            if self._state is None:
                raise M2TError("SemanticLoss: call load_image_encoder(state_dict) first (MedCLIP weights are not vendored)")
            self._enc.load(self._state)
        return self._enc

    def _text_feature(self, caption: str) -> torch.Tensor:
        t = self._text.get(caption)
        if t is not None:
            return t
        if self._text_state is not None and self.tokenizer is not None:
            # losses.py:64-65: tokenizer(text=[caption]) then encode_text(outputs['token_type_ids'], outputs['attention_mask'])
            # -- the token-type ids (zeros) travel in the input_ids slot, so the feature is a function of the token count
            tok = self.tokenizer(caption)
            ids = [int(v) for v in torch.as_tensor(tok["token_type_ids"]).reshape(-1).tolist()]
            mask = [int(v) for v in torch.as_tensor(tok["attention_mask"]).reshape(-1).tolist()]
            key = len(ids) if (not any(ids) and all(mask)) else None
            t = self._by_count.get(key) if key is not None else None
            if t is None:
                t = self._text_encoder().encode([ids], [mask])[0].cpu()
                if key is not None:
                    self._by_count[key] = t
            self._text[caption] = t
            return t
        if not self.synthetic_text:
            raise M2TError(f"SemanticLoss: no text feature for caption {caption!r}: inject the MedCLIP text embeddings with "
                           "set_text_features({caption: tensor[512]}) (the text tower is not part of this build), or construct "
                           "SemanticLoss(synthetic_text=True) for a benchmark with stand-in embeddings")
        t = hash_text_feature(caption)
        self._text[caption] = t                    # deterministic: computed once per caption
        return t

    # ---- reference semantics ------------------------------------------------------------------
    def createNRandompatches(self, hs: int, ws: int, N: int, patch_size: int = 224):
        """Coordinates only (losses.py:29-40): x then y per patch, torch.randint on the global CPU RNG;
        `x` indexes rows (size(2)), `y` columns -- naming kept from the reference."""
        out = []
        for _ in range(N):
            xcoord = int(torch.randint(hs - patch_size, ()))
            ycoord = int(torch.randint(ws - patch_size, ()))
            out.append((xcoord, ycoord))
        return out

    def batch(self, sr: torch.Tensor, hr: torch.Tensor, captions: Iterable[str]) -> torch.Tensor:
        """Sum over the batch of loss_clip(sr[i], hr[i], captions[i]) (train.py:203-205, without the
        lambda_clip factor) -> Tensor[1]; also leaves the per-sample values in ``self.last_per_sample``.
        With ``differentiable=True`` and ``sr.requires_grad`` the result is connected to ``sr``: d total / d sr is computed
        here (an eager vector-Jacobian product: the output is a scalar), and the autograd backward only scales and returns it."""
        if self.differentiable and sr.requires_grad and torch.is_grad_enabled():
            tot, g, origins = self._value_and_grad(sr, hr, captions)
            return _SemanticLossGrad.apply(sr, tot, g, origins)
        tot, _, _ = self._run(sr, hr, captions, want_grad=False)
        return tot

    def _value_and_grad(self, sr: torch.Tensor, hr: torch.Tensor, captions):
        """(total [1], g, origins): d total / d sr as g [B,C,gh,gw] with per-sample (row0, col0) origins (the last random crop),
        or the dense gradient and origins None (N_patches == 1).  A 1-channel sr is differentiated through the channel repeat."""
        c = sr.shape[1]
        tot, g, origins = self._run(sr, hr, captions, want_grad=True)
        if c != 3:
            g = g.sum(dim=1, keepdim=True)
        return tot, g, origins

    def _run(self, sr: torch.Tensor, hr: torch.Tensor, captions, want_grad: bool):
        captions = list(captions)
        B = sr.shape[0]
        if len(captions) != B or tuple(sr.shape) != tuple(hr.shape):
            raise M2TError("SemanticLoss.batch: need one caption per sample and sr/hr of equal shape")
        if sr.shape[1] != 3:
            sr, hr = sr.repeat(1, 3, 1, 1), hr.repeat(1, 3, 1, 1)         # losses.py:47-49
        enc = self._encoder()
        if 2 * B > enc.max_images:
            raise M2TError(f"batch {B} exceeds max_batch {self.max_batch}")
        hs, ws = sr.shape[2], sr.shape[3]
        g, origins = None, None
        with torch.no_grad():
            if self.N_patches > 1:
                last = []
                for _ in range(B):                                       # same RNG order as B sequential calls
                    last.append(self.createNRandompatches(hs, ws, self.N_patches - 1)[-1])
                crops = [(i, last[i][0], last[i][1]) for i in range(B)] + [(B + i, last[i][0], last[i][1]) for i in range(B)]
                if want_grad:
                    emb = enc.encode_grad(sr.detach(), hr.detach(), crops, B)
                    origins = [(int(last[i][0]), int(last[i][1])) for i in range(B)]
                else:
                    emb = enc.encode_pair(sr.detach(), hr.detach(), crops)   # SR crops then HR crops, no torch.cat of the batches
            else:
                src = torch.cat((sr.detach().float(), hr.detach().float()), dim=0).contiguous()
                small = torch.empty(2 * B, 3, 224, 224, dtype=torch.float32, device=sr.device)
                with torch.cuda.device(sr.device):
                    _lib.check(_lib.load().m2t_bicubic_resize(_lib.ptr(src), _lib.ptr(small), 2 * B * 3, hs, ws, 224, 224,
                                                              _lib.stream_ptr()), "m2t_bicubic_resize")
                if want_grad:
                    emb = enc.encode_grad(small, None, [(i, 0, 0) for i in range(2 * B)], B)
                else:
                    emb = enc.encode(small, [(i, 0, 0) for i in range(2 * B)])
            dev = sr.device
            key = tuple(captions)
            if self._text_dev is None or self._text_dev[0] != key or self._text_dev[1].device != dev:
                # the text features are constants of the frozen model: one upload per distinct caption list
                self._text_dev = (key, torch.stack([self._text_feature(c) for c in captions]).to(dev))
            text = self._text_dev[1]
            per = torch.empty(B, dtype=torch.float32, device=dev)
            tot = torch.empty(1, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.load().m2t_semantic_loss(_lib.ptr(emb), _lib.ptr(text), B, self.N_patches, _lib.ptr(per),
                                                         _lib.ptr(tot), _lib.stream_ptr()), "m2t_semantic_loss")
                if want_grad:
                    lib = _lib.load()
                    g_emb = torch.empty(B, 512, dtype=torch.float32, device=dev)
                    _lib.check(lib.m2t_semantic_loss_backward(_lib.ptr(emb), _lib.ptr(text), B, self.N_patches, _lib.ptr(g_emb),
                                                              _lib.stream_ptr()), "m2t_semantic_loss_backward")
                    g_crops = enc.backward(g_emb, B)
                    if self.N_patches > 1:
                        g = g_crops
                    else:
                        g = torch.empty(B, 3, hs, ws, dtype=torch.float32, device=dev)
                        _lib.check(lib.m2t_bicubic_resize_backward(_lib.ptr(g_crops), _lib.ptr(g), B * 3, hs, ws, 224, 224,
                                                                   _lib.stream_ptr()), "m2t_bicubic_resize_backward")
        self.last_per_sample = per
        self.last_embeddings = emb            # [2B,512]: SR rows then HR rows, unit norm (kept for inspection)
        return tot, g, origins

    def __call__(self, x: torch.Tensor, y: torch.Tensor, batch_tokens: str) -> torch.Tensor:
        """Single sample, as called by train.py:205: x, y [3,Hs,Ws] (or [1,Hs,Ws]) -> Tensor[1]."""
        return self.batch(x.unsqueeze(0).to(self.device), y.unsqueeze(0).to(self.device), [batch_tokens])


def paste_crops(g: torch.Tensor, origins, shape) -> torch.Tensor:
    """Dense [B,C,H,W] gradient from per-sample blocks g [B,C,gh,gw] at (row0, col0) origins (None: g is dense already)."""
    if origins is None:
        return g
    out = torch.zeros(shape, dtype=g.dtype, device=g.device)
    gh, gw = g.shape[2], g.shape[3]
    for i, (y0, x0) in enumerate(origins):
        out[i, :, y0:y0 + gh, x0:x0 + gw] = g[i]
    return out


class _SemanticLossGrad(torch.autograd.Function):
    """Edge from the SemanticLoss total to sr.  The gradient was computed eagerly with the value (a scalar output: one
    vector-Jacobian product), so nothing of the encoder is kept across calls; backward scales it by the upstream gradient."""

    @staticmethod
    def forward(ctx, sr, tot, g, origins):
        ctx.origins = origins
        ctx.shape = tuple(sr.shape)
        ctx.save_for_backward(g)
        return tot.clone()

    @staticmethod
    def backward(ctx, go):
        (g,) = ctx.saved_tensors
        return paste_crops(g * go.reshape(()), ctx.origins, ctx.shape).to(go.dtype), None, None, None


# ---------------------------------------------------------------------------------------------------------------
# What the image-pair losses below share: the refusals of a pair of tensors, the buffers around one m2t_*_loss_tensor call, and the
# autograd edge of a loss whose value and gradient come from that one call.
# ---------------------------------------------------------------------------------------------------------------
def _pair_check(what, x, y, device=True, y_no_grad=True):
    """Two [B,C,H,W] tensors of equal shape; on a HIP device; y without grad (a metric passes y_no_grad=False; a caller with rules
    of its own between the shape and the device refusal passes device=False first and comes back)."""
    if x.dim() != 4 or x.shape != y.shape:
        raise M2TError(f"{what}: expected two [B,C,H,W] tensors of equal shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if device and not (x.is_cuda and y.is_cuda):
        raise M2TError(f"{what} needs HIP device tensors (there is no host implementation)")
    if device and y_no_grad and y.requires_grad:
        raise M2TError(f"{what} gives the gradient with respect to x only: y must not require grad (detach it)")


def _tensor_loss(name, no_scratch, x, y, want_grad, per_count, args):
    """One ``m2t_<name>_loss_tensor`` call on device tensors [B,C,H,W] -> (loss [1] float32, gradient or None, per-item float64 or
    None).  Made here: the contiguous fp32 copies, the entry's scratch (a shape it names no size for is refused with ``no_scratch``),
    the value, the zeroed gradient if wanted, ``per_count(B, C)`` per-item results if wanted.  ``args(B, C, H, W, grad, out, per,
    scratch)`` gives the entry's arguments behind x_row_stride, the four buffers as pointers."""
    lib = _lib.load()
    xc, yc = x.detach().contiguous().float(), y.detach().contiguous().float()
    B, Cn, H, W = xc.shape
    nbytes = getattr(lib, f"m2t_{name}_loss_scratch_bytes")(B, Cn, H, W)
    if nbytes == 0:
        raise M2TError(no_scratch.format(B=B, C=Cn, H=H, W=W))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=xc.device)
    out = torch.empty(1, dtype=torch.float32, device=xc.device)
    grad = torch.zeros_like(xc) if want_grad else None
    per = torch.empty(per_count(B, Cn), dtype=torch.float64, device=xc.device) if per_count is not None else None
    entry = f"m2t_{name}_loss_tensor"
    with torch.cuda.device(xc.device):
        _lib.check(getattr(lib, entry)(_lib.ptr(xc), _lib.ptr(yc), B, Cn, H, W, Cn * H * W, W,
                                       *args(B, Cn, H, W, _lib.ptr(grad), _lib.ptr(out), _lib.ptr(per), _lib.ptr(scratch)),
                                       _lib.stream_ptr()), entry)
    return out, grad, per


class _EagerGradFn(torch.autograd.Function):
    """Edge from a loss to ``x`` when value and gradient come from one eager call: ``call(want_grad) -> (out [1], gradient of the
    value or None)``.  Nothing else is kept; backward scales that gradient by the upstream one."""

    @staticmethod
    def forward(ctx, x, call):
        out, ctx.grad = call(ctx.needs_input_grad[0])
        ctx.x_dtype = x.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        return (ctx.grad * g).to(ctx.x_dtype), None


# ---------------------------------------------------------------------------------------------------------------
# The structural term: 1 - SSIM (the reference imports SSIMLoss / MultiScaleSSIMLoss from piq, losses.py:8, and scores every
# epoch by SSIM, utils.py:232-234).  Value and gradient are HIP (m2t_ssim_loss_tensor, k_ssim_loss.hip); there is no torch fallback.
# ---------------------------------------------------------------------------------------------------------------
def _ssim_call(x, y, data_range, want_grad):
    """(loss [1] float32, gradient of the mean or None) of device tensors [B,C,H,W]."""
    return _tensor_loss("ssim", "ssim_loss: image {H}x{W} is smaller than the 11 x 11 window", x, y, want_grad, None,
                        lambda B, Cn, H, W, grad, out, per, scratch:
                        (float(data_range), 0, 1.0 / (B * Cn * (H - 10) * (W - 10)), grad, out, 0, scratch))[:2]


def ssim_loss(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """mean(1 - SSIM(x, y)) over the per-channel VALID map, the ``pytorch_msssim.ssim`` / ``piq.ssim(downsample=False)`` form
    (11-tap Gaussian sigma 1.5, K = (0.01, 0.03), no clamp of the map, inputs NOT clamped to the data range), for device tensors
    [B,C,H,W] with H, W >= 11; differentiable with respect to ``x`` only.  ``piq.SSIMLoss``'s default ``downsample=True`` (an
    average pooling in front, by 2 at 512 x 512) is not applied.  fp64 inside the kernel, fp32 in and out."""
    _pair_check("ssim_loss", x, y)
    if not (float(data_range) > 0.0):
        raise M2TError(f"ssim_loss: data_range must be > 0, got {data_range!r}")
    return _EagerGradFn.apply(x, lambda want_grad: _ssim_call(x, y, data_range, want_grad))


class SSIMLoss(nn.Module):
    """``ssim_loss`` as a module (``piq.SSIMLoss(downsample=False, data_range=...)``'s value for inputs inside the data range)."""

    def __init__(self, data_range: float = 1.0):
        super().__init__()
        self.data_range = float(data_range)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return ssim_loss(x, y, self.data_range)


# ---------------------------------------------------------------------------------------------------------------
# The multi-scale structural term: 1 - MS-SSIM (the reference imports MultiScaleSSIMLoss from piq, losses.py:8).  Value and gradient
# are HIP (m2t_msssim_loss_tensor of include/m2t_msssim.h, k_msssim_loss.hip); there is no torch fallback.
# ---------------------------------------------------------------------------------------------------------------
def _msssim_call(x, y, data_range, want_grad, want_per_channel):
    """(loss [1] float32, gradient of the mean or None, M_bc [B*C] float64 or None) of device tensors [B,C,H,W]."""
    return _tensor_loss("msssim", "ms_ssim: no scratch size for [{B},{C},{H},{W}] (height and width must be larger than 160, B * C at most 65535)",
                        x, y, want_grad, (lambda B, Cn: B * Cn) if want_per_channel else None,
                        lambda B, Cn, H, W, grad, out, per, scratch: (float(data_range), 0, 1.0 / (B * Cn), grad, out, per, 0, scratch))


def _msssim_check(what, x, y, data_range, y_no_grad=False):
    _pair_check(what, x, y, y_no_grad=y_no_grad)
    if not (float(data_range) > 0.0):
        raise M2TError(f"{what}: data_range must be > 0, got {data_range!r}")
    H, W = int(x.shape[2]), int(x.shape[3])
    if min(H, W) < _lib.MSSSIM_MIN_SIDE:
        raise M2TError(f"{what}: image {H}x{W} is too small for five levels under the 11-tap window (height and width must be larger than 160)")


def ms_ssim_loss(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """1 - mean over (image, channel) of MS-SSIM(x, y), the ``pytorch_msssim.ms_ssim`` / ``piq.multi_scale_ssim`` form (five levels,
    weights 0.0448, 0.2856, 0.3001, 0.2363, 0.1333, 11-tap Gaussian sigma 1.5, K = (0.01, 0.03), the 2 x 2 average with padding
    side % 2 between the levels, inputs NOT clamped to the data range), for device tensors [B,C,H,W] with H, W > 160; differentiable
    with respect to ``x`` only.  An (image, channel) one of whose level means is not positive has MS-SSIM 0 and gradient 0 (torch's
    autograd gives 0 * inf there).  fp64 inside the kernels, fp32 in and out."""
    _msssim_check("ms_ssim_loss", x, y, data_range, y_no_grad=True)
    return _EagerGradFn.apply(x, lambda want_grad: _msssim_call(x, y, data_range, want_grad, False)[:2])


class MSSSIMLoss(nn.Module):
    """``ms_ssim_loss`` as a module."""

    def __init__(self, data_range: float = 1.0):
        super().__init__()
        self.data_range = float(data_range)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return ms_ssim_loss(x, y, self.data_range)


# ---------------------------------------------------------------------------------------------------------------
# The information-fidelity term: 1 - VIF, pixel domain (the reference imports VIFLoss from piq, losses.py:8).  Value and gradient are
# HIP (m2t_vif_loss_tensor of include/m2t_vif.h, k_vif_loss.hip); there is no torch fallback.
# ---------------------------------------------------------------------------------------------------------------
def _vif_call(x, y, data_range, sigma_n_sq, want_grad, want_per_image):
    """(loss [1] float32, gradient of the mean or None, VIF_b [B] float64 or None) of device tensors [B,C,H,W]."""
    return _tensor_loss("vif", "vif: no scratch size for [{B},{C},{H},{W}] (height and width at least 41, 1 or 3 channels, B at most 65535)",
                        x, y, want_grad, (lambda B, Cn: B) if want_per_image else None,
                        lambda B, Cn, H, W, grad, out, per, scratch:
                        (float(data_range), float(sigma_n_sq), 0, 1.0 / B, grad, out, per, 0, scratch))


def _vif_check(what, x, y, data_range, sigma_n_sq, y_no_grad=False):
    _pair_check(what, x, y, y_no_grad=y_no_grad)
    if not (math.isfinite(float(data_range)) and float(data_range) > 0.0):
        raise M2TError(f"{what}: data_range must be a finite number > 0, got {data_range!r}")
    if not (math.isfinite(float(sigma_n_sq)) and float(sigma_n_sq) > 0.0):
        raise M2TError(f"{what}: sigma_n_sq must be a finite number > 0, got {sigma_n_sq!r}")
    if int(x.shape[1]) not in (1, 3):
        raise M2TError(f"{what}: VIF works on the luminance of 1 or 3 channels, got {int(x.shape[1])}")
    H, W = int(x.shape[2]), int(x.shape[3])
    if min(H, W) < _lib.VIF_MIN_SIDE:
        raise M2TError(f"{what}: image {H}x{W} is too small for four scales under the 17 / 9 / 5 / 3-tap windows (height and width must be at least 41)")


def vif_loss(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, sigma_n_sq: float = 2.0) -> torch.Tensor:
    """1 - mean over the images of VIF(x, y), the pixel-domain visual information fidelity of Sheikh & Bovik in the ``piq.vif_p``
    form (luminance of an RGB image on the 0 .. 255 scale, four scales with Gaussian windows of 17, 9, 5, 3 taps, a filtered and
    decimated pyramid, inputs NOT clamped to the data range), for device tensors [B,C,H,W] with C = 1 or 3 and H, W >= 41;
    differentiable with respect to ``x`` only.  VIF exceeds 1 for a contrast-enhanced ``x``: the value may be negative and is not
    clipped.  fp64 inside the kernels, fp32 in and out."""
    _vif_check("vif_loss", x, y, data_range, sigma_n_sq, y_no_grad=True)
    return _EagerGradFn.apply(x, lambda want_grad: _vif_call(x, y, data_range, sigma_n_sq, want_grad, False)[:2])


class VIFLoss(nn.Module):
    """``vif_loss`` as a module."""

    def __init__(self, data_range: float = 1.0, sigma_n_sq: float = 2.0):
        super().__init__()
        self.data_range = float(data_range)
        self.sigma_n_sq = float(sigma_n_sq)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return vif_loss(x, y, self.data_range, self.sigma_n_sq)


# ---------------------------------------------------------------------------------------------------------------
# LR-consistency (the "dual regression" / cycle term): rho(D(clamp(sr)) - lr), D the bicubic down-sampler that made the training
# pairs.  The only term that needs no HR: ``ConsistencyLoss(4)(model(lr), lr).backward()`` fine-tunes on real LR frames.  Value and
# gradient are HIP (m2t_consistency_loss_tensor of include/m2t_consistency.h, k_consistency.hip); there is no torch fallback.
# ---------------------------------------------------------------------------------------------------------------
def _consistency_check(what, sr, lr, scale, eps, data_range, lr_no_grad=True):
    if scale not in (2, 3, 4):
        raise M2TError(f"{what}: scale must be 2, 3 or 4, got {scale!r}")
    if not (math.isfinite(float(data_range)) and float(data_range) > 0.0):
        raise M2TError(f"{what}: data_range must be a finite number > 0, got {data_range!r}")
    if not (math.isfinite(float(eps)) and float(eps) >= 0.0):
        raise M2TError(f"{what}: eps must be a finite number >= 0, got {eps!r}")
    if sr.dim() != 4 or lr.dim() != 4 or tuple(sr.shape) != (lr.shape[0], lr.shape[1], lr.shape[2] * scale, lr.shape[3] * scale):
        raise M2TError(f"{what}: expected sr [B,C,H*{scale},W*{scale}] and lr [B,C,H,W], got {tuple(sr.shape)} and {tuple(lr.shape)}")
    if int(sr.shape[1]) not in (1, 3):
        raise M2TError(f"{what}: 1 or 3 channels, got {int(sr.shape[1])}")
    if not (sr.is_cuda and lr.is_cuda):
        raise M2TError(f"{what} needs HIP device tensors (there is no host implementation)")
    if lr_no_grad and lr.requires_grad:
        raise M2TError(f"{what} gives the gradient with respect to sr only: lr must not require grad (detach it)")


def _consistency_call(sr, lr, scale, eps, data_range, clamp, want_grad, want_stats=False):
    """(loss [1] float32 = mean rho(r), its gradient or None, {mean |r|, max |r|, mean r^2} float64 [3] or None)."""
    lib = _lib.load()
    xc, yc = sr.detach().contiguous().float(), lr.detach().contiguous().float()
    B, Cn, H, W = yc.shape
    nbytes = lib.m2t_consistency_scratch_bytes(B, Cn, H, W, int(scale))
    if nbytes == 0:
        raise M2TError(f"consistency: no scratch size for LR [{B},{Cn},{H},{W}] x{scale} (SR sides at most 16384, B * C at most 65535)")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=xc.device)
    out = torch.empty(1, dtype=torch.float32, device=xc.device)
    grad = torch.zeros_like(xc) if want_grad else None
    stats = torch.empty(3, dtype=torch.float64, device=xc.device) if want_stats else None
    Hs, Ws = H * int(scale), W * int(scale)
    with torch.cuda.device(xc.device):
        _lib.check(lib.m2t_consistency_loss_tensor(_lib.ptr(xc), _lib.ptr(yc), B, Cn, H, W, int(scale), Cn * Hs * Ws, Ws, float(data_range),
                                                   int(bool(clamp)), float(eps), 1.0 / (B * Cn * H * W), _lib.ptr(grad), _lib.ptr(out),
                                                   _lib.ptr(stats), 0, _lib.ptr(scratch), _lib.stream_ptr()), "m2t_consistency_loss_tensor")
    return out, grad, stats


def consistency_loss(sr: torch.Tensor, lr: torch.Tensor, scale: int, eps: float = 0.0, data_range: float = 1.0,
                     clamp: bool = True) -> torch.Tensor:
    """mean rho((D(c(sr)) - lr) / data_range) over the LR elements: D the bicubic x`scale` down-sampler of `resize.imresize`,
    c the clamp to [0, data_range] (clamp=False: none), rho(r) = |r| for eps = 0 and sqrt(r^2 + eps^2) otherwise.  Device tensors
    sr [B,C,H*scale,W*scale] and lr [B,C,H,W], C = 1 or 3; differentiable with respect to ``sr`` only, through the adjoint of D and
    the clamp mask (the ends of the range pass).  fp64 inside the kernels, fp32 in and out."""
    _consistency_check("consistency_loss", sr, lr, scale, eps, data_range)
    return _EagerGradFn.apply(sr, lambda want_grad: _consistency_call(sr, lr, scale, eps, data_range, clamp, want_grad)[:2])


class ConsistencyLoss(nn.Module):
    """``consistency_loss`` as a module: ``ConsistencyLoss(4)(model(lr), lr)``."""

    def __init__(self, scale: int, eps: float = 0.0, data_range: float = 1.0):
        super().__init__()
        if scale not in (2, 3, 4):
            raise M2TError(f"ConsistencyLoss: scale must be 2, 3 or 4, got {scale!r}")
        self.scale, self.eps, self.data_range = int(scale), float(eps), float(data_range)

    def forward(self, sr: torch.Tensor, lr: torch.Tensor) -> torch.Tensor:
        return consistency_loss(sr, lr, self.scale, self.eps, self.data_range)


# ---------------------------------------------------------------------------------------------------------------
# The gradient-magnitude term: GMSD (the reference scores every model by it, test.py:95-122; piq ships GMSDLoss next to the classes
# the reference imports).  Value and gradient are HIP (m2t_gmsd_loss_tensor of include/m2t_gmsd.h, k_gmsd_loss.hip); there is no torch
# fallback -- autograd through sqrt(gx^2 + gy^2) is NaN wherever the image is locally flat.
# ---------------------------------------------------------------------------------------------------------------
def _gmsd_call(x, y, data_range, want_grad, want_per_image):
    """(loss [1] float32, gradient of the mean or None, GMSD_b [B] float64 or None) of device tensors [B,C,H,W]."""
    return _tensor_loss("gmsd", "gmsd: no scratch size for [{B},{C},{H},{W}] (height and width at least 2, 1 or 3 channels, B at most 65535)",
                        x, y, want_grad, (lambda B, Cn: B) if want_per_image else None,
                        lambda B, Cn, H, W, grad, out, per, scratch: (float(data_range), 0, 1.0 / B, grad, out, per, 0, scratch))


def _gmsd_check(what, x, y, data_range, y_no_grad=False):
    _pair_check(what, x, y, y_no_grad=y_no_grad)
    if not (math.isfinite(float(data_range)) and float(data_range) > 0.0):
        raise M2TError(f"{what}: data_range must be a finite number > 0, got {data_range!r}")
    if int(x.shape[1]) not in (1, 3):
        raise M2TError(f"{what}: GMSD works on the luminance of 1 or 3 channels, got {int(x.shape[1])}")
    H, W = int(x.shape[2]), int(x.shape[3])
    if min(H, W) < _lib.GMSD_MIN_SIDE:
        raise M2TError(f"{what}: image {H}x{W} is too small (height and width must be at least 2: one 2 x 2 cell)")


def gmsd_loss(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """The mean over the images of GMSD(x, y), the gradient magnitude similarity deviation of Xue et al. in the ``piq.gmsd`` form
    (luminance / data_range, a 2 x 2 average with a zero pad to an even size, the zero-padded Prewitt pair, T = 170 / 255^2, the
    standard deviation of the similarity map; inputs NOT clamped to the data range), for device tensors [B,C,H,W] with C = 1 or 3
    and H, W >= 2; differentiable with respect to ``x`` only.  0 = identical: the value is the distortion itself, there is no
    "1 -".  Where the pooled x is locally flat the gradient is exactly 0 (torch's autograd gives 0 * inf = NaN there), and an image
    whose GMSD is 0 adds no gradient.  fp64 inside the kernels, fp32 in and out."""
    _gmsd_check("gmsd_loss", x, y, data_range, y_no_grad=True)
    return _EagerGradFn.apply(x, lambda want_grad: _gmsd_call(x, y, data_range, want_grad, False)[:2])


class GMSDLoss(nn.Module):
    """``gmsd_loss`` as a module."""

    def __init__(self, data_range: float = 1.0):
        super().__init__()
        self.data_range = float(data_range)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return gmsd_loss(x, y, self.data_range)


# ---------------------------------------------------------------------------------------------------------------
# The wavelet-domain term: an L1 (or Charbonnier) on the detail bands of an undecimated 2-D wavelet transform with periodic borders
# (the model itself moves between its scales through a Haar DWT).  Value, gradient and the transform alone are HIP
# (m2t_wavelet_loss_tensor / m2t_swt2 of include/m2t_wavelet.h, k_wavelet_loss.hip); there is no torch fallback -- torch has no SWT.
# ---------------------------------------------------------------------------------------------------------------
def _wavelet_check(what, x, w, min_what="image"):
    if int(x.shape[1]) not in (1, 3):
        raise M2TError(f"{what}: the wavelet kernels take 1 or 3 channels, got {int(x.shape[1])}")
    H, W = int(x.shape[2]), int(x.shape[3])
    need = _lib.wavelet_min_side(len(w.lo), w.levels)
    if min(H, W) < need:
        raise M2TError(f"{what}: {min_what} {H}x{W} is too small for {len(w.lo)} taps at {w.levels} levels (height and width must be at "
                       f"least {need}: a tap index wraps at most once)")


def _wavelet_scratch(what, lib, xc, w):
    B, Cn, H, W = xc.shape
    nbytes = lib.m2t_wavelet_loss_scratch_bytes(B, Cn, H, W, w.levels, len(w.lo))
    if nbytes == 0:
        raise M2TError(f"{what}: no scratch size for [{B},{Cn},{H},{W}] (1 or 3 channels, B * C at most 65535)")
    return torch.empty(nbytes, dtype=torch.uint8, device=xc.device)


def _wavelet_call(x, y, data_range, w, want_grad, want_per_band=False):
    """(loss [1] float32, gradient of the mean or None, band sums [3 J + 1] float64 or None) of device tensors [B,C,H,W]."""
    from .train_step import wavelet_call_args
    lib = _lib.load()
    xc, yc = x.detach().contiguous().float(), y.detach().contiguous().float()
    B, Cn, H, W = xc.shape
    scratch = _wavelet_scratch("wavelet_loss", lib, xc, w)
    out = torch.empty(1, dtype=torch.float32, device=xc.device)
    grad = torch.zeros_like(xc) if want_grad else None
    per = torch.empty(3 * w.levels + 1, dtype=torch.float64, device=xc.device) if want_per_band else None
    with torch.cuda.device(xc.device):
        _lib.check(lib.m2t_wavelet_loss_tensor(_lib.ptr(xc), _lib.ptr(yc), B, Cn, H, W, Cn * H * W, W, float(data_range), 0,
                                               1.0 / (B * Cn * H * W), *wavelet_call_args(w), _lib.ptr(grad), _lib.ptr(out),
                                               _lib.ptr(per), 0, _lib.ptr(scratch), _lib.stream_ptr()), "m2t_wavelet_loss_tensor")
    return out, grad, per


def wavelet_loss(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, wavelet="haar", levels: int = 2, band_weights=None,
                 eps: float = 0.0) -> torch.Tensor:
    """The mean over the coefficients of ``sum_band w_band rho(c_band)`` on the undecimated (stationary, a-trous) 2-D wavelet
    transform of ``x / data_range - y / data_range`` with periodic borders, for device tensors [B,C,H,W] with C = 1 or 3;
    differentiable with respect to ``x`` only.  ``wavelet``: ``'haar'``, ``'db2'`` (the orthonormal filters divided by sqrt(2)) or a
    pair ``(lo, hi)`` of 2 to 8 taps each; ``levels`` 1 .. 3; ``band_weights``: 3 levels + 1 numbers for (LH, HL, HH) of each level,
    then LL -- by default 1 for every detail band and 0 for LL; ``rho(c) = |c|`` for ``eps = 0`` and ``sqrt(c^2 + eps^2)`` otherwise.
    Inputs are NOT clamped to the data range.  fp64 inside the kernels, fp32 in and out."""
    from .train_step import resolve_wavelet
    _pair_check("wavelet_loss", x, y, device=False)
    w = resolve_wavelet(wavelet, levels, band_weights, eps)
    if not (math.isfinite(float(data_range)) and float(data_range) > 0.0):
        raise M2TError(f"wavelet_loss: data_range must be a finite number > 0, got {data_range!r}")
    _wavelet_check("wavelet_loss", x, w)
    _pair_check("wavelet_loss", x, y, y_no_grad=True)
    return _EagerGradFn.apply(x, lambda want_grad: _wavelet_call(x, y, data_range, w, want_grad)[:2])


class WaveletLoss(nn.Module):
    """``wavelet_loss`` as a module."""

    def __init__(self, data_range: float = 1.0, wavelet="haar", levels: int = 2, band_weights=None, eps: float = 0.0):
        super().__init__()
        from .train_step import resolve_wavelet
        w = resolve_wavelet(wavelet, levels, band_weights, eps)
        self.data_range, self.wavelet, self.levels, self.band_weights, self.eps = float(data_range), w.wavelet, w.levels, w.band_weights, w.eps

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return wavelet_loss(x, y, self.data_range, self.wavelet, self.levels, self.band_weights, self.eps)


def swt2(x: torch.Tensor, wavelet="haar", levels: int = 2) -> torch.Tensor:
    """The undecimated 2-D wavelet transform of a device tensor [B,C,H,W] (C = 1 or 3) with periodic borders: float32
    [B,C,3 levels + 1,H,W], the bands (LH_1, HL_1, HH_1, ..., LH_J, HL_J, HH_J, LL_J), each value one fp32 rounding of the fp64
    coefficient.  Not differentiable."""
    from .train_step import resolve_wavelet, wavelet_call_args
    if x.dim() != 4:
        raise M2TError(f"swt2: expected a [B,C,H,W] tensor, got {tuple(x.shape)}")
    w = resolve_wavelet(wavelet, levels)
    _wavelet_check("swt2", x, w)
    if not x.is_cuda:
        raise M2TError("swt2 needs a HIP device tensor (there is no host implementation)")
    lib = _lib.load()
    xc = x.detach().contiguous().float()
    B, Cn, H, W = xc.shape
    scratch = _wavelet_scratch("swt2", lib, xc, w)
    out = torch.empty((B, Cn, 3 * w.levels + 1, H, W), dtype=torch.float32, device=xc.device)
    lo, hi, taps, J, _, _ = wavelet_call_args(w)
    with torch.cuda.device(xc.device):
        _lib.check(lib.m2t_swt2(_lib.ptr(xc), B, Cn, H, W, Cn * H * W, W, lo, hi, taps, J, _lib.ptr(out), _lib.ptr(scratch),
                                _lib.stream_ptr()), "m2t_swt2")
    return out


# ---------------------------------------------------------------------------------------------------------------
# The frequency-domain term: an L1 on the coefficients of rfft2 (the reference imports torch.fft, losses.py:5, and never calls it;
# MIMO-UNet's F.l1_loss(view_as_real(rfft2(x)), view_as_real(rfft2(y)))).  Value and gradient are HIP (m2t_fft_loss_tensor of
# include/m2t_spectral.h, k_fft_loss.hip); there is no torch fallback.
# ---------------------------------------------------------------------------------------------------------------
def _fft_call(x, y, data_range, norm, want_grad):
    """(loss [1] float32, gradient of the mean or None) of device tensors [B,C,H,W]."""
    return _tensor_loss("fft", "fft_loss: no scratch size for [{B},{C},{H},{W}] (B * C must be 1 .. 65535)", x, y, want_grad, None,
                        lambda B, Cn, H, W, grad, out, per, scratch:
                        (float(data_range), 0, _lib.FFT_NORMS[norm], 1.0 / (2 * B * Cn * H * (W // 2 + 1)), grad, out, 0, scratch))[:2]


def fft_loss(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, norm: str = "backward") -> torch.Tensor:
    """``F.l1_loss(view_as_real(rfft2(x / data_range, norm=norm)), view_as_real(rfft2(y / data_range, norm=norm)))`` as ONE transform
    of the difference, for device tensors [B,C,H,W] (inputs NOT clamped to the data range); differentiable with respect to ``x``
    only.  H and W must be even, 8 .. 2048 and of the form 2^a * 3^b.  The imaginary part of the four self-conjugate bins is
    exactly 0 (torch leaves rounding noise there and takes its sign); sign(0) = 0.  fp32 butterflies, fp64 sums."""
    from .train_step import FFT_SIZE_RULE, fft_size_supported, resolve_fft_norm
    _pair_check("fft_loss", x, y)
    if not (float(data_range) > 0.0):
        raise M2TError(f"fft_loss: data_range must be > 0, got {data_range!r}")
    H, W = int(x.shape[2]), int(x.shape[3])
    if not (fft_size_supported(H) and fft_size_supported(W)):
        raise M2TError(f"fft_loss: image size {H}x{W} is not supported by the HIP transform (height and width must be {FFT_SIZE_RULE})")
    norm = resolve_fft_norm(norm)
    return _EagerGradFn.apply(x, lambda want_grad: _fft_call(x, y, data_range, norm, want_grad))


class FFTLoss(nn.Module):
    """``fft_loss`` as a module."""

    def __init__(self, data_range: float = 1.0, norm: str = "backward"):
        super().__init__()
        from .train_step import resolve_fft_norm
        self.data_range = float(data_range)
        self.norm = resolve_fft_norm(norm)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return fft_loss(x, y, self.data_range, self.norm)


# ---------------------------------------------------------------------------------------------------------------
# The VGG19 feature ("perceptual") term: PerceptualLoss of the reference's losses.py:222-270.  Value and gradient are HIP
# (m2t_vgg_loss_tensor of include/m2t_perceptual.h; k_vgg.hip, m2t_vgg.hip: bf16 MFMA convolutions); there is no torch fallback.
# Inference semantics: plain vgg19 weights, or vgg19_bn weights folded on the host in fp64; training-mode batch statistics are not
# reproduced.  No weights ship: load_vgg_state_dict first.
# ---------------------------------------------------------------------------------------------------------------
PERCEPTUAL_CRITERIA = {"l1": (0, 0.0), "sl1": (3, 1.0), "l2": (1, 0.0)}     # (M2T_LOSS_* kind, param); nn.SmoothL1Loss: beta = 1
_VGG19_BN_CONVS = (0, 3, 7, 10, 14, 17, 20, 23, 27, 30, 33, 36, 40)         # torchvision vgg19_bn: features.<i> of the same convolutions


def vgg_param_names() -> List[str]:
    """The 26 tensors the tower takes, torchvision ``vgg19`` naming, in flat order."""
    return [f"features.{i}.{k}" for i in _lib.VGG_LAYERS for k in ("weight", "bias")]


def _vgg_strip(key: str) -> str:
    for prefix in ("module.", "vgg."):
        if key.startswith(prefix):
            key = key[len(prefix):]
    if not key.startswith("features.") and key[:1].isdigit():
        key = "features." + key
    return key


def vgg_fold_state_dict(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A ``vgg19`` or ``vgg19_bn`` state dict (keys with or without a ``features.`` / ``vgg.`` prefix; classifier and deeper layers
    ignored) -> the 26 float32 tensors under ``vgg19`` names.  Batch norm is folded in fp64 with its running statistics (eval mode):
    w' = w * gamma / sqrt(var + eps), b' = (b - mean) * gamma / sqrt(var + eps) + beta, eps = 1e-5."""
    sd = {_vgg_strip(k): v for k, v in state.items()}
    is_bn = any(k.endswith("running_mean") for k in sd)
    out = {}
    for plain, bn in zip(_lib.VGG_LAYERS, _VGG19_BN_CONVS):
        src = bn if is_bn else plain
        try:
            w = sd[f"features.{src}.weight"].detach().double().cpu()
            b = sd[f"features.{src}.bias"].detach().double().cpu()
            if is_bn:
                g, beta = sd[f"features.{src + 1}.weight"].detach().double().cpu(), sd[f"features.{src + 1}.bias"].detach().double().cpu()
                mean, var = sd[f"features.{src + 1}.running_mean"].detach().double().cpu(), sd[f"features.{src + 1}.running_var"].detach().double().cpu()
                s = g / torch.sqrt(var + 1e-5)
                w, b = w * s.view(-1, 1, 1, 1), (b - mean) * s + beta
        except KeyError as e:
            raise M2TError(f"load_vgg_state_dict: missing {e.args[0]} ({'vgg19_bn' if is_bn else 'vgg19'} naming)") from None
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or b.shape[0] != w.shape[0]:
            raise M2TError(f"load_vgg_state_dict: features.{src} is not a 3x3 convolution: {tuple(w.shape)}")
        out[f"features.{plain}.weight"], out[f"features.{plain}.bias"] = w.float(), b.float()
    return out



class PerceptualLoss(nn.Module, _lib.Handle):
    """The reference's ``PerceptualLoss(weights, resize, criterion)`` plus ``data_range``: ``sum_k weights[k] * crit(F_k(x), F_k(y))`` on
    VGG19's relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 of ``((t / data_range) - mean) / std`` (one channel repeated to three; inputs
    not clamped), ``crit`` the mean L1 / smooth-L1 / L2.  ``resize=True`` takes both images to 224 x 224 first (bicubic,
    align_corners).  bf16 compute; differentiable with respect to ``x`` only.  Call ``load_vgg_state_dict`` first."""
    family = "vgg"

    def __init__(self, weights=(1.0, 1.0, 1.0, 1.0, 1.0), resize: bool = False, criterion: str = "l1", data_range: float = 1.0, device=None):
        super().__init__()
        if criterion not in PERCEPTUAL_CRITERIA:
            raise NotImplementedError("Loss [{}] is not implemented".format(criterion))
        weights = [float(w) for w in weights]
        if len(weights) != 5 or not all(math.isfinite(w) for w in weights):
            raise M2TError(f"PerceptualLoss: weights must be five finite numbers (relu1_1 .. relu5_1), got {weights!r}")
        if not (math.isfinite(float(data_range)) and float(data_range) > 0.0):
            raise M2TError(f"PerceptualLoss: data_range must be a finite number > 0, got {data_range!r}")
        self.weights, self.resize, self.criterion, self.data_range = weights, bool(resize), criterion, float(data_range)
        self.kind, self.param = PERCEPTUAL_CRITERIA[criterion]
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        h = C.c_void_p()
        _lib.check(_lib.load().m2t_vgg_create(C.byref(h), _lib.BF16), "m2t_vgg_create")
        self.handle = h
        self.flat = self.packed = None
        self._ws: Dict[tuple, torch.Tensor] = {}

    @property
    def loaded(self) -> bool:
        return self.packed is not None

    def configure(self, weights, criterion: str, resize: bool):
        """Replace the tap weights, the criterion and the resize flag (checkpoint.import_checkpoint); the tower's weights stay."""
        if criterion not in PERCEPTUAL_CRITERIA:
            raise NotImplementedError("Loss [{}] is not implemented".format(criterion))
        weights = [float(w) for w in weights]
        if len(weights) != 5 or not all(math.isfinite(w) for w in weights):
            raise M2TError(f"PerceptualLoss: weights must be five finite numbers (relu1_1 .. relu5_1), got {weights!r}")
        self.weights, self.resize, self.criterion = weights, bool(resize), criterion
        self.kind, self.param = PERCEPTUAL_CRITERIA[criterion]

    def tap_weights(self):
        return (C.c_double * 5)(*self.weights)

    def load_vgg_state_dict(self, sd: Dict[str, torch.Tensor]):
        folded = vgg_fold_state_dict(sd)
        if self.device.type != "cuda":
            raise M2TError("PerceptualLoss needs a HIP device (there is no host implementation)")
        lib = _lib.load()
        flat = torch.zeros(self.query("num_params"), dtype=torch.float32, device=self.device)
        for n, (o, cnt) in self.inventory()[1].items():
            if folded[n].numel() != cnt:
                raise M2TError(f"load_vgg_state_dict: shape mismatch for {n}: {tuple(folded[n].shape)}")
            flat[o:o + cnt].copy_(folded[n].reshape(-1))
        packed = torch.empty(self.query("packed_bytes"), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.m2t_vgg_load_weights(self.handle, _lib.ptr(flat), _lib.ptr(packed), _lib.stream_ptr()), "m2t_vgg_load_weights")
        self.flat, self.packed = flat, packed
        return self

    def workspace(self, B: int, H: int, W: int, want_grad: bool) -> torch.Tensor:
        """The device workspace of one shape, cached."""
        key = (B, H, W, bool(want_grad))
        if key not in self._ws:
            nbytes = _lib.load().m2t_vgg_workspace_bytes(B, H, W, 1 if want_grad else 0)
            if nbytes == 0:
                raise M2TError(f"PerceptualLoss: no workspace for [{B},*,{H},{W}] (height and width at least {_lib.VGG_MIN_SIDE}, B at most 32767)")
            self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws[key]

    def check(self, x, y):
        _pair_check("PerceptualLoss", x, y, device=False)
        if int(x.shape[1]) not in (1, 3):
            raise M2TError(f"PerceptualLoss: 1 or 3 channels, got {int(x.shape[1])}")
        H, W = (224, 224) if self.resize else (int(x.shape[2]), int(x.shape[3]))
        if min(H, W) < _lib.VGG_MIN_SIDE or min(int(x.shape[2]), int(x.shape[3])) < 1:
            raise M2TError(f"PerceptualLoss: image {H}x{W} is too small (height and width must be at least {_lib.VGG_MIN_SIDE}: four pools before relu5_1)")
        if not self.loaded:
            raise M2TError("PerceptualLoss: no VGG19 weights loaded (none ship with the library): call load_vgg_state_dict first")
        _pair_check("PerceptualLoss", x, y)

    def _call(self, x, y, want_grad):
        """(loss [1] float32, gradient or None) of device tensors [B,C,H,W]."""
        lib = _lib.load()
        xc, yc = x.detach().contiguous().float(), y.detach().contiguous().float()
        B, Cn, H, W = xc.shape
        with torch.cuda.device(xc.device):
            st = _lib.stream_ptr()
            xs, ys, Ht, Wt = xc, yc, H, W
            if self.resize:
                Ht = Wt = 224
                xs, ys = torch.empty(B, Cn, 224, 224, dtype=torch.float32, device=xc.device), torch.empty(B, Cn, 224, 224, dtype=torch.float32, device=xc.device)
                _lib.check(lib.m2t_bicubic_resize(_lib.ptr(xc), _lib.ptr(xs), B * Cn, H, W, 224, 224, st), "m2t_bicubic_resize")
                _lib.check(lib.m2t_bicubic_resize(_lib.ptr(yc), _lib.ptr(ys), B * Cn, H, W, 224, 224, st), "m2t_bicubic_resize")
            out = torch.empty(1, dtype=torch.float32, device=xc.device)
            gs = torch.zeros_like(xs) if want_grad else None
            _lib.check(lib.m2t_vgg_loss_tensor(self.handle, _lib.ptr(xs), _lib.ptr(ys), B, Cn, Ht, Wt, Cn * Ht * Wt, Wt, self.data_range, 0,
                                               self.kind, self.param, self.tap_weights(), 1.0, _lib.ptr(gs), _lib.ptr(out), None, 0,
                                               _lib.ptr(self.workspace(B, Ht, Wt, want_grad)), st), "m2t_vgg_loss_tensor")
            grad = gs
            if want_grad and self.resize:
                grad = torch.empty_like(xc)
                _lib.check(lib.m2t_bicubic_resize_backward(_lib.ptr(gs), _lib.ptr(grad), B * Cn, H, W, 224, 224, st), "m2t_bicubic_resize_backward")
        return out, grad

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        self.check(x, y)
        return _EagerGradFn.apply(x, lambda want_grad: self._call(x, y, want_grad))
