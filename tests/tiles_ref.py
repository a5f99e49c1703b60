"""The restatement of the definitions of include/m2t_tiles.h: the tile grid in plain Python, the gather by slicing, and the blend and the
seam in torch fp64 in exactly the stated order (ky ascending outside, kx ascending inside, each sum starting at 0.0, one IEEE operation
per step) with the single-cover copy.  The covering tiles of a coordinate are found by trying every tile, not by the kernels' index
arithmetic.  Runs on any device."""
import torch

MAX_COVER = 3                                                # tiles that can cover a pixel on one axis


def grid(L: int, T: int, v: int):
    """(tile length, origins) of one axis: LR length L, tile size T >= 1, overlap v with 0 <= 2 v <= T."""
    assert L >= 1 and T >= 1 and 0 <= 2 * v <= T, (L, T, v)
    if L <= T:
        return L, [0]
    S = T - v
    n = -(-(L - T) // S) + 1
    return T, [min(k * S, L - T) for k in range(n)]


def axis_pairs(L: int, T: int, v: int, s: int):
    """(t, origins, pairs): pairs[p] lists, for SR coordinate p, the covering tiles as (k, u, w) with k ascending."""
    t, o = grid(L, T, v)
    n = len(o)
    pairs = []
    for p in range(s * L):
        here = []
        for k in range(n):
            u = p - s * o[k]
            if 0 <= u < s * t:
                a = s * (o[k - 1] + t - o[k]) if k >= 1 else 0
                b = s * (o[k] + t - o[k + 1]) if k <= n - 2 else 0
                w = 1.0
                if a > 0:
                    w = min(w, (u + 0.5) / a)
                if b > 0:
                    w = min(w, (s * t - u - 0.5) / b)
                here.append((k, u, w))
        pairs.append(here)
    return t, o, pairs


def cover(L: int, T: int, v: int):
    """How many tiles cover each LR pixel of one axis."""
    t, o = grid(L, T, v)
    return [sum(1 for ok in o if ok <= q < ok + t) for q in range(L)]


def gather(x: torch.Tensor, T: int, v: int, first: int = 0, count=None) -> torch.Tensor:
    """[B,C,H,W] -> the tiles first .. first + count - 1 of the global order g = (b ny + ky) nx + kx as [count,C,th,tw]."""
    B, C, H, W = x.shape
    (th, oy), (tw, ox) = grid(H, T, v), grid(W, T, v)
    ny, nx = len(oy), len(ox)
    count = B * ny * nx - first if count is None else count
    out = []
    for g in range(first, first + count):
        b, ky, kx = g // (ny * nx), (g // nx) % ny, g % nx
        out.append(x[b, :, oy[ky]:oy[ky] + th, ox[kx]:ox[kx] + tw])
    return torch.stack(out).contiguous()


def crops(sr: torch.Tensor, H: int, W: int, T: int, v: int, s: int) -> torch.Tensor:
    """The SR tiles a pointwise model would give: crops of sr [B,C,s H,s W] at s times the LR tiles."""
    B, C = sr.shape[:2]
    (th, oy), (tw, ox) = grid(H, T, v), grid(W, T, v)
    return torch.stack([sr[b, :, s * y:s * (y + th), s * x:s * (x + tw)] for b in range(B) for y in oy for x in ox]).contiguous()


def _columns(pairs, device):
    """pairs -> (count [P], k [3][P], u [3][P], w [3][P] in fp64); unused slots hold tile 0, u 0, weight 0."""
    P = len(pairs)
    cnt = torch.tensor([len(h) for h in pairs], dtype=torch.int64, device=device)
    assert 1 <= int(cnt.min()) and int(cnt.max()) <= MAX_COVER
    k = torch.zeros(MAX_COVER, P, dtype=torch.int64)
    u = torch.zeros(MAX_COVER, P, dtype=torch.int64)
    w = torch.zeros(MAX_COVER, P, dtype=torch.float64)
    for p, here in enumerate(pairs):
        for m, (kk, uu, ww) in enumerate(here):
            k[m, p], u[m, p], w[m, p] = kk, uu, ww
    return cnt, k.to(device), u.to(device), w.to(device)


def blend(tiles: torch.Tensor, B: int, H: int, W: int, T: int, v: int, s: int):
    """tiles [B ny nx,C,s th,s tw] -> (out float32 [B,C,s H,s W], q / den in fp64, seam float32, single [s H,s W] bool): the header's
    sums, m = num / den, out = (float) m, seam = sqrtf((float)(q / den)); where one tile covers, out = z and seam = 0."""
    dev = tiles.device
    th, oy, py = axis_pairs(H, T, v, s)
    tw, ox, px = axis_pairs(W, T, v, s)
    ny, nx = len(oy), len(ox)
    C = tiles.shape[1]
    assert tuple(tiles.shape) == (B * ny * nx, C, s * th, s * tw), (tuple(tiles.shape), (B * ny * nx, C, s * th, s * tw))
    cy, Ky, Uy, Wy = _columns(py, dev)
    cx, Kx, Ux, Wx = _columns(px, dev)
    single = (cy[:, None] == 1) & (cx[None, :] == 1)
    out = torch.empty(B, C, s * H, s * W, dtype=torch.float32, device=dev)
    var = torch.zeros(B, C, s * H, s * W, dtype=torch.float64, device=dev)
    for b in range(B):
        z, wt, ok = [], [], []
        for a in range(MAX_COVER):
            for e in range(MAX_COVER):
                g = ((b * ny + Ky[a])[:, None] * nx + Kx[e][None, :])
                z.append(tiles[g, :, Uy[a][:, None], Ux[e][None, :]].permute(2, 0, 1))          # [C,s H,s W]
                wt.append(Wy[a][:, None] * Wx[e][None, :])
                ok.append((a < cy)[:, None] & (e < cx)[None, :])
        num = torch.zeros(C, s * H, s * W, dtype=torch.float64, device=dev)
        den = torch.zeros(s * H, s * W, dtype=torch.float64, device=dev)
        for zi, wi, oi in zip(z, wt, ok):
            num = torch.where(oi, num + wi * zi.double(), num)
            den = torch.where(oi, den + wi, den)
        m = num / den
        q = torch.zeros_like(num)
        for zi, wi, oi in zip(z, wt, ok):
            d = zi.double() - m
            q = torch.where(oi, q + wi * (d * d), q)
        out[b] = torch.where(single, z[0], m.float())
        var[b] = torch.where(single, torch.zeros_like(q), q / den)
    return out, var, torch.sqrt(var.float()), single


def tiled(model, lr: torch.Tensor, T: int, v: int, tile_batch: int, s: int, blend_device=None):
    """The hand composition: restated gather -> `model` on the same chunks -> restated blend (on `blend_device` when given), for
    every tensor the model returns; a list of (out, var, seam, single), one per returned tensor."""
    B, _, H, W = lr.shape
    (th, oy), (tw, ox) = grid(H, T, v), grid(W, T, v)
    total = B * len(oy) * len(ox)
    chunks = []
    for first in range(0, total, tile_batch):
        got = model(gather(lr, T, v, first, min(tile_batch, total - first)))
        chunks.append(tuple(got) if isinstance(got, (tuple, list)) else (got,))
    whole = [torch.cat([c[i] for c in chunks]) for i in range(len(chunks[0]))]
    return [blend(t if blend_device is None else t.to(blend_device), B, H, W, T, v, s) for t in whole]


def pointwise_stub(s: int, gain: float = 1.5, offset: float = -0.25):
    """Nearest-neighbour upsampling by s times an affine map: every output element depends on one input element alone, so the
    output of a tile is the crop of the output of the whole image, bit for bit."""
    def up(x: torch.Tensor) -> torch.Tensor:
        y = x.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)
        return (y * gain + offset).contiguous()
    return up
