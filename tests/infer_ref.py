"""The torch restatement of the definitions of include/m2t_infer.h, in exactly the stated order: the eight views, their inverses, the
mean, the variance, the spread and the 8-bit export.  Runs on any device; every operation is an elementwise fp32 torch operation
(no fused multiply-add), so the mean and the variance are the bits the kernels must give.

View k = 4 t + 2 v + h of a plane x[H,W]: y[i,j] = x[v ? H-1-i : i, h ? W-1-j : j]; V_k(x) = y for t = 0, the transpose of y for
t = 1.  Inverse on an output z_k: u = z_k (t = 0) or its transpose (t = 1), then the same flips.  All functions take [..., H, W]."""
import torch


def _flips(y: torch.Tensor, v: int, h: int) -> torch.Tensor:
    if v:
        y = y.flip(-2)
    if h:
        y = y.flip(-1)
    return y


def view(x: torch.Tensor, k: int) -> torch.Tensor:
    t, v, h = k >> 2, (k >> 1) & 1, k & 1
    y = _flips(x, v, h)
    return (y.transpose(-1, -2) if t else y).contiguous()


def inverse(z: torch.Tensor, k: int) -> torch.Tensor:
    t, v, h = k >> 2, (k >> 1) & 1, k & 1
    u = z.transpose(-1, -2) if t else z                     # un-transpose first
    return _flips(u, v, h).contiguous()                      # then the same flips


def pack(x: torch.Tensor):
    """[N,C,H,W] -> (a [4N,C,H,W], b [4N,C,W,H]): view k of image n at batch index (k mod 4) N + n."""
    return torch.cat([view(x, k) for k in range(4)]), torch.cat([view(x, k) for k in range(4, 8)])


def unpack(a: torch.Tensor, b: torch.Tensor) -> list:
    """The eight U_k [N,C,Hs,Ws] of the outputs a [4N,C,Hs,Ws] and b [4N,C,Ws,Hs]."""
    n = a.shape[0] // 4
    return [inverse(a[k * n:(k + 1) * n], k) for k in range(4)] + [inverse(b[k * n:(k + 1) * n], 4 + k) for k in range(4)]


def merge(a: torch.Tensor, b: torch.Tensor):
    """(mean, var, spread) of the eight outputs, fp32, in the order of the header."""
    U = [u.float() for u in unpack(a, b)]
    eighth = torch.tensor(0.125, dtype=torch.float32, device=a.device)
    mean = (((U[0] + U[1]) + (U[2] + U[3])) + ((U[4] + U[5]) + (U[6] + U[7]))) * eighth
    d = [u - mean for u in U]
    q = [t * t for t in d]
    var = (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) * eighth
    return mean, var, torch.sqrt(var)


def ensemble(model, x: torch.Tensor):
    """The self-ensemble of `model` on x [B,3,H,W] with torch operations alone: one call on [8B,3,H,H] for a square input, else two
    ([4B,3,H,W], then [4B,3,W,H]); returns (mean, var, spread)."""
    a, b = pack(x)
    if x.shape[-1] == x.shape[-2]:
        out = model(torch.cat([a, b]))
        sa, sb = out[:a.shape[0]], out[a.shape[0]:]
    else:
        sa, sb = model(a), model(b)
    return merge(sa, sb)


def nearest_up(s: int):
    """The equivariant stub: nearest-neighbour upsampling by s (repeat_interleave on both axes).  It commutes with every flip and
    with the transpose, so its self-ensemble is its own output, bit for bit, and the spread is exactly 0."""
    def up(x: torch.Tensor) -> torch.Tensor:
        return x.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1).contiguous()
    return up


def export_u8(src: torch.Tensor, rgb_range: float = 1.0) -> torch.Tensor:
    """[C,H,W] float32 -> [H,W,C] uint8: (uint8) min(max(src * s + 0.5f, 0.f), 255.f), s = 255.0f / rgb_range in fp32, the cast
    truncating; a NaN becomes 0."""
    s = torch.tensor(255.0, dtype=torch.float32, device=src.device) / torch.tensor(rgb_range, dtype=torch.float32, device=src.device)
    t = src.float() * s + torch.tensor(0.5, dtype=torch.float32, device=src.device)
    t = torch.where(t.isnan(), torch.zeros_like(t), t.clamp(0.0, 255.0))
    return t.to(torch.int32).to(torch.uint8).permute(1, 2, 0).contiguous()
