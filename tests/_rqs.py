"""
The monotone rational-quadratic spline of Neural Spline Flows (Durkan et al. 2019, eq. 4-8, appendix A.1) restated in torch ops, dtype-generic:
the yard-stick of csrc/rqspline.hip in float64, its float32 twin, and (through torch ops on the device) the layer tests' reference.
There is no reference implementation of this transform; the conventions are the ones nfhip.h states for nf_rqs_coupling_*.

    raw (..., 3K - 1) = rw[0..K) | rh[0..K) | rd[0..K-1)   for an x of shape (...)
"""
import math

import torch
import torch.nn.functional as F

MIN = 1.0e-3
DC = math.log(math.expm1(1.0 - MIN))          # softplus(DC) = 1 - MIN: zero parameters give unit slopes


def knots(raw, K, bound):
    rw, rh, rd = raw[..., :K], raw[..., K:2 * K], raw[..., 2 * K:]
    w = 2 * bound * (MIN + (1 - MIN * K) * torch.softmax(rw, -1))
    h = 2 * bound * (MIN + (1 - MIN * K) * torch.softmax(rh, -1))
    edge = torch.full_like(w[..., :1], bound)
    xk = torch.cat([-edge, -bound + torch.cumsum(w, -1)[..., :-1], edge], -1)       # the last knot is exactly +bound
    yk = torch.cat([-edge, -bound + torch.cumsum(h, -1)[..., :-1], edge], -1)
    one = torch.ones_like(w[..., :1])
    d = torch.cat([one, MIN + F.softplus(rd + DC), one], -1)
    return xk, yk, d


def rqs(x, raw, K, bound=3.0, inverse=False):
    """(y, per-element log-det term): forward log dy/dx, inverse -log dy/dx at the recovered point"""
    xk, yk, d = knots(raw, K, bound)
    inside = (x > -bound) & (x < bound)
    xc = torch.where(inside, x, torch.zeros_like(x))
    kn = yk if inverse else xk
    k = torch.sum(xc[..., None] >= kn[..., 1:-1], -1)[..., None]

    def g(t):
        return t.gather(-1, k)[..., 0]
    x0, y0, d0, d1 = g(xk), g(yk), g(d), g(d[..., 1:])
    W, H = g(xk[..., 1:]) - x0, g(yk[..., 1:]) - y0                                 # knot differences, not the widths
    s = H / W
    if not inverse:
        th = (xc - x0) / W
    else:
        dy = xc - y0
        t = dy * (d1 + d0 - 2 * s)
        a, b, c = H * (s - d0) + t, H * d0 - t, -s * dy
        th = (2 * c / (-b - torch.sqrt(torch.clamp(b * b - 4 * a * c, min=0)))).clamp(0, 1)
    den = s + (d1 + d0 - 2 * s) * th * (1 - th)
    ld = torch.log(s * s * (d1 * th * th + 2 * s * th * (1 - th) + d0 * (1 - th) ** 2)) - 2 * torch.log(den)
    y = x0 + th * W if inverse else y0 + H * (s * th * th + d0 * th * (1 - th)) / den
    return torch.where(inside, y, x), torch.where(inside, -ld if inverse else ld, torch.zeros_like(ld))


def knot_values(raw, K, bound=3.0):
    """the K + 1 x knots (..., K + 1) of each element"""
    return knots(raw, K, bound)[0]


def nudge_off_knots(x, raw, K, bound=3.0, near=1.0e-4, by=3.0e-4):
    """x with every element closer than ``near`` to one of its float64 knots moved by ``by``: the gradient of the log-det term jumps at
    a knot, and two implementations may place an element a few ulp from one in different bins"""
    xk = knot_values(raw.double(), K, bound)
    close = ((x.double()[..., None] - xk).abs() < near).any(-1)
    return torch.where(close, x + by, x), int(close.sum())


def to_channels(raw):
    """(B, Ch, [h, w,] 3K - 1) per-element parameters -> the conditioner layout (B, (3K - 1) Ch, [h, w]): parameter p of channel m at
    channel p Ch + m"""
    P = raw.shape[-1]
    if raw.dim() == 3:
        return raw.permute(0, 2, 1).reshape(raw.shape[0], P * raw.shape[1]).contiguous()
    B, Ch, h, w, _ = raw.shape
    return raw.permute(0, 4, 1, 2, 3).reshape(B, P * Ch, h, w).contiguous()


def from_channels(params, Ch):
    """the inverse of to_channels"""
    B = params.shape[0]
    P = params.shape[1] // Ch
    if params.dim() == 2:
        return params.reshape(B, P, Ch).permute(0, 2, 1)
    return params.reshape(B, P, Ch, params.shape[2], params.shape[3]).permute(0, 2, 3, 4, 1)
