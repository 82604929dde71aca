"""A compact restatement of the reference's planar flow (flows/planar.py) in plain torch, for any dtype and device: the yardstick of
tests/test_planar_host.py and tests/test_gpu_planar.py (float32 and float64 on the CPU).  Parameters are lists (u, w, b) per layer with
the reference's shapes: u, w (1, D), b (1,)."""
import torch
import torch.nn.functional as F


def project(u, w):
    """PlanarTransform._make_invertible (planar.py:23-33): the projected u (u itself where w.u >= -1)"""
    wu = torch.mm(u, w.t())
    if wu.item() >= -1.0:
        return u
    norm_w = w / torch.norm(w, p=2, dim=1)**2
    return u + (-1.0 + F.softplus(wu) - wu) * norm_w


def _logdet(wu, affine):
    t = torch.tanh(affine)
    det = 1.0 + wu * (1.0 - t * t)
    return torch.sum(torch.log(torch.abs(det) + 1.0e-5), dim=1)


def forward(z, ld, params):
    """planar.py:35-45 over the layers in order; returns (z, ld, the projected u of each layer) -- autograd flows to the projected u
    as in the reference (it assigns ``u.data``): pass leaves that are already projected to differentiate."""
    us = []
    for u, w, b in params:
        with torch.no_grad():
            up = project(u, w)
        if up is not u:
            u = up
        us.append(u)
        wu = torch.mm(u, w.t())
        affine = torch.mm(z, w.t()) + b
        z = z + u * torch.tanh(affine)
        ld = ld + _logdet(wu, affine)
    return z, ld, us


def bisect(wz, wu, b, max_iter=100):
    """planar.py:50-61: (lo, hi, iterations run) with the batch-global exit"""
    lo = torch.full_like(wz, -1.0e3)
    hi = torch.full_like(wz, 1.0e3)
    n = max_iter
    for it in range(max_iter):
        mid = (lo + hi) * 0.5
        val = mid + wu * torch.tanh(mid + b)
        lo = torch.where(val < wz, mid, lo)
        hi = torch.where(val > wz, mid, hi)
        if torch.all(torch.abs(hi - lo) < 1.0e-5):
            n = it + 1
            break
    return lo, hi, n


def inverse(z, ld, params):
    """planar.py:47-68 over the layers in reverse; returns (z, ld, iteration count per layer in layer order).  The midpoint is a
    constant of the graph (torch.where over constants), as in the reference."""
    iters = [0] * len(params)
    for k in range(len(params) - 1, -1, -1):
        u, w, b = params[k]
        wz = torch.mm(z, w.t())
        wu = torch.mm(u, w.t())
        with torch.no_grad():
            lo, hi, iters[k] = bisect(wz.detach(), wu.detach(), b.detach())
        affine = (lo + hi) * 0.5 + b
        z = z - u * torch.tanh(affine)
        ld = ld - _logdet(wu, affine)
    return z, ld, iters


def params_of(state, K, dtype=torch.float64, requires_grad=False):
    """[(u, w, b)] of a PlanarFlow state_dict (keys net.layers.{i}.u / .w / .b)"""
    out = []
    for i in range(K):
        p = []
        for n in ('u', 'w', 'b'):
            t = state['net.layers.%d.%s' % (i, n)].detach().clone().to(dtype)
            p.append(t.requires_grad_(requires_grad))
        out.append(tuple(p))
    return out


def nll(z, ld):
    """main.py:85 written out: -mean(log N(z; 0, I) + ld)"""
    D = z.shape[1]
    return -torch.mean(-0.5 * (z * z).sum(1) - 0.5 * D * torch.log(torch.tensor(2 * torch.pi, dtype=z.dtype)) + ld)
