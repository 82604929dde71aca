"""
CPU-side checks of the rational-quadratic spline coupling: the float64 restatement the GPU tests measure against (tests/_rqs.py) has the
properties a spline flow needs, the new C-ABI entry points validate their arguments on the host, and the layer / model surface is there.
"""
from types import SimpleNamespace as NS

import pytest
import torch

from tests import _rqs as R

BOUND = 3.0


def _inputs(K, n=512, scale=0.5, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(n, generator=g, dtype=torch.float64)
    raw = scale * torch.randn(n, 3 * K - 1, generator=g, dtype=torch.float64)
    return x, raw


@pytest.mark.parametrize('K', [4, 8, 16])
def test_restatement_logdet_is_the_log_of_the_derivative(K):
    x, raw = _inputs(K)
    x.requires_grad_(True)
    y, ld = R.rqs(x, raw, K, BOUND)
    gx, = torch.autograd.grad(y.sum(), x)
    assert float(gx.min()) > 0.0                                     # monotone
    assert float((gx.log() - ld.detach()).abs().max()) <= 1e-10


@pytest.mark.parametrize('K', [4, 8, 16])
def test_restatement_round_trip(K):
    x, raw = _inputs(K)
    y, ld = R.rqs(x, raw, K, BOUND)
    xi, ldi = R.rqs(y, raw, K, BOUND, inverse=True)
    assert float((xi - x).abs().max()) <= 1e-8
    assert float((ldi + ld).abs().max()) <= 1e-8


@pytest.mark.parametrize('K', [4, 8, 16])
def test_restatement_zero_parameters_are_the_identity(K):
    x, _ = _inputs(K)
    raw = torch.zeros(x.shape[0], 3 * K - 1, dtype=torch.float64)
    y, ld = R.rqs(x, raw, K, BOUND)
    assert float((y - x).abs().max()) <= 1e-12 and float(ld.abs().max()) <= 1e-12
    y32, ld32 = R.rqs(x.float(), raw.float(), K, BOUND)
    assert float((y32 - x.float()).abs().max()) <= 1e-6 and float(ld32.abs().max()) <= 1e-6


@pytest.mark.parametrize('K', [4, 8, 16])
def test_restatement_is_continuous_across_every_knot(K):
    """y and the log-det term on the two sides of each interior knot, and of the two ends of the interval, differ by O(step)"""
    _, raw = _inputs(K, n=64)
    xk = R.knot_values(raw, K, BOUND)                               # (n, K + 1)
    step = 1e-9
    for j in range(K + 1):
        lo, hi = xk[:, j] - step, xk[:, j] + step
        y0, l0 = R.rqs(lo, raw, K, BOUND)
        y1, l1 = R.rqs(hi, raw, K, BOUND)
        assert float((y1 - y0).abs().max()) <= 1e-6, j
        # the two bins of an interior knot share its slope; d_0 = d_K = 1 joins the tails with slope 1
        assert float((l1 - l0).abs().max()) <= 1e-5, j


def test_restatement_tails_are_the_identity():
    K = 8
    _, raw = _inputs(K, n=6)
    x = torch.tensor([-1e3, -3.0000001, -3.0, 3.0, 3.0000001, 1e3], dtype=torch.float64)
    for inverse in (False, True):
        y, ld = R.rqs(x, raw, K, BOUND, inverse=inverse)
        assert torch.equal(y, x) and bool((ld == 0).all())
    x.requires_grad_(True)
    raw.requires_grad_(True)
    y, ld = R.rqs(x, raw, K, BOUND)
    gx, gr = torch.autograd.grad((y * 2.0).sum() + ld.sum(), [x, raw])
    assert bool((gx == 2.0).all()) and bool((gr == 0).all())


def test_layout_helpers_round_trip():
    raw = torch.randn(3, 2, 4, 4, 11)
    assert torch.equal(R.from_channels(R.to_channels(raw), 2), raw)
    raw = torch.randn(5, 3, 23)
    p = R.to_channels(raw)
    assert p.shape == (5, 69) and torch.equal(R.from_channels(p, 3), raw)
    assert float(p[2, 7 * 3 + 1]) == float(raw[2, 1, 7])            # parameter p of channel m at channel p * Ch + m


def test_cabi_argument_errors_without_gpu(pkg):
    pkg.build()
    lib = pkg._native.load()
    f, g = lib.nf_rqs_coupling_fwd, lib.nf_rqs_coupling_bwd
    # (z, params, y, ld, K, bound, mode, odd, inverse, B, C, H, W, stream)
    assert f(None, None, None, None, 5, 3.0, 0, 0, 0, 4, 2, 1, 1, None) == 10002          # bins outside {4, 8, 16}
    assert f(None, None, None, None, 8, 0.0, 0, 0, 0, 4, 2, 1, 1, None) == 10001          # bound <= 0
    assert f(None, None, None, None, 8, -1.0, 0, 0, 1, 4, 2, 1, 1, None) == 10001
    assert f(None, None, None, None, 8, 3.0, 0, 0, 0, 4, 3, 1, 1, None) == 10001          # odd feature count, mode 1D
    assert f(None, None, None, None, 8, 3.0, 3, 0, 0, 4, 2, 1, 1, None) == 10001          # no split: not a coupling
    assert f(None, None, None, None, 8, 3.0, 0, 0, 0, 4, 2, 1, 1, None) == 10001          # NULL pointers with B > 0
    assert f(None, None, None, None, 8, 3.0, 0, 0, 0, 0, 2, 1, 1, None) == 0              # B = 0: nothing to launch
    # (g_y, g_ld, z, params, g_z, g_params, K, bound, mode, odd, B, C, H, W, stream)
    assert g(None, None, None, None, None, None, 7, 3.0, 0, 0, 4, 2, 1, 1, None) == 10002
    assert g(None, None, None, None, None, None, 16, 0.0, 0, 0, 4, 2, 1, 1, None) == 10001
    assert g(None, None, None, None, None, None, 4, 3.0, 0, 1, 4, 5, 1, 1, None) == 10001
    assert g(None, None, None, None, None, None, 4, 3.0, 1, 0, 4, 3, 3, 4, None) == 10001  # checkerboard needs even H and W
    assert g(None, None, None, None, None, None, 4, 3.0, 2, 0, 4, 4, 4, 4, None) == 10001  # NULL pointers with B > 0
    assert g(None, None, None, None, None, None, 4, 3.0, 2, 0, 0, 4, 4, 4, None) == 0


def test_layer_conditioner_widths_and_bins(pkg):
    cond = __import__('importlib').import_module(pkg.__name__ + '.conditioners')
    k = pkg.RQSplineCoupling((2, ), bins=8)
    assert isinstance(k, pkg.AbstractCoupling) and isinstance(k.net, cond.MLP) and k.net.fused
    assert [n for n, _ in k.named_parameters() if not n.startswith('net.')] == []         # no parameters of its own
    assert _out_width(k.net) == 23 and _in_width(k.net) == 1                              # inside MLP.fused's limit of 32 outputs
    k = pkg.RQSplineCoupling((6, ), bins=16, odd=True)
    assert _out_width(k.net) == 3 * 47 and _in_width(k.net) == 3 and not k.net.fused
    k = pkg.RQSplineCoupling((3, 8, 8), 'checkerboard', bins=4)
    assert isinstance(k.net, cond.ConvNet) and _in_width(k.net) == 6 and _out_width(k.net) == 6 * 11
    k = pkg.RQSplineCoupling((4, 4, 4), 'channelwise')
    assert _in_width(k.net) == 2 and _out_width(k.net) == 2 * 23 and k.bins == 8 and k.tail_bound == 3.0
    for bad in (5, 0, 32):
        with pytest.raises(ValueError, match='bins'):
            pkg.RQSplineCoupling((2, ), bins=bad)
    with pytest.raises(ValueError, match='tail_bound'):
        pkg.RQSplineCoupling((2, ), tail_bound=0.0)


def _leaves(net):
    return [m for m in net.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d))]


def _in_width(net):
    m = _leaves(net)[0]
    return m.in_features if isinstance(m, torch.nn.Linear) else m.in_channels


def _out_width(net):
    m = _leaves(net)[-1]
    return m.out_features if isinstance(m, torch.nn.Linear) else m.out_channels


def test_model_builds_and_refuses_cpu_tensors(pkg):
    pkg.build()
    net = pkg.SplineFlow((2, ), '2d', NS(layers=2))
    kinds = [type(m).__name__ for m in net.net.layers]
    assert kinds == ['ActNorm', 'InvertibleConv1x1', 'RQSplineCoupling'] * 2
    assert [m.odd for m in net.net.layers if isinstance(m, pkg.RQSplineCoupling)] == [False, True]
    assert all(m.bins == 8 and m.tail_bound == 3.0 for m in net.net.layers if isinstance(m, pkg.RQSplineCoupling))
    net = pkg.SplineFlow((2, ), '2d', NS(layers=1, bins=16, tail_bound=5.0))
    assert net.net.layers[2].bins == 16 and net.net.layers[2].tail_bound == 5.0
    with pytest.raises(RuntimeError, match='no CPU'):
        net(torch.randn(8, 2))
    with pytest.raises(RuntimeError, match='no CPU'):
        pkg.functional.rqs_coupling(torch.randn(8, 2), torch.randn(8, 23), torch.zeros(8), 8, 3.0, 0, False)
    img = pkg.SplineFlow((3, 8, 8), 'image', NS(layers=1))
    assert sum(isinstance(m, pkg.RQSplineCoupling) for m in img.net.layers) == 2
