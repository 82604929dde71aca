"""
Host-side checks of the autoregressive spline (layers.AutoregressiveSpline, csrc/arspline.hip): the masks, the autoregressive structure of
the float64 restatement (tests/_arspline.py) with the layer's masks, the identity start, the inverse's pass structure, constructor errors,
the state_dict, and the C ABI's argument checks -- none of which needs a GPU.
"""
import copy
import importlib

import numpy as np
import pytest
import torch

from tests import _arspline as A


def _randomised(pkg, D, bins=8, seed=0):
    """a float64 layer with RANDOM head parameters (the constructor's are zero)"""
    torch.manual_seed(seed)
    layer = pkg.AutoregressiveSpline(D, bins=bins).double()
    with torch.no_grad():
        layer.head_weight.copy_(0.18 * torch.randn_like(layer.head_weight))
        layer.head_bias.copy_(0.5 * torch.randn_like(layer.head_bias))
    return layer


@pytest.mark.parametrize('D', [1, 2, 3, 8])
def test_masks_are_made_masks_of_the_stated_degrees(pkg, D):
    cond = importlib.import_module(pkg.__name__ + '.conditioners')
    layer = pkg.AutoregressiveSpline(D)
    want = cond.made_masks_from_degrees(D, [np.arange(32) % max(1, D - 1)] * 3)
    got = layer.masks
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape and np.array_equal(g.numpy(), w)
    assert tuple(layer.head_mask.shape) == (D, 32) and float(layer.head_mask[0].abs().sum()) == 0.0      # feature 0: the bias alone
    assert not layer.masks_redrawn_per_call
    assert dict(layer.named_buffers()).keys() >= {'perm', 'mask0', 'mask1', 'mask2', 'head_mask'}
    assert tuple(layer.head_weight.shape) == (23 * D, 32) and tuple(layer.head_bias.shape) == (23 * D, )
    assert not isinstance(layer, pkg.AutoregressiveTransfrom)


@pytest.mark.parametrize('D', [1, 2, 3, 8])
def test_jacobian_is_lower_triangular_in_permuted_order(pkg, D):
    layer = _randomised(pkg, D, seed=D)
    g = torch.Generator().manual_seed(10 + D)
    for row in range(4):
        zp = 1.5 * torch.randn(D, dtype=torch.float64, generator=g)
        J = torch.autograd.functional.jacobian(lambda v: A.layer_forward_permuted(layer, v[None], torch.zeros(1, dtype=v.dtype))[0][0], zp)
        assert tuple(J.shape) == (D, D)
        assert bool((torch.triu(J, diagonal=1) == 0).all()), J                    # exactly zero: d y_i / d z_j for j > i
        assert bool((torch.diagonal(J) > 0).all()), J
        if D > 1:
            assert float(torch.tril(J, diagonal=-1).abs().max()) > 0              # (and the conditioner is not a constant)


@pytest.mark.parametrize('D', [1, 3, 8])
def test_zero_head_is_the_identity(pkg, D):
    torch.manual_seed(1)
    layer = pkg.AutoregressiveSpline(D).double()
    z = 2.0 * torch.randn(64, D, dtype=torch.float64)
    with torch.no_grad():
        y, ld = A.layer_forward(layer, z, torch.zeros(64, dtype=torch.float64))
    assert float((y - torch.mm(z, layer.perm)).abs().max()) <= 1e-12
    assert float(ld.abs().max()) <= 1e-12


@pytest.mark.parametrize('D', [1, 2, 3, 8])
@pytest.mark.parametrize('bins', [4, 8, 16])
def test_inverse_pass_structure_round_trips(pkg, D, bins):
    layer = _randomised(pkg, D, bins=bins, seed=20 + D + bins)
    g = torch.Generator().manual_seed(D + bins)
    z = 2.0 * torch.randn(200, D, dtype=torch.float64, generator=g)
    zero = torch.zeros(200, dtype=torch.float64)
    with torch.no_grad():
        y, ld = A.layer_forward(layer, z, zero)
        x, ldi = A.layer_inverse(layer, y, ld)
    assert float((x - z).abs().max()) <= 1e-10
    assert float(ldi.abs().max()) <= 1e-10                                        # the two directions' log-dets cancel


def test_constructor_errors(pkg):
    for kw in (dict(bins=5), dict(bins=0), dict(tail_bound=0.0), dict(tail_bound=-1.0)):
        with pytest.raises(ValueError):
            pkg.AutoregressiveSpline(4, **kw)
    for D in (0, 9, 16):
        with pytest.raises(ValueError):
            pkg.AutoregressiveSpline(D)
    with pytest.raises(ValueError):
        pkg.AutoregressiveSpline(4, base_filters=64)
    from types import SimpleNamespace as NS
    with pytest.raises(NotImplementedError):
        pkg.SplineMAF((3, 8, 8), 'image', NS(layers=1))
    net = pkg.SplineMAF((3, ), '2d', NS(layers=2, bins=4, tail_bound=2.0))
    kinds = [type(m).__name__ for m in net.net.layers]
    assert kinds == ['BatchNorm', 'AutoregressiveSpline'] * 2
    assert net.net.layers[1].bins == 4 and net.net.layers[1].tail_bound == 2.0
    assert pkg.SplineMAF((3, ), '2d', NS(layers=1)).net.layers[1].bins == 8


def test_state_dict_round_trip(pkg):
    a = _randomised(pkg, 5, seed=3).float()
    torch.manual_seed(99)
    b = pkg.AutoregressiveSpline(5)
    assert not torch.equal(a.perm, b.perm) or not torch.equal(a.weights[0], b.weights[0])
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    assert a.state_dict().keys() == b.state_dict().keys()
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    z = torch.randn(16, 5)
    ya, la = A.layer_forward(a, z, torch.zeros(16))
    yb, lb = A.layer_forward(b, z, torch.zeros(16))
    assert torch.equal(ya, yb) and torch.equal(la, lb)


def test_no_cpu_path(pkg):
    layer = pkg.AutoregressiveSpline(3)
    with pytest.raises(RuntimeError, match='no CPU'):
        layer(torch.randn(4, 3), torch.zeros(4))
    with pytest.raises(RuntimeError, match='no CPU'):
        layer.backward(torch.randn(4, 3), torch.zeros(4))


def test_cabi_argument_checks_without_gpu(pkg):
    """everything here returns on the host before any launch"""
    pkg.build()
    lib = pkg._native.load()
    BAD, UNSUP = 10001, 10002
    assert [lib.nf_arspline_usable(D, 8, 32) for D in (0, 1, 8, 9)] == [0, 1, 1, 0]
    assert [lib.nf_arspline_usable(4, K, 32) for K in (4, 5, 8, 16, 32)] == [1, 0, 1, 1, 0]
    assert lib.nf_arspline_usable(4, 8, 64) == 0
    rows = pkg._native.header_constant('NF_ARS_ROWS')
    cap = pkg._native.header_constant('NF_ARS_MAX_SLABS')
    assert [lib.nf_arspline_head_slabs(B) for B in (0, 1, rows, rows + 1, 777, 10 ** 7)] == [0, 1, 1, 2, -(-777 // rows), cap]

    def fwd(K=8, bound=3.0, inverse=0, col=-1, B=4, D=4, H=32):
        return lib.nf_arspline_head_fwd(None, None, None, None, None, None, None, K, bound, inverse, col, B, D, H, None)

    def bwd(K=8, bound=3.0, B=4, D=4, H=32):
        return lib.nf_arspline_head_bwd(None, None, None, None, None, None, None, None, None, None, None, K, bound, B, D, H, None)

    assert fwd(D=9) == UNSUP and fwd(K=5) == UNSUP and fwd(H=16) == UNSUP and fwd(D=0) == UNSUP
    assert bwd(D=9) == UNSUP and bwd(K=5) == UNSUP and bwd(H=16) == UNSUP
    assert fwd(bound=0.0) == BAD and fwd(bound=-1.0) == BAD and bwd(bound=0.0) == BAD
    assert fwd(inverse=1, col=-1) == BAD and fwd(inverse=1, col=4) == BAD         # a column the inverse does not have
    assert fwd(inverse=0, col=0) == BAD                                           # a column the forward does not take
    assert fwd(B=-1) == BAD and bwd(B=-1) == BAD
    assert fwd() == BAD and fwd(inverse=1, col=0) == BAD and bwd() == BAD         # NULL pointers with B > 0
    assert fwd(B=0) == 0 and fwd(B=0, inverse=1, col=3) == 0 and bwd(B=0) == 0    # an empty batch launches nothing
