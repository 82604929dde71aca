"""
The rational-quadratic spline coupling on the device (csrc/rqspline.hip) against its restatement in torch ops (tests/_rqs.py), which runs
on the CPU in float32 and in float64 on the same inputs.  Bars follow tests/test_gpu_ops.py:

    bar(want32, want64) = TOL max(1, max |want32|) + SLACK max |want32 - want64|

Parity inputs: x = 2 randn (about 13 % of the elements in the linear tails), raw parameters 0.5 randn, fixed seeds; every element closer
than 1e-4 to one of its float64 knots is moved by 3e-4 first (the gradient of the log-det term jumps at a knot, and two implementations
may place an element a few ulp from one in different bins), so no element is excluded anywhere.  Needs a real MI355X.
"""
import copy
import functools
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import indexmaps as IM
from tests import _rqs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-5
SLACK = 4.0
BOUND = 3.0
MODES = {'1d': IM.MODE_1D, 'checkerboard': IM.MODE_CHECKER, 'channelwise': IM.MODE_CHANNEL}


def bar(want32, want64):
    want32, want64 = want32.detach().double().cpu(), want64.detach().double().cpu()
    return TOL * max(1.0, float(want32.abs().max())) + SLACK * float((want32 - want64).abs().max())


def held(got, want32, want64, what):
    err = float((got.detach().double().cpu() - want32.detach().double().cpu()).abs().max())
    lim = bar(want32, want64)
    print('%-28s err %.3e  bar %.3e  (fp32-fp64 gap %.3e)' % (what, err, lim, (lim - TOL * max(1.0, float(want32.abs().max()))) / SLACK))
    assert err <= lim, '%s: max abs err %.3e over the bar %.3e' % (what, err, lim)


def restated(z, params, ld, K, mode, odd, inverse=False, bound=BOUND):
    """the coupling in torch ops, any dtype and device: split, spline on the transformed half, merge, log-det"""
    z0, z1 = IM.split(z, mode, odd)
    y0, l = R.rqs(z0, R.from_channels(params, z0.shape[1]), K, bound, inverse=inverse)
    return IM.merge(y0, z1, mode, odd, tuple(z.shape[1:])), ld + l.reshape(l.shape[0], -1).sum(1)


CASES = [((2, ), '1d', 257, K) for K in (4, 8, 16)] + [((4, ), '1d', 64, K) for K in (4, 8, 16)] + [((6, ), '1d', 33, K) for K in (4, 8, 16)] + \
        [((3, 8, 8), 'checkerboard', 3, 8), ((4, 4, 4), 'channelwise', 5, 8), ((12, 4, 4), 'channelwise', 2, 8), ((3, 8, 8), 'checkerboard', 3, 4)]


def _inputs(dims, masking, B, K, odd, seed=0, scale=0.5):
    """float32 CPU inputs of one case: z (nudged off the knots), params in the conditioner layout, ld0, and the upstream gradients"""
    mode = MODES[masking]
    g = torch.Generator().manual_seed(seed + 1000 * K + sum(dims) + 7 * int(odd))
    z = 2.0 * torch.randn((B, ) + tuple(dims), generator=g)
    z0, z1 = IM.split(z, mode, odd)
    raw = scale * torch.randn(tuple(z0.shape) + (3 * K - 1, ), generator=g)
    z0, moved = R.nudge_off_knots(z0, raw, K, BOUND)
    z = IM.merge(z0, z1, mode, odd, dims).contiguous()
    ld0 = torch.randn(B, generator=g)
    g_y, g_ld = torch.randn(z.shape, generator=g), torch.randn(B, generator=g)
    return mode, z, R.to_channels(raw), ld0, g_y, g_ld, moved


@functools.lru_cache(maxsize=None)
def reference(dims, masking, B, K, odd):
    """the CPU restatement of one case in float32 and float64, computed once: forward, gradients, inverse of its own y"""
    mode, z, params, ld0, g_y, g_ld, moved = _inputs(dims, masking, B, K, odd)
    out = {'moved': moved}
    for dt in (torch.float32, torch.float64):
        zz, pp = z.to(dt).clone().requires_grad_(True), params.to(dt).clone().requires_grad_(True)
        y, ld = restated(zz, pp, ld0.to(dt), K, mode, odd)
        gz, gp = torch.autograd.grad([y, ld], [zz, pp], [g_y.to(dt), g_ld.to(dt)])
        xi, ldi = restated(y.detach(), pp.detach(), ld.detach(), K, mode, odd, inverse=True)
        out[dt] = dict(y=y.detach(), dld=(ld - ld0.to(dt)).detach(), gz=gz, gp=gp, rt=float((xi - zz.detach()).abs().max()))
    return out


@pytest.mark.parametrize('odd', [False, True])
@pytest.mark.parametrize('dims,masking,B,K', CASES)
def test_op_parity(pkg, dims, masking, B, K, odd):
    NF = pkg.functional
    mode, z, params, ld0, g_y, g_ld, moved = _inputs(dims, masking, B, K, odd)
    ref = reference(dims, masking, B, K, odd)
    w32, w64 = ref[torch.float32], ref[torch.float64]
    assert moved <= 8, moved
    zd, pd = z.to(DEV).requires_grad_(True), params.to(DEV).requires_grad_(True)
    ld_in = ld0.to(DEV).clone()
    y, ld = NF.rqs_coupling(zd, pd, ld_in, K, BOUND, mode, odd)
    assert ld.data_ptr() == ld_in.data_ptr()                                      # ld0 + the sums, in place
    held(y, w32['y'], w64['y'], 'y')
    held(ld.detach().cpu() - ld0, w32['dld'], w64['dld'], 'ld increment')
    gz, gp = torch.autograd.grad([y, ld], [zd, pd], [g_y.to(DEV), g_ld.to(DEV)])
    held(gz, w32['gz'], w64['gz'], 'g_z')
    held(gp, w32['gp'], w64['gp'], 'g_params')
    # the inverse of the DEVICE's y against the restatement's inverse of that same y
    yd = y.detach()
    ld_mid = ld.detach().clone()
    x, ldi = NF.rqs_coupling(yd, pd.detach(), ld_mid.clone(), K, BOUND, mode, odd, inverse=True)
    i32 = restated(yd.cpu(), params, ld_mid.cpu(), K, mode, odd, inverse=True)
    i64 = restated(yd.cpu().double(), params.double(), ld_mid.cpu().double(), K, mode, odd, inverse=True)
    held(x, i32[0], i64[0], 'inverse x')
    held(ldi.cpu() - ld_mid.cpu(), i32[1] - ld_mid.cpu(), i64[1] - ld_mid.cpu().double(), 'inverse ld increment')
    rt = float((x.cpu() - z).abs().max())
    print('round trip %.3e (float32 restatement %.3e)' % (rt, w32['rt']))
    assert rt <= 2e-5 + SLACK * w32['rt']


@pytest.mark.parametrize('K', [4, 8, 16])
def test_edges(pkg, K):
    """x exactly at +-bound, one float either side of them, at +-1e3 and at the float32 value of every float64 knot"""
    NF = pkg.functional
    g = torch.Generator().manual_seed(5 + K)
    b = np.float32(BOUND)
    fixed = [b, -b, np.nextafter(b, np.float32(4)), np.nextafter(-b, np.float32(-4)), np.float32(1e3), np.float32(-1e3),
             np.nextafter(b, np.float32(0)), np.nextafter(-b, np.float32(0))]
    n_out, B = 6, 8 + (K - 1)
    raw = 0.5 * torch.randn(B, 1, 3 * K - 1, generator=g)
    xk = R.knot_values(raw.double(), K, BOUND)[:, 0]                              # (B, K + 1)
    x = torch.tensor(np.array(fixed, dtype=np.float32))
    x = torch.cat([x, torch.stack([xk[8 + j - 1, j] for j in range(1, K)]).float()])
    z = torch.stack([x, torch.randn(B, generator=g)], 1).contiguous()             # feature 0 is transformed (odd = False)
    params, ld0 = R.to_channels(raw), torch.randn(B, generator=g)
    g_y, g_ld = torch.randn(B, 2, generator=g), torch.randn(B, generator=g)
    zd, pd = z.to(DEV).requires_grad_(True), params.to(DEV).requires_grad_(True)
    y, ld = NF.rqs_coupling(zd, pd, ld0.to(DEV).clone(), K, BOUND, IM.MODE_1D, False)
    gz, gp = torch.autograd.grad([y, ld], [zd, pd], [g_y.to(DEV), g_ld.to(DEV)])
    y, ld, gz, gp = y.detach().cpu(), ld.detach().cpu(), gz.cpu(), gp.cpu()
    assert torch.equal(y[:n_out].view(torch.int32), z[:n_out].view(torch.int32))            # outside: bit for bit
    assert torch.equal(ld[:n_out].view(torch.int32), ld0[:n_out].view(torch.int32))
    assert bool((gp[:n_out] == 0).all()) and torch.equal(gz[:n_out], g_y[:n_out])
    assert torch.equal(y[:, 1], z[:, 1]) and torch.equal(gz[n_out:, 1], g_y[n_out:, 1])     # the pass-through half
    w32 = restated(z, params, ld0, K, IM.MODE_1D, False)
    w64 = restated(z.double(), params.double(), ld0.double(), K, IM.MODE_1D, False)
    held(y[n_out:], w32[0][n_out:], w64[0][n_out:], 'y at knots and ends')
    held(ld[n_out:] - ld0[n_out:], w32[1][n_out:] - ld0[n_out:], w64[1][n_out:] - ld0[n_out:].double(), 'ld at knots and ends')
    # the same points through the inverse: outside passes through, inside stays inside
    xi, ldi = NF.rqs_coupling(z.to(DEV), params.to(DEV), ld0.to(DEV).clone(), K, BOUND, IM.MODE_1D, False, inverse=True)
    xi, ldi = xi.cpu(), ldi.cpu()
    assert torch.equal(xi[:n_out].view(torch.int32), z[:n_out].view(torch.int32)) and torch.equal(ldi[:n_out].view(torch.int32), ld0[:n_out].view(torch.int32))
    assert bool((xi[n_out:, 0].abs() <= BOUND).all()) and bool(torch.isfinite(ldi).all())


@pytest.mark.parametrize('dims,masking,B', [((2, ), '1d', 300), ((6, ), '1d', 17), ((3, 8, 8), 'checkerboard', 2)])
@pytest.mark.parametrize('K', [4, 8, 16])
def test_zero_parameters_are_the_identity(pkg, dims, masking, B, K):
    NF = pkg.functional
    mode = MODES[masking]
    torch.manual_seed(3)
    z = (2.0 * torch.randn((B, ) + dims)).to(DEV)
    half = NF._half_shape(z, mode)
    n = int(np.prod(half[1:]))
    params = torch.zeros((B, (3 * K - 1) * half[1]) + tuple(half[2:]), device=DEV)
    for inverse in (False, True):
        y, ld = NF.rqs_coupling(z, params, torch.zeros(B, device=DEV), K, BOUND, mode, False, inverse=inverse)
        print('zero parameters, inverse %d: |y - x| %.3e, |ld| %.3e (n = %d)' % (inverse, float((y - z).abs().max()), float(ld.abs().max()), n))
        assert float((y - z).abs().max()) <= 1e-6
        assert float(ld.abs().max()) <= 1e-6 * n


@pytest.mark.parametrize('dims,masking,B', [((2, ), '1d', 2048), ((4, 4, 4), 'channelwise', 16)])
def test_extreme_parameters_stay_finite(pkg, dims, masking, B):
    """raw parameters 3 randn at K = 16: no accuracy bar (the float32 restatement's own round trip is 0.2 off there, by conditioning);
    every output and gradient is finite and the inverse of an inside point stays inside"""
    NF = pkg.functional
    mode, K = MODES[masking], 16
    torch.manual_seed(11)
    z = (2.0 * torch.randn((B, ) + dims)).to(DEV).requires_grad_(True)
    half = NF._half_shape(z, mode)
    params = (3.0 * torch.randn((B, (3 * K - 1) * half[1]) + tuple(half[2:]))).to(DEV).requires_grad_(True)
    y, ld = NF.rqs_coupling(z, params, torch.zeros(B, device=DEV), K, BOUND, mode, True)
    gz, gp = torch.autograd.grad([y, ld], [z, params], [torch.randn_like(y), torch.randn_like(ld)])
    x, ldi = NF.rqs_coupling(y.detach(), params.detach(), ld.detach().clone(), K, BOUND, mode, True, inverse=True)
    for name, t in (('y', y), ('ld', ld), ('g_z', gz), ('g_params', gp), ('x', x), ('ld inverse', ldi)):
        assert bool(torch.isfinite(t).all()), name
    y0 = IM.split(y.detach(), mode, True)[0]
    x0 = IM.split(x, mode, True)[0]
    inside = y0.abs() < BOUND
    assert bool((x0[inside].abs() <= BOUND).all())
    assert torch.equal(x0[~inside], y0[~inside])


def test_same_bits_twice(pkg):
    """the log-det sums and the gradients use no float atomics: two runs from the same inputs agree bit for bit with the ordered mode off"""
    NF, N = pkg.functional, pkg._native
    N.load()
    was = N.deterministic()
    N.deterministic(False)
    try:
        dims, K, B = (12, 4, 4), 8, 2
        for d, masking in ((dims, 'channelwise'), ((2, ), '1d'), ((3, 32, 32), 'checkerboard')):
            mode = MODES[masking]
            torch.manual_seed(2)
            z = (2.0 * torch.randn((B, ) + d)).to(DEV)
            half = NF._half_shape(z, mode)
            params = (0.5 * torch.randn((B, (3 * K - 1) * half[1]) + tuple(half[2:]))).to(DEV)
            g_y, g_ld = torch.randn_like(z), torch.randn(B, device=DEV)
            runs = []
            for _ in range(2):
                zz, pp = z.clone().requires_grad_(True), params.clone().requires_grad_(True)
                y, ld = NF.rqs_coupling(zz, pp, torch.ones(B, device=DEV), K, BOUND, mode, False)
                gz, gp = torch.autograd.grad([y, ld], [zz, pp], [g_y, g_ld])
                xi, ldi = NF.rqs_coupling(y.detach(), pp.detach(), torch.ones(B, device=DEV), K, BOUND, mode, False, inverse=True)
                runs.append((y.detach(), ld.detach(), gz, gp, xi, ldi))
            for a, b in zip(*runs):
                assert torch.equal(a, b), masking
    finally:
        N.deterministic(was)


# ---- layer -------------------------------------------------------------------------------------------------------------------------
def _layer_restated(layer, z, ld):
    """the layer in torch ops, on whatever device and dtype its parameters have: module-by-module conditioner + the restatement"""
    z1 = IM.split(z, layer.mode, layer.odd)[1]
    params = layer.net.forward_reference(z1.contiguous())
    return restated(z, params, ld, layer.bins, layer.mode, layer.odd, bound=layer.tail_bound)


@pytest.mark.parametrize('dims,masking,B', [((2, ), 'checkerboard', 200), ((4, 4, 4), 'channelwise', 6)])
def test_layer_against_restatement(pkg, dims, masking, B):
    torch.manual_seed(4)
    layer = pkg.RQSplineCoupling(dims, masking, bins=8).train()
    l64 = copy.deepcopy(layer).double()
    l32 = copy.deepcopy(layer).to(DEV)
    layer = layer.to(DEV)
    z = 1.5 * torch.randn((B, ) + dims)
    ld0, g_y, g_ld = torch.randn(B), torch.randn((B, ) + dims), torch.randn(B)
    outs = []
    for net, dev, dt, fn in ((layer, DEV, torch.float32, lambda z, ld: layer(z, ld)), (l32, DEV, torch.float32, lambda z, ld: _layer_restated(l32, z, ld)),
                             (l64, 'cpu', torch.float64, lambda z, ld: _layer_restated(l64, z, ld))):
        zz = z.to(dev, dt).requires_grad_(True)
        y, ld = fn(zz, ld0.to(dev, dt).clone())
        ((y * g_y.to(dev, dt)).sum() + (ld * g_ld.to(dev, dt)).sum()).backward()
        outs.append(dict(y=y.detach(), dld=ld.detach().cpu() - ld0.to(dt), gz=zz.grad, **{'grad ' + k: p.grad for k, p in net.named_parameters()}))
    got, w32, w64 = outs
    assert set(got) == set(w32) == set(w64) and len(got) > 6
    for k in got:
        if w32[k] is None and w64[k] is None:                                     # (a parameter nothing depends on)
            assert got[k] is None, k
            continue
        held(got[k], w32[k], w64[k], k)


# ---- model and trainer -------------------------------------------------------------------------------------------------------------
def _walk_restated(net, y, inverse=False):
    """the model layer by layer in float32 on the device: ActNorm and the 1x1 convolution through their own calls, every spline coupling
    through the restatement"""
    ld = torch.zeros(y.shape[0], device=y.device)
    layers = list(net.net.layers)
    with torch.no_grad():
        for m in (reversed(layers) if inverse else layers):
            if type(m).__name__ == 'RQSplineCoupling':
                z1 = IM.split(y, m.mode, m.odd)[1]
                y, ld = restated(y, m.net.forward_reference(z1.contiguous()), ld, m.bins, m.mode, m.odd, inverse=inverse, bound=m.tail_bound)
            else:
                y, ld = (m.backward if inverse else m)(y.contiguous(), ld)
    return y, ld


def test_model_round_trip(pkg):
    torch.manual_seed(6)
    net = pkg.SplineFlow((2, ), '2d', NS(layers=4)).to(DEV)
    y = torch.randn(512, 2, device=DEV)
    net.train()
    with torch.no_grad():
        net(y)                                                                    # data-dependent ActNorm initialisation
    net.eval()
    with torch.no_grad():
        z, ld = net(y)
        x, ldi = net.backward(z)
    zr, ldr = _walk_restated(net, y)
    xr, _ = _walk_restated(net, zr, inverse=True)
    rt, rt_ref = float((x - y).abs().max()), float((xr - y).abs().max())
    # measured on an MI355X: round trip 8.1e-06, the restatement's 3.7e-06, |z - z_restated| 6.3e-06
    print('SplineFlow layers=4 round trip %.3e, layer-by-layer float32 restatement %.3e; |z - z_restated| %.3e' %
          (rt, rt_ref, float((z - zr).abs().max())))
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ld).all()) and bool(torch.isfinite(ldi).all())
    assert rt <= max(2e-5, SLACK * rt_ref)
    assert float((ld + ldi).abs().max()) <= 1e-3 * max(1.0, float(ld.abs().max()))  # the two directions' log-dets cancel


def test_image_model_runs_both_ways(pkg):
    """the shared multi-scale recipe on (3, 8, 8): forward, gradients and inverse run and are finite in training and in evaluation mode;
    the evaluation-mode round trip is held to the layer-by-layer restatement's as in test_model_round_trip.  (Pixels stay inside
    [0.05, 0.95]: the model's Logit(0.01) clamps to [0.01, 0.99] on the way in, modules.py:147, which no inverse undoes.)"""
    torch.manual_seed(7)
    net = pkg.SplineFlow((3, 8, 8), 'image', NS(layers=1)).to(DEV).train()
    y = 0.05 + 0.9 * torch.rand(4, 3, 8, 8, device=DEV)
    z, ld = net(y)
    (z.square().sum() + ld.sum()).backward()
    assert z.shape == y.shape and ld.shape == (4, ) and bool(torch.isfinite(z).all()) and bool(torch.isfinite(ld).all())
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert len(grads) > 20 and all(bool(torch.isfinite(g).all()) for g in grads)
    for mode in ('train', 'eval'):
        getattr(net, mode)()
        with torch.no_grad():
            z, ld = net(y)
            x, ldi = net.backward(z)
        assert x.shape == y.shape and bool(torch.isfinite(z).all()) and bool(torch.isfinite(ld).all())
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(ldi).all())
        rt = float((x - y).abs().max())
        print('image SplineFlow, %s mode: round trip %.3e' % (mode, rt))
    zr, _ = _walk_restated(net, y)
    xr, _ = _walk_restated(net, zr, inverse=True)
    rt_ref = float((xr - y).abs().max())
    print('layer-by-layer float32 restatement, eval mode: round trip %.3e' % rt_ref)
    assert rt <= max(2e-5, SLACK * rt_ref)


def test_differentiable_inverse_is_refused(pkg):
    net = pkg.SplineFlow((2, ), '2d', NS(layers=1)).to(DEV)
    with torch.no_grad():
        net(torch.randn(64, 2, device=DEV))
    with pkg.differentiable_inverse():
        with pytest.raises(NotImplementedError, match='RQSplineCoupling'):
            net.backward(torch.randn(8, 2, device=DEV))


@pytest.fixture
def det_mode(pkg):
    """the ordered mode for the EXISTING kernels of the step (the spline kernels need none), as in tests/test_gpu_trainer_loop.py"""
    N = pkg._native
    N.load()
    was = N.deterministic()
    N.deterministic(True)
    yield N
    N.deterministic(was)


def test_trainer_with_device_sampler_captures_and_replays(pkg):
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    nfdata = importlib.import_module(pkg.__name__ + '.data')
    torch.manual_seed(0)
    net = pkg.SplineFlow((2, ), '2d', NS(layers=2, bins=4)).to(DEV)
    tr = nftrain.FlowTrainer(net, graph=True, warmup=2, sampler=nfdata.DeviceSampler('moons', 512, (2, ), device=DEV))
    losses = [float(tr.train_on_batch()[1]) for _ in range(8)]
    torch.cuda.synchronize()
    assert tr._g_fb is not None and all(np.isfinite(losses)) and len(set(losses)) == len(losses)      # a fresh batch every replay


def test_trainer_captures_and_learns(pkg, det_mode):
    """FlowTrainer(graph=True) on moons: the step is captured and replayed, the loss falls over 40 steps (five batches, cycled, so the
    first and the last five steps see the same data), and two trainers from one seed fed the same batches end on the same bits"""
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    nfdata = importlib.import_module(pkg.__name__ + '.data')
    B = 256
    ys = [nfdata.sample('moons', B, 100 + i).to(DEV) for i in range(5)]
    ends = []
    for _ in range(2):
        torch.manual_seed(0)
        np.random.seed(0)
        net = pkg.SplineFlow((2, ), '2d', NS(layers=4)).to(DEV)
        tr = nftrain.FlowTrainer(net, lr=1e-3, graph=True, warmup=2)
        losses = []
        for step in range(40):
            z, loss = tr.train_on_batch(ys[step % 5])
            losses.append(float(loss))
        torch.cuda.synchronize()
        assert tr._g_fb is not None
        assert all(np.isfinite(losses)), losses
        print('loss: first five %.4f, last five %.4f' % (np.mean(losses[:5]), np.mean(losses[-5:])))
        assert np.mean(losses[-5:]) < np.mean(losses[:5])
        ends.append(tr.bucket.flat_params.detach().clone())
    assert torch.equal(ends[0], ends[1])
    assert det_mode.deterministic_timeouts() == 0 and det_mode.persistent_timeouts() == 0
