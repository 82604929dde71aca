"""
The planar flow on the MI355X (csrc/planar.hip): goldens of the reference, shapes against the float64 restatement (tests/_planar.py) in
both forms of the inverse, the batch-global exit rule through the kernels' iteration counts, reproducible gradients, the trainer's
captured step, gradients through the inverse, and the input-shape check.
"""
from types import SimpleNamespace as NS

import pytest
import torch

from tests import _planar as P
from tests._golden import group

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def NF(pkg):
    pkg.build()
    torch.cuda.set_device(0)
    pkg._native.load()
    yield pkg.functional
    pkg.functional.planar_config(False)


@pytest.fixture(params=['wg', 'grid'])
def form(request, NF):
    NF.planar_config(request.param == 'grid')
    yield request.param
    NF.planar_config(False)


def _bar(a, ref64, ref32, K):
    """1e-5 at K <= 4; the full-depth bar 1e-5 * scale + 4 |cpu32 - cpu64| at larger K"""
    scale = max(1.0, float(ref64.abs().max()) if ref64.numel() else 1.0)
    if K <= 4:
        return 1e-5 * scale
    return 1e-5 * scale + 4.0 * float((ref32.double() - ref64).abs().max())


def _check(got, ref64, ref32, K, what, extra=None):
    got = got.detach().double().cpu()
    err = float((got - ref64).abs().max()) if got.numel() else 0.0
    bar = extra if extra is not None else _bar(got, ref64, ref32, K)
    assert err <= bar, '%s: max abs err %.3e > %.3e' % (what, err, bar)


def _engine(pkg, sd, K, D):
    net = pkg.PlanarFlow((D, ), '2d', NS(layers=K))
    net.load_state_dict(sd)
    return net.to(DEV)


def _sd(g, prefix):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


@pytest.mark.parametrize('D', [2, 3])
def test_goldens(pkg, NF, form, D):
    g = group('model_planar', 'd%d/' % D)
    net = _engine(pkg, _sd(g, 'sd0/'), 4, D).train()
    z, ld = net(g['y'].to(DEV))
    loss = NF.nll_loss(z, ld)
    loss.backward()
    tol = 1e-5
    assert torch.allclose(z.detach().cpu(), g['z'], atol=tol, rtol=tol)
    assert torch.allclose(ld.detach().cpu(), g['ld'], atol=tol, rtol=tol)
    assert abs(float(loss.detach()) - float(g['loss'])) < tol * max(1.0, abs(float(g['loss'])))
    for k, p in net.named_parameters():
        ref = g['grad/' + k]
        assert torch.allclose(p.grad.cpu(), ref, atol=tol * max(1.0, float(ref.abs().max())), rtol=tol), k
    with torch.no_grad():
        x, ldi = net.backward(g['z'].to(DEV))
    assert torch.allclose(x.cpu(), g['x_inv'], atol=tol, rtol=tol)
    assert torch.allclose(ldi.cpu(), g['ld_inv'], atol=tol, rtol=tol)


def test_golden_projection(pkg, NF):
    g = group('model_planar', 'proj/')
    net = _engine(pkg, _sd(g, 'sd0/'), 4, 2)
    for mode in ('train', 'eval'):
        net.load_state_dict(_sd(g, 'sd0/'))
        getattr(net, mode)()
        with torch.no_grad() if mode == 'eval' else torch.enable_grad():
            z, ld = net(g['y'].to(DEV))
        assert torch.allclose(z.detach().cpu(), g['z'], atol=1e-5, rtol=1e-5), mode
        assert torch.allclose(ld.detach().cpu(), g['ld'], atol=1e-5, rtol=1e-5), mode
        for k, v in _sd(g, 'sd1/').items():
            assert torch.allclose(net.state_dict()[k].cpu(), v, atol=1e-6, rtol=1e-6), (mode, k)


def test_golden_mainloop(pkg, NF):
    """main.py's train_on_batch with torch.optim.Adam + StepLR for three steps"""
    g = group('model_planar', 'main/')
    net = _engine(pkg, _sd(g, 'sd0/'), 4, 2).train()
    optim = torch.optim.Adam(net.parameters(), lr=1.0e-4, betas=(0.9, 0.999), weight_decay=0.0)
    sched = torch.optim.lr_scheduler.StepLR(optim, step_size=10000, gamma=0.5)
    for s in range(3):
        y = g['step%d/y' % s].to(DEV)
        z, ld = net(y)
        loss = NF.nll_loss(z, ld)
        optim.zero_grad()
        loss.backward()
        optim.step()
        sched.step()
        assert torch.allclose(z.detach().cpu(), g['step%d/z' % s], atol=1e-5, rtol=1e-5), s
        assert abs(float(loss) - float(g['step%d/loss' % s])) < 1e-5 * max(1.0, abs(float(g['step%d/loss' % s]))), s
    for k, v in _sd(g, 'sdN/').items():
        assert torch.allclose(net.state_dict()[k].cpu(), v, atol=1e-5, rtol=1e-5), k


# (K, D, B); D = 3072 at K = 4 only (the float64 restatement at K = 32 is minutes of CPU time there)
SHAPES = [(K, D, B) for K in (4, 32) for D in (1, 2, 3, 5, 8) for B in (1, 255, 1024, 65536)] + \
         [(K, D, B) for K in (4, 32) for D in (9, 64) for B in (1, 255, 1024, 20000)] + [(4, 3072, 1), (4, 3072, 255)]


def _random_flow(pkg, K, D, seed):
    torch.manual_seed(seed)
    net = pkg.PlanarFlow((D, ), '2d', NS(layers=K))
    with torch.no_grad():
        for m in net.net.layers:
            m.u.copy_(torch.randn(1, D) * (0.6 / D**0.5))
            m.w.copy_(torch.randn(1, D) * (1.2 / D**0.5))
            m.b.copy_(torch.randn(1) * 0.2)
    return net


@pytest.mark.parametrize('K,D,B', SHAPES)
def test_shapes_against_float64(pkg, NF, form, K, D, B):
    net = _random_flow(pkg, K, D, 1000 + D + B)
    with torch.no_grad():                                           # the reference's construction-time projection has run; the forward's
        for m in net.net.layers:                                    # own projection is a no-op unless w.u < -1: project on the CPU first
            m.u.copy_(P.project(m.u.double(), m.w.double()).float())
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    y = torch.randn(B, D, generator=torch.Generator().manual_seed(B + D)) * 0.7
    p64 = P.params_of(sd, K, torch.float64, requires_grad=True)
    p32 = P.params_of(sd, K, torch.float32, requires_grad=True)
    z64, ld64, _ = P.forward(y.double(), torch.zeros(B, dtype=torch.float64), p64)
    z32, ld32, _ = P.forward(y, torch.zeros(B), p32)
    want_grads = B <= 1024 and D <= 64
    if want_grads:
        P.nll(z64, ld64).backward()
        P.nll(z32, ld32).backward()
    net = net.to(DEV).train()
    z, ld = net(y.to(DEV))
    _check(z, z64.detach(), z32.detach(), K, 'z')
    _check(ld, ld64.detach(), ld32.detach(), K, 'ld')
    if want_grads:
        NF.nll_loss(z, ld).backward()
        for i, m in enumerate(net.net.layers):
            for n, a64, a32 in zip('uwb', p64[i], p32[i]):
                g = getattr(m, n).grad
                _check(g, a64.grad, a32.grad, K, 'grad %d.%s' % (i, n), extra=_bar(g, a64.grad, a32.grad, 32))
    # inverse of a latent batch
    zin = torch.randn(B, D, generator=torch.Generator().manual_seed(7 + B)) * 0.8
    with torch.no_grad():
        x64, li64, _ = P.inverse(zin.double(), torch.zeros(B, dtype=torch.float64), P.params_of(sd, K, torch.float64))
        x32, li32, _ = P.inverse(zin, torch.zeros(B), P.params_of(sd, K, torch.float32))
        x, li = net.backward(zin.to(DEV))
    _check(x, x64, x32, K, 'x_inv', extra=_bar(x, x64, x32, 32))
    _check(li, li64, li32, K, 'ld_inv', extra=_bar(li, li64, li32, 32))


def _exit_layer(pkg):
    m = pkg.PlanarTransform(2)
    with torch.no_grad():
        m.u.copy_(torch.tensor([[0.0, 0.5]]))
        m.w.copy_(torch.tensor([[1.0, 0.0]]))
        m.b.zero_()
    return m.to(DEV)


@pytest.mark.parametrize('B', [64, 1024, 20000])
def test_exit_rule(pkg, NF, form, B):
    """w.u = 0 makes val = mid exactly: the counts do not depend on tanh's rounding.  28 iterations; one row whose target is the first
    midpoint (0.0) sticks the whole batch at 100; so does one rounding-limited root (300.3)"""
    m = _exit_layer(pkg)
    base = torch.stack([torch.full((B, ), 0.5), torch.randn(B)], 1)
    for extra, want in ((None, 28), ([0.0, 0.3], 100), ([300.3, -0.2], 100)):
        z = base if extra is None else torch.cat([base, torch.tensor([extra])])
        ref_n = P.inverse(z, torch.zeros(z.shape[0]), [(m.u.cpu(), m.w.cpu(), m.b.cpu())])[2]
        assert ref_n == [want]
        x, ld, iters = NF.planar_inverse(z.to(DEV), torch.zeros(z.shape[0], device=DEV), [m])
        assert iters.cpu().tolist() == [want], (form, B, extra, iters)
        x32, ld32, _ = P.inverse(z, torch.zeros(z.shape[0]), [(m.u.cpu(), m.w.cpu(), m.b.cpu())])
        assert torch.allclose(x.cpu(), x32, atol=1e-5, rtol=1e-5)
        assert torch.allclose(ld.cpu(), ld32, atol=1e-5)


def test_iteration_counts_per_layer_agree_between_forms(pkg, NF):
    net = _random_flow(pkg, 8, 2, 5).to(DEV)
    z = torch.randn(3000, 2, device=DEV)
    layers = list(net.net.layers)
    NF.planar_config(False)
    a = NF.planar_inverse(z, torch.zeros(3000, device=DEV), layers, mids=True)
    NF.planar_config(True)
    b = NF.planar_inverse(z, torch.zeros(3000, device=DEV), layers, mids=True)
    NF.planar_config(False)
    assert torch.equal(a[2], b[2])
    assert torch.equal(a[3], b[3]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(28 <= n <= 100 for n in a[2].cpu().tolist())


def test_backward_bit_reproducible(pkg, NF):
    assert not pkg._native.deterministic()                          # NF_DETERMINISTIC=0: no float atomics on this path anyway
    net = _random_flow(pkg, 32, 2, 11).to(DEV).train()
    y = torch.randn(65536, 2, device=DEV)
    grads = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        yy = y.clone().requires_grad_(True)
        z, ld = net(yy)
        NF.nll_loss(z, ld).backward()
        grads.append([p.grad.clone() for p in net.parameters()] + [yy.grad.clone()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_flow_trainer_graph_matches_eager(pkg, NF):
    from importlib import import_module
    train = import_module(pkg.__name__ + '.train')
    nets = [_random_flow(pkg, 8, 2, 21).to(DEV) for _ in range(2)]
    eager = train.FlowTrainer(nets[0], lr=1e-3, graph=False)
    graph = train.FlowTrainer(nets[1], lr=1e-3, graph=True, warmup=2)
    gen = torch.Generator(device=DEV).manual_seed(3)
    for s in range(6):
        y = torch.randn(1024, 2, device=DEV, generator=gen)
        if s == 2:                                                  # the capturing call takes one extra eager step on its batch first
            eager.train_on_batch(y)
        za, la = eager.train_on_batch(y)
        zb, lb = graph.train_on_batch(y)
        assert torch.allclose(za, zb, atol=1e-6, rtol=1e-6), s
        assert abs(float(la) - float(lb)) <= 1e-6 * max(1.0, abs(float(la))), s
    assert graph._g_fb is not None, 'the planar step was not captured'
    for (k, a), b in zip(nets[0].named_parameters(), nets[1].parameters()):
        assert torch.allclose(a, b, atol=1e-6, rtol=1e-6), k
    y, p = graph.sample_y(512, (2, ))
    assert y.shape == (512, 2) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(p).all())


def test_graph_step_projects_flat_bucket(pkg, NF):
    """a u that the first captured forward must project: the replayed graph writes it through the bucket's storage"""
    from importlib import import_module
    train = import_module(pkg.__name__ + '.train')
    net = _random_flow(pkg, 4, 2, 31)
    tr = train.FlowTrainer(net.to(DEV), lr=1e-4, graph=True, warmup=1)
    y = torch.randn(256, 2, device=DEV)
    tr.train_on_batch(y)
    tr.train_on_batch(y)                                            # captured
    m = net.net.layers[2]
    with torch.no_grad():
        m.w.copy_(torch.tensor([[0.8, -0.6]], device=DEV))
        m.u.copy_(torch.tensor([[-1.5, 0.7]], device=DEV))
    expect = P.project(m.u.detach().cpu(), m.w.detach().cpu())
    tr.train_on_batch(y)
    torch.cuda.synchronize()
    wu = float((m.u.detach() * m.w.detach()).sum())
    assert wu > -1.0 - 1e-3, wu                                     # projected (then one Adam step of lr 1e-4)
    assert torch.allclose(m.u.detach().cpu(), expect, atol=1e-3)


def test_differentiable_inverse_gradients(pkg, NF):
    net = _random_flow(pkg, 4, 2, 41)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.to(DEV)
    z = torch.randn(256, 2, generator=torch.Generator().manual_seed(5))
    with pkg.differentiable_inverse():
        x, ld = net.backward(z.to(DEV))
        loss = (x * x).sum() * 0.01 + ld.sum() * 0.01
        loss.backward()
    p64 = P.params_of(sd, 4, torch.float64, requires_grad=True)
    x64, ld64, _ = P.inverse(z.double(), torch.zeros(256, dtype=torch.float64), p64)
    ((x64 * x64).sum() * 0.01 + ld64.sum() * 0.01).backward()
    for i, m in enumerate(net.net.layers):
        for n, r in zip('uwb', p64[i]):
            g = getattr(m, n).grad
            assert g is not None, (i, n)
            err = float((g.double().cpu() - r.grad).abs().max())
            assert err <= 1e-4 * max(1.0, float(r.grad.abs().max())), (i, n, err)
    zg = z.to(DEV).requires_grad_(True)                             # an input that requires grad records the graph as well
    x2, _ = net.backward(zg)
    x2.sum().backward()
    assert zg.grad is not None and bool(torch.isfinite(zg.grad).all())


def test_four_d_input_raises_on_gpu(pkg, NF):
    net = pkg.PlanarFlow((3, 4, 4), 'image', NS(layers=2)).to(DEV)
    with pytest.raises(RuntimeError, match=r'\(2, 3, 4, 4\)'):
        net(torch.rand(2, 3, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match=r'\(2, 3, 4, 4\)'):
        net.backward(torch.rand(2, 3, 4, 4, device=DEV))
