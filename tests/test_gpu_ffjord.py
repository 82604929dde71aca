"""
FFJORD on the MI355X (csrc/cnf.hip): goldens of the reference through the engine, a single CNF layer in float64 against the float64
restatement (tests/_ffjord.py) on the CPU over solvers x trace modes x D x B, the softplus threshold, bit-reproducible gradients, the three
noise sources, the inverse direction and its gradients, and two steps of the reference's training loop.

Measured maxima of the float64 comparisons are printed (run with -s) and recorded in profiles/r08_ffjord.txt.
"""
from types import SimpleNamespace as NS

import pytest
import torch

from tests import _ffjord as FJ
from tests._golden import group

pytestmark = pytest.mark.gpu
DEV = 'cuda'
L = 2
SOLVERS = ('midpoint', 'rk4', 'bosha3', 'dopri5')
TIMES = torch.linspace(0.0, 1.0, 11, dtype=torch.float32).double()
MODES = {'train': ('hutchinson', 1, True), 'exact': ('exact', 1, False), 'hutch4': ('hutchinson', 4, False)}


def cfg_of(solver, trace='hutchinson', **kw):
    return NS(layers=L, stepsize=0.1, t0=0.0, t1=1.0, solver=solver, trace=trace, backprop='adjoint', **kw)


def _err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    return err, max(1.0, float(b.abs().max()) if b.numel() else 1.0)


def _close(a, b, tol, what):
    err, ref = _err(a, b)
    print('%s: max abs err %.3e (scale %.3e)' % (what, err, ref))
    assert err <= tol * ref, '%s: max abs err %.3e > %.1e * %.3e' % (what, err, tol, ref)
    return err / ref


class _Feed:
    """noise_source of an ODENet: hands out the given (E, B, S, D) tensors pass by pass"""

    def __init__(self, *tensors):
        self.q = list(tensors)

    def __call__(self, E, B, S, D):
        t = self.q.pop(0)
        assert tuple(t.shape) == (E, B, S, D), (tuple(t.shape), (E, B, S, D))
        return t


def _cnfs(net):
    return [m for m in net.net.layers if hasattr(m, 'func')]


def _field(D, seed, scale=(1.0, 1.0, 1.0)):
    """six float64 field parameters, reference-style init (nn.Linear), layer j times ``scale[j]``"""
    g = torch.Generator().manual_seed(seed)
    scale = (scale, ) * 3 if isinstance(scale, float) else scale
    shapes = [(32, D + 1), (32, ), (32, 33), (32, ), (D, 33), (D, )]
    return [((torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1) * scale[i // 2] / (s[-1] ** 0.5 if len(s) == 2 else 6.0))
            for i, s in enumerate(shapes)]


def _layer(pkg, D, solver, trace, training, params):
    m = pkg.CNF((D, ), TIMES, solver, trace_estimator=trace)
    with torch.no_grad():
        for p, q in zip(m.func.field_params(), params):
            p.copy_(q)
    m.train(training)
    return m.to(DEV)


def _single_layer_case(pkg, D, B, solver, mode, flipped=True, scale=(1.0, 1.0, 1.0), seed=5):
    """one CNF direction in float64 in and out, engine against restatement: returns {name: relative error}"""
    trace, S, training = MODES[mode]
    g = torch.Generator().manual_seed(seed + 17 * D + B)
    params = _field(D, seed, scale)
    z = torch.randn(B, D, generator=g, dtype=torch.float64) * 0.8
    ld = torch.randn(B, generator=g, dtype=torch.float64) * 0.1
    gz = torch.randn(B, D, generator=g, dtype=torch.float64)
    gl = torch.randn(B, generator=g, dtype=torch.float64)
    E = FJ.STAGES[solver] * 10
    nf = torch.randn(E, B, S, D, generator=g)
    nb = torch.randn(E, B, S, D, generator=g)
    # the restatement, float64 on the CPU
    pr = [p.clone().requires_grad_(True) for p in params]
    zr, lr = z.clone().requires_grad_(True), ld.clone().requires_grad_(True)
    z1, l1 = FJ.cnf(pr, zr, lr, TIMES, solver, trace, list(nf), list(nb), flipped)
    torch.autograd.backward([z1, l1], [gz, gl])
    # the engine
    m = _layer(pkg, D, solver, trace, training, params)
    ze, le = z.to(DEV).requires_grad_(True), ld.to(DEV).requires_grad_(True)
    run = m.forward if flipped else m.backward
    z2, l2 = run(ze, le, noise=nf.to(DEV), noise_bwd=nb.to(DEV))
    assert z2.dtype == torch.float64 and l2.dtype == torch.float64
    torch.autograd.backward([z2, l2], [gz.to(DEV), gl.to(DEV)])
    out = {}
    for name, a, b in [('z', z2, z1), ('ld', l2, l1), ('g_z', ze.grad, zr.grad), ('g_ld', le.grad, lr.grad)] + \
            [('g_p%d' % i, p.grad, q.grad) for i, (p, q) in enumerate(zip(m.func.field_params(), pr))]:
        err, ref = _err(a, b)
        assert err <= 1e-9 * ref, '%s D=%d B=%d %s %s: max abs err %.3e (scale %.3e)' % (name, D, B, solver, mode, err, ref)
        out[name] = err / ref
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# goldens through the engine with the recorded noise
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [2, 3])
@pytest.mark.parametrize('solver', SOLVERS)
def test_training_goldens_with_recorded_noise(pkg, D, solver):
    """outputs are float32: 1e-6 max(1, |ref|) (the planar GPU bar); parameter gradients through the whole model: the project's 1e-5 (they
    inherit the float32 rounding of the ActNorm layers between the CNFs)"""
    g = group('model_ffjord', 'd%d/' % D)
    nz = group('model_ffjord_noise_d%d' % D, solver + '/')
    net = pkg.Ffjord((D, ), '2d', cfg_of(solver))
    net.load_state_dict({k[len('sd0/'):]: v for k, v in g.items() if k.startswith('sd0/')})
    net = net.to(DEV)
    for i, m in enumerate(_cnfs(net)):
        m.func.noise_source = _Feed(nz['fwd'][i], nz['bwd'][i])
    z, ld = net(g['y'].to(DEV))
    assert z.dtype == torch.float32 and ld.dtype == torch.float32
    loss = FJ.nll(z, ld)
    loss.backward()
    p = solver + '/'
    _close(z, g[p + 'z'], 1e-6, 'z')
    _close(ld, g[p + 'ld'], 1e-6, 'ld')
    _close(loss, g[p + 'loss'], 1e-6, 'loss')
    for k, q in net.named_parameters():
        _close(q.grad, g[p + 'grad/' + k], 1e-5, 'grad ' + k)
        assert q.grad.dtype == q.dtype
    for k, v in g.items():
        if k.startswith(p + 'an/'):
            _close(net.state_dict()[k[len(p + 'an/'):]], v, 1e-6, 'actnorm init ' + k)


@pytest.mark.parametrize('D', [2, 3])
@pytest.mark.parametrize('trace', ['exact', 'hutchinson'])
def test_evaluation_goldens(pkg, D, trace):
    from tests.test_ffjord_host import regenerated_noise
    g = group('model_ffjord', 'd%d/eval/' % D)
    net = pkg.Ffjord((D, ), '2d', cfg_of('dopri5', trace))
    net.load_state_dict({k[len('sd/'):]: v for k, v in g.items() if k.startswith('sd/')})
    for m in net.net.layers:
        m.initialized = True
    net = net.to(DEV).eval()
    E = 70
    for direction in ('fwd', 'inv'):
        c = {k[len(trace + '/' + direction + '/'):]: v for k, v in g.items() if k.startswith(trace + '/' + direction + '/')}
        if trace == 'hutchinson':
            draws = regenerated_noise(c, E, (64, 4, D))
            parts = [torch.stack(draws[i * E:(i + 1) * E]) for i in range(L)]
            for i, m in enumerate(_cnfs(net)):
                m.func.noise_source = _Feed(parts[i] if direction == 'fwd' else parts[L - 1 - i])
        with torch.no_grad():
            if direction == 'fwd':
                a, b = net(group('model_ffjord', 'd%d/' % D)['y'].to(DEV))
                _close(a, c['z'], 1e-6, 'z')
            else:
                a, b = net.backward(c['u'].to(DEV))
                _close(a, c['x'], 1e-6, 'x')
            _close(b, c['ld'], 1e-6, 'ld')


# ---------------------------------------------------------------------------------------------------------------------------------------
# a single CNF layer, float64 in and out, against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('solver', SOLVERS)
def test_single_layer_float64_sweep(pkg, solver, mode):
    """bar 1e-9 max(1, max|ref|): fp64 unit roundoff 1.1e-16, at most ~6e5 terms in any sum (4 097 rows x 70 evaluations x 2 pairs), an
    order of magnitude for growth along the ODE.  Anything above 1e-10 wants an explanation (profiles/r08_ffjord.txt holds the maxima)."""
    worst = {}
    for D in (1, 2, 3, 8):
        for B in (1, 63, 64, 4097):
            for k, v in _single_layer_case(pkg, D, B, solver, mode).items():
                k = k if k in ('z', 'ld', 'g_z', 'g_ld') else 'g_theta'
                worst[k] = max(worst.get(k, 0.0), v)
    print('float64 sweep %s %s: ' % (solver, mode) + ' '.join('%s %.2e' % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1e-9


def test_softplus_threshold(pkg):
    """weights scaled so that the pre-activations span +-40: value, trace and gradients still meet the 1e-9 bar, on both branches"""
    D, B, scale = 3, 257, (30.0, 2.0, 0.05)
    pre = []
    params = _field(D, 5, scale)
    g = torch.Generator().manual_seed(5 + 17 * D + B)
    z = torch.randn(B, D, generator=g, dtype=torch.float64) * 0.8
    FJ.field(params, TIMES[3], z, None, 'exact', pre=pre)
    for h in pre:
        print('pre-activations: min %.1f max %.1f, %d above 20' % (float(h.min()), float(h.max()), int((h > 20).sum())))
        assert float(h.max()) > 20.0 and float(h.min()) < 20.0 and int((h > 20).sum()) > 10 and int((h < -20).sum()) > 10
    for mode in MODES:
        errs = _single_layer_case(pkg, D, B, 'rk4', mode, scale=scale)
        print('threshold %s: ' % mode + ' '.join('%s %.2e' % kv for kv in sorted(errs.items())))


def test_gradients_are_bit_reproducible(pkg):
    D, B = 2, 4097
    m = _layer(pkg, D, 'dopri5', 'hutchinson', True, _field(D, 9))
    g = torch.Generator().manual_seed(1)
    z, ld = torch.randn(B, D, generator=g).to(DEV), torch.zeros(B, device=DEV)
    nf, nb = torch.randn(70, B, 1, D, generator=g).to(DEV), torch.randn(70, B, 1, D, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        zz = z.clone().requires_grad_(True)
        for p in m.parameters():
            p.grad = None
        a, b = m(zz, ld.clone(), noise=nf, noise_bwd=nb)
        (a.sum() + (b * b).sum()).backward()
        runs.append([zz.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][3].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------------------------------------------------
def _main_steps(pkg, net, g, steps=2):
    optim = torch.optim.Adam(net.parameters(), lr=1.0e-4, betas=(0.9, 0.999), weight_decay=0.0)       # main.py:56-71
    sched = torch.optim.lr_scheduler.StepLR(optim, step_size=10000, gamma=0.5)
    losses = []
    for s in range(steps):
        y = g['step%d/y' % s].to(DEV)
        z, ld = net(y.contiguous())
        loss = FJ.nll(z.view(y.shape[0], -1), ld)
        optim.zero_grad()
        loss.backward()
        optim.step()
        sched.step()
        _close(z, g['step%d/z' % s], 1e-5, 'step %d z' % s)
        _close(loss, g['step%d/loss' % s], 1e-5, 'step %d loss' % s)
        losses.append(float(loss.detach()))
    return losses


def test_training_steps_with_cpu_noise_match_goldens(pkg):
    """noise_on_cpu=True reproduces the reference's draw order, the backward pass's draws included: two steps of main.py's loop (Adam) on
    the engine's Ffjord match the goldens with nothing injected, after torch.manual_seed"""
    g = group('model_ffjord', 'main/')
    net = pkg.Ffjord((2, ), '2d', cfg_of('dopri5', noise_on_cpu=True))
    net.load_state_dict({k[len('sd0/'):]: v for k, v in g.items() if k.startswith('sd0/')})
    net = net.to(DEV)
    assert all(m.noise_on_cpu for m in _cnfs(net))
    torch.manual_seed(int(g['noise_seed']))
    _main_steps(pkg, net, g)
    sd = net.state_dict()
    for k, v in g.items():
        if k.startswith('sdN/'):
            _close(sd[k[len('sdN/'):]], v, 1e-5, 'state after 2 steps ' + k)
            assert sd[k[len('sdN/'):]].dtype == v.dtype


def test_in_kernel_noise_is_standard_normal_and_is_what_the_kernels_use(pkg):
    NF = pkg.functional
    E, B, S, D = 70, 4096, 1, 4
    seed = torch.tensor([1234, 7], dtype=torch.int64, device=DEV)
    w = NF.cnf_noise(seed, E, B, S, D)
    assert w.dtype == torch.float32 and w.numel() >= 10 ** 6
    n = w.numel()
    x = w.double()
    mean, var = float(x.mean()), float(x.var())
    print('in-kernel noise: n %d mean %.3e var %.6f' % (n, mean, var))
    assert abs(mean) <= 5.0 / n ** 0.5                                       # standard error of the mean of N(0, 1)
    assert abs(var - 1.0) <= 5.0 * (2.0 / n) ** 0.5                          # ... and of its variance
    assert not torch.equal(w[0], w[1]) and not torch.equal(w[:, 0], w[:, 1]) and float((w[0] - w[1]).abs().max()) > 1.0
    seed2 = torch.tensor([1234, 8], dtype=torch.int64, device=DEV)
    assert not torch.equal(w, NF.cnf_noise(seed2, E, B, S, D))               # another pass, another stream
    # the integration with in-kernel noise equals the integration fed that noise explicitly
    params = [p.to(DEV) for p in _field(D, 3)]
    sched, steps = NF.cnf_pack_schedule(TIMES, 'dopri5', DEV)
    z = torch.randn(B, D, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(DEV)
    ld = torch.zeros(B, dtype=torch.float64, device=DEV)
    a = NF.cnf_integrate(z, ld, params, sched, steps, 'dopri5', 'hutchinson', S, None, seed)
    b = NF.cnf_integrate(z, ld, params, sched, steps, 'dopri5', 'hutchinson', S, w, None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a layer left to itself draws in the kernel, freshly per pass
    m = _layer(pkg, D, 'rk4', 'hutchinson', True, _field(D, 3))
    with torch.no_grad():
        l1 = m(z, ld)[1]
        l2 = m(z, ld)[1]
    assert not torch.equal(l1, l2)


def test_hutchinson_average_approaches_the_exact_trace(pkg):
    """the mean of the estimate over 256 seeds lies within 5 standard errors (of its own sample spread) of the exact trace, per row"""
    NF = pkg.functional
    D, B, R = 3, 64, 256
    params = [p.to(DEV) for p in _field(D, 21, 3.0)]
    sched, steps = NF.cnf_pack_schedule(TIMES, 'rk4', DEV)
    z = torch.randn(B, D, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(DEV)
    ld = torch.zeros(B, dtype=torch.float64, device=DEV)
    exact = NF.cnf_integrate(z, ld, params, sched, steps, 'rk4', 'exact')[1]
    runs = torch.stack([NF.cnf_integrate(z, ld, params, sched, steps, 'rk4', 'hutchinson', 1, None,
                                         torch.tensor([1000 + r, 0], dtype=torch.int64, device=DEV))[1] for r in range(R)])
    mean, se = runs.mean(0), runs.std(0) / R ** 0.5
    dev = ((mean - exact).abs() / se).max()
    print('hutchinson vs exact: worst row %.2f standard errors, |exact| max %.3e, spread %.3e' % (float(dev), float(exact.abs().max()),
                                                                                                  float(runs.std(0).max())))
    assert float(se.min()) > 0.0 and float(dev) <= 5.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inverse direction
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_exact_trace_round_trip(pkg):
    """backward(forward(y)) of a CNF returns y and the log-dets cancel, as far as the float64 restatement's own round trip does on the
    same case (times 2): the solver's truncation error is the reference's too.  float64 in and out, so that nothing but the integration
    is in the comparison."""
    D, B = 2, 64
    g = group('model_ffjord', 'd%d/eval/' % D)
    params = [g['sd/net.layers.1.func.layers.%d.linear.%s' % (j, n)] for j in range(3) for n in ('weight', 'bias')]
    y = group('model_ffjord', 'd%d/' % D)['y'].double()
    zero = torch.zeros(B, dtype=torch.float64)
    with torch.no_grad():
        z, ld = FJ.cnf(params, y, zero, TIMES, 'dopri5', 'exact', None, None, True)
        x, ldi = FJ.cnf(params, z, zero, TIMES, 'dopri5', 'exact', None, None, False)
    bar_x, bar_ld = 2.0 * float((x - y).abs().max()), 2.0 * float((ld + ldi).abs().max())
    m = _layer(pkg, D, 'dopri5', 'exact', False, params)
    with torch.no_grad():
        z2, ld2 = m(y.to(DEV), zero.to(DEV))
        x2, ldi2 = m.backward(z2, zero.to(DEV))
    ex, el = float((x2.cpu() - y).abs().max()), float((ld2 + ldi2).abs().max())
    print('round trip: x %.3e (bar %.3e), ld %.3e (bar %.3e)' % (ex, bar_x, el, bar_ld))
    assert bar_x > 0.0 and ex <= bar_x and el <= bar_ld


def test_gradients_through_the_inverse(pkg):
    D, B = 2, 64
    g = group('model_ffjord', 'd%d/eval/' % D)
    sd = {k[len('sd/'):]: v for k, v in g.items() if k.startswith('sd/')}
    u = g['exact/inv/u']
    gen = torch.Generator().manual_seed(8)
    nf = [torch.randn(70, B, 1, D, generator=gen) for _ in range(L)]
    nb = [torch.randn(70, B, 1, D, generator=gen) for _ in range(L)]
    layers = FJ.model_params(sd, L, requires_grad=True)
    ur = u.clone().requires_grad_(True)
    x, ld = FJ.model_inverse(layers, ur, TIMES, 'dopri5', 'hutchinson', [list(t) for t in nf], [list(t) for t in nb])
    (FJ.nll(x, ld) + x.sum()).backward()
    net = pkg.Ffjord((D, ), '2d', cfg_of('dopri5'))
    net.load_state_dict(sd)
    for m in net.net.layers:
        m.initialized = True
    net = net.to(DEV)                                                       # training mode: one sample, as the restatement above
    for i, m in enumerate(_cnfs(net)):
        m.func.noise_source = _Feed(nf[i], nb[i])
    ue = u.to(DEV).requires_grad_(True)
    x2, ld2 = net.backward(ue)
    (FJ.nll(x2, ld2) + x2.sum()).backward()
    _close(x2, x, 1e-6, 'x')
    _close(ld2, ld, 1e-6, 'ld')
    _close(ue.grad, ur.grad, 1e-5, 'grad u')
    flat = [t for ls, b, prm in layers for t in [ls, b] + prm]
    for (k, q), t in zip(net.named_parameters(), flat):
        _close(q.grad, t.grad, 1e-5, 'grad ' + k)
    # parameters alone: the differentiable_inverse() context
    for i, m in enumerate(_cnfs(net)):
        m.func.noise_source = _Feed(nf[i], nb[i])
    for q in net.parameters():
        q.grad = None
    with pkg.differentiable_inverse():
        x3, ld3 = net.backward(u.to(DEV))
    (FJ.nll(x3, ld3) + x3.sum()).backward()
    for (k, q), t in zip(net.named_parameters(), flat):
        _close(q.grad, t.grad, 1e-5, 'grad (context) ' + k)


def test_normal_backprop_raises_when_run(pkg):
    m = pkg.CNF((2, ), TIMES, 'rk4', backprop='normal').to(DEV)
    with pytest.raises(NotImplementedError):
        m(torch.randn(4, 2, device=DEV), torch.zeros(4, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_adam_steps_with_in_kernel_noise_train(pkg):
    """the default configuration (noise drawn in the kernel): the reference's loop runs, gradients reach every parameter in its own dtype,
    the loss stays finite; the first step's z equals the golden's (z does not depend on the noise realisation)"""
    g = group('model_ffjord', 'main/')
    torch.manual_seed(3)
    net = pkg.Ffjord((2, ), '2d', cfg_of('dopri5'))
    net.load_state_dict({k[len('sd0/'):]: v for k, v in g.items() if k.startswith('sd0/')})
    net = net.to(DEV)
    optim = torch.optim.Adam(net.parameters(), lr=1.0e-4)
    for s in range(2):
        z, ld = net(g['step%d/y' % s].to(DEV))
        loss = FJ.nll(z, ld)
        optim.zero_grad()
        loss.backward()
        optim.step()
        assert all(q.grad is not None and q.grad.dtype == q.dtype and bool(torch.isfinite(q.grad).all()) for q in net.parameters())
        assert bool(torch.isfinite(loss))
        if s == 0:
            _close(z, g['step0/z'], 1e-5, 'step 0 z (z does not depend on the noise)')
