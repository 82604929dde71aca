"""
The whole-stack Residual Flow kernels on the MI355X (csrc/resflow.hip) against the per-block path (NF_RESFLOW_STACK=0: one ActNorm launch and
the kernels of csrc/resmlp.hip per block), against nested autograd in float64 on the CPU, and on their own: launch counts that do not
depend on the depth, in-kernel draws, the one-workgroup inverse, the ActNorm initialisation hand-over, deterministic mode, the trainer's
captured step.
"""
import copy
import math
from importlib import import_module
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-5


@pytest.fixture(scope='module')
def NF(pkg):
    pkg.build()
    torch.cuda.set_device(0)
    pkg._native.load()
    old = pkg.functional.RESFLOW_STACK
    yield pkg.functional
    pkg.functional.RESFLOW_STACK = old


def _net(pkg, L, D, logdet='unbias', seed=0, init=True):
    """a ResFlow with non-trivial ActNorm parameters and LipSwish slopes, CPU noise (so that both paths see the same values)"""
    torch.manual_seed(seed)
    net = pkg.ResFlow((D, ), '2d', NS(layers=L, spnorm_coeff=0.9, logdet=logdet))
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, pkg.ActNorm) and init:
                m.log_scale.copy_(0.2 * torch.randn_like(m.log_scale))
                m.bias.copy_(0.3 * torch.randn_like(m.bias))
                m.initialized = True
            if isinstance(m, pkg.LipSwish):
                m.beta.fill_(0.8 + 0.3 * torch.rand(()).item())
            if isinstance(m, pkg.InvertibleResLinear):
                m.noise_on_cpu = True
    return net


def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)


def _close(got, want, tol, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max()) if got.numel() else 0.0
    bar = tol * max(1.0, float(want.abs().max()) if want.numel() else 1.0)
    assert err <= bar, '%s: max abs err %.3e > %.3e' % (what, err, bar)


def _uv(net):
    return {k: v.detach().clone() for k, v in net.named_buffers() if k.endswith('weight_u') or k.endswith('weight_v')}


def _train_pass(NF, net0, x, gz, gld, stack, seed=7):
    net = copy.deepcopy(net0).to(DEV).train()
    NF.RESFLOW_STACK = stack
    _seed(seed)
    xx = x.clone().to(DEV).requires_grad_(True)
    z, ld = net(xx)
    torch.autograd.backward([z, ld], [gz.to(DEV), gld.to(DEV)])
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    return z.detach(), ld.detach(), xx.grad.detach(), grads, _uv(net)


def _eval_pass(NF, net0, x, stack, seed=9):
    net = copy.deepcopy(net0).to(DEV).eval()
    NF.RESFLOW_STACK = stack
    _seed(seed)
    with torch.no_grad():
        z, ld = net(x.to(DEV))
    return z, ld, _uv(net)


def _compare_paths(pkg, NF, B, D, L):
    net0 = _net(pkg, L, D, seed=100 * L + 10 * D + 1)
    g = torch.Generator().manual_seed(B + D)
    x = 0.7 * torch.randn(B, D, generator=g)
    gz, gld = torch.randn(B, D, generator=g), torch.full((B, ), -1.0 / B) + 0.01 * torch.randn(B, generator=g)
    a = _train_pass(NF, net0, x, gz, gld, True)
    b = _train_pass(NF, net0, x, gz, gld, False)
    tag = 'B%d D%d L%d ' % (B, D, L)
    _close(a[0], b[0], TOL, tag + 'z')
    _close(a[1], b[1], TOL, tag + 'ld')
    _close(a[2], b[2], TOL, tag + 'd_x')
    assert set(a[3]) == set(b[3]) and len(a[3]) == 10 * L, (sorted(a[3]), sorted(b[3]))
    for k in b[3]:
        _close(a[3][k], b[3][k], TOL, tag + 'grad ' + k)
    for k in b[4]:
        assert float((a[4][k] - b[4][k]).abs().max()) <= 2e-6, tag + k
    for est in ('exact', 'fixed', 'unbias'):
        for m in net0.modules():
            if isinstance(m, pkg.InvertibleResLinear):
                m.estimator = est
        a, b = _eval_pass(NF, net0, x, True), _eval_pass(NF, net0, x, False)
        _close(a[0], b[0], TOL, tag + est + ' z')
        _close(a[1], b[1], TOL, tag + est + ' ld')
        for k in b[2]:
            assert float((a[2][k] - b[2][k]).abs().max()) <= 2e-6, tag + est + ' ' + k


@pytest.mark.parametrize('D', [1, 2, 3, 4])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257])
def test_stack_matches_per_block_with_host_draws(pkg, NF, B, D):
    """same seeds, NF_RESFLOW_STACK 1 vs 0: training forward + backward (z, ld, d_x, every parameter gradient, the ActNorms' included) and
    the three evaluation estimators within the project's TOL; the power-iteration buffers after the call to 2e-6"""
    for L in (1, 2, 5):
        _compare_paths(pkg, NF, B, D, L)


def test_stack_longer_than_the_per_launch_cap(pkg, NF):
    L = NF.RESFLOW_MAX_LAYERS + 1
    assert L == pkg._native.header_constant('NF_RESFLOW_MAX_LAYERS') + 1
    _compare_paths(pkg, NF, 8, 2, L)


@pytest.mark.parametrize('B,D', [(65, 2), (33, 3)])
def test_stack_matches_nested_autograd_in_float64(pkg, NF, B, D):
    """a 3-layer ResFlow through the whole-stack kernels against the formulation the reference uses: ActNorm in torch ops and every block
    differentiated by nested autograd sweeps, FLOAT64 on the CPU, identical lengths and noise.  Bar (test_iresblock_training_hip_matches_
    autograd's): 2e-5 max(1, max|cpu64|) + 4 |cpu32 - cpu64|."""
    L = 3
    net0 = _net(pkg, L, D, seed=5)
    g = torch.Generator().manual_seed(17)
    x = 0.7 * torch.randn(B, D, generator=g)
    gz, gld = torch.randn(B, D, generator=g), torch.full((B, ), -1.0 / B)

    def cpu(dt):
        net = copy.deepcopy(net0).to(dt).train()
        _seed(7)
        xx = x.clone().to(dt).requires_grad_(True)
        z, ld = xx, torch.zeros(B, dtype=dt)
        for m in net.net.layers:
            if isinstance(m, pkg.ActNorm):                               # modules.py:244-250
                z = (z - m.bias) / torch.exp(m.log_scale)
                ld = ld - m.log_scale.sum()
            else:
                m.hip_training = False
                if dt == torch.float64:                                  # the same float32 noise values in every run
                    m._randn_like = lambda t, shape=None: torch.randn(tuple(t.shape) if shape is None else shape).double()
                z, ld = m(z, ld)
        torch.autograd.backward([z, ld], [gz.to(dt), gld.to(dt)])
        grads = {k: p.grad.detach().double() for k, p in net.named_parameters() if p.grad is not None}
        return z.detach().double(), ld.detach().double(), xx.grad.detach().double(), grads
    ref, c32 = cpu(torch.float64), cpu(torch.float32)
    got = _train_pass(NF, net0, x, gz, gld, True)

    def check(what, a, want, fp32):
        a = a.detach().double().cpu()
        bar = 2e-5 * max(1.0, float(want.abs().max())) + 4.0 * float((fp32 - want).abs().max())
        err = float((a - want).abs().max())
        assert err <= bar, '%s: |gpu - cpu64| %.3e > %.3e (cpu32 itself %.3e)' % (what, err, bar, float((fp32 - want).abs().max()))
    check('z', got[0], ref[0], c32[0])
    check('ld', got[1], ref[1], c32[1])
    check('d_x', got[2], ref[2], c32[2])
    assert set(got[3]) == set(ref[3])
    for k in ref[3]:
        check('grad ' + k, got[3][k], ref[3][k], c32[3][k])


class _Calls:
    """counts the C-ABI calls that go through _native.call"""

    def __init__(self, pkg):
        self.N, self.names = pkg._native, []

    def __enter__(self):
        self.orig = self.N.call

        def call(name, *args):
            self.names.append(name)
            return self.orig(name, *args)
        self.N.call = call
        return self

    def __exit__(self, *exc):
        self.N.call = self.orig
        return False


def _counted(pkg, NF, L, stack=True):
    net = _net(pkg, L, 2, seed=3).to(DEV)
    x = torch.randn(64, 2, device=DEV)
    NF.RESFLOW_STACK = stack
    net.train()
    _seed(1)
    with _Calls(pkg) as train:
        z, ld = net(x.clone().requires_grad_(True))
        (z.sum() + ld.sum()).backward()
    net.eval()
    with _Calls(pkg) as ev, torch.no_grad():
        net(x)
    return train.names, ev.names


def test_launch_count_does_not_depend_on_depth(pkg, NF):
    t2, e2 = _counted(pkg, NF, 2)
    t5, e5 = _counted(pkg, NF, 5)
    assert t2 == t5 and e2 == e5, (t2, t5, e2, e5)
    assert t2 == ['nf_resflow_spectral', 'nf_resflow_fwd', 'nf_resflow_bwd', 'nf_resflow_spectral_bwd'], t2
    assert e2 == ['nf_resflow_spectral', 'nf_resflow_fwd'], e2
    for names in (t2, e2):
        for old in ('nf_resmlp_fwd', 'nf_spectral_weights', 'nf_resmlp_train_bwd', 'nf_chan_affine_fwd'):
            assert old not in names, (old, names)
    t2o, _ = _counted(pkg, NF, 2, stack=False)                           # the switch really selects the per-block path
    assert 'nf_resmlp_train_bwd' in t2o and 'nf_resflow_fwd' not in t2o


# ---- device draws ------------------------------------------------------------------------------------------------------------------
def _stack_with(NF, pkg, net, x, gz, gld, n_terms, noise, seed):
    """one training pass through the autograd Function with the given source of draws"""
    pairs = net.net._resflow_run(0, x, 1)
    assert len(pairs) == net.n_layers
    _, params = NF._resflow_members(pairs)
    xx = x.clone().requires_grad_(True)
    z, ld = NF._ResFlowStack.apply(xx, torch.zeros(x.shape[0], device=DEV), (pairs, 0), n_terms, noise, seed, *params)
    torch.autograd.backward([z, ld], [gz, gld])
    return z.detach(), ld.detach(), xx.grad.detach(), [p.grad.detach().clone() for p in params]


@pytest.mark.parametrize('B,D', [(257, 2), (65, 3), (64, 4), (3, 1)])
def test_device_draws_fed_back_are_bit_identical(pkg, NF, B, D):
    """what nf_resflow_draws writes for the seed words, fed back as explicit arrays, gives the bits of the in-kernel draws: values, input
    gradient, parameter gradients.  The lengths have no row index -- (L, 2, S) -- so equality over several workgroups (B = 257) also says
    that all rows of a block share one length."""
    L = 3
    NF.RESFLOW_STACK = True
    net0 = _net(pkg, L, D, seed=8).to(DEV).train()
    x = 0.7 * torch.randn(B, D, device=DEV)
    gz, gld = torch.randn(B, D, device=DEV), torch.full((B, ), -1.0 / B, device=DEV)
    seed = torch.tensor([20240229, 5], dtype=torch.int64, device=DEV)
    a = _stack_with(NF, pkg, copy.deepcopy(net0), x, gz, gld, None, None, seed.clone())
    n_terms, noise = NF.resflow_draws(seed, L, B, D, 1, 1)
    assert tuple(n_terms.shape) == (L, 2, 1) and tuple(noise.shape) == (L, 2, B, 1, D)
    assert int(n_terms.min()) >= 2 and int(n_terms.max()) <= 64
    b = _stack_with(NF, pkg, copy.deepcopy(net0), x, gz, gld, n_terms, noise, None)
    for i, what in enumerate(('z', 'ld', 'd_x')):
        assert torch.equal(a[i], b[i]), what
    for ga, gb in zip(a[3], b[3]):
        assert torch.equal(ga, gb)
    # evaluation (unbias: S = 4, n_exact = 8) through the model: draws = 'device' against the same arrays
    net = copy.deepcopy(net0).eval()
    net.draws = 'device'
    net.seed.copy_(seed)
    with torch.no_grad():
        z1, ld1 = net(x)
    assert net.seed.tolist() == [20240229, 6]                           # the stream offset advanced on the device
    n_terms, noise = NF.resflow_draws(seed, L, B, D, 4, 8)
    net2 = copy.deepcopy(net0).eval()
    with torch.no_grad():
        packed, _ = NF.resflow_spectral_(net2.net._resflow_run(0, x, 1), D)
        z2, ld2 = torch.empty_like(x), torch.zeros(B, device=DEV)
        pkg._native.call('nf_resflow_fwd', x.data_ptr(), z2.data_ptr(), ld2.data_ptr(), None, packed.data_ptr(), n_terms.data_ptr(),
                         noise.data_ptr(), None, 2, 4, 8, 0, 0.5, L, 0, B, D, pkg._native.stream())
    assert torch.equal(z1, z2) and torch.equal(ld1, ld2)


def test_device_draws_change_from_pass_to_pass(pkg, NF):
    NF.RESFLOW_STACK = True
    net = _net(pkg, 3, 2, seed=8).to(DEV).train()
    net.draws = 'device'
    net.seed.copy_(torch.tensor([77, 0]))
    x = 0.7 * torch.randn(64, 2, device=DEV)
    d0 = NF.resflow_draws(net.seed, 3, 64, 2, 1, 1)
    _, ld_a = net(x)
    d1 = NF.resflow_draws(net.seed, 3, 64, 2, 1, 1)
    _, ld_b = net(x)
    assert net.seed.tolist() == [77, 2]
    assert not torch.equal(d0[1], d1[1]) and not torch.equal(ld_a, ld_b)
    assert float((d0[1] - d1[1]).abs().max()) > 0.5                     # other noise, not a shifted copy of a few entries


def test_device_draw_statistics(pkg, NF):
    """8 192 lengths at a fixed seed: mean(n - n_exact) within six standard errors of a geometric(0.5)'s 2 (6 sqrt(2 / 8192) = 0.094 < 0.1);
    the noise: mean and variance within six standard errors of 0 and 1"""
    seed = torch.tensor([424242, 0], dtype=torch.int64, device=DEV)
    n_terms, _ = NF.resflow_draws(seed, 2048, 1, 2, 4, 8, slots=1)
    assert n_terms.numel() == 8192
    extra = (n_terms.double() - 8.0).cpu()
    assert float(extra.min()) >= 1.0
    assert abs(float(extra.mean()) - 2.0) <= 0.1, float(extra.mean())
    assert abs(float((extra == 1).double().mean()) - 0.5) <= 6 * math.sqrt(0.25 / 8192)
    n_terms, noise = NF.resflow_draws(seed, 2, 4096, 4, 4, 8, slots=2)
    v = noise[:, 1].double().flatten().cpu()                            # slot 1: every sample is live
    n = v.numel()
    assert n == 2 * 4096 * 4 * 4
    assert abs(float(v.mean())) <= 6.0 / math.sqrt(n), float(v.mean())
    assert abs(float(v.var()) - 1.0) <= 6.0 * math.sqrt(2.0 / n), float(v.var())
    v0 = noise[:, 0, :, 0].double().flatten().cpu()                     # slot 0: sample 0 is live, the rest stays zero
    assert abs(float(v0.mean())) <= 6.0 / math.sqrt(v0.numel()) and abs(float(v0.var()) - 1.0) <= 6.0 * math.sqrt(2.0 / v0.numel())
    assert not noise[:, 0, :, 1:].any()
    for d in range(4):                                                   # the features of a row are distinct draws
        for e in range(d):
            c = float((noise[:, 1, :, :, d].double() * noise[:, 1, :, :, e].double()).mean())
            assert abs(c) <= 6.0 / math.sqrt(n / 4), (d, e, c)


# ---- inverse ------------------------------------------------------------------------------------------------------------------------
def _oracle_margins(pkg, net, z):
    """the oracle's fixed-point loop (iresblock.py:236-255) in float64 on the CPU, last block first: per block (iterations, max|dx| at
    the exit iteration, max|dx| at the one before)"""
    net = copy.deepcopy(net).double().eval()
    out = []
    z = z.double()
    layers = list(net.net.layers)
    with torch.no_grad():
        for i in range(len(layers) - 1, 0, -2):
            a, blk = layers[i - 1], layers[i]
            x, hist = z.clone(), []
            for _ in range(100):
                x, prev = z - blk.g_fn(x), x
                hist.append(float((x - prev).abs().max()))
                if hist[-1] < blk.ftol:
                    break
            blk.g_fn(x)                                                  # the reference's final g_fn(x): one more power iteration
            out.append((len(hist), hist[-1], hist[-2] if len(hist) > 1 else float('inf')))
            z = x * torch.exp(a.log_scale) + a.bias
    return out[::-1]


def _clear_seed(pkg, B, D, L, logdet):
    """the first seed in 0 .. 9 at which, for every block, max|dx| at the exit iteration and at the one before are each at least 10 % away
    from ftol in the float64 oracle: float32 kernels then leave the loop at the same iteration (knife-edge exits are excluded)"""
    for s in range(10):
        net = _net(pkg, L, D, logdet=logdet, seed=600 + s)          # (checked on the CPU: a seed qualifies at every B of the tests below)
        z = torch.randn(B, D, generator=torch.Generator().manual_seed(s))
        ftol = net.net.layers[1].ftol
        if all(abs(last - ftol) >= 0.1 * ftol and abs(before - ftol) >= 0.1 * ftol and it < 100 for it, last, before in _oracle_margins(pkg, net, z)):
            return net, z
    raise AssertionError('no seed in 0 .. 9 keeps every exit 10 %% away from ftol at B=%d' % B)


@pytest.mark.parametrize('logdet', ['exact', 'unbias'])
@pytest.mark.parametrize('B', [1, 64, 1000, 4096, 4097])
def test_inverse_matches_per_block(pkg, NF, B, logdet):
    L, D = 3, 2
    cap = pkg._native.header_constant('NF_RESFLOW_INV_WG_MAX_ROWS')
    assert cap == 4096
    net0, z = _clear_seed(pkg, B, D, L, logdet)
    z = z.to(DEV)
    keep = z.clone()
    res = {}
    for stack in (True, False):
        net = copy.deepcopy(net0).to(DEV).eval()
        NF.RESFLOW_STACK = stack
        _seed(5)
        with _Calls(pkg) as calls:
            x, ld = net.backward(z)
        blocks = [m for m in net.net.layers if isinstance(m, pkg.InvertibleResLinear)]
        res[stack] = (x, ld, torch.stack([b.last_inverse_iters for b in blocks]).cpu(), _uv(net), calls.names)
    assert torch.equal(z, keep), 'the caller\'s tensor was mutated'
    on_stack = B <= cap
    assert ('nf_resflow_inv' in res[True][4]) == on_stack and 'nf_resflow_inv' not in res[False][4]
    if on_stack:
        assert res[True][4] == ['nf_resflow_inv'], res[True][4]
    else:
        assert 'nf_resmlp_fixed_point_step' in res[True][4]              # above the row cap: the per-block path, unchanged
    assert res[True][2].tolist() == res[False][2].tolist(), (res[True][2], res[False][2])
    assert 1 <= int(res[True][2].min()) and int(res[True][2].max()) < 100
    _close(res[True][0], res[False][0], 2e-4, 'x')
    _close(res[True][1], res[False][1], 2e-4, 'ld')
    for k in res[False][3]:
        assert float((res[True][3][k] - res[False][3][k]).abs().max()) <= 2e-6, k


def _converge_power_iteration(net):
    """weight_u / weight_v := the top singular pair of weight_bar (float64 SVD): the state the power iteration has reached in a model
    that has been in use, and a fixed point of it"""
    with torch.no_grad():
        for m in net.modules():
            if 'weight_u' in getattr(m, '_buffers', {}):
                U, _, Vh = torch.linalg.svd(m.weight_bar.detach().double().view(m.weight_bar.shape[0], -1), full_matrices=False)
                m.weight_u.copy_(U[:, 0])
                m.weight_v.copy_(Vh[0])


@pytest.mark.parametrize('B', [1, 64, 1000, 4096])
def test_inverse_round_trip(pkg, NF, B):
    """net.backward(net(y)[0]) returns y to 2e-4.  Every g_fn call runs one power iteration (spectral_norm.py:26-43), so the inverse
    inverts the map the forward applied only where the iteration has converged: with the random weight_u / weight_v of a fresh model
    the forward's W_eff and the inverse's differ, and the reference's own arithmetic in float64 on the CPU misses y by 2.4e-2 at B = 1
    (6e-2 at B = 64) for this model; with converged vectors it returns y to 1.3e-6.  The model is therefore put into the converged
    state first."""
    NF.RESFLOW_STACK = True
    net = _net(pkg, 3, 2, logdet='exact', seed=2)
    _converge_power_iteration(net)
    net = net.to(DEV).eval()
    y = torch.randn(B, 2, device=DEV)
    with torch.no_grad():
        z, ld = net(y)
        x, ldi = net.backward(z)
    _close(x, y, 2e-4, 'round trip')
    _close(ldi, -ld, 2e-4, 'log-det of the round trip')


# ---- ActNorm initialisation, deterministic mode, trainer ------------------------------------------------------------------------------
def test_actnorm_initialisation_hands_over_to_the_stack(pkg, NF):
    net0 = _net(pkg, 3, 2, seed=6, init=False)
    x = (1.5 * torch.randn(128, 2) + 0.4).to(DEV)
    res = {}
    for stack in (True, False):
        net = copy.deepcopy(net0).to(DEV).train()
        NF.RESFLOW_STACK = stack
        _seed(3)
        with _Calls(pkg) as first:
            z, ld = net(x)
        acts = [m for m in net.net.layers if isinstance(m, pkg.ActNorm)]
        assert all(a.initialized for a in acts)
        with _Calls(pkg) as second:
            net(x)
        res[stack] = (z.detach(), ld.detach(), [a.log_scale.detach().clone() for a in acts], [a.bias.detach().clone() for a in acts],
                      first.names, second.names)
    assert 'nf_resflow_fwd' not in res[True][4] and 'nf_resmlp_fwd' in res[True][4]       # the first batch: the per-layer path
    assert res[True][5] == ['nf_resflow_spectral', 'nf_resflow_fwd'], res[True][5]        # the second: the stack
    assert 'nf_resflow_fwd' not in res[False][5]
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    for i in (2, 3):
        for a, b in zip(res[True][i], res[False][i]):
            assert torch.equal(a, b)
    assert float(res[True][2][0].abs().max()) > 0.1                                        # really data dependent


def test_deterministic_mode_gives_identical_gradients(pkg, NF):
    N = pkg._native
    net0 = _net(pkg, 5, 2, seed=12)
    x = 0.7 * torch.randn(1000, 2)
    gz, gld = torch.randn(1000, 2), torch.full((1000, ), -1.0e-3)
    was = N.deterministic()
    try:
        N.deterministic(True)
        a = _train_pass(NF, net0, x, gz, gld, True)
        b = _train_pass(NF, net0, x, gz, gld, True)
    finally:
        N.deterministic(was)
    assert N.deterministic_timeouts() == 0
    assert torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def _trainer_nets(pkg, n):
    nets = [_net(pkg, 4, 2, seed=21, init=False) for _ in range(n)]
    for net in nets:
        for m in net.modules():
            if isinstance(m, pkg.InvertibleResLinear):
                m.noise_on_cpu = False
        net.to(DEV)
        net.seed.copy_(torch.tensor([99, 0]))
    return nets


def test_trainer_graph_draws_afresh_on_every_replay(pkg, NF):
    """FlowTrainer(graph=True) serves a ResFlow: it switches the draws to the device, captures the step, and 20 replays of an IDENTICAL
    batch at learning rate 0 (constant parameters) give finite losses that differ -- every replay draws its own lengths and noise"""
    NF.RESFLOW_STACK = True
    train = import_module(pkg.__name__ + '.train')
    (net, ) = _trainer_nets(pkg, 1)
    tr = train.FlowTrainer(net, lr=0.0, graph=True, warmup=2)
    assert net.draws == 'device'
    y = 0.8 * torch.randn(256, 2, device=DEV)
    _seed(1)
    losses = []
    for s in range(23):
        _, loss = tr.train_on_batch(y)
        losses.append(float(loss))
        assert math.isfinite(losses[-1]), (s, losses)
    assert tr._g_fb is not None and tr.graph, 'the ResFlow step was not captured'
    replays = losses[3:]
    assert len(replays) == 20
    assert len(set(replays)) >= 19, replays                             # (two equal float32 losses by chance are not an error)
    assert net.seed.tolist()[0] == 99 and net.seed.tolist()[1] >= 22


def test_trainer_graph_matches_eager_device_draws(pkg, NF):
    """graph and eager trainers in lockstep from the same state and seed words: parameters equal to 2e-6 after every step"""
    NF.RESFLOW_STACK = True
    train = import_module(pkg.__name__ + '.train')
    nets = _trainer_nets(pkg, 2)
    nets[0].draws = 'device'
    eager = train.FlowTrainer(nets[0], lr=1e-3, graph=False)
    graph = train.FlowTrainer(nets[1], lr=1e-3, graph=True, warmup=2)
    gen = torch.Generator(device=DEV).manual_seed(3)
    for s in range(6):
        y = 0.8 * torch.randn(256, 2, device=DEV, generator=gen)
        if s == 2:                                                       # the capturing call takes one extra eager step on its batch first
            eager.train_on_batch(y)
        _seed(50 + s)                                                    # (the first call initialises the ActNorms on the per-layer path:
        eager.train_on_batch(y)                                          #  host draws, the same for both)
        _seed(50 + s)
        graph.train_on_batch(y)
        assert nets[0].seed.tolist() == nets[1].seed.tolist(), s
        for (k, a), b in zip(nets[0].named_parameters(), nets[1].parameters()):
            assert float((a - b).abs().max()) <= 2e-6, (s, k, float((a - b).abs().max()))
    assert graph._g_fb is not None, 'the ResFlow step was not captured'
