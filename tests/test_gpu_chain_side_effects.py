"""What the persistent chain launches leave behind BESIDES their outputs (csrc/conv_chain.hip): the BatchNorm bookkeeping of the
forward (saved constants, running statistics, batch counters), the per-layer sums and the gamma / beta accumulators of the backward,
and the fused coupling at sizes where a tile is ragged.  Workgroup 0 writes the bookkeeping out in one pass per step from a stash in
shared memory, and the coupling requests its operands in batches; these tests pin down what must not move when it does:

1. the forward's bookkeeping, recomputed in float64 from the pre-BatchNorm outputs the launch itself stored -- one launch, the same
   launch twice (the update applied twice), a run of three steps with parameters of their own, and evaluation mode;
2. the backward's sums against float64 sums of what the launch stored, and the accumulators ADDED to (prefilled with random values;
   the same fp32 addition of the same two operands, so exact), once and twice, with a layer whose accumulators are absent;
3. the fused coupling against the unfused path (conditioner launch + coupling kernel) at odd batch sizes and single samples.
"""
import ctypes

import pytest
import torch

from tests import test_gpu_convnet as T
from tests import test_gpu_convnet_run as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NB = 5
EPS, MOM = 1e-5, 0.1

# (I0, O, H, W), B, split -- the smallest shapes that reach each path of the kernels
SHAPES = [
    ((24, 48, 8, 8), 1, 'channel'),         # one workgroup: no exchange
    ((24, 48, 8, 8), 5, 'channel'),         # five workgroups
    ((96, 192, 4, 4), 3, 'checker'),        # 32-pixel tiles, the last tile half empty
    ((6, 12, 16, 16), 3, 'channel'),        # two tiles per sample with the halo hand-over, six workgroups
    ((8, 16, 4, 8), 4, 'channel'),          # a geometry without an instantiation of its own
]
RUNS = [SHAPES[1], SHAPES[2]]


def _side(pkg, shape, B, split, n, seed=23):
    Nn = pkg._native
    mode = Nn.SPLIT_CHANNEL if split == 'channel' else Nn.SPLIT_CHECKER
    assert int(Nn.load().nf_convnet_chain_usable(B, *shape))
    side = R._Side(pkg, n, *shape, B, mode, 0, seed=seed)
    need = int(Nn.load().nf_convnet_chain_ws_floats(B, *shape))      # (a sample split over two tiles adds the halo slots)
    if need > side.slots.numel():
        side.slots = torch.zeros(need, device=DEV)
    for t in side.steps:                    # (rmean and rvar are random already)
        for j in range(NB):
            t['nbt'][j].fill_(41)
    return side


def _forward(side, training, run, gen0):
    descs = side.fwd_descs(gen0)
    if run:
        arr = R._array(descs)
        side.Nn.call('nf_convnet_chain_fwd_run', ctypes.addressof(arr), side.n, *side.args, training, EPS, MOM, side.Nn.stream())
    else:
        for d in descs:
            side.Nn.call('nf_convnet_chain_fwd', ctypes.addressof(d), *side.args, training, EPS, MOM, side.Nn.stream())
    torch.cuda.synchronize()
    assert side.Nn.persistent_timeouts() == 0


def _close(a, ref, what):
    ref = ref.to(torch.float64)
    err = (a.double() - ref).abs()
    assert bool((err <= 1e-5 + 1e-5 * ref.abs()).all()), '%s: max error %g' % (what, float(err.max()))


def _check_training_bookkeeping(side, before, times):
    """save_* and the running statistics after ``times`` launches, from the launch's own acts (float64 on the host)"""
    for s, t in enumerate(side.steps):
        for l in range(NB):
            a = t['acts'][l].double()
            assert not torch.isnan(a).any()
            n = a.numel() // 32
            mean = a.mean((0, 2, 3))
            var = ((a - mean.view(1, 32, 1, 1)) ** 2).mean((0, 2, 3))
            unb = var * n / (n - 1)
            what = 'step %d layer %d' % (s, l)
            _close(t['save_mean'][l], mean, what + ' save_mean')
            _close(t['save_invstd'][l], 1.0 / torch.sqrt(var + EPS), what + ' save_invstd')
            rm, rv = before[s]['rmean'][l].double(), before[s]['rvar'][l].double()
            for _ in range(times):
                rm, rv = (1 - MOM) * rm + MOM * mean, (1 - MOM) * rv + MOM * unb
            _close(t['rmean'][l], rm, what + ' running mean after %d launches' % times)
            _close(t['rvar'][l], rv, what + ' running variance after %d launches' % times)
            assert int(t['nbt'][l]) == 41 + times, what + ' num_batches_tracked'


def _snapshot(side):
    return [{k: [v.clone() for v in t[k]] for k in ('rmean', 'rvar', 'nbt')} for t in side.steps]


def _fwd_bookkeeping(pkg, shape, B, split, n, run):
    side = _side(pkg, shape, B, split, n)
    before = _snapshot(side)
    _forward(side, 1, run, 1)
    _check_training_bookkeeping(side, before, 1)
    _forward(side, 1, run, n + 1)           # the same descriptors again (under fresh exchange tags): the update applied twice
    _check_training_bookkeeping(side, before, 2)
    return side


@pytest.mark.parametrize('shape,B,split', SHAPES)
def test_forward_bookkeeping_single_launch(pkg, shape, B, split):
    _fwd_bookkeeping(pkg, shape, B, split, 1, False)


@pytest.mark.parametrize('shape,B,split', RUNS)
def test_forward_bookkeeping_run_of_three(pkg, shape, B, split):
    """every step has parameters and statistics of its own: a stash left over from another step shows"""
    _fwd_bookkeeping(pkg, shape, B, split, 3, True)


def test_forward_bookkeeping_evaluation_mode(pkg):
    shape, B, split = SHAPES[1]
    side = _side(pkg, shape, B, split, 1)
    before = _snapshot(side)
    _forward(side, 0, False, 1)
    t = side.steps[0]
    for l in range(NB):
        for k in ('rmean', 'rvar', 'nbt'):
            assert torch.equal(t[k][l], before[0][k][l]), '%s[%d] changed in evaluation mode' % (k, l)
        assert torch.equal(t['save_mean'][l], t['rmean'][l])
        ref = (1.0 / torch.sqrt(t['rvar'][l].double() + EPS)).float()
        ulp = torch.nextafter(ref.abs(), torch.full_like(ref, float('inf'))) - ref.abs()
        assert bool(((t['save_invstd'][l] - ref).abs() <= 2 * ulp).all()), 'save_invstd[%d]' % l


# ---- the backward's sums and accumulators --------------------------------------------------------------------------------------------
def _backward(side, bw, training, run, gen0, drop=None):
    descs = side.bwd_descs(bw, gen0)
    if drop is not None:
        for d in descs:
            d.g_gamma[drop], d.g_beta[drop] = None, None
    if run:
        arr = R._array(descs)
        side.Nn.call('nf_convnet_chain_bwd_run', ctypes.addressof(arr), side.n, *side.args, training, side.Nn.stream())
    else:
        for d in descs:
            side.Nn.call('nf_convnet_chain_bwd', ctypes.addressof(d), *side.args, training, side.Nn.stream())
    torch.cuda.synchronize()
    assert side.Nn.persistent_timeouts() == 0


def _sinks(pkg, shape, B, split, n, run, drop=None):
    side = _side(pkg, shape, B, split, n)
    _forward(side, 1, run, 1)
    bw = side.bwd_buffers(5)
    g = torch.Generator(device=DEV).manual_seed(77)
    for u in bw['k']:
        for l in range(NB):
            u['g_gamma'][l].copy_(torch.randn(32, device=DEV, generator=g))
            u['g_beta'][l].copy_(torch.randn(32, device=DEV, generator=g))
    pre = [{k: [v.clone() for v in u[k]] for k in ('g_gamma', 'g_beta')} for u in bw['k']]
    _backward(side, bw, 1, run, n + 1, drop)
    once = [{k: [v.clone() for v in u[k]] for k in ('g_gamma', 'g_beta')} for u in bw['k']]
    for k, u in enumerate(bw['k']):
        t = side.steps[n - 1 - k]
        for l in range(NB):
            what = 'entry %d layer %d' % (k, l)
            sg, sgx = u['sum_g'][l][:32], u['sum_gx'][l][:32]
            gn = u['gn'][l].double()
            assert not torch.isnan(gn).any()
            xh = (t['acts'][l].double() - t['save_mean'][l].double().view(1, 32, 1, 1)) * t['save_invstd'][l].double().view(1, 32, 1, 1)
            ref_g, ref_gx = gn.sum((0, 2, 3)), (gn * xh).sum((0, 2, 3))
            for got, ref, name in ((sg, ref_g, 'sum_g'), (sgx, ref_gx, 'sum_gx')):
                tol = 2e-4 * max(1.0, float(ref.abs().max()))
                err = float((got.double() - ref).abs().max())
                assert err <= tol, '%s %s: error %g > %g' % (what, name, err, tol)
            if l == drop:                   # no accumulators for this layer: the buffers the descriptor no longer names stay as they were
                assert torch.equal(u['g_beta'][l], pre[k]['g_beta'][l]) and torch.equal(u['g_gamma'][l], pre[k]['g_gamma'][l])
            else:
                assert torch.equal(u['g_beta'][l], pre[k]['g_beta'][l] + sg), what + ' g_beta'
                assert torch.equal(u['g_gamma'][l], pre[k]['g_gamma'][l] + sgx), what + ' g_gamma'
    _backward(side, bw, 1, run, 2 * n + 1, drop)         # the same launch again: added once more
    for k, u in enumerate(bw['k']):
        for l in range(NB):
            if l == drop:
                continue
            sg, sgx = u['sum_g'][l][:32], u['sum_gx'][l][:32]
            assert torch.equal(u['g_beta'][l], once[k]['g_beta'][l] + sg), 'entry %d layer %d g_beta, second launch' % (k, l)
            assert torch.equal(u['g_gamma'][l], once[k]['g_gamma'][l] + sgx), 'entry %d layer %d g_gamma, second launch' % (k, l)


@pytest.mark.parametrize('shape,B,split', SHAPES)
def test_backward_sinks_accumulate_single_launch(pkg, shape, B, split):
    _sinks(pkg, shape, B, split, 1, False)


@pytest.mark.parametrize('shape,B,split', RUNS)
def test_backward_sinks_accumulate_run_of_three(pkg, shape, B, split):
    _sinks(pkg, shape, B, split, 3, True)


def test_backward_sinks_absent_for_one_layer(pkg):
    shape, B, split = SHAPES[1]
    _sinks(pkg, shape, B, split, 1, False, drop=2)


# ---- the fused coupling at ragged sizes, against the unfused path --------------------------------------------------------------------
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('dims,masking,odd,B', [((3, 32, 32), 'checkerboard', True, 3), ((12, 16, 16), 'checkerboard', False, 1),
                                                ((48, 8, 8), 'checkerboard', True, 5), ((48, 8, 8), 'channelwise', True, 1)])
def test_fused_coupling_at_ragged_sizes(pkg, dims, masking, odd, B, training):
    """body, tolerances and the cap on ReLU flips are those of test_coupling_fused_into_the_conditioner_launch (it asserts
    coupling_fusable first): forward, backward, inverse and round trip"""
    T.test_coupling_fused_into_the_conditioner_launch(pkg, dims, masking, odd, B, training)
    torch.cuda.synchronize()
    assert pkg._native.persistent_timeouts() == 0
