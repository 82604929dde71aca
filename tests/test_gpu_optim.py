"""
The fused optimizers on the MI355X (csrc/optim.hip): FlatRMSprop against torch.optim.RMSprop (main.py:56-59), the StepLR schedule as a
launch inside a captured graph against torch.optim.lr_scheduler.StepLR stepped after every optimizer step (main.py:68-70, :89-90), and
optimizer state travelling between the flat buffers and torch.optim in checkpoint format (main.py:94-107).

Bar: the project's own for Adam (tests/test_gpu_ops.py::test_flat_adam_matches_torch_adam), 2e-6 + 2e-6 |x| per entry.  On the CPU
torch's float32 RMSprop sits at 0.08 of it from its float64 self on these inputs, a float32 restatement of the kernel's arithmetic at
0.07 from torch's float32.
"""
import importlib

import numpy as np
import pytest
import torch

from tests._optim import SPECIAL, _close, _feed, _fresh, _pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(32, 32), (32, ), (1, ), (2, 32), (1, 2, 1, 1)]
OPTS = [('FlatAdam', 'Adam'), ('FlatRMSprop', 'RMSprop')]


@pytest.fixture(scope='module')
def mods(pkg):
    pkg._native.load()
    return importlib.import_module(pkg.__name__ + '.train'), importlib.import_module(pkg.__name__ + '.dist')


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_flat_rmsprop_matches_torch_rmsprop(mods, wd):
    train, _ = mods
    pa, pb, bucket, g = _pair(mods, SHAPES)
    opt_a = train.FlatRMSprop(bucket, lr=1e-2, weight_decay=wd)
    opt_b = torch.optim.RMSprop(pb, lr=1e-2, weight_decay=wd)
    for it in range(7):
        _feed(bucket, pb, _fresh(bucket, g, special=(it == 0)))     # (step 0: the square average starts at zero under the tiny entries)
        opt_a.step()
        opt_b.step()
        for k, (a, b) in enumerate(zip(pa, pb)):
            _close(a, b, 'rmsprop wd %g step %d tensor %d' % (wd, it, k))
    assert int(opt_a.step_count) == 7
    assert pa[0].data_ptr() == bucket.flat_params.data_ptr()


@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 4099])
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'offset4B'])
def test_rmsprop_tails_and_misaligned_ends(pkg, mods, n, aligned):
    """one flat tensor of n elements: the float4 body with its scalar tail where the buffers sit on 16 bytes, the scalar form where they
    start 4 bytes off -- through the C entry point on views with guard elements on both sides, which must stay untouched.
    The square average is held to the same bar: alpha crosses the C ABI as a float, so the kernel's 1 - alpha is 1 - float32(0.99),
    9.3e-7 (relative) from the float32(1 - 0.99) torch multiplies by; with two float32 roundings on top that stays under 2e-6 |v|."""
    N = pkg._native
    off = 4 if aligned else 1
    g = torch.Generator(device=DEV).manual_seed(n)
    bufs = [torch.randn(n + 8, device=DEV, generator=g) for _ in range(3)]
    bufs[2].abs_()
    p, gr, v = (b[off:off + n] for b in bufs)
    assert (p.data_ptr() % 16 == 0) == aligned
    gr[:min(n, len(SPECIAL))] = torch.tensor(SPECIAL[:n], device=DEV)
    before = [b.clone() for b in bufs]
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.RMSprop([q], lr=1e-2, weight_decay=0.01)
    opt.state[q]['step'] = torch.tensor(0.0)
    opt.state[q]['square_avg'] = v.clone()
    q.grad = gr.clone()
    step, lr = torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1, ), 1e-2, device=DEV)
    N.call('nf_rmsprop_step', p.data_ptr(), gr.data_ptr(), v.data_ptr(), step.data_ptr(), lr.data_ptr(), 0.99, 1e-8, 0.01, 1.0, n, N.stream())
    opt.step()
    _close(p, q, 'n %d param' % n)
    _close(v, opt.state[q]['square_avg'], 'n %d square_avg' % n)
    assert int(step) == 1
    for b, b0 in zip(bufs, before):
        assert torch.equal(b[:off], b0[:off]) and torch.equal(b[off + n:], b0[off + n:]), 'wrote outside [0, n)'
    assert torch.equal(bufs[1], before[1])                       # the gradient is read only


@pytest.mark.parametrize('ratio', [0.5, 0.9])
@pytest.mark.parametrize('flat_cls,torch_cls', OPTS, ids=[o[1] for o in OPTS])
def test_steplr_decays_inside_a_captured_graph(mods, flat_cls, torch_cls, ratio):
    """opt.step() alone in a hipGraph; 7 replays cross three decay boundaries (decay_steps = 2) without any host-side rate update"""
    train, _ = mods
    pa, pb, bucket, g = _pair(mods, SHAPES, seed=1)
    opt_a = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=0.01, decay_steps=2, decay_ratio=ratio)
    opt_b = getattr(torch.optim, torch_cls)(pb, lr=1e-2, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.StepLR(opt_b, step_size=2, gamma=ratio)
    start = bucket.flat_params.clone()
    _feed(bucket, pb, _fresh(bucket, g))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt_a.step()                                             # warm-up on a side stream ...
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(opt_a.sched_pos) == 1 and int(opt_a.step_count) == 1
    bucket.flat_params.copy_(start)                              # ... and undone: both sides start from step 0
    for k in opt_a.MOMENTS:
        getattr(opt_a, k).zero_()
    opt_a.step_count.zero_()
    opt_a.set_schedule(1e-2, 0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_a.step()
    assert int(opt_a.sched_pos) == 0                             # (a capture runs nothing)
    for it in range(7):
        _feed(bucket, pb, _fresh(bucket, g, special=(it == 3)))
        want_lr = np.float32(sched.get_last_lr()[0])             # the rate of THIS step: StepLR as it stood before it
        graph.replay()
        opt_b.step()
        sched.step()
        got_lr = np.float32(float(opt_a.lr))
        assert abs(float(got_lr) - float(want_lr)) <= float(np.spacing(want_lr)), (it, got_lr, want_lr)
        assert want_lr == np.float32(1e-2 * ratio ** (it // 2)) or ratio == 0.9
        for k, (a, b) in enumerate(zip(pa, pb)):
            _close(a, b, '%s ratio %g replay %d tensor %d' % (torch_cls, ratio, it, k))
    assert int(opt_a.step_count) == 7 and int(opt_a.sched_pos) == 7


def test_no_schedule_means_no_schedule_state(mods):
    train, _ = mods
    pa, pb, bucket, g = _pair(mods, SHAPES)
    opt = train.FlatAdam(bucket, lr=1e-3)
    assert opt.decay_steps is None and not hasattr(opt, 'sched_pos')
    _feed(bucket, pb, _fresh(bucket, g))
    opt.step()
    opt.set_lr(5e-4)
    assert float(opt.lr) == float(np.float32(5e-4))


@pytest.mark.parametrize('flat_cls,torch_cls', OPTS, ids=[o[1] for o in OPTS])
def test_optimizer_state_travels_both_ways_on_the_device(mods, flat_cls, torch_cls):
    train, nfdist = mods
    # flat -> torch: three fused steps, the state into a fresh torch optimizer, the same fourth gradient on both sides
    pa, pb, bucket, g = _pair(mods, SHAPES, seed=2)
    opt_a = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=0.01)
    for _ in range(3):
        _feed(bucket, pb, _fresh(bucket, g))
        opt_a.step()
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    opt_b = getattr(torch.optim, torch_cls)(pb, lr=1e-2, weight_decay=0.01)
    opt_b.load_state_dict(opt_a.torch_state_dict())
    _feed(bucket, pb, _fresh(bucket, g))
    opt_a.step()
    opt_b.step()
    for k, (a, b) in enumerate(zip(pa, pb)):
        _close(a, b, '%s flat -> torch, tensor %d' % (torch_cls, k))
    assert float(opt_b.state[pb[0]]['step']) == 4.0
    # torch -> flat
    pa, pb, bucket, g = _pair(mods, SHAPES, seed=3)
    opt_b = getattr(torch.optim, torch_cls)(pb, lr=1e-2, weight_decay=0.01)
    for _ in range(3):
        _feed(bucket, pb, _fresh(bucket, g))
        opt_b.step()
    with torch.no_grad():
        for a, b in zip(pa, pb):
            a.copy_(b)
    opt_a = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=0.01)
    opt_a.load_torch_state_dict(opt_b.state_dict())
    assert pa[0].data_ptr() == bucket.flat_params.data_ptr()
    _feed(bucket, pb, _fresh(bucket, g))
    opt_a.step()
    opt_b.step()
    for k, (a, b) in enumerate(zip(pa, pb)):
        _close(a, b, '%s torch -> flat, tensor %d' % (torch_cls, k))
    assert int(opt_a.step_count) == 4
