"""
Gradient clipping, the non-finite step guard and averaged weights of FlowTrainer on the torch.optim path (CPU): the host forms that
are the parity reference of the fused path (tests/test_gpu_trainer_guard.py).  The reference's loop (main.py:78-92) has none of the
three; the yardsticks are torch's own: torch.nn.utils.clip_grad_norm_, torch.optim, Tensor.lerp_.
The last test checks the new C entry points' argument validation, which happens on the host before any launch.
"""
import ctypes
import importlib

import pytest
import torch

PKG = 'normalizing-flows-pytorch_amd'


def _train():
    return importlib.import_module(PKG + '.train')


class _Affine(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.s = torch.nn.Parameter(torch.tensor([0.1, -0.2, 0.3]))
        self.t = torch.nn.Parameter(torch.tensor([0.5, 0.0, -0.5]))


class _TinyFlow(torch.nn.Module):
    """per-sample independent toy flow with one child module: z = y exp(s) + t, ld = sum s"""

    def __init__(self):
        super().__init__()
        self.aff = _Affine()
        self.frozen = torch.nn.Parameter(torch.ones(2), requires_grad=False)

    def forward(self, y):
        return y * torch.exp(self.aff.s) + self.aff.t, self.aff.s.sum().expand(y.shape[0])

    def backward(self, z):
        return (z - self.aff.t) * torch.exp(-self.aff.s), (-self.aff.s.sum()).expand(z.shape[0])


def _batches(n, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(16, 3, generator=g) * 1.5 + 0.3 for _ in range(n)]


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters() if p.requires_grad])


def _trainable(net):
    return [p for p in net.parameters() if p.requires_grad]


def _opt_state(tr):
    """every tensor of the torch optimizer's state, cloned, in a fixed order"""
    out = []
    for p in tr.bucket.params:
        for k, v in sorted(tr.optim.state.get(p, {}).items()):
            out.append((k, v.clone() if isinstance(v, torch.Tensor) else v))
    return out


def _same_state(a, b):
    assert len(a) == len(b)
    for (ka, va), (kb, vb) in zip(a, b):
        assert ka == kb
        assert torch.equal(va, vb) if isinstance(va, torch.Tensor) else va == vb, ka


def _hand_step(train, ref, opt, y, max_norm=None):
    z, ld = ref(y)                                               # main.py:82-89, with the clip between backward and step
    loss = train.nll_loss(z, ld)
    opt.zero_grad()
    loss.backward()
    norm64 = torch.cat([p.grad.double().reshape(-1) for p in _trainable(ref)]).norm()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(_trainable(ref), max_norm)
    opt.step()
    return float(norm64)


# ---- clipping ---------------------------------------------------------------------------------------------------------------------------
def test_clipping_equals_clip_grad_norm_then_step_to_the_bit():
    train = _train()
    ys = _batches(7)
    # the unclipped run's gradient norms place the threshold: between the smallest and the largest of the seven
    probe, popt = _TinyFlow(), None
    popt = torch.optim.Adam(_trainable(probe), lr=1e-2, weight_decay=0.01)
    free = [_hand_step(train, probe, popt, y) for y in ys]
    c = 0.5 * (min(free) + max(free))
    assert min(free) < c < max(free)

    net = _TinyFlow()
    tr = train.FlowTrainer(net, lr=1e-2, weight_decay=0.01, max_grad_norm=c)
    assert isinstance(tr.optim, torch.optim.Adam)
    ref = _TinyFlow()
    opt = torch.optim.Adam(_trainable(ref), lr=1e-2, weight_decay=0.01)
    norms = []
    for y in ys:
        tr.train_on_batch(y)
        norms.append(_hand_step(train, ref, opt, y, max_norm=c))
        assert torch.equal(_flat(net), _flat(ref))
        st = tr.guard_state()
        assert st['grad_norm'] == pytest.approx(norms[-1], rel=1e-5)
        assert st['clip_scale'] == pytest.approx(min(1.0, c / (norms[-1] + 1e-6)), rel=1e-5)
    print('gradient norms', norms, 'threshold', c)
    assert any(n > c for n in norms) and any(n + 1e-6 < c for n in norms), 'both branches of the clip must occur'
    assert tr.guard_state()['skipped'] == 0 and tr.guard_state()['steps'] == 7


# ---- the guard --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['adam', 'rmsprop'])
def test_nonfinite_batch_is_skipped_and_training_goes_on(name):
    train = _train()
    kw = dict(lr=1e-2, optimizer=name, decay_steps=2, decay_ratio=0.5, skip_nonfinite=True, ema_decay=0.9)
    ys = _batches(5)
    bad = ys[4].clone()
    bad[3, 1] = float('nan')                                     # one sample of the batch
    a_net, b_net = _TinyFlow(), _TinyFlow()
    a = train.FlowTrainer(a_net, **kw)                           # sees the bad batch after two good ones
    b = train.FlowTrainer(b_net, **kw)                           # never sees it
    for y in ys[:2]:
        a.train_on_batch(y)
        b.train_on_batch(y)
    before = (_flat(a_net).clone(), _opt_state(a), [e.clone() for e in a._ema])
    assert a._sched.last_epoch == 2
    a.train_on_batch(bad)
    assert a.guard_state()['skipped'] == 1 and a.guard_state()['steps'] == 2
    assert torch.equal(_flat(a_net), before[0])
    _same_state(_opt_state(a), before[1])
    assert all(torch.equal(e, e0) for e, e0 in zip(a._ema, before[2]))
    assert a._sched.last_epoch == 3                              # the schedule position advances, as an unconditional scheduler.step() does
    assert bool(torch.isfinite(_flat(a_net)).all())
    # the next finite batches train; apart from the schedule position the run equals the one that never saw the bad batch
    b._sched.step()                                              # (put b's schedule where a's stands)
    for y in ys[2:4]:
        a.train_on_batch(y)
        b.train_on_batch(y)
    assert not torch.equal(_flat(a_net), before[0])
    assert torch.equal(_flat(a_net), _flat(b_net))
    assert all(torch.equal(e, f) for e, f in zip(a._ema, b._ema))
    assert b.guard_state()['skipped'] == 0 and a.guard_state()['steps'] == b.guard_state()['steps'] == 4


def test_guard_off_lets_the_nan_through():
    """the contrast: without skip_nonfinite the same batch destroys the parameters (what the guard is for)"""
    train = _train()
    net = _TinyFlow()
    tr = train.FlowTrainer(net, lr=1e-2, max_grad_norm=1.0)
    bad = _batches(1)[0]
    bad[3, 1] = float('nan')
    tr.train_on_batch(bad)
    assert not bool(torch.isfinite(_flat(net)).all())


def test_skip_with_a_captured_framework_optimizer_is_refused_only_on_the_gpu():
    """on the CPU graph=True records nothing real (a stand-in factory re-runs the closure): the host check is allowed there"""
    train = _train()
    from tests.test_dist_cpu import _RerunGraph
    tr = train.FlowTrainer(_TinyFlow(), lr=1e-2, graph=True, warmup=1, graph_factory=_RerunGraph, skip_nonfinite=True, max_grad_norm=2.0)
    _RerunGraph.trainer = tr
    ys = _batches(3)
    for y in ys:
        tr.train_on_batch(y)
    assert tr._g_fb is not None
    bad = ys[0].clone()
    bad[0, 0] = float('inf')
    before = _flat(tr.net).clone()
    tr.train_on_batch(bad)
    assert torch.equal(_flat(tr.net), before) and tr.guard_state()['skipped'] == 1


# ---- the average ------------------------------------------------------------------------------------------------------------------------
def test_ema_matches_the_hand_written_float32_loop():
    train = _train()
    d = 0.9
    net = _TinyFlow()
    tr = train.FlowTrainer(net, lr=1e-2, ema_decay=d)
    ref = _TinyFlow()
    opt = torch.optim.Adam(_trainable(ref), lr=1e-2)
    avg = None
    for t, y in enumerate(_batches(7)):
        tr.train_on_batch(y)
        _hand_step(train, ref, opt, y)
        with torch.no_grad():
            if avg is None:
                avg = [p.detach().clone() for p in _trainable(ref)]
                assert all(torch.equal(e, p) for e, p in zip(tr._ema, _trainable(net))), 'the first update is a copy'
            else:
                for e, p in zip(avg, _trainable(ref)):
                    e.lerp_(p.detach(), 1.0 - d)                 # e + (1 - d) (p - e)
        assert all(torch.equal(e, f) for e, f in zip(tr._ema, avg)), t
    assert not any(torch.equal(e, p) for e, p in zip(tr._ema, _trainable(net)))


def test_ema_weights_swaps_in_place_and_restores_also_on_an_exception():
    train = _train()
    net = _TinyFlow()
    tr = train.FlowTrainer(net, lr=1e-2, ema_decay=0.9)
    ys = _batches(4)
    for y in ys[:3]:
        tr.train_on_batch(y)
    iterate, avg = _flat(net).clone(), torch.cat([e.reshape(-1) for e in tr._ema]).clone()
    ptrs = [p.data_ptr() for p in net.parameters()]
    with tr.ema_weights():
        assert torch.equal(_flat(net), avg)
        assert [p.data_ptr() for p in net.parameters()] == ptrs
        lp = tr.log_py(ys[3])
        with pytest.raises(RuntimeError, match='ema_weights'):
            tr.train_on_batch(ys[3])
        with pytest.raises(RuntimeError, match='nest'):
            with tr.ema_weights():
                pass
    assert torch.equal(_flat(net), iterate)
    assert torch.equal(torch.cat([e.reshape(-1) for e in tr._ema]), avg)
    assert not torch.equal(lp, tr.log_py(ys[3]))
    with pytest.raises(KeyError):
        with tr.ema_weights():
            raise KeyError('from the body')
    assert torch.equal(_flat(net), iterate) and not tr._in_ema
    tr.train_on_batch(ys[3])                                     # training goes on
    assert not torch.equal(_flat(net), iterate)


def test_ema_weights_without_ema_decay_raises():
    train = _train()
    tr = train.FlowTrainer(_TinyFlow(), lr=1e-2, max_grad_norm=1.0)
    with pytest.raises(ValueError, match='ema_decay'):
        tr.ema_weights()
    with pytest.raises(ValueError, match='ema_decay'):
        train.FlowTrainer(_TinyFlow(), ema_decay=1.0)


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_with_ema_and_skipped(tmp_path):
    train = _train()
    kw = dict(lr=1e-2, skip_nonfinite=True, ema_decay=0.9, max_grad_norm=5.0)
    ys = _batches(6)
    bad = ys[5].clone()
    bad[0, 0] = float('nan')
    a = train.FlowTrainer(_TinyFlow(), **kw)
    for y in ys[:3] + [bad]:
        a.train_on_batch(y)
    f = str(tmp_path / 'ckpt.pth')
    a.save_ckpt(4, f)
    ckpt = torch.load(f)
    assert set(ckpt) == {'net', 'optim', 'step', 'ema', 'skipped'} and ckpt['skipped'] == 1
    assert list(ckpt['ema']) == ['aff.s', 'aff.t']               # the trainable parameters, named and shaped as in net.state_dict()
    for k, v in ckpt['ema'].items():
        assert v.shape == ckpt['net'][k].shape and v.dtype == ckpt['net'][k].dtype
    assert all(torch.equal(ckpt['ema'][k], e) for k, e in zip(('aff.s', 'aff.t'), a._ema))
    # the reference's way of reading the three keys it knows (main.py:102-107)
    ref_net = _TinyFlow()
    ref_opt = torch.optim.Adam(ref_net.parameters(), lr=1.0)
    ref_net.load_state_dict(ckpt['net'])
    ref_opt.load_state_dict(ckpt['optim'])
    assert ref_opt.param_groups[0]['lr'] == pytest.approx(1e-2) and torch.equal(_flat(ref_net), _flat(a.net))

    b = train.FlowTrainer(_TinyFlow(), **kw)
    ema_ptrs = [e.data_ptr() for e in b._ema]
    assert b.load_ckpt(f) == 4
    assert [e.data_ptr() for e in b._ema] == ema_ptrs            # restored into the tensors that exist
    assert all(torch.equal(e, e0) for e, e0 in zip(b._ema, a._ema)) and b.guard_state()['skipped'] == 1
    for y in ys[3:5]:                                            # the next update blends (no second "first copy")
        a.train_on_batch(y)
        b.train_on_batch(y)
    assert torch.equal(_flat(a.net), _flat(b.net))
    assert all(torch.equal(e, e0) for e, e0 in zip(b._ema, a._ema))
    assert not any(torch.equal(e, p) for e, p in zip(b._ema, _trainable(b.net)))


def test_checkpoint_without_ema_seeds_the_average(tmp_path):
    train = _train()
    ys = _batches(4)
    plain = train.FlowTrainer(_TinyFlow(), lr=1e-2)
    for y in ys[:3]:
        plain.train_on_batch(y)
    f = str(tmp_path / 'plain.pth')
    plain.save_ckpt(3, f)
    assert set(torch.load(f)) == {'net', 'optim', 'step'}       # with the options off the file is what it always was
    d = 0.75
    tr = train.FlowTrainer(_TinyFlow(), lr=1e-2, ema_decay=d)
    tr.load_ckpt(f)
    loaded = [p.detach().clone() for p in _trainable(tr.net)]
    assert all(torch.equal(e, p) for e, p in zip(tr._ema, loaded)) and tr.guard_state()['skipped'] == 0
    tr.train_on_batch(ys[3])
    for e, p0, p in zip(tr._ema, loaded, _trainable(tr.net)):    # blended with the seed, not copied
        assert torch.equal(e, p0.clone().lerp_(p.detach(), 1.0 - d)) and not torch.equal(e, p)


def test_options_off_change_nothing():
    train = _train()
    ys = _batches(5)
    a_net, b_net = _TinyFlow(), _TinyFlow()
    a = train.FlowTrainer(a_net, lr=1e-2, max_grad_norm=None, skip_nonfinite=False, ema_decay=None)
    b = train.FlowTrainer(b_net, lr=1e-2)
    for y in ys:
        a.train_on_batch(y)
        b.train_on_batch(y)
    assert torch.equal(_flat(a_net), _flat(b_net))
    assert a._ema is None and not a._guarded
    with pytest.raises(ValueError, match='guard state'):
        a.guard_state()


def test_flat_optimizers_take_the_options_and_default_to_none():
    """construction alone (the launches are the GPU tests'): off means no control block and no average"""
    train = _train()
    nfdist = importlib.import_module(PKG + '.dist')
    for cls in (train.FlatAdam, train.FlatRMSprop):
        ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
        opt = cls(nfdist.GradBucket(ps, flatten_params=True), lr=1e-2)
        assert not opt.guarded and opt.guard_ctl is None and opt.ema is None
        opt = cls(nfdist.GradBucket(ps, flatten_params=True), lr=1e-2, max_grad_norm=5.0)
        assert opt.guarded and opt.ema is None and opt.guard_ctl.dtype == torch.int32 and opt.guard_ctl.numel() == 8
        opt = cls(nfdist.GradBucket(ps, flatten_params=True), lr=1e-2, ema_decay=0.99)
        assert opt.guarded and torch.equal(opt.ema, opt.bucket.flat_params) and opt.ema.data_ptr() != opt.bucket.flat_params.data_ptr()
        assert opt.guard_state() == {'grad_norm': 0.0, 'clip_scale': 0.0, 'skipped': 0, 'steps': 0}
        assert set(opt.state_dict()) == set(opt.MOMENTS) | {'step', 'lr'}      # not torch optimizer state


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------------
def test_new_entry_points_validate_arguments_without_gpu(pkg):
    pkg.build()
    lib = pkg._native.load()
    ctl = (ctypes.c_int * 8)()
    some = (ctypes.c_float * 8)()
    ctl_p, some_p = ctypes.addressof(ctl), ctypes.addressof(some)
    assert lib.nf_grad_guard(some_p, -1, 1.0, 1, some_p, ctl_p, None, None) == 10001
    assert lib.nf_grad_guard(some_p, 8, 1.0, 1, some_p, None, None, None) == 10001
    assert lib.nf_adam_step_guarded(some_p, some_p, some_p, some_p, ctl_p, some_p, 0.9, 0.999, 1e-8, 0.0, ctl_p, None, 0.0, -1, None) == 10001
    assert lib.nf_rmsprop_step_guarded(some_p, some_p, some_p, some_p, 0.99, 1e-8, 0.0, ctl_p, None, 0.0, -1, None) == 10001
    assert lib.nf_swap_f32(some_p, some_p, -1, None) == 10001
    # n = 0: success, and nothing is launched (there is no device here to launch on)
    assert lib.nf_grad_guard(None, 0, 1.0, 1, None, ctl_p, None, None) == 0
    assert lib.nf_adam_step_guarded(None, None, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, ctl_p, None, 0.0, 0, None) == 0
    assert lib.nf_rmsprop_step_guarded(None, None, None, None, 0.99, 1e-8, 0.0, ctl_p, None, 0.0, 0, None) == 0
    assert lib.nf_swap_f32(None, None, 0, None) == 0
    assert list(ctl) == [0] * 8
