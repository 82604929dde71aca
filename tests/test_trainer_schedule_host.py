"""
The learning-rate rule (linear warmup times constant / StepLR / cosine decay) and the Adamax / AdamW optimizers of FlowTrainer, without
a GPU: the host restatement of nf_lr_schedule against torch's own schedulers stepped after every optim.step() (main.py:89-90), the
argument checks, checkpoints in torch.optim.Adamax / AdamW format (main.py:94-107), and the torch.optim path of the trainer.
The launches themselves are tests/test_gpu_optim_recipes.py's.

Bar of the rule: 1e-12 of the base rate -- torch's chained schedulers and the closed form differ by a few double roundings (1.1e-16 of
the base at most over these schedules).  Past the cosine's end the rate is lr_min exactly: it holds, torch's CosineAnnealingLR does not.
"""
import ctypes
import importlib

import pytest
import torch
from torch.optim import lr_scheduler as S

from tests.test_dist_cpu import _RerunGraph
from tests.test_trainer_guard_host import _TinyFlow, _batches, _flat

PKG = 'normalizing-flows-pytorch_amd'
SHAPES = [(32, 32), (32, ), (1, ), (2, 32), (1, 2, 1, 1)]
BASE = 1e-3
W, START, T, LR_MIN = 5, 0.25, 12, 1e-5
RECIPES = [('FlatAdamax', 'Adamax', ('exp_avg', 'exp_inf')), ('FlatAdamW', 'AdamW', ('exp_avg', 'exp_avg_sq'))]


def _mods():
    return importlib.import_module(PKG + '.train'), importlib.import_module(PKG + '.dist')


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _flat_opt(cls_name='FlatAdam', **kw):
    train, nfdist = _mods()
    ps = _params()
    bucket = nfdist.GradBucket(ps, flatten_params=True)
    return ps, bucket, getattr(train, cls_name)(bucket, **kw)


def _torch_rates(make_sched, n):
    """the rate each of the steps 0 .. n - 1 runs at under torch's scheduler(s), stepped after optim.step()"""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    sched = make_sched(opt)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]['lr'])
        p.grad = torch.ones(1)
        opt.step()
        sched.step()
    return out


def _warm(o):
    return S.LinearLR(o, start_factor=START, end_factor=1.0, total_iters=W)


SCHEDULES = {
    'warmup': (dict(lr_warmup_steps=W, lr_warmup_start=START), _warm, W + T),
    'cosine': (dict(cosine_steps=T, lr_min=LR_MIN), lambda o: S.CosineAnnealingLR(o, T_max=T, eta_min=LR_MIN), T),
    'warmup_cosine': (dict(lr_warmup_steps=W, lr_warmup_start=START, cosine_steps=T, lr_min=LR_MIN),
                      lambda o: S.SequentialLR(o, [_warm(o), S.CosineAnnealingLR(o, T_max=T, eta_min=LR_MIN)], milestones=[W]), W + T),
    'warmup_step': (dict(lr_warmup_steps=W, lr_warmup_start=START, decay_steps=3, decay_ratio=0.5),
                    lambda o: S.SequentialLR(o, [_warm(o), S.StepLR(o, step_size=3, gamma=0.5)], milestones=[W]), 20),
}


# ---- 1. the rule against torch's schedulers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SCHEDULES))
def test_scheduled_lr_is_torchs_schedulers_stepped_after_the_optimizer(name):
    import warnings
    kw, make, last = SCHEDULES[name]
    _, _, opt = _flat_opt(lr=BASE, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                          # (SequentialLR's own deprecation chatter about the epoch argument)
        want = _torch_rates(make, last + 1)
    worst = 0.0
    for pos in range(last + 1):
        got = opt.scheduled_lr(BASE, pos)
        worst = max(worst, abs(got - want[pos]) / BASE)
        assert abs(got - want[pos]) <= 1e-12 * BASE, (name, pos, got, want[pos])
    print('%s: worst difference %.3e of the base rate over pos 0 .. %d' % (name, worst, last))
    assert float(opt.lr) == float(torch.tensor(opt.scheduled_lr(BASE, 0), dtype=torch.float32))      # the rate of the first step


@pytest.mark.parametrize('name', ['cosine', 'warmup_cosine'])
def test_rate_holds_at_lr_min_past_the_cosines_end(name):
    kw = SCHEDULES[name][0]
    w = kw.get('lr_warmup_steps', 0)
    _, _, opt = _flat_opt(lr=BASE, **kw)
    for pos in range(w + T, w + T + 7):
        assert opt.scheduled_lr(BASE, pos) == LR_MIN, pos
    assert opt.scheduled_lr(BASE, w + T - 1) > LR_MIN


def test_decay_steps_alone_is_the_steplr_it_was():
    _, _, opt = _flat_opt(lr=BASE, decay_steps=3, decay_ratio=0.9)
    assert not opt._rule.general
    for pos in range(20):
        assert opt.scheduled_lr(BASE, pos) == BASE * 0.9 ** (pos // 3)
    _, _, plain = _flat_opt(lr=BASE)
    assert not plain._rule.active and not hasattr(plain, 'sched_pos')


# ---- 2. argument errors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw,match', [
    (dict(decay_steps=3, cosine_steps=4), 'decay_steps'),
    (dict(lr_warmup_steps=3, lr_warmup_start=0.0), 'lr_warmup_start'),
    (dict(lr_warmup_steps=3, lr_warmup_start=1.5), 'lr_warmup_start'),
    (dict(lr_warmup_steps=3, lr_warmup_start=-0.1), 'lr_warmup_start'),
    (dict(lr_warmup_steps=0), 'lr_warmup_steps'),
    (dict(cosine_steps=0), 'cosine_steps'),
    (dict(decay_steps=0), 'decay_steps'),
    (dict(cosine_steps=4, lr_min=-1e-6), 'lr_min'),
    (dict(cosine_steps=4, lr_min=2e-3), 'lr_min'),
])
def test_schedule_arguments_are_checked(kw, match):
    train, _ = _mods()
    for cls in ('FlatAdam', 'FlatRMSprop', 'FlatAdamax', 'FlatAdamW'):
        with pytest.raises(ValueError, match=match):
            _flat_opt(cls, lr=BASE, **kw)
    with pytest.raises(ValueError, match=match):
        train.FlowTrainer(_TinyFlow(), lr=BASE, **kw)


def test_new_entry_points_validate_arguments_without_gpu(pkg):
    pkg.build()
    lib = pkg._native.load()
    N = pkg._native
    CONST, STEP, COS = (N.header_constant(k) for k in ('NF_LR_CONST', 'NF_LR_STEP', 'NF_LR_COSINE'))
    assert (CONST, STEP, COS) == (0, 1, 2)
    ctl = (ctypes.c_int * 8)()
    some = (ctypes.c_float * 8)()
    ctl_p, p = ctypes.addressof(ctl), ctypes.addressof(some)
    bad = 10001
    # nf_lr_schedule(lr, base_lr, pos, warmup_steps, warmup_start, kind, span, arg, stream): every refusal comes before any launch
    assert lib.nf_lr_schedule(None, p, p, 5, 0.25, COS, 12, 1e-5, None) == bad
    assert lib.nf_lr_schedule(p, None, p, 5, 0.25, COS, 12, 1e-5, None) == bad
    assert lib.nf_lr_schedule(p, p, None, 5, 0.25, COS, 12, 1e-5, None) == bad
    assert lib.nf_lr_schedule(p, p, p, -1, 0.25, COS, 12, 1e-5, None) == bad
    assert lib.nf_lr_schedule(p, p, p, 5, 0.0, COS, 12, 1e-5, None) == bad
    assert lib.nf_lr_schedule(p, p, p, 5, 1.5, CONST, 0, 0.0, None) == bad
    assert lib.nf_lr_schedule(p, p, p, 5, float('nan'), CONST, 0, 0.0, None) == bad
    assert lib.nf_lr_schedule(p, p, p, 5, 0.25, 3, 12, 1e-5, None) == bad
    assert lib.nf_lr_schedule(p, p, p, 5, 0.25, -1, 12, 1e-5, None) == bad
    assert lib.nf_lr_schedule(p, p, p, 5, 0.25, COS, 0, 1e-5, None) == bad
    assert lib.nf_lr_schedule(p, p, p, 5, 0.25, STEP, 0, 0.5, None) == bad
    assert lib.nf_lr_schedule(p, p, p, 0, 0.25, COS, 12, -1e-5, None) == bad
    # the four step entry points: (param, grad, m, s, step, lr, b1, b2, eps, wd, grad_scale | ctl, ema, ema_decay, n, stream)
    for name in ('nf_adamax_step', 'nf_adamw_step'):
        f = getattr(lib, name)
        assert f(p, p, p, p, ctl_p, p, 0.9, 0.999, 1e-8, 0.0, 1.0, -1, None) == bad
        assert f(None, p, p, p, ctl_p, p, 0.9, 0.999, 1e-8, 0.0, 1.0, 4, None) == bad
        assert f(p, p, p, None, ctl_p, p, 0.9, 0.999, 1e-8, 0.0, 1.0, 4, None) == bad
        assert f(p, p, p, p, ctl_p, None, 0.9, 0.999, 1e-8, 0.0, 1.0, 4, None) == bad
        assert f(None, None, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, None) == 0
    for name in ('nf_adamax_step_guarded', 'nf_adamw_step_guarded'):
        f = getattr(lib, name)
        assert f(p, p, p, p, ctl_p, p, 0.9, 0.999, 1e-8, 0.0, ctl_p, None, 0.0, -1, None) == bad
        assert f(p, p, p, p, ctl_p, p, 0.9, 0.999, 1e-8, 0.0, None, None, 0.0, 4, None) == bad
        assert f(p, None, p, p, ctl_p, p, 0.9, 0.999, 1e-8, 0.0, ctl_p, None, 0.0, 4, None) == bad
        assert f(p, p, p, p, None, p, 0.9, 0.999, 1e-8, 0.0, ctl_p, None, 0.0, 4, None) == bad
        assert f(None, None, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, ctl_p, None, 0.0, 0, None) == 0
    assert list(ctl) == [0] * 8 and list(some) == [0.0] * 8


# ---- 3. checkpoints in torch.optim.Adamax / AdamW format ---------------------------------------------------------------------------------
def _slices(flat, ps):
    o, out = 0, []
    for p in ps:
        out.append(flat[o:o + p.numel()].view_as(p))
        o += p.numel()
    return out


@pytest.mark.parametrize('flat_cls,torch_cls,moments', RECIPES, ids=[o[1] for o in RECIPES])
def test_torch_state_dict_is_what_torch_optim_writes_and_loads_into_it(flat_cls, torch_cls, moments):
    train, _ = _mods()
    ps, bucket, opt = _flat_opt(flat_cls, lr=1e-2, weight_decay=0.01)
    assert (opt.KIND, opt.MOMENTS) == (torch_cls, moments)
    g = torch.Generator().manual_seed(1)
    for k in moments:
        getattr(opt, k).copy_(torch.rand(bucket.numel, generator=g) + 0.01 * len(k))
    opt.step_count.fill_(5)
    sd = opt.torch_state_dict()
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ref = getattr(torch.optim, torch_cls)(qs, lr=1e-2, weight_decay=0.01)
    for q in qs:
        q.grad = torch.ones_like(q)
    ref.step()
    want = ref.state_dict()
    assert set(sd) == set(want)
    assert set(sd['state']) == set(want['state']) == set(range(len(SHAPES)))
    for i in want['state']:
        assert set(sd['state'][i]) == set(want['state'][i]) == set(moments) | {'step'}
        for k, v in want['state'][i].items():
            assert sd['state'][i][k].shape == v.shape and sd['state'][i][k].dtype == v.dtype, (i, k)
    assert len(sd['param_groups']) == 1 and set(sd['param_groups'][0]) == set(want['param_groups'][0])
    assert sd['param_groups'][0]['params'] == want['param_groups'][0]['params']
    assert sd['param_groups'][0]['lr'] == 1e-2
    if torch_cls == 'AdamW':
        assert sd['param_groups'][0]['decoupled_weight_decay'] is True
    ref.load_state_dict(sd)
    for k in moments:
        for q, want_slice in zip(qs, _slices(getattr(opt, k), ps)):
            assert torch.equal(ref.state[q][k], want_slice), k
    assert all(float(ref.state[q]['step']) == 5.0 for q in qs)
    # and back: three torch steps, their state into a fresh flat optimizer
    gen = torch.Generator().manual_seed(2)
    for _ in range(3):
        for q in qs:
            q.grad = torch.randn(q.shape, generator=gen)
        ref.step()
    _, _, back = _flat_opt(flat_cls, lr=1e-2, weight_decay=0.01)
    back.load_torch_state_dict(ref.state_dict())
    for k in moments:
        for q, got in zip(qs, _slices(getattr(back, k), ps)):
            assert torch.equal(got, ref.state[q][k]), k
    assert int(back.step_count) == 8
    # hyper-parameters are launch arguments: a file written with others is refused, and so is plain Adam's file by FlatAdamW
    other = getattr(torch.optim, torch_cls)(qs, lr=1e-2, weight_decay=0.5)
    with pytest.raises(ValueError, match='weight_decay'):
        back.load_torch_state_dict(other.state_dict())
    if torch_cls == 'AdamW':
        adam = torch.optim.Adam(qs, lr=1e-2, weight_decay=0.01)
        with pytest.raises(ValueError, match='decoupled_weight_decay'):
            back.load_torch_state_dict(adam.state_dict())
        _, _, plain = _flat_opt('FlatAdam', lr=1e-2, weight_decay=0.01)
        with pytest.raises(ValueError, match='decoupled_weight_decay'):
            plain.load_torch_state_dict(ref.state_dict())


def test_scheduled_state_dict_holds_the_next_rate_and_the_base():
    kw = SCHEDULES['warmup_cosine'][0]
    _, _, opt = _flat_opt('FlatAdamax', lr=BASE, **kw)
    opt.set_schedule(BASE, 7)
    group = opt.torch_state_dict()['param_groups'][0]
    assert group['lr'] == opt.scheduled_lr(BASE, 7) and group['initial_lr'] == BASE
    assert float(opt.lr) == float(torch.tensor(opt.scheduled_lr(BASE, 7), dtype=torch.float32)) and int(opt.sched_pos) == 7
    opt.set_lr(2 * BASE)                                          # the BASE rate of a scheduled optimizer
    assert float(opt.base_lr) == 2 * BASE and float(opt.lr) == float(torch.tensor(opt.scheduled_lr(2 * BASE, 7), dtype=torch.float32))


# ---- 4. the torch.optim path of the trainer ----------------------------------------------------------------------------------------------
def test_torch_optim_path_follows_the_rule_through_a_captured_step_and_a_checkpoint(tmp_path):
    train, _ = _mods()
    kw = dict(lr=1e-2, optimizer='adamax', lr_warmup_steps=4, lr_warmup_start=0.25, cosine_steps=7, lr_min=1e-4,
              graph=True, warmup=1, graph_factory=_RerunGraph)
    tr = train.FlowTrainer(_TinyFlow(), **kw)
    _RerunGraph.trainer = tr
    assert isinstance(tr.optim, torch.optim.Adamax)
    rule = tr._rule
    assert tr.current_lr() == rule.rate(1e-2, 0) == pytest.approx(0.25e-2, rel=1e-12)
    ys = _batches(10)
    seen = []
    for k, y in enumerate(ys):
        tr.train_on_batch(y)
        pos = k + 1 if k == 0 else k + 2                         # (the capturing call takes one extra eager step on its batch)
        assert tr._sched.last_epoch == pos
        assert tr.current_lr() == rule.rate(1e-2, pos), (k, pos)
        seen.append(tr.current_lr())
    assert tr._g_fb is not None
    # pos 4: the warmup's end, the cosine's start; pos 11 = 4 + 7: the floor, reached exactly
    assert seen[2] == pytest.approx(1e-2, rel=1e-12) and seen[-2] > 1e-4 and seen[-1] == 1e-4
    f = str(tmp_path / 'sched.pth')
    tr.save_ckpt(11, f)
    group = torch.load(f)['optim']['param_groups'][0]
    assert group['lr'] == 1e-4 and group['initial_lr'] == 1e-2
    torch.optim.Adamax(_TinyFlow().parameters(), lr=1.0).load_state_dict(torch.load(f)['optim'])

    # a fresh trainer continues the schedule at the saved position ...
    kw_eager = dict(kw, graph=False)
    kw_eager.pop('graph_factory')
    a = train.FlowTrainer(_TinyFlow(), **kw_eager)
    assert a.load_ckpt(f, resume_schedule=True) == 11
    assert a._sched.last_epoch == 11 and a.current_lr() == rule.rate(1e-2, 11)
    before = _flat(a.net).clone()
    a.train_on_batch(ys[0])
    assert a._sched.last_epoch == 12 and a.current_lr() == 1e-4 and not torch.equal(_flat(a.net), before)
    # ... and without resume_schedule restarts at position 0 from the saved rate, warmup included (the reference's StepLR behaviour)
    b = train.FlowTrainer(_TinyFlow(), **kw_eager)
    b.load_ckpt(f)
    assert b._sched.last_epoch == 0 and b.current_lr() == rule.rate(1e-4, 0) == pytest.approx(0.25e-4, rel=1e-12)


def test_torch_optim_adamax_trainer_equals_a_hand_loop_with_torchs_schedulers():
    """the whole torch.optim path against main.py:82-90 written out with torch.optim.Adamax and SequentialLR, while t <= T"""
    train, _ = _mods()
    net, ref = _TinyFlow(), _TinyFlow()
    tr = train.FlowTrainer(net, lr=1e-2, optimizer='adamax', lr_warmup_steps=3, lr_warmup_start=0.5, cosine_steps=5, lr_min=1e-4)
    params = [p for p in ref.parameters() if p.requires_grad]
    opt = torch.optim.Adamax(params, lr=1e-2)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sched = S.SequentialLR(opt, [S.LinearLR(opt, start_factor=0.5, end_factor=1.0, total_iters=3),
                                     S.CosineAnnealingLR(opt, T_max=5, eta_min=1e-4)], milestones=[3])
        for y in _batches(8):
            tr.train_on_batch(y)
            z, ld = ref(y)
            loss = train.nll_loss(z, ld)
            opt.zero_grad()
            loss.backward()
            opt.step()
            sched.step()
            assert abs(tr.current_lr() - opt.param_groups[0]['lr']) <= 1e-12 * 1e-2
    # the two rates differ by 1e-10 (relative) at most, far below float32's 6e-8: the parameters may part by an ulp per step at most
    assert torch.allclose(_flat(net), _flat(ref), rtol=1e-6, atol=1e-7)


# ---- 5. the optimizer switch ---------------------------------------------------------------------------------------------------------------
def test_adamax_and_adamw_are_accepted_and_other_names_raise_the_references_words():
    train, _ = _mods()
    assert isinstance(train.FlowTrainer(_TinyFlow(), optimizer='adamax').optim, torch.optim.Adamax)
    w = train.FlowTrainer(_TinyFlow(), optimizer='adamw', weight_decay=0.01).optim
    assert isinstance(w, torch.optim.AdamW) and w.param_groups[0]['weight_decay'] == 0.01
    with pytest.raises(Exception, match='optimizer "sgd" is currently not supported'):
        train.FlowTrainer(_TinyFlow(), optimizer='sgd')
    assert issubclass(train.FlatAdamax, train._FlatOptimizer) and issubclass(train.FlatAdamW, train._FlatOptimizer)
