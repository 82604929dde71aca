"""
The fused Adamax and AdamW steps, their guarded forms and the warmup / cosine schedule launch on the MI355X (csrc/optim.hip,
csrc/optim_guard.hip, csrc/nf_optim_recipes.h) against torch.optim.Adamax / AdamW, torch.nn.utils.clip_grad_norm_ and torch's
schedulers stepped after every optimizer step (main.py:56-70, :89-90 with the optimizers and schedules Glow and Flow++ are published
with), and all of it inside a captured FlowTrainer step.

Bar: the project's own for the fused optimizers (tests/test_gpu_optim.py), 2e-6 + 2e-6 |x| per entry, on parameters, moments and
averages.  The rate: the float32 rounding of the host's double, or one float32 ulp from it (the device's cos is far closer than half
an ulp of a float to the host's; only a rounding boundary can differ).
"""
import copy
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
from torch.optim import lr_scheduler as S

from tests._optim import SPECIAL, _close, _feed, _fresh, _pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(32, 32), (32, ), (1, ), (2, 32), (1, 2, 1, 1)]        # tests/test_gpu_optim.py
RECIPES = [('FlatAdamax', 'Adamax', 'nf_adamax_step'), ('FlatAdamW', 'AdamW', 'nf_adamw_step')]
ALL = [('FlatAdam', 'Adam'), ('FlatRMSprop', 'RMSprop'), ('FlatAdamax', 'Adamax'), ('FlatAdamW', 'AdamW')]
W, START, T, LR_MIN = 5, 0.25, 12, 1e-5


@pytest.fixture(scope='module')
def mods(pkg):
    pkg._native.load()
    return importlib.import_module(pkg.__name__ + '.train'), importlib.import_module(pkg.__name__ + '.dist')


def _all_close(opt_a, opt_b, pa, pb, what):
    """parameters and both moments, tensor by tensor"""
    o = 0
    for k, (a, b) in enumerate(zip(pa, pb)):
        _close(a, b, '%s tensor %d' % (what, k))
        for name in opt_a.MOMENTS:
            _close(getattr(opt_a, name)[o:o + a.numel()], opt_b.state[b][name], '%s tensor %d %s' % (what, k, name))
        o += a.numel()


# ---- 1. the plain steps against torch.optim ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('flat_cls,torch_cls,entry', RECIPES, ids=[o[1] for o in RECIPES])
def test_flat_recipe_matches_torch_optim(mods, flat_cls, torch_cls, entry, wd):
    train, _ = mods
    pa, pb, bucket, g = _pair(mods, SHAPES)
    opt_a = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=wd)
    opt_b = getattr(torch.optim, torch_cls)(pb, lr=1e-2, weight_decay=wd)
    assert opt_a.ENTRY == entry
    for it in range(7):
        _feed(bucket, pb, _fresh(bucket, g, special=(it == 0)))   # (step 0: the moments start at zero under the tiny entries)
        opt_a.step()
        opt_b.step()
        _all_close(opt_a, opt_b, pa, pb, '%s wd %g step %d' % (torch_cls, wd, it))
        if it == 0 and wd == 0.0 and torch_cls == 'Adamax':
            # a zero gradient on a zero exp_inf: u = max(0, 0 + eps) = eps, and 0 / eps leaves the parameter where it was
            assert float(opt_a.exp_inf[0]) == float(np.float32(1e-8)) and float(opt_a.exp_avg[0]) == 0.0
            assert float(bucket.flat_params.detach()[0]) == float(pb[0].detach().reshape(-1)[0])
    assert int(opt_a.step_count) == 7
    assert pa[0].data_ptr() == bucket.flat_params.data_ptr()


# ---- 2. the C entry points: tails, misaligned ends, guard elements ------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 4099])
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'offset4B'])
@pytest.mark.parametrize('flat_cls,torch_cls,entry', RECIPES, ids=[o[1] for o in RECIPES])
def test_recipe_tails_and_misaligned_ends(pkg, mods, flat_cls, torch_cls, entry, n, aligned):
    """one flat tensor of n elements: the float4 body with its scalar tail where the buffers sit on 16 bytes, the scalar form where they
    start 4 bytes off -- on views with guard elements on both sides, which must stay untouched"""
    N = pkg._native
    train, _ = mods
    names = getattr(train, flat_cls).MOMENTS
    off = 4 if aligned else 1
    g = torch.Generator(device=DEV).manual_seed(n)
    bufs = [torch.randn(n + 8, device=DEV, generator=g) for _ in range(4)]
    bufs[3].abs_()                                               # exp_inf / exp_avg_sq are not negative
    p, gr, m, s = (b[off:off + n] for b in bufs)
    assert (p.data_ptr() % 16 == 0) == aligned
    gr[:min(n, len(SPECIAL))] = torch.tensor(SPECIAL[:n], device=DEV)
    before = [b.clone() for b in bufs]
    q = torch.nn.Parameter(p.clone())
    opt = getattr(torch.optim, torch_cls)([q], lr=1e-2, weight_decay=0.01)
    opt.state[q]['step'] = torch.tensor(0.0)
    opt.state[q][names[0]] = m.clone()
    opt.state[q][names[1]] = s.clone()
    q.grad = gr.clone()
    step, lr = torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1, ), 1e-2, device=DEV)
    N.call(entry, p.data_ptr(), gr.data_ptr(), m.data_ptr(), s.data_ptr(), step.data_ptr(), lr.data_ptr(), 0.9, 0.999, 1e-8, 0.01, 1.0, n,
           N.stream())
    opt.step()
    _close(p, q, '%s n %d param' % (torch_cls, n))
    _close(m, opt.state[q][names[0]], '%s n %d %s' % (torch_cls, n, names[0]))
    _close(s, opt.state[q][names[1]], '%s n %d %s' % (torch_cls, n, names[1]))
    assert int(step) == 1
    for b, b0 in zip(bufs, before):
        assert torch.equal(b[:off], b0[:off]) and torch.equal(b[off + n:], b0[off + n:]), 'wrote outside [0, n)'
    assert torch.equal(bufs[1], before[1])                       # the gradient is read only


# ---- 3. the guarded forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flat_cls,torch_cls,entry', RECIPES, ids=[o[1] for o in RECIPES])
def test_clipped_recipe_step_matches_clip_grad_norm_then_torch_optim(mods, flat_cls, torch_cls, entry):
    train, _ = mods
    c = 5.0
    pa, pb, bucket, _ = _pair(mods, SHAPES)
    opt_a = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=0.01, max_grad_norm=c)
    opt_b = getattr(torch.optim, torch_cls)(pb, lr=1e-2, weight_decay=0.01)
    cpu = torch.Generator().manual_seed(0)
    norms = []
    for it in range(7):
        flat = (torch.randn(bucket.numel, generator=cpu) * (1e-2, 1.0, 1e2)[it % 3]).to(DEV)
        _feed(bucket, pb, flat)
        norms.append(float(flat.double().norm()))
        opt_a.step()
        torch.nn.utils.clip_grad_norm_(pb, c)
        opt_b.step()
        assert torch.equal(bucket.flat, flat), 'the step must leave the bucket\'s gradient unscaled'
        _all_close(opt_a, opt_b, pa, pb, 'clipped %s step %d' % (torch_cls, it))
    assert any(v > c for v in norms) and any(v + 1e-6 < c for v in norms), 'both branches of the clip must occur'
    assert int(opt_a.step_count) == 7 and opt_a.guard_state()['skipped'] == 0


@pytest.mark.parametrize('flat_cls,torch_cls,entry', RECIPES, ids=[o[1] for o in RECIPES])
def test_nan_gradient_skips_the_whole_recipe_step_and_the_average_follows_the_taken_ones(mods, flat_cls, torch_cls, entry):
    train, _ = mods
    d = 0.9
    pa, pb, bucket, g = _pair(mods, [(4099, )], seed=3)
    opt = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=0.01, max_grad_norm=1e3, skip_nonfinite=True, ema_decay=d)
    d32 = torch.tensor(d, dtype=torch.float32, device=DEV)       # the decay crosses the C ABI as a float
    ref, taken = None, 0
    for it in range(6):
        flat = torch.randn(bucket.numel, device=DEV, generator=g)
        if it == 3:
            flat[4098] = float('nan')                            # (in the scalar tail)
        bucket.flat.copy_(flat)
        held = [t.clone() for t in [bucket.flat_params, opt.step_count, opt.ema] + [getattr(opt, k) for k in opt.MOMENTS]]
        opt.step()
        now = [bucket.flat_params, opt.step_count, opt.ema] + [getattr(opt, k) for k in opt.MOMENTS]
        if it == 3:
            # parameters (AdamW's decoupled decay included), step count, average and moments: bit for bit
            assert all(torch.equal(a, b) for a, b in zip(now, held)) and opt.guard_state()['skipped'] == 1
            continue
        taken += 1
        assert not torch.equal(now[0], held[0])
        p = bucket.flat_params
        if ref is None:
            assert torch.equal(opt.ema, p), 'the first update copies'
        else:
            _close(opt.ema, held[2].lerp(p, 1.0 - d32), '%s step %d average against Tensor.lerp' % (torch_cls, it))
            _close(opt.ema, d32 * ref + (1.0 - d32) * p, '%s step %d average against d e + (1 - d) p' % (torch_cls, it))
        ref = opt.ema.clone()
    assert taken == 5 and opt.guard_state()['steps'] == 5 and int(opt.step_count) == 5
    assert bool(torch.isfinite(bucket.flat_params).all()) and not torch.equal(opt.ema, bucket.flat_params)


# ---- 4. the schedule inside a captured graph ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flat_cls,torch_cls', ALL, ids=[o[1] for o in ALL])
def test_warmup_and_cosine_run_inside_a_captured_graph(mods, flat_cls, torch_cls):
    """opt.step() alone in a hipGraph; 24 replays cross the warmup's end (5) and the cosine's end (17) without a host write"""
    import warnings
    train, _ = mods
    base = 1e-2
    pa, pb, bucket, g = _pair(mods, SHAPES, seed=1)
    opt_a = getattr(train, flat_cls)(bucket, lr=base, weight_decay=0.01, lr_warmup_steps=W, lr_warmup_start=START, cosine_steps=T,
                                     lr_min=LR_MIN)
    opt_b = getattr(torch.optim, torch_cls)(pb, lr=base, weight_decay=0.01)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sched = S.SequentialLR(opt_b, [S.LinearLR(opt_b, start_factor=START, end_factor=1.0, total_iters=W),
                                       S.CosineAnnealingLR(opt_b, T_max=T, eta_min=LR_MIN)], milestones=[W])
    assert float(opt_a.lr) == float(np.float32(base * START))
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
    opt_a.set_schedule(base, 0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_a.step()
    assert int(opt_a.sched_pos) == 0                             # (a capture runs nothing)
    rates = []
    for it in range(24):
        _feed(bucket, pb, _fresh(bucket, g, special=(it == 3)))
        graph.replay()
        want = np.float32(opt_a.scheduled_lr(base, it))          # the rate of THIS step: pos = it completed ones before it
        got = np.float32(float(opt_a.lr))
        rates.append(float(got))
        assert abs(float(got) - float(want)) <= float(np.spacing(want)), (it, got, want)
        if it <= W + T:                                          # torch's cosine swings back up past its end; this one holds
            assert abs(sched.get_last_lr()[0] - opt_a.scheduled_lr(base, it)) <= 1e-12 * base
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                opt_b.step()
                sched.step()
            for k, (a, b) in enumerate(zip(pa, pb)):
                _close(a, b, '%s replay %d tensor %d' % (torch_cls, it, k))
    assert int(opt_a.step_count) == 24 and int(opt_a.sched_pos) == 24
    assert rates[0] < rates[1] < rates[W - 1] < rates[W] == max(rates) and abs(rates[W] - base) <= 2e-9      # (a float32 ulp of 1e-2: 9.3e-10)
    assert all(r == float(np.float32(LR_MIN)) for r in rates[W + T:]) and rates[W + T - 1] > rates[W + T]
    assert opt_a.torch_state_dict()['param_groups'][0]['lr'] == LR_MIN


def test_warmup_with_steplr_counts_the_decay_from_the_warmups_end(mods):
    """the NF_LR_STEP kind of nf_lr_schedule (eager launches): W = 5, decay_steps = 3, against torch's SequentialLR"""
    import warnings
    train, _ = mods
    base = 1e-2
    pa, pb, bucket, g = _pair(mods, SHAPES, seed=2)
    opt_a = train.FlatAdamax(bucket, lr=base, lr_warmup_steps=W, lr_warmup_start=START, decay_steps=3, decay_ratio=0.5)
    opt_b = torch.optim.Adamax(pb, lr=base)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sched = S.SequentialLR(opt_b, [S.LinearLR(opt_b, start_factor=START, end_factor=1.0, total_iters=W),
                                       S.StepLR(opt_b, step_size=3, gamma=0.5)], milestones=[W])
        for it in range(15):
            _feed(bucket, pb, _fresh(bucket, g))
            want = np.float32(sched.get_last_lr()[0])
            opt_a.step()
            opt_b.step()
            sched.step()
            got = np.float32(float(opt_a.lr))
            assert abs(float(got) - float(want)) <= float(np.spacing(want)), (it, got, want)
            if it >= W:
                assert got == np.float32(base * 0.5 ** ((it - W) // 3))
    for k, (a, b) in enumerate(zip(pa, pb)):
        _close(a, b, 'warmup + StepLR, tensor %d' % k)


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
def test_adamax_warmup_cosine_clip_ema_captured_against_eager(pkg, mods, tmp_path):
    """twelve optimizer steps each: the captured trainer's eleven calls (the capturing call takes one extra eager step on its batch)
    against twelve eager calls on the same batches"""
    import warnings
    train, _ = mods
    torch.manual_seed(21)
    np.random.seed(21)
    net_g = pkg.MAF((2, ), '2d', NS(layers=2))
    net_e = copy.deepcopy(net_g)
    kw = dict(lr=1e-3, optimizer='adamax', lr_warmup_steps=4, cosine_steps=8, max_grad_norm=1.0, ema_decay=0.9)
    tg = train.FlowTrainer(net_g.to(DEV), graph=True, warmup=2, **kw)
    te = train.FlowTrainer(net_e.to(DEV), graph=False, **kw)
    net_e.draws = net_g.draws                                    # (a captured MAF draws its masks on the device: the same rule, D = 2)
    assert type(tg.optim).__name__ == type(te.optim).__name__ == 'FlatAdamax'
    gen = torch.Generator(device=DEV).manual_seed(4)
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='hipGraph capture failed')      # a fall-back to eager launches is a failure here
        for s in range(11):
            y = torch.randn(64, 2, device=DEV, generator=gen) * 0.5
            if s == 2:
                te.train_on_batch(y)
            te.train_on_batch(y)
            tg.train_on_batch(y)
    assert tg._g_fb is not None, 'the step was not captured'
    assert int(tg.optim.sched_pos) == int(te.optim.sched_pos) == 12 and int(tg.optim.step_count) == int(te.optim.step_count) == 12
    assert tg.current_lr() == te.current_lr() == tg.optim.scheduled_lr(1e-3, 12) == 0.0      # W + T completed: the floor, lr_min = 0
    last = np.float32(tg.optim.scheduled_lr(1e-3, 11))             # the rate the twelfth step ran at
    assert float(tg.optim.lr) == float(te.optim.lr) and abs(float(tg.optim.lr) - float(last)) <= float(np.spacing(last))
    assert bool(torch.isfinite(tg.bucket.flat_params).all())
    _close(tg.bucket.flat_params, te.bucket.flat_params, 'captured against eager, parameters')
    _close(tg.optim.ema, te.optim.ema, 'captured against eager, average')
    assert tg.guard_state()['steps'] == 12 and tg.guard_state()['skipped'] == 0
    f = str(tmp_path / 'adamax.pth')
    tg.save_ckpt(11, f)
    ckpt = torch.load(f)
    ref = torch.optim.Adamax(pkg.MAF((2, ), '2d', NS(layers=2)).parameters(), lr=1.0)
    ref.load_state_dict(ckpt['optim'])
    group = ref.param_groups[0]
    assert group['lr'] == 0.0 and group['initial_lr'] == 1e-3
    assert set(next(iter(ref.state.values()))) == {'step', 'exp_avg', 'exp_inf'}
    assert pkg._native.persistent_timeouts() == 0


# ---- 6. with no new argument the launches are the ones they were ----------------------------------------------------------------------------
def test_launch_names_without_and_with_the_new_arguments(pkg, mods, monkeypatch):
    train, _ = mods
    N = pkg._native
    names = []
    real = N.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(N, 'call', spy)

    def launches(cls, **kw):
        pa, pb, bucket, g = _pair(mods, SHAPES)
        opt = getattr(train, cls)(bucket, lr=1e-3, **kw)
        bucket.flat.copy_(_fresh(bucket, g))
        del names[:]
        opt.step()
        opt.step()
        return list(names)

    guard = dict(max_grad_norm=1.0, ema_decay=0.9)
    # the parent commit's launches, name for name
    assert launches('FlatAdam') == ['nf_adam_step'] * 2
    assert launches('FlatRMSprop') == ['nf_rmsprop_step'] * 2
    assert launches('FlatAdam', decay_steps=2) == ['nf_lr_step_decay', 'nf_adam_step'] * 2
    assert launches('FlatRMSprop', decay_steps=2) == ['nf_lr_step_decay', 'nf_rmsprop_step'] * 2
    assert launches('FlatAdam', **guard) == ['nf_grad_guard', 'nf_adam_step_guarded'] * 2
    assert launches('FlatRMSprop', decay_steps=2, **guard) == ['nf_lr_step_decay', 'nf_grad_guard', 'nf_rmsprop_step_guarded'] * 2
    # the new ones: one schedule launch in the same place, one step launch
    assert launches('FlatAdamax') == ['nf_adamax_step'] * 2
    assert launches('FlatAdamW', lr_warmup_steps=3) == ['nf_lr_schedule', 'nf_adamw_step'] * 2
    assert launches('FlatAdam', cosine_steps=5) == ['nf_lr_schedule', 'nf_adam_step'] * 2
    assert launches('FlatAdamax', lr_warmup_steps=3, decay_steps=2, **guard) == ['nf_lr_schedule', 'nf_grad_guard', 'nf_adamax_step_guarded'] * 2
