"""
The guarded optimizer step on the MI355X (csrc/optim_guard.hip and the guarded modes of csrc/optim.hip's step kernel): the gradient
norm and its control block, the skip of a non-finite step,
clipping against torch.nn.utils.clip_grad_norm_ + torch.optim, the averaged weights updated in the fused pass, nf_swap_f32, and all of
it inside a captured FlowTrainer step (main.py:78-92 has none of the three; the yardsticks are torch's own).

Bars.  Norm and clip scale: relative 2^-22 -- the squares are summed in float64 (relative error about n 2^-53), the one float32 rounding
is the final conversion (2^-24); a factor of 4 is left.  Parameters, moments and averages: the project's optimizer bar,
2e-6 + 2e-6 |x| per entry (tests/test_gpu_optim.py).  Log-densities: 1e-5 (1 + |x|).
"""
import copy
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests._optim import SPECIAL, _close, _feed, _pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(32, 32), (32, ), (1, ), (2, 32), (1, 2, 1, 1)]        # tests/test_gpu_optim.py: 1 123 elements
OPTS = [('FlatAdam', 'Adam'), ('FlatRMSprop', 'RMSprop')]
PARTIALS = 1024                                                  # NF_GUARD_MAX_PARTIALS
ONE_PASS = PARTIALS * 256 * 4                                    # elements one pass of the float4 partials grid covers
NS_LIST = [1, 3, 255, 256, 257, 4099, ONE_PASS + 5]
REL = 2.0 ** -22


@pytest.fixture(scope='module')
def mods(pkg):
    pkg._native.load()
    return importlib.import_module(pkg.__name__ + '.train'), importlib.import_module(pkg.__name__ + '.dist')


def _ctl(t):
    """the control block as the header lays it out: float grad_norm, clip_scale; int skip, skipped, ema_count"""
    w = t.cpu()
    f = w[:2].view(torch.float32)
    return {'grad_norm': float(f[0]), 'clip_scale': float(f[1]), 'skip': int(w[2]), 'skipped': int(w[3]), 'ema_count': int(w[4]),
            'bits': tuple(int(x) for x in w)}


def _guard(N, g, n, max_norm, skip_nonfinite, partials, ctl, step):
    N.call('nf_grad_guard', g.data_ptr(), n, max_norm, skip_nonfinite, partials.data_ptr(), ctl.data_ptr(), step.data_ptr(), N.stream())


def _guard_buffers():
    return (torch.zeros(PARTIALS, dtype=torch.float64, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV),
            torch.zeros(1, dtype=torch.int32, device=DEV))


# ---- the norm -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', NS_LIST)
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'offset4B'])
def test_grad_norm_in_float64_same_bits_every_call(pkg, n, aligned):
    N = pkg._native
    off = 4 if aligned else 1
    gen = torch.Generator(device=DEV).manual_seed(n)
    buf = torch.randn(n + 8, device=DEV, generator=gen)
    g = buf[off:off + n]
    assert (g.data_ptr() % 16 == 0) == aligned
    g[:min(n, len(SPECIAL))] = torch.tensor(SPECIAL[:n], device=DEV)
    before = buf.clone()
    partials, ctl, step = _guard_buffers()
    _guard(N, g, n, 5.0, 1, partials, ctl, step)
    first = _ctl(ctl)
    _guard(N, g, n, 5.0, 1, partials, ctl, step)
    second = _ctl(ctl)
    want = float(g.double().norm())
    rel = abs(first['grad_norm'] - want) / want if want > 0.0 else abs(first['grad_norm'])      # (n = 1 holds SPECIAL[0] = 0 alone)
    print('n %d: norm %.9g, float64 %.9g, relative error %.3e (bar %.3e)' % (n, first['grad_norm'], want, rel, REL))
    assert rel <= REL
    want_scale = min(1.0, 5.0 / (want + 1e-6))
    assert abs(first['clip_scale'] - want_scale) <= REL * want_scale
    assert first['bits'][:3] == second['bits'][:3], 'two calls on the same gradient must return the same bits'
    assert first['skip'] == 0 and (first['skipped'], first['ema_count']) == (0, 1) and (second['skipped'], second['ema_count']) == (0, 2)
    assert int(step) == 2                                        # the finalise launch ticks the optimizer's counter on a step that is taken
    assert torch.equal(buf, before)                              # the gradient is read only
    assert float(partials[min(PARTIALS, (n + 255) // 256):].abs().sum()) == 0.0     # no partial written past the grid


@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'offset4B'])
def test_grad_norm_squares_that_overflow_float32(pkg, aligned):
    """two entries of 1e20: each square is 1e40, beyond float32; the norm, 1.41e20, is not"""
    N = pkg._native
    n, off = 4099, (4 if aligned else 1)
    gen = torch.Generator(device=DEV).manual_seed(7)
    buf = torch.randn(n + 8, device=DEV, generator=gen)
    g = buf[off:off + n]
    g[17] = 1e20
    g[n - 1] = -1e20                                             # (in the scalar tail)
    partials, ctl, step = _guard_buffers()
    _guard(N, g, n, 5.0, 1, partials, ctl, step)
    got = _ctl(ctl)
    want = float(g.double().norm())
    assert not bool(torch.isfinite((g * g).sum())) and np.isfinite(want)
    assert got['skip'] == 0 and abs(got['grad_norm'] - want) <= REL * want
    want_scale = 5.0 / (want + 1e-6)
    assert abs(got['clip_scale'] - want_scale) <= REL * want_scale


# ---- the non-finite step ------------------------------------------------------------------------------------------------------------------
def _snapshot(opt):
    return [t.clone() for t in [opt.bucket.flat_params, opt.step_count, opt.ema] + [getattr(opt, k) for k in opt.MOMENTS]]


@pytest.mark.parametrize('where', [0, 2048, 4098], ids=['first', 'middle', 'scalar_tail'])
@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')], ids=['nan', 'inf', 'neg_inf'])
def test_nonfinite_gradient_skips_the_whole_step(mods, value, where):
    train, _ = mods
    n = 4099
    for flat_cls, _torch_cls in OPTS:
        pa, pb, bucket, g = _pair(mods, [(n, )], seed=3)
        opt = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=0.01, max_grad_norm=5.0, skip_nonfinite=True, ema_decay=0.9)
        for _ in range(2):                                       # moments and average hold something
            bucket.flat.copy_(torch.randn(n, device=DEV, generator=g))
            opt.step()
        assert opt.guard_state()['steps'] == 2 and int(opt.step_count) == 2
        before = _snapshot(opt)
        bad = torch.randn(n, device=DEV, generator=g)
        bad[where] = value
        bucket.flat.copy_(bad)
        opt.step()
        st = opt.guard_state()
        assert _ctl(opt.guard_ctl)['skip'] == 1 and st['skipped'] == 1 and st['steps'] == 2, (flat_cls, st)
        for a, b in zip(_snapshot(opt), before):
            assert torch.equal(a, b), flat_cls                   # parameters, step count, average, moments: bit for bit
        bucket.flat.copy_(torch.randn(n, device=DEV, generator=g))
        opt.step()                                               # and the next finite one is taken
        st = opt.guard_state()
        assert _ctl(opt.guard_ctl)['skip'] == 0 and st['skipped'] == 1 and st['steps'] == 3 and int(opt.step_count) == 3
        assert not torch.equal(bucket.flat_params, before[0]) and bool(torch.isfinite(bucket.flat_params).all())


@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')], ids=['nan', 'inf', 'neg_inf'])
def test_guard_switched_off_never_sets_the_flag(pkg, value):
    N = pkg._native
    n = 4099
    g = torch.randn(n, device=DEV)
    g[n - 1] = value
    partials, ctl, step = _guard_buffers()
    _guard(N, g, n, 0.0, 0, partials, ctl, step)
    got = _ctl(ctl)
    assert got['skip'] == 0 and got['skipped'] == 0 and got['clip_scale'] == 1.0 and int(step) == 1
    assert not np.isfinite(got['grad_norm'])


# ---- clipping against clip_grad_norm_ + torch.optim ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('flat_cls,torch_cls', OPTS, ids=[o[1] for o in OPTS])
def test_clipped_step_matches_clip_grad_norm_then_torch_optim(mods, flat_cls, torch_cls, wd):
    train, _ = mods
    c = 5.0
    pa, pb, bucket, _ = _pair(mods, SHAPES)
    opt_a = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=wd, max_grad_norm=c)
    opt_b = getattr(torch.optim, torch_cls)(pb, lr=1e-2, weight_decay=wd)
    cpu = torch.Generator().manual_seed(0)
    norms = []
    for it in range(7):
        flat = (torch.randn(bucket.numel, generator=cpu) * (1e-2, 1.0, 1e2)[it % 3]).to(DEV)
        _feed(bucket, pb, flat)
        norm64 = float(flat.double().norm())
        norms.append(norm64)
        opt_a.step()
        torch.nn.utils.clip_grad_norm_(pb, c)
        opt_b.step()
        st = opt_a.guard_state()
        want_scale = min(1.0, c / (norm64 + 1e-6))
        assert abs(st['grad_norm'] - norm64) <= REL * norm64 and abs(st['clip_scale'] - want_scale) <= REL * want_scale, (it, st)
        assert torch.equal(bucket.flat, flat), 'the step must leave the bucket\'s gradient unscaled'
        for k, (a, b) in enumerate(zip(pa, pb)):
            _close(a, b, '%s wd %g step %d tensor %d' % (torch_cls, wd, it, k))
    print('float64 norms', ['%.4g' % v for v in norms])
    assert any(v > c for v in norms) and any(v + 1e-6 < c for v in norms), 'both branches of the clip must occur'
    assert int(opt_a.step_count) == 7 and opt_a.guard_state()['skipped'] == 0
    assert pa[0].data_ptr() == bucket.flat_params.data_ptr()


# ---- the average in the fused pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [0.9, 0.999])
@pytest.mark.parametrize('flat_cls,torch_cls', OPTS, ids=[o[1] for o in OPTS])
def test_ema_in_the_fused_pass(mods, flat_cls, torch_cls, d):
    train, _ = mods
    pa, pb, bucket, g = _pair(mods, SHAPES, seed=5)
    opt = getattr(train, flat_cls)(bucket, lr=1e-2, weight_decay=0.01, skip_nonfinite=True, ema_decay=d)
    d32 = torch.tensor(d, dtype=torch.float32, device=DEV)       # the decay crosses the C ABI as a float
    ref = None
    for it in range(7):
        flat = torch.randn(bucket.numel, device=DEV, generator=g)
        if it == 3:
            flat[100] = float('nan')                             # a skipped step in the middle
        bucket.flat.copy_(flat)
        held = opt.ema.clone()
        opt.step()
        p = bucket.flat_params
        if it == 3:
            assert torch.equal(opt.ema, held) and opt.guard_state()['skipped'] == 1
            continue
        if ref is None:
            ref = p.clone()
            assert torch.equal(opt.ema, p), 'the first update copies'
        else:
            ref = d32 * ref + (1.0 - d32) * p                    # the float32 restatement
            _close(opt.ema, ref, '%s d %g step %d average' % (torch_cls, d, it))
            ref = opt.ema.clone()                                # (per-step comparison: the next step starts from the kernel's own value)
    assert not torch.equal(opt.ema, bucket.flat_params) and opt.guard_state()['steps'] == 6


# ---- nf_swap_f32 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', NS_LIST)
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'offset4B'])
def test_swap_twice_is_the_identity(pkg, n, aligned):
    N = pkg._native
    off = 4 if aligned else 1
    gen = torch.Generator(device=DEV).manual_seed(n)
    bufs = [torch.randn(n + 8, device=DEV, generator=gen) for _ in range(2)]
    a, b = (t[off:off + n] for t in bufs)
    before = [t.clone() for t in bufs]
    N.call('nf_swap_f32', a.data_ptr(), b.data_ptr(), n, N.stream())
    assert torch.equal(a, before[1][off:off + n]) and torch.equal(b, before[0][off:off + n])
    for t, t0 in zip(bufs, before):
        assert torch.equal(t[:off], t0[:off]) and torch.equal(t[off + n:], t0[off + n:]), 'wrote outside [0, n)'
    N.call('nf_swap_f32', a.data_ptr(), b.data_ptr(), n, N.stream())
    assert torch.equal(bufs[0], before[0]) and torch.equal(bufs[1], before[1])


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------------
def _glow2d(pkg, seed):
    torch.manual_seed(seed)
    return pkg.Glow((2, ), '2d', NS(layers=2))


def _flat_of(tr):
    return tr.bucket.flat_params.clone()


def test_captured_step_skips_a_nan_batch_and_goes_on(pkg, mods):
    """the one test that sends a NaN through the flow's kernels.  Training mode throughout: the NaN forward has written into the running
    statistics, which the guard does not protect (the known limit)."""
    train, _ = mods
    net_g = _glow2d(pkg, 11)
    net_e = copy.deepcopy(net_g)
    kw = dict(lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99)
    tg = train.FlowTrainer(net_g.to(DEV), graph=True, warmup=2, **kw)
    te = train.FlowTrainer(net_e.to(DEV), graph=False, **kw)
    gen = torch.Generator(device=DEV).manual_seed(3)
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='hipGraph capture failed')      # a fall-back to eager launches is a failure here
        for s in range(9):
            y = torch.randn(256, 2, device=DEV, generator=gen) * 0.5
            if s == 2:                                           # the capturing call takes one extra eager step on its batch first
                te.train_on_batch(y)
            if s == 5:
                assert tg._g_fb is not None, 'the step was not captured'
                y[7, 0] = float('nan')                           # one sample
                held = (_flat_of(tg), tg.optim.ema.clone(), tg.optim.step_count.clone())
            te.train_on_batch(y)
            tg.train_on_batch(y)
            if s == 5:
                st = tg.guard_state()
                assert st['skipped'] == 1 and not np.isfinite(st['grad_norm']), st
                assert torch.equal(_flat_of(tg), held[0]) and torch.equal(tg.optim.ema, held[1]) and torch.equal(tg.optim.step_count, held[2])
                assert bool(torch.isfinite(held[0]).all()) and bool(torch.isfinite(held[1]).all())
            if s == 6:
                assert not torch.equal(_flat_of(tg), held[0]), 'the replay after the skipped one must train'
                assert np.isfinite(tg.guard_state()['grad_norm'])
    assert net_g.training
    sg, se = tg.guard_state(), te.guard_state()
    assert sg['skipped'] == se['skipped'] == 1 and sg['steps'] == se['steps'] == 9
    assert bool(torch.isfinite(tg.bucket.flat_params).all())
    _close(tg.bucket.flat_params, te.bucket.flat_params, 'captured against eager, parameters')
    _close(tg.optim.ema, te.optim.ema, 'captured against eager, average')
    assert pkg._native.persistent_timeouts() == 0


def test_averaged_weights_in_use_and_through_a_checkpoint(pkg, mods, tmp_path):
    train, _ = mods
    D = importlib.import_module(pkg.__name__ + '.data')
    rows = D.moons(1000, np.random.default_rng(1))
    net = _glow2d(pkg, 12).to(DEV)
    ds = D.DeviceDataset(rows, 96, seed=1, device=DEV)
    kw = dict(lr=1e-2, max_grad_norm=50.0, skip_nonfinite=True, ema_decay=0.9)
    tr = train.FlowTrainer(net, sampler=ds, **kw)
    for _ in range(6):
        tr.train_on_batch()
    ev = ds.sweep_view()
    y = torch.from_numpy(rows[:256]).to(DEV)
    iterate = _flat_of(tr)
    avg = {k: v.clone() for k, v in zip(tr._ema_names(), tr._ema_views())}
    assert not torch.equal(tr.optim.ema, iterate)
    # a deep copy of the net loaded with the averaged values (buffers: the live ones, as inside the context)
    twin = copy.deepcopy(net)
    with torch.no_grad():
        for k, p in twin.named_parameters():
            if k in avg:
                p.copy_(avg[k])
    t2 = train.FlowTrainer(twin)
    want_lp = t2.log_py(y)
    want_nll = t2.evaluate(ev)['nll']
    with tr.ema_weights():
        got_lp = tr.log_py(y)
        assert torch.equal(tr.bucket.flat_params, torch.cat([avg[k].reshape(-1) for k in tr._ema_names()]))
    got_nll = tr.evaluate(ev, ema=True)['nll']
    live_nll = tr.evaluate(ev)['nll']
    err = float(((got_lp - want_lp).abs() / (1.0 + want_lp.abs())).max())
    print('log_py inside ema_weights against the twin: %.3e of 1e-5; nll averaged %.6f twin %.6f live %.6f' % (err, got_nll, want_nll, live_nll))
    assert err <= 1e-5 and abs(got_nll - want_nll) <= 1e-5 * (1.0 + abs(want_nll))
    assert live_nll != got_nll
    assert torch.equal(_flat_of(tr), iterate), 'after the block the iterate is back, bit for bit'
    assert torch.equal(tr.optim.ema, torch.cat([avg[k].reshape(-1) for k in tr._ema_names()]))
    rep = tr.report(y, ema=True)
    assert np.isfinite(rep['py_map']).all() and torch.equal(_flat_of(tr), iterate)
    # save -> a fresh CAPTURED trainer loads: average and skip count arrive in the tensors its graph reads, and replays go on
    tr.optim.guard_ctl[3].fill_(2)                               # (a count to carry over; no NaN is sent through the flow here)
    f = str(tmp_path / 'guard.pth')
    tr.save_ckpt(6, f)
    ckpt = torch.load(f)
    assert set(ckpt) == {'net', 'optim', 'step', 'ema', 'skipped'} and ckpt['skipped'] == 2 and list(ckpt['ema']) == tr._ema_names()
    fresh = train.FlowTrainer(_glow2d(pkg, 13).to(DEV), graph=True, warmup=1, **kw)
    for s in range(3):
        fresh.train_on_batch(y)
    graph, ema_ptr = fresh._g_fb, fresh.optim.ema.data_ptr()
    assert graph is not None
    assert fresh.load_ckpt(f) == 6
    assert fresh.optim.ema.data_ptr() == ema_ptr and torch.equal(fresh.optim.ema, tr.optim.ema) and torch.equal(_flat_of(fresh), iterate)
    assert fresh.guard_state()['skipped'] == 2
    loaded_avg = fresh.optim.ema.clone()
    for s in range(2):
        fresh.train_on_batch(y)
    assert fresh._g_fb is graph and fresh.guard_state()['skipped'] == 2
    assert bool(torch.isfinite(_flat_of(fresh)).all()) and not torch.equal(_flat_of(fresh), iterate)
    assert not torch.equal(fresh.optim.ema, loaded_avg) and not torch.equal(fresh.optim.ema, fresh.bucket.flat_params)      # blended, not copied


def test_options_off_are_the_step_as_it_was(pkg, mods):
    """named-but-off and not named at all: the same launches, hence (in deterministic mode) the same bits; no control block, no average"""
    train, _ = mods
    N = pkg._native
    was = N.deterministic()
    try:
        N.deterministic(True)
        a = train.FlowTrainer(_glow2d(pkg, 14).to(DEV), lr=1e-3, max_grad_norm=None, skip_nonfinite=False, ema_decay=None)
        b = train.FlowTrainer(_glow2d(pkg, 14).to(DEV), lr=1e-3)
        gen = torch.Generator(device=DEV).manual_seed(5)
        for _ in range(5):
            y = torch.randn(256, 2, device=DEV, generator=gen) * 0.5
            a.train_on_batch(y)
            b.train_on_batch(y)
        assert torch.equal(a.bucket.flat_params, b.bucket.flat_params)
    finally:
        N.deterministic(was)
    for tr in (a, b):
        assert not tr.optim.guarded and tr.optim.guard_ctl is None and tr.optim.ema is None and tr.optim._partials is None
    with pytest.raises(ValueError, match='ema_decay'):
        a.ema_weights()
    with pytest.raises(ValueError, match='skip_nonfinite'):
        train.FlowTrainer(_glow2d(pkg, 15).to(DEV), graph=True, fused_adam=False, skip_nonfinite=True)
