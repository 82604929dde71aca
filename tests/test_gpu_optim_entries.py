"""
All eight optimizer step entry points of csrc/optim.hip on the MI355X -- nf_{adam,rmsprop,adamax,adamw}_step and their _guarded forms,
which are one kernel body (k_optim_step) behind one launcher -- through the C ABI: tails and misaligned ends, the grid-stride wrap of
the float4 body, plain against guarded bit for bit, and the argument checks.

Yardstick: one torch.optim step from the same state, at the project's bar for the fused optimizers, 2e-6 + 2e-6 |x| per entry
(tests/_optim.py), on the parameter and on every state buffer.  The betas cross the C ABI as floats.  Adamax and AdamW recover the
decimal the caller wrote and form 1 - beta from it as torch does (csrc/nf_optim_recipes.h), so torch is handed the decimals 0.9 / 0.999.
Adam forms (1.f - beta) in float from the float it was handed (its arithmetic is left as it is), so torch.optim.Adam is
handed the same two numbers, float32(0.9) and float32(0.999): 1 - float32(0.999) is 1.3e-5 (relative) from 1 - 0.999, which on
exp_avg_sq under the gradient entry 3e4 (SPECIAL) would be 6.5 times the bar and says nothing about the loop under test.  RMSprop's
1 - float32(0.99) is 9.3e-7 from 1 - 0.99 and stays under the bar with the decimal (tests/test_gpu_optim.py).
The average: a copy of the new parameter when ema_count == 1 (torch.equal), else d ema + (1 - d) p formed in float64 from the float32
decay, at the same bar.
"""
import numpy as np
import pytest
import torch

from tests._optim import SPECIAL, _close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BADARG = 10001                                                   # NF_E_BADARG
NF_BLOCK, NF_MAX_GRID = 256, 4096                                # csrc/nf_common.h's values
WRAP_N = 4 * NF_MAX_GRID * NF_BLOCK + 4 * NF_BLOCK + 3           # 4 195 331: one full pass of the largest float4 grid, one more block, a tail
LR, WD, DECAY = 1e-2, 0.01, 0.9


def F32(x):
    return float(np.float32(x))


# recipe -> (torch.optim class, its state names in the entry point's order, hyper-parameters as the entry point takes them, torch's)
RECIPES = {
    'adam': ('Adam', ('exp_avg', 'exp_avg_sq'), (0.9, 0.999, 1e-8), dict(betas=(F32(0.9), F32(0.999)), eps=1e-8)),
    'rmsprop': ('RMSprop', ('square_avg', ), (0.99, 1e-8), dict(alpha=0.99, eps=1e-8)),
    'adamax': ('Adamax', ('exp_avg', 'exp_inf'), (0.9, 0.999, 1e-8), dict(betas=(0.9, 0.999), eps=1e-8)),
    'adamw': ('AdamW', ('exp_avg', 'exp_avg_sq'), (0.9, 0.999, 1e-8), dict(betas=(0.9, 0.999), eps=1e-8)),
}
ENTRIES = [(r, guarded) for r in RECIPES for guarded in (False, True)]
ENTRY_IDS = ['nf_%s_step%s' % (r, '_guarded' if guarded else '') for r, guarded in ENTRIES]


@pytest.fixture(scope='module')
def N(pkg):
    pkg._native.load()
    return pkg._native


class Bufs:
    """parameter, gradient, the recipe's state buffers and an average as views [off, off + n) of buffers with guard elements on both
    sides (off = 4: on 16 bytes, off = 1: 4 bytes off), and the device words a step reads"""

    def __init__(self, recipe, n, aligned, seed):
        self.recipe, self.n, self.off = recipe, n, (4 if aligned else 1)
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.names = ['param', 'grad'] + list(RECIPES[recipe][1]) + ['ema']
        self.whole = [torch.randn(n + 8, device=DEV, generator=gen) for _ in self.names]
        self.whole[len(self.names) - 2].abs_()                   # exp_avg_sq / exp_inf / square_avg are not negative
        self.views = [w[self.off:self.off + n] for w in self.whole]
        assert all((v.data_ptr() % 16 == 0) == aligned for v in self.views)
        self.p, self.g, self.ema = self.views[0], self.views[1], self.views[-1]
        self.states = self.views[2:-1]
        self.g[:min(n, len(SPECIAL))] = torch.tensor(SPECIAL[:n], device=DEV)
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.lr = torch.full((1, ), LR, device=DEV)
        self.ctl = torch.zeros(8, dtype=torch.int32, device=DEV)
        self.partials = torch.zeros(1024, dtype=torch.float64, device=DEV)       # NF_GUARD_MAX_PARTIALS

    def snapshot(self):
        return [w.clone() for w in self.whole]

    def assert_outside_untouched(self, before, ema_written):
        for name, w, w0 in zip(self.names, self.whole, before):
            if name == 'grad' or (name == 'ema' and not ema_written):
                assert torch.equal(w, w0), '%s was written' % name
            else:
                assert torch.equal(w[:self.off], w0[:self.off]) and torch.equal(w[self.off + self.n:], w0[self.off + self.n:]), \
                    '%s: wrote outside [0, n)' % name

    def args(self, guarded, n=None, ema=False, grad_scale=1.0):
        """(entry point, [(argument name, value)]) in the order nfhip.h declares"""
        r = self.recipe
        a = [('param', self.p.data_ptr()), ('grad', self.g.data_ptr())] + [(k, s.data_ptr()) for k, s in zip(RECIPES[r][1], self.states)]
        if not (guarded and r == 'rmsprop'):
            a.append(('step', self.step.data_ptr()))
        a.append(('lr', self.lr.data_ptr()))
        a += [('hyper%d' % i, h) for i, h in enumerate(RECIPES[r][2])] + [('weight_decay', WD)]
        if guarded:
            a += [('ctl', self.ctl.data_ptr()), ('ema', self.ema.data_ptr() if ema else None), ('ema_decay', DECAY)]
        else:
            a.append(('grad_scale', grad_scale))
        a += [('n', self.n if n is None else n), ('stream', None)]
        return 'nf_%s_step%s' % (r, '_guarded' if guarded else ''), a

    def run(self, N, guarded, ema=False):
        """one step: the plain entry point with grad_scale = 1, or nf_grad_guard(max_norm = 0, skip_nonfinite = 0) and the guarded one"""
        if guarded:
            N.call('nf_grad_guard', self.g.data_ptr(), self.n, 0.0, 0, self.partials.data_ptr(), self.ctl.data_ptr(), self.step.data_ptr(),
                   N.stream())
        entry, a = self.args(guarded, ema=ema)
        N.call(entry, *[N.stream() if k == 'stream' else v for k, v in a])

    def torch_step(self):
        """what one torch.optim step makes of the current parameter, gradient and state: (parameter, [state buffers])"""
        cls, names, _, kw = RECIPES[self.recipe]
        q = torch.nn.Parameter(self.p.clone())
        opt = getattr(torch.optim, cls)([q], lr=LR, weight_decay=WD, **kw)
        opt.state[q]['step'] = torch.tensor(float(int(self.step)))
        for k, s in zip(names, self.states):
            opt.state[q][k] = s.clone()
        q.grad = self.g.clone()
        opt.step()
        return q.detach(), [opt.state[q][k] for k in names]


def _step_and_compare(N, b, guarded, ema, what):
    """one step against torch.optim, guard elements and gradient bit-identical, the step count one higher; with an average, its rule"""
    before, count = b.snapshot(), int(b.step)
    held = b.ema.clone()
    want_p, want_s = b.torch_step()
    b.run(N, guarded, ema=ema)
    _close(b.p, want_p, what + ' param')
    for k, s, w in zip(RECIPES[b.recipe][1], b.states, want_s):
        _close(s, w, what + ' ' + k)
    assert int(b.step) == count + 1
    b.assert_outside_untouched(before, ema_written=ema)
    if ema:
        if int(b.ctl[4]) == 1:
            assert torch.equal(b.ema, b.p), what + ': the first update copies'
        else:
            d = F32(DECAY)
            _close(b.ema, d * held.double() + (1.0 - d) * b.p.double(), what + ' average')
            assert not torch.equal(b.ema, b.p)


def _entry_case(N, recipe, guarded, n, aligned):
    what = 'nf_%s_step%s n %d' % (recipe, '_guarded' if guarded else '', n)
    _step_and_compare(N, Bufs(recipe, n, aligned, seed=n), guarded, False, what)
    if guarded:
        b = Bufs(recipe, n, aligned, seed=n + 1)
        _step_and_compare(N, b, True, True, what + ' with the average, first step')
        assert int(b.ctl[4]) == 1
        _step_and_compare(N, b, True, True, what + ' with the average, second step')
        assert int(b.ctl[4]) == 2


# ---- 1. tails and misaligned ends, every entry point ------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 4099])
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'offset4B'])
@pytest.mark.parametrize('recipe,guarded', ENTRIES, ids=ENTRY_IDS)
def test_entry_tails_and_misaligned_ends(N, recipe, guarded, n, aligned):
    """the float4 body with its scalar tail where the buffers sit on 16 bytes, the scalar form where they start 4 bytes off; a guarded form
    without an average, then with one: the step that copies and the step that blends"""
    _entry_case(N, recipe, guarded, n, aligned)


# ---- 2. the grid-stride wrap of the float4 body -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('recipe,guarded', [('adam', False), ('rmsprop', False), ('adam', True)],
                         ids=['nf_adam_step', 'nf_rmsprop_step', 'nf_adam_step_guarded'])
def test_float4_body_wraps_the_grid(N, recipe, guarded):
    """n / 4 float4s are more than NF_MAX_GRID blocks of NF_BLOCK threads: every thread of the first block takes a second float4, and three
    elements are left for the scalar tail.  A two-state recipe, the one-state recipe and the widest mode (guarded, with the average)."""
    assert WRAP_N // 4 > NF_MAX_GRID * NF_BLOCK and WRAP_N % 4 == 3
    _entry_case(N, recipe, guarded, WRAP_N, True)


# ---- 3. plain and guarded are the same arithmetic -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'offset4B'])
@pytest.mark.parametrize('recipe', list(RECIPES))
def test_plain_and_guarded_give_the_same_bits(N, recipe, aligned):
    """with max_norm <= 0 the control block's clip_scale is exactly 1: nf_X_step(grad_scale = 1) and nf_grad_guard + nf_X_step_guarded
    (ema = NULL) are the same kernel body on the same numbers"""
    n = 4099
    plain, guarded = Bufs(recipe, n, aligned, seed=5), Bufs(recipe, n, aligned, seed=5)
    gen = torch.Generator(device=DEV).manual_seed(6)
    for it in range(3):
        fresh = torch.randn(n, device=DEV, generator=gen)
        for b in (plain, guarded):
            b.g.copy_(fresh)
        assert all(torch.equal(a, b) for a, b in zip(plain.whole, guarded.whole))
        plain.run(N, False)
        guarded.run(N, True)
        assert guarded.ctl[:2].view(torch.float32)[1].item() == 1.0 and int(guarded.ctl[2]) == 0
        for name, a, b in zip(plain.names, plain.whole, guarded.whole):
            assert torch.equal(a, b), '%s step %d: %s differs' % (recipe, it, name)
        assert int(plain.step) == int(guarded.step) == it + 1
    assert not torch.equal(plain.p, Bufs(recipe, n, aligned, seed=5).p)


# ---- 4. the argument checks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('recipe,guarded', ENTRIES, ids=ENTRY_IDS)
def test_entry_argument_checks(N, recipe, guarded):
    """n < 0 and a required pointer that is NULL are refused, n = 0 is accepted, all three before any launch: nothing is touched"""
    lib = N.load()
    b = Bufs(recipe, 4, True, seed=9)
    before, ctl0 = b.snapshot(), b.ctl.clone()
    entry, a = b.args(guarded, ema=True)
    fn = getattr(lib, entry)

    def rc(**change):
        return fn(*[change.get(k, N.stream() if k == 'stream' else v) for k, v in a])

    assert rc(n=-1) == BADARG
    required = ['param', 'grad'] + list(RECIPES[recipe][1]) + ['lr'] + ([] if guarded and recipe == 'rmsprop' else ['step']) + \
        (['ctl'] if guarded else [])
    assert set(required) <= set(k for k, _ in a)
    for k in required:
        assert rc(**{k: None}) == BADARG, k
    assert rc(n=0) == 0
    if guarded:
        assert rc(n=0, ema=None) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(w, w0) for w, w0 in zip(b.whole, before)) and int(b.step) == 0 and torch.equal(b.ctl, ctl0)
