"""The run scope of the chain launches (fused_conv.ChainRuns) on its own: fake descriptors, a recording launcher, no GPU."""
import importlib
from types import SimpleNamespace as NS

import pytest


@pytest.fixture()
def runs(pkg, monkeypatch):
    fc = importlib.import_module(pkg.__name__ + '.fused_conv')
    r = fc.ChainRuns()
    log = []
    r.launcher = lambda name, descs, args: log.append((name, list(descs), tuple(args)))
    monkeypatch.setattr(fc, 'RUNS', r)
    monkeypatch.setattr(fc, 'CHAIN_RUNS_ON', True)
    return fc, r, log


KEY = (16, 24, 48, 8, 8, 1, 1e-5, 0.1, True)        # forward: the entry point's arguments + the weight form
BKEY = (16, 24, 48, 8, 8, 1, True)


def _forward(fc, r, n, key=KEY):
    ctxs = [NS() for _ in range(n)]
    with fc.chain_run():
        for i, c in enumerate(ctxs):
            r.launch_fwd(c, 'f%d' % i, key, None, True)
    return ctxs


def test_forward_scope_launches_once_in_order(runs):
    fc, r, log = runs
    ctxs = _forward(fc, r, 4)
    assert log == [('nf_convnet_chain_fwd', ['f0', 'f1', 'f2', 'f3'], KEY[:-1])]
    rec = ctxs[0].chain_run[0]
    assert rec.n == 4 and [c.chain_run[1] for c in ctxs] == [0, 1, 2, 3] and all(c.chain_run[0] is rec for c in ctxs)


def test_nothing_is_collected_outside_a_scope(runs):
    fc, r, log = runs
    c = NS()
    r.launch_fwd(c, 'f', KEY, None, True)
    assert log == [('nf_convnet_chain_fwd', ['f'], KEY[:-1])] and not hasattr(c, 'chain_run')


def test_a_run_is_cut_at_the_maximum_length(runs, pkg):
    fc, r, log = runs
    nmax = pkg._native.header_constant('NF_CONVNET_RUN_MAX')
    _forward(fc, r, nmax + 2)
    assert [len(e[1]) for e in log] == [nmax, 2]


def test_mismatched_shape_and_unchainable_launches(runs):
    fc, r, log = runs
    other = (16, 96, 192, 4, 4, 1, 1e-5, 0.1, True)
    a, b, c, d = NS(), NS(), NS(), NS()
    with fc.chain_run():
        r.launch_fwd(a, 'a', KEY, None, True)
        r.launch_fwd(b, 'b', other, None, True)        # another shape: what was collected leaves first
        r.launch_fwd(c, 'c', other, None, False)       # not chainable (no head, or a halo shape): launched singly, in order
        r.launch_fwd(d, 'd', other, None, True)
    assert [(e[1], e[2]) for e in log] == [(['a'], KEY[:-1]), (['b'], other[:-1]), (['c'], other[:-1]), (['d'], other[:-1])]
    assert not hasattr(c, 'chain_run') and a.chain_run[0].n == 1


def test_backward_collects_in_reverse_and_launches_at_the_first_member(runs):
    fc, r, log = runs
    ctxs = _forward(fc, r, 3)
    del log[:]
    r.launch_bwd(ctxs[2], 'b2', BKEY, None, True, False)       # the run's last step: its g_y comes from outside
    r.launch_bwd(ctxs[1], 'b1', BKEY, None, True, True)
    assert log == []
    r.launch_bwd(ctxs[0], 'b0', BKEY, None, True, True)
    assert log == [('nf_convnet_chain_bwd', ['b2', 'b1', 'b0'], BKEY[:-1])]
    assert not r.bwd and not r.fwd


def test_foreign_launch_flushes(runs, pkg):
    fc, r, log = runs
    ctxs = _forward(fc, r, 3)
    del log[:]
    r.launch_bwd(ctxs[2], 'b2', BKEY, None, True, False)
    r.launch_bwd(ctxs[1], 'b1', BKEY, None, True, True)
    r.before_call('nf_half_scatter')
    assert log == [('nf_convnet_chain_bwd', ['b2', 'b1'], BKEY[:-1])]
    r.launch_bwd(ctxs[0], 'b0', BKEY, None, True, True)        # the rest of the run: a collection of its own
    assert log[1:] == [('nf_convnet_chain_bwd', ['b0'], BKEY[:-1])]
    # ... and a forward scope is flushed the same way
    with fc.chain_run():
        r.launch_fwd(NS(), 'f0', KEY, None, True)
        r.before_call('nf_conv_weight_pack')
        assert log[2:] == [('nf_convnet_chain_fwd', ['f0'], KEY[:-1])]
    # the hook of the package-wide run scope is what _native.call consults
    mod = importlib.import_module(pkg.__name__ + '.fused_conv')
    assert pkg._native._before_call is not None and pkg._native._before_call.__func__ is mod.ChainRuns.before_call


def test_incomplete_run_is_launched_at_the_end_of_pass_flush(runs):
    fc, r, log = runs
    ctxs = _forward(fc, r, 3)
    del log[:]
    r.launch_bwd(ctxs[2], 'b2', BKEY, None, True, False)
    r.launch_bwd(ctxs[1], 'b1', BKEY, None, True, True)
    fc.ConvDefer().flush()
    assert log == [('nf_convnet_chain_bwd', ['b2', 'b1'], BKEY[:-1])]


def test_backward_outside_a_trainer_step_and_broken_chains_launch_singly(runs):
    fc, r, log = runs
    ctxs = _forward(fc, r, 3)
    del log[:]
    r.launch_bwd(ctxs[2], 'b2', BKEY, None, False, False)      # not inside a trainer step: as before
    assert log == [('nf_convnet_chain_bwd', ['b2'], BKEY[:-1])]
    del log[:]
    r.launch_bwd(ctxs[2], 'b2', BKEY, None, True, False)
    r.launch_bwd(ctxs[1], 'b1', BKEY, None, True, False)       # its g_y did not come from the member before it: that one leaves first
    assert log == [('nf_convnet_chain_bwd', ['b2'], BKEY[:-1])]
    r.launch_bwd(NS(), 'x', BKEY, None, True, True)            # a step that belongs to no run
    assert log[1:] == [('nf_convnet_chain_bwd', ['b1'], BKEY[:-1]), ('nf_convnet_chain_bwd', ['x'], BKEY[:-1])]


def test_switch_off(runs, monkeypatch):
    fc, r, log = runs
    monkeypatch.setattr(fc, 'CHAIN_RUNS_ON', False)
    ctxs = _forward(fc, r, 3)
    assert [e[1] for e in log] == [['f0'], ['f1'], ['f2']] and not any(hasattr(c, 'chain_run') for c in ctxs)
