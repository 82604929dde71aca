"""Image Glow with the chain launches of a level's flow steps leaving as ONE launch per direction (fused_conv.CHAIN_RUNS_ON) against
one launch per step: a (3, 32, 32) Glow with three steps per level, batch 16, ordered mode -- the run kernels equal the single
launches bit for bit (tests/test_gpu_convnet_run.py), so do the models."""
import copy
import importlib
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _mods(pkg):
    return importlib.import_module(pkg.__name__ + '.fused_conv'), importlib.import_module(pkg.__name__ + '.train'), pkg._native


@pytest.fixture()
def ordered(pkg):
    Nn = pkg._native
    was = Nn.deterministic()
    Nn.deterministic(True)
    yield Nn
    Nn.deterministic(was)


def _glow(pkg, seed):
    torch.manual_seed(seed)
    return pkg.Glow((3, 32, 32), 'image', NS(layers=3, mixtures=None)).to(DEV)


def _batch(seed=6):
    return torch.rand(16, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _record(monkeypatch, Nn, fc):
    """(entry point, n, (I0, H, W, split mode, channels of z)) of every chain launch that goes through _native.call; any other native
    launch as (name, 0, None)"""
    log, real = [], Nn.call
    descs = {'nf_convnet_chain_fwd': fc.ConvNetDesc, 'nf_convnet_chain_bwd': fc.ConvNetBwdDesc}

    def call(name, *args):
        base = name[:-4] if name.endswith('_run') else name
        if base in descs:
            run = name.endswith('_run')
            d = descs[base].from_address(args[0])
            a = args[2:] if run else args[1:]
            log.append((name, args[1] if run else 1, (a[1], a[3], a[4], d.cp_mode, d.cp_C)))
        else:
            log.append((name, 0, None))
        return real(name, *args)
    monkeypatch.setattr(Nn, 'call', call)
    return log


def _eager_pass(net, y):
    net.train()
    for p in net.parameters():
        p.grad = None
    z, ld = net(y)
    (0.5 * (z ** 2).sum() - ld.sum()).backward()
    torch.cuda.synchronize()
    return z.detach().clone(), ld.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


def _assert_passes_equal(a, b):
    assert torch.equal(a[0], b[0]), 'z'
    assert torch.equal(a[1], b[1]), 'log-det'
    assert a[2].keys() == b[2].keys() and len(a[2]) > 100
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_eager_training_pass(pkg, monkeypatch, ordered):
    """(a) one eager training pass after the ActNorm initialisation: z, log-det and every parameter gradient, bitwise; the forward of the
    8 x 8 and 4 x 4 levels leaves as runs (outside a trainer step the backward launches per step)"""
    fc, _, Nn = _mods(pkg)
    net = _glow(pkg, 2)
    y = _batch()
    with torch.no_grad():
        net(y)                                          # data-dependent ActNorm initialisation
    log = _record(monkeypatch, Nn, fc)
    outs = []
    for on in (True, False):
        monkeypatch.setattr(fc, 'CHAIN_RUNS_ON', on)
        del log[:]
        outs.append(_eager_pass(copy.deepcopy(net), y))
        names = [e[0] for e in log]
        assert ('nf_convnet_chain_fwd_run' in names) == on and 'nf_convnet_chain_bwd_run' not in names
    _assert_passes_equal(*outs)
    assert Nn.persistent_timeouts() == 0


def test_first_pass_with_uninitialised_actnorm(pkg, monkeypatch, ordered):
    """(c) the very first pass: every ActNorm awaits its data-dependent initialisation, the run route declines, the per-step route
    initialises and serves -- same results as with the switch off, no run launch"""
    fc, _, Nn = _mods(pkg)
    net = _glow(pkg, 3)
    y = _batch(7)
    log = _record(monkeypatch, Nn, fc)
    outs = []
    for on in (True, False):
        monkeypatch.setattr(fc, 'CHAIN_RUNS_ON', on)
        outs.append(_eager_pass(copy.deepcopy(net), y))
    assert not [e for e in log if e[0].endswith('_run')]
    _assert_passes_equal(*outs)
    assert Nn.persistent_timeouts() == 0


@pytest.mark.parametrize('graph', [False, True])
def test_trainer_steps(pkg, monkeypatch, ordered, graph):
    """(b) four FlowTrainer steps, eager and as a replayed hipGraph: the same losses and the same parameters"""
    fc, nftrain, Nn = _mods(pkg)
    y = _batch()
    outs = []
    for on in (True, False):
        monkeypatch.setattr(fc, 'CHAIN_RUNS_ON', on)
        net = _glow(pkg, 4)
        tr = nftrain.FlowTrainer(net, graph=graph, warmup=1)
        losses = [float(tr.train_on_batch(y)[1]) for _ in range(4)]
        torch.cuda.synchronize()
        outs.append((losses, torch.cat([p.detach().reshape(-1) for p in net.parameters()]).clone()))
    assert outs[0][0] == outs[1][0], (outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert all(l == l and abs(l) < 1e6 for l in outs[0][0])
    assert Nn.persistent_timeouts() == 0


def test_launch_counts_inside_a_trainer_step(pkg, monkeypatch, ordered):
    """(d) the chain launches of one trainer step: at the 8 x 8 and 4 x 4 levels ONE run launch per direction per run of steps (and no
    single-step launch), at 16 x 16 -- a sample over two workgroups -- the per-step launches, unchanged"""
    fc, nftrain, Nn = _mods(pkg)
    y = _batch()
    log = _record(monkeypatch, Nn, fc)
    seen = {}
    for on in (False, True):
        monkeypatch.setattr(fc, 'CHAIN_RUNS_ON', on)
        net = _glow(pkg, 5)
        tr = nftrain.FlowTrainer(net, graph=False, warmup=1)
        tr.train_on_batch(y)                            # (ActNorm initialisation)
        del log[:]
        tr.train_on_batch(y)
        torch.cuda.synchronize()
        seen[on] = list(log)

    def groups(entries, name):
        """lengths of the maximal runs of consecutive single launches ``name`` of one shape and split below 16 x 16 (any other native
        launch in between ends a run)"""
        out, last = [], None
        for e in entries:
            if e[0] == name and e[2][1] < 16:
                if e[2] == last:
                    out[-1] += 1
                else:
                    out.append(1)
            last = e[2] if e[0] == name else None
        return out

    for d in ('fwd', 'bwd'):
        single, run = 'nf_convnet_chain_' + d, 'nf_convnet_chain_%s_run' % d
        want = groups(seen[False], single)
        assert want and all(n >= fc.CHAIN_RUN_MIN for n in want), want
        assert [e[1] for e in seen[True] if e[0] == run] == want
        assert not [e for e in seen[True] if e[0] == single and e[2][1] < 16]
        assert not [e for e in seen[False] if e[0] == run]
        big = lambda es: [e for e in es if e[0] == single and e[2][1] >= 16]
        assert big(seen[True]) == big(seen[False]) and len(big(seen[True])) >= 3
    assert Nn.persistent_timeouts() == 0
