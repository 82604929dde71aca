"""
Host-side checks of layers.Compose's dispatch (no GPU, no kernel runs): the matcher of every step shape finds the steps of its model
family and nothing one layer off, declines under hooks, with fusion off and under synchronised statistics, ``_collect`` gathers the
same run from either end, and the two route tuples keep their priority order.
"""
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch


class Cuda:
    """no GPU here: the shape / dtype / device of a GPU batch of 64 rows of 2 features (tests/test_resflow_host.py's stand-in)"""
    is_cuda, dtype, shape = True, torch.float32, torch.Size([64, 2])

    def dim(self):
        return 2

    def __getitem__(self, idx):
        return self                                         # (fused.flowpp_post_actnorm_usable asks the same of a column slice)


def _family(pkg, family):
    """(Compose of a 3-step vector model with initialised ActNorms, matcher, step width, first layer of the first step)"""
    L = importlib.import_module(pkg.__name__ + '.layers')
    torch.manual_seed(0)
    np.random.seed(0)
    cls = {'glow': 'Glow', 'realnvp': 'RealNVP', 'maf': 'MAF', 'flowpp': 'Flowpp'}[family]
    comp = getattr(pkg, cls)((2, ), '2d', NS(layers=3, mixtures=8)).train().net
    for m in comp.layers:
        if isinstance(m, pkg.ActNorm):
            m.initialized = True
    if family == 'glow':
        return comp, comp._glow_triple_at, 3, 0
    if family == 'realnvp':
        return comp, lambda i, z: comp._bn_pair_at(i, z, False, L._vector_coupling), 2, 0
    if family == 'maf':
        return comp, lambda i, z: comp._bn_pair_at(i, z, False, L._autoregressive), 2, 0
    return comp, comp._flowpp_pair_at, 2, 1                 # [ActNorm, coupling] x 3: the pairs are (coupling, NEXT ActNorm)


@pytest.mark.parametrize('family', ['glow', 'realnvp', 'maf', 'flowpp'])
def test_matchers_find_the_steps_and_decline_what_fusion_does_not_serve(pkg, family, monkeypatch):
    nfdist = importlib.import_module(pkg.__name__ + '.dist')
    comp, at, width, first = _family(pkg, family)
    layers, z = list(comp.layers), Cuda()
    n = len(layers)
    starts = [i for i in range(first, n, width) if i + width <= n]
    assert len(starts) == (2 if family == 'flowpp' else 3)
    for i in range(-1, n + 1):
        got = at(i, z)
        if i in starts:                                     # the members, in layer order, at a step boundary ...
            assert got is not None and len(got) == width and all(a is b for a, b in zip(got, layers[i:i + width])), i
        else:                                               # ... and nothing one layer off, in front of the stack or past its end
            assert got is None, i
    if family in ('realnvp', 'maf'):                        # the training-only form of the same matcher: same steps while training
        assert all(comp._bn_pair_at(i, z, True) is not None for i in starts)
        comp.eval()
        assert all(comp._bn_pair_at(i, z, True) is None and at(i, z) is not None for i in starts)
        comp.train()
        assert all(at(i, Cuda4()) is None and comp._bn_pair_at(i, Cuda4(), True) is not None for i in starts)
    i = starts[1]
    for m in layers[i:i + width]:
        for register in (m.register_forward_hook, m.register_forward_pre_hook):
            h = register(lambda *a: None)
            assert at(i, z) is None and at(starts[0], z) is not None
            h.remove()
            assert at(i, z) is not None
    comp.fuse = False
    assert at(i, z) is None
    del comp.fuse
    assert at(i, z) is not None
    monkeypatch.setattr(nfdist, 'sync_stats_active', lambda: True)
    assert at(i, z) is None
    monkeypatch.undo()
    assert at(i, z) is not None
    cpu = torch.zeros(64, 2)
    assert at(i, cpu) is None                               # CPU tensors: the layers' own path
    # the same run from the first layer forward as from the last layer backward
    last = starts[-1] + width - 1
    fwd, bwd = comp._collect(first, z, 1, width, at), comp._collect(last, z, -1, width, at)
    assert len(fwd) == len(starts) and len(bwd) == len(fwd)
    assert all(a is b for s, t in zip(fwd, bwd) for a, b in zip(s, t))
    assert all(a is b for s, j in zip(fwd, starts) for a, b in zip(s, layers[j:j + width]))
    assert comp._collect(starts[1], z, 1, width, at) == fwd[1:] and comp._collect(starts[1] - 1, z, -1, width, at) == fwd[:1]
    assert comp._collect(first + 1, z, 1, width, at) == [] and comp._collect(last - 1, z, -1, width, at) == []


class Cuda4(Cuda):
    """an image batch: the evaluation and inverse launches of the flow-BatchNorm steps serve vector data only"""
    shape = torch.Size([8, 2, 4, 4])

    def dim(self):
        return 4


def test_route_tuples_keep_their_priority_order(pkg):
    """earlier routes shadow later ones: the order is part of what a model computes with"""
    assert [r.__name__ for r in pkg.Compose._FORWARD] == [
        '_planar', '_resflow', '_realnvp_eval', '_maf_eval', '_bn_step', '_glow_step', '_glow_step_w', '_flowpp_pair', '_layer']
    assert [r.__name__ for r in pkg.Compose._INVERSE] == [
        '_planar_inverse', '_resflow_inverse', '_glow_inverse', '_realnvp_inverse', '_maf_inverse', '_layer_inverse']
    for r in pkg.Compose._FORWARD + pkg.Compose._INVERSE:
        assert getattr(pkg.Compose, r.__name__) is r
