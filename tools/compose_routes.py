"""which native entry points a model's passes call, in order: the record of the routes layers.Compose takes

    python tools/compose_routes.py            # every case: entry-point names with their int and float arguments, then a sha256 of it all
    python tools/compose_routes.py --write    # rewrite tests/golden/compose_routes.json (names only) after a route changed on purpose

Cases: the eight models of tests/_golden.MODEL_CASES on their golden batch, the vector ones at three steps as well, a PlanarFlow of three
layers, a MAF on 3-D data with device-drawn masks, and the vector Glow and RealNVP under every setting of fused.GLOW_FLOW on either side
of the batch size at which the per-step launches start (2 * NF_MLP_ROWS_PER_BLOCK rows).  Each case runs two training steps (the first
one initialises the ActNorms from its batch), a no_grad forward in eval() and in train(), and net.backward in both modes.  Seeds are
fixed.  tests/test_gpu_compose_routes.py records the same on the tree under test and compares the names."""
import ctypes
import hashlib
import importlib
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _golden as G  # noqa: E402

GOLDEN = os.path.join(G.GOLDEN_DIR, 'compose_routes.json')
PHASES = ('train step 1', 'train step 2', 'eval forward', 'train forward, no_grad', 'eval inverse', 'train inverse')
BELOW, ABOVE = 150, 300        # batches on either side of 2 * NF_MLP_ROWS_PER_BLOCK (fused._glow_steps_on)


def cases():
    """{case id: (model class, dims, datatype, layers, mixtures, batch (None: the golden one of ``golden``), golden, GLOW_FLOW, draws)}"""
    out = {}
    for name, (kind, cls, dims, datatype, layers, mix) in G.MODEL_CASES.items():
        out[name] = (cls, dims, datatype, layers, mix, None, name, None, None)
        if len(dims) == 1:
            out[name + ' x3'] = (cls, dims, datatype, 3, mix, None, name, None, None)
    out['planar x3'] = ('PlanarFlow', (2, ), '2d', 3, None, None, 'glow2d', None, None)
    out['maf3d device draws'] = ('MAF', (3, ), '2d', 2, None, 200, None, None, 'device')
    for name in ('glow2d', 'realnvp2d'):
        for flow in ('1', 'steps', '0'):
            for B in (BELOW, ABOVE):
                out['%s x3 GLOW_FLOW=%s B=%d' % (name, flow, B)] = (G.MODEL_CASES[name][1], (2, ), '2d', 3, None, B, None, flow, None)
    return out


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def record(pkg, case):
    """{phase: [(entry point, (its int and float arguments, pointers dropped))]} of one case"""
    Nn = pkg._native
    fused = importlib.import_module(pkg.__name__ + '.fused')
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    ws = importlib.import_module(pkg.__name__ + '.workspace')
    cls, dims, datatype, layers, mix, B, golden, flow, draws = cases()[case]
    assert BELOW <= 2 * Nn.header_constant('NF_MLP_ROWS_PER_BLOCK') < ABOVE
    scalars = {name: [i for i, t in enumerate(types) if t is not ctypes.c_void_p] for name, types in Nn.header_prototypes().items()}
    seen, real_call, was, arena = [], Nn.call, fused.GLOW_FLOW, ws.ARENA

    def call(name, *a):
        seen.append((name, tuple(a[i] for i in scalars[name])))
        return real_call(name, *a)

    _seed(0)
    net = getattr(pkg, cls)(dims, datatype, NS(layers=layers, mixtures=mix, logdet='exact', spnorm_coeff=0.9)).to('cuda')
    if draws is not None:
        net.draws = draws
    y = G.group('model_' + golden, '', 'cuda')['y'].clone() if B is None else (torch.randn(B, *dims) * 0.7).to('cuda')
    tr = nftrain.FlowTrainer(net, graph=False)
    out = {}
    Nn.call = call
    ws.ARENA = ws.ZeroArena()      # the step scratch of a fresh process: how much of it a step clears depends on the steps before it
    try:
        if flow is not None:
            fused.GLOW_FLOW = flow
        for n, phase in enumerate(PHASES):
            _seed(100 + n)
            del seen[:]
            if n < 2:
                net.train()
                tr.train_on_batch(y)
            else:
                net.train(phase.startswith('train'))
                with torch.no_grad():
                    if 'forward' in phase:
                        z, _ = net(y)
                    else:
                        net.backward(z.clone())
            torch.cuda.synchronize()
            out[phase] = list(seen)
    finally:
        Nn.call, fused.GLOW_FLOW, ws.ARENA = real_call, was, arena
    assert Nn.persistent_timeouts() == 0
    return out


def names(rec):
    return {phase: ' '.join(name for name, _ in calls) for phase, calls in rec.items()}


def main():
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    pkg._native.load()
    text, golden = [], {}
    for case in cases():
        rec = record(pkg, case)
        golden[case] = names(rec)
        for phase in PHASES:
            text.append('== %s / %s: %d calls' % (case, phase, len(rec[phase])))
            text += ['%s(%s)' % (name, ', '.join(repr(v) for v in args)) for name, args in rec[phase]]
    text = '\n'.join(text) + '\n'
    sys.stdout.write(text)
    print('sha256 %s' % hashlib.sha256(text.encode()).hexdigest())
    if '--write' in sys.argv[1:]:
        with open(GOLDEN, 'w') as f:
            json.dump(golden, f, indent=0, sort_keys=True)
            f.write('\n')
        print('wrote %s' % GOLDEN)


if __name__ == '__main__':
    main()
