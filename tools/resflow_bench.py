"""Residual Flow timings on one GPU (L = 32 blocks, D = 2, the shipped config's spnorm_coeff 0.9): the whole-stack kernels of
csrc/resflow.hip against the per-block path (NF_RESFLOW_STACK=0: the parent tree's code, one ActNorm launch and the kernels of
csrc/resmlp.hip per block) in the same process on the same GPU.

    python tools/resflow_bench.py [--layers 32] [--batches 1024,65536] [--iters 30] [--repeats 5] [--out profiles/r10_resflow.txt]

Per batch size: a training step (stack: FlowTrainer(graph=True) replay with in-kernel draws, and the eager step with host draws;
per-block: the eager step, the only form it has), density evaluation net(y) under no_grad with the `unbias` and the `exact`
estimator, sampling net.backward(z) at 1 024 rows and at the one-workgroup inverse's row cap.  Every figure is the median of
--repeats timed loops of --iters calls between two events, after warm-up calls; the spread (min .. max of the repeats) is printed with
it.  Also the C-ABI calls of one training forward + backward and one evaluation at two depths (they must not depend on the depth).
Kernel launches per step: ``rocprofv3 --kernel-trace -- python tools/resflow_bench.py --trace K --trace-evals K2 --stack 1|0`` at two values of K
(of K2); the dispatch counts of the two traces differ by the launches of the extra training steps (evaluations)."""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pkg = importlib.import_module('normalizing-flows-pytorch_amd')
train = importlib.import_module('normalizing-flows-pytorch_amd.train')
NF = pkg.functional
DEV = torch.device('cuda:0')


def timed(fn, iters, repeats, warmup=3):
    """(median, min, max) microseconds per call over `repeats` loops of `iters` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def make_net(L, D, logdet='unbias', seed=0):
    torch.manual_seed(seed)
    np.random.seed(seed)
    return pkg.ResFlow((D, ), '2d', NS(layers=L, spnorm_coeff=0.9, logdet=logdet)).to(DEV)


def calls_per_pass(L, D, B):
    """names of the C-ABI calls of one training forward + backward and of one evaluation (ActNorms initialised)"""
    N = pkg._native
    net = make_net(L, D)
    x = torch.randn(B, D, device=DEV)
    net.train()
    net(x)                                              # the first batch initialises the ActNorms on the per-layer path
    names = []
    orig = N.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    N.call = call
    try:
        z, ld = net(x.clone().requires_grad_(True))
        (z.sum() + ld.sum()).backward()
        n_train = list(names)
        del names[:]
        net.eval()
        with torch.no_grad():
            net(x)
        n_eval = list(names)
    finally:
        N.call = orig
    return n_train, n_eval


def measure(L, D, B, iters, repeats, stack, rows_cap):
    NF.RESFLOW_STACK = stack
    out = {}
    y = 0.8 * torch.randn(B, D, device=DEV)
    net = make_net(L, D)
    tr = train.FlowTrainer(net, graph=False)
    for _ in range(2):
        tr.train_on_batch(y)
    out['step_eager_us'] = timed(lambda: tr.train_on_batch(y), iters, repeats)
    if stack:
        net = make_net(L, D)
        tr = train.FlowTrainer(net, graph=True, warmup=2)
        for _ in range(4):
            tr.train_on_batch(y)
        out['captured'] = tr._g_fb is not None
        out['step_graph_us'] = timed(lambda: tr.train_on_batch(y), iters, repeats)
    for est in ('unbias', 'exact'):
        net = make_net(L, D, est)
        net.train()
        net(y)                                          # ActNorm initialisation
        net.eval()
        with torch.no_grad():
            out['eval_%s_us' % est] = timed(lambda: net(y), iters, repeats)
    net = make_net(L, D)
    net.train()
    net(y)
    net.eval()
    for rows in sorted({min(B, 1024), min(B, rows_cap)}):
        z = torch.randn(rows, D, device=DEV)
        with torch.no_grad():
            out['sample_%d_us' % rows] = timed(lambda: net.backward(z), max(2, iters // 5), repeats, warmup=1)
            blocks = [m for m in net.net.layers if isinstance(m, pkg.InvertibleResLinear)]
            out['inverse_iters_%d' % rows] = [int(b.last_inverse_iters) for b in blocks]
    return out


def trace(L, D, B, stack, steps, evals):
    """for a kernel-trace run: set-up and warm-up, then `steps` eager training steps and `evals` `unbias` evaluations of one path.  Two
    runs that differ only in `steps` (or only in `evals`) differ by the launches of those calls: (dispatches(K2) - dispatches(K1)) / (K2 - K1)
    is the launches of one step (one evaluation), optimizer and loss included."""
    NF.RESFLOW_STACK = bool(stack)
    y = 0.8 * torch.randn(B, D, device=DEV)
    net = make_net(L, D)
    tr = train.FlowTrainer(net, graph=False)
    ev = make_net(L, D)
    ev.train()
    ev(y)
    ev.eval()
    for _ in range(2):
        tr.train_on_batch(y)
        with torch.no_grad():
            ev(y)
    for _ in range(steps):
        tr.train_on_batch(y)
    with torch.no_grad():
        for _ in range(evals):
            ev(y)
    torch.cuda.synchronize()
    print('traced %d steps and %d evaluations, L = %d, %s path' % (steps, evals, L, 'stack' if stack else 'per-block'), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trace', type=int, default=None, metavar='STEPS', help='kernel-trace mode: only STEPS training steps and --trace-evals evaluations')
    ap.add_argument('--trace-evals', type=int, default=None)
    ap.add_argument('--stack', type=int, default=1)
    ap.add_argument('--layers', type=int, default=32)
    ap.add_argument('--dim', type=int, default=2)
    ap.add_argument('--batches', default='1024,65536')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    pkg.build()
    if a.trace is not None:
        trace(a.layers, a.dim, int(a.batches.split(',')[0]), a.stack, a.trace, a.trace if a.trace_evals is None else a.trace_evals)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cap = pkg._native.header_constant('NF_RESFLOW_INV_WG_MAX_ROWS')
    res = {'layers': a.layers, 'dim': a.dim, 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'repeats': a.repeats}
    say('Residual Flow, L = %d blocks, D = %d, %s; microseconds per call, median of %d loops of %d calls (min .. max)'
        % (a.layers, a.dim, res['device'], a.repeats, a.iters))
    for stack in (True, False):
        NF.RESFLOW_STACK = stack
        for L in (8, a.layers):
            t, e = calls_per_pass(L, a.dim, 1024)
            res['calls_%s_L%d' % ('stack' if stack else 'block', L)] = {'train': len(t), 'eval': len(e)}
            say('C-ABI calls, %s path, L = %2d: training forward + backward %4d, evaluation %4d%s'
                % ('stack' if stack else 'per-block', L, len(t), len(e), ('  ' + ' '.join(t)) if stack else ''))

    def f(v):
        return '%10.1f (%.1f .. %.1f)' % v
    for B in [int(b) for b in a.batches.split(',')]:
        s = measure(a.layers, a.dim, B, a.iters, a.repeats, True, cap)
        p = measure(a.layers, a.dim, B, a.iters, a.repeats, False, cap)
        res['B%d' % B] = {'stack': s, 'per_block': p}
        say('B = %d' % B)
        say('  training step, hipGraph replay, device draws   stack %s   captured: %s' % (f(s['step_graph_us']), s['captured']))
        say('  training step, eager, host draws               stack %s   per-block %s   x%.2f'
            % (f(s['step_eager_us']), f(p['step_eager_us']), p['step_eager_us'][0] / s['step_eager_us'][0]))
        for est in ('unbias', 'exact'):
            k = 'eval_%s_us' % est
            say('  density evaluation, %-6s                     stack %s   per-block %s   x%.2f' % (est, f(s[k]), f(p[k]), p[k][0] / s[k][0]))
        for k in sorted(x for x in s if x.startswith('sample_')):
            say('  sampling, %5s rows                            stack %s   per-block %s   x%.2f   iterations per block %s'
                % (k.split('_')[1], f(s[k]), f(p[k]), p[k][0] / s[k][0], s['inverse_iters_' + k.split('_')[1]]))
    say(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
