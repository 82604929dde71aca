"""What the rational-quadratic spline coupling costs beside the mixture-of-logistics coupling, and what a captured SplineFlow step costs
beside a Glow step of the same depth, on one GPU (csrc/rqspline.hip: nf_rqs_coupling_fwd / _bwd; csrc/mixlog.hip is the yardstick).

    python tools/spline_bench.py [--rounds 5] [--layers 32] [--out profiles/r18_spline.txt]

One process, so that every form shares the GPU and its state:
    kernel  two features (D = 2), K = 8, B in {4096, 65536, 1048576}: the spline's forward, inverse and backward and the mixture coupling's
            (nf_mixlog_coupling_fwd / _inv / _bwd, K = 8) on inputs of the same distribution -- microseconds per call between two events
            over 20 calls, alternated, median (min .. max) of --rounds, and the bytes each must move as a share of 8 TB/s
            (spline: 23 parameters, mixture: 26 parameters per row; the inverse of each runs on its own forward's output)
    step    the captured training step of SplineFlow (layers = --layers, B = 4096, DeviceSampler('moons')) beside Glow at the same depth and
            batch: --rounds alternated loops of 30 steps each, wall-clock microseconds per step, median (min .. max) over the loops
No figure is a pass bar.  A measurement needs the GPU: without one the tool fails."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
K = 8
BOUND = 3.0
# algorithmic bytes per row of two features: z and y (8 each), ld read and written (8), the parameter row; backward: g_y, z, g_z (8 each),
# g_ld (4), the parameter row read and its gradient row written
BYTES = {'rqs': {'fwd': 24 + 4 * 23, 'inv': 24 + 4 * 23, 'bwd': 28 + 8 * 23},
         'mixlog': {'fwd': 24 + 4 * 26, 'inv': 24 + 4 * 26, 'bwd': 28 + 8 * 26}}


def _stats(v):
    return statistics.median(v), min(v), max(v)


def _f(v):
    return '%10.2f (%.2f .. %.2f)' % tuple(v)


def kernel_case(torch, pkg, B, rounds, dev):
    N = pkg._native
    g = torch.Generator(device=dev).manual_seed(0)
    z = 2.0 * torch.randn(B, 2, device=dev, generator=g)
    g_y, g_ld = torch.randn(B, 2, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
    ld = torch.zeros(B, device=dev)
    P = {'rqs': 0.5 * torch.randn(B, 3 * K - 1, device=dev, generator=g), 'mixlog': 0.5 * torch.randn(B, 2 + 3 * K, device=dev, generator=g)}
    y = {k: torch.empty_like(z) for k in P}
    x = {k: torch.empty_like(z) for k in P}
    g_z = torch.empty_like(z)
    g_p = {k: torch.empty_like(v) for k, v in P.items()}
    a, c = torch.full((1, ), 0.01, device=dev), torch.full((1, ), 0.01, device=dev)
    g_ac = torch.zeros(2, device=dev)
    scratch, flag = torch.empty(3 * B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    s = N.stream
    forms = {
        ('rqs', 'fwd'): lambda: N.call('nf_rqs_coupling_fwd', z.data_ptr(), P['rqs'].data_ptr(), y['rqs'].data_ptr(), ld.data_ptr(), K, BOUND, 0, 0, 0,
                                       B, 2, 1, 1, s()),
        ('rqs', 'inv'): lambda: N.call('nf_rqs_coupling_fwd', y['rqs'].data_ptr(), P['rqs'].data_ptr(), x['rqs'].data_ptr(), ld.data_ptr(), K, BOUND, 0,
                                       0, 1, B, 2, 1, 1, s()),
        ('rqs', 'bwd'): lambda: N.call('nf_rqs_coupling_bwd', g_y.data_ptr(), g_ld.data_ptr(), z.data_ptr(), P['rqs'].data_ptr(), g_z.data_ptr(),
                                       g_p['rqs'].data_ptr(), K, BOUND, 0, 0, B, 2, 1, 1, s()),
        ('mixlog', 'fwd'): lambda: N.call('nf_mixlog_coupling_fwd', z.data_ptr(), P['mixlog'].data_ptr(), a.data_ptr(), c.data_ptr(),
                                          y['mixlog'].data_ptr(), ld.data_ptr(), K, 1e-5, 0, 0, B, 2, 1, 1, s()),
        ('mixlog', 'inv'): lambda: N.call('nf_mixlog_coupling_inv', y['mixlog'].data_ptr(), P['mixlog'].data_ptr(), a.data_ptr(), c.data_ptr(),
                                          x['mixlog'].data_ptr(), ld.data_ptr(), scratch.data_ptr(), flag.data_ptr(), K, 0, 0, B, 2, 1, 1, s()),
        ('mixlog', 'bwd'): lambda: N.call('nf_mixlog_coupling_bwd', g_y.data_ptr(), g_ld.data_ptr(), z.data_ptr(), P['mixlog'].data_ptr(), a.data_ptr(),
                                          c.data_ptr(), g_z.data_ptr(), g_p['mixlog'].data_ptr(), g_ac.data_ptr(), g_ac.data_ptr() + 4, K, 1e-5, 0, 0,
                                          B, 2, 1, 1, s()),
    }
    got = {k: [] for k in forms}
    for fn in forms.values():                                # (forward before inverse: the inverses run on their forward's output)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):                                  # alternated
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            got[name].append(e0.elapsed_time(e1) * 1e3 / 20)
    rt = float((x['rqs'] - z).abs().max())
    return {'B': B, 'us': {'%s_%s' % k: _stats(v) for k, v in got.items()}, 'rqs_round_trip': rt}


def step_case(torch, pkg, train, nfdata, layers, rounds, dev):
    import numpy as np
    B = 4096
    trainers = {}
    for name, cls in (('SplineFlow', pkg.SplineFlow), ('Glow', pkg.Glow)):
        torch.manual_seed(0)
        np.random.seed(0)
        net = cls((2, ), '2d', NS(layers=layers)).to(dev)
        tr = train.FlowTrainer(net, graph=True, warmup=2, sampler=nfdata.DeviceSampler('moons', B, (2, ), device=dev))
        for _ in range(6):
            tr.train_on_batch()
        trainers[name] = tr
    torch.cuda.synchronize()
    got = {k: [] for k in trainers}
    for _ in range(rounds):                                  # alternated
        for name, tr in trainers.items():
            t0 = time.perf_counter()
            for _ in range(30):
                tr.train_on_batch()
            torch.cuda.synchronize()
            got[name].append((time.perf_counter() - t0) * 1e6 / 30)
    out = {'B': B, 'layers': layers}
    for name, tr in trainers.items():
        out['captured_' + name] = tr._g_fb is not None
        out['numel_' + name] = tr.bucket.numel
        out['step_%s_us' % name] = _stats(got[name])
        out['loss_' + name] = float(tr.train_on_batch()[1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layers', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'r18_spline.txt'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('spline_bench measures on the GPU and there is none: not measured')
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    train = importlib.import_module('normalizing-flows-pytorch_amd.train')
    nfdata = importlib.import_module('normalizing-flows-pytorch_amd.data')
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('rational-quadratic spline coupling beside the mixture-of-logistics coupling, and SplineFlow beside Glow, %s' % torch.cuda.get_device_name(0))
    say('the launches alone, two features, K = %d: microseconds per call between two events over 20 calls, median of %d alternated rounds '
        '(min .. max), and the algorithmic bytes as a share of 8 TB/s' % (K, a.rounds))
    cases = []
    for B in (4096, 65536, 1048576):
        k = kernel_case(torch, pkg, B, a.rounds, dev)
        cases.append(k)
        say('  B = %d (spline round trip %.2e)' % (B, k['rqs_round_trip']))
        for fam in ('rqs', 'mixlog'):
            for d in ('fwd', 'inv', 'bwd'):
                us = k['us']['%s_%s' % (fam, d)]
                say('    %-7s %s   %s   %5.1f %% of 8 TB/s' % (fam, d, _f(us), 100.0 * BYTES[fam][d] * B / (us[0] * 1e-6) / HBM_PEAK))
        u = k['us']
        say('    inverse / forward: spline %.2f, mixture %.2f' % (u['rqs_inv'][0] / u['rqs_fwd'][0], u['mixlog_inv'][0] / u['mixlog_fwd'][0]))
    s = step_case(torch, pkg, train, nfdata, a.layers, a.rounds, dev)
    say('captured training step on moons, layers = %d, B = %d: microseconds per step, median of %d alternated loops of 30 (min .. max)'
        % (s['layers'], s['B'], a.rounds))
    for name in ('SplineFlow', 'Glow'):
        say('  %-11s %s   captured: %s   %d parameters   loss %.4f' % (name, _f(s['step_%s_us' % name]), s['captured_' + name], s['numel_' + name],
                                                                     s['loss_' + name]))
    say('  SplineFlow / Glow: %.2f' % (s['step_SplineFlow_us'][0] / s['step_Glow_us'][0]))
    say('  persistent-kernel timeouts: %d' % pkg._native.persistent_timeouts())
    say(json.dumps([cases, s]))
    if a.out:
        path = os.path.join(ROOT, a.out)
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        with open(path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
