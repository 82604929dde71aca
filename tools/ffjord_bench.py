"""FFJORD timings on one GPU, shipped config (dopri5, stepsize 0.1, 3 layers, Hutchinson trace), D = 2: the engine against the
reference's algorithm restated with framework ops on the same GPU (tests/_ffjord.py: the forward-mode field, the solvers' host loops, the
adjoint through torch.autograd.grad; one CPU torch.randn copied to the device per field evaluation, as cnf.py:29-30 does).

    python tools/ffjord_bench.py [--batches 1024,65536] [--iters 20] [--framework-iters 2]

Per batch size: a training step (forward + main.py's loss + backward + torch.optim.Adam, the reference's own loop), density evaluation
net(y) in eval mode under no_grad (S = 4 samples), sampling net.backward(z).  Also the kernel launches of one engine training step
(torch.profiler).  The engine draws its noise in the kernel (the default); --cpu-noise times noise_on_cpu=True as well."""
import argparse
import importlib
import json
import os
import sys
from types import SimpleNamespace as NS

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _ffjord as FJ  # noqa: E402

pkg = importlib.import_module('normalizing-flows-pytorch_amd')
DEV = torch.device('cuda:0')
CFG = dict(layers=3, stepsize=0.1, t0=0.0, t1=1.0, solver='dopri5', trace='hutchinson', backprop='adjoint')
TIMES = torch.linspace(0.0, 1.0, 11, dtype=torch.float32).double()
E = 70


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us


def make_net(D, cpu_noise=False, seed=0):
    torch.manual_seed(seed)
    return pkg.Ffjord((D, ), '2d', NS(noise_on_cpu=cpu_noise, **CFG)).to(DEV)


def engine_step(net, opt, y):
    z, ld = net(y)
    loss = FJ.nll(z, ld)
    opt.zero_grad()
    loss.backward()
    opt.step()


def kernels_per_step(D, B):
    from torch.profiler import ProfilerActivity, profile
    net = make_net(D)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    y = torch.randn(B, D, device=DEV)
    for _ in range(2):
        engine_step(net, opt, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        z, ld = net(y)
        loss = FJ.nll(z, ld)
        loss.backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    cnf = [n for n in names if 'k_cnf' in n]
    return len(names), len(cnf), sorted(set(cnf))


def engine(D, B, iters, cpu_noise=False):
    out = {}
    net = make_net(D, cpu_noise)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    y = torch.randn(B, D, device=DEV)
    out['step_us'] = timed(lambda: engine_step(net, opt, y), iters)
    net.eval()
    with torch.no_grad():
        out['eval_us'] = timed(lambda: net(y), iters)
        z = torch.randn(B, D, device=DEV)
        out['sample_us'] = timed(lambda: net.backward(z), iters)
    return out


def framework(D, B, iters):
    """the reference's algorithm with framework ops on the GPU; noise as the reference draws it (CPU randn, one copy per evaluation)"""
    out = {}
    net = make_net(D)
    layers = FJ.model_params({k: v for k, v in net.state_dict().items()}, CFG['layers'], requires_grad=True)
    for ls, b, p in layers:
        ls.data = ls.data.to(DEV)
        b.data = b.data.to(DEV)
        for q in p:
            q.data = q.data.to(DEV)
    flat = [t for ls, b, p in layers for t in [ls, b] + p]
    opt = torch.optim.Adam(flat, lr=1e-4)
    y = torch.randn(B, D, device=DEV)
    times = TIMES.to(DEV)

    class Draws:                                        # a lazily drawn "list" of the evaluation noise
        def __init__(self, S):
            self.S = S

        def __iter__(self):
            while True:
                yield torch.randn([B, self.S, D]).to(DEV)

    def step():
        n = [Draws(1) for _ in layers]
        z, ld = FJ.model_forward(layers, y, times, 'dopri5', 'hutchinson', n, n)
        loss = FJ.nll(z, ld)
        opt.zero_grad()
        loss.backward()
        opt.step()
    out['step_us'] = timed(step, iters, warmup=1)
    with torch.no_grad():
        n4 = [Draws(4) for _ in layers]
        out['eval_us'] = timed(lambda: FJ.model_forward(layers, y, times, 'dopri5', 'hutchinson', n4, None), iters, warmup=1)
        z = torch.randn(B, D, device=DEV)
        out['sample_us'] = timed(lambda: FJ.model_inverse(layers, z, times, 'dopri5', 'hutchinson', n4), iters, warmup=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, default=2)
    ap.add_argument('--batches', default='1024,65536')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--framework-iters', type=int, default=2)
    ap.add_argument('--cpu-noise', action='store_true')
    ap.add_argument('--no-framework', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {'config': CFG, 'dim': a.dim, 'device': torch.cuda.get_device_name(0)}
    n, n_cnf, names = kernels_per_step(a.dim, 1024)
    res['kernels_fwd_bwd'] = n
    res['cnf_kernels_fwd_bwd'] = n_cnf
    res['cnf_kernel_names'] = names
    print('kernels of one forward + loss + backward (3 x [ActNorm, CNF]): %d, of which CNF launches: %d' % (n, n_cnf), flush=True)
    for B in [int(b) for b in a.batches.split(',')]:
        e = engine(a.dim, B, a.iters)
        res['B%d' % B] = {'engine': e}
        line = 'B = %6d  step %10.1f us  eval %10.1f us  sample %10.1f us' % (B, e['step_us'], e['eval_us'], e['sample_us'])
        if a.cpu_noise:
            c = engine(a.dim, B, max(2, a.iters // 4), cpu_noise=True)
            res['B%d' % B]['engine_cpu_noise'] = c
            line += '   [noise_on_cpu: step %10.1f us  eval %10.1f us  sample %10.1f us]' % (c['step_us'], c['eval_us'], c['sample_us'])
        if not a.no_framework:
            f = framework(a.dim, B, a.framework_iters)
            res['B%d' % B]['framework'] = f
            line += '   framework: step %12.1f us (x%.1f)  eval %12.1f us (x%.1f)  sample %12.1f us (x%.1f)' % (
                f['step_us'], f['step_us'] / e['step_us'], f['eval_us'], f['eval_us'] / e['eval_us'], f['sample_us'],
                f['sample_us'] / e['sample_us'])
        print(line, flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
