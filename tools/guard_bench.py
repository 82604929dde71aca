"""What gradient clipping, the non-finite guard and the averaged weights cost inside the captured training step, on one GPU
(csrc/optim_guard.hip, FlowTrainer(max_grad_norm=, skip_nonfinite=, ema_decay=)).

    python tools/guard_bench.py [--rounds 5] [--glow-layers 32] [--maf-layers 10] [--out profiles/r16_guard.txt]

One process, so that every form shares the GPU and its state:
    step    the captured step of the C4 shape (Glow on (3, 32, 32), B = 64, batches gathered in-graph from a device-resident uint8 set)
            and of the C5 shape (MAF on `normals`, B = 16 384), each with the three options off -- the step as it is without this
            feature, the yardstick -- and with all three on: --rounds alternated loops of 30 steps each, wall-clock microseconds per
            step, median (min .. max) over the loops
    kernel  at the C4 model's bucket size: nf_grad_guard (partials + finalise), the guarded Adam step with the average, and the plain
            nf_adam_step for comparison; microseconds between two events over 50 calls, median (min .. max) of --rounds, and the bytes each
            must move as a share of 8 TB/s
A measurement needs the GPU: without one the tool fails."""
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
ON = dict(max_grad_norm=100.0, skip_nonfinite=True, ema_decay=0.999)


def _stats(v):
    return statistics.median(v), min(v), max(v)


def _f(v):
    return '%10.2f (%.2f .. %.2f)' % tuple(v)


def step_case(torch, pkg, train, nfdata, what, layers, rounds, dev):
    import numpy as np
    trainers = {}
    if what == 'c4':
        B = 64
        arr = np.random.default_rng(0).integers(0, 256, size=(50000, 32, 32, 3), dtype=np.uint8)
    else:
        B = 16384
        arr = nfdata.GENERATORS['normals'](nfdata.N_DATASET_SIZE, np.random.default_rng(0))
    for name, kw in (('off', {}), ('on', ON)):
        torch.manual_seed(0)
        np.random.seed(0)
        if what == 'c4':
            net = pkg.Glow((3, 32, 32), 'image', NS(layers=layers, mixtures=None)).to(dev)
        else:
            net = pkg.MAF((2, ), '2d', NS(layers=layers)).to(dev)
        ds = nfdata.DeviceDataset(arr, B, device=dev)
        tr = train.FlowTrainer(net, graph=True, warmup=2, sampler=ds, **kw)
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
    out = {'what': what, 'B': B, 'layers': layers, 'numel': trainers['on'].bucket.numel}
    for name, tr in trainers.items():
        out['captured_' + name] = tr._g_fb is not None
        out['step_%s_us' % name] = _stats(got[name])
        out['loss_' + name] = float(tr.train_on_batch()[1])
    out['guard_state'] = trainers['on'].guard_state()
    return out


def kernel_case(torch, pkg, n, rounds, dev):
    N = pkg._native
    g = torch.Generator(device=dev).manual_seed(0)
    p, gr, m, ema = (torch.randn(n, device=dev, generator=g) for _ in range(4))
    v = torch.rand(n, device=dev, generator=g)
    step, lr = torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1, ), 1e-4, device=dev)
    ctl = torch.zeros(8, dtype=torch.int32, device=dev)
    partials = torch.zeros(N.header_constant('NF_GUARD_MAX_PARTIALS'), dtype=torch.float64, device=dev)
    forms = {
        'nf_grad_guard (two launches)': (4 * n, lambda: N.call(
            'nf_grad_guard', gr.data_ptr(), n, 100.0, 1, partials.data_ptr(), ctl.data_ptr(), step.data_ptr(), N.stream())),
        'nf_adam_step_guarded with the average': (36 * n, lambda: N.call(
            'nf_adam_step_guarded', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), lr.data_ptr(), 0.9, 0.999, 1e-8,
            0.0, ctl.data_ptr(), ema.data_ptr(), 0.999, n, N.stream())),
        'nf_adam_step (the plain step, for comparison)': (28 * n, lambda: N.call(
            'nf_adam_step', p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), lr.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0,
            n, N.stream())),
    }
    forms['nf_grad_guard (two launches)'][1]()                # the guarded step needs a control block that says "take it"
    got = {k: [] for k in forms}
    for _, fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):                                  # alternated
        for name, (_, fn) in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(50):
                fn()
            b.record()
            torch.cuda.synchronize()
            got[name].append(a.elapsed_time(b) * 1e3 / 50)
    return {'n': n, 'forms': {k: {'bytes': forms[k][0], 'us': _stats(got[k])} for k in forms}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--glow-layers', type=int, default=32)
    ap.add_argument('--maf-layers', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'r16_guard.txt'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('guard_bench measures on the GPU and there is none: not measured')
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    train = importlib.import_module('normalizing-flows-pytorch_amd.train')
    nfdata = importlib.import_module('normalizing-flows-pytorch_amd.data')
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('clipping + non-finite guard + averaged weights inside the captured step, %s' % torch.cuda.get_device_name(0))
    say('options on: %s' % json.dumps(ON))
    results = []
    for what, layers in (('c4', a.glow_layers), ('c5', a.maf_layers)):
        s = step_case(torch, pkg, train, nfdata, what, layers, a.rounds, dev)
        results.append(s)
        off, on = s['step_off_us'], s['step_on_us']
        say('%s, layers = %d, B = %d, bucket of %d parameters: microseconds per captured step, median of %d alternated loops of 30 '
            '(min .. max)' % ('Glow on (3, 32, 32)' if what == 'c4' else 'MAF on normals', s['layers'], s['B'], s['numel'], a.rounds))
        say('  options off   %s   captured: %s   loss %.4f' % (_f(off), s['captured_off'], s['loss_off']))
        say('  all three on  %s   captured: %s   loss %.4f' % (_f(on), s['captured_on'], s['loss_on']))
        say('  difference of the medians %+.2f us = %+.3f %% of the options-off step; guard state %s'
            % (on[0] - off[0], 100.0 * (on[0] - off[0]) / off[0], json.dumps(s['guard_state'])))
    k = kernel_case(torch, pkg, results[0]['numel'], a.rounds, dev)
    results.append(k)
    say('the launches alone at the C4 bucket size, n = %d: microseconds per call between two events over 50 calls, median of %d '
        'alternated rounds (min .. max)' % (k['n'], a.rounds))
    for name, e in k['forms'].items():
        say('  %-46s %s   %6.1f MB   %5.1f %% of 8 TB/s' % (name, _f(e['us']), e['bytes'] / 1e6, 100.0 * e['bytes'] / (e['us'][0] * 1e-6) / HBM_PEAK))
    say('  persistent-kernel timeouts: %d' % pkg._native.persistent_timeouts())
    say(json.dumps(results))
    if a.out:
        path = os.path.join(ROOT, a.out)
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        with open(path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
