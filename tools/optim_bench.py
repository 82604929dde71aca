"""What the fused optimizer steps cost, and what the warmup + cosine schedule launch costs the captured training step, on one GPU
(csrc/optim.hip: the eight nf_X_step / nf_X_step_guarded entry points, nf_lr_schedule).

    python tools/optim_bench.py [--rounds 5] [--maf-layers 10] [--out profiles/r17_optim.txt]

One process, so that every form shares the GPU and its state:
    kernel  at the C4 model's bucket size (8 380 754 parameters): all eight step entry points of csrc/optim.hip, the guarded ones with
            the average -- microseconds between two events over 50 calls, alternated, median (min .. max) of --rounds, and the bytes
            each must move as a share of 8 TB/s.  nf_adam_step is the yardstick of the plain 28 B steps: one of them is within it when
            its median is no further above nf_adam_step's than nf_adam_step's own min .. max spread in this run; if it is not, the
            line says by how much.  The same rule compares two builds: an entry point's median against its own in the other build.
    step    the captured step of the C5 shape (MAF on `normals`, B = 16 384) without a schedule and with lr_warmup_steps +
            cosine_steps (one more one-thread node in the graph): --rounds alternated loops of 30 steps each, wall-clock microseconds
            per step, median (min .. max) over the loops
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
C4_NUMEL = 8380754
SCHEDULE = dict(lr_warmup_steps=50, lr_warmup_start=1.0 / 3.0, cosine_steps=100000, lr_min=1e-6)


def _stats(v):
    return statistics.median(v), min(v), max(v)


def _f(v):
    return '%10.2f (%.2f .. %.2f)' % tuple(v)


ENTRIES = tuple('nf_%s_step%s' % (r, g) for g in ('', '_guarded') for r in ('adam', 'rmsprop', 'adamax', 'adamw'))


def kernel_case(torch, pkg, n, rounds, dev):
    N = pkg._native
    g = torch.Generator(device=dev).manual_seed(0)
    p, gr, m, ema = (torch.randn(n, device=dev, generator=g) for _ in range(4))
    v = torch.rand(n, device=dev, generator=g)
    step, lr = torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1, ), 1e-4, device=dev)
    ctl = torch.zeros(8, dtype=torch.int32, device=dev)
    partials = torch.zeros(N.header_constant('NF_GUARD_MAX_PARTIALS'), dtype=torch.float64, device=dev)
    for _ in range(2):                                       # a control block that says "take it", past the step that copies the average
        N.call('nf_grad_guard', gr.data_ptr(), n, 100.0, 1, partials.data_ptr(), ctl.data_ptr(), step.data_ptr(), N.stream())

    def form(entry):
        """(bytes the launch must move, the call): RMSprop has one state buffer, alpha for the betas and, guarded, no step argument"""
        rms, guarded = 'rmsprop' in entry, entry.endswith('_guarded')
        args = [p.data_ptr(), gr.data_ptr()] + ([] if rms else [m.data_ptr()]) + [v.data_ptr()]
        args += ([] if rms and guarded else [step.data_ptr()]) + [lr.data_ptr()] + ([0.99] if rms else [0.9, 0.999]) + [1e-8, 0.01]
        args += [ctl.data_ptr(), ema.data_ptr(), 0.999] if guarded else [1.0]
        return 4 * n * ((5 if rms else 7) + (2 if guarded else 0)), lambda: N.call(entry, *args, n, N.stream())

    forms = {name: form(name) for name in ENTRIES}
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
    return {'n': n, 'bytes': {k: forms[k][0] for k in forms}, 'us': {k: _stats(got[k]) for k in forms}}


def step_case(torch, pkg, train, nfdata, layers, rounds, dev):
    import numpy as np
    B = 16384
    arr = nfdata.GENERATORS['normals'](nfdata.N_DATASET_SIZE, np.random.default_rng(0))
    trainers = {}
    for name, kw in (('plain', {}), ('scheduled', SCHEDULE)):
        torch.manual_seed(0)
        np.random.seed(0)
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
    out = {'B': B, 'layers': layers, 'numel': trainers['plain'].bucket.numel}
    for name, tr in trainers.items():
        out['captured_' + name] = tr._g_fb is not None
        out['step_%s_us' % name] = _stats(got[name])
        out['loss_' + name] = float(tr.train_on_batch()[1])
        out['lr_' + name] = tr.current_lr()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maf-layers', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--numel', type=int, default=C4_NUMEL)
    ap.add_argument('--out', default=os.path.join('profiles', 'r17_optim.txt'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('optim_bench measures on the GPU and there is none: not measured')
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    train = importlib.import_module('normalizing-flows-pytorch_amd.train')
    nfdata = importlib.import_module('normalizing-flows-pytorch_amd.data')
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('the fused optimizer steps, and the schedule launch inside the captured step, %s' % torch.cuda.get_device_name(0))
    k = kernel_case(torch, pkg, a.numel, a.rounds, dev)
    say('the launches alone at the C4 bucket size, n = %d: microseconds per call between two events over 50 calls, median of %d '
        'alternated rounds (min .. max)' % (k['n'], a.rounds))
    yard = k['us']['nf_adam_step']
    spread = yard[2] - yard[1]
    for name, us in k['us'].items():
        note = ''
        if name == 'nf_adam_step':
            note = 'the yardstick of the 28 B plain steps; its own spread %.2f us' % spread
        elif k['bytes'][name] == k['bytes']['nf_adam_step']:
            over = us[0] - yard[0]
            note = ('%+.2f us against the yardstick: within its spread' % over if over <= spread else
                    '%+.2f us against the yardstick: SLOWER than its spread of %.2f us allows, by %.2f us' % (over, spread, over - spread))
        say('  %-24s %s   %6.1f MB   %5.1f %% of 8 TB/s   %s' % (name, _f(us), k['bytes'][name] / 1e6,
                                                                100.0 * k['bytes'][name] / (us[0] * 1e-6) / HBM_PEAK, note))
    s = step_case(torch, pkg, train, nfdata, a.maf_layers, a.rounds, dev)
    plain, sched = s['step_plain_us'], s['step_scheduled_us']
    say('MAF on normals, layers = %d, B = %d, bucket of %d parameters: microseconds per captured step, median of %d alternated '
        'loops of 30 (min .. max)' % (s['layers'], s['B'], s['numel'], a.rounds))
    say('  no schedule       %s   captured: %s   loss %.4f   rate %.3e' % (_f(plain), s['captured_plain'], s['loss_plain'], s['lr_plain']))
    say('  warmup + cosine   %s   captured: %s   loss %.4f   rate %.3e' % (_f(sched), s['captured_scheduled'], s['loss_scheduled'],
                                                                           s['lr_scheduled']))
    say('  difference of the medians %+.2f us = %+.3f %% of the unscheduled step (options: %s)'
        % (sched[0] - plain[0], 100.0 * (sched[0] - plain[0]) / plain[0], json.dumps(SCHEDULE)))
    say('  persistent-kernel timeouts: %d' % pkg._native.persistent_timeouts())
    say(json.dumps([k, s]))
    if a.out:
        path = os.path.join(ROOT, a.out)
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        with open(path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
