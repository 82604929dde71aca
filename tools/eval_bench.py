"""Held-out evaluation and dequantised batches on one GPU: FlowTrainer.evaluate over a device-resident sweep set (csrc/dataset.hip,
csrc/logp.hip) against the host loop it replaces, the dequantising gather against the plain one, and the captured training step on
dequantised batches against the same step on uint8 / 255.

    python tools/eval_bench.py [--repeats 5] [--glow-layers 32] [--out profiles/r14_eval.txt]

Cases, each in ONE child process (every form of a case shares a GPU and its state):
    eval_maf       C5-shaped MAF (2-D, 10 layers) over the 65 536-point toy set `normals`, B = 16 384 (4 steps)
    eval_glow_64   C4-shaped Glow on (3, 32, 32) over a random uint8 (10000, 32, 32, 3) set, B = 64 (157 steps, tail of 16)
    eval_glow_512  the same at B = 512 (20 steps, tail of 272)
                   three forms, wall-clock milliseconds per whole sweep, median of --repeats (min .. max):
                     evaluate()            eager launches, one read at the end
                     evaluate(graph=True)  one captured step replayed (the figure includes the capture, which every call repeats)
                     the host loop         host_batch(step) -> .to('cuda') -> log_py -> .sum().item() per batch
                   The image set is scored WITHOUT dequantisation, so that the host loop does what a user's loop does (index, / 255,
                   transpose) and not a numpy restatement of Philox.
    gather         the gather launch alone on CIFAR-shaped images (set of 50000), plain against dequantised, B = 64 / 512 / 4096,
                   alternated loop by loop, microseconds between two events
    train          the captured C4 training step (Glow, B = 64) from DeviceDataset(dequantize=True) against dequantize=False: four
                   alternated loops each, wall-clock microseconds per step, mean and (min .. max)
The driver process never touches the GPU: every child runs under its own `timeout`, and the first failure stops the tool (nothing
further is started on the GPU)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT_S = 300
CASES = ('eval_maf', 'eval_glow_64', 'eval_glow_512', 'gather', 'train')


def _stats(v):
    return statistics.median(v), min(v), max(v)


def _sweep_ms(torch, fn, repeats):
    fn()                                                     # warm-up: allocations, first launches
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stats(out)


def child(what, layers, repeats):
    import numpy as np
    import torch
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    train = importlib.import_module('normalizing-flows-pytorch_amd.train')
    nfdata = importlib.import_module('normalizing-flows-pytorch_amd.data')
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    out = {'what': what, 'device': torch.cuda.get_device_name(0)}
    torch.manual_seed(0)
    np.random.seed(0)
    if what.startswith('eval_'):
        if what == 'eval_maf':
            B, net = 16384, pkg.MAF((2, ), '2d', NS(layers=layers)).to(dev)
            arr = nfdata.GENERATORS['normals'](nfdata.N_DATASET_SIZE, np.random.default_rng(0))
        else:
            B, net = int(what.rsplit('_', 1)[1]), pkg.Glow((3, 32, 32), 'image', NS(layers=layers, mixtures=None)).to(dev)
            arr = np.random.default_rng(0).integers(0, 256, size=(10000, 32, 32, 3), dtype=np.uint8)
        ds = nfdata.DeviceDataset(arr, B, device=dev)
        tr = train.FlowTrainer(net, sampler=ds)
        for _ in range(4):                                   # the data-dependent initialisations
            tr.train_on_batch()
        ev = ds.sweep_view()
        out.update(B=B, layers=layers, n=ev.n, steps=ev.steps_per_epoch)

        def host_loop():
            total = 0.0
            for s in range(ev.steps_per_epoch):
                lp = tr.log_py(ev.host_batch(s).to('cuda'))
                total += lp[:ev.valid(s)].sum().item()
            return -total / ev.n
        import warnings
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            res_g = tr.evaluate(ev, graph=True)
        out['captured'] = not any('capture' in str(w.message) for w in caught)
        res = tr.evaluate(ev)
        out['nll_eager'], out['nll_graph'], out['nll_host'], out['n_counted'] = res['nll'], res_g['nll'], host_loop(), res['n']
        out['eager_ms'] = _sweep_ms(torch, lambda: tr.evaluate(ev), repeats)
        out['graph_ms'] = _sweep_ms(torch, lambda: tr.evaluate(ev, graph=True), repeats)
        out['host_ms'] = _sweep_ms(torch, host_loop, repeats)
    elif what == 'gather':
        arr = np.random.default_rng(0).integers(0, 256, size=(50000, 32, 32, 3), dtype=np.uint8)
        base = nfdata.DeviceDataset(arr, 64, device=dev)
        for B in (64, 512, 4096):
            sets = {}
            for name, dq in (('plain', False), ('dequant', True)):
                sets[name] = nfdata.DeviceDataset(arr, B, device=None, dequantize=dq, _share=base.data)
            for ds in sets.values():
                for _ in range(5):
                    ds.next()
            torch.cuda.synchronize()
            got = {'plain': [], 'dequant': []}
            for _ in range(repeats):                         # alternated
                for name, ds in sets.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(50):
                        ds.gather()
                    b.record()
                    torch.cuda.synchronize()
                    got[name].append(a.elapsed_time(b) * 1e3 / 50)
            for name in got:
                out['gather_%s_%d_us' % (name, B)] = _stats(got[name])
    else:
        arr = np.random.default_rng(0).integers(0, 256, size=(50000, 32, 32, 3), dtype=np.uint8)
        base, trainers = None, {}
        for name, dq in (('plain', False), ('dequant', True)):
            torch.manual_seed(0)
            net = pkg.Glow((3, 32, 32), 'image', NS(layers=layers, mixtures=None)).to(dev)
            ds = nfdata.DeviceDataset(arr, 64, device=dev if base is None else None, dequantize=dq, _share=None if base is None else base.data)
            base = base or ds
            tr = train.FlowTrainer(net, graph=True, warmup=2, sampler=ds)
            for _ in range(6):
                tr.train_on_batch()
            trainers[name] = tr
            out['captured_' + name] = tr._g_fb is not None
        torch.cuda.synchronize()
        got = {'plain': [], 'dequant': []}
        for _ in range(4):                                   # four alternated loops each
            for name, tr in trainers.items():
                t0 = time.perf_counter()
                for _ in range(30):
                    tr.train_on_batch()
                torch.cuda.synchronize()
                got[name].append((time.perf_counter() - t0) * 1e6 / 30)
        for name, tr in trainers.items():
            out['step_%s_us' % name] = [statistics.mean(got[name]), min(got[name]), max(got[name])]
            out['loss_' + name] = float(tr.train_on_batch()[1])
        out['B'], out['layers'] = 64, layers
    out['persistent_timeouts'] = pkg._native.persistent_timeouts()
    print('RESULT ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, choices=CASES, help='(internal) measure one case in this process')
    ap.add_argument('--layers', type=int, default=None, help='(internal)')
    ap.add_argument('--maf-layers', type=int, default=10)
    ap.add_argument('--glow-layers', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'r14_eval.txt'))
    a = ap.parse_args()
    if a.child is not None:
        child(a.child, a.layers, a.repeats)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def f(v):
        return '%9.2f (%.2f .. %.2f)' % tuple(v)
    results = []
    for what in CASES:
        layers = a.maf_layers if what == 'eval_maf' else (0 if what == 'gather' else a.glow_layers)
        cmd = ['timeout', '-k', '10', str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), '--child', what, '--layers', str(layers),
               '--repeats', str(a.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not res:
            say('%s: the measuring process ended with status %d; stopping here' % (what, r.returncode))
            say(r.stderr[-2000:])
            break
        s = json.loads(res[-1][7:])
        results.append(s)
        if not results[:-1]:
            say('held-out evaluation and dequantised batches, %s' % s['device'])
        if what.startswith('eval_'):
            say('%s, layers = %d, N = %d, B = %d, %d steps: milliseconds per whole sweep, median of %d (min .. max)'
                % ('MAF on normals' if what == 'eval_maf' else 'Glow on uint8 (10000, 32, 32, 3)', s['layers'], s['n'], s['B'], s['steps'], a.repeats))
            e, g, h = s['eager_ms'], s['graph_ms'], s['host_ms']
            say('  evaluate(), eager launches                 %s   nll %.6f   n %d' % (f(e), s['nll_eager'], s['n_counted']))
            say('  evaluate(graph=True), capture included     %s   nll %.6f   captured: %s' % (f(g), s['nll_graph'], s['captured']))
            say('  host loop (host_batch, copy, log_py, item) %s   nll %.6f   host / eager = %.2f   host / graph = %.2f'
                % (f(h), s['nll_host'], h[0] / e[0], h[0] / g[0]))
        elif what == 'gather':
            say('gather launch alone, CIFAR shape, set of 50000 images: microseconds between events, median of %d alternated loops of 50 '
                '(min .. max)' % a.repeats)
            for B in (64, 512, 4096):
                p, d = s['gather_plain_%d_us' % B], s['gather_dequant_%d_us' % B]
                say('  B = %4d   plain %s   dequantised %s   dequantised / plain = %.2f' % (B, f(p), f(d), d[0] / p[0]))
        else:
            p, d = s['step_plain_us'], s['step_dequant_us']
            say('captured training step, Glow layers = %d, B = %d: microseconds per step, mean of 4 alternated loops of 30 (min .. max)'
                % (s['layers'], s['B']))
            say('  dequantize=False   %s   captured: %s   loss %.4f' % (f(p), s['captured_plain'], s['loss_plain']))
            say('  dequantize=True    %s   captured: %s   loss %.4f   dequantised / plain = %.4f'
                % (f(d), s['captured_dequant'], s['loss_dequant'], d[0] / p[0]))
        say('  persistent-kernel timeouts: %d' % s['persistent_timeouts'])
    say(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)) or '.', exist_ok=True)
        with open(os.path.join(ROOT, a.out), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    sys.exit(0 if len(results) == len(CASES) else 1)


if __name__ == '__main__':
    main()
