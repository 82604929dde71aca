"""Training from a data SET on one GPU: batches gathered inside the captured step by data.DeviceDataset (csrc/dataset.hip) against the
way a data set had to be fed before it existed -- the batch indexed and built on the host as flows/dataset.py:111-127 does, copied to
the device (main.py:79) and handed to FlowTrainer.train_on_batch(y) under graph=True, which copies it into the graph's static input.

    python tools/dataset_bench.py [--iters 30] [--repeats 5] [--glow-layers 32] [--out profiles/r12_dataset.txt]

Workloads, each in ONE child process (both forms share a GPU and its state):
    maf     C5-shaped MAF (2-D, 10 layers), B = 16 384 rows of the 65 536-point toy set `normals`
    glow    C4-shaped Glow on (3, 32, 32), B = 64 images of a random uint8 (50000, 32, 32, 3) array
    gather  the gather launch alone at B = 64 / 512 / 4096 CIFAR-shaped images, as bytes moved (uint8 read + float32 written) over
            8 TB/s
A training figure is wall-clock microseconds per step -- the host's share is what is being compared -- over loops of --iters steps
closed by a synchronise; the gather's is the time between two events.  Medians of --repeats loops with (min .. max).  The driver
process never touches the GPU: every child runs under its own `timeout`, and the first failure stops the tool (nothing further is
started on the GPU)."""
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
HBM_BYTES_PER_S = 8.0e12


def _stats(v):
    return statistics.median(v), min(v), max(v)


def wall(torch, fn, iters, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / iters)
    return _stats(out)


def events(torch, fn, iters, repeats, warmup=3):
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
    return _stats(out)


class HostLoader:
    """flows/dataset.py:103-127 on an in-memory array: shuffle an index array per pass, slice it, build the batch with numpy"""

    def __init__(self, np, arr, batch):
        self.np, self.arr, self.batch, self.rng = np, arr, batch, np.random.default_rng(0)
        self._initialize()

    def _initialize(self):
        self.iter, self.indices = 0, self.np.arange(len(self.arr))
        self.rng.shuffle(self.indices)

    def next(self):
        np = self.np
        if len(self.arr) <= self.iter + self.batch:
            self._initialize()
        idx = self.indices[self.iter:self.iter + self.batch]
        self.iter += self.batch
        if self.arr.dtype == np.uint8:
            return np.ascontiguousarray(np.transpose(self.arr[idx].astype('float32') / 255.0, (0, 3, 1, 2)))
        return self.arr[idx]


def child(what, layers, iters, repeats):
    import numpy as np
    import torch
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    train = importlib.import_module('normalizing-flows-pytorch_amd.train')
    nfdata = importlib.import_module('normalizing-flows-pytorch_amd.data')
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    out = {'what': what, 'device': torch.cuda.get_device_name(0)}
    if what == 'gather':
        arr = np.random.default_rng(0).integers(0, 256, size=(50000, 32, 32, 3), dtype=np.uint8)
        for B in (64, 512, 4096):
            ds = nfdata.DeviceDataset(arr, B, device=dev)
            N = ds._N

            def gather():
                N.call('nf_dataset_gather_u8', ds.data.data_ptr(), ds.out.data_ptr(), ds.n, 32, 32, 3, 0, B, B, 0, ds.steps_per_epoch, ds.seed, 1,
                       ds.step.data_ptr(), ds.last_indices.data_ptr(), N.stream())
            out['gather_%d_us' % B] = events(torch, gather, max(iters, 50), repeats)
            out['gather_%d_bytes' % B] = B * 3072 * 5
    else:
        if what == 'maf':
            B, make = 16384, lambda: pkg.MAF((2, ), '2d', NS(layers=layers))
            arr = nfdata.GENERATORS['normals'](nfdata.N_DATASET_SIZE, np.random.default_rng(0))
        else:
            B, make = 64, lambda: pkg.Glow((3, 32, 32), 'image', NS(layers=layers, mixtures=None))
            arr = np.random.default_rng(0).integers(0, 256, size=(50000, 32, 32, 3), dtype=np.uint8)
        out['B'], out['layers'] = B, layers
        for name in ('host', 'device'):
            torch.manual_seed(0)
            np.random.seed(0)
            net = make().to(dev)
            if name == 'host':
                loader = HostLoader(np, arr, B)
                tr = train.FlowTrainer(net, graph=True, warmup=2)

                def step():
                    return tr.train_on_batch(torch.from_numpy(loader.next()).to(dev, non_blocking=True))
            else:
                tr = train.FlowTrainer(net, graph=True, warmup=2, sampler=nfdata.DeviceDataset(arr, B, device=dev))
                step = tr.train_on_batch
            for _ in range(4):
                step()
            out['captured_' + name] = tr._g_fb is not None
            out['step_%s_us' % name] = wall(torch, step, iters, repeats)
            out['loss_' + name] = float(step()[1])
    out['persistent_timeouts'] = pkg._native.persistent_timeouts()
    print('RESULT ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, choices=('maf', 'glow', 'gather'), help='(internal) measure one workload in this process')
    ap.add_argument('--layers', type=int, default=None, help='(internal)')
    ap.add_argument('--maf-layers', type=int, default=10)
    ap.add_argument('--glow-layers', type=int, default=32)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'r12_dataset.txt'))
    a = ap.parse_args()
    if a.child is not None:
        child(a.child, a.layers, a.iters, a.repeats)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def f(v):
        return '%9.1f (%.1f .. %.1f)' % tuple(v)
    results = []
    jobs = (('maf', a.maf_layers), ('glow', a.glow_layers), ('gather', 0))
    for what, layers in jobs:
        cmd = ['timeout', '-k', '10', str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), '--child', what, '--layers', str(layers),
               '--iters', str(a.iters), '--repeats', str(a.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not res:
            say('%s: the measuring process ended with status %d; stopping here' % (what, r.returncode))
            say(r.stderr[-2000:])
            break
        s = json.loads(res[-1][7:])
        results.append(s)
        if not results[:-1]:
            say('training from a data set, %s; microseconds per call, median of %d loops of %d calls (min .. max)'
                % (s['device'], a.repeats, a.iters))
        if what == 'gather':
            say('gather launch alone, CIFAR shape, set of 50000 images (between events)')
            for B in (64, 512, 4096):
                us, nb = s['gather_%d_us' % B], s['gather_%d_bytes' % B]
                say('  B = %4d   %s   %.3f GB moved   %.1f %% of 8 TB/s' % (B, f(us), nb / 1e9, 100.0 * nb / (us[0] * 1e-6) / HBM_BYTES_PER_S))
        else:
            h, d = s['step_host_us'], s['step_device_us']
            say('%s, layers = %d, B = %d (wall clock, hipGraph step)' % ('MAF on normals (65536 points)' if what == 'maf' else
                                                                       'Glow on uint8 (50000, 32, 32, 3)', s['layers'], s['B']))
            say('  (a) batch built on the host, copied, train_on_batch(y)   %s   captured: %s   loss %.4f' % (f(h), s['captured_host'], s['loss_host']))
            say('  (b) sampler = DeviceDataset, gathered inside the graph  %s   captured: %s   loss %.4f   (a) / (b) = %.2f'
                % (f(d), s['captured_device'], s['loss_device'], h[0] / d[0]))
        say('  persistent-kernel timeouts: %d' % s['persistent_timeouts'])
    say(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)) or '.', exist_ok=True)
        with open(os.path.join(ROOT, a.out), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    sys.exit(0 if len(results) == len(jobs) else 1)


if __name__ == '__main__':
    main()
