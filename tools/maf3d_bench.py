"""MAF on 3-D data (the shipped config: layers = 10, on `swiss`) on one GPU: the captured training step and the one-launch inverse with
device-drawn MADE masks (MAF.draws = 'device', csrc/made_masks.hip) against the host-drawn forms of the same model.

    python tools/maf3d_bench.py [--batches 1024,16384] [--iters 30] [--repeats 5] [--out profiles/r11_maf3d.txt]

Per batch size, in ONE child process (so the forms share a GPU and its state):
    training step   FlowTrainer(graph=True), 'device' draws: one hipGraph replay, batch drawn by data.DeviceSampler inside the graph
                    FlowTrainer(graph=False), 'host' draws: eager launches, masks redrawn from np.random and uploaded when they change
                    (what FlowTrainer ran for this model before the device draw existed), same sampler
    sample_y        'device' draws: one nf_maf_step_inv_drawn launch per step;  'host' draws: D conditioner passes per step on per-layer launches
Every figure is the median of --repeats timed loops of --iters calls between two events, after warm-up calls; the spread (min .. max of the
repeats) is printed with it.  The driver process never touches the GPU: every child runs under its own `timeout`, and the first failure
stops the tool (nothing further is started on the GPU)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT_S = 240


def timed(torch, fn, iters, repeats, warmup=3):
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


def child(B, layers, data, iters, repeats):
    import numpy as np
    import torch
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    train = importlib.import_module('normalizing-flows-pytorch_amd.train')
    nfdata = importlib.import_module('normalizing-flows-pytorch_amd.data')
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    D = 3

    def make(graph):
        torch.manual_seed(0)
        np.random.seed(0)
        net = pkg.MAF((D, ), '2d', NS(layers=layers)).to(dev)
        return train.FlowTrainer(net, graph=graph, warmup=2, sampler=nfdata.DeviceSampler(data, B, (D, )))

    out = {'B': B, 'layers': layers, 'data': data, 'device': torch.cuda.get_device_name(0)}
    for name, graph in (('device_graph', True), ('host_eager', False)):
        tr = make(graph)
        for _ in range(4):
            tr.train_on_batch()
        out['draws_' + name] = tr.net.draws
        out['captured_' + name] = tr._g_fb is not None
        out['step_%s_us' % name] = timed(torch, tr.train_on_batch, iters, repeats)
        z, loss = tr.train_on_batch()
        out['loss_' + name] = float(loss)
        out['sample_%s_us' % tr.net.draws] = timed(torch, lambda: tr.sample_y(B, (D, )), max(2, iters // 3), repeats, warmup=2)
    out['persistent_timeouts'] = pkg._native.persistent_timeouts()
    print('RESULT ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', type=int, default=None, metavar='B', help='(internal) measure batch size B in this process')
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--data', default='swiss')
    ap.add_argument('--batches', default='1024,16384')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'r11_maf3d.txt'))
    a = ap.parse_args()
    if a.child is not None:
        child(a.child, a.layers, a.data, a.iters, a.repeats)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def f(v):
        return '%9.1f (%.1f .. %.1f)' % tuple(v)
    results = []
    for B in [int(b) for b in a.batches.split(',')]:
        cmd = ['timeout', '-k', '10', str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), '--child', str(B), '--layers', str(a.layers),
               '--data', a.data, '--iters', str(a.iters), '--repeats', str(a.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        res = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not res:
            say('B = %d: the measuring process ended with status %d; stopping here' % (B, r.returncode))
            say(r.stderr[-2000:])
            break
        s = json.loads(res[-1][7:])
        results.append(s)
        if not results[:-1]:
            say('MAF, layers = %d, D = 3, %s, %s; microseconds per call, median of %d loops of %d calls (min .. max)'
                % (a.layers, a.data, s['device'], a.repeats, a.iters))
        g, e = s['step_device_graph_us'], s['step_host_eager_us']
        say('B = %d' % B)
        say('  training step, hipGraph replay, device draws   %s   captured: %s   loss %.4f' % (f(g), s['captured_device_graph'], s['loss_device_graph']))
        say('  training step, eager launches, host draws      %s   x%.2f   loss %.4f' % (f(e), e[0] / g[0], s['loss_host_eager']))
        sd, sh = s['sample_device_us'], s['sample_host_us']
        say('  sample_y, %5d rows, device draws              %s' % (B, f(sd)))
        say('  sample_y, %5d rows, host draws                %s   x%.2f' % (B, f(sh), sh[0] / sd[0]))
        say('  persistent-kernel timeouts: %d' % s['persistent_timeouts'])
    say(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)) or '.', exist_ok=True)
        with open(os.path.join(ROOT, a.out), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    sys.exit(0 if len(results) == len(a.batches.split(',')) else 1)


if __name__ == '__main__':
    main()
