"""What the fused autoregressive spline head costs beside the same transform through the kernels that existed before it, and what a captured
SplineMAF step costs beside a MAF step of the same depth, on one GPU (csrc/arspline.hip: nf_arspline_head_fwd / _bwd).

    python tools/spline_maf_bench.py [--rounds 5] [--layers 10] [--out profiles/r20_spline_maf.txt]

One process, so that every form shares the GPU and its state:
    head    D in {2, 8} features, K = 8, hidden width 32, B in {4096, 65536, 1048576}; microseconds per call between two events over 20
            calls, alternated, median (min .. max) of --rounds:
              fused         forward (all D features), backward (the launch + the nf_slab_sum that folds its weight / bias slabs) and the
                            inverse of ONE column (what each of the layer's D passes launches)
              materialised  the same results from existing kernels: F.linear writes params (B, (3K - 1) D), nf_rqs_coupling_fwd / _bwd run on
                            the features interleaved with a zero pass-through half (NF_SPLIT_1D transforms the even positions: exactly the
                            p D + d layout); its backward adds the three products of the linear layer (g_a, g_weight, g_bias); its inverse
                            inverts every column (the existing kernel has no one-column form)
            and the bytes of the (B, (3K - 1) D) tensor the fused form never writes
    step    the captured training step of SplineMAF (layers = --layers, B = 16384, DeviceSampler('moons')) beside MAF at the same depth and
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
K = 8
BOUND = 3.0
H = 32
PS = 3 * K - 1


def _stats(v):
    return statistics.median(v), min(v), max(v)


def _f(v):
    return '%10.2f (%.2f .. %.2f)' % tuple(v)


def head_case(torch, pkg, B, D, rounds, dev):
    import numpy as np
    import torch.nn.functional as F
    N, NF = pkg._native, pkg.functional
    cond = importlib.import_module(pkg.__name__ + '.conditioners')
    fconv = importlib.import_module(pkg.__name__ + '.fused_conv')
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.relu(torch.randn(B, H, device=dev, generator=g))
    w = 0.18 * torch.randn(PS * D, H, device=dev, generator=g)
    b = 0.5 * torch.randn(PS * D, device=dev, generator=g)
    mask = torch.from_numpy(cond.made_masks_from_degrees(D, [np.arange(H) % max(1, D - 1)] * 3)[-1]).to(dev)
    z = 2.0 * torch.randn(B, D, device=dev, generator=g)
    g_y, g_ld = torch.randn(B, D, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
    ld = torch.zeros(B, device=dev)
    y, x, g_a, g_z = torch.empty_like(z), torch.empty_like(z), torch.empty_like(a), torch.empty_like(z)
    g_w, g_b = torch.empty_like(w), torch.empty_like(b)
    n = int(N.load().nf_arspline_head_slabs(B))
    gw_s, gb_s = torch.empty(n * PS * D * H, device=dev), torch.empty(n * PS * D, device=dev)
    s = N.stream
    # the materialised route's tensors
    wm = (w * mask.repeat(PS, 1)).contiguous()
    zz = torch.stack([z, torch.zeros_like(z)], 2).reshape(B, 2 * D).contiguous()
    g_yy = torch.stack([g_y, torch.zeros_like(g_y)], 2).reshape(B, 2 * D).contiguous()
    yy, xx, g_zz = torch.empty_like(zz), torch.empty_like(zz), torch.empty_like(zz)
    keep = {}

    def fused_bwd():
        N.call('nf_arspline_head_bwd', g_y.data_ptr(), g_ld.data_ptr(), a.data_ptr(), w.data_ptr(), b.data_ptr(), mask.data_ptr(), z.data_ptr(),
               g_a.data_ptr(), g_z.data_ptr(), gw_s.data_ptr(), gb_s.data_ptr(), K, BOUND, B, D, H, s())
        fconv._slab_sum([(gw_s, g_w, PS * D * H, PS * D * H, n, False, 1), (gb_s, g_b, PS * D, PS * D, n, False, 1)])

    def mat_fwd():
        keep['p'] = F.linear(a, wm, b)
        N.call('nf_rqs_coupling_fwd', zz.data_ptr(), keep['p'].data_ptr(), yy.data_ptr(), ld.data_ptr(), K, BOUND, 0, 0, 0, B, 2 * D, 1, 1, s())

    def mat_inv():
        p = F.linear(a, wm, b)
        N.call('nf_rqs_coupling_fwd', yy.data_ptr(), p.data_ptr(), xx.data_ptr(), ld.data_ptr(), K, BOUND, 0, 0, 1, B, 2 * D, 1, 1, s())

    def mat_bwd():
        p = keep['p']
        g_p = torch.empty_like(p)
        N.call('nf_rqs_coupling_bwd', g_yy.data_ptr(), g_ld.data_ptr(), zz.data_ptr(), p.data_ptr(), g_zz.data_ptr(), g_p.data_ptr(), K, BOUND, 0, 0,
               B, 2 * D, 1, 1, s())
        keep['g'] = (torch.mm(g_p, wm), torch.mm(g_p.t(), a), g_p.sum(0))

    forms = {
        ('fused', 'fwd'): lambda: N.call('nf_arspline_head_fwd', a.data_ptr(), w.data_ptr(), b.data_ptr(), mask.data_ptr(), z.data_ptr(), y.data_ptr(),
                                         ld.data_ptr(), K, BOUND, 0, -1, B, D, H, s()),
        ('fused', 'inv'): lambda: N.call('nf_arspline_head_fwd', a.data_ptr(), w.data_ptr(), b.data_ptr(), mask.data_ptr(), y.data_ptr(), x.data_ptr(),
                                         ld.data_ptr(), K, BOUND, 1, D - 1, B, D, H, s()),
        ('fused', 'bwd'): fused_bwd,
        ('materialised', 'fwd'): mat_fwd,
        ('materialised', 'inv'): mat_inv,
        ('materialised', 'bwd'): mat_bwd,
    }
    got = {k: [] for k in forms}
    for fn in forms.values():                                # (forward before inverse and backward: they run on the forward's output)
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
    # the two routes must agree (last column: the one the fused inverse inverted)
    gap_y = float((y - yy.view(B, D, 2)[:, :, 0]).abs().max())
    gap_x = float((x[:, D - 1] - xx.view(B, D, 2)[:, D - 1, 0]).abs().max())
    gap_gw = float((g_w - keep['g'][1] * mask.repeat(PS, 1)).abs().max() / max(1.0, float(keep['g'][1].abs().max())))
    return {'B': B, 'D': D, 'us': {'%s_%s' % k: _stats(v) for k, v in got.items()}, 'gap_y': gap_y, 'gap_x': gap_x, 'gap_gw_rel': gap_gw,
            'params_bytes': 4 * B * PS * D}


def step_case(torch, pkg, train, nfdata, layers, rounds, dev):
    import numpy as np
    B = 16384
    trainers = {}
    for name, cls in (('SplineMAF', pkg.SplineMAF), ('MAF', pkg.MAF)):
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
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'r20_spline_maf.txt'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('spline_maf_bench measures on the GPU and there is none: not measured')
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    train = importlib.import_module('normalizing-flows-pytorch_amd.train')
    nfdata = importlib.import_module('normalizing-flows-pytorch_amd.data')
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('fused autoregressive spline head beside the materialised route through the existing kernels, and SplineMAF beside MAF, %s'
        % torch.cuda.get_device_name(0))
    say('the head alone, K = %d, hidden width %d: microseconds per call between two events over 20 calls, median of %d alternated rounds '
        '(min .. max)' % (K, H, a.rounds))
    cases = []
    for D in (2, 8):
        for B in (4096, 65536, 1048576):
            k = head_case(torch, pkg, B, D, a.rounds, dev)
            cases.append(k)
            say('  D = %d, B = %d: the parameter tensor the fused form never writes is %.1f MB; fused - materialised: |y| %.2e, |x| %.2e, '
                '|g_weight| %.2e of its largest entry' % (D, B, k['params_bytes'] / 1e6, k['gap_y'], k['gap_x'], k['gap_gw_rel']))
            u = k['us']
            for d, note in (('fwd', ''), ('bwd', ''), ('inv', '   (fused: one column; materialised: every column)')):
                say('    %-3s  fused %s   materialised %s   fused / materialised %.2f%s'
                    % (d, _f(u['fused_' + d]), _f(u['materialised_' + d]), u['fused_' + d][0] / u['materialised_' + d][0], note))
    s = step_case(torch, pkg, train, nfdata, a.layers, a.rounds, dev)
    say('captured training step on moons, layers = %d, B = %d: microseconds per step, median of %d alternated loops of 30 (min .. max)'
        % (s['layers'], s['B'], a.rounds))
    for name in ('SplineMAF', 'MAF'):
        say('  %-11s %s   captured: %s   %d parameters   loss %.4f' % (name, _f(s['step_%s_us' % name]), s['captured_' + name], s['numel_' + name],
                                                                     s['loss_' + name]))
    say('  SplineMAF / MAF: %.2f' % (s['step_SplineMAF_us'][0] / s['step_MAF_us'][0]))
    say('  persistent-kernel timeouts: %d' % pkg._native.persistent_timeouts())
    say(json.dumps([cases, s]))
    if a.out:
        path = os.path.join(ROOT, a.out)
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        with open(path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
