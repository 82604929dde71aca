"""FlowTrainer.report on one GPU against the host loop it replaces (main.py:135-284 without the figure library).

    python tools/report_bench.py [--repeats 5] [--layers 4] [--image-layers 2] [--out profiles/r15_report.txt]

One process, one GPU; wall-clock milliseconds per whole report, median of --repeats (min .. max), after one warm-up call each:
    2-D      Glow on (2, ), a batch of n = 1 024 `moons` points: three 512 x 512 scatter panels (radius 2), 1 024 samples, the
             256 x 256 density map
    images   Glow on (3, 32, 32), a batch of n = 64: two 8 x 8 grids, 64 samples
in three forms:
    report()             eager launches, one host read
    report(graph=True)   the density map is one hipGraph replay (captured by the warm-up call); the image case has no map and is
                         listed for completeness
    the host loop        net(y) / sample_y / log_py -> .cpu() -> report.colorize_host / scatter_host / image_grid_host: the numpy
                         restatements, which draw the same pixels
The parent commit has no such path, so no ratio is fixed in advance: the file records the columns."""
import argparse
import importlib
import os
import statistics
import sys
import time
import warnings
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ms(torch, fn, repeats):
    fn()                                                     # warm-up: allocations, first launches, the capture
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--image-layers', type=int, default=2)
    ap.add_argument('--out', default=os.path.join('profiles', 'r15_report.txt'))
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module('normalizing-flows-pytorch_amd')
    train = importlib.import_module('normalizing-flows-pytorch_amd.train')
    nfdata = importlib.import_module('normalizing-flows-pytorch_amd.data')
    R = importlib.import_module('normalizing-flows-pytorch_amd.report')
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def f(v):
        return '%9.2f (%.2f .. %.2f)' % tuple(v)
    say('FlowTrainer.report against the host loop, %s: milliseconds per report, median of %d (min .. max)' % (torch.cuda.get_device_name(0), a.repeats))

    # ---- 2-D ---------------------------------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    np.random.seed(0)
    net = pkg.Glow((2, ), '2d', NS(layers=a.layers)).to(dev)
    y = nfdata.sample('moons', 1024, 0).to(dev)
    tr = train.FlowTrainer(net)
    for _ in range(4):
        tr.train_on_batch(y)
    jet0 = np.tile(R.cmap_table('jet')[0], (1024, 1))
    grid_h = R.grid_host(256)

    def host_2d():
        with torch.no_grad():
            net.eval()
            z, _ = net(y)
            pz = torch.exp(train.standard_normal_logprob(z))
            z, pz = z.cpu().numpy(), pz.cpu().numpy()
            out = {'z_rgb': R.scatter_host(z, R.colorize_host(pz, *R.minmax_host(pz), 'jet'), 512, 2)}
            ys, py = tr.sample_y(1024, (2, ))
            ys, py = ys.cpu().numpy(), py.cpu().numpy()
            out['y_rgb'] = R.scatter_host(ys, R.colorize_host(py, *R.minmax_host(py), 'jet'), 512, 2)
            out['y_data_rgb'] = R.scatter_host(y.cpu().numpy(), jet0, 512, 2)
            py_map = torch.exp(tr.log_py(torch.from_numpy(grid_h).to(dev))).cpu().numpy().reshape(256, 256)
            out['py_map_rgb'] = R.colorize_host(py_map, 0.0, 1.0, 'inferno')
            return out
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        tr.report(y, graph=True)
    captured = tr._report_maps[256].graph is not None and not any('capture' in str(w.message) for w in caught)
    res, ref = tr.report(y), host_2d()
    same = bool(np.array_equal(res['y_data_rgb'], ref['y_data_rgb'])) and bool(np.array_equal(res['z_rgb'], ref['z_rgb']))
    e, g, h = _ms(torch, lambda: tr.report(y), a.repeats), _ms(torch, lambda: tr.report(y, graph=True), a.repeats), _ms(torch, host_2d, a.repeats)
    say('2-D: Glow layers = %d, n = 1024, canvas 512, radius 2, map 256 x 256' % a.layers)
    say('  report(), eager launches        %s' % f(e))
    say('  report(graph=True)              %s   map captured: %s' % (f(g), captured))
    say('  host loop (numpy restatements)  %s   host / eager = %.2f   host / graph = %.2f   data and z panels equal: %s'
        % (f(h), h[0] / e[0], h[0] / g[0], same))

    # ---- images ------------------------------------------------------------------------------------------------------------------------
    torch.manual_seed(1)
    inet = pkg.Glow((3, 32, 32), 'image', NS(layers=a.image_layers)).to(dev)
    yi = torch.rand(64, 3, 32, 32, device=dev)
    ti = train.FlowTrainer(inet)
    for _ in range(4):
        ti.train_on_batch(yi)

    def host_img():
        with torch.no_grad():
            out = {'data_grid': R.image_grid_host(yi.cpu().numpy())}
            ys, _ = ti.sample_y(64, (3, 32, 32))
            out['sample_grid'] = R.image_grid_host(ys.cpu().numpy()[:64])
            return out
    same = bool(np.array_equal(ti.report(yi)['data_grid'], host_img()['data_grid']))
    e, g, h = _ms(torch, lambda: ti.report(yi), a.repeats), _ms(torch, lambda: ti.report(yi, graph=True), a.repeats), _ms(torch, host_img, a.repeats)
    say('images: Glow on (3, 32, 32), layers = %d, n = 64, two 8 x 8 grids' % a.image_layers)
    say('  report(), eager launches        %s' % f(e))
    say('  report(graph=True)              %s   (no map in this case: the same launches)' % f(g))
    say('  host loop (numpy restatements)  %s   host / eager = %.2f   data grids equal: %s' % (f(h), h[0] / e[0], same))
    say('  persistent-kernel timeouts: %d' % pkg._native.persistent_timeouts())
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)) or '.', exist_ok=True)
        with open(os.path.join(ROOT, a.out), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
