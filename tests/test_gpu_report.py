"""
FlowTrainer.report on the device (csrc/report.hip, report.py): every kernel bit for bit against its numpy restatement at the smallest
shapes where it can still go wrong (one element, odd sizes, more than one workgroup, more than one grid-stride pass where that is
cheap), then the method end to end on a 2-D, a 3-D and an image model, and between replays of a captured training step.
Needs a real MI355X.
"""
import importlib
import warnings
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def R(pkg):
    pkg._native.load()
    return importlib.import_module(pkg.__name__ + '.report')


def _close(got, want):
    """the project's 1e-5: rtol 1e-5 with an absolute floor of 1e-5 of the largest magnitude (as __graft_entry__.smoke compares)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.allclose(got, want, rtol=1e-5, atol=1e-5 * max(1.0, float(np.abs(want).max())))


@pytest.mark.parametrize('map_size', [1, 37, 256])
def test_grid(R, map_size):
    got = R.grid(map_size, DEV)
    assert got.shape == (map_size * map_size, 2) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), torch.from_numpy(R.grid_host(map_size)))


def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=n).astype(np.float32) * 3.0
    if n >= 1000:
        v[rng.choice(n, 40, replace=False)] = np.repeat(np.array([np.nan, np.inf, -np.inf, 1e30], dtype=np.float32), 10)
    return v


@pytest.mark.parametrize('n', [1, 1000, 70001])
def test_minmax(R, n):
    v = _mixed(n, n)
    got = R.minmax(torch.from_numpy(v).to(DEV))
    assert got.dtype == torch.float64 and tuple(got.cpu().tolist()) == R.minmax_host(v)
    if n >= 1000:
        assert got.cpu().tolist()[1] == float(np.float32(1e30))              # the infinities and NaNs were passed over


def test_minmax_without_a_finite_value(R):
    v = np.array([np.nan] * 300 + [np.inf, -np.inf], dtype=np.float32)
    assert R.minmax(torch.from_numpy(v).to(DEV)).cpu().tolist() == [0.0, 1.0]
    assert R.minmax(torch.full((1, ), float('nan'), device=DEV)).cpu().tolist() == [0.0, 1.0]


@pytest.mark.parametrize('n', [1000, 65537])
@pytest.mark.parametrize('cmap', ['inferno', 'jet'])
def test_colorize(R, n, cmap):
    rng = np.random.default_rng(n)
    lin = rng.uniform(-0.2, 1.3, n).astype(np.float32)
    lin[:257] = (np.arange(257) / 256.0).astype(np.float32)                 # every bin edge
    lin[300:304] = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)
    logv = rng.uniform(-12.0, 0.5, n).astype(np.float32)
    logv[300:304] = np.array([np.nan, np.inf, -np.inf, 0.0], dtype=np.float32)
    for v, is_log in ((lin, False), (logv, True)):
        dv = torch.from_numpy(v).to(DEV)
        with np.errstate(over='ignore'):
            want_p = np.exp(v.astype(np.float64)).astype(np.float32) if is_log else v
        for dev_range in (False, True):
            p = torch.empty(n, dtype=torch.float32, device=DEV)
            if dev_range:
                rd = R.minmax(torch.from_numpy(want_p).to(DEV))
                lo, hi = rd.cpu().tolist()
                assert (lo, hi) == R.minmax_host(want_p)
                rgb = R.colorize(dv, cmap=cmap, is_log=is_log, range_dev=rd, p_out=p)
            else:
                lo, hi = (0.0, 1.0) if not is_log else (0.1, 0.7)
                rgb = R.colorize(dv, lo, hi, cmap=cmap, is_log=is_log, p_out=p)
            p_h, rgb_h = p.cpu().numpy(), rgb.cpu().numpy()
            assert rgb_h.shape == (n, 3) and rgb_h.dtype == np.uint8
            fin = np.isfinite(want_p)
            assert np.array_equal(np.isnan(p_h), np.isnan(want_p)) and np.array_equal(p_h[~fin & ~np.isnan(want_p)], want_p[~fin & ~np.isnan(want_p)])
            assert np.all(np.abs(p_h[fin].astype(np.float64) - want_p[fin]) <= 1e-6 * np.abs(want_p[fin].astype(np.float64)))
            if not is_log:
                assert np.array_equal(p_h[fin], want_p[fin])
            assert np.array_equal(rgb_h, R.colorize_host(p_h, lo, hi, cmap)), (is_log, dev_range)
    # p_out alone, in place
    dv = torch.from_numpy(logv).to(DEV)
    want = R.colorize(dv.clone(), is_log=True, p_out=torch.empty(n, dtype=torch.float32, device=DEV), rgb=False)
    assert R.colorize(dv, is_log=True, p_out=dv, rgb=False) is dv and torch.equal(torch.nan_to_num(dv), torch.nan_to_num(want))


def _cloud(D, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.2, 1.2, (300, D)).astype(np.float32)
    pts[100:130] = pts[0:30]                                                # thirty pairs on shared pixels (and at equal depth)
    pts[200:210] = pts[50:60] + np.float32(1e-4)                            # ten more that mostly share a pixel without being equal
    pts[290, 0], pts[291, 1], pts[292, D - 1] = np.nan, np.inf, -np.inf
    pts[293] = 1e30
    pts[294, 0] = -1.0
    pts[295, 0] = 1.0
    return pts, rng.integers(0, 256, (300, 3)).astype(np.uint8)


@pytest.mark.parametrize('D', [2, 3])
@pytest.mark.parametrize('radius', [0, 2])
def test_scatter(R, D, radius):
    pts, cols = _cloud(D, 10 * D + radius)
    view = R.view_matrix() if D == 3 else None
    want = R.scatter_host(pts, cols, 64, radius, view)
    a = R.scatter(torch.from_numpy(pts).to(DEV), torch.from_numpy(cols).to(DEV), 64, radius, view)
    b = R.scatter(torch.from_numpy(pts).to(DEV), torch.from_numpy(cols).to(DEV), 64, radius, view)
    assert a.shape == (64, 64, 3) and a.dtype == torch.uint8
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), want)
    assert 0 < int((want != 255).any(axis=2).sum()) < 64 * 64


@pytest.mark.parametrize('D', [2, 3])
def test_scatter_edge_cases(R, D):
    none = R.scatter(torch.empty((0, D), device=DEV), torch.empty((0, 3), dtype=torch.uint8, device=DEV), 16, 2)
    assert none.shape == (16, 16, 3) and bool((none == 255).all())
    pts = np.array([[0.3, -0.2, 0.1][:D], [0.0, 0.0, 0.0][:D], [1.0, 0.0, 0.0][:D]], dtype=np.float32)
    cols = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.uint8)
    view = R.view_matrix() if D == 3 else None
    for radius in (0, 1):
        got = R.scatter(torch.from_numpy(pts).to(DEV), torch.from_numpy(cols).to(DEV), 1, radius, view)
        assert got.shape == (1, 1, 3) and np.array_equal(got.cpu().numpy(), R.scatter_host(pts, cols, 1, radius, view))


@pytest.mark.parametrize('shape', [(1, 8, 8), (3, 8, 8), (3, 6, 10)])
def test_image_grid(R, shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.uniform(-0.3, 1.3, (64, ) + shape).astype(np.float32)
    x[0, 0, 0, :4] = np.array([np.nan, 0.999, 1.0, -0.0], dtype=np.float32)
    dx = torch.from_numpy(x).to(DEV)
    for n in (1, 5, 10, 64):
        for nrow in (8, 3):
            got = R.image_grid(dx[:n], nrow=nrow)
            want = R.image_grid_host(x[:n], nrow=nrow)
            assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (n, nrow)
            assert np.array_equal(got.cpu().numpy(), want), (n, nrow)
    got = R.image_grid(dx[:5], nrow=2, padding=0, pad_value=0.25)
    assert np.array_equal(got.cpu().numpy(), R.image_grid_host(x[:5], nrow=2, padding=0, pad_value=0.25))


def _trained(pkg, net, y, steps=2, **kw):
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    tr = nftrain.FlowTrainer(net, **kw)
    for _ in range(steps):
        tr.train_on_batch(y)
    return tr


KEYS_2D = {'z', 'pz', 'y_sample', 'py_sample', 'z_rgb', 'y_rgb', 'y_data_rgb', 'py_map', 'py_map_rgb'}


def test_report_2d_end_to_end(pkg, R):
    nfdata = importlib.import_module(pkg.__name__ + '.data')
    torch.manual_seed(0)
    np.random.seed(0)
    net = pkg.Glow((2, ), '2d', NS(layers=2)).to(DEV)
    y = nfdata.sample('moons', 256, 100).to(DEV)
    tr = _trained(pkg, net, y)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    res = tr.report(y)
    assert set(res) == KEYS_2D and not net.training
    assert all(isinstance(v, np.ndarray) for v in res.values())
    assert res['z'].shape == (256, 2) and res['pz'].shape == (256, ) and res['y_sample'].shape == (256, 2) and res['py_sample'].shape == (256, )
    assert res['py_map'].shape == (256, 256) and res['py_map'].dtype == np.float32 and res['py_map_rgb'].shape == (256, 256, 3)
    for k in ('z_rgb', 'y_rgb', 'y_data_rgb'):
        assert res[k].shape == (512, 512, 3) and res[k].dtype == np.uint8
    # the map against log_py on the reference's grid
    want = torch.exp(tr.log_py(torch.from_numpy(R.grid_host(256)).to(DEV))).cpu().numpy().reshape(256, 256)
    assert _close(res['py_map'], want) and float(res['py_map'].max()) > 0.0
    assert np.array_equal(res['py_map_rgb'], R.colorize_host(res['py_map'], 0.0, 1.0, 'inferno'))
    # z and pz against the model, the panels against the host rasteriser on the RETURNED arrays
    z, _ = net(y)
    assert _close(res['z'], z.detach().cpu().numpy())
    assert _close(res['pz'], np.exp(-0.5 * (res['z'].astype(np.float64) ** 2).sum(1) - np.log(2.0 * np.pi)))
    assert np.array_equal(res['z_rgb'], R.scatter_host(res['z'], R.colorize_host(res['pz'], *R.minmax_host(res['pz']), 'jet'), 512, 2))
    assert np.array_equal(res['y_rgb'], R.scatter_host(res['y_sample'], R.colorize_host(res['py_sample'], *R.minmax_host(res['py_sample']), 'jet'),
                                                       512, 2))
    assert np.array_equal(res['y_data_rgb'], R.scatter_host(y.cpu().numpy(), np.tile(R.cmap_table('jet')[0], (256, 1)), 512, 2))
    # a smaller request: n_samples, canvas, radius, map_size and the generator are honoured
    g = torch.Generator(device=DEV).manual_seed(5)
    small = tr.report(y[:7], n_samples=9, generator=g, map_size=37, canvas=33, radius=0)
    g2 = torch.Generator(device=DEV).manual_seed(5)
    again = tr.report(y[:7], n_samples=9, generator=g2, map_size=37, canvas=33, radius=0)
    assert small['y_sample'].shape == (9, 2) and small['z'].shape == (7, 2) and small['z_rgb'].shape == (33, 33, 3) and small['py_map'].shape == (37, 37)
    assert all(np.array_equal(small[k], again[k], equal_nan=k in ('pz', 'py_sample')) for k in small)
    # the captured map: same numbers, one graph object for every later call
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        r1 = tr.report(y, graph=True)
        graph = tr._report_maps[256].graph
        assert graph is not None
        r2 = tr.report(y, graph=True)
    assert tr._report_maps[256].graph is graph
    assert _close(r1['py_map'], res['py_map']) and np.array_equal(r1['py_map'], r2['py_map'])
    assert np.array_equal(r1['py_map_rgb'], R.colorize_host(r1['py_map'], 0.0, 1.0, 'inferno'))
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert pkg._native.persistent_timeouts() == 0


def test_report_3d(pkg, R):
    nfdata = importlib.import_module(pkg.__name__ + '.data')
    torch.manual_seed(1)
    np.random.seed(1)
    net = pkg.MAF((3, ), '2d', NS(layers=2)).to(DEV)
    y = nfdata.sample('swiss', 256, 7).to(DEV)
    tr = _trained(pkg, net, y)
    res = tr.report(y, canvas=128)
    assert set(res) == KEYS_2D - {'py_map', 'py_map_rgb'}
    assert res['z'].shape == (256, 3) and res['y_sample'].shape == (256, 3) and res['z_rgb'].shape == (128, 128, 3)
    V = R.view_matrix()
    assert np.array_equal(res['z_rgb'], R.scatter_host(res['z'], R.colorize_host(res['pz'], *R.minmax_host(res['pz']), 'jet'), 128, 2, V))
    assert np.array_equal(res['y_rgb'], R.scatter_host(res['y_sample'], R.colorize_host(res['py_sample'], *R.minmax_host(res['py_sample']), 'jet'),
                                                       128, 2, V))
    assert np.array_equal(res['y_data_rgb'], R.scatter_host(y.cpu().numpy(), np.tile(R.cmap_table('jet')[0], (256, 1)), 128, 2, V))
    assert int((res['y_data_rgb'] != 255).any(axis=2).sum()) > 100
    assert pkg._native.persistent_timeouts() == 0


def test_report_images(pkg, R):
    torch.manual_seed(2)
    net = pkg.Glow((3, 8, 8), 'image', NS(layers=1)).to(DEV)
    y = torch.rand(4, 3, 8, 8, device=DEV)
    tr = _trained(pkg, net, y)
    res = tr.report(y)
    assert set(res) == {'data_grid', 'sample_grid', 'y_sample'}
    assert res['y_sample'].shape == (64, 3, 8, 8) and res['data_grid'].shape == (12, 42, 3) and res['sample_grid'].shape == (82, 82, 3)
    assert np.array_equal(res['data_grid'], R.image_grid_host(y.cpu().numpy()))
    assert np.array_equal(res['sample_grid'], R.image_grid_host(res['y_sample']))
    assert res['data_grid'].dtype == np.uint8 and not net.training
    assert pkg._native.persistent_timeouts() == 0


def test_report_between_graph_replays_changes_nothing(pkg):
    """mirrors test_evaluation_between_graph_replays_changes_nothing: trainer A makes six captured calls, trainer B four, a report with the
    captured map, and two more.  B keeps its training graph and ends on A's parameters and running statistics, bit for bit."""
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    nfdata = importlib.import_module(pkg.__name__ + '.data')
    N = pkg._native
    N.load()
    was = N.deterministic()
    N.deterministic(True)
    try:
        def build():
            torch.manual_seed(0)
            np.random.seed(0)
            return nftrain.FlowTrainer(pkg.Glow((2, ), '2d', NS(layers=2)).to(DEV), graph=True, warmup=2)
        ys = [nfdata.sample('moons', 256, 100 + i).to(DEV) for i in range(6)]
        a, b = build(), build()
        for y in ys:
            a.train_on_batch(y)
        for y in ys[:4]:
            b.train_on_batch(y)
        graph = b._g_fb
        assert graph is not None
        res = b.report(ys[0], graph=True, map_size=64, canvas=64)
        assert b._report_maps[64].graph is not None and not b.net.training and np.isfinite(res['py_map']).all()
        for y in ys[4:]:
            b.train_on_batch(y)
        torch.cuda.synchronize()
        assert b.net.training and all(m.training for m in b.net.modules())
        assert b._g_fb is graph and a._g_fb is not None
        assert int(a.optim.step_count) == int(b.optim.step_count) == 7
        assert torch.equal(a.bucket.flat_params, b.bucket.flat_params)
        for (k, u), (_, v) in zip(a.net.state_dict().items(), b.net.state_dict().items()):
            assert torch.equal(u, v), k
        assert N.deterministic_timeouts() == 0 and N.persistent_timeouts() == 0
    finally:
        N.deterministic(was)
