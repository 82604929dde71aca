"""
FlowTrainer.report without a GPU: the numpy restatements in report.py (the yardsticks of tests/test_gpu_report.py) against the
reference's own expressions (main.py:199-206), matplotlib's colour mapping (common/utils.py:19, :59), hand-written scatter and grid
cases, and the host-side argument checks of the nf_report_* entry points.
"""
import ctypes
import importlib

import numpy as np
import pytest


@pytest.fixture(scope='module')
def R(pkg):
    pkg.build()
    return importlib.import_module(pkg.__name__ + '.report')


@pytest.mark.parametrize('map_size', [256, 37])
def test_grid_is_the_reference_expression(R, map_size):
    ix = (np.arange(map_size) + 0.5) / map_size * 2.0 - 1.0
    iy = (np.arange(map_size) + 0.5) / map_size * -2.0 + 1.0
    ix, iy = np.meshgrid(ix, iy)
    ix = ix.reshape((-1))
    iy = iy.reshape((-1))
    y = np.stack([ix, iy], axis=1).astype(np.float32)           # torch.tensor(y, dtype=torch.float32) rounds the same way
    got = R.grid_host(map_size)
    assert got.dtype == np.float32 and got.shape == (map_size * map_size, 2)
    assert np.array_equal(got, y)


def _values():
    rng = np.random.default_rng(0)
    v = rng.uniform(-0.2, 1.3, 200000).astype(np.float32)
    edges = (np.arange(257) / 256.0).astype(np.float32)
    extra = np.array([0.0, -0.0, 1e-30, 0.99999994, 1.0000001], dtype=np.float32)
    return np.concatenate([v, edges, extra])


def _mpl(name, v, lo, hi):
    matplotlib = pytest.importorskip('matplotlib')
    from matplotlib.colors import Normalize
    return np.asarray(matplotlib.colormaps[name](Normalize(lo, hi)(v), bytes=True))[:, :3]


@pytest.mark.parametrize('name', ['inferno', 'jet'])
def test_colorize_equals_matplotlib_on_the_unit_range(R, name):
    v = _values()
    want = _mpl(name, v, 0.0, 1.0)
    got = R.colorize_host(v, 0.0, 1.0, name)
    assert got.dtype == np.uint8 and got.shape == (v.size, 3)
    assert int((got != want).any(axis=1).sum()) == 0


@pytest.mark.parametrize('name', ['inferno', 'jet'])
@pytest.mark.parametrize('rng', ['minmax', (0.1, 0.7), (-3.0, 2.5)])
def test_colorize_equals_matplotlib_away_from_bin_edges(R, name, rng):
    """matplotlib normalises a float32 array in float32, report.py in double: at a bin edge the two may sit one bin apart.  Values within
    1e-3 of an edge (in units of a bin) are left out -- they must be under 0.5 % of the sample -- and the rest is exact."""
    v = _values()
    lo, hi = R.minmax_host(v) if rng == 'minmax' else rng
    want = _mpl(name, v, lo, hi)
    got = R.colorize_host(v, lo, hi, name)
    x256 = (v.astype(np.float64) - lo) / (hi - lo) * 256.0
    near = np.abs(x256 - np.round(x256)) < 1e-3
    assert near.mean() < 0.005, near.mean()
    assert int((got[~near] != want[~near]).any(axis=1).sum()) == 0


def test_colorize_nan_and_degenerate_range(R):
    v = np.array([np.nan, 0.5, np.inf, -np.inf], dtype=np.float32)
    got = R.colorize_host(v, 0.0, 1.0, 'inferno')
    tab = R.cmap_table('inferno')
    assert np.array_equal(got[0], [0, 0, 0]) and np.array_equal(got[1], tab[128])
    assert np.array_equal(got[2], tab[255]) and np.array_equal(got[3], tab[0])
    assert np.array_equal(R.colorize_host(v[1:2], 0.5, 0.5, 'jet')[0], R.cmap_table('jet')[0])
    assert R.minmax_host(v) == (0.5, 0.5) and R.minmax_host(v[[0, 2, 3]]) == (0.0, 1.0)


@pytest.mark.parametrize('name,first,last', [('inferno', [0, 0, 3], [252, 254, 164]), ('jet', [0, 0, 127], [127, 0, 0])])
def test_cmap_table_is_matplotlibs_and_the_librarys(R, pkg, name, first, last):
    t = R.cmap_table(name)
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert t[0].tolist() == first and t[255].tolist() == last
    buf = (ctypes.c_uint8 * 768)()
    assert pkg._native.load().nf_report_cmap(R.CMAPS[name], ctypes.addressof(buf)) == 0
    assert np.array_equal(np.frombuffer(buf, dtype=np.uint8).reshape(256, 3), t)
    matplotlib = pytest.importorskip('matplotlib')
    assert np.array_equal(t, np.asarray(matplotlib.colormaps[name](np.arange(256), bytes=True))[:, :3])


RED, GREEN = np.array([200, 10, 20], dtype=np.uint8), np.array([5, 180, 40], dtype=np.uint8)


def _painted(img):
    return (img != 255).any(axis=2)


@pytest.mark.parametrize('radius', [0, 1, 2, 3])
def test_scatter_single_point_is_a_disc(R, radius):
    S = 16
    img = R.scatter_host(np.array([[0.01, -0.01]], dtype=np.float32), RED[None], S, radius)
    cx, cy = int(np.floor(1.01 * 0.5 * S)), int(np.floor(1.01 * 0.5 * S))
    yy, xx = np.mgrid[0:S, 0:S]
    disc = (xx - cx) ** 2 + (yy - cy) ** 2 <= radius * radius
    assert (cx, cy) == (8, 8) and np.array_equal(_painted(img), disc)
    assert (img[disc] == RED).all()


def test_scatter_orientation(R):
    """x grows to the right, y grows upwards"""
    img = R.scatter_host(np.array([[0.9, 0.9]], dtype=np.float32), RED[None], 10, 0)
    assert np.argwhere(_painted(img)).tolist() == [[0, 9]]


def test_scatter_2d_later_point_wins(R):
    pts = np.array([[0.1, 0.1], [0.1, 0.1]], dtype=np.float32)
    img = R.scatter_host(pts, np.stack([RED, GREEN]), 8, 1)
    assert int(_painted(img).sum()) == 5 and (img[_painted(img)] == GREEN).all()
    assert (R.scatter_host(pts, np.stack([GREEN, RED]), 8, 0)[3, 4] == RED).all()


def test_scatter_3d_nearer_point_wins_whatever_the_order(R):
    V = R.view_matrix()
    assert V.shape == (3, 3) and np.allclose(V @ V.T, np.eye(3), atol=1e-15)
    near, far = 0.5 * V[2], -0.5 * V[2]                      # both project onto the centre pixel, `near` is closer to the viewer
    for order in ((near, far), (far, near)):
        pts = np.array(order, dtype=np.float32)
        cols = np.stack([RED if p is near else GREEN for p in order])
        img = R.scatter_host(pts, cols, 9, 0, V)
        assert np.argwhere(_painted(img)).tolist() == [[4, 4]] and (img[4, 4] == RED).all()
    same = np.array([near, near], dtype=np.float32)          # a tie in depth goes to the later index
    assert (R.scatter_host(same, np.stack([RED, GREEN]), 9, 0, V)[4, 4] == GREEN).all()


def test_scatter_view_is_the_references_camera(R):
    """elev 10, azim -80: the viewer sits at the direction (cos e cos a, cos e sin a, sin e); z points up on the canvas"""
    V = R.view_matrix(10.0, -80.0)
    e, a = np.radians(10.0), np.radians(-80.0)
    assert np.allclose(V[2], [np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    assert V[1, 2] > 0.9 and V[0, 2] == 0.0 and abs(np.linalg.det(V) - 1.0) < 1e-12


def test_scatter_outside_edge_nan_and_empty(R):
    S = 8
    white = np.full((S, S, 3), 255, dtype=np.uint8)
    assert np.array_equal(R.scatter_host(np.array([[1.5, 0.0]], dtype=np.float32), RED[None], S, 1), white)
    assert np.array_equal(R.scatter_host(np.array([[np.nan, 0.0], [0.0, np.inf]], dtype=np.float32), np.stack([RED, RED]), S, 2), white)
    assert np.array_equal(R.scatter_host(np.zeros((0, 2), dtype=np.float32), np.zeros((0, 3), dtype=np.uint8), S, 2), white)
    assert np.array_equal(R.scatter_host(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.uint8), S, 2, R.view_matrix()), white)
    # x = -1 sits on pixel column 0: the left part of its disc is clipped
    img = R.scatter_host(np.array([[-1.0, 0.0]], dtype=np.float32), RED[None], S, 1)
    assert sorted(np.argwhere(_painted(img)).tolist()) == [[3, 0], [4, 0], [4, 1], [5, 0]]
    # x = 1 is the first pixel PAST the canvas; with radius 1 its disc still reaches column S - 1
    img = R.scatter_host(np.array([[1.0, 0.0]], dtype=np.float32), RED[None], S, 1)
    assert np.argwhere(_painted(img)).tolist() == [[4, 7]]
    assert np.array_equal(R.scatter_host(np.array([[1.0, 0.0]], dtype=np.float32), RED[None], S, 0), white)


def _byte(v):
    return int(np.float32(min(max(v, 0.0), 1.0)) * np.float32(255.0))


@pytest.mark.parametrize('n,shape', [(5, (1, 4, 4)), (10, (1, 4, 4)), (5, (3, 4, 6)), (10, (3, 4, 6))])
def test_image_grid_against_a_hand_written_array(R, n, shape):
    C, H, W = shape
    rng = np.random.default_rng(n * 10 + C)
    x = rng.uniform(-0.3, 1.3, (n, C, H, W)).astype(np.float32)
    x[0, 0, 0, 0], x[0, 0, 0, 1], x[0, 0, 0, 2], x[n - 1, C - 1, H - 1, W - 1] = -0.5, 1.5, 0.999, 0.999
    xmaps = min(8, n)
    ymaps = (n + xmaps - 1) // xmaps
    want = np.full(((H + 2) * ymaps + 2, (W + 2) * xmaps + 2, 3), 255, dtype=np.uint8)
    for k in range(n):
        for i in range(H):
            for j in range(W):
                for c in range(3):
                    want[(k // xmaps) * (H + 2) + 2 + i, (k % xmaps) * (W + 2) + 2 + j, c] = _byte(float(x[k, c if C == 3 else 0, i, j]))
    got = R.image_grid_host(x)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert got[2, 2, 0] == 0 and got[2, 3, 0] == 255 and got[2, 4, 0] == 254         # -0.5, 1.5, 0.999 (254.745 truncates)
    if n == 10:
        assert (got[H + 4:, 2 * (W + 2):] == 255).all()         # the six empty cells of the second row hold pad_value = 1
    assert _byte(0.999) == 254


def test_image_grid_nan_and_pad_value(R):
    x = np.full((1, 1, 2, 2), np.nan, dtype=np.float32)
    got = R.image_grid_host(x, nrow=3, padding=1, pad_value=0.5)
    assert got.shape == (4, 4, 3) and (got[1:3, 1:3] == 0).all() and got[0, 0, 0] == 127 and got[3, 3, 2] == 127


def test_entry_points_refuse_bad_arguments_without_a_gpu(pkg, R):
    lib = pkg._native.load()
    f32 = (ctypes.c_float * 64)()
    u8 = (ctypes.c_uint8 * 768)()
    f64 = (ctypes.c_double * 9)()
    u64 = (ctypes.c_uint64 * 16)()
    pf, pu, pd, pk = (ctypes.addressof(b) for b in (f32, u8, f64, u64))
    BAD = 10001
    assert lib.nf_report_grid(None, 8, None) == BAD
    assert lib.nf_report_grid(pf, 0, None) == BAD
    assert lib.nf_report_minmax(None, 4, pd, None) == BAD
    assert lib.nf_report_minmax(pf, 4, None, None) == BAD
    assert lib.nf_report_minmax(pf, 0, pd, None) == BAD
    assert lib.nf_report_colorize(None, 4, 0, None, 0.0, 1.0, 0, pf, pu, None) == BAD
    assert lib.nf_report_colorize(pf, 4, 0, None, 0.0, 1.0, 0, None, None, None) == BAD
    assert lib.nf_report_colorize(pf, 4, 0, None, 0.0, 1.0, 2, pf, pu, None) == BAD
    assert lib.nf_report_colorize(pf, 4, 0, None, 0.0, 1.0, -1, pf, pu, None) == BAD
    assert lib.nf_report_colorize(pf, 4, 0, None, float('nan'), 1.0, 0, pf, pu, None) == BAD
    assert lib.nf_report_cmap(2, pu) == BAD and lib.nf_report_cmap(0, None) == BAD
    assert lib.nf_report_scatter(None, pu, 4, 2, None, 4, 1, pk, pu, None) == BAD
    assert lib.nf_report_scatter(pf, None, 4, 2, None, 4, 1, pk, pu, None) == BAD
    assert lib.nf_report_scatter(pf, pu, 4, 2, None, 4, 1, None, pu, None) == BAD
    assert lib.nf_report_scatter(pf, pu, 4, 2, None, 4, 1, pk, None, None) == BAD
    assert lib.nf_report_scatter(pf, pu, 4, 3, None, 4, 1, pk, pu, None) == BAD       # 3-D without a view
    assert lib.nf_report_scatter(pf, pu, 4, 4, pd, 4, 1, pk, pu, None) == BAD
    assert lib.nf_report_scatter(pf, pu, 4, 2, None, 0, 1, pk, pu, None) == BAD
    assert lib.nf_report_scatter(pf, pu, 4, 2, None, 4097, 1, pk, pu, None) == BAD
    assert lib.nf_report_scatter(pf, pu, 4, 2, None, 4, 9, pk, pu, None) == BAD
    assert lib.nf_report_scatter(pf, pu, -1, 2, None, 4, 1, pk, pu, None) == BAD
    assert lib.nf_report_image_grid(None, 1, 1, 2, 2, 8, 2, 1.0, pu, None) == BAD
    assert lib.nf_report_image_grid(pf, 1, 1, 2, 2, 8, 2, 1.0, None, None) == BAD
    assert lib.nf_report_image_grid(pf, 1, 2, 2, 2, 8, 2, 1.0, pu, None) == BAD
    assert lib.nf_report_image_grid(pf, 1, 1, 2, 2, 0, 2, 1.0, pu, None) == BAD
    assert lib.nf_report_image_grid(pf, 0, 1, 2, 2, 8, 2, 1.0, pu, None) == BAD
    assert lib.nf_report_image_grid(pf, 1, 1, 2, 2, 8, -1, 1.0, pu, None) == BAD
    with pytest.raises(ValueError):
        R.cmap_table('viridis')
    with pytest.raises(ValueError):
        R.scatter_host(np.zeros((1, 4), dtype=np.float32), np.zeros((1, 3), dtype=np.uint8), 8, 1)
    with pytest.raises(ValueError):
        R.scatter_host(np.zeros((1, 2), dtype=np.float32), np.zeros((1, 3), dtype=np.uint8), 4097, 1)
    with pytest.raises(ValueError):
        R.image_grid_host(np.zeros((1, 2, 4, 4), dtype=np.float32))
