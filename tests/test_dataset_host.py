"""
Device-resident data sets, the host side (data.dataset_perm, data.DeviceDataset with device=None; csrc/dataset.hip's argument checks):
the epoch permutation is a bijection and looks uniform, the batch schedule is the reference loader's (flows/dataset.py:111-117), the
host restatement of a batch is what dataset.py:116-125 builds.  Runs without a GPU; tests/test_gpu_dataset.py holds the kernels
against these functions.

The chi-square bars are dof + 5 sqrt(2 dof) (five standard deviations of a chi-square variable above its mean), not fitted to the
construction: position x value counts of N x N cells have (N - 1)^2 degrees of freedom, a 16 x 16 binning 225.
"""
import importlib

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def D(pkg):
    return importlib.import_module(pkg.__name__ + '.data')


def _chi2(counts):
    exp = counts.sum() / counts.size
    return float(((counts - exp) ** 2 / exp).sum())


@pytest.mark.parametrize('n', [2, 3, 5, 8, 17, 1000, 4097, 50000, 60000, 65536, 65537])
def test_perm_is_a_bijection(D, n):
    for epoch in (0, 1, 7):
        p = D.dataset_perm(123, epoch, np.arange(n), n)
        assert p.dtype == np.int64 and p.shape == (n, )
        assert np.array_equal(np.sort(p), np.arange(n))


def test_perm_scalar_position_and_range_checks(D):
    p = D.dataset_perm(5, 2, np.arange(100), 100)
    assert int(D.dataset_perm(5, 2, 17, 100)) == p[17]
    with pytest.raises(ValueError):
        D.dataset_perm(0, 0, 100, 100)
    with pytest.raises(ValueError):
        D.dataset_perm(0, 0, 0, 1 << 31)


def test_epochs_and_seeds_give_unrelated_orders(D):
    n = 60000
    a, b = D.dataset_perm(1, 0, np.arange(n), n), D.dataset_perm(1, 1, np.arange(n), n)
    c = D.dataset_perm(2, 0, np.arange(n), n)
    # two independent permutations agree on Poisson(1) positions: P(> 10) < 1e-8
    assert int((a == b).sum()) <= 10
    assert int((a == c).sum()) <= 10
    big = D.dataset_perm(1, (1 << 33) + 1, np.arange(n), n)           # the epoch's high word takes part
    assert int((big == b).sum()) <= 10


@pytest.mark.parametrize('n,bound', [(5, 44), (8, 98), (13, 229)])
def test_position_value_counts_are_uniform(D, n, bound):
    dof = (n - 1) ** 2
    assert bound == round(dof + 5 * np.sqrt(2 * dof))
    counts = np.zeros((n, n))
    vals = D.dataset_perm(0, np.arange(8000)[:, None], np.arange(n)[None, :], n)
    np.add.at(counts, (np.broadcast_to(np.arange(n), vals.shape), vals), 1)
    chi = _chi2(counts)
    print('N = %d: chi2 %.1f (dof %d, bound %d)' % (n, chi, dof, bound))
    assert chi < bound


def test_four_rounds_would_not_pass(D):
    """the bar above tells the shipped 8 rounds from 4 (the construction at 4 rounds is visibly non-uniform at small N)"""
    n, counts = 8, np.zeros((8, 8))
    vals = D.dataset_perm(0, np.arange(8000)[:, None], np.arange(n)[None, :], n, rounds=4)
    np.add.at(counts, (np.broadcast_to(np.arange(n), vals.shape), vals), 1)
    assert _chi2(counts) > 98


def test_coarse_bins_are_uniform_at_1000(D):
    n, counts = 1000, np.zeros((16, 16))
    pos_bin = np.arange(n) * 16 // n
    vals = D.dataset_perm(9, np.arange(400)[:, None], np.arange(n)[None, :], n)
    np.add.at(counts, (np.broadcast_to(pos_bin, vals.shape), vals * 16 // n), 1)
    exp = np.outer(np.bincount(pos_bin), np.bincount(pos_bin)) * 400.0 / n        # bins of 62 and 63 positions
    chi = float(((counts - exp) ** 2 / exp).sum())
    print('N = 1000, 16 x 16 bins: chi2 %.1f (bound %.1f)' % (chi, 225 + 5 * np.sqrt(450)))
    assert chi < 225 + 5 * np.sqrt(450)


def test_lag_one_correlation(D):
    n = 65536
    p = D.dataset_perm(3, 0, np.arange(n), n).astype(np.float64)
    r = np.corrcoef(p[:-1], p[1:])[0, 1]
    print('lag-1 correlation %.5f (bound %.5f)' % (r, 5 / np.sqrt(n)))
    assert abs(r) < 5 / np.sqrt(n)


def _rows(n, d=2):
    return np.arange(n * d, dtype=np.float32).reshape(n, d)


def test_steps_per_epoch_is_the_loaders(D):
    assert D.DeviceDataset(_rows(65536), 1024, device=None).steps_per_epoch == 63          # B | N: the last full batch is dropped too
    assert D.DeviceDataset(_rows(65537), 1024, device=None).steps_per_epoch == 64
    assert D.DeviceDataset(_rows(1000), 96, device=None).steps_per_epoch == 10
    assert D.DeviceDataset(_rows(1000), 96, device=None, rank=1, world=2).steps_per_epoch == 5
    for n, b, w in ((1000, 96, 1), (1000, 100, 2), (37, 8, 1), (65536, 16384, 1)):
        # the loader's own rule (dataset.py:111-117): serve while N > iter + B
        it, steps = 0, 0
        while n > it + w * b:
            it, steps = it + w * b, steps + 1
        assert D.DeviceDataset(_rows(n), b, device=None, rank=0, world=w).steps_per_epoch == steps == (n - 1) // (w * b)


@pytest.mark.parametrize('world', [1, 2])
def test_ranks_and_steps_of_an_epoch_are_disjoint(D, world):
    n, b = 1000, 96
    sets = [D.DeviceDataset(_rows(n), b, seed=4, device=None, rank=r, world=world) for r in range(world)]
    E = sets[0].steps_per_epoch
    assert E == (n - 1) // (world * b)
    for epoch in (0, 1):
        got = np.concatenate([s.indices(epoch * E + k) for k in range(E) for s in sets])
        assert got.min() >= 0 and got.max() < n
        assert len(np.unique(got)) == E * world * b == len(got)
    # step E starts pass 1: the order of (seed, 1) from position 0
    first = np.concatenate([s.indices(E) for s in sets])
    assert np.array_equal(first, D.dataset_perm(4, 1, np.arange(world * b), n))
    assert not np.array_equal(first, np.concatenate([s.indices(0) for s in sets]))


def test_ordered_mode_is_arange(D):
    s = D.DeviceDataset(_rows(1000), 96, shuffle=False, device=None)
    assert np.array_equal(s.indices(0), np.arange(96))
    assert np.array_equal(s.indices(3), np.arange(3 * 96, 4 * 96))
    assert np.array_equal(s.indices(s.steps_per_epoch + 1), np.arange(96, 192))
    t = D.DeviceDataset(_rows(1000), 96, shuffle=False, device=None, rank=1, world=2)
    assert np.array_equal(t.indices(2), np.arange(2 * 192 + 96, 2 * 192 + 192))


def test_too_small_a_set_is_refused(D):
    for n, b, w in ((96, 96, 1), (95, 96, 1), (192, 96, 2)):
        with pytest.raises(ValueError, match='world \\* batch'):
            D.DeviceDataset(_rows(n), b, device=None, rank=0, world=w)
    D.DeviceDataset(_rows(97), 96, device=None)
    with pytest.raises(ValueError):
        D.DeviceDataset(np.zeros((10, 2), dtype=np.float64), 2, device=None)
    with pytest.raises(ValueError):
        D.DeviceDataset(_rows(10), 2, pad=1, device=None)
    with pytest.raises(RuntimeError):
        D.DeviceDataset(_rows(10), 2, device=None).next()


def test_host_batch_is_the_loaders(D):
    rng = np.random.default_rng(0)
    arr = rng.integers(0, 256, size=(37, 5, 7, 3), dtype=np.uint8)
    s = D.DeviceDataset(arr, 8, seed=2, device=None)
    assert s.dims == (3, 5, 7) and s.dtype == 'image'
    for step in (0, 3, 4, 9):
        idx = s.indices(step)
        want = np.transpose(arr[idx].astype('float32') / 255.0, (0, 3, 1, 2))
        got = s.host_batch(step)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    mn = rng.integers(0, 256, size=(50, 28, 28), dtype=np.uint8)
    m = D.DeviceDataset(torch.from_numpy(mn), 16, pad=2, seed=2, device=None)
    assert m.dims == (1, 32, 32)
    got, idx = m.host_batch(1).numpy(), m.indices(1)
    assert got.shape == (16, 1, 32, 32)
    assert np.array_equal(got[:, 0, 2:30, 2:30], mn[idx].astype('float32') / 255.0)
    ring = got.copy()
    ring[:, :, 2:30, 2:30] = 0
    assert not ring.any()
    rows = rng.normal(size=(1000, 3)).astype(np.float32)
    r = D.DeviceDataset(rows, 96, device=None)
    assert r.dims == (3, ) and r.dtype == '3d'
    assert np.array_equal(r.host_batch(11).numpy(), rows[r.indices(11)])
    assert D.DeviceDataset(rows[:, :2].copy(), 96, device=None).dtype == '2d'


def test_toy_and_npz_constructors(D, tmp_path):
    t = D.DeviceDataset.toy('swiss', 256, seed=3, device=None)
    assert t.n == D.N_DATASET_SIZE == 65536 and t.dims == (3, ) and t.dtype == '3d' and t.steps_per_epoch == 255
    assert np.array_equal(t.host, D.GENERATORS['swiss'](65536, np.random.default_rng(3)))
    assert D.DeviceDataset.toy('moons', 1024, device=None).dtype == '2d'
    with pytest.raises(ValueError):
        D.DeviceDataset.toy('cifar', 64, device=None)
    arr = np.random.default_rng(1).integers(0, 256, size=(20, 4, 4, 3), dtype=np.uint8)
    np.savez(tmp_path / 'set.npz', train=arr)
    z = D.DeviceDataset.from_npz(str(tmp_path / 'set.npz'), 'train', 4, pad=1, device=None)
    assert z.dims == (3, 6, 6) and np.array_equal(z.host, arr)


def test_c_entry_points_check_arguments_without_gpu(pkg):
    pkg.build()
    lib = pkg._native.load()
    P = 4096                                              # a non-null pointer that is never dereferenced: the checks come first

    def u8(data=P, out=P, N=100, H=4, W=4, C=3, pad=0, B=8, stride=8, offset=0, E=12):
        return lib.nf_dataset_gather_u8(data, out, N, H, W, C, pad, B, stride, offset, E, 1, 1, None, None, None)

    def f32(data=P, out=P, N=100, D=2, B=8, stride=8, offset=0, E=12):
        return lib.nf_dataset_gather_f32(data, out, N, D, B, stride, offset, E, 1, 1, None, None, None)
    bad = [dict(data=None), dict(out=None), dict(N=0), dict(N=-5), dict(N=1 << 31), dict(B=0), dict(E=0), dict(E=13),
           dict(stride=16, offset=9, E=6), dict(offset=-1)]
    for kw in bad:
        assert u8(**kw) == 10001, kw
        assert f32(**kw) == 10001, kw
    for kw in (dict(pad=-1), dict(C=0), dict(H=0), dict(W=0), dict(W=20000, C=3)):
        assert u8(**kw) == 10001, kw
    assert f32(D=0) == 10001
