"""
The MADE mask draw on the device (csrc/made_masks.hip, nf_made_draw_masks) against the host rule (conditioners.made_masks_from_degrees,
flows/maf.py:66-85): masks from the degrees the kernel wrote, the bounds of the degrees, reproducibility, the stream offset and the
frequency of the two values at D = 3.  Needs a real MI355X.
"""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N_DRAWS = 1024


def _seed(seed=20240611, offset=0):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _read(pkg, seed, n, D, **kw):
    NF = importlib.import_module(pkg.__name__ + '.functional')
    sets, deg = NF.made_draw_masks(seed, n, D, want_degrees=True, **kw)
    buf = sets[0][0]._base                                  # every set is a view of the one tensor of the call: one copy to the host
    assert buf.shape == (n, pkg._native.header_constant('NF_MADE_MASK_STRIDE'))
    return [[m.numpy() for m in s] for s in NF.made_mask_views(buf.cpu(), D)], deg.cpu().numpy()


@pytest.mark.parametrize('D', [1, 2, 3, 4])
def test_masks_follow_the_reference_rule(pkg, D):
    cond = importlib.import_module(pkg.__name__ + '.conditioners')
    sets, deg = _read(pkg, _seed(), N_DRAWS, D)
    assert deg.shape == (N_DRAWS, 3, 32) and deg.dtype == np.int32
    for d in range(N_DRAWS):
        m_prev = np.arange(D)
        for l in range(3):
            lo = min(int(m_prev.min()), D - 2)
            assert deg[d, l].min() >= lo and deg[d, l].max() <= D - 2, (d, l, lo, deg[d, l])
            m_prev = deg[d, l]
        want = cond.made_masks_from_degrees(D, list(deg[d]))
        for l in range(4):
            assert sets[d][l].dtype == np.float32 and sets[d][l].shape == want[l].shape
            assert np.array_equal(sets[d][l], want[l]), (d, l)
    if D <= 2:                                              # a range of one value: the host draw, whatever its generator's state
        host = cond.made_degrees_to_masks(D, 3, 32, np.random.RandomState(0))
        assert (deg == D - 2).all()
        for d in (0, N_DRAWS - 1):
            for l in range(4):
                assert np.array_equal(sets[d][l], host[l])
    else:
        assert all(len(np.unique(deg[:, l])) == D - 1 for l in range(3))     # every value of the range turns up
    assert pkg._native.persistent_timeouts() == 0


@pytest.mark.parametrize('D', [3, 4])
def test_draws_are_a_function_of_the_seed_words(pkg, D):
    NF = importlib.import_module(pkg.__name__ + '.functional')
    seed = _seed(77, 5)
    a, da = _read(pkg, seed, N_DRAWS, D)
    b, db = _read(pkg, seed, 3, D)                          # another grid, the same words: the same first draws
    assert seed.tolist() == [77, 5]                        # the read-back helper leaves the words alone
    assert np.array_equal(da[:3], db) and all(np.array_equal(x, y) for d in range(3) for x, y in zip(a[d], b[d]))
    c, dc = _read(pkg, seed.clone(), N_DRAWS, D)
    assert np.array_equal(da, dc) and all(np.array_equal(x, y) for d in range(N_DRAWS) for x, y in zip(a[d], c[d]))
    # the offset word moves on by n_draws per launch, on the device; the next launch continues the stream where this one ended
    NF.made_draw_masks(seed, 7, D, advance=True)
    assert seed.tolist() == [77, 12]
    e, de = _read(pkg, seed, 16, D, advance=True)
    assert seed.tolist() == [77, 28]
    assert np.array_equal(de, da[7:23]) and not np.array_equal(de, da[:16])
    other, do = _read(pkg, _seed(78, 5), N_DRAWS, D)
    assert not np.array_equal(do, da)
    assert pkg._native.persistent_timeouts() == 0


def test_both_degrees_are_equally_frequent_at_three_dimensions(pkg):
    """D = 3: every hidden degree is 0 or 1 with probability 1/2 each (the lower bound is 0 unless all 32 units of the layer below drew
    1: probability 2^-32).  The mean of n = 1024 x 3 x 32 = 98 304 such draws has standard deviation 0.5 / sqrt(n); 5 sigma."""
    _, deg = _read(pkg, _seed(4242), N_DRAWS, 3)
    n = deg.size
    assert n == 98304
    mean = float(deg.astype(np.float64).mean())
    sigma = 0.5 / np.sqrt(n)
    print('mean degree %.6f, |mean - 1/2| = %.3g sigma' % (mean, abs(mean - 0.5) / sigma))
    assert abs(mean - 0.5) <= 5.0 * sigma, (mean, sigma)
    assert pkg._native.persistent_timeouts() == 0
