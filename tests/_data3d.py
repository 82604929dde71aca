"""
Distribution-level comparison of two samples of a 3-D toy set (swiss, s_curve), shared by the host test (data.py against
sklearn) and the GPU test (csrc/datagen.hip against data.py).  The statistics are those of tests/test_gpu_datagen.py carried to
three dimensions.  Two INDEPENDENT draws of n = 2^18 points from the same generator (sklearn against sklearn included) sit at 0.43 of
the mean bar, 0.11 of the covariance bar, 0.009 on the quantiles and 0.020 of total variation -- the 12^3 cells hold ~150 points
each, so the histogram distance of two honest samples is sampling noise of that size, and the 2-D tests' 0.01 quantile bar would
sit right at the noise of the wide t cos t / t sin t marginals.
"""
import numpy as np


def assert_same_distribution(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    n = got.shape[0]
    assert got.shape == want.shape == (n, 3)
    se = 4.0 / np.sqrt(n)                                    # ~4 standard errors of a unit-scale statistic
    d_mean = np.abs(got.mean(0) - want.mean(0)).max()
    d_cov = np.abs(np.cov(got.T) - np.cov(want.T)).max()
    qs = np.linspace(0.02, 0.98, 25)
    d_q = max(np.abs(np.quantile(got[:, j], qs) - np.quantile(want[:, j], qs)).max() for j in range(3))
    rng = [[-1.3, 1.3]] * 3
    h1 = np.histogramdd(got, bins=12, range=rng)[0] / n
    h2 = np.histogramdd(want, bins=12, range=rng)[0] / n
    tv = 0.5 * np.abs(h1 - h2).sum()
    print('mean %.3g (bar %.3g)  cov %.3g (bar %.3g)  quantiles %.3g (bar 0.02)  TV %.3g (bar 0.04)' % (d_mean, se, d_cov, 2 * se, d_q, tv))
    assert d_mean < se
    assert d_cov < 2 * se
    assert d_q < 0.02
    assert tv < 0.04
    assert h1.sum() > 0.99 and h2.sum() > 0.99               # (the grid holds the sets: nothing is compared outside it)
