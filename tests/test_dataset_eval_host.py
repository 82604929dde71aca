"""
Host-side rules of the dequantised batches and of the sweep schedule of data.DeviceDataset (numpy only, no GPU): the value construction
((v * 2^15 + 15 noise bits) + 0.5) * 2^-23, what the noise is keyed by, its quality, the schedule that serves every sample exactly once,
and the refusals.  tests/test_gpu_dataset_eval.py holds the kernels to these same functions bit for bit.
"""
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch


def _data(pkg):
    return importlib.import_module(pkg.__name__ + '.data')


def _every_byte(shape, seed=5):
    n_bytes = int(np.prod(shape))
    return (np.random.default_rng(seed).permutation(n_bytes) % 256).astype(np.uint8).reshape(shape)


@pytest.mark.parametrize('pad', [0, 3])
def test_dequantised_host_batch_values(pkg, pad):
    D = _data(pkg)
    arr = _every_byte((37, 5, 7, 3))
    ds = D.DeviceDataset(arr, 8, pad=pad, seed=3, device=None, dequantize=True)
    seen = []
    for step in range(ds.steps_per_epoch + 1):                          # over the epoch boundary
        x = ds.host_batch(step).numpy()
        assert x.dtype == np.float32 and x.shape == (8, 3, 5 + 2 * pad, 7 + 2 * pad)
        v = np.transpose(arr[ds.indices(step)], (0, 3, 1, 2))
        inner = x[:, :, pad:pad + 5, pad:pad + 7]
        assert (inner > 0).all() and (inner < 1).all()
        assert np.array_equal(np.floor(inner.astype(np.float64) * 256.0), v)
        q = inner.astype(np.float64) * 2.0 ** 23 - 0.5
        assert np.array_equal(q, np.round(q)) and (q >= 0).all() and (q < 2 ** 23).all()
        ring = x.copy()
        ring[:, :, pad:pad + 5, pad:pad + 7] = 0
        assert not ring.any()                                           # the pad ring: exact zeros
        seen.append(v)
    assert len(np.unique(np.concatenate(seen))) == 256


def test_noise_keying(pkg):
    D = _data(pkg)
    arr = _every_byte((37, 5, 7, 3))
    a = D.DeviceDataset(arr, 8, seed=3, device=None, dequantize=True)
    b = D.DeviceDataset(arr, 8, seed=3, device=None, dequantize=True)
    c = D.DeviceDataset(arr, 8, seed=4, device=None, dequantize=True, shuffle=False)
    a0 = D.DeviceDataset(arr, 8, seed=3, device=None, dequantize=True, shuffle=False)
    assert torch.equal(a.host_batch(2), b.host_batch(2))
    assert not torch.equal(a0.host_batch(0), c.host_batch(0))           # identity order: the same samples, another seed
    idx = np.arange(8)
    w = D.dequant_words(3, 2, idx, 105)
    assert w.dtype == np.uint32 and w.shape == (8, 105)
    assert np.array_equal(w, D.dequant_words(3, 2, idx, 105))
    for other in (D.dequant_words(3, 3, idx, 105), D.dequant_words(4, 2, idx, 105), D.dequant_words(3, 2 + (1 << 32), idx, 105),
                  D.dequant_words(3 + (1 << 32), 2, idx, 105), D.dequant_words(3, 2, idx + 8, 105)):
        assert (other != w).mean() > 0.99                               # 32-bit words: equal by chance once in 2^32
    assert np.array_equal(D.dequant_words(3, 2, idx, 7), w[:, :7])      # a word belongs to its byte, whatever the sample size
    # the same sample served in two epochs gets different noise
    e = a0.steps_per_epoch
    assert np.array_equal(a0.indices(1), a0.indices(1 + e))
    x0, x1 = a0.host_batch(1), a0.host_batch(1 + e)
    assert torch.equal(torch.floor(x0 * 256), torch.floor(x1 * 256)) and (x0 != x1).float().mean() > 0.99


def test_noise_quality(pkg):
    """15-bit noise folded to 64 bins: chi-square within the 99.9 % band of 63 degrees of freedom (two-sided, 0.05 % each side: the
    quantiles 32.455 and 106.583 of the chi-square distribution); lag-1 correlation of neighbouring bytes below 4 / sqrt(n) (a 4-sigma
    bound for independent uniforms)."""
    D = _data(pkg)
    w = D.dequant_words(11, 5, np.arange(80), 3072)                     # 245 760 draws
    u = (w >> np.uint32(17)).astype(np.int64)
    n = u.size
    assert n >= 200000 and u.min() >= 0 and u.max() < 1 << 15
    counts = np.bincount((u >> 9).reshape(-1), minlength=64)            # the top 6 of the 15 bits
    chi2 = float(((counts - n / 64.0) ** 2 / (n / 64.0)).sum())
    assert 32.455 < chi2 < 106.583, chi2
    low = np.bincount((u & 63).reshape(-1), minlength=64)               # and the low 6
    chi2_low = float(((low - n / 64.0) ** 2 / (n / 64.0)).sum())
    assert 32.455 < chi2_low < 106.583, chi2_low
    x = (u.astype(np.float64) + 0.5) / (1 << 15) - 0.5
    a, b = x[:, :-1].reshape(-1), x[:, 1:].reshape(-1)
    r = float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))
    assert abs(r) < 4.0 / np.sqrt(a.size), r


@pytest.mark.parametrize('world', [1, 2])
@pytest.mark.parametrize('batch', [8, 96])
@pytest.mark.parametrize('n', [5, 37, 96, 1000])
@pytest.mark.parametrize('shuffle', [False, True])
def test_sweep_schedule_counts_every_sample_once(pkg, n, batch, world, shuffle):
    D = _data(pkg)
    rows = np.arange(n * 2, dtype=np.float32).reshape(n, 2)
    sets = [D.DeviceDataset(rows, batch, seed=9, shuffle=shuffle, device=None, rank=r, world=world, sweep=True) for r in range(world)]
    S = sets[0].steps_per_epoch
    assert S == -(-n // (batch * world))
    for first in (0, S):                                                # two passes
        served, total = [], 0
        for step in range(first, first + S):
            for ds in sets:
                idx, v = ds.indices(step), ds.valid(step)
                assert idx.shape == (batch, ) and 0 <= v <= batch and idx.min() >= 0 and idx.max() < n
                assert (idx[v:] == n - 1).all()                         # clamped rows
                assert np.array_equal(ds.host_batch(step).numpy(), rows[idx])
                served.append(idx[:v])
                total += v
        served = np.concatenate(served)
        assert total == n and np.array_equal(np.sort(served), np.arange(n))
        if not shuffle:
            assert world > 1 or np.array_equal(served, np.arange(n))
    if shuffle and n >= 37:
        assert not np.array_equal(np.concatenate([sets[0].indices(s) for s in range(S)]),
                                  np.concatenate([sets[0].indices(S + s) for s in range(S)]))   # another order in the next pass


def test_sweep_view_of_a_host_only_set(pkg):
    D = _data(pkg)
    arr = _every_byte((37, 5, 7, 3))
    ds = D.DeviceDataset(arr, 8, pad=1, seed=3, device=None, dequantize=True)
    v = ds.sweep_view()
    assert v.sweep and not v.shuffle and v.dequantize and v.batch == 8 and v.pad == 1 and v.steps_per_epoch == 5 and v.host is ds.host
    assert [v.valid(s) for s in range(5)] == [8, 8, 8, 8, 5]
    w = ds.sweep_view(batch=64, dequantize=False)
    assert w.steps_per_epoch == 1 and w.valid(0) == 37 and not w.dequantize
    assert ds.steps_per_epoch == 4 and ds.valid(3) == 8                 # the loader's schedule is what it was
    with pytest.raises(ValueError):
        D.DeviceDataset(arr, 64, device=None)                           # N <= stride: still refused there


def test_refusals(pkg):
    D = _data(pkg)
    rows = np.zeros((100, 2), dtype=np.float32)
    with pytest.raises(ValueError, match='dequantize'):
        D.DeviceDataset(rows, 8, device=None, dequantize=True)
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    trainer = nftrain.FlowTrainer(pkg.PlanarFlow((2, ), '2d', NS(layers=1)), fused_adam=False)      # on the CPU: the check comes first
    with pytest.raises(ValueError, match='sweep_view'):
        trainer.evaluate(D.DeviceDataset(rows, 8, device=None))
