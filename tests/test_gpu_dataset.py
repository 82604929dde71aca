"""
Device-resident data sets on the GPU (csrc/dataset.hip, data.DeviceDataset) against the numpy restatement of the same object
(indices / host_batch, themselves held to the reference loader's rules by tests/test_dataset_host.py): every batch is BIT-equal -- the
gather moves values and divides by 255 exactly as numpy does -- across slices, load paths, pads, the epoch boundary, two ranks, the
longest cycle walks and a step counter beyond 2^32; bad arguments launch nothing; a FlowTrainer captures the gather in its hipGraph
and the replays walk through the epochs.  Needs a real MI355X.
"""
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _data(pkg):
    return importlib.import_module(pkg.__name__ + '.data')


def _check_step(ds):
    """one next() of ``ds`` against the host, at whatever step the device counter holds"""
    step = int(ds.step.item())
    ds.out.fill_(7.0)                                        # an unwritten pad ring or tail would keep the 7
    ds.last_indices.fill_(-1)
    out = ds.next()
    torch.cuda.synchronize()
    assert int(ds.step.item()) == step + 1
    assert np.array_equal(ds.last_indices.cpu().numpy(), ds.indices(step))
    want = ds.host_batch(step)
    assert out.shape == want.shape == (ds.batch, ) + ds.dims
    assert torch.equal(out.cpu(), want), 'step %d: %d elements differ' % (step, int((out.cpu() != want).sum()))
    return ds.indices(step)


@pytest.mark.parametrize('shape,batch,pad', [((37, 5, 7, 3), 8, 0), ((300, 32, 32, 3), 64, 0), ((300, 28, 28), 64, 2), ((64, 4, 4, 1), 8, 1),
                                              ((37, 5, 7, 3), 8, 3), ((600, 8, 8, 3), 512, 0), ((1100, 7, 8, 3), 1024, 1)])   # (512, 1024: two slices, one slice per sample)
def test_image_batches_are_bit_equal(pkg, shape, batch, pad):
    D = _data(pkg)
    rng = np.random.default_rng(5)
    n_bytes = int(np.prod(shape))
    arr = (rng.permutation(n_bytes) % 256).astype(np.uint8).reshape(shape)          # every byte value, evenly
    ds = D.DeviceDataset(arr, batch, pad=pad, seed=3, device=DEV)
    seen = np.concatenate([_check_step(ds) for _ in range(min(ds.steps_per_epoch, 4))])
    if shape[0] == 37:                # all 256 byte values went through the division: v * (1 / 255.f) differs from v / 255.f for 126 of them
        assert len(np.unique(arr[seen])) == 256


def test_image_identity_order(pkg):
    D = _data(pkg)
    arr = np.random.default_rng(0).integers(0, 256, size=(40, 6, 6, 2), dtype=np.uint8)
    ds = D.DeviceDataset(arr, 8, shuffle=False, device=DEV)
    for k in range(ds.steps_per_epoch + 1):
        assert np.array_equal(_check_step(ds), np.arange(8) + 8 * (k % ds.steps_per_epoch))


@pytest.mark.parametrize('d', [2, 3, 5])
@pytest.mark.parametrize('world', [1, 2])
def test_rows_walk_over_the_epoch_boundary(pkg, d, world):
    D = _data(pkg)
    rows = np.random.default_rng(d).normal(size=(1000, d)).astype(np.float32)
    sets = [D.DeviceDataset(rows, 96, seed=8, device=DEV, rank=r, world=world) for r in range(world)]
    E = sets[0].steps_per_epoch
    assert E == 999 // (96 * world)
    for k in range(E + 2):
        got = np.concatenate([_check_step(s) for s in sets])
        assert len(np.unique(got)) == 96 * world             # the ranks of one step hold disjoint samples


@pytest.mark.parametrize('n', [4097, 65537])
def test_sizes_with_the_longest_walks(pkg, n):
    D = _data(pkg)
    rows = np.arange(n * 2, dtype=np.float32).reshape(n, 2)
    _check_step(D.DeviceDataset(rows, 512, seed=1, device=DEV))
    img = (np.arange(n * 8) % 251).astype(np.uint8).reshape(n, 2, 2, 2)
    _check_step(D.DeviceDataset(img, 512, seed=1, device=DEV))


def test_step_beyond_32_bits(pkg):
    D = _data(pkg)
    rows = np.random.default_rng(1).normal(size=(1000, 3)).astype(np.float32)
    ds = D.DeviceDataset(rows, 96, seed=2, device=DEV)
    ds.step.fill_((1 << 33) + 5)
    _check_step(ds)                                          # E = 10: a 64-bit division of the step
    one = D.DeviceDataset(rows, 512, seed=2, device=DEV)     # E = 1: the epoch itself is 2^33 + 5
    assert one.steps_per_epoch == 1
    one.step.fill_((1 << 33) + 5)
    idx = _check_step(one)
    assert not np.array_equal(idx, one.indices(5))           # the epoch's high word is part of the counter
    img = np.random.default_rng(2).integers(0, 256, size=(100, 4, 4, 3), dtype=np.uint8)
    di = D.DeviceDataset(img, 16, seed=2, device=DEV)
    di.step.fill_((1 << 33) + 5)
    _check_step(di)


def test_bad_arguments_launch_nothing(pkg):
    N = pkg._native
    lib = N.load()
    data8 = torch.zeros((100, 4, 4, 3), dtype=torch.uint8, device=DEV)
    dataf = torch.zeros((100, 2), dtype=torch.float32, device=DEV)
    out = torch.full((8, 3, 4, 4), 7.0, device=DEV)
    idx = torch.full((8, ), -1, dtype=torch.int64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)

    def u8(data=data8.data_ptr(), o=out.data_ptr(), N_=100, H=4, W=4, C=3, pad=0, B=8, stride=8, offset=0, E=12):
        return lib.nf_dataset_gather_u8(data, o, N_, H, W, C, pad, B, stride, offset, E, 1, 1, step.data_ptr(), idx.data_ptr(), N.stream())

    def f32(data=dataf.data_ptr(), o=out.data_ptr(), N_=100, D_=2, B=8, stride=8, offset=0, E=12):
        return lib.nf_dataset_gather_f32(data, o, N_, D_, B, stride, offset, E, 1, 1, step.data_ptr(), idx.data_ptr(), N.stream())
    for kw in (dict(data=None), dict(o=None), dict(N_=0), dict(N_=1 << 31), dict(B=0), dict(E=0), dict(E=13), dict(stride=16, offset=9, E=6),
               dict(offset=-1)):
        assert u8(**kw) == 10001, kw                         # NF_E_BADARG
        assert f32(**kw) == 10001, kw
    for kw in (dict(pad=-1), dict(C=0)):
        assert u8(**kw) == 10001, kw
    assert f32(D_=0) == 10001
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((idx == -1).all())      # refused on the host: nothing was launched
    with pytest.raises(ValueError):
        _data(pkg).DeviceDataset(np.zeros((96, 2), dtype=np.float32), 96, device=DEV)


def _train_from(pkg, net, ds, calls):
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    trainer = nftrain.FlowTrainer(net, graph=True, warmup=2, sampler=ds)
    losses = []
    for _ in range(calls):
        z, loss = trainer.train_on_batch()
        torch.cuda.synchronize()
        step = int(ds.step.item()) - 1                       # the step whose batch this call trained on
        assert torch.equal(ds.out.cpu(), ds.host_batch(step)), 'batch of step %d' % step
        assert np.array_equal(ds.last_indices.cpu().numpy(), ds.indices(step))
        losses.append(float(loss))
    assert trainer._g_fb is not None
    assert int(ds.step.item()) == calls + 1                  # the calls + the capture's extra step
    assert all(np.isfinite(losses))
    return z


def test_trainer_gathers_rows_inside_the_graph(pkg):
    D = _data(pkg)
    torch.manual_seed(0)
    net = pkg.PlanarFlow((3, ), '2d', NS(layers=2)).to(DEV)
    ds = D.DeviceDataset.toy('swiss', 256, seed=1, n=2000, device=DEV)
    E = ds.steps_per_epoch
    assert E == 7 and ds.dims == (3, ) and ds.dtype == '3d'
    z = _train_from(pkg, net, ds, E + 3)                     # the replays cross into the second pass
    assert z.shape == (256, 3)


def test_trainer_gathers_images_inside_the_graph(pkg):
    D = _data(pkg)
    torch.manual_seed(0)
    img = np.random.default_rng(4).integers(0, 256, size=(100, 4, 4), dtype=np.uint8)
    ds = D.DeviceDataset(img, 16, pad=2, seed=1, device=DEV)
    assert ds.dims == (1, 8, 8) and ds.steps_per_epoch == 6
    net = pkg.Glow(ds.dims, 'image', NS(layers=1, mixtures=None)).to(DEV)
    z = _train_from(pkg, net, ds, ds.steps_per_epoch + 3)
    assert z.shape == (16, 1, 8, 8)
