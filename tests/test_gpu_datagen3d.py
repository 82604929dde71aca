"""
The reference's 3-D toy sets (flows/dataset.py:37-50, :92-99) drawn on the device (csrc/datagen.hip, kinds 4 and 5) against the host
restatement in data.py (itself checked against sklearn in tests/test_trainer_host.py): distribution-level agreement at the bars of
tests/_data3d.py, reproducibility, argument checks, and a D = 3 model trained from the sampler inside a hipGraph.  Needs a real MI355X.
"""
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests._data3d import assert_same_distribution

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _data(pkg):
    return importlib.import_module(pkg.__name__ + '.data')


@pytest.mark.parametrize('name', ['swiss', 's_curve'])
def test_device_sampler_3d_matches_host_distribution(pkg, name):
    D = _data(pkg)
    n = 1 << 18
    s = D.DeviceSampler(name, n, (3, ), seed=11, device=DEV)
    got = s.next().cpu().numpy()
    assert got.shape == (n, 3) and np.isfinite(got).all()
    assert_same_distribution(got, D.sample(name, n, 99).numpy())


@pytest.mark.parametrize('name', ['swiss', 's_curve'])
def test_device_sampler_3d_is_reproducible_and_advances(pkg, name):
    D = _data(pkg)
    a = D.DeviceSampler(name, 4096, (3, ), seed=3, device=DEV)
    b = D.DeviceSampler(name, 4096, (3, ), seed=3, device=DEV)
    x0, y0 = a.next().clone(), b.next().clone()
    assert torch.equal(x0, y0)                               # pure function of (seed, step, index)
    x1 = a.next().clone()
    assert not torch.equal(x0, x1)                           # the device-side step moved on
    assert int(a.step.item()) == 2
    c = D.DeviceSampler(name, 4096, (3, ), seed=4, device=DEV)
    assert not torch.equal(c.next(), x0)


def test_wrong_shapes_are_refused(pkg):
    D = _data(pkg)
    for name, dims in (('swiss', (2, )), ('s_curve', (3, 1, 1)), ('swiss', (1, 3))):
        with pytest.raises(ValueError, match='is a 3-D data set'):
            D.DeviceSampler(name, 16, dims, device=DEV)
    with pytest.raises(ValueError, match='moons is a 2-D data set'):
        D.DeviceSampler('moons', 16, (3, ), device=DEV)


def test_c_entry_refuses_a_3d_kind_with_two_values_per_sample(pkg):
    N = pkg._native
    lib = N.load()
    out = torch.full((64, 3), 7.0, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for kind, per in ((4, 2), (5, 2), (4, 4), (0, 3), (6, 3)):
        assert lib.nf_sample_data(kind, out.data_ptr(), 64, per, 1, step.data_ptr(), N.stream()) == 10001      # NF_E_BADARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                          # refused on the host: nothing was launched


def test_trainer_draws_3d_batches_inside_the_graph(pkg):
    D = _data(pkg)
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    torch.manual_seed(0)
    net = pkg.PlanarFlow((3, ), '2d', NS(layers=2)).to(DEV)
    sampler = D.DeviceSampler('swiss', 256, (3, ), seed=1, device=DEV)
    trainer = nftrain.FlowTrainer(net, graph=True, warmup=2, sampler=sampler)
    losses, batches = [], []
    for _ in range(5):
        z, loss = trainer.train_on_batch()
        torch.cuda.synchronize()
        losses.append(float(loss))
        batches.append(sampler.out.clone())
    assert trainer._g_fb is not None
    assert z.shape == (256, 3)
    assert int(sampler.step.item()) == int(trainer.optim.step_count.item()) == 6      # five calls + the capture's extra step
    assert not torch.equal(batches[-1], batches[-2]) and not torch.equal(batches[-2], batches[-3])
    assert all(np.isfinite(losses)) and len(set(losses[-3:])) == 3
