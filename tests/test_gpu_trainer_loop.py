"""
The reference's training loop (main.py:323-340: train, report in eval mode, train on; RMSprop + StepLR; checkpoints) on the captured
step of FlowTrainer.  Everything runs in the ordered mode (tests/test_gpu_deterministic.py), switched on before the capture, so that two
trainers fed the same batches can be compared bit for bit.  Needs a real MI355X.
"""
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = 256


@pytest.fixture
def det_mode(pkg):
    """switches the ordered mode on for the test and puts the previous setting back"""
    N = pkg._native
    N.load()
    was = N.deterministic()
    N.deterministic(True)
    yield N
    N.deterministic(was)


def _trainer(pkg, seed=0, **kw):
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    torch.manual_seed(seed)
    np.random.seed(seed)
    net = pkg.Glow((2, ), '2d', NS(layers=2)).to(DEV)
    return nftrain.FlowTrainer(net, graph=True, warmup=2, **kw)


def _batches(pkg, n):
    nfdata = importlib.import_module(pkg.__name__ + '.data')
    return [nfdata.sample('moons', B, 100 + i).to(DEV) for i in range(n)]


def _flat(tr):
    return tr.bucket.flat_params.detach().clone()


def test_evaluation_between_graph_replays_changes_nothing(pkg, det_mode):
    """trainer A: six calls.  Trainer B: four calls, sample_y and log_py (both leave the model in eval mode), two more calls.  B keeps
    replaying the graph it captured and ends on A's parameters and running statistics, bit for bit."""
    ys = _batches(pkg, 6)
    a, b = _trainer(pkg), _trainer(pkg)
    for y in ys:
        a.train_on_batch(y)
    for y in ys[:4]:
        b.train_on_batch(y)
    graph = b._g_fb
    assert graph is not None
    y_s, p_s = b.sample_y(64, (2, ))
    lp = b.log_py(ys[0])
    assert y_s.shape == (64, 2) and lp.shape == (B, ) and bool(torch.isfinite(lp).all()) and not b.net.training
    for y in ys[4:]:
        z, loss = b.train_on_batch(y)
    torch.cuda.synchronize()
    assert b.net.training and all(m.training for m in b.net.modules())
    assert b._g_fb is graph and a._g_fb is not None
    assert int(a.optim.step_count) == int(b.optim.step_count) == 7
    assert torch.equal(_flat(a), _flat(b))
    for (k, u), (_, v) in zip(a.net.state_dict().items(), b.net.state_dict().items()):
        assert torch.equal(u, v), k
    assert det_mode.deterministic_timeouts() == 0 and det_mode.persistent_timeouts() == 0


def test_rmsprop_steplr_graph_run_and_checkpoint_into_a_captured_step(pkg, det_mode, tmp_path):
    """five calls at warmup = 2 are SIX optimizer steps (the capturing call takes one extra eager step), four of them around the capture
    and in replays: steps 5 and 6 run at 1e-4 * 0.5 ** 2.  The checkpoint then goes into ANOTHER trainer whose step is already
    captured; one more step on the same batch leaves both on the same bits (the loaded schedule restarts from the saved rate, which
    is the rate the first trainer's step 7 uses)."""
    ys = _batches(pkg, 6)
    a = _trainer(pkg, optimizer='rmsprop', decay_steps=2)
    assert type(a.optim).__name__ == 'FlatRMSprop'
    losses = []
    for y in ys[:5]:
        z, loss = a.train_on_batch(y)
        losses.append(float(loss))
    assert a._g_fb is not None
    assert int(a.optim.step_count) == 6 and int(a.optim.sched_pos) == 6
    assert float(a.optim.lr) == float(np.float32(1e-4 * 0.5 ** 2))
    assert all(np.isfinite(losses)) and len(set(losses)) == len(losses)
    f = str(tmp_path / 'ckpt.pth')
    a.save_ckpt(5, f)
    b = _trainer(pkg, seed=1, optimizer='rmsprop', decay_steps=2)
    for y in ys[:3]:
        b.train_on_batch(y + 0.05)
    graph = b._g_fb
    assert graph is not None and not torch.equal(_flat(a), _flat(b))
    assert b.load_ckpt(f) == 5
    assert torch.equal(_flat(a), _flat(b)) and torch.equal(a.optim.square_avg, b.optim.square_avg)
    assert int(b.optim.step_count) == 6 and int(b.optim.sched_pos) == 0
    assert b.current_lr() == a.current_lr() == 1e-4 * 0.5 ** 3
    a.train_on_batch(ys[5])
    b.train_on_batch(ys[5])
    torch.cuda.synchronize()
    assert b._g_fb is graph
    assert float(a.optim.lr) == float(b.optim.lr) == float(np.float32(1e-4 * 0.5 ** 3))
    assert torch.equal(_flat(a), _flat(b))
    assert det_mode.deterministic_timeouts() == 0 and det_mode.persistent_timeouts() == 0
