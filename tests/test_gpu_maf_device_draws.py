"""
MAF with its MADE masks drawn on the device (MAF.draws = 'device', csrc/made_masks.hip): the training step, the one-launch inverse with a
mask set per pass (nf_maf_step_inv_drawn) and the captured trainer step on 3-D data, each against the host-drawn path fed the SAME hidden
degrees -- read back through functional.made_draw_masks from the same seed words and replayed through np.random.randint.
Needs a real MI355X.
"""
import copy
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import models as om
from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'


class ReplayRng:
    """stands in for np.random: hands out the recorded degree vectors in order and checks the bounds the caller asks for"""

    def __init__(self, degrees):
        self.degrees, self.at = np.asarray(degrees).reshape(-1, 32), 0

    def randint(self, lo, hi, size=None):
        m = self.degrees[self.at]
        self.at += 1
        assert size == 32 and (m >= lo).all() and (m < hi).all(), (lo, hi, size, m)
        return m.astype(np.int64)


def _recorded(pkg, net, n_draws, D):
    """the degrees of the next n_draws draws of ``net``, the seed words untouched"""
    NF = importlib.import_module(pkg.__name__ + '.functional')
    _, deg = NF.made_draw_masks(net.seed.clone(), n_draws, D, want_degrees=True)
    return deg.cpu().numpy()


def _buffers_close(net1, net2, atol, rtol):
    b1, b2 = dict(net1.named_buffers()), dict(net2.named_buffers())
    for name in b2:
        if name != 'seed':                                  # (the stream offset of the device draws: only one of the two moves)
            G.assert_close(b1[name].float(), b2[name].float(), atol, rtol=rtol, what='buffer ' + name)


@pytest.mark.parametrize('D,B,K', [(3, 300, 2), (4, 129, 3), (3, 9, 1)])
def test_training_step_matches_host_draws_of_the_same_degrees(pkg, D, B, K, monkeypatch):
    """three ragged workgroups; one row over a workgroup boundary; fewer rows than a tile (and a single step: the per-step node)"""
    train = importlib.import_module(pkg.__name__ + '.train')
    fused = importlib.import_module(pkg.__name__ + '.fused')
    torch.manual_seed(D * 1000 + B)
    net1 = pkg.MAF((D, ), '2d', NS(layers=K, mixtures=8)).to(DEV)
    net2 = copy.deepcopy(net1)
    net1.draws = 'device'
    net3 = copy.deepcopy(net1)                              # same seed words: the same draws once more, for the oracle comparison
    sd0 = om.clone_state(net1.state_dict())
    y = (torch.randn(B, D) * 0.7).to(DEV)
    deg = _recorded(pkg, net1, 2 * K, D)
    assert D < 3 or len(np.unique(deg)) == D - 1
    t1, t2 = train.FlowTrainer(net1, graph=False), train.FlowTrainer(net2, graph=False)
    assert net1.draws == 'device' and net2.draws == 'host'
    off0 = int(net1.seed[1])
    net1.train()
    z1, l1 = t1._forward_backward(y)
    assert int(net1.seed[1]) == off0 + 2 * K                # one launch of 2 K draws per run (2 per step on the per-step path)
    replay = ReplayRng(deg)
    monkeypatch.setattr(fused, 'MAF_FLOW', False)
    monkeypatch.setattr(np.random, 'randint', replay.randint)
    net2.train()
    z2, l2 = t2._forward_backward(y)
    monkeypatch.undo()
    assert replay.at == 2 * K * 3
    G.assert_close(z1, z2, 1e-6, rtol=1e-6, what='z')
    G.assert_close(l1, l2, 1e-6, rtol=1e-6, what='loss')
    G.assert_close(t1.bucket.flat, t2.bucket.flat, 2e-5 * max(1.0, float(t2.bucket.flat.abs().max())), what='flat grads')
    _buffers_close(net1, net2, 1e-6, 1e-6)
    # the oracle on the same degrees: z and log-det
    net3.train()
    with torch.no_grad():
        z3, ld3 = net3(y)
    ora = om.FlowOracle('maf', (D, ), '2d', K, sd0, training=True, mask_rng=ReplayRng(deg))
    with torch.no_grad():
        z0, ld0 = ora.forward(y.cpu())
    assert ora.mask_rng.at == 2 * K * 3
    G.assert_close(z3, z0, 1e-5, rtol=1e-5, what='z against the oracle')
    G.assert_close(ld3, ld0, 1e-5, rtol=1e-5, what='log-det against the oracle')
    assert fused.N.persistent_timeouts() == 0


@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('D,B,K', [(3, 300, 2), (4, 9, 1)])
def test_inverse_is_one_launch_per_step_with_a_mask_set_per_pass(pkg, D, B, K, training, monkeypatch):
    """net.backward in 'device' mode (one nf_maf_step_inv_drawn launch per step: 2 D draws, pass-major) against the layer-by-layer
    inverse in 'host' mode fed the same degrees.  No round trip at D > 2: the reference's inverse draws other masks than its forward."""
    fused = importlib.import_module(pkg.__name__ + '.fused')
    torch.manual_seed(D * 100 + B + 5)
    np.random.seed(D + B)
    net1 = pkg.MAF((D, ), '2d', NS(layers=K, mixtures=8)).to(DEV)
    with torch.no_grad():
        net1.train()
        for _ in range(2):                                  # running statistics away from their initial values
            net1((torch.randn(max(B, 64), D) * 0.8 + 0.1).to(DEV))
        for p in net1.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    net2 = copy.deepcopy(net1)
    net1.draws = 'device'
    net1.train(training)
    net2.train(training)
    y = (torch.randn(B, D) * 0.9).to(DEV)
    deg = _recorded(pkg, net1, K * 2 * D, D)
    calls = {'drawn': 0, 'inv': 0}
    real_drawn, real_inv = fused.maf_step_inverse_drawn, fused.maf_step_inverse

    def c_drawn(*a, **k):
        calls['drawn'] += 1
        return real_drawn(*a, **k)

    def c_inv(*a, **k):
        calls['inv'] += 1
        return real_inv(*a, **k)

    monkeypatch.setattr(fused, 'maf_step_inverse_drawn', c_drawn)
    monkeypatch.setattr(fused, 'maf_step_inverse', c_inv)
    off0 = int(net1.seed[1])
    with torch.no_grad():
        z1, l1 = net1.backward(y.clone())
        assert int(net1.seed[1]) == off0 + K * 2 * D
        replay = ReplayRng(deg)
        monkeypatch.setattr(fused, 'GLOW_INVERSE', False)
        monkeypatch.setattr(np.random, 'randint', replay.randint)
        z2, l2 = net2.backward(y.clone())
    monkeypatch.undo()
    assert replay.at == K * 2 * D * 3
    assert calls == {'drawn': K, 'inv': 0}, calls
    G.assert_close(z1, z2, 2e-5, rtol=2e-5, what='inverse samples')
    G.assert_close(l1, l2, 2e-5, rtol=2e-5, what='inverse log-det')
    _buffers_close(net1, net2, 2e-6, 1e-5)
    assert fused.N.persistent_timeouts() == 0


def test_trainer_captures_the_step_on_three_dimensional_data(pkg):
    """FlowTrainer(graph=True) on a 3-D MAF switches the draws to the device and keeps the graph (the parent commit fell back to eager
    launches: tr.graph was False).  Ordered mode, as tests/test_gpu_trainer_loop.py: six calls at warmup = 2 are SEVEN optimizer steps (the
    capturing call takes one extra eager step), and an eager trainer in 'device' mode built from the same seeds ends on the same parameter
    bits after the same seven steps."""
    nftrain = importlib.import_module(pkg.__name__ + '.train')
    nfdata = importlib.import_module(pkg.__name__ + '.data')
    N = pkg._native
    N.load()
    was = N.deterministic()
    N.deterministic(True)
    try:
        def build(graph):
            torch.manual_seed(3)
            np.random.seed(3)
            net = pkg.MAF((3, ), '2d', NS(layers=2)).to(DEV)
            if not graph:
                net.draws = 'device'
            return nftrain.FlowTrainer(net, graph=graph, warmup=2, sampler=nfdata.DeviceSampler('swiss', 256, (3, )))

        tr = build(True)
        assert tr.graph is True and tr.net.draws == 'device'
        losses, offsets = [], []
        for call in range(6):
            z, loss = tr.train_on_batch()
            losses.append(float(loss))
            offsets.append(int(tr.net.seed[1]))
            if call == 3:
                assert tr.graph is True and tr._g_fb is not None
        graph = tr._g_fb
        assert graph is not None
        # two steps of two MADEs each: four draws per step, eager or replayed (the capturing call ran two steps)
        assert offsets == [4, 8, 16, 20, 24, 28], offsets
        assert all(np.isfinite(losses)) and len(set(losses)) == len(losses), losses
        assert int(tr.optim.step_count) == 7
        eager = build(False)
        assert eager.graph is False
        for _ in range(7):
            eager.train_on_batch()
        torch.cuda.synchronize()
        assert int(eager.optim.step_count) == 7 and int(eager.net.seed[1]) == 28
        assert torch.equal(tr.bucket.flat_params, eager.bucket.flat_params)
        assert N.deterministic_timeouts() == 0 and N.persistent_timeouts() == 0
    finally:
        N.deterministic(was)
