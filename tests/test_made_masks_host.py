"""
Host side of the device-drawn MADE masks (csrc/made_masks.hip, MAF.draws): the mask rule from given degrees, the model's switch and
seed words, the two C-ABI entry points in the header.  No GPU needed.
"""
import importlib
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ReplayRng:
    """stands in for np.random: hands out recorded degree vectors in order and checks the bounds the caller asks for"""

    def __init__(self, degrees):
        self.degrees, self.at = [np.asarray(d) for d in degrees], 0

    def randint(self, lo, hi, size=None):
        m = self.degrees[self.at]
        self.at += 1
        assert m.shape == (size, ) and (m >= lo).all() and (m < hi).all(), (lo, hi, size, m)
        return m.copy()


def _degrees(D, rng, H=32, layers=3):
    m_prev, out = np.arange(D), []
    for _ in range(layers):
        lo = min(int(m_prev.min()), D - 2)
        m_prev = rng.randint(lo, D - 1, size=H)
        out.append(m_prev)
    return out


@pytest.mark.parametrize('D', [1, 2, 3, 4, 5])
def test_masks_from_degrees_equal_the_drawing_rule_and_are_autoregressive(pkg, D):
    cond = importlib.import_module(pkg.__name__ + '.conditioners')
    for trial in range(8):
        deg = _degrees(D, np.random.RandomState(10 * D + trial))
        direct = cond.made_masks_from_degrees(D, deg)
        stub = ReplayRng(deg)
        drawn = cond.made_degrees_to_masks(D, 3, 32, stub)
        assert stub.at == 3
        assert [m.shape for m in direct] == [(32, D), (32, 32), (32, 32), (D, 32)]
        for a, b in zip(direct, drawn):
            assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b)
        # output r may depend on input c only for c < r (maf.py:66-85): the product of the masks counts the open paths
        paths = direct[3] @ direct[2] @ direct[1] @ direct[0]
        for r in range(D):
            for c in range(r, D):
                assert paths[r, c] == 0, (D, r, c)
        if D >= 2:
            assert paths[D - 1, 0] > 0                      # (and the last output does see the first input)


def test_maf_draws_switch_and_seed_words(pkg):
    torch.manual_seed(1234)
    net = pkg.MAF((3, ), '2d', NS(layers=2, mixtures=None))
    assert net.draws == 'host'
    assert net.seed.dtype == torch.int64 and net.seed.tolist() == [1234, 0]
    assert 'seed' not in net.state_dict() and 'seed' in dict(net.named_buffers())
    net.draws = 'device'
    mades = [m for m in net.modules() if isinstance(m, pkg.MADE)]
    assert net.draws == 'device' and len(mades) == 4 and all(m.draws == 'device' and m._seed is net.seed for m in mades)
    with pytest.raises(ValueError):
        net.draws = 'elsewhere'
    assert net.draws == 'device'
    net.draws = 'host'
    assert all(m.draws == 'host' for m in mades)
    assert pkg.MAF((3, ), '2d', NS(layers=1, mixtures=None)).draws == 'host'
    with pytest.raises(ValueError):
        pkg.MAF((5, ), '2d', NS(layers=1, mixtures=None)).draws = 'device'      # the draw kernel serves D <= 4


def test_host_mode_consumes_np_random_as_before(pkg):
    """'host' mode: two MADE draws per step and call from the global np.random, in order"""
    cond = importlib.import_module(pkg.__name__ + '.conditioners')
    torch.manual_seed(0)
    net = pkg.MAF((3, ), '2d', NS(layers=2, mixtures=None)).train()
    np.random.seed(5)
    x = torch.randn(16, 3)
    for m in net.modules():
        if isinstance(m, pkg.AutoregressiveTransfrom):
            s_raw, t = m.conditioners(x)                    # (CPU: the two MADE modules one after the other)
            assert s_raw.shape == t.shape == (16, 3)
    after = np.random.randint(0, 1 << 30)
    np.random.seed(5)
    for _ in range(4):
        cond.made_degrees_to_masks(3, 3, 32, np.random)
    assert after == np.random.randint(0, 1 << 30)


def test_header_declares_the_new_entry_points(pkg):
    protos = pkg._native.header_prototypes(os.path.join(ROOT, 'include', 'nfhip.h'))
    assert len(protos['nf_made_draw_masks']) == 7
    assert len(protos['nf_maf_step_inv_drawn']) == len(protos['nf_maf_step_inv']) + 1
    hc = pkg._native.header_constant
    assert hc('NF_MADE_MASK_STRIDE') == 2 * 32 * 32 + 2 * 4 * 32
    assert [hc('NF_MADE_MASK_OFF_%d' % l) for l in range(4)] == [0, 128, 128 + 1024, 128 + 2048]
