"""
Host-side checks of the planar flow (no GPU): the restatement in tests/_planar.py against the live reference (where it exists) and the
committed goldens (tests/golden/model_planar.npz, make_goldens_planar.py), the engine's seeded construction, the NF_DROPIN_PLANAR switch
of the drop-in, and the host-side argument checks of the new C-ABI entry points.
"""
import ctypes
import os
import subprocess
import sys
import textwrap
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import _planar as P
from tests._golden import group

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, 'normalizing-flows-pytorch_amd', 'dropin')
K = 4


def _close(a, b, tol, what):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol * max(1.0, float(b.abs().max()) if b.numel() else 1.0), '%s: max abs err %.3e' % (what, err)


def _fwd_loss_grads(sd, y, dtype):
    params = P.params_of(sd, K, dtype, requires_grad=True)
    z, ld, _ = P.forward(y.to(dtype), torch.zeros(y.shape[0], dtype=dtype), params)
    loss = P.nll(z, ld)
    loss.backward()
    return z, ld, loss, params


@pytest.mark.parametrize('D', [2, 3])
def test_restatement_matches_goldens(D):
    g = group('model_planar', 'd%d/' % D)
    sd = {k[len('sd0/'):]: v for k, v in g.items() if k.startswith('sd0/')}
    z, ld, loss, params = _fwd_loss_grads(sd, g['y'], torch.float32)
    _close(z, g['z'], 1e-6, 'z')
    _close(ld, g['ld'], 1e-6, 'ld')
    _close(loss, g['loss'], 1e-6, 'loss')
    for i, (u, w, b) in enumerate(params):
        for n, t in zip('uwb', (u, w, b)):
            _close(t.grad, g['grad/net.layers.%d.%s' % (i, n)], 1e-6, 'grad %d.%s' % (i, n))
    with torch.no_grad():
        x, ldi, _ = P.inverse(g['z'], torch.zeros(g['z'].shape[0]), P.params_of(sd, K, torch.float32))
    _close(x, g['x_inv'], 1e-6, 'x_inv')
    _close(ldi, g['ld_inv'], 1e-6, 'ld_inv')


def test_restatement_projection_matches_goldens():
    g = group('model_planar', 'proj/')
    sd0 = {k[len('sd0/'):]: v for k, v in g.items() if k.startswith('sd0/')}
    with torch.no_grad():
        z, ld, us = P.forward(g['y'], torch.zeros(g['y'].shape[0]), P.params_of(sd0, K, torch.float32))
    _close(z, g['z'], 1e-6, 'z')
    _close(ld, g['ld'], 1e-6, 'ld')
    for i in range(K):
        _close(us[i], g['sd1/net.layers.%d.u' % i], 1e-6, 'projected u %d' % i)
    assert not torch.equal(g['sd0/net.layers.1.u'], g['sd1/net.layers.1.u'])


def test_restatement_matches_live_reference(ref_flows):
    for D in (2, 3):
        torch.manual_seed(7)
        net = ref_flows.PlanarFlow((D, ), '2d', NS(layers=K))
        with torch.no_grad():                                       # parameters large enough to exercise the projection
            for m in net.net.layers:
                m.u.mul_(100.0)
                m.w.mul_(100.0)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        y = torch.randn(128, D) * 0.5
        z0, ld0 = net(y.clone())
        with torch.no_grad():
            z, ld, us = P.forward(y, torch.zeros(128), P.params_of(sd, K, torch.float32))
        _close(z, z0, 1e-6, 'z')
        _close(ld, ld0, 1e-6, 'ld')
        for i, m in enumerate(net.net.layers):
            _close(us[i], m.u, 1e-6, 'u %d' % i)
        with torch.no_grad():
            x0, ldi0 = net.backward(z0.detach().clone())
            x, ldi, _ = P.inverse(z0.detach(), torch.zeros(128), P.params_of(net.state_dict(), K, torch.float32))
        _close(x, x0, 1e-6, 'x_inv')
        _close(ldi, ldi0, 1e-6, 'ld_inv')


def test_exit_rule_counts_on_cpu():
    """the reference's float32 loop on the layer w = (1, 0), u = (0, 0.5), b = 0 (w.u = 0: val = mid exactly): 28 iterations; one row
    whose target is hit exactly at the first midpoint (0.0) sticks the batch at 100, so does a rounding-limited root (300.3)"""
    params = [(torch.tensor([[0.0, 0.5]]), torch.tensor([[1.0, 0.0]]), torch.zeros(1))]
    z = torch.stack([torch.full((8, ), 0.5), torch.randn(8)], 1)
    assert P.inverse(z, torch.zeros(8), params)[2] == [28]
    z1 = torch.cat([z, torch.tensor([[0.0, 0.3]])])
    assert P.inverse(z1, torch.zeros(9), params)[2] == [100]
    z2 = torch.cat([z, torch.tensor([[300.3, -0.2]])])
    assert P.inverse(z2, torch.zeros(9), params)[2] == [100]


@pytest.mark.parametrize('D', [2, 3])
def test_engine_construction_matches_golden_state(pkg, D):
    g = group('model_planar', 'd%d/sd0/' % D)
    torch.manual_seed(100)
    net = pkg.PlanarFlow((D, ), '2d', NS(layers=K))
    sd = net.state_dict()
    assert sorted(sd) == sorted(g)
    for k, v in g.items():
        assert torch.equal(sd[k], v), k
    assert net.dims == (D, ) and net.dim == D and net.n_layers == K and len(net.net.layers) == K


def test_four_d_input_raises(pkg):
    net = pkg.PlanarFlow((3, 4, 4), 'image', NS(layers=2))
    assert net.dim == 48
    with pytest.raises(RuntimeError, match=r'\(2, 3, 4, 4\)'):
        net(torch.rand(2, 3, 4, 4))
    with pytest.raises(RuntimeError, match=r'\(2, 3, 4, 4\)'):
        net.backward(torch.rand(2, 3, 4, 4))


def test_dropin_planar_switch_without_reference(tmp_path, pkg):
    pkg.build()
    code = textwrap.dedent('''
        import os, sys
        sys.path = [p for p in sys.path if 'reference' not in p]
        from types import SimpleNamespace as NS
        import flows
        from flows import PlanarFlow
        assert flows.REFERENCE_DIR is None, flows.REFERENCE_DIR
        if os.environ.get('NF_DROPIN_PLANAR') == '1':
            import flows.planar
            net = PlanarFlow((2,), '2d', NS(layers=3))
            assert type(net).__module__.endswith('.models') and type(net).__name__ == 'PlanarFlow', type(net)
            assert type(net) is flows._pkg.PlanarFlow and flows.planar.PlanarFlow is PlanarFlow
            assert flows.planar.PlanarTransform is flows._pkg.PlanarTransform
            assert sorted(net.state_dict())[:3] == ['net.layers.0.b', 'net.layers.0.u', 'net.layers.0.w']
        else:
            try:
                PlanarFlow((2,), '2d', None)
            except NotImplementedError:
                pass
            else:
                raise SystemExit('PlanarFlow constructed without a reference and without the switch')
            try:
                import flows.planar
            except ImportError:
                pass
            else:
                raise SystemExit('flows.planar resolved without a reference and without the switch')
        print('ok')
    ''')
    for val in ('1', '0'):
        env = dict(os.environ, PYTHONPATH=DROPIN, PYTHONDONTWRITEBYTECODE='1', NF_DROPIN_PLANAR=val)
        env.pop('NF_REFERENCE_FLOWS', None)
        r = subprocess.run([sys.executable, '-c', code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith('ok'), (val, r.stdout, r.stderr)


def test_planar_cabi_rejects_bad_arguments(pkg):
    pkg.build()
    N = pkg._native
    lib = N.load()
    assert N.header_constant('NF_PLANAR_MAX_LAYERS') == pkg.functional.PLANAR_MAX_LAYERS
    assert N.header_constant('NF_PLANAR_INV_WG_MAX_ROWS') == 16384
    dummy = (ctypes.c_int64 * 3)(16, 16, 16)                       # (never dereferenced: every call below fails its host checks)
    zeros = (ctypes.c_int64 * 3)(0, 0, 0)
    big = (ctypes.c_int64 * (3 * 129))(*([16] * (3 * 129)))
    E = 10001
    assert lib.nf_planar_project(None, 1, 2, None) == E
    assert lib.nf_planar_project(zeros, 1, 2, None) == E
    assert lib.nf_planar_project(dummy, 0, 2, None) == E
    assert lib.nf_planar_project(big, 129, 2, None) == E
    assert lib.nf_planar_project(dummy, 1, 0, None) == E
    assert lib.nf_planar_fwd(None, None, None, None, dummy, 1, 4, 2, None) == E           # B > 0 without z / out / ld
    assert lib.nf_planar_fwd(None, None, None, None, dummy, 1, -1, 2, None) == E
    assert lib.nf_planar_fwd(None, None, None, None, None, 1, 0, 2, None) == E
    n = ctypes.c_int64(0)
    assert lib.nf_planar_bwd_slab_floats(0, 4, 2, ctypes.byref(n)) == E
    assert lib.nf_planar_bwd_slab_floats(2, 4, 2, None) == E
    assert lib.nf_planar_bwd_slab_floats(2, 300, 2, ctypes.byref(n)) == 0 and n.value == 2 * 4 * 2 * 5
    assert lib.nf_planar_bwd(None, None, None, dummy, dummy, None, None, 1, 4, 2, None) == E
    assert lib.nf_planar_bwd(None, None, None, dummy, None, None, None, 1, 0, 2, None) == E
    assert lib.nf_planar_inv(None, None, None, None, None, None, None, dummy, 1, 0, 2, None) == E  # no iters
    assert lib.nf_planar_inv(None, None, None, None, None, None, None, None, 1, 0, 2, None) == E
    assert lib.nf_planar_inv(None, None, None, None, None, None, None, dummy, 1, -3, 2, None) == E
    assert lib.nf_planar_inv(None, None, None, None, None, None, None, dummy, 0, 4, 2, None) == E


def test_planar_goldens_are_data_only():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'model_planar.npz')) as f:
        assert all(f[k].dtype.kind in 'fiu' for k in f.files)
        assert 'main/step2/loss' in f.files and 'proj/sd1/net.layers.1.u' in f.files
