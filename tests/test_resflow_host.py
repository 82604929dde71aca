"""
Host-side checks of the whole-stack Residual Flow path (no GPU): the C ABI of csrc/resflow.hip is exported and rejects bad arguments on the
host, the in-kernel series-length and coefficient formulas (restated in resflow.series_length / series_coefficients) equal the
coefficients of the per-block path, Compose._resflow_run declines everything the kernels do not serve, and the seed buffer of
``draws = 'device'`` leaves the state_dict alone.
"""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

NEW = ['nf_resflow_param_floats', 'nf_resflow_spectral', 'nf_resflow_fwd', 'nf_resflow_bwd_slab_floats', 'nf_resflow_bwd',
       'nf_resflow_spectral_bwd', 'nf_resflow_inv', 'nf_resflow_draws']


def _net(pkg, L=3, D=2, logdet='unbias'):
    return pkg.ResFlow((D, ), '2d', NS(layers=L, spnorm_coeff=0.9, logdet=logdet))


def test_new_symbols_are_exported(pkg):
    pkg.build()
    N = pkg._native
    lib = N.load()
    protos = N.header_prototypes()
    for name in NEW:
        assert name in protos, name
        assert getattr(lib, name) is not None
    assert N.header_constant('NF_RESFLOW_MAX_LAYERS') == pkg.functional.RESFLOW_MAX_LAYERS
    assert N.header_constant('NF_RESFLOW_INV_WG_MAX_ROWS') == 4096


def test_packed_row_size_matches_the_library(pkg):
    import ctypes
    pkg.build()
    lib = pkg._native.load()
    for D in (1, 2, 3, 4):
        n = ctypes.c_int(0)
        assert lib.nf_resflow_param_floats(D, ctypes.byref(n)) == 0
        assert n.value == pkg.functional.resflow_param_floats(D)
    assert lib.nf_resflow_param_floats(5, ctypes.byref(n)) != 0


def test_cabi_rejects_bad_arguments_on_the_host(pkg):
    """every check below fails before anything is launched: no GPU is touched"""
    import ctypes
    pkg.build()
    lib = pkg._native.load()
    one = ctypes.c_void_p(16)                               # a non-NULL stand-in: rejected calls never dereference it
    cap = pkg._native.header_constant('NF_RESFLOW_MAX_LAYERS')
    assert lib.nf_resflow_spectral(one, one, cap + 1, 2, 0.9, 1e-5, None) != 0
    assert lib.nf_resflow_spectral(one, one, 2, 5, 0.9, 1e-5, None) != 0
    assert lib.nf_resflow_spectral(None, one, 2, 2, 0.9, 1e-5, None) != 0
    # series mode without draws, too many samples, a bad geometric law
    assert lib.nf_resflow_fwd(one, one, one, None, one, None, None, None, 2, 1, 1, 0, 0.5, 2, 0, 8, 2, None) != 0
    assert lib.nf_resflow_fwd(one, one, one, None, one, one, one, None, 2, 5, 1, 0, 0.5, 2, 0, 8, 2, None) != 0
    assert lib.nf_resflow_fwd(one, one, one, None, one, one, one, None, 2, 1, 1, 0, 1.0, 2, 0, 8, 2, None) != 0
    assert lib.nf_resflow_fwd(one, one, one, None, one, one, one, None, 3, 1, 1, 0, 0.5, 2, 0, 8, 2, None) != 0
    assert lib.nf_resflow_bwd(one, one, one, one, one, None, None, None, 1, 0.5, one, 2, 0, 8, 2, None) != 0
    assert lib.nf_resflow_spectral_bwd(one, one, one, one, 2, 8, 2, 0.9, 1e-5, None) != 0       # sinks AND a flat buffer
    assert lib.nf_resflow_spectral_bwd(one, None, None, one, 2, 8, 2, 0.9, 1e-5, None) != 0     # neither
    rows = pkg._native.header_constant('NF_RESFLOW_INV_WG_MAX_ROWS')
    assert lib.nf_resflow_inv(one, one, one, one, one, one, None, None, None, 1, 0, 0, 0, 0.5, 0.9, 1e-5, 1e-4, 2, 0, rows + 1, 2, None) != 0
    assert lib.nf_resflow_draws(one, one, None, 2, 1, 1, 0, 0.5, 2, 0, 8, 2, None) != 0
    n = ctypes.c_int64(0)
    assert lib.nf_resflow_bwd_slab_floats(2, 1024, 2, ctypes.byref(n)) == 0
    assert n.value == 64 * 2 * pkg.functional.resflow_param_floats(2)                            # the grid cap: 64 workgroups
    assert lib.nf_resflow_bwd_slab_floats(2, 6, 2, ctypes.byref(n)) == 0
    assert n.value == 1 * 2 * pkg.functional.resflow_param_floats(2)


@pytest.mark.parametrize('n', list(range(2, 65)))
def test_coefficient_restatement_equals_the_per_block_tables(pkg, n):
    """the kernels build their coefficients from (n, n_exact, p) with a running float32 product; the per-block path builds tables on the
    host in float64 and rounds (resflow._series, _ResidualBranchHip.forward).  For p = 0.5 both are exact to the last bit."""
    RF = pkg.resflow
    p = 0.5
    for n_exact in (1, 8):                                  # training value estimator, evaluation `unbias`
        want = np.zeros(n, dtype=np.float32)
        for k in range(1, n + 1):
            want[k - 1] = (-1) ** (k + 1) / (k * (1.0 - p) ** max(0, (k - n_exact) - 1))       # resflow._series
        assert np.array_equal(RF.series_coefficients(n, n_exact, p), want)
    want = np.zeros(n, dtype=np.float32)
    for k in range(1, n + 1):
        want[k - 1] = (-1) ** k / (1.0 - p) ** max(0, (k - 1) - 1)                             # _ResidualBranchHip.forward
    assert np.array_equal(RF.series_coefficients(n, 1, p, neumann=True), want)
    if n <= 8:                                              # the `fixed` estimator is n_exact >= n: (-1)^(k+1) / k
        want = np.array([(-1) ** (k + 1) / k for k in range(1, n + 1)], dtype=np.float32)
        assert np.array_equal(RF.series_coefficients(n, 8, p), want)


def test_series_coefficients_match_the_block_on_a_seeded_draw(pkg):
    """the tables InvertibleResLinear._series really builds, for the lengths it really draws"""
    RF = pkg.resflow
    blk = pkg.InvertibleResLinear(2, 2, coeff=0.9, logdet_estimator='unbias')
    blk.noise_on_cpu = True
    np.random.seed(3)
    x = torch.zeros(4, 2)
    for training, n_exact, S in ((True, 1, 1), (False, 8, 4)):
        mode, noise, coef, nts, S_ = blk._series(x, training)
        assert mode == 2 and S_ == S
        for s in range(S):
            n = int(nts[s])
            assert np.array_equal(coef[s, :n].numpy(), RF.series_coefficients(n, n_exact))
            assert not coef[s, n:].any()


def test_length_restatement(pkg):
    """n = n_exact + ceil(log(u) / log(1 - p)): a geometric(p) on {1, 2, ..} shifted by n_exact, clamped to 64"""
    RF = pkg.resflow
    assert RF.series_length(0.75, 1) == 2 and RF.series_length(0.5, 1) == 2 and RF.series_length(0.49, 1) == 3
    assert RF.series_length(0.25, 8) == 10 and RF.series_length(0.2, 8) == 11
    assert RF.series_length(1e-30, 8) == RF.SERIES_MAXK
    u = (np.arange(1 << 16) + 0.5) / (1 << 16)
    n = np.array([RF.series_length(v, 1) for v in u]) - 1
    assert abs(n.mean() - 2.0) < 1e-3 and n.min() == 1      # the mean of a geometric(0.5)
    assert abs((n == 1).mean() - 0.5) < 1e-3 and abs((n == 2).mean() - 0.25) < 1e-3


def test_stack_draws_consume_the_generators_as_the_blocks_do(pkg):
    """host draws of the stack = the per-block path's, block by block, surrogate first (same np.random and torch streams)"""
    RF = pkg.resflow
    net = _net(pkg, L=3)
    blocks = [m for m in net.net.layers if isinstance(m, pkg.InvertibleResLinear)]
    for b in blocks:
        b.noise_on_cpu = True
    x = torch.zeros(5, 2)
    np.random.seed(11)
    torch.manual_seed(11)
    n_terms, noise = RF.stack_draws(blocks, x, True, 2)
    assert tuple(n_terms.shape) == (3, 2, 1) and tuple(noise.shape) == (3, 2, 5, 1, 2)
    np.random.seed(11)
    torch.manual_seed(11)
    for l, b in enumerate(blocks):
        n0 = min(int(1 + np.random.geometric(0.5)), RF.SERIES_MAXK)
        v0 = b._randn_like(x)
        _, v1, _, nts, _ = b._series(x, True)
        assert int(n_terms[l, 0, 0]) == n0 and int(n_terms[l, 1, 0]) == int(nts[0])
        assert torch.equal(noise[l, 0, :, 0], v0) and torch.equal(noise[l, 1], v1)
    after = (np.random.geometric(0.5), torch.randn(1))
    np.random.seed(11)
    torch.manual_seed(11)
    RF.stack_draws(blocks, x, True, 2)
    assert after[0] == np.random.geometric(0.5) and torch.equal(after[1], torch.randn(1))
    # evaluation: `unbias` draws 4 samples after the discarded surrogate draw; `exact` consumes the surrogate's draw alone
    for b in blocks:
        b.eval()
    np.random.seed(12)
    torch.manual_seed(12)
    n_terms, noise = RF.stack_draws(blocks, x, False, 2)
    assert tuple(n_terms.shape) == (3, 2, 4) and tuple(noise.shape) == (3, 2, 5, 4, 2)
    np.random.seed(12)
    torch.manual_seed(12)
    for l, b in enumerate(blocks):
        np.random.geometric(0.5)
        b._randn_like(x)
        _, v1, _, nts, _ = b._series(x, False)
        assert n_terms[l, 1].tolist() == nts.tolist() and torch.equal(noise[l, 1], v1)
    for b in blocks:
        b.estimator = 'exact'
    np.random.seed(13)
    torch.manual_seed(13)
    assert RF.stack_draws(blocks, x, False, 2) == (None, None)
    got = (np.random.geometric(0.5), torch.randn(1))
    np.random.seed(13)
    torch.manual_seed(13)
    for b in blocks:
        np.random.geometric(0.5)
        b._randn_like(x)
    assert got[0] == np.random.geometric(0.5) and torch.equal(got[1], torch.randn(1))


def test_resflow_run_is_empty_where_the_kernels_do_not_serve(pkg):
    net = _net(pkg, L=2, D=2).eval()
    acts = [m for m in net.net.layers if isinstance(m, pkg.ActNorm)]
    x = torch.zeros(4, 2)
    with torch.no_grad():
        for a in acts:
            a.initialized = True
        assert net.net._resflow_run(0, x, 1) == []                      # CPU tensors
        assert net.net._resflow_run(3, x, -1) == []
        fake = torch.zeros(4, 2, device='meta')                          # the remaining checks need `is_cuda`: a stand-in tensor

        class Cuda:                                                      # (no GPU here: the shape / dtype / device of a GPU batch)
            is_cuda, dtype, shape = True, torch.float32, fake.shape

            def dim(self):
                return 2
        z = Cuda()
        assert len(net.net._resflow_run(0, z, 1)) == 2                   # the positive control: both pairs
        assert [id(k) for _, k in net.net._resflow_run(3, z, -1)] == [id(k) for _, k in net.net._resflow_run(0, z, 1)]
        acts[1].initialized = False                                      # an uninitialised ActNorm ends the run in front of it
        assert len(net.net._resflow_run(0, z, 1)) == 1
        assert net.net._resflow_run(3, z, -1) == []
        acts[0].initialized = False
        assert net.net._resflow_run(0, z, 1) == []
        for a in acts:
            a.initialized = True
        h = net.net.layers[1].register_forward_hook(lambda m, i, o: None)   # a forward hook on a member
        assert net.net._resflow_run(0, z, 1) == []
        h.remove()
        assert len(net.net._resflow_run(0, z, 1)) == 2
        net.train()                                                      # training-mode blocks under no_grad: the block's own route
        assert net.net._resflow_run(0, z, 1) == []
        net.eval()
        old = pkg.functional.RESFLOW_STACK
        try:
            pkg.functional.RESFLOW_STACK = False                         # NF_RESFLOW_STACK=0
            assert net.net._resflow_run(0, z, 1) == []
        finally:
            pkg.functional.RESFLOW_STACK = old
    net5 = _net(pkg, L=2, D=5).eval()                                    # D = 5: more features than the kernels take
    for m in net5.net.layers:
        if isinstance(m, pkg.ActNorm):
            m.initialized = True

    class Cuda5:
        is_cuda, dtype, shape = True, torch.float32, torch.Size([4, 5])

        def dim(self):
            return 2
    with torch.no_grad():
        assert net5.net._resflow_run(0, Cuda5(), 1) == []


def test_seed_buffer_is_not_in_the_state_dict(pkg):
    net = _net(pkg, L=2)
    keys = set(net.state_dict().keys())
    assert 'seed' not in keys and not any('seed' in k for k in keys)
    assert net.seed.dtype == torch.int64 and tuple(net.seed.shape) == (2, )
    want = set()
    for i in range(2):
        want |= {'net.layers.%d.log_scale' % (2 * i), 'net.layers.%d.bias' % (2 * i)}
    assert want <= keys and all(k.startswith('net.layers.') for k in keys)
    assert net.draws == 'host'
    net.draws = 'device'
    assert net.draws == 'device' and net.net._resflow_draws == 'device'
    assert set(net.state_dict().keys()) == keys
    with pytest.raises(ValueError):
        net.draws = 'elsewhere'
    fresh = _net(pkg, L=2)
    fresh.load_state_dict(net.state_dict())                               # strict: no missing or unexpected key
    assert fresh.draws == 'host'
