"""GPU parity of the pixel-contraction weight-gradient kernel (csrc/conv_bulk.hip: k_conv3_bulk_wgrad) at the smallest shapes at which
its tile pipeline can go wrong: the filling waves keep the loads of two tiles in flight in two register sets and convert them into two
LDS frame pairs while the walking waves are a tile behind, so what matters is the number of tiles a workgroup walks (the prologue's
n > 0 / 1 / 2 branches, odd and even ends), ragged and half-empty tiles, the halo rows of the first and last tile of a sample, several
samples per tile, and the descriptor-table launch form.  (The kernel takes maps 8 or 16 pixels wide: at W = 32 its filling threads
would need a sixth activation item, the launch goes to conv_bn.hip, and four-row tiles -- TH = 4 -- cannot be reached.  Every case
asserts that ITS launch is the bulk kernel's: nf_conv_bulk_wgrad_plan.  The 32 x 32 cases are kept as a check of that hand-over: the same
comparisons, and an assertion that the plan says conv_bn.hip.)  Through nf_conv_bn_wgrad_multi and nf_conv_bn_wgrad_table (which takes the slab
count: that is how a workgroup gets more than one tile at a tiny batch) with the bulk path forced, every layer's summed weight gradient
and bias sums against float64 and against the per-layer kernel of conv_bn.hip; two runs from the same inputs leave identical slabs."""
import ctypes
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
R = 8            # NF_STAT_REPL


def _cfg(pkg, on, min_px=-1, nblk=-1):
    pkg._native.call('nf_conv_bulk_config', int(on), int(min_px), int(nblk))


@pytest.fixture()
def bulk(pkg):
    pkg._native.load()
    _cfg(pkg, 1, 0, 0)
    yield pkg
    _cfg(pkg, 1, 16385, 0)


# the three forms of the output gradient G
DIRECT, SRC, SRC_SKIP = 'direct', 'src', 'src_skip'

_layers = {}


@pytest.fixture(scope='module', autouse=True)
def _drop_layers():
    yield
    _layers.clear()                              # (the operands live on the GPU: not beyond this module)


def _make_layers(B, I, H, W, nl, form):
    """operands of nl layers and their float64 results, built once per shape and shared by the launch forms that walk it"""
    key = (B, I, H, W, nl, form)
    if key in _layers:
        return _layers[key]
    torch.manual_seed(B * 7 + I + nl + 13 * H + len(form))
    has_bn = I == 32 or form == SRC                  # the filler's BatchNorm + ReLU of the activations at I = 6 and 17 as well
    n = B * H * W
    layers = []
    for _ in range(nl):
        x = torch.randn(B, I, H, W, device=DEV)
        out = torch.randn(B, 32, H, W, device=DEV) * 2.0 + 0.5
        src = form != DIRECT
        gn_src = torch.randn(B, 32, H, W, device=DEV) if src else None
        g_skip = torch.randn(B, 32, H, W, device=DEV) if form == SRC_SKIP else None
        g_direct = torch.randn(B, 32, H, W, device=DEV) if form == DIRECT else None
        gamma, beta = torch.rand(I, device=DEV) + 0.5, torch.randn(I, device=DEV) * 0.3
        cgamma = torch.rand(32, device=DEV) + 0.5
        xd, od = x.double(), out.double()
        mean = xd.mean((0, 2, 3))
        invstd = 1.0 / torch.sqrt(xd.var((0, 2, 3), unbiased=False) + 1e-5)
        cmean = od.mean((0, 2, 3))
        cinvstd = 1.0 / torch.sqrt(od.var((0, 2, 3), unbiased=False) + 1e-5)
        Gd = torch.zeros(B, 32, H, W, dtype=torch.float64, device=DEV)
        cs1, cs2 = torch.zeros(R, 32, device=DEV), torch.zeros(R, 32, device=DEV)
        if src:
            gd = gn_src.double()
            xh = (od - cmean.view(1, -1, 1, 1)) * cinvstd.view(1, -1, 1, 1)
            sg_c, sgx_c = gd.sum((0, 2, 3)), (gd * xh).sum((0, 2, 3))
            cs1[2] = sg_c.float() * 0.5
            cs1[7] = sg_c.float() * 0.5
            cs2[4] = sgx_c.float()
            Gd = cgamma.double().view(1, -1, 1, 1) * cinvstd.view(1, -1, 1, 1) * (gd - (sg_c / n).view(1, -1, 1, 1) - xh * (sgx_c / n).view(1, -1, 1, 1))
        if g_skip is not None:
            Gd = Gd + g_skip.double()
        if g_direct is not None:
            Gd = Gd + g_direct.double()
        act = torch.relu((xd - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)) if has_bn else xd
        want_w = torch.nn.grad.conv2d_weight(act, (32, I, 3, 3), Gd, padding=1)
        want_b = Gd.sum((0, 2, 3))
        # the bar of a sum of n products: 1e-5 of the largest sum of |G| |act| over a tap; 2e-5 of the largest sum of |G| for the bias sums
        mag = float(torch.nn.grad.conv2d_weight(act.abs(), (32, I, 3, 3), Gd.abs(), padding=1).max())
        magb = float(Gd.abs().sum((0, 2, 3)).max())
        kw = dict(in_=x, weight=torch.zeros(32, I, 3, 3, device=DEV), out=out, g_skip=g_skip, g_direct=g_direct)
        if src:
            kw.update(gn_src=gn_src, cbn_gamma=cgamma, cbn_save_mean=cmean.float(), cbn_save_invstd=cinvstd.float(), cbn_sum_g=cs1.view(-1), cbn_sum_gx=cs2.view(-1))
        if has_bn:
            kw.update(bn_gamma=gamma, bn_beta=beta, bn_save_mean=mean.float(), bn_save_invstd=invstd.float())
        layers.append((kw, want_w, want_b, mag, magb))
    _layers[key] = layers
    return layers


def _run(pkg, layers, on, B, I, H, W, slabs):
    """one launch over `layers` (slabs None: nf_conv_bn_wgrad_multi and its own slab count; else the table form) -> per layer
    (summed weight gradient, summed bias sums, the raw slabs, the raw bias replicas)"""
    fc = importlib.import_module(pkg.__name__ + '.fused_conv')
    N = pkg._native
    _cfg(pkg, on, 0, 0)
    nl = len(layers)
    ns = int(N.load().nf_conv_wgrad_slabs(B, H, W, nl)) if slabs is None else slabs
    arr = (fc.ConvBwdDesc * nl)()
    regions, gbs, keep = [], [], []
    for i, (kw, *_rest) in enumerate(layers):
        region = torch.full((ns * 32 * I * 9, ), float('nan'), device=DEV)
        gb = torch.zeros(R * 256, device=DEV)
        d = fc._desc(fc.ConvBwdDesc, g_weff=region, g_bias=gb, **kw)
        ctypes.memmove(ctypes.addressof(arr) + i * ctypes.sizeof(fc.ConvBwdDesc), ctypes.addressof(d), ctypes.sizeof(fc.ConvBwdDesc))
        regions.append(region)
        gbs.append(gb)
        keep.append(d)
    if slabs is None:
        N.call('nf_conv_bn_wgrad_multi', ctypes.addressof(arr), nl, B, I, 32, H, W, 3, N.stream())
    else:
        tab = torch.empty(nl * ctypes.sizeof(fc.ConvBwdDesc), dtype=torch.uint8, device=DEV)
        keep.append(tab)
        N.call('nf_conv_bn_wgrad_table', ctypes.addressof(arr), tab.data_ptr(), nl, ns, B, I, 32, H, W, 3, N.stream())
    outs = []
    for region, gb in zip(regions, gbs):
        g_w = torch.empty(32, I, 3, 3, device=DEV)
        fc._slab_sum([(region, g_w, g_w.numel(), g_w.numel(), ns, False, 9)])
        outs.append((g_w, gb.view(R, 256).sum(0)[:32].clone(), region, gb))
    torch.cuda.synchronize()
    return outs


# B, I, H, W, layers, G form, slabs (None: nf_conv_bn_wgrad_multi; else nf_conv_bn_wgrad_table with that many slabs), ordered mode
CASES = [
    # 16 x 16, B = 3: 6 tiles -> 6 / 3 / 2 / 1 tiles per workgroup
    (3, 32, 16, 16, 2, SRC_SKIP, 1, False), (3, 6, 16, 16, 1, SRC, 2, False), (3, 17, 16, 16, 2, DIRECT, 3, False), (3, 32, 16, 16, 1, SRC, 6, False),
    (3, 32, 16, 16, 3, SRC_SKIP, None, False),
    # 16 x 16, B = 7: 14 tiles -> 14 / 7 / 5, 5, 4 / 3, 3, 2, 2, 2, 2 tiles per workgroup
    (7, 17, 16, 16, 1, SRC_SKIP, 1, False), (7, 32, 16, 16, 2, SRC, 2, False), (7, 32, 16, 16, 1, DIRECT, 3, False), (7, 6, 16, 16, 2, SRC_SKIP, 6, False),
    (7, 32, 16, 16, 2, SRC, None, False),
    # 8 x 8 (two samples per tile): B = 3 is 192 pixels, the second tile half empty; B = 1 half a tile
    (3, 32, 8, 8, 2, SRC_SKIP, 1, False), (3, 17, 8, 8, 1, SRC, None, False), (1, 32, 8, 8, 1, SRC_SKIP, None, False), (1, 6, 8, 8, 2, DIRECT, 1, False),
    # halo rows at the top and bottom tile of a sample: 16 x 16 with B = 1 (two tiles of one sample: the first has only a bottom halo
    # row, the second only a top one), 32 x 16 with B = 1 and 2 (four tiles per sample: the middle ones have both)
    (1, 32, 16, 16, 1, SRC_SKIP, 1, False), (1, 17, 16, 16, 2, SRC, None, False), (1, 32, 32, 16, 1, SRC, 1, False), (2, 6, 32, 16, 1, SRC_SKIP, 3, False),
    (1, 32, 32, 16, 2, DIRECT, None, False),
    # maps that are not square: (16, 8) is one sixteen-row tile per sample, (8, 16) one eight-row tile
    (2, 32, 16, 8, 2, SRC_SKIP, 1, False), (2, 17, 16, 8, 1, DIRECT, None, False), (3, 6, 8, 16, 1, SRC, 1, False),
    # more than sixteen layers in one table launch
    (2, 32, 8, 8, 17, SRC, 1, False),
    # the ordered mode, one case of each G form
    (3, 32, 16, 16, 2, DIRECT, 2, True), (7, 32, 16, 16, 2, SRC, 3, True), (3, 17, 8, 8, 2, SRC_SKIP, None, True),
]


# 32 x 32 with B = 1 (eight 128-pixel tiles of four rows): not the bulk kernel's (W = 32) -- the launch must go to conv_bn.hip, whole
WIDE = [(1, 32, 32, 32, 1, SRC, 1, False), (1, 6, 32, 32, 1, SRC_SKIP, 3, False), (1, 32, 32, 32, 2, DIRECT, None, False)]


@pytest.mark.parametrize('B,I,H,W,nl,form,slabs,det', WIDE)
def test_maps_32_wide_are_handed_to_the_per_layer_kernel(bulk, B, I, H, W, nl, form, slabs, det):
    _check(bulk, B, I, H, W, nl, form, slabs, det, 0)


@pytest.mark.parametrize('B,I,H,W,nl,form,slabs,det', CASES)
def test_bulk_weight_gradient_tile_pipeline(bulk, B, I, H, W, nl, form, slabs, det):
    _check(bulk, B, I, H, W, nl, form, slabs, det, 1)


def _check(bulk, B, I, H, W, nl, form, slabs, det, plan):
    N = bulk._native
    _cfg(bulk, 1, 0, 0)
    assert int(N.load().nf_conv_bulk_wgrad_plan(B, I, 32, H, W, 3)) == plan, 'k_conv3_bulk_wgrad %s this shape' % ('does not run' if plan else 'runs')
    layers = _make_layers(B, I, H, W, nl, form)
    was = N.deterministic()
    try:
        if det:
            N.deterministic(True)
        got = _run(bulk, layers, 1, B, I, H, W, slabs)
        again = _run(bulk, layers, 1, B, I, H, W, slabs)
        old = _run(bulk, layers, 0, B, I, H, W, slabs)
        if det:
            assert N.deterministic_timeouts() == 0
    finally:
        N.deterministic(was)
    for k, ((kw, want_w, want_b, mag, magb), (gw, gb, region, rep), (gw2, gb2, region2, rep2), (ow, ob, _r, _g)) in enumerate(zip(layers, got, again, old)):
        ew64, ewold = float((gw.double() - want_w).abs().max()), float((gw - ow).abs().max())
        eb64, ebold = float((gb.double() - want_b).abs().max()), float((gb - ob).abs().max())
        print('layer %d: g_weff vs float64 %.3e, vs per-layer kernel %.3e (bar %.3e); g_bias vs float64 %.3e, vs per-layer kernel %.3e (bar %.3e)'
              % (k, ew64, ewold, 1e-5 * max(1.0, mag), eb64, ebold, 2e-5 * max(1.0, magb)))
        assert bool(torch.isfinite(region).all()), 'a slab element was not written'
        assert ew64 <= 1e-5 * max(1.0, mag), ('g_weff vs float64', k, ew64, mag)
        assert ewold <= 1e-5 * max(1.0, mag), ('g_weff vs per-layer kernel', k, ewold, mag)
        assert eb64 <= 2e-5 * max(1.0, magb), ('g_bias vs float64', k, eb64, magb)
        assert ebold <= 2e-5 * max(1.0, magb), ('g_bias vs per-layer kernel', k, ebold, magb)
        assert torch.equal(region, region2), ('slabs differ between two runs from the same inputs', k)
        if det:
            assert torch.equal(rep, rep2), ('ordered mode: bias sums differ between two runs from the same inputs', k)
