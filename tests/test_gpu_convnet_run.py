"""nf_convnet_chain_fwd_run / nf_convnet_chain_bwd_run through the C ABI: ONE launch over n flow steps against n calls of the
single-step entry points in the same order -- the contract of include/nfhip.h is "the same, bit for bit", so every output and
by-product is compared with torch.equal.  Random weights, the steps chained as a model chains them (forward: hd_x of step s + 1 is
cp_y of step s; backward: hd_g_h of the step in front is cp_g_z of the step behind), coupling and head in the launch, packed weight
images (one case with the kernels splitting the weights themselves), all steps of a side sharing ONE exchange-slot buffer under
their own generations, as a trainer step shares it.

The backward comparison runs in the ordered mode (_native.deterministic): cp_g_a / cp_g_c are sums over the workgroups by float
atomics, which race in the default mode -- two single launches from the same inputs do not agree in their last bit there, so only
the ordered mode gives that pair a bitwise meaning.  Everything else is ordered by construction in either mode."""
import ctypes
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NL, NB = 6, 5


def _mods(pkg):
    return (importlib.import_module(pkg.__name__ + '.fused_conv'), importlib.import_module(pkg.__name__ + '.fused'), pkg._native)


def _full_shape(I0, H, W, mode, Nn):
    return (2 * I0, H, W) if mode == Nn.SPLIT_CHANNEL else (I0 // 2, 2 * H, 2 * W)


class _Side:
    """n chained steps of one shape: parameters and forward inputs drawn from ``seed`` (two sides of one seed are identical)"""

    def __init__(self, pkg, n, I0, O, H, W, B, mode, odd0, seed, packed=True):
        fc, fused, Nn = _mods(pkg)
        self.fc, self.Nn, self.n, self.args = fc, Nn, n, (B, I0, O, H, W)
        self.mode, self.packed = mode, packed
        g = torch.Generator(device=DEV).manual_seed(seed)
        rn = lambda *s, k=1.0: torch.randn(*s, device=DEV, generator=g) * k
        ru = lambda *s: torch.rand(*s, device=DEV, generator=g) + 0.5
        C, Hf, Wf = _full_shape(I0, H, W, mode, Nn)
        self.full = (B, C, Hf, Wf)
        R = fused.R
        img = Nn.header_constant('NF_CONV_PACK_IMAGE_FLOATS')
        self.x0 = rn(B, C, Hf, Wf)
        self.ld = torch.zeros(B, device=DEV)
        self.slots = torch.zeros(Nn.header_constant('NF_CONVNET_WS_FLOATS'), device=DEV)
        self.steps = []
        packs = []
        for s in range(n):
            t = {}
            t['w'] = [rn(32, I0, 3, 3, k=0.1)] + [rn(32, 32, 3, 3, k=0.06) for _ in range(4)] + [rn(O, 32, 1, 1, k=0.05)]
            t['b'] = [rn(32, k=0.1) for _ in range(5)] + [rn(O, k=0.1)]
            t['gamma'], t['beta'] = [ru(32) for _ in range(NB)], [rn(32, k=0.1) for _ in range(NB)]
            t['rmean'], t['rvar'] = [rn(32, k=0.1) for _ in range(NB)], [ru(32) for _ in range(NB)]
            t['nbt'] = [torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(NB)]
            t['hd_ls'], t['hd_bias'], t['hd_log_s'] = rn(C, k=0.1), rn(C, k=0.1), rn(C, k=0.1)
            t['hd_W'] = (torch.eye(C, device=DEV) + rn(C, C, k=0.1)).contiguous()
            t['cp_a'], t['cp_c'] = torch.full((1, ), 0.5, device=DEV), torch.full((1, ), 0.1, device=DEV)
            t['odd'] = (odd0 + s) & 1
            # written by the forward
            t['acts'] = [torch.full((B, 32, H, W), float('nan'), device=DEV) for _ in range(NB)]
            t['out'] = torch.full((B, O, H, W), float('nan'), device=DEV)
            t['save_mean'] = [torch.full((32, ), float('nan'), device=DEV) for _ in range(NB)]
            t['save_invstd'] = [torch.full((32, ), float('nan'), device=DEV) for _ in range(NB)]
            t['z'] = torch.full(self.full, float('nan'), device=DEV)
            t['y'] = torch.full(self.full, float('nan'), device=DEV)
            t['x1'] = torch.full((B, I0, H, W), float('nan'), device=DEV)
            t['pk'] = []
            for w in t['w']:
                k = int(Nn.load().nf_conv_weight_pack_images(w.shape[0], w.shape[1], w.shape[2]))
                assert k > 0
                buf = torch.empty(k * img, device=DEV)
                t['pk'].append(buf)
                packs.append(fc.ConvPackDesc(w.data_ptr(), buf.data_ptr(), w.shape[0], w.shape[1], w.shape[2], 0))
            self.steps.append(t)
        if packed:
            arr = (fc.ConvPackDesc * len(packs))(*packs)
            Nn.call('nf_conv_weight_pack', ctypes.addressof(arr), len(packs), Nn.stream())
        self.R = R

    def fwd_descs(self, gen0=1):
        out = []
        for s, t in enumerate(self.steps):
            d = self.fc.ConvNetDesc()
            d.x = t['x1'].data_ptr()
            for i in range(NL):
                d.w[i], d.b[i] = t['w'][i].data_ptr(), t['b'][i].data_ptr()
                if self.packed:
                    d.wpk[i] = t['pk'][i].data_ptr()
            for j in range(NB):
                d.gamma[j], d.beta[j], d.rmean[j], d.rvar[j] = (t[k][j].data_ptr() for k in ('gamma', 'beta', 'rmean', 'rvar'))
                d.nbt[j], d.acts[j] = t['nbt'][j].data_ptr(), t['acts'][j].data_ptr()
                d.save_mean[j], d.save_invstd[j] = t['save_mean'][j].data_ptr(), t['save_invstd'][j].data_ptr()
            d.out, d.ws_zero, d.ws_gen = t['out'].data_ptr(), self.slots.data_ptr(), gen0 + s
            d.cp_z, d.cp_y, d.cp_ld = t['z'].data_ptr(), t['y'].data_ptr(), self.ld.data_ptr()
            d.cp_a, d.cp_c = t['cp_a'].data_ptr(), t['cp_c'].data_ptr()
            d.cp_mode, d.cp_odd, d.cp_C, d.cp_inverse = self.mode, t['odd'], self.full[1], 0
            d.hd_x = (self.x0 if s == 0 else self.steps[s - 1]['y']).data_ptr()
            d.hd_ls, d.hd_bias, d.hd_W, d.hd_log_s = (t[k].data_ptr() for k in ('hd_ls', 'hd_bias', 'hd_W', 'hd_log_s'))
            d.hd_x1 = t['x1'].data_ptr()
            out.append(d)
        return out

    def fwd_outputs(self):
        o = {'ld': self.ld}
        for s, t in enumerate(self.steps):
            for k in ('y', 'z', 'out', 'x1'):
                o['%s[%d]' % (k, s)] = t[k]
            for k in ('acts', 'save_mean', 'save_invstd', 'rmean', 'rvar', 'nbt'):
                for j in range(NB):
                    o['%s[%d][%d]' % (k, s, j)] = t[k][j]
        return o

    def bwd_buffers(self, seed):
        """gradient inputs (drawn from ``seed``) and output buffers of one backward over the forward products of this side"""
        B, I0, O, H, W = self.args
        g = torch.Generator(device=DEV).manual_seed(seed)
        bw = {'g_y': torch.randn(self.full, device=DEV, generator=g), 'g_ld': torch.randn(B, device=DEV, generator=g), 'k': []}
        for k in range(self.n):
            nan = lambda *s: torch.full(s, float('nan'), device=DEV)
            bw['k'].append(dict(
                gn=[nan(B, 32, H, W) for _ in range(NB)], sum_g=[torch.zeros(self.R * 32, device=DEV) for _ in range(NB)],
                sum_gx=[torch.zeros(self.R * 32, device=DEV) for _ in range(NB)], g_store=[nan(B, 32, H, W) for _ in range(2)],
                g_gamma=[torch.zeros(32, device=DEV) for _ in range(NB)], g_beta=[torch.zeros(32, device=DEV) for _ in range(NB)],
                g_z=nan(*self.full), g_out=nan(B, O, H, W), g_a=torch.zeros(1, device=DEV), g_c=torch.zeros(1, device=DEV),
                g_y=(bw['g_y'] if k == 0 else nan(*self.full))))
        return bw

    def bwd_descs(self, bw, gen0):
        """descriptors in BACKWARD order: entry k is forward step n - 1 - k"""
        B, I0, O, H, W = self.args
        out = []
        for k in range(self.n):
            t, u = self.steps[self.n - 1 - k], bw['k'][k]
            d = self.fc.ConvNetBwdDesc()
            for i in range(NL):
                d.w[i] = t['w'][i].data_ptr()
                if self.packed:
                    d.wpk[i] = t['pk'][i].data_ptr()
            for j in range(NB):
                d.gamma[j], d.beta[j] = t['gamma'][j].data_ptr(), t['beta'][j].data_ptr()
                d.save_mean[j], d.save_invstd[j] = t['save_mean'][j].data_ptr(), t['save_invstd'][j].data_ptr()
                d.acts[j], d.gn[j] = t['acts'][j].data_ptr(), u['gn'][j].data_ptr()
                d.sum_g[j], d.sum_gx[j] = u['sum_g'][j].data_ptr(), u['sum_gx'][j].data_ptr()
                d.g_gamma[j], d.g_beta[j] = u['g_gamma'][j].data_ptr(), u['g_beta'][j].data_ptr()
            d.g_store[0], d.g_store[1] = u['g_store'][0].data_ptr(), u['g_store'][1].data_ptr()
            d.ws_zero, d.ws_gen = self.slots.data_ptr(), gen0 + k
            d.cp_g_y, d.cp_g_ld, d.cp_z, d.cp_out = u['g_y'].data_ptr(), bw['g_ld'].data_ptr(), t['z'].data_ptr(), t['out'].data_ptr()
            d.cp_a, d.cp_c, d.cp_g_z, d.cp_g_out = t['cp_a'].data_ptr(), t['cp_c'].data_ptr(), u['g_z'].data_ptr(), u['g_out'].data_ptr()
            d.cp_g_a, d.cp_g_c = u['g_a'].data_ptr(), u['g_c'].data_ptr()
            d.cp_mode, d.cp_odd, d.cp_C = self.mode, t['odd'], self.full[1]
            if k > 0:                                   # the head of the step behind (forward step n - k), transposed in the prologue
                h = self.steps[self.n - k]
                d.hd_g_h, d.hd_W, d.hd_ls = bw['k'][k - 1]['g_z'].data_ptr(), h['hd_W'].data_ptr(), h['hd_ls'].data_ptr()
            out.append(d)
        return out

    @staticmethod
    def bwd_outputs(bw):
        o = {}
        for k, u in enumerate(bw['k']):
            for name in ('g_z', 'g_out', 'g_a', 'g_c', 'g_y'):
                o['%s[%d]' % (name, k)] = u[name]
            for name in ('gn', 'sum_g', 'sum_gx', 'g_gamma', 'g_beta', 'g_store'):
                for j, v in enumerate(u[name]):
                    o['%s[%d][%d]' % (name, k, j)] = v
        return o


def _array(descs):
    arr = (type(descs[0]) * len(descs))()
    size = ctypes.sizeof(descs[0])
    for i, d in enumerate(descs):
        ctypes.memmove(ctypes.addressof(arr) + i * size, ctypes.addressof(d), size)
    return arr


def _fwd_singly(side, training, eps=1e-5, mom=0.1):
    for d in side.fwd_descs():
        side.Nn.call('nf_convnet_chain_fwd', ctypes.addressof(d), *side.args, training, eps, mom, side.Nn.stream())


def _fwd_run(side, training, eps=1e-5, mom=0.1):
    arr = _array(side.fwd_descs())
    side.Nn.call('nf_convnet_chain_fwd_run', ctypes.addressof(arr), side.n, *side.args, training, eps, mom, side.Nn.stream())


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert not torch.isnan(a[k].float()).any(), k + ' was not written'
        assert torch.equal(a[k], b[k]), '%s differs: max |d| = %g' % (k, float((a[k].float() - b[k].float()).abs().max()))


def _compare(pkg, n, I0, O, H, W, B, mode_name, odd0, training, packed=True):
    fc, fused, Nn = _mods(pkg)
    mode = Nn.SPLIT_CHANNEL if mode_name == 'channel' else Nn.SPLIT_CHECKER
    assert int(Nn.load().nf_convnet_chain_usable(B, I0, O, H, W))
    one = _Side(pkg, n, I0, O, H, W, B, mode, odd0, seed=11, packed=packed)
    run = _Side(pkg, n, I0, O, H, W, B, mode, odd0, seed=11, packed=packed)
    _fwd_singly(one, training)
    _fwd_run(run, training)
    torch.cuda.synchronize()
    assert Nn.persistent_timeouts() == 0
    _assert_same(one.fwd_outputs(), run.fwd_outputs())
    # backward over the forward products of ``one`` (read-only for both)
    was = Nn.deterministic()
    Nn.deterministic(True)
    try:
        bw1, bw2 = one.bwd_buffers(5), one.bwd_buffers(5)
        for d in one.bwd_descs(bw1, n + 1):
            Nn.call('nf_convnet_chain_bwd', ctypes.addressof(d), *one.args, training, Nn.stream())
        torch.cuda.synchronize()
        arr = _array(one.bwd_descs(bw2, 2 * n + 1))
        Nn.call('nf_convnet_chain_bwd_run', ctypes.addressof(arr), n, *one.args, training, Nn.stream())
        torch.cuda.synchronize()
    finally:
        Nn.deterministic(was)
    assert Nn.persistent_timeouts() == 0 and Nn.deterministic_timeouts() == 0
    _assert_same(_Side.bwd_outputs(bw1), _Side.bwd_outputs(bw2))


# (I0, O, H, W), B, n, split, odd of the first step, training -- smallest shapes first
CASES = [
    ((24, 48, 8, 8), 5, 3, 'channel', 0, 1),        # 64-pixel tiles, 5 workgroups: a real exchange, odd count
    ((96, 192, 4, 4), 3, 3, 'checker', 1, 1),       # 32-pixel tiles, two samples per tile, the last tile half empty
    ((24, 48, 8, 8), 5, 3, 'checker', 1, 0),        # evaluation mode: no exchange at all
    ((96, 192, 4, 4), 3, 3, 'checker', 0, 0),
    ((8, 16, 4, 8), 4, 2, 'channel', 1, 1),         # a geometry without an instantiation of its own
    ((96, 192, 4, 4), 64, 4, 'checker', 0, 1),      # 32 workgroups
    ((24, 48, 8, 8), 64, 1, 'channel', 0, 1),       # 64 workgroups, n = 1
]


@pytest.mark.parametrize('shape,B,n,split,odd0,training', CASES)
def test_run_equals_single_launches(pkg, shape, B, n, split, odd0, training):
    _compare(pkg, n, *shape, B, split, odd0, training)


def test_run_of_the_maximum_length(pkg):
    Nn = pkg._native
    _compare(pkg, Nn.header_constant('NF_CONVNET_RUN_MAX'), 24, 48, 8, 8, 64, 'channel', 1, 1)


def test_run_with_weights_split_in_the_kernel(pkg):
    _compare(pkg, 2, 24, 48, 8, 8, 5, 'channel', 0, 1, packed=False)


def test_bad_arguments(pkg):
    fc, fused, Nn = _mods(pkg)
    lib = Nn.load()
    bad = Nn.header_constant('NF_E_BADARG')
    nmax = Nn.header_constant('NF_CONVNET_RUN_MAX')
    side = _Side(pkg, 2, 24, 48, 8, 8, 5, Nn.SPLIT_CHANNEL, 0, seed=3)
    _fwd_singly(side, 1)                                # (forward products for the backward descriptors)
    bw = side.bwd_buffers(1)

    def fwd(descs, n, args=side.args):
        arr = _array(descs)
        return lib.nf_convnet_chain_fwd_run(ctypes.addressof(arr), n, *args, 1, 1e-5, 0.1, Nn.stream())

    def bwd(descs, n, args=side.args):
        arr = _array(descs)
        return lib.nf_convnet_chain_bwd_run(ctypes.addressof(arr), n, *args, 1, Nn.stream())

    assert fwd(side.fwd_descs(), 0) == bad and bwd(side.bwd_descs(bw, 9), 0) == bad
    assert fwd(side.fwd_descs(), nmax + 1) == bad and bwd(side.bwd_descs(bw, 9), nmax + 1) == bad
    ds = side.fwd_descs()
    ds[1].hd_x = None                                   # the head in one descriptor only
    assert fwd(ds, 2) == bad
    ds = side.fwd_descs()
    for i in range(NL):
        ds[1].wpk[i] = None                             # packed images in one descriptor only
    assert fwd(ds, 2) == bad
    ds = side.fwd_descs()
    ds[0].cp_z = ds[0].hd_x = None                      # no coupling
    assert fwd(ds, 2) == bad
    ds = side.bwd_descs(bw, 9)
    for i in range(NL):
        ds[0].wpk[i] = None
    assert bwd(ds, 2) == bad
    ds = side.bwd_descs(bw, 9)
    ds[1].cp_g_y = None
    assert bwd(ds, 2) == bad
    # a sample over two workgroups (16 x 16 maps on 128-pixel tiles): the halo hand-over takes one step per launch
    halo = _Side(pkg, 2, 6, 12, 16, 16, 4, Nn.SPLIT_CHANNEL, 0, seed=4)
    assert int(lib.nf_convnet_chain_ws_floats(4, 6, 12, 16, 16)) > Nn.header_constant('NF_CONVNET_WS_FLOATS')
    assert fwd(halo.fwd_descs(), 2, halo.args) == bad
    assert bwd(halo.bwd_descs(halo.bwd_buffers(1), 9), 2, halo.args) == bad
    torch.cuda.synchronize()
    assert Nn.persistent_timeouts() == 0
