"""
torch.autograd.Function wrappers over the C ABI of libnfhip.so -- the only place where the product path touches
the kernels.  Forward-direction ops carry hand-written autograd (backward kernels); inverse-direction ops
(sampling, ``layer.backward`` in the reference's naming) run without building a graph, like the reference's
own ``torch.no_grad`` inverse of the invertible 1x1 convolution (flows/modules.py:485).

``ld`` (``log_df_dz``) is updated IN PLACE and returned, as the reference does (coupling.py:110,
modules.py:249,305,480); only the returned tensor is contractual.
"""
import ctypes
import os

import torch

from . import _native as N
from . import workspace as WS

MODE_OF = {'1d': N.SPLIT_1D, 'checkerboard': N.SPLIT_CHECKER, 'channelwise': N.SPLIT_CHANNEL, 'none': N.SPLIT_NONE}


def _bchw(z):
    """(B, C, H, W) view of the problem: 2-D data is (B, D, 1, 1)."""
    if z.dim() == 2:
        return z.shape[0], z.shape[1], 1, 1
    if z.dim() == 4:
        return tuple(z.shape)
    raise ValueError('flow tensors are (B, D) or (B, C, H, W), got shape %s' % (tuple(z.shape), ))


def _half_shape(z, mode):
    B, C, H, W = _bchw(z)
    if mode == N.SPLIT_1D:
        return (B, C // 2)
    if mode == N.SPLIT_CHECKER:
        return (B, 2 * C, H // 2, W // 2)
    if mode == N.SPLIT_CHANNEL:
        return (B, C // 2, H, W)
    return tuple(z.shape)


def _contig(t):
    return t if t.is_contiguous() else t.contiguous()


def grad_sink(p):
    """the buffer a hand-written backward may accumulate into directly instead of returning a temporary: ``p.grad`` of a
    parameter that a GradBucket tagged (``_nf_direct_grad``).  Same ``+=`` semantics as autograd's AccumulateGrad, one
    launch less per parameter.  None -> return the gradient to autograd as usual."""
    if not getattr(p, '_nf_direct_grad', False):
        return None
    g = p.grad
    if g is None or not g.is_contiguous() or g.dtype != torch.float32 or g.device != p.device:
        return None
    return g


def _sinks(*params):
    """all-or-nothing list of gradient sinks for the parameters of one op."""
    out = [grad_sink(p) for p in params]
    return out if all(t is not None for t in out) else None


def _owned_ld(ld, *others):
    """ld is mutated in place; a leaf that requires grad (never the case in the models) gets copied first."""
    if ld.requires_grad and ld.is_leaf:
        return ld.clone()
    return ld


# ----------------------------------------------------------------------------------------------------------------------
# index maps
# ----------------------------------------------------------------------------------------------------------------------
class _HalfGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, which, mode, odd):
        z = _contig(z)
        B, C, H, W = _bchw(z)
        out = torch.empty(_half_shape(z, mode), dtype=z.dtype, device=z.device)
        N.call('nf_half_gather', N.ptr(z), N.ptr(out), which, mode, int(odd), B, C, H, W, N.stream())
        ctx.meta = (which, mode, int(odd), tuple(z.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        which, mode, odd, shape = ctx.meta
        g = _contig(g)
        full = torch.empty(shape, dtype=g.dtype, device=g.device)
        B, C, H, W = _bchw(full)
        N.call('nf_half_scatter', N.ptr(g), N.ptr(full), which, mode, odd, B, C, H, W, N.stream())
        return full, None, None, None


def half_gather(z, which, mode, odd):
    """contiguous z0 (which=0, transformed half) or z1 (which=1, conditioning half) of the split map."""
    return _HalfGather.apply(z, which, mode, odd)


class _SpaceDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, to_depth):
        z = _contig(z)
        B, C, H, W = z.shape
        if to_depth:
            out = torch.empty((B, 4 * C, H // 2, W // 2), dtype=z.dtype, device=z.device)
            N.call('nf_squeeze2d', N.ptr(z), N.ptr(out), B, C, H, W, N.stream())
        else:
            out = torch.empty((B, C // 4, 2 * H, 2 * W), dtype=z.dtype, device=z.device)
            N.call('nf_unsqueeze2d', N.ptr(z), N.ptr(out), B, C // 4, 2 * H, 2 * W, N.stream())
        ctx.to_depth = to_depth
        return out

    @staticmethod
    def backward(ctx, g):
        return _SpaceDepth.apply(g, not ctx.to_depth), None


def squeeze2d(z):
    if z.dim() != 4 or z.shape[2] % 2 or z.shape[3] % 2:
        raise ValueError('squeeze2d needs (B, C, even H, even W)')
    return _SpaceDepth.apply(z, True)


def unsqueeze2d(z):
    if z.dim() != 4 or z.shape[1] % 4:
        raise ValueError('unsqueeze2d needs (B, 4C, h, w)')
    return _SpaceDepth.apply(z, False)


# ----------------------------------------------------------------------------------------------------------------------
# affine coupling
# ----------------------------------------------------------------------------------------------------------------------
class _AffineCoupling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, t, s_raw, pbs, a, c, ld, mode, odd):
        B, C, H, W = _bchw(z)
        y = torch.empty_like(z)
        N.call('nf_affine_coupling_fwd', N.ptr(z), N.ptr(t), N.ptr(s_raw), pbs, N.ptr(a), N.ptr(c), N.ptr(y),
               N.ptr(ld), mode, int(odd), 0, B, C, H, W, N.stream())
        ctx.save_for_backward(z, t, s_raw, a, c)
        ctx.meta = (pbs, mode, int(odd))
        ctx.sinks = _sinks(a, c)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        z, t, s_raw, a, c = ctx.saved_tensors
        pbs, mode, odd = ctx.meta
        B, C, H, W = _bchw(z)
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_z = torch.empty_like(z)
        g_t = torch.empty_like(t)
        g_s = torch.empty_like(s_raw)
        if ctx.sinks is not None:
            pa, pc, ga, gc = ctx.sinks[0].data_ptr(), ctx.sinks[1].data_ptr(), None, None
        else:
            g_ac = WS.zeros(2, z.device)
            pa, pc = g_ac.data_ptr(), g_ac.data_ptr() + 4
            ga, gc = g_ac[0:1].view_as(a), g_ac[1:2].view_as(c)
        N.call('nf_affine_coupling_bwd', N.ptr(g_y), N.ptr(g_ld), N.ptr(z), N.ptr(t), N.ptr(s_raw), pbs, N.ptr(a),
               N.ptr(c), N.ptr(g_z), N.ptr(g_t), N.ptr(g_s), pa, pc, mode, odd, B, C, H, W, N.stream())
        return g_z, g_t, g_s, None, ga, gc, g_ld, None, None


class _AffineCouplingPacked(torch.autograd.Function):
    """conditioner output packed as one tensor (B, 2*Ch, h, w): t = params[:, :Ch], s_raw = params[:, Ch:]."""

    @staticmethod
    def forward(ctx, z, params, a, c, ld, mode, odd):
        B, C, H, W = _bchw(z)
        n_half = params.numel() // (2 * B) if B else 0
        y = torch.empty_like(z)
        N.call('nf_affine_coupling_fwd', N.ptr(z), N.ptr(params), params.data_ptr() + 4 * n_half, 2 * n_half, N.ptr(a),
               N.ptr(c), N.ptr(y), N.ptr(ld), mode, int(odd), 0, B, C, H, W, N.stream())
        ctx.save_for_backward(z, params, a, c)
        ctx.meta = (n_half, mode, int(odd))
        ctx.sinks = _sinks(a, c)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        z, params, a, c = ctx.saved_tensors
        n_half, mode, odd = ctx.meta
        B, C, H, W = _bchw(z)
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_z = torch.empty_like(z)
        g_p = torch.empty_like(params)
        if ctx.sinks is not None:
            pa, pc, ga, gc = ctx.sinks[0].data_ptr(), ctx.sinks[1].data_ptr(), None, None
        else:
            g_ac = WS.zeros(2, z.device)
            pa, pc = g_ac.data_ptr(), g_ac.data_ptr() + 4
            ga, gc = g_ac[0:1].view_as(a), g_ac[1:2].view_as(c)
        N.call('nf_affine_coupling_bwd', N.ptr(g_y), N.ptr(g_ld), N.ptr(z), N.ptr(params),
               params.data_ptr() + 4 * n_half, 2 * n_half, N.ptr(a), N.ptr(c), N.ptr(g_z), N.ptr(g_p),
               g_p.data_ptr() + 4 * n_half, pa, pc, mode, odd, B, C, H, W, N.stream())
        return g_z, g_p, ga, gc, g_ld, None, None


def affine_coupling(z, params, s_log_scale, s_bias, ld, mode, odd, inverse=False):
    """AbstractCoupling.forward/backward around AffineCoupling._transform/_inverse_transform, given ``params`` =
    conditioner(z1).  (flows/coupling.py:32-43, :104-122)"""
    z, params = _contig(z), _contig(params)
    half = _half_shape(z, mode)
    if tuple(params.shape) != (half[0], 2 * half[1]) + tuple(half[2:]):
        raise ValueError('conditioner output has shape %s, expected %s' % (tuple(params.shape),
                                                                         (half[0], 2 * half[1]) + tuple(half[2:])))
    ld = _owned_ld(ld)
    if not inverse:
        return _AffineCouplingPacked.apply(z, params, s_log_scale, s_bias, ld, mode, odd)
    with torch.no_grad():
        B, C, H, W = _bchw(z)
        n_half = params.numel() // (2 * B) if B else 0
        y = torch.empty_like(z)
        N.call('nf_affine_coupling_fwd', N.ptr(z), N.ptr(params), params.data_ptr() + 4 * n_half, 2 * n_half,
               N.ptr(s_log_scale), N.ptr(s_bias), N.ptr(y), N.ptr(ld), mode, int(odd), 1, B, C, H, W, N.stream())
    return y, ld


def affine_transform(z, s_raw, t, s_log_scale, s_bias, ld, inverse=False):
    """un-split affine transform with separate scale / shift tensors (MAF: flows/maf.py:103-106, :114-115)."""
    z, s_raw, t = _contig(z), _contig(s_raw), _contig(t)
    ld = _owned_ld(ld)
    pbs = s_raw.numel() // s_raw.shape[0] if s_raw.shape[0] else 0
    if not inverse:
        return _AffineCoupling.apply(z, t, s_raw, pbs, s_log_scale, s_bias, ld, N.SPLIT_NONE, False)
    with torch.no_grad():
        B, C, H, W = _bchw(z)
        y = torch.empty_like(z)
        N.call('nf_affine_coupling_fwd', N.ptr(z), N.ptr(t), N.ptr(s_raw), pbs, N.ptr(s_log_scale), N.ptr(s_bias),
               N.ptr(y), N.ptr(ld), N.SPLIT_NONE, 0, 1, B, C, H, W, N.stream())
    return y, ld


# ----------------------------------------------------------------------------------------------------------------------
# per-channel affine bijectors (ActNorm, flow BatchNorm) and their statistics
# ----------------------------------------------------------------------------------------------------------------------
def _bcp(x):
    B, C = x.shape[0], x.shape[1]
    P = 1
    for d in x.shape[2:]:
        P *= int(d)
    return B, C, P


class _ChanAffine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op, x, ld, p0, p1, p2, p3):
        B, C, P = _bcp(x)
        y = torch.empty_like(x)
        N.call('nf_chan_affine_fwd', op, N.ptr(x), N.ptr(p0), N.ptr(p1), N.ptr(p2), N.ptr(p3), N.ptr(y), N.ptr(ld), 0,
               B, C, P, N.stream())
        ctx.op = op
        ctx.save_for_backward(x, p0, p1, p2, p3)
        ctx.sinks = _sinks(p0, p1) if op == N.OP_ACTNORM else (_sinks(p2, p3) if p2 is not None else None)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        x, p0, p1, p2, p3 = ctx.saved_tensors
        op = ctx.op
        B, C, P = _bcp(x)
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_x = torch.empty_like(x)
        pa, pb = (p0, p1) if op == N.OP_ACTNORM else (p2, p3)
        want = ctx.needs_input_grad[3 if op == N.OP_ACTNORM else 5]
        ga = gb = None
        if want and ctx.sinks is not None:
            ga_ptr, gb_ptr = ctx.sinks[0].data_ptr(), ctx.sinks[1].data_ptr()
        elif want:
            g_ab = WS.zeros(2 * pa.numel(), x.device).view((2, ) + tuple(pa.shape))
            ga_ptr, gb_ptr = g_ab.data_ptr(), g_ab.data_ptr() + 4 * pa.numel()
            ga, gb = g_ab[0], g_ab[1]
        else:
            ga_ptr, gb_ptr = None, None
        N.call('nf_chan_affine_bwd', op, N.ptr(g_y), N.ptr(g_ld), N.ptr(x), N.ptr(p0), N.ptr(p1), N.ptr(p2), N.ptr(p3),
               N.ptr(g_x), ga_ptr, gb_ptr, B, C, P, N.stream())
        if op == N.OP_ACTNORM:
            return None, g_x, g_ld, ga, gb, None, None
        return None, g_x, g_ld, None, None, ga, gb


def chan_affine(op, x, ld, p0, p1, p2=None, p3=None, inverse=False):
    x = _contig(x)
    ld = _owned_ld(ld)
    if not inverse:
        return _ChanAffine.apply(op, x, ld, p0, p1, p2, p3)
    with torch.no_grad():
        B, C, P = _bcp(x)
        y = torch.empty_like(x)
        N.call('nf_chan_affine_fwd', op, N.ptr(x), N.ptr(p0), N.ptr(p1), N.ptr(p2), N.ptr(p3), N.ptr(y), N.ptr(ld), 1,
               B, C, P, N.stream())
    return y, ld


def chan_stats(x):
    """per-channel (sum, sum of squared deviations) over batch and pixels, two passes (no E[x^2]-E[x]^2)."""
    x = _contig(x)
    B, C, P = _bcp(x)
    st = torch.zeros((2, C), dtype=x.dtype, device=x.device)
    N.call('nf_chan_sum', N.ptr(x), st.data_ptr(), B, C, P, N.stream())
    N.call('nf_chan_sqdev', N.ptr(x), st.data_ptr(), st.data_ptr() + 4 * C, B, C, P, N.stream())
    return st, B * P


def actnorm_init_(x, log_scale, bias, eps):
    """data-dependent ActNorm initialisation, writes the parameters in place (flows/modules.py:238-244)."""
    with torch.no_grad():
        st, n = chan_stats(x)
        C = st.shape[1]
        N.call('nf_actnorm_init_finalize', st.data_ptr(), st.data_ptr() + 4 * C, N.ptr(log_scale.data),
               N.ptr(bias.data), float(eps), n, C, N.stream())


def flowbn_update_(x, batch_mean, batch_var, running_mean, running_var, eps, momentum):
    """train-mode statistics of the flow BatchNorm, all buffers written in place (flows/modules.py:284-294)."""
    with torch.no_grad():
        st, n = chan_stats(x)
        C = st.shape[1]
        N.call('nf_flowbn_finalize', st.data_ptr(), st.data_ptr() + 4 * C, N.ptr(batch_mean), N.ptr(batch_var),
               N.ptr(running_mean), N.ptr(running_var), float(eps), float(momentum), n, C, N.stream())


# ----------------------------------------------------------------------------------------------------------------------
# invertible 1x1 convolution
# ----------------------------------------------------------------------------------------------------------------------
class _InvConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, W, ld, log_s):
        B, C, P = _bcp(z)
        y = torch.empty_like(z)
        N.call('nf_invconv_apply', N.ptr(z), N.ptr(W), 0, N.ptr(y), N.ptr(ld), N.ptr(log_s), 1.0, B, C, P, N.stream())
        ctx.save_for_backward(z, W)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        z, W = ctx.saved_tensors
        B, C, P = _bcp(z)
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_z = g_W = g_ls = None
        if ctx.needs_input_grad[0]:
            g_z = torch.empty_like(z)
            N.call('nf_invconv_apply', N.ptr(g_y), N.ptr(W), 1, N.ptr(g_z), None, None, 0.0, B, C, P, N.stream())
        if ctx.needs_input_grad[1]:
            g_W = torch.zeros_like(W)
            N.call('nf_invconv_wgrad', N.ptr(g_y), N.ptr(z), N.ptr(g_W), B, C, P, N.stream())
        if ctx.needs_input_grad[3]:
            g_ls = (g_ld.sum() * float(P)).expand(C)
        return g_z, g_W, g_ld, g_ls


def invconv(z, W, ld, log_s):
    """forward 1x1 convolution y = W z per pixel, ld += P * sum(log_s)  (flows/modules.py:475-480)."""
    return _InvConv.apply(_contig(z), _contig(W), _owned_ld(ld), _contig(log_s))


def invconv_inverse(y, W_inv, ld, log_s):
    """z = W^-1 y per pixel, ld -= P * sum(log_s)  (flows/modules.py:484-497), no autograd like the reference."""
    with torch.no_grad():
        y, W_inv = _contig(y), _contig(W_inv)
        ld = _owned_ld(ld)
        B, C, P = _bcp(y)
        z = torch.empty_like(y)
        N.call('nf_invconv_apply', N.ptr(y), N.ptr(W_inv), 0, N.ptr(z), N.ptr(ld), N.ptr(_contig(log_s)), -1.0, B, C, P,
               N.stream())
    return z, ld


class _InvConvPLU(torch.autograd.Function):
    """whole InvertibleConv1x1.forward: PLU assembly + per-pixel mat-vec + log-det, 2 launches forward, 4 backward."""

    @staticmethod
    def forward(ctx, z, ld, P, L, U, L_mask, U_mask, sign_s, log_s):
        B, C, Px = _bcp(z)
        W = torch.empty((C, C), dtype=z.dtype, device=z.device)
        N.call('nf_invconv_weight_fwd', N.ptr(P), N.ptr(L), N.ptr(U), N.ptr(L_mask), N.ptr(U_mask), N.ptr(sign_s),
               N.ptr(log_s), N.ptr(W), C, N.stream())
        y = torch.empty_like(z)
        N.call('nf_invconv_apply', N.ptr(z), N.ptr(W), 0, N.ptr(y), N.ptr(ld), N.ptr(log_s), 1.0, B, C, Px, N.stream())
        ctx.save_for_backward(z, W, P, L, U, L_mask, U_mask, sign_s, log_s)
        ctx.sinks = _sinks(L, U, log_s)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        z, W, P, L, U, L_mask, U_mask, sign_s, log_s = ctx.saved_tensors
        B, C, Px = _bcp(z)
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_z = None
        if ctx.needs_input_grad[0]:
            g_z = torch.empty_like(z)
            N.call('nf_invconv_apply', N.ptr(g_y), N.ptr(W), 1, N.ptr(g_z), None, None, 0.0, B, C, Px, N.stream())
        g_W = WS.zeros(W.numel(), W.device).view_as(W)
        N.call('nf_invconv_wgrad', N.ptr(g_y), N.ptr(z), N.ptr(g_W), B, C, Px, N.stream())
        direct = ctx.sinks is not None
        g_L, g_U, g_ls = ctx.sinks if direct else (torch.empty_like(L), torch.empty_like(U), torch.empty_like(log_s))
        N.call('nf_invconv_weight_bwd', N.ptr(g_W), N.ptr(P), N.ptr(L), N.ptr(U), N.ptr(L_mask), N.ptr(U_mask),
               N.ptr(sign_s), N.ptr(log_s), N.ptr(g_ld), N.ptr(g_L), N.ptr(g_U), N.ptr(g_ls), int(direct), C, B, Px,
               N.stream())
        if direct:
            return g_z, g_ld, None, None, None, None, None, None, None
        return g_z, g_ld, None, g_L, g_U, None, None, None, g_ls


PLU_MAX_C = 64


class PluHolder:
    """what the per-layer applications leave for the batched PLU backward of the same pass: their incoming log-det gradient
    (g_log_s has a pixels * sum_b g_ld term, modules.py:480) and their batch / pixel counts."""

    def __init__(self, n):
        self.g_ld = [None] * n
        self.meta = [None] * n
        self.pending = []       # heads whose parameter gradients wait for the batched launch (_GlowHeadW.backward -> flush_head_params)


class _InvConvApplyW(torch.autograd.Function):
    """InvertibleConv1x1.forward with the weight W = P L' U' computed elsewhere (fused.plu_weights_all: every layer of the model
    in a few launches): per-pixel mat-vec + log-det forward, transposed mat-vec + weight gradient backward."""

    @staticmethod
    def forward(ctx, z, ld, W, log_s, holder, idx):
        B, C, Px = _bcp(z)
        y = torch.empty_like(z)
        N.call('nf_invconv_apply', N.ptr(z), N.ptr(W), 0, N.ptr(y), N.ptr(ld), N.ptr(log_s), 1.0, B, C, Px, N.stream())
        ctx.save_for_backward(z, W)
        ctx.holder, ctx.idx = holder, idx
        holder.meta[idx] = (B, Px)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        z, W = ctx.saved_tensors
        B, C, Px = _bcp(z)
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_z = None
        if ctx.needs_input_grad[0]:
            g_z = torch.empty_like(z)
            N.call('nf_invconv_apply', N.ptr(g_y), N.ptr(W), 1, N.ptr(g_z), None, None, 0.0, B, C, Px, N.stream())
        g_W = WS.zeros(W.numel(), W.device).view_as(W)
        N.call('nf_invconv_wgrad', N.ptr(g_y), N.ptr(z), N.ptr(g_W), B, C, Px, N.stream())
        ctx.holder.g_ld[ctx.idx] = g_ld
        return g_z, g_ld, g_W, None, None, None


def invconv_apply_w(z, ld, W, log_s, holder, idx):
    return _InvConvApplyW.apply(_contig(z), _owned_ld(ld), W, log_s, holder, idx)


def invconv_plu(z, ld, P, L, U, L_mask, U_mask, sign_s, log_s):
    """InvertibleConv1x1.forward from its stored PLU parameters (flows/modules.py:470-482)."""
    return _InvConvPLU.apply(_contig(z), _owned_ld(ld), P, L, U, L_mask, U_mask, sign_s, log_s)


FLOWBN_FUSED = True           # (internal: image data's flow BatchNorm head in one persistent launch; False = statistics + apply launches)


class _FlowBNHead(torch.autograd.Function):
    """training-mode flow BatchNorm (affine=False) + optional conditioning-half gather: 2 launches forward, 1 backward."""

    @staticmethod
    def forward(ctx, x, ld, log_gamma, beta, batch_mean, batch_var, running_mean, running_var, eps, momentum, mode, odd,
                gather):
        B, C, H, W = _bchw(x)
        y = torch.empty_like(x)
        z1c = torch.empty(_half_shape(x, mode), dtype=x.dtype, device=x.device) if gather else None
        nws = int(N.load().nf_flowbn_head_fused_ws_floats(B, C, H, W)) if (FLOWBN_FUSED and x.dim() == 4) else 0
        if nws > 0:
            # statistics and apply in ONE persistent launch: the workgroups exchange their per-channel sums (csrc/flowbn_head.hip)
            ws = WS.zeros(nws, x.device)
            N.call('nf_flowbn_head_fused', N.ptr(x), N.ptr(log_gamma), N.ptr(beta), N.ptr(batch_mean), N.ptr(batch_var),
                   N.ptr(running_mean), N.ptr(running_var), float(eps), float(momentum), N.ptr(y), N.ptr(z1c), N.ptr(ld), N.ptr(ws),
                   mode, int(odd), B, C, H, W, N.stream())
        else:
            ws = WS.zeros(3 * C, x.device)
            N.call('nf_flowbn_stats', N.ptr(x), N.ptr(running_mean), N.ptr(ws), B, C, H * W, N.stream())
            N.call('nf_flowbn_head_fwd', N.ptr(x), N.ptr(ws), N.ptr(log_gamma), N.ptr(beta), N.ptr(batch_mean),
                   N.ptr(batch_var), N.ptr(running_mean), N.ptr(running_var), float(eps), float(momentum), N.ptr(y),
                   N.ptr(z1c), N.ptr(ld), mode, int(odd), B, C, H, W, N.stream())
        ctx.save_for_backward(batch_var, log_gamma)
        ctx.meta = (mode, int(odd), tuple(x.shape), gather)
        ctx.mark_dirty(ld)
        ctx.set_materialize_grads(False)          # the gathered half has no gradient of its own under the fused image coupling
        if gather:
            return y, z1c, ld
        return y, ld

    @staticmethod
    def backward(ctx, *grads):
        batch_var, log_gamma = ctx.saved_tensors
        mode, odd, shape, gather = ctx.meta
        if gather:
            g_h, g_z1c, g_ld = grads
            g_z1c = _contig(g_z1c) if g_z1c is not None else None
        else:
            (g_h, g_ld), g_z1c = grads, None
        if g_h is None:                            # (grads are not materialised: an unused output arrives as None)
            g_h = torch.zeros(shape, dtype=batch_var.dtype, device=batch_var.device)
        g_h = _contig(g_h)
        B, C, H, W = shape if len(shape) == 4 else (shape[0], shape[1], 1, 1)
        g_x = torch.empty_like(g_h)
        N.call('nf_flowbn_head_bwd', N.ptr(g_h), N.ptr(g_z1c), N.ptr(batch_var), N.ptr(log_gamma), N.ptr(g_x), mode, odd,
               B, C, H, W, N.stream())
        return (g_x, g_ld) + (None, ) * 11


def flowbn_head(x, ld, bn, mode=N.SPLIT_NONE, odd=False, gather=False):
    """train-mode ``BatchNorm.forward`` of a flow BatchNorm with affine=False (+ the split gather of the coupling that
    follows): (y, [z1c,] ld).  flows/modules.py:283-307, flows/coupling.py:33."""
    return _FlowBNHead.apply(_contig(x), _owned_ld(ld), bn.log_gamma, bn.beta, bn.batch_mean, bn.batch_var,
                             bn.running_mean, bn.running_var, bn.eps, bn.momentum, mode, odd, gather)


class _GlowHead(torch.autograd.Function):
    """ActNorm + invertible 1x1 (PLU assembled in-kernel) + conditioning-half gather: 1 launch forward, 2 backward."""

    @staticmethod
    def forward(ctx, z, ld, log_scale, bias, P, L, U, L_mask, U_mask, sign_s, log_s, mode, odd, bwd_defer=False, defer=False):
        B, C, H, W = _bchw(z)
        ctx.bwd_defer = bool(bwd_defer)
        h = torch.empty_like(z)
        z1c = torch.empty(_half_shape(z, mode), dtype=z.dtype, device=z.device)
        Wm = torch.empty((C, C), dtype=z.dtype, device=z.device)
        if defer:
            # (as in _GlowHeadW.forward: the coupling's chain launch performs this head in its prologue -- nf_cc_head_small_fwd)
            PENDING_HEADS[h.data_ptr()] = (z, log_scale, bias, None, log_s, h, z1c, ld, mode, int(odd), (P, L, U, L_mask, U_mask, sign_s, Wm))
        else:
            N.call('nf_glow_head_fwd', N.ptr(z), N.ptr(log_scale), N.ptr(bias), N.ptr(P), N.ptr(L), N.ptr(U), N.ptr(L_mask),
                   N.ptr(U_mask), N.ptr(sign_s), N.ptr(log_s), N.ptr(h), N.ptr(z1c), N.ptr(Wm), N.ptr(ld), mode, int(odd), B,
                   C, H, W, N.stream())
        ctx.save_for_backward(z, log_scale, bias, Wm, P, L, U, L_mask, U_mask, sign_s, log_s)
        ctx.meta = (mode, int(odd))
        ctx.sinks = _sinks(log_scale, bias, L, U, log_s)
        ctx.mark_dirty(ld)
        ctx.set_materialize_grads(False)          # the gathered half has no gradient of its own under the fused image coupling
        return h, z1c, ld

    @staticmethod
    def backward(ctx, g_h, g_z1c, g_ld):
        z, log_scale, bias, Wm, P, L, U, L_mask, U_mask, sign_s, log_s = ctx.saved_tensors
        mode, odd = ctx.meta
        B, C, H, W = _bchw(z)
        if g_h is None:                            # (grads are not materialised: an unused output arrives as None)
            g_h = torch.zeros_like(z)
        if g_ld is None:
            g_ld = torch.zeros(z.shape[0], dtype=z.dtype, device=z.device)
        g_h, g_z1c, g_ld = _contig(g_h), (_contig(g_z1c) if g_z1c is not None else None), _contig(g_ld)
        g_z = torch.empty_like(z)
        direct = ctx.sinks is not None
        tmp = WS.zeros(C * C + 4 + (0 if direct else 2 * C), z.device)
        g_W, sum_gld = tmp[:C * C], tmp[C * C:C * C + 1]
        if direct:
            g_ls, g_b, g_L, g_U, g_logs = ctx.sinks
        else:
            g_ls, g_b = tmp[C * C + 4:C * C + 4 + C].view_as(log_scale), tmp[C * C + 4 + C:].view_as(bias)
            g_L, g_U, g_logs = torch.empty_like(L), torch.empty_like(U), torch.empty_like(log_s)
        from .fused_conv import CONV_DEFER
        if direct and CONV_DEFER.active and HEAD_PARAMS_DEFER:
            # the data gradient now; the parameter sums of all such heads in one launch at the end-of-pass flush, in front of their PLU jobs
            if ctx.bwd_defer and HEAD_BWD_IN_CHAIN and g_z1c is None and z.dim() == 4 and 2 <= C <= 4:
                # (as in _GlowHeadW.backward: the previous step's chain launch computes g_z in its prologue -- nf_cc_head_small_bwd)
                PENDING_HEAD_BWD[g_z.data_ptr()] = (g_h, log_scale, Wm, g_z, (mode, odd))
            else:
                N.call('nf_glow_head_bwd_data', N.ptr(g_h), N.ptr(g_z1c), N.ptr(log_scale), N.ptr(Wm), N.ptr(g_z), mode, odd, B, C, H, W, N.stream())
            CONV_DEFER.head_jobs.append(((mode, B, C, H, W), g_h, g_z1c, g_ld, z, log_scale, bias, Wm, g_ls, g_b, g_W, sum_gld, int(odd)))
        else:
            N.call('nf_glow_head_bwd', N.ptr(g_h), N.ptr(g_z1c), N.ptr(g_ld), N.ptr(z), N.ptr(log_scale), N.ptr(bias),
                   N.ptr(Wm), N.ptr(g_z), N.ptr(g_ls), N.ptr(g_b), N.ptr(g_W), N.ptr(sum_gld), mode, odd, B, C, H, W,
                   N.stream())
        if direct and CONV_DEFER.active:
            # inside a trainer step the PLU backward (8 us per layer on the backward pass's latency chain, nothing but Adam waits for
            # it) joins the end-of-pass flush: all queued layers in one nf_invconv_weight_bwd_multi launch per 24
            CONV_DEFER.plu_jobs.append((g_W, P, L, U, L_mask, U_mask, sign_s, log_s, sum_gld, g_L, g_U, g_logs, C, H * W))
        else:
            N.call('nf_invconv_weight_bwd', N.ptr(g_W), N.ptr(P), N.ptr(L), N.ptr(U), N.ptr(L_mask), N.ptr(U_mask),
                   N.ptr(sign_s), N.ptr(log_s), N.ptr(sum_gld), N.ptr(g_L), N.ptr(g_U), N.ptr(g_logs), int(direct), C, 1,
                   H * W, N.stream())
        if direct:
            return (g_z, g_ld) + (None, ) * 13
        return g_z, g_ld, g_ls, g_b, None, g_L, g_U, None, None, None, g_logs, None, None, None, None


class _GlowHeadW(torch.autograd.Function):
    """ActNorm + invertible 1x1 with its weight W given assembled (fused.plu_weights_all) + conditioning-half gather on 9 .. 64
    channels of image data: one MFMA launch per direction (csrc/glow_head_mfma.hip)."""

    @staticmethod
    def forward(ctx, x, ld, log_scale, bias, W, log_s, holder, idx, mode, odd, defer=False, bwd_defer=False):
        B, C, H, Wd = x.shape
        ctx.bwd_defer = bool(bwd_defer)
        h = torch.empty_like(x)
        z1c = torch.empty(_half_shape(x, mode), dtype=x.dtype, device=x.device)
        if defer:
            # the launch is left to the coupling's chain kernel, whose prologue does this head's work (csrc/conv_chain.hip:
            # nf_cc_head_fwd): it finds the operands under the address of h, which it receives as its z
            PENDING_HEADS[h.data_ptr()] = (x, log_scale, bias, W, log_s, h, z1c, ld, mode, int(odd), None)
        else:
            N.call('nf_glow_head_w_fwd', N.ptr(x), N.ptr(log_scale), N.ptr(bias), N.ptr(W), N.ptr(log_s), N.ptr(h), N.ptr(z1c),
                   N.ptr(ld), mode, int(odd), B, C, H, Wd, N.stream())
        ctx.save_for_backward(x, log_scale, bias, W)
        ctx.holder, ctx.idx, ctx.meta = holder, idx, (mode, int(odd))
        holder.meta[idx] = (B, H * Wd)
        ctx.sinks = _sinks(log_scale, bias)
        ctx.mark_dirty(ld)
        ctx.set_materialize_grads(False)          # the gathered half has no gradient of its own under the fused image coupling
        return h, z1c, ld

    @staticmethod
    def backward(ctx, g_h, g_z1c, g_ld):
        x, log_scale, bias, W = ctx.saved_tensors
        mode, odd = ctx.meta
        B, C, H, Wd = x.shape
        if g_h is None:
            g_h = torch.zeros_like(x)
        if g_ld is None:
            g_ld = torch.zeros(B, dtype=x.dtype, device=x.device)
        g_h, g_ld = _contig(g_h), _contig(g_ld)
        if g_z1c is not None:                       # (a coupling that was not fused into its conditioner's launches: image Flow++)
            full = torch.empty_like(x)
            N.call('nf_half_scatter_add', N.ptr(_contig(g_z1c)), N.ptr(g_h), N.ptr(full), 1, mode, odd, B, C, H, Wd, N.stream())
            g_h = full
        g_x = torch.empty_like(x)
        direct = ctx.sinks is not None
        tmp = WS.zeros(C * C + (0 if direct else 2 * C), x.device)
        g_W = tmp[:C * C].view_as(W)
        if HEAD_PARAMS_DEFER and direct and ctx.needs_input_grad[4]:
            # only g_x is on the way of the backward pass: the contractions over the batch (g_W, g_log_scale, g_bias) of all heads of one
            # shape run in one launch where the pass ends -- in front of the PLU backward that reads g_W (fused._PLUWeightsMulti.backward).
            # What they read is kept alive here: g_h, g_ld (nothing writes to a gradient autograd has handed over), x.
            from .fused_conv import CONV_DEFER
            if ctx.bwd_defer and HEAD_BWD_IN_CHAIN and CONV_DEFER.active:
                # x is the output of a fused image coupling: g_x is the g_y of that coupling's chain launch, which autograd runs next and
                # which computes it in its own prologue (csrc/conv_chain.hip: nf_cc_head_bwd) -- no launch here.  Inside a trainer step
                # only: the flush at the end of the pass performs whatever was not picked up (fused_conv.ConvDefer.flush).
                PENDING_HEAD_BWD[g_x.data_ptr()] = (g_h, log_scale, W, g_x, None)
            else:
                N.call('nf_glow_head_w_bwd_data', N.ptr(g_h), N.ptr(log_scale), N.ptr(W), N.ptr(g_x), B, C, H, Wd, N.stream())
            ctx.holder.pending.append(((B, C, H, Wd), g_h, g_ld, x, log_scale, bias, W, ctx.sinks[0], ctx.sinks[1], g_W))
            ctx.holder.g_ld[ctx.idx] = g_ld
            return g_x, g_ld, None, None, g_W, None, None, None, None, None, None, None
        if direct:
            p_ls, p_b, g_ls, g_b = ctx.sinks[0].data_ptr(), ctx.sinks[1].data_ptr(), None, None
        else:
            g_ls, g_b = tmp[C * C:C * C + C].view_as(log_scale), tmp[C * C + C:].view_as(bias)
            p_ls, p_b = g_ls.data_ptr(), g_b.data_ptr()
        N.call('nf_glow_head_w_bwd', N.ptr(g_h), N.ptr(g_ld), N.ptr(x), N.ptr(log_scale), N.ptr(bias), N.ptr(W), N.ptr(g_x), p_ls,
               p_b, N.ptr(g_W), B, C, H, Wd, N.stream())
        ctx.holder.g_ld[ctx.idx] = g_ld
        return g_x, g_ld, g_ls, g_b, g_W, None, None, None, None, None, None, None


HEAD_PARAMS_DEFER = True      # (internal constant: tests flip it to compare the two forms of the head backward)
HEAD_BWD_IN_CHAIN = True      # (internal: the head's data gradient in the prologue of the previous coupling's backward chain launch)
PENDING_HEAD_BWD = {}         # address of g_x -> (g_h, log_scale, W, g_x, small) of a head whose data gradient the next chain launch computes
                              # (small: None for the MFMA head, (mode, odd) for the 2 .. 4 channel head with its saved weight)


def flush_pending_head_bwd(entry):
    """the data gradient of a head left to a chain launch (``entry`` of PENDING_HEAD_BWD) on its own kernel after all"""
    g_h, log_scale, W, g_x, small = entry
    B, C, H, Wd = g_x.shape
    if small is None:
        N.call('nf_glow_head_w_bwd_data', N.ptr(g_h), N.ptr(log_scale), N.ptr(W), N.ptr(g_x), B, C, H, Wd, N.stream())
    else:
        N.call('nf_glow_head_bwd_data', N.ptr(g_h), None, N.ptr(log_scale), N.ptr(W), N.ptr(g_x), small[0], small[1], B, C, H, Wd, N.stream())


def flush_all_pending_head_bwd():
    """end of a trainer's backward pass: nothing may be left.  An entry that no chain launch picked up means the gradient autograd handed
    to the coupling was not the tensor the head returned (the coupling's output has a second consumer, so autograd summed two gradients
    first; or only part of the graph was differentiated): the pass consumed a tensor that had not been computed -- loud, not silent."""
    n = len(PENDING_HEAD_BWD)
    while PENDING_HEAD_BWD:
        flush_pending_head_bwd(PENDING_HEAD_BWD.pop(next(iter(PENDING_HEAD_BWD))))
    if n:
        raise RuntimeError('%d Glow head(s) left their data gradient to the previous coupling\'s backward launch, which never asked for it: '
                           'the output of a fused image coupling must feed the next flow step only (functional.HEAD_BWD_IN_CHAIN = False '
                           'restores the stand-alone launches)' % n)


class GlowHeadParamsDesc(ctypes.Structure):
    """include/nfhip.h: nf_glow_head_params_desc"""
    _fields_ = [(f, ctypes.c_void_p) for f in ('g_h', 'g_ld', 'x', 'act_log_scale', 'act_bias', 'W', 'g_log_scale', 'g_bias', 'g_W')]


class GlowHeadSmallParamsDesc(ctypes.Structure):
    """include/nfhip.h: nf_glow_head_small_params_desc"""
    _fields_ = [(f, ctypes.c_void_p) for f in ('g_h', 'g_z1c', 'g_ld', 'z', 'log_scale', 'bias', 'W_saved', 'g_log_scale', 'g_bias', 'g_W',
                                                'sum_g_ld')] + [('odd', ctypes.c_int), ('reserved', ctypes.c_int)]


def launch_small_head_params(jobs):
    """the parameter sums of the C <= 4 heads queued by _GlowHead.backward (fused_conv.ConvDefer.flush)"""
    step = N.header_constant('NF_GLOW_HEAD_MULTI_MAX')
    groups = {}
    for e in jobs:
        groups.setdefault(e[0], []).append(e)
    for (mode, B, C, H, W), es in groups.items():
        for k0 in range(0, len(es), step):
            chunk = es[k0:k0 + step]
            arr = (GlowHeadSmallParamsDesc * len(chunk))()
            for i, (_, g_h, g_z1c, g_ld, z, ls, bs, Wm, g_ls, g_b, g_W, sum_gld, odd) in enumerate(chunk):
                d = arr[i]
                d.g_h, d.g_z1c, d.g_ld, d.z = g_h.data_ptr(), (g_z1c.data_ptr() if g_z1c is not None else None), g_ld.data_ptr(), z.data_ptr()
                d.log_scale, d.bias, d.W_saved = ls.data_ptr(), bs.data_ptr(), Wm.data_ptr()
                d.g_log_scale, d.g_bias, d.g_W, d.sum_g_ld, d.odd = g_ls.data_ptr(), g_b.data_ptr(), g_W.data_ptr(), sum_gld.data_ptr(), odd
            N.call('nf_glow_head_bwd_params_multi', ctypes.addressof(arr), len(chunk), mode, B, C, H, W, N.stream())


def flush_head_params(holder):
    """the parameter gradients of the heads queued on ``holder``: heads of one shape share launches of NF_GLOW_HEAD_MULTI_MAX"""
    pend, holder.pending = holder.pending, []
    if not pend:
        return
    step = N.header_constant('NF_GLOW_HEAD_MULTI_MAX')
    groups = {}
    for e in pend:
        groups.setdefault(e[0], []).append(e)
    for (B, C, H, Wd), es in groups.items():
        for k0 in range(0, len(es), step):
            chunk = es[k0:k0 + step]
            arr = (GlowHeadParamsDesc * len(chunk))()
            for i, (_, g_h, g_ld, x, ls, bs, W, s_ls, s_b, g_W) in enumerate(chunk):
                d = arr[i]
                d.g_h, d.g_ld, d.x, d.act_log_scale, d.act_bias, d.W = g_h.data_ptr(), g_ld.data_ptr(), x.data_ptr(), ls.data_ptr(), bs.data_ptr(), W.data_ptr()
                d.g_log_scale, d.g_bias, d.g_W = s_ls.data_ptr(), s_b.data_ptr(), g_W.data_ptr()
            N.call('nf_glow_head_w_bwd_params_multi', ctypes.addressof(arr), len(chunk), B, C, H, Wd, N.stream())


PENDING_HEADS = {}      # address of h -> operands of a head forward that its coupling's chain launch performs (_GlowHeadW.forward(defer=True))


def flush_pending_head(h):
    """launch the head whose output buffer is ``h`` on its own kernel, if it is still pending (a coupling that did not take the chain
    launch after all); returns True if there was one"""
    pend = PENDING_HEADS.pop(h.data_ptr(), None)
    if pend is None:
        return False
    x, log_scale, bias, W, log_s, h_, z1c, ld, mode, odd, small = pend
    B, C, H, Wd = x.shape
    if small is None:
        N.call('nf_glow_head_w_fwd', N.ptr(x), N.ptr(log_scale), N.ptr(bias), N.ptr(W), N.ptr(log_s), N.ptr(h_), N.ptr(z1c), N.ptr(ld), mode,
               odd, B, C, H, Wd, N.stream())
    else:
        P, L, U, Lm, Um, sign_s, Wm = small
        N.call('nf_glow_head_fwd', N.ptr(x), N.ptr(log_scale), N.ptr(bias), N.ptr(P), N.ptr(L), N.ptr(U), N.ptr(Lm), N.ptr(Um), N.ptr(sign_s),
               N.ptr(log_s), N.ptr(h_), N.ptr(z1c), N.ptr(Wm), N.ptr(ld), mode, odd, B, C, H, Wd, N.stream())
    return True


def glow_head_w_usable(z, mode):
    return (z.is_cuda and z.dim() == 4 and z.dtype == torch.float32
            and bool(N.load().nf_glow_head_w_usable(z.shape[0], z.shape[1], z.shape[2], z.shape[3], int(mode))))


def glow_head_w(z, ld, log_scale, bias, W, log_s, holder, idx, mode, odd, defer=False, bwd_defer=False):
    """(h, z1c, ld): ActNorm.forward -> InvertibleConv1x1.forward (weight given) -> conditioning half of the split, fused.
    defer: no launch -- the caller guarantees that the coupling's chain launch follows and performs it (fused_conv._cn_forward).
    bwd_defer: the caller guarantees that z IS the output of a fused image coupling (fused_conv._FusedConvCoupling) of the same
    shape: inside a trainer step the backward leaves this head's data gradient to that coupling's backward launch."""
    return _GlowHeadW.apply(_contig(z), _owned_ld(ld), log_scale, bias, W, log_s, holder, idx, mode, odd, defer, bwd_defer)


HEAD_MAX_C = 4


def glow_head(z, ld, log_scale, bias, P, L, U, L_mask, U_mask, sign_s, log_s, mode, odd, bwd_defer=False, defer=False):
    """(h, z1c, ld): ActNorm.forward -> InvertibleConv1x1.forward -> conditioning half of the split, fused (C <= 4).
    defer, bwd_defer: as in glow_head_w."""
    return _GlowHead.apply(_contig(z), _owned_ld(ld), log_scale, bias, P, L, U, L_mask, U_mask, sign_s, log_s, mode, odd, bwd_defer, defer)


def from_fused_coupling(z):
    """z is the (first) output of a fused image coupling's chain launch (fused_conv._FusedConvCoupling): the gradient a head returns for it
    is consumed by that launch's backward and by nothing else"""
    fn = z.grad_fn
    return fn is not None and type(fn).__name__ == '_FusedConvCouplingBackward' and not z._backward_hooks and z.is_contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# logit
# ----------------------------------------------------------------------------------------------------------------------
class _Logit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ld, eps):
        B = x.shape[0]
        n = x.numel() // B if B else 1
        y = torch.empty_like(x)
        N.call('nf_logit_fwd', N.ptr(x), N.ptr(y), N.ptr(ld), float(eps), 0, B, n, N.stream())
        ctx.save_for_backward(x)
        ctx.eps = float(eps)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        (x, ) = ctx.saved_tensors
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_x = torch.empty_like(x)
        N.call('nf_logit_bwd', N.ptr(g_y), N.ptr(g_ld), N.ptr(x), N.ptr(g_x), ctx.eps, x.shape[0], x.numel() // max(x.shape[0], 1),
               N.stream())
        return g_x, g_ld, None


def logit(x, ld, eps, inverse=False):
    x = _contig(x)
    ld = _owned_ld(ld)
    if not inverse:
        return _Logit.apply(x, ld, eps)
    with torch.no_grad():
        y = torch.empty_like(x)
        N.call('nf_logit_fwd', N.ptr(x), N.ptr(y), N.ptr(ld), float(eps), 1, x.shape[0], x.numel() // max(x.shape[0], 1), N.stream())
    return y, ld


# ----------------------------------------------------------------------------------------------------------------------
# Sigmoid / Tanh / Arctanh (flows/modules.py:125-183) and Squeeze1d / Unsqueeze1d (flows/squeeze.py:114-151)
# ----------------------------------------------------------------------------------------------------------------------
BIJ_SIGMOID, BIJ_SIGMOID_INV, BIJ_TANH, BIJ_ARCTANH = 0, 1, 2, 3


class _Bijector(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ld, kind):
        B = x.shape[0]
        n = x.numel() // B if B else 1
        y = torch.empty_like(x)
        N.call('nf_bijector_fwd', N.ptr(x), N.ptr(y), N.ptr(ld), kind, B, n, N.stream())
        ctx.save_for_backward(x)
        ctx.kind = kind
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        (x, ) = ctx.saved_tensors
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_x = torch.empty_like(x)
        N.call('nf_bijector_bwd', N.ptr(g_y), N.ptr(g_ld), N.ptr(x), N.ptr(g_x), ctx.kind, x.shape[0], x.numel() // max(x.shape[0], 1),
               N.stream())
        return g_x, g_ld, None


def bijector(x, ld, kind):
    """one elementwise bijector pass, ld[b] += its per-sample log-det.  The modules' forward directions (sigmoid, tanh, arctanh) build an
    autograd graph; the Sigmoid module's inverse (kind BIJ_SIGMOID_INV) builds none, like every inverse direction here."""
    x = _contig(x)
    ld = _owned_ld(ld)
    if kind != BIJ_SIGMOID_INV and torch.is_grad_enabled() and (x.requires_grad or ld.requires_grad):
        return _Bijector.apply(x, ld, kind)
    with torch.no_grad():
        y = torch.empty_like(x)
        N.call('nf_bijector_fwd', N.ptr(x), N.ptr(y), N.ptr(ld), kind, x.shape[0], x.numel() // max(x.shape[0], 1), N.stream())
    return y, ld


class _Squeeze1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, odd, inverse):
        z = _contig(z)
        out = torch.empty_like(z)
        N.call('nf_squeeze1d', N.ptr(z), N.ptr(out), z.shape[0], z.shape[1], int(odd), int(inverse), N.stream())
        ctx.meta = (int(odd), int(inverse))
        return out

    @staticmethod
    def backward(ctx, g):
        odd, inverse = ctx.meta
        g = _contig(g)
        out = torch.empty_like(g)
        N.call('nf_squeeze1d', N.ptr(g), N.ptr(out), g.shape[0], g.shape[1], odd, 1 - inverse, N.stream())
        return out, None, None


def squeeze1d(z, odd=False, inverse=False):
    """(B, D) -> cat(z[:, odd::2], z[:, 1 - odd::2]) (flows/squeeze.py:63-83, :124-127); inverse=True: the inverse map."""
    if z.dim() != 2 or z.shape[1] % 2:
        raise ValueError('squeeze1d takes (B, D) data with even D, got %s' % (tuple(z.shape), ))
    return _Squeeze1d.apply(z, bool(odd), bool(inverse))


# ----------------------------------------------------------------------------------------------------------------------
# Flow++ mixture-of-logistics coupling
# ----------------------------------------------------------------------------------------------------------------------
class _MixLogCoupling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, params, a, c, ld, K, eps, mode, odd):
        B, C, H, W = _bchw(z)
        y = torch.empty_like(z)
        N.call('nf_mixlog_coupling_fwd', N.ptr(z), N.ptr(params), N.ptr(a), N.ptr(c), N.ptr(y), N.ptr(ld), K, float(eps),
               mode, int(odd), B, C, H, W, N.stream())
        ctx.save_for_backward(z, params, a, c)
        ctx.meta = (K, float(eps), mode, int(odd))
        ctx.sinks = _sinks(a, c)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        z, params, a, c = ctx.saved_tensors
        K, eps, mode, odd = ctx.meta
        B, C, H, W = _bchw(z)
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_z = torch.empty_like(z)
        g_p = torch.empty_like(params)
        if ctx.sinks is not None and z.dim() == 4:
            # image data inside a trainer step: the coupling's scale / shift gradients leave as per-workgroup partial sums and are folded
            # with the conditioners' slabs where the pass ends (fused_flowpp_img.FlowppImgDefer) -- no same-address atomics
            from .fused_flowpp_img import FPP_IMG_DEFER
            n = int(N.load().nf_mixlog_bwd_blocks(K, mode, B, C, H, W)) if FPP_IMG_DEFER.active else 0
            if n > 0:
                part = torch.empty(2 * n, dtype=torch.float32, device=z.device)
                N.call('nf_mixlog_coupling_bwd_partials', N.ptr(g_y), N.ptr(g_ld), N.ptr(z), N.ptr(params), N.ptr(a), N.ptr(c), N.ptr(g_z),
                       N.ptr(g_p), N.ptr(part), K, eps, mode, odd, B, C, H, W, N.stream())
                FPP_IMG_DEFER.sums.append((part[:n], ctx.sinks[0], 1, 1, n, True, 1))
                FPP_IMG_DEFER.sums.append((part[n:], ctx.sinks[1], 1, 1, n, True, 1))
                return g_z, g_p, None, None, g_ld, None, None, None, None
        if ctx.sinks is not None:
            pa, pc, ga, gc = ctx.sinks[0].data_ptr(), ctx.sinks[1].data_ptr(), None, None
        else:
            g_ac = WS.zeros(2, z.device)
            pa, pc = g_ac.data_ptr(), g_ac.data_ptr() + 4
            ga, gc = g_ac[0:1].view_as(a), g_ac[1:2].view_as(c)
        N.call('nf_mixlog_coupling_bwd', N.ptr(g_y), N.ptr(g_ld), N.ptr(z), N.ptr(params), N.ptr(a), N.ptr(c),
               N.ptr(g_z), N.ptr(g_p), pa, pc, K, eps, mode, odd, B, C, H, W, N.stream())
        return g_z, g_p, ga, gc, g_ld, None, None, None, None


def mixlog_coupling(z, params, a_log_scale, a_bias, ld, n_mixtures, mode, odd, inverse=False, logit_eps=1.0e-5):
    """MixLogAttnCoupling._transform / _inverse_transform + split + merge given ``params`` = conditioner(z1)
    (flows/coupling.py:172-210).  The inverse reproduces the reference's 25-or-100 iteration bisection rule."""
    z, params = _contig(z), _contig(params)
    half = _half_shape(z, mode)
    want = (half[0], (2 + 3 * n_mixtures) * half[1]) + tuple(half[2:])
    if tuple(params.shape) != want:
        raise ValueError('conditioner output has shape %s, expected %s' % (tuple(params.shape), want))
    ld = _owned_ld(ld)
    if not inverse:
        return _MixLogCoupling.apply(z, params, a_log_scale, a_bias, ld, n_mixtures, logit_eps, mode, odd)
    with torch.no_grad():
        B, C, H, W = _bchw(z)
        y = torch.empty_like(z)
        n_el = z.numel() // 2
        scratch = torch.empty(3 * max(n_el, 1), dtype=z.dtype, device=z.device)
        flag = torch.empty(1, dtype=torch.int32, device=z.device)
        N.call('nf_mixlog_coupling_inv', N.ptr(z), N.ptr(params), N.ptr(a_log_scale), N.ptr(a_bias), N.ptr(y), N.ptr(ld),
               N.ptr(scratch), N.ptr(flag), n_mixtures, mode, int(odd), B, C, H, W, N.stream())
    return y, ld


# ----------------------------------------------------------------------------------------------------------------------
# rational-quadratic spline coupling (Durkan et al. 2019; csrc/rqspline.hip)
# ----------------------------------------------------------------------------------------------------------------------
RQS_BINS = (4, 8, 16)           # the template instances of csrc/rqspline.hip


class _RQSCoupling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, params, ld, K, bound, mode, odd):
        B, C, H, W = _bchw(z)
        y = torch.empty_like(z)
        N.call('nf_rqs_coupling_fwd', N.ptr(z), N.ptr(params), N.ptr(y), N.ptr(ld), K, bound, mode, int(odd), 0, B, C, H, W, N.stream())
        ctx.save_for_backward(z, params)
        ctx.meta = (K, bound, mode, int(odd))
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        z, params = ctx.saved_tensors
        K, bound, mode, odd = ctx.meta
        B, C, H, W = _bchw(z)
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_z = torch.empty_like(z)
        g_p = torch.empty_like(params)
        N.call('nf_rqs_coupling_bwd', N.ptr(g_y), N.ptr(g_ld), N.ptr(z), N.ptr(params), N.ptr(g_z), N.ptr(g_p), K, bound, mode, odd,
               B, C, H, W, N.stream())
        return g_z, g_p, g_ld, None, None, None, None


def rqs_coupling(z, params, ld, K, bound, mode, odd, inverse=False):
    """the monotone rational-quadratic spline coupling of Neural Spline Flows given ``params`` = conditioner(z1), shape
    (B, (3K - 1) Ch, h, w): split + spline + merge + log-det in one launch; linear tails outside (-bound, bound).  The inverse is
    closed-form (one quadratic solve per element) and runs without building a graph, like ``mixlog_coupling``'s."""
    z, params = _contig(z), _contig(params)
    N.ptr(z)                                                                # raises the engine's "no CPU path" error
    K, bound = int(K), float(bound)
    if K not in RQS_BINS:
        raise ValueError('the spline kernels are built for %s bins, got %d' % (' / '.join(str(k) for k in RQS_BINS), K))
    if not bound > 0.0:
        raise ValueError('the spline interval (-bound, bound) needs bound > 0, got %r' % bound)
    half = _half_shape(z, mode)
    want = (half[0], (3 * K - 1) * half[1]) + tuple(half[2:])
    if tuple(params.shape) != want:
        raise ValueError('conditioner output has shape %s, expected %s' % (tuple(params.shape), want))
    ld = _owned_ld(ld)
    if not inverse:
        return _RQSCoupling.apply(z, params, ld, K, bound, mode, odd)
    with torch.no_grad():
        B, C, H, W = _bchw(z)
        y = torch.empty_like(z)
        N.call('nf_rqs_coupling_fwd', N.ptr(z), N.ptr(params), N.ptr(y), N.ptr(ld), K, bound, mode, int(odd), 1, B, C, H, W, N.stream())
    return y, ld


# ----------------------------------------------------------------------------------------------------------------------
# autoregressive spline head: masked output layer + spline in one launch (csrc/arspline.hip)
# ----------------------------------------------------------------------------------------------------------------------
ARS_MAX_D = 8                   # features the head kernels serve
ARS_HIDDEN = 32                 # hidden width they are built for


class _ARSHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, weight, bias, mask, z, ld, K, bound):
        B, D = z.shape
        y = torch.empty_like(z)
        N.call('nf_arspline_head_fwd', N.ptr(a), N.ptr(weight), N.ptr(bias), N.ptr(mask), N.ptr(z), N.ptr(y), N.ptr(ld), K, bound, 0, -1,
               B, D, ARS_HIDDEN, N.stream())
        ctx.save_for_backward(a, weight, bias, mask, z)
        ctx.meta = (K, bound)
        ctx.sinks = _sinks(weight, bias)
        ctx.mark_dirty(ld)
        return y, ld

    @staticmethod
    def backward(ctx, g_y, g_ld):
        a, weight, bias, mask, z = ctx.saved_tensors
        K, bound = ctx.meta
        B, D = z.shape
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        g_a, g_z = torch.empty_like(a), torch.empty_like(z)
        rows = weight.shape[0]
        n = int(N.load().nf_arspline_head_slabs(B))
        if n == 0:                                                              # an empty batch: nothing depends on the parameters
            return g_a, torch.zeros_like(weight), torch.zeros_like(bias), None, g_z, g_ld, None, None
        # per-workgroup partial sums of the weight and bias gradients, every element written by the launch; one nf_slab_sum folds both
        slabs = torch.empty(n * rows * (ARS_HIDDEN + 1), dtype=torch.float32, device=z.device)
        gw_s, gb_s = slabs[:n * rows * ARS_HIDDEN], slabs[n * rows * ARS_HIDDEN:]
        N.call('nf_arspline_head_bwd', N.ptr(g_y), N.ptr(g_ld), N.ptr(a), N.ptr(weight), N.ptr(bias), N.ptr(mask), N.ptr(z), N.ptr(g_a),
               N.ptr(g_z), N.ptr(gw_s), N.ptr(gb_s), K, bound, B, D, ARS_HIDDEN, N.stream())
        from .fused_conv import _slab_sum
        if ctx.sinks is not None:                                               # inside a trainer step: += into the bucket's gradients
            g_w, g_b, acc = ctx.sinks[0], ctx.sinks[1], True
        else:
            g_w, g_b, acc = torch.empty_like(weight), torch.empty_like(bias), False
        _slab_sum([(gw_s, g_w, rows * ARS_HIDDEN, rows * ARS_HIDDEN, n, acc, 1), (gb_s, g_b, rows, rows, n, acc, 1)])
        if acc:
            g_w = g_b = None
        return g_a, g_w, g_b, None, g_z, g_ld, None, None


def ars_head(a, weight, bias, mask, z, ld, K, bound, inverse=False, col=None, out=None):
    """the output layer of a masked-autoregressive conditioner and the rational-quadratic spline it parameterises, in one launch: for
    row b, feature d and parameter p, ``P[p] = bias[p D + d] + sum_i a[b, i] weight[p D + d, i] mask[d, i]`` and
    ``y[b, d] = rqs(z[b, d]; P)`` with the conventions of ``rqs_coupling``; the (B, (3K - 1) D) parameter tensor is never materialised.
    ``a`` (B, 32) is the activated hidden layer, ``weight`` ((3K - 1) D, 32), ``bias`` ((3K - 1) D, ), ``mask`` (D, 32) of 0 / 1, ``z``
    (B, D) with D <= 8.  Forward: every feature, ``ld`` += the log-det terms in place, autograd for ``a``, ``weight``, ``bias`` and
    ``z`` (the direct dependence; the path through the conditioner reaches ``z`` through ``a``).  ``inverse=True`` needs ``col``: the
    closed-form inverse of that ONE column from that feature's parameters, ``ld`` -= its term, every other column as in ``z``; it runs
    without a graph and writes into ``out`` (default: a clone of ``z``; ``out=z`` inverts the column in place)."""
    a, z = _contig(a), _contig(z)
    N.ptr(z)                                                                # raises the engine's "no CPU path" error
    K, bound = int(K), float(bound)
    if K not in RQS_BINS:
        raise ValueError('the spline kernels are built for %s bins, got %d' % (' / '.join(str(k) for k in RQS_BINS), K))
    if not bound > 0.0:
        raise ValueError('the spline interval (-bound, bound) needs bound > 0, got %r' % bound)
    if z.dim() != 2 or not 1 <= z.shape[1] <= ARS_MAX_D:
        raise ValueError('the autoregressive spline head takes (B, D) data with 1 <= D <= %d, got shape %s' % (ARS_MAX_D, tuple(z.shape)))
    B, D = z.shape
    rows = (3 * K - 1) * D
    for name, t, want in (('hidden activations', a, (B, ARS_HIDDEN)), ('head weight', weight, (rows, ARS_HIDDEN)), ('head bias', bias, (rows, )),
                          ('head mask', mask, (D, ARS_HIDDEN)), ('log_df_dz', ld, (B, ))):
        if tuple(t.shape) != want:
            raise ValueError('%s has shape %s, expected %s' % (name, tuple(t.shape), want))
    ld = _owned_ld(ld)
    if not inverse:
        if col is not None or out is not None:
            raise ValueError('col and out belong to the inverse direction (the forward transforms every feature into a new tensor)')
        return _ARSHead.apply(a, weight, bias, mask, z, ld, K, bound)
    if col is None or not 0 <= int(col) < D:
        raise ValueError('the inverse takes one column per call: 0 <= col < %d, got %r' % (D, col))
    with torch.no_grad():
        if out is None:
            out = z.clone()
        elif tuple(out.shape) != (B, D):
            raise ValueError('out has shape %s, expected %s' % (tuple(out.shape), (B, D)))
        N.call('nf_arspline_head_fwd', N.ptr(a), N.ptr(weight), N.ptr(bias), N.ptr(mask), N.ptr(z), N.ptr(out), N.ptr(ld), K, bound, 1, int(col),
               B, D, ARS_HIDDEN, N.stream())
    return out, ld


# ----------------------------------------------------------------------------------------------------------------------
# standalone MixLogCDF (flows/modules.py:186-212)
# ----------------------------------------------------------------------------------------------------------------------
def _mixcdf_shapes(x, log_pi):
    B = x.shape[0]
    n = x.numel() // B if B else 0
    if log_pi.dim() != x.dim() + 1 or log_pi.shape[0] != B or tuple(log_pi.shape[2:]) != tuple(x.shape[1:]):
        raise ValueError('MixLogCDF: x %s needs log_pi / mu / s of shape (B, K) + x.shape[1:], got %s'
                         % (tuple(x.shape), tuple(log_pi.shape)))
    return B, n, log_pi.shape[1]


class _MixLogCDF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, log_pi, mu, s, ld):
        B, n, K = _mixcdf_shapes(x, log_pi)
        out = torch.empty_like(x)
        N.call('nf_mixlogcdf_fwd', N.ptr(x), N.ptr(log_pi), N.ptr(mu), N.ptr(s), N.ptr(out), N.ptr(ld), K, B, n, N.stream())
        ctx.save_for_backward(x, log_pi, mu, s)
        ctx.mark_dirty(ld)
        return out, ld

    @staticmethod
    def backward(ctx, g_out, g_ld):
        x, log_pi, mu, s = ctx.saved_tensors
        B, n, K = _mixcdf_shapes(x, log_pi)
        g_out, g_ld = _contig(g_out), _contig(g_ld)
        g_x, g_lp, g_mu, g_s = torch.empty_like(x), torch.empty_like(log_pi), torch.empty_like(mu), torch.empty_like(s)
        N.call('nf_mixlogcdf_bwd', N.ptr(g_out), N.ptr(g_ld), N.ptr(x), N.ptr(log_pi), N.ptr(mu), N.ptr(s), N.ptr(g_x),
               N.ptr(g_lp), N.ptr(g_mu), N.ptr(g_s), K, B, n, N.stream())
        return g_x, g_lp, g_mu, g_s, g_ld


def mixlogcdf(x, log_pi, mu, s, ld, inverse=False):
    """MixLogCDF.forward / .backward (flows/modules.py:190-212): ``log_pi`` is already log-softmaxed over the mixture axis.
    Unlike the in-place transforms, the reference returns a NEW log-det tensor here (modules.py:194): so does this."""
    x, log_pi, mu, s = _contig(x), _contig(log_pi), _contig(mu), _contig(s)
    if mu.shape != log_pi.shape or s.shape != log_pi.shape:
        raise ValueError('MixLogCDF: log_pi, mu and s must have one shape')
    ld = ld.clone()
    if not inverse:
        return _MixLogCDF.apply(x, log_pi, mu, s, ld)
    with torch.no_grad():
        B, n, K = _mixcdf_shapes(x, log_pi)
        out = torch.empty_like(x)
        scratch = torch.empty(2 * max(x.numel(), 1), dtype=x.dtype, device=x.device)
        flag = torch.empty(1, dtype=torch.int32, device=x.device)
        N.call('nf_mixlogcdf_inv', N.ptr(x), N.ptr(log_pi), N.ptr(mu), N.ptr(s), N.ptr(out), N.ptr(ld), N.ptr(scratch),
               N.ptr(flag), K, B, n, N.stream())
    return out, ld


# ----------------------------------------------------------------------------------------------------------------------
# planar flow (flows/planar.py): a run of K PlanarTransform layers per launch
# ----------------------------------------------------------------------------------------------------------------------
PLANAR_GRID = False           # (tests: nf_planar_config(1), the grid form of the inverse at every batch size)


def planar_config(grid):
    """select the forms of nf_planar_inv: ``grid=True`` takes the three-launch-per-layer grid form at every batch size"""
    global PLANAR_GRID
    PLANAR_GRID = bool(grid)
    N.call('nf_planar_config', 1 if PLANAR_GRID else 0)


def _planar_check(z):
    if z.dim() != 2:
        raise RuntimeError('PlanarFlow takes (B, D) input (planar.py:39 multiplies z by w.t() with torch.mm), got shape %s'
                           % (tuple(z.shape), ))


def _planar_table(tensors):
    """host array of device pointers u_0 .. u_{K-1}, w_0 .., b_0 .. (include/nfhip.h: the params / grads tables)"""
    return (ctypes.c_int64 * len(tensors))(*[N.ptr(t) for t in tensors])


def _planar_params(layers):
    return [m.u for m in layers] + [m.w for m in layers] + [m.b for m in layers]


def planar_project_(layers):
    """PlanarTransform._make_invertible of every layer (planar.py:23-33): u projected IN PLACE through the parameter's current
    storage (a view of the flat bucket after GradBucket(flatten_params=True)), one launch, no host round trip"""
    with torch.no_grad():
        K, D = len(layers), layers[0].u.shape[1]
        N.call('nf_planar_project', _planar_table([p.data for p in _planar_params(layers)]), K, D, N.stream())


class _PlanarFlow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, ld, K, *params):
        B, D = z.shape
        out = torch.empty_like(z)
        save = torch.empty(K * B * D, dtype=z.dtype, device=z.device)
        N.call('nf_planar_fwd', N.ptr(z), N.ptr(out), N.ptr(ld), N.ptr(save), _planar_table(params), K, B, D, N.stream())
        ctx.K = K
        ctx.sinks = _sinks(*params)
        ctx.save_for_backward(save, *params)
        ctx.mark_dirty(ld)
        return out, ld

    @staticmethod
    def backward(ctx, g_out, g_ld):
        save, *params = ctx.saved_tensors
        K = ctx.K
        D = params[0].shape[1]
        B = save.numel() // (K * D)
        g_out, g_ld = _contig(g_out), _contig(g_ld)
        want_z = ctx.needs_input_grad[0]
        g_z = torch.empty((B, D), dtype=g_out.dtype, device=g_out.device) if (want_z or D > 8) else None
        n = ctypes.c_int64(0)
        rc = N.load().nf_planar_bwd_slab_floats(K, B, D, ctypes.byref(n))
        if rc != 0:
            raise N.NativeLibraryError('nf_planar_bwd_slab_floats failed with code %d' % rc)
        slab = torch.empty(max(int(n.value), 1), dtype=torch.float32, device=g_out.device)
        if ctx.sinks is not None:
            grads, ret = ctx.sinks, [None] * (3 * K)
        else:
            flat = WS.zeros(K * (2 * D + 1), g_out.device)
            gu = flat[:K * D].view(K, 1, D)
            gw = flat[K * D:2 * K * D].view(K, 1, D)
            gb = flat[2 * K * D:].view(K, 1)
            ret = [gu[k] for k in range(K)] + [gw[k] for k in range(K)] + [gb[k] for k in range(K)]
            grads = ret
        N.call('nf_planar_bwd', N.ptr(g_out), N.ptr(g_ld), N.ptr(save), _planar_table(params), _planar_table(grads), N.ptr(g_z),
               N.ptr(slab), K, B, D, N.stream())
        return (g_z if want_z else None, g_ld, None) + tuple(ret)


PLANAR_MAX_LAYERS = 128       # include/nfhip.h NF_PLANAR_MAX_LAYERS (checked against the header in tests/test_planar_host.py)


def planar_flow(z, ld, layers):
    """PlanarTransform.forward of ``layers`` in order (planar.py:35-45): the projection of every u (one launch), then all layers in
    one launch; training (autograd on) saves the layer inputs for the one-launch backward + fold"""
    _planar_check(z)
    z = _contig(z)
    ld = _owned_ld(ld)
    for i in range(0, len(layers), PLANAR_MAX_LAYERS):
        run = layers[i:i + PLANAR_MAX_LAYERS]
        planar_project_(run)
        params = _planar_params(run)
        if torch.is_grad_enabled() and (z.requires_grad or ld.requires_grad or any(p.requires_grad for p in params)):
            z, ld = _PlanarFlow.apply(z, ld, len(run), *params)
        else:
            with torch.no_grad():
                B, D = z.shape
                out = torch.empty_like(z)
                N.call('nf_planar_fwd', N.ptr(z), N.ptr(out), N.ptr(ld), None, _planar_table(params), len(run), B, D, N.stream())
                z = out
    return z, ld


def planar_inverse(z, ld, layers, mids=False):
    """PlanarTransform.backward of ``layers`` in reverse order (planar.py:47-68), no graph.  Returns (z, ld, iters) -- iters: int32
    (K,), the bisection's iteration count per layer in layer order -- and, with ``mids=True``, the midpoints (K, B) as a fourth value."""
    _planar_check(z)
    with torch.no_grad():
        z = _contig(z)
        ld = _owned_ld(ld)
        B, D = z.shape
        K = len(layers)
        iters = torch.zeros(K, dtype=torch.int32, device=z.device)
        mid = torch.empty((K, B), dtype=z.dtype, device=z.device) if mids else None
        wg = not PLANAR_GRID and B <= N.header_constant('NF_PLANAR_INV_WG_MAX_ROWS')
        scratch = None if wg else torch.empty(2 * max(B, 1), dtype=torch.float32, device=z.device)
        ctl = None if wg else torch.empty(2 * PLANAR_MAX_LAYERS, dtype=torch.int32, device=z.device)
        out = torch.empty_like(z)
        cur = z
        for j in range(((K + PLANAR_MAX_LAYERS - 1) // PLANAR_MAX_LAYERS) - 1, -1, -1):
            a, b = j * PLANAR_MAX_LAYERS, min(K, (j + 1) * PLANAR_MAX_LAYERS)
            run = layers[a:b]
            N.call('nf_planar_inv', N.ptr(cur), N.ptr(out), N.ptr(ld), N.ptr(mid[a:b]) if mids else None, N.ptr(iters[a:b]),
                   N.ptr(scratch), N.ptr(ctl), _planar_table([p.data for p in _planar_params(run)]), len(run), B, D, N.stream())
            cur = out
        if mids:
            return cur, ld, iters, mid
        return cur, ld, iters


# ----------------------------------------------------------------------------------------------------------------------
# Residual Flow (flows/resflow.py, flows/iresblock.py): the whole stack [ActNorm, InvertibleResLinear] x L per launch (csrc/resflow.hip)
# ----------------------------------------------------------------------------------------------------------------------
RESFLOW_STACK = os.environ.get('NF_RESFLOW_STACK', '1') != '0'     # 0: one ActNorm launch + the per-block kernels of csrc/resmlp.hip
RESFLOW_MAX_LAYERS = 32       # include/nfhip.h NF_RESFLOW_MAX_LAYERS (checked against the header in tests/test_resflow_host.py)
RESFLOW_P = 0.5               # the geometric law of the series lengths (iresblock.py:59, :84)
_resflow_tables = {}          # (device index, pointers) -> device int64 table: uploaded once, so a captured step replays against it


def _resflow_table(tensors, device):
    key = (device.index, tuple(t.data_ptr() for t in tensors))
    tab = _resflow_tables.get(key)
    if tab is None:
        if len(_resflow_tables) >= 64:
            _resflow_tables.clear()
        tab = torch.tensor(key[1], dtype=torch.int64).to(device)
        _resflow_tables[key] = tab
    return tab


def resflow_param_floats(D):
    """floats of one block's row of the packed parameter / gradient buffers: W1 | b1 | W2 | b2 | W3 | b3 | beta1 beta2 | log_scale | bias"""
    return 32 * D + 32 + 1024 + 32 + D * 32 + D + 2 + 2 * D


def _resflow_members(pairs):
    """(table tensors in include/nfhip.h's order, parameters in the gradient table's order) of [(ActNorm, InvertibleResLinear), ..]"""
    tab, params = [], []
    for a, blk in pairs:
        wbar, u, v, bias, beta = blk._stack_members()
        tab += wbar + u + v + bias + beta + [a.log_scale, a.bias]
        params += wbar + bias + beta + [a.log_scale, a.bias]
    return tab, params


def _resflow_series(blk, training):
    """(mode, S, n_exact, fixed_n) of the estimator the reference picks (iresblock.py:131-137)"""
    if training:
        return 2, 1, 1, 0
    if blk.estimator == 'exact':
        return 1, 0, 0, 0
    if blk.estimator == 'fixed':
        return 2, 4, 8, 8
    if blk.estimator == 'unbias':
        return 2, 4, 8, 0
    raise Exception('Unknown log-det estimator: %s' % (blk.estimator, ))


def resflow_spectral_(pairs, D):
    """spectral normalisation of every matrix of the stack in ONE launch (weight_u / weight_v updated in place): returns the packed
    effective parameters (L, n_tot) and the device pointer table"""
    tab, _ = _resflow_members(pairs)
    dev = tab[0].device
    table = _resflow_table([t.detach() for t in tab], dev)
    packed = torch.empty((len(pairs), resflow_param_floats(D)), dtype=torch.float32, device=dev)
    blk = pairs[0][1]
    N.call('nf_resflow_spectral', N.ptr(table, (torch.int64, )), N.ptr(packed), len(pairs), D, float(blk.coeff), float(blk._sn_eps()), N.stream())
    return packed, table


def resflow_draws(seed, L, B, D, S, n_exact, fixed_n=0, slots=2, layer0=0):
    """(n_terms int32 (L, slots, S), noise float32 (L, slots, B, S, D)) the kernels draw for the seed words ``seed`` (device int64[2]) as
    they stand now; slots=1 is the inverse's layout (squeezed: (L, S), (L, B, S, D))"""
    n_terms = torch.empty((L, slots, S), dtype=torch.int32, device=seed.device)
    noise = torch.empty((L, slots, B, S, D), dtype=torch.float32, device=seed.device)
    N.call('nf_resflow_draws', N.ptr(n_terms), N.ptr(noise), N.ptr(seed, (torch.int64, )), slots, S, n_exact, fixed_n, RESFLOW_P, L, layer0, B, D,
           N.stream())
    if slots == 1:
        return n_terms[:, 0], noise[:, 0]
    return n_terms, noise


def made_mask_views(buf, D):
    """per draw of a (n_draws, NF_MADE_MASK_STRIDE) buffer of nf_made_draw_masks: the four masks [(32, D), (32, 32), (32, 32), (D, 32)] as
    contiguous views"""
    offs = [N.header_constant('NF_MADE_MASK_OFF_%d' % l) for l in range(4)]
    shapes = [(32, D), (32, 32), (32, 32), (D, 32)]
    return [[buf[d, o:o + r * c].view(r, c) for o, (r, c) in zip(offs, shapes)] for d in range(buf.shape[0])]


def made_draw_masks(seed, n_draws, D, want_degrees=False, advance=False):
    """the MADE masks (flows/maf.py:66-85; three hidden layers of 32, D <= 4) the device draws for the seed words ``seed`` (device
    int64[2]: seed, stream offset) as they stand now: a list of ``n_draws`` mask sets [(32, D), (32, 32), (32, 32), (D, 32)], views of ONE
    tensor allocated for this call -- and, with ``want_degrees``, the int32 (n_draws, 3, 32) hidden degrees behind them.  ``advance``
    moves the stream offset on by n_draws on the device, behind the draw (what the model's own call sites do)."""
    buf = torch.empty((n_draws, N.header_constant('NF_MADE_MASK_STRIDE')), dtype=torch.float32, device=seed.device)
    deg = torch.empty((n_draws, 3, 32), dtype=torch.int32, device=seed.device) if want_degrees else None
    N.call('nf_made_draw_masks', N.ptr(buf), N.ptr(deg), N.ptr(seed, (torch.int64, )), n_draws, D, int(bool(advance)), N.stream())
    sets = made_mask_views(buf, D)
    return (sets, deg) if want_degrees else sets


class _ResFlowStack(torch.autograd.Function):
    """training forward of <= RESFLOW_MAX_LAYERS blocks (spectral launch + one stack launch) and its backward (one stack launch + the
    fold / spectral-norm autograd launch, gradients added to the parameters' sinks where a GradBucket offers them)"""

    @staticmethod
    def forward(ctx, z, ld, cfg, n_terms, noise, seed, *params):
        pairs, layer0 = cfg
        B, D = z.shape
        L = len(pairs)
        packed, table = resflow_spectral_(pairs, D)
        save = torch.empty((L, B, D), dtype=z.dtype, device=z.device)
        out, ld_out = torch.empty_like(z), ld.clone()
        N.call('nf_resflow_fwd', N.ptr(z), N.ptr(out), N.ptr(ld_out), N.ptr(save), N.ptr(packed), N.ptr(n_terms), N.ptr(noise),
               N.ptr(seed, (torch.int64, )) if noise is None else None, 2, 1, 1, 0, RESFLOW_P, L, layer0, B, D, N.stream())
        ctx.pairs, ctx.layer0, ctx.table = pairs, layer0, table
        ctx.sinks = _sinks(*params)
        ctx.save_for_backward(save, packed, n_terms, noise, seed, *params)
        return out, ld_out

    @staticmethod
    def backward(ctx, g_y, g_ld):
        save, packed, n_terms, noise, seed, *params = ctx.saved_tensors
        L, B, D = save.shape
        blk = ctx.pairs[0][1]
        g_y, g_ld = _contig(g_y), _contig(g_ld)
        n = ctypes.c_int64(0)
        rc = N.load().nf_resflow_bwd_slab_floats(L, B, D, ctypes.byref(n))
        if rc != 0:
            raise N.NativeLibraryError('nf_resflow_bwd_slab_floats failed with code %d' % rc)
        slab = torch.empty(max(int(n.value), 1), dtype=torch.float32, device=g_y.device)
        d_z = torch.empty_like(g_y)
        N.call('nf_resflow_bwd', N.ptr(g_y), N.ptr(g_ld), N.ptr(d_z), N.ptr(save), N.ptr(packed), N.ptr(n_terms), N.ptr(noise),
               N.ptr(seed, (torch.int64, )) if noise is None else None, 1, RESFLOW_P, N.ptr(slab), L, ctx.layer0, B, D, N.stream())
        if ctx.sinks is not None:
            gtab, flat, ret = _resflow_table(ctx.sinks, g_y.device), None, [None] * len(params)
        else:
            nt = resflow_param_floats(D)
            gtab, flat, ret = None, WS.zeros(L * nt, g_y.device).view(L, nt), []
            o = (0, 32 * D + 32, 32 * D + 32 + 1024 + 32)                            # W1, W2, W3 in a row of flat
            for l in range(L):
                r = flat[l]
                ret += [r[o[0]:o[0] + 32 * D].view(32, D), r[o[1]:o[1] + 1024].view(32, 32), r[o[2]:o[2] + 32 * D].view(D, 32),
                        r[32 * D:32 * D + 32], r[o[1] + 1024:o[1] + 1056], r[o[2] + 32 * D:o[2] + 33 * D],
                        r[o[2] + 33 * D:o[2] + 33 * D + 1], r[o[2] + 33 * D + 1:o[2] + 33 * D + 2],
                        r[o[2] + 33 * D + 2:o[2] + 34 * D + 2].view(params[10 * l + 8].shape),
                        r[o[2] + 34 * D + 2:o[2] + 35 * D + 2].view(params[10 * l + 9].shape)]
        N.call('nf_resflow_spectral_bwd', N.ptr(ctx.table, (torch.int64, )), N.ptr(gtab, (torch.int64, )), N.ptr(flat), N.ptr(slab), L, B, D,
               float(blk.coeff), float(blk._sn_eps()), N.stream())
        return (d_z, g_ld, None, None, None, None) + tuple(ret)


def resflow_flow(z, ld, pairs, draws='host', seed=None):
    """[ActNorm, InvertibleResLinear] x L forward (flows/resflow.py:30-33) on initialised ActNorms: per <= RESFLOW_MAX_LAYERS blocks one
    spectral-normalisation launch and one stack launch -- training (autograd on, blocks in training mode) through _ResFlowStack,
    density evaluation (no_grad, eval mode) without a graph.  draws='host': lengths and noise from the host generators in the
    reference's order (resflow.stack_draws); 'device': drawn in the kernels from ``seed`` (device int64[2]; seed[1] is advanced on the
    device once per launch)."""
    from . import resflow as RF
    z = _contig(z)
    blk = pairs[0][1]
    training = blk.training
    B, D = z.shape
    mode, S, n_exact, fixed_n = _resflow_series(blk, training)
    for i in range(0, len(pairs), RESFLOW_MAX_LAYERS):
        run = pairs[i:i + RESFLOW_MAX_LAYERS]
        n_terms = noise = None
        if draws == 'host':
            n_terms, noise = RF.stack_draws([b for _, b in run], z, training, 2)
        elif seed is None:
            raise RuntimeError("draws='device' needs the seed words (a device int64[2] tensor)")
        sd = seed.clone() if (draws != 'host' and training) else seed            # the backward regenerates the slot-0 noise from these
        if training:
            _, params = _resflow_members(run)
            z, ld = _ResFlowStack.apply(z, ld, (run, i), n_terms, noise, sd if draws != 'host' else None, *params)
        else:
            with torch.no_grad():
                packed, _ = resflow_spectral_(run, D)
                out, ld = torch.empty_like(z), ld.clone()
                N.call('nf_resflow_fwd', N.ptr(z), N.ptr(out), N.ptr(ld), None, N.ptr(packed), N.ptr(n_terms), N.ptr(noise),
                       N.ptr(sd, (torch.int64, )) if draws != 'host' else None, mode, S, n_exact, fixed_n, RESFLOW_P, len(run), i, B, D,
                       N.stream())
                z = out
        if draws != 'host':
            seed[1] += 1                                                            # a stream of its own for the next pass (device side)
    return z, ld


def resflow_inverse(z, ld, pairs, draws='host', seed=None):
    """the inverse of the stack, last block first (iresblock.py:236-255, modules.py:252-256), for B <= NF_RESFLOW_INV_WG_MAX_ROWS: one
    launch per <= RESFLOW_MAX_LAYERS blocks, no graph.  Returns (x, ld, iters) -- iters: int32 (L,), fixed-point iterations per block in
    layer order (also left on every block as ``last_inverse_iters``)."""
    from . import resflow as RF
    with torch.no_grad():
        z = _contig(z)
        B, D = z.shape
        L = len(pairs)
        blk = pairs[0][1]
        mode, S, n_exact, fixed_n = _resflow_series(blk, blk.training)
        iters = torch.zeros(L, dtype=torch.int32, device=z.device)
        ld = ld.clone()
        out = torch.empty_like(z)
        cur = z
        for j in range(((L + RESFLOW_MAX_LAYERS - 1) // RESFLOW_MAX_LAYERS) - 1, -1, -1):
            a, b = j * RESFLOW_MAX_LAYERS, min(L, (j + 1) * RESFLOW_MAX_LAYERS)
            run = pairs[a:b]
            n_terms = noise = None
            if draws == 'host':
                # the reference inverts the LAST block first: its draws come first in the host generators' streams
                n_terms, noise = RF.stack_draws([blk_ for _, blk_ in run][::-1], z, blk.training, 1)
                if n_terms is not None:
                    n_terms, noise = n_terms.flip(0).contiguous(), noise.flip(0).contiguous()
            elif seed is None:
                raise RuntimeError("draws='device' needs the seed words (a device int64[2] tensor)")
            tab, _ = _resflow_members(run)
            table = _resflow_table([t.detach() for t in tab], z.device)
            packed = torch.empty((len(run), resflow_param_floats(D)), dtype=torch.float32, device=z.device)
            N.call('nf_resflow_inv', N.ptr(cur), N.ptr(out), N.ptr(ld), N.ptr(iters[a:b]), N.ptr(table, (torch.int64, )), N.ptr(packed),
                   N.ptr(n_terms), N.ptr(noise), N.ptr(seed, (torch.int64, )) if draws != 'host' else None, mode, S, n_exact, fixed_n,
                   RESFLOW_P, float(blk.coeff), float(blk._sn_eps()), float(blk.ftol), len(run), a, B, D, N.stream())
            cur = out
            if draws != 'host':
                seed[1] += 1
        for l, (_, blk_) in enumerate(pairs):
            blk_.last_inverse_iters = iters[l]
    return cur, ld, iters


# ----------------------------------------------------------------------------------------------------------------------
# FFJORD (flows/cnf.py, flows/odeint.py): a whole ODE integration of one CNF layer per launch, fp64 (csrc/cnf.hip)
# ----------------------------------------------------------------------------------------------------------------------
CNF_METHODS = {'midpoint': 0, 'rk4': 1, 'bosha3': 2, 'dopri5': 3}      # include/nfhip.h NF_CNF_MIDPOINT ..; odeint.py:163-168
CNF_STAGES = (2, 4, 5, 7)                                               # field evaluations per step
CNF_TRACES = {'hutchinson': 0, 'exact': 1}
_F64 = (torch.float64, )
_F3264 = (torch.float32, torch.float64)


def _cnf_method(method):
    try:
        return CNF_METHODS[method]
    except KeyError:
        raise KeyError(method)                                              # (SOLVERS[method], odeint.py:211)


def cnf_schedule(times, method):
    """the evaluation schedule of ``odeint(func, x, times, method)`` (odeint.py:13-20, :68-94) as float64 CPU tensors:
    (stage_t [steps * stages], step_dt [steps], slope).  Host only: no GPU is touched."""
    m = _cnf_method(method)
    tt = torch.as_tensor(times).detach().to('cpu', torch.float64).contiguous()
    lib = N.load()
    n, slope = ctypes.c_int(0), ctypes.c_double(0.0)
    rc = lib.nf_cnf_schedule(tt.data_ptr(), tt.numel(), m, None, None, ctypes.byref(slope), ctypes.byref(n), 0)
    if rc != 0:
        raise N.NativeLibraryError('nf_cnf_schedule failed with code %d' % rc)
    steps = int(n.value)
    stage_t = torch.empty(steps * CNF_STAGES[m], dtype=torch.float64)
    step_dt = torch.empty(steps, dtype=torch.float64)
    rc = lib.nf_cnf_schedule(tt.data_ptr(), tt.numel(), m, stage_t.data_ptr(), step_dt.data_ptr(), ctypes.byref(slope),
                             ctypes.byref(n), steps)
    if rc != 0:
        raise N.NativeLibraryError('nf_cnf_schedule failed with code %d' % rc)
    return stage_t, step_dt, float(slope.value)


def cnf_pack_schedule(times, method, device):
    """(packed device schedule [slope, dt .., stage_t ..], steps) as nf_cnf_integrate takes it"""
    stage_t, step_dt, slope = cnf_schedule(times, method)
    packed = torch.cat([torch.tensor([slope], dtype=torch.float64), step_dt, stage_t])
    return packed.to(device), step_dt.numel()


def _cnf_check(z, params):
    if not z.is_cuda:
        N.ptr(z)                                                            # raises the engine's "no CPU path" error
    if z.dim() != 2:
        raise RuntimeError('CNF takes (B, D) input, got shape %s' % (tuple(z.shape), ))
    D = z.shape[1]
    H = N.header_constant('NF_CNF_HIDDEN')
    if D > N.header_constant('NF_CNF_MAX_DIM'):
        raise RuntimeError('the CNF kernels serve D <= %d features, got %d' % (N.header_constant('NF_CNF_MAX_DIM'), D))
    want = [(H, D + 1), (H, ), (H, H + 1), (H, ), (D, H + 1), (D, )]
    if len(params) != 6 or [tuple(p.shape) for p in params] != want:
        raise RuntimeError('the CNF kernels serve the field CNF.__init__ builds (D+1 -> 32 -> 32 -> D), got parameter shapes %s'
                           % ([tuple(p.shape) for p in params], ))
    if z.dtype not in _F3264:
        raise RuntimeError('CNF takes float32 or float64 data, got %s' % z.dtype)


def _cnf_table(params):
    return (ctypes.c_int64 * 6)(*[N.ptr(p, _F64) for p in params])


def _cnf_noise_ok(noise, E, B, S, D, trace):
    if noise is None or trace == CNF_TRACES['exact']:
        return None
    if tuple(noise.shape) != (E, B, S, D) or noise.dtype != torch.float32:
        raise RuntimeError('CNF noise must be float32 of shape (E, B, S, D) = %s, got %s %s'
                           % ((E, B, S, D), noise.dtype, tuple(noise.shape)))
    return _contig(noise)


def cnf_integrate(z, ld, params, sched, steps, method, trace='hutchinson', n_samples=1, noise=None, seed=None, want_state=False):
    """``odeint(func, (z, ld), times, method)`` of the field with the six float64 ``params`` in ONE launch, no graph.  ``sched, steps``:
    cnf_pack_schedule(times, method, device).  noise: float32 (E, B, n_samples, D) in evaluation order, or None with ``seed`` (device
    int64[2]: seed, stream offset) for in-kernel draws.  Returns (z, ld) in the input's dtype -- and, with ``want_state``, the final
    float64 state (B, D + 1) OdeIntAdjoint saves (odeint.py:261-262)."""
    with torch.no_grad():
        params = [p.detach() for p in params]
        _cnf_check(z, params)
        m, tr = _cnf_method(method), CNF_TRACES[trace]
        B, D = z.shape
        z = _contig(z)
        ld = _contig(ld.to(z.dtype))
        noise = _cnf_noise_ok(noise, steps * CNF_STAGES[m], B, n_samples, D, tr)
        out, ld_out = torch.empty_like(z), torch.empty_like(ld)
        state = torch.empty((B, D + 1), dtype=torch.float64, device=z.device) if want_state else None
        N.call('nf_cnf_integrate', N.ptr(z, _F3264), N.ptr(ld, _F3264), N.ptr(out, _F3264), N.ptr(ld_out, _F3264), N.ptr(state, _F64),
               _cnf_table(params), N.ptr(sched, _F64), steps, m, tr, n_samples, N.ptr(noise),
               N.ptr(seed, (torch.int64, )) if noise is None and tr == 0 else None, 1 if z.dtype == torch.float64 else 0, B, D,
               N.stream())
    if want_state:
        return out, ld_out, state
    return out, ld_out


def cnf_noise(seed, E, B, S, D):
    """the (E, B, S, D) float32 noise the CNF kernels draw for the seed words ``seed`` (device int64[2]) as they stand now"""
    out = torch.empty((E, B, S, D), dtype=torch.float32, device=seed.device)
    N.call('nf_cnf_noise', N.ptr(out), N.ptr(seed, (torch.int64, )), E, B, S, D, N.stream())
    return out


def cnf_param_count(D):
    H = N.header_constant('NF_CNF_HIDDEN')
    return H * (D + 1) + H + H * (H + 1) + H + D * (H + 1) + D


class _CNFIntegrate(torch.autograd.Function):
    """OdeIntAdjoint (odeint.py:250-284) for both directions of a CNF: the forward saves the final float64 state only, the backward
    integrates (a_z, z, ld) over the reversed schedule in one launch and folds the parameter gradients in a second.  ``cfg``:
    (sched, steps, sched_rev, steps_rev, method, trace, n_samples, draw) -- draw(E) gives the backward pass's noise at backward time
    (fresh draws, as the reference's: odeint.py:237 evaluates the field again), or None for in-kernel noise from ``seed``."""

    @staticmethod
    def forward(ctx, z, ld, cfg, noise, noise_bwd, seed, *params):
        sched, steps, sched_rev, steps_rev, method, trace, S, draw = cfg
        out, ld_out, state = cnf_integrate(z, ld, params, sched, steps, method, trace, S, noise, seed, want_state=True)
        ctx.cfg, ctx.noise_bwd, ctx.seed = cfg, noise_bwd, seed
        ctx.f64 = z.dtype == torch.float64
        ctx.save_for_backward(state, *params)
        return out, ld_out

    @staticmethod
    def backward(ctx, g_z, g_ld):
        state, *params = ctx.saved_tensors
        _, _, sched, steps, method, trace, S, draw = ctx.cfg
        m, tr = _cnf_method(method), CNF_TRACES[trace]
        B, D = state.shape[0], state.shape[1] - 1
        dt = torch.float64 if ctx.f64 else torch.float32
        g_z, g_ld = _contig(g_z.to(dt)), _contig(g_ld.to(dt))
        E = steps * CNF_STAGES[m]
        noise = ctx.noise_bwd
        if noise is None and tr == 0 and draw is not None:
            noise = draw(E)
        noise = _cnf_noise_ok(noise, E, B, S, D, tr)
        seed = ctx.seed if noise is None and tr == 0 else None
        if seed is not None:
            seed[1] += 1                                                    # a stream of its own for this pass (device side, no sync)
        n = ctypes.c_int64(0)
        rc = N.load().nf_cnf_slab_doubles(B, D, ctypes.byref(n))
        if rc != 0:
            raise N.NativeLibraryError('nf_cnf_slab_doubles failed with code %d' % rc)
        slab = torch.empty(max(int(n.value), 1), dtype=torch.float64, device=state.device)
        flat = torch.empty(cnf_param_count(D), dtype=torch.float64, device=state.device)
        a_z, a_ld = torch.empty_like(g_z), torch.empty_like(g_ld)
        with torch.no_grad():
            N.call('nf_cnf_adjoint', N.ptr(state, _F64), N.ptr(g_z, _F3264), N.ptr(g_ld, _F3264), N.ptr(a_z, _F3264), N.ptr(a_ld, _F3264),
                   N.ptr(slab, _F64), N.ptr(flat, _F64), _cnf_table([p.detach() for p in params]), N.ptr(sched, _F64), steps, m, tr, S,
                   N.ptr(noise), N.ptr(seed, (torch.int64, )), 1 if ctx.f64 else 0, B, D, N.stream())
        grads, o = [], 0
        for p in params:
            grads.append(flat[o:o + p.numel()].view(p.shape))
            o += p.numel()
        return (a_z, a_ld, None, None, None, None) + tuple(grads)


def cnf_flow(z, ld, params, cfg, noise=None, noise_bwd=None, seed=None):
    """one direction of a CNF layer (cnf.py:145-173 with backprop='adjoint'): the autograd Function where a gradient is wanted, the
    plain launch otherwise"""
    _cnf_check(z, params)
    ld = ld.to(z.dtype)
    sched, steps, _, _, method, trace, S, _ = cfg
    if torch.is_grad_enabled() and (z.requires_grad or ld.requires_grad or any(p.requires_grad for p in params)):
        return _CNFIntegrate.apply(z, ld, cfg, noise, noise_bwd, seed, *params)
    return cnf_integrate(z, ld, params, sched, steps, method, trace, S, noise, seed)


# ----------------------------------------------------------------------------------------------------------------------
# NLL under the standard-normal prior (training harness, main.py:49-51, :85)
# ----------------------------------------------------------------------------------------------------------------------
class _NLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, ld):
        B = z.shape[0]
        D = z.numel() // B
        loss = WS.zeros_owned((), z.device) if z.dtype == torch.float32 else torch.zeros((), dtype=z.dtype, device=z.device)
        N.call('nf_nll_loss', N.ptr(z), N.ptr(ld), N.ptr(loss), B, D, N.stream())
        ctx.save_for_backward(z)
        return loss

    @staticmethod
    def backward(ctx, g):
        (z, ) = ctx.saved_tensors
        B = z.shape[0]
        D = z.numel() // B
        g = _contig(g)
        g_z = torch.empty_like(z)
        g_ld = torch.empty(B, dtype=z.dtype, device=z.device)
        N.call('nf_nll_loss_bwd', N.ptr(z), N.ptr(g), N.ptr(g_z), N.ptr(g_ld), B, D, N.stream())
        return g_z, g_ld


def nll_loss(z, ld):
    """-mean_b( log N(z_b; 0, I) + ld_b ): one reduction kernel (the reference builds a D x D MultivariateNormal)."""
    return _NLL.apply(_contig(z), _contig(ld))
