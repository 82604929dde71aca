"""
Bijective layers with the reference's nn.Module surface:

    layer(z, log_df_dz)          -> (z', log_df_dz')      forward flow  (data -> latent)
    layer.backward(y, log_df_dz) -> (y', log_df_dz')      INVERSE flow  (latent -> data; not autograd!)

Same class names, constructor signatures, parameter / buffer names and shapes as flows/modules.py,
flows/coupling.py, flows/squeeze.py and flows/maf.py, so reference ``state_dict``s load unchanged.  The
transforms themselves run as HIP kernels (functional.py -> libnfhip.so); there is no CPU path.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N
from . import functional as NF
from . import fused as FUSED
from . import fused_flowpp_img as FPI
from .conditioners import MLP, ConvNet, flowpp_conditioner, made_degrees_to_masks, made_masks_from_degrees


class Identity(nn.Module):
    def forward(self, x, log_df_dz):
        return x, log_df_dz

    def backward(self, x, log_df_dz):
        return x, log_df_dz


GLOW_HEAD_W_ON = True           # (internal: the MFMA head of image flow steps, csrc/glow_head_mfma.hip)
HEAD_IN_CHAIN = True            # (internal: that head's forward in the prologue of the coupling's chain launch, csrc/conv_chain.hip)
FLOWPP_HEAD_ON = True           # (internal: image Flow++ steps take the fused Glow heads too; tests compare with the three layers' own launches)


def _unhooked(*mods, backward=()):
    """no forward or pre-forward hook on any of ``mods`` and no backward hook on any of ``backward``: the fused launches run none
    of them (the reference's debug mode registers NaN hooks, main.py:312-313)"""
    for m in mods:
        if m._forward_hooks or m._forward_pre_hooks:
            return False
    for m in backward:
        if m._backward_hooks:
            return False
    return True


def _vector_coupling(k):
    """an AffineCoupling over the two halves of a vector whose conditioner is the MLP the fused vector steps carry"""
    return type(k) is AffineCoupling and k.mode == N.SPLIT_1D and isinstance(k.net, MLP)


def _autoregressive(k):
    return type(k) is AutoregressiveTransfrom


class Compose(nn.Module):
    """flows/modules.py:325-339.  Both directions walk the layers through an ordered list of routes (``_FORWARD``, ``_INVERSE``; DESIGN.md
    section 4): each route recognises a step shape at the current layer -- a run of planar layers, of ResFlow pairs, of vector Glow,
    RealNVP or MAF steps, one flow-BatchNorm or Glow step, a Flow++ pair -- and serves it with the fused launches of fused.py /
    functional.py, or declines; the last route is the layer's own call.  Earlier routes shadow later ones.  Same math, same parameters,
    same state_dict; every fused route declines when a member carries forward hooks, when ``fuse`` is off and in the
    synchronised-statistics parity mode."""

    fuse = True
    _resflow_draws = 'host'         # (ResFlow.draws: where the whole-stack ResFlow kernels take series lengths and noise from)
    _resflow_seed = None            # (ResFlow.seed: device int64[2], the seed words of draws = 'device')

    def __init__(self, layers):
        super().__init__()
        self.layers = nn.ModuleList(layers)

    @property
    def _fuse_now(self):
        """peephole fusion is off in the synchronised-statistics parity mode: the fused kernels take their batch statistics
        in-kernel, per replica (dist.sync_statistics)"""
        from . import dist as nfdist
        return self.fuse and not nfdist.sync_stats_active()

    # ---- matchers: one per step shape, the members or None ---------------------------------------------------------------------------
    @staticmethod
    def _flowpp_image_coupling(k, z):
        """an image Flow++ step [ActNorm, InvertibleConv1x1, MixLogAttnCoupling] (flows/flowpp.py:64-70) takes the same fused head as a Glow
        step: ActNorm + 1x1 + the conditioner-input gather in one launch, its backward in two parts (round 5)"""
        return FLOWPP_HEAD_ON and type(k) is MixLogAttnCoupling and z.dim() == 4 and k.mode in (N.SPLIT_CHANNEL, N.SPLIT_CHECKER)

    def _glow_triple_at(self, i, z):
        """[ActNorm, InvertibleConv1x1, AffineCoupling | image MixLogAttnCoupling] at layers i .. i + 2, whatever the channel count"""
        L = self.layers
        if not (self._fuse_now and z.is_cuda and 0 <= i and i + 2 < len(L)):
            return None
        a, c, k = L[i], L[i + 1], L[i + 2]
        if not (type(a) is ActNorm and type(c) is InvertibleConv1x1 and (type(k) is AffineCoupling or self._flowpp_image_coupling(k, z))):
            return None
        return (a, c, k) if _unhooked(a, c, k) else None

    def _glow_vec_step_at(self, i, z):
        """the Glow triple at i whose coupling is a vector coupling: a member of the fused runs of both directions"""
        m = self._glow_triple_at(i, z) if z.shape[1] <= NF.HEAD_MAX_C else None
        return m if m is not None and _vector_coupling(m[2]) else None

    def _bn_pair_at(self, i, z, training_only, kind=None):
        """[flow BatchNorm(affine=False), AffineCoupling | AutoregressiveTransfrom] at layers i, i + 1.  ``training_only``: the BatchNorm
        in training mode on any data (the fused BatchNorm head and the steps built on it); otherwise any mode, vector data (the
        evaluation and inverse launches).  ``kind``: a narrower test of the second layer (_vector_coupling | _autoregressive)"""
        L = self.layers
        if not (self._fuse_now and z.is_cuda and 0 <= i and i + 1 < len(L) and (training_only or z.dim() == 2)):
            return None
        a, k = L[i], L[i + 1]
        if not (type(a) is BatchNorm and not isinstance(a.log_gamma, nn.Parameter) and (a.training or not training_only)):
            return None
        if not (kind(k) if kind is not None else type(k) is AffineCoupling or type(k) is AutoregressiveTransfrom):
            return None
        return (a, k) if _unhooked(a, k) else None

    def _realnvp_any_mode_at(self, i, z):
        return self._bn_pair_at(i, z, False, _vector_coupling)

    def _flowpp_pair_at(self, i, z):
        """[MixLogAttnCoupling, ActNorm (initialised)] on two features -> the next step's ActNorm rides the coupling's launches"""
        L = self.layers
        if not (self._fuse_now and z.is_cuda and 0 <= i and i + 1 < len(L)):
            return None
        k, a = L[i], L[i + 1]
        if not (type(k) is MixLogAttnCoupling and type(a) is ActNorm and k.mode == N.SPLIT_1D):
            return None
        return (k, a) if _unhooked(a, k) and FUSED.flowpp_post_actnorm_usable(z, k, a) else None

    # ---- runs ------------------------------------------------------------------------------------------------------------------------
    def _collect(self, i, z, step, width, member):
        """the maximal run of steps of ``width`` layers each, in forward order.  step +1: layer i is the first layer of the first step;
        -1: layer i is the last layer of the last step.  ``member(j, z)`` yields the step that starts at layer j, or None"""
        run, j, n = [], (i if step > 0 else i - width + 1), len(self.layers)
        while 0 <= j and j + width <= n:
            m = member(j, z)
            if m is None:
                break
            run.append(m)
            j += step * width
        return run if step > 0 else run[::-1]

    def _planar_run(self, i, z, step):
        """the maximal run of PlanarTransforms without hooks from layer i on, on the GPU"""
        L = self.layers
        if not z.is_cuda:
            return []
        return self._collect(i, z, step, 1, lambda j, z: L[j] if type(L[j]) is PlanarTransform and _unhooked(L[j]) else None)

    def _resflow_run(self, i, z, step):
        """the maximal run of [ActNorm (initialised), InvertibleResLinear] pairs from layer i on (step +1: i is the first pair's ActNorm;
        -1: i is the last pair's block), as [(ActNorm, block), ..] in forward order -- blocks the HIP kernels serve (``_hip_ok``: D <= 4,
        hidden width 32, two LipSwish layers, float32 on the GPU), of one mind (mode, estimator, coeff, ftol, noise source), no hooks.
        While an ActNorm awaits its data-dependent initialisation the per-layer path runs."""
        from .resflow import InvertibleResLinear
        L, first = self.layers, []
        if not (NF.RESFLOW_STACK and z.is_cuda):
            return []

        def mind(k):
            return (k.training, k.estimator, k.coeff, k.ftol, k.noise_on_cpu, k._sn_eps())

        def member(j, z):
            a, k = L[j], L[j + 1]
            if not (type(a) is ActNorm and type(k) is InvertibleResLinear and a.initialized and k._hip_ok(z)):
                return None
            if not _unhooked(a, k, backward=(a, k)):               # (the one route that looks at both members' backward hooks)
                return None
            if step > 0 and not ((not k.training and not torch.is_grad_enabled()) or (k.training and torch.is_grad_enabled() and k.hip_training)):
                return None                                        # (the combinations the block itself serves with kernels, resflow.py)
            if first and mind(k) != mind(first[0]):                # of one mind with the first member collected
                return None
            first.append(k)
            return a, k
        return self._collect(i, z, step, 2, member)

    # ---- forward routes: (i, z, ld) -> (z, ld, layers consumed), or None where the route does not serve layer i ------------------------
    def _planar(self, i, z, ld):
        run = self._planar_run(i, z, 1) if self._fuse_now else []
        if run:                                                    # the run of planar layers: projection + one launch
            return (*NF.planar_flow(z, ld, run), len(run))

    def _resflow(self, i, z, ld):
        run = self._resflow_run(i, z, 1) if self._fuse_now else []
        if run:                                                    # the run of residual blocks: a handful of launches whatever its length
            return (*NF.resflow_flow(z, ld, run, self._resflow_draws, self._resflow_seed), 2 * len(run))

    def _realnvp_eval(self, i, z, ld):
        run = [] if torch.is_grad_enabled() else self._collect(i, z, 1, 2, self._realnvp_any_mode_at)
        if run and FUSED.realnvp_eval_usable(z, run):              # density evaluation: the run in one launch, no exchange
            return (*FUSED.realnvp_flow_vec_eval(z, ld, run), 2 * len(run))

    def _maf_eval(self, i, z, ld):
        m = self._bn_pair_at(i, z, False, _autoregressive)
        if m is not None and FUSED.maf_step_eval_usable(z, *m):    # density evaluation: one launch, no exchange
            return (*FUSED.maf_step_eval(z, ld, *m), 2)

    def _bn_step(self, i, z, ld):
        """a training-mode flow BatchNorm in front of a coupling or a MADE transform: the run of steps, the whole step, or the fused
        BatchNorm head in front of the second layer's own launches"""
        m = self._bn_pair_at(i, z, True)
        if m is None:
            return None
        a, k = m
        if _vector_coupling(k):
            run = self._collect(i, z, 1, 2, lambda j, z: self._bn_pair_at(j, z, True, _vector_coupling)) if z.dim() == 2 else []
            if FUSED.realnvp_flow_vec_usable(z, run):              # the whole run of steps: one launch per direction
                return (*FUSED.realnvp_flow_vec(z, ld, run), 2 * len(run))
            if FUSED.realnvp_step_vec_usable(z, a, k.net):
                return (*FUSED.realnvp_step_vec(z, ld, a, k), 2)                  # the whole step: one launch
        if type(k) is AffineCoupling:
            h, z1c, ld = NF.flowbn_head(z, ld, a, k.mode, k.odd, gather=True)
            return (*k.couple(h, z1c, ld), 2)
        if FUSED.maf_step_usable(z, a, k):
            run = self._collect(i, z, 1, 2, lambda j, z: self._bn_pair_at(j, z, True, _autoregressive)) if z.dim() == 2 else []
            if FUSED.maf_flow_vec_usable(z, run):                  # the run as one autograd node, one fold for all steps
                return (*FUSED.maf_flow_vec(z, ld, run), 2 * len(run))
            return (*FUSED.maf_step_vec(z, ld, a, k), 2)                          # the whole step: one launch
        h, ld = NF.flowbn_head(z, ld, a)
        return (*k(h, ld), 2)

    def _glow_step(self, i, z, ld):
        """a Glow flow step on vector data or on up to HEAD_MAX_C channels: the run of steps, the whole step, or the head + the coupling"""
        m = self._glow_triple_at(i, z) if z.shape[1] <= NF.HEAD_MAX_C else None
        if m is None:
            return None
        a, c, k = m
        if z.dim() == 2:
            # (initialised ActNorms, training-mode conditioners of one mind; the `usable` tests ask for direct gradient sinks)
            def member(j, z, training=k.net.training):
                s = self._glow_vec_step_at(j, z)
                return s if s is not None and s[0].initialized and s[2].net.training == training else None
            run = self._collect(i, z, 1, 3, member)
            if FUSED.glow_flow_nograd_usable(z, run):              # density evaluation: no autograd node at all
                return (*FUSED.glow_flow_vec_nograd(z, ld, run), 3 * len(run))
            if FUSED.glow_flow_vec_usable(z, run):                 # the whole run of steps: one launch per direction
                return (*FUSED.glow_flow_vec(z, ld, run), 3 * len(run))
        if _vector_coupling(k) and FUSED.glow_step_vec_usable(z, k.net):
            self._actnorm_init(a, z)
            return (*FUSED.glow_step_vec(z, ld, a, c, k), 3)                      # the whole step: one launch
        return self._head_step(a, c, k, z, ld)

    def _glow_chain_run(self, i, z, ld):
        """consecutive image Glow steps of one shape where a workgroup of the chain kernels owns whole samples (the 8 x 8 and 4 x 4 levels
        of the CIFAR pyramid): every step as in _head_step -- its own autograd nodes, its head left to its coupling's chain launch --
        but the chain launches of the run leave as ONE (fused_conv.chain_run).  Declines, and the per-step routes serve, for fewer than
        fused_conv.CHAIN_RUN_MIN steps, while a
        member's ActNorm awaits its initialisation, when the members' conditioners are not of one training mode, when a head would
        not ride its chain launch, and on the halo hand-over shapes (16 x 16 maps on two tiles per sample)."""
        from . import fused_conv as FC
        if not (FC.CHAIN_RUNS_ON and GLOW_HEAD_W_ON and HEAD_IN_CHAIN and z.dim() == 4 and z.shape[1] > NF.HEAD_MAX_C and z.is_contiguous()):
            return None
        first = []

        def member(j, z):
            m = self._glow_triple_at(j, z)
            if m is None:
                return None
            a, c, k = m
            if not (a.initialized and type(k) is AffineCoupling and isinstance(k.net, ConvNet) and c._W_eff is not None
                    and k.mode in (N.SPLIT_CHANNEL, N.SPLIT_CHECKER) and (not first or (k.net.training, k.mode) == first[0])
                    and NF.glow_head_w_usable(z, k.mode) and FC.chain_run_ok(k.net, z, k.mode)):
                return None
            first.append((k.net.training, k.mode))
            return m
        run = self._collect(i, z, 1, 3, member)
        if len(run) < FC.CHAIN_RUN_MIN:                            # (a pair of steps keeps its two launches: nothing measurable to gain)
            return None
        with FC.chain_run():
            for a, c, k in run:
                out = self._head_step(a, c, k, z, ld)
                if out is None:
                    raise RuntimeError('a member of a run of Glow steps declined its fused head (the route tested the same conditions)')
                z, ld = out[:2]
        return z, ld, 3 * len(run)

    def _glow_step_w(self, i, z, ld):
        """image data with more channels than the in-kernel PLU head takes (9 .. 64): head in one MFMA launch"""
        m = self._glow_triple_at(i, z) if GLOW_HEAD_W_ON and z.dim() == 4 and z.shape[1] > NF.HEAD_MAX_C else None
        if m is not None:
            # (the run of such steps first: part of this route, not an entry of its own -- the route list is the documented order)
            return self._glow_chain_run(i, z, ld) or self._head_step(*m, z, ld)

    @staticmethod
    def _actnorm_init(a, z):
        if not a.initialized:
            NF.actnorm_init_(z, a.log_scale, a.bias, a.eps)
            a.initialized = True

    def _head_step(self, a, c, k, z, ld):
        """one flow step as the fused head (ActNorm + 1x1 + the coupling's split-gather in one launch) and the coupling's own launches.
        Up to HEAD_MAX_C channels the head factors the PLU weight in the kernel (functional.glow_head); above, it multiplies by the
        weight the model's batched PLU pre-pass assembled, on the MFMA units (functional.glow_head_w) -- or declines where that head
        does not serve."""
        wide = z.shape[1] > NF.HEAD_MAX_C
        if wide and (c._W_eff is None or k.mode not in (N.SPLIT_CHANNEL, N.SPLIT_CHECKER) or not NF.glow_head_w_usable(z, k.mode)):
            return None
        self._actnorm_init(a, z)
        # image data: the head's forward rides the prologue of the coupling's chain launch when that launch follows (round 5) ...
        from . import fused_conv as FC
        defer = (HEAD_IN_CHAIN and z.dim() == 4 and type(k) is AffineCoupling and isinstance(k.net, ConvNet) and z.is_contiguous()
                 and FC.head_in_chain_ok(k.net, z, k.mode))
        # ... and its data gradient the prologue of the PREVIOUS step's backward chain launch, when z is that launch's output (round 6)
        bwd_defer = defer and NF.from_fused_coupling(z)
        if wide:
            W, holder, idx = c._W_eff
            h, z1c, ld = NF.glow_head_w(z, ld, a.log_scale, a.bias, W, c.log_s, holder, idx, k.mode, k.odd, defer=defer, bwd_defer=bwd_defer)
        else:
            h, z1c, ld = NF.glow_head(z, ld, a.log_scale, a.bias, c.P, c.L, c.U, c.L_mask, c.U_mask, c.sign_s, c.log_s, k.mode, k.odd,
                                      bwd_defer=bwd_defer, defer=defer)
        z, ld = k.couple(h, z1c, ld)
        if defer and NF.flush_pending_head(h):
            raise RuntimeError('a deferred Glow head was not performed by its coupling launch')
        return z, ld, 3

    def _flowpp_pair(self, i, z, ld):
        m = self._flowpp_pair_at(i, z)
        if m is not None:                                          # coupling + next ActNorm
            return (*FUSED.flowpp_coupling_vec(z, ld, m[0], post=m[1]), 2)

    def _layer(self, i, z, ld):
        return (*self.layers[i](z, ld), 1)

    _FORWARD = (_planar, _resflow, _realnvp_eval, _maf_eval, _bn_step, _glow_step, _glow_step_w, _flowpp_pair, _layer)

    def forward(self, z, log_df_dz):
        i, n = 0, len(self.layers)
        while i < n:
            for route in self._FORWARD:                            # in priority order; _layer serves whatever the others decline
                out = route(self, i, z, log_df_dz)
                if out is not None:
                    z, log_df_dz, used = out
                    i += used
                    break
        return z, log_df_dz

    # ---- inverse routes: layer i is the LAST layer of what a route serves; all of them run under no_grad (see backward) ----------------
    def _planar_inverse(self, i, z, ld):
        run = self._planar_run(i, z, -1) if self._fuse_now else []
        if run:                                                    # the run of planar layers: one bisection launch (or 3 per layer)
            return (*NF.planar_inverse(z, ld, run)[:2], len(run))

    def _resflow_inverse(self, i, z, ld):
        run = self._resflow_run(i, z, -1) if (self._fuse_now and z.dim() == 2
                                              and z.shape[0] <= N.header_constant('NF_RESFLOW_INV_WG_MAX_ROWS')) else []
        if run:                                                    # the run of residual blocks: the whole inverse in one workgroup
            return (*NF.resflow_inverse(z, ld, run, self._resflow_draws, self._resflow_seed)[:2], 2 * len(run))

    def _glow_inverse(self, i, z, ld):
        """the run of fused-step-capable Glow steps on (N, 2 | 4) data that ends at layer i: one launch per step, or one for the run"""
        if z.dim() != 2:
            return None

        def member(j, z):
            s = self._glow_vec_step_at(j, z)
            # (the coupling's backward hooks alone: those of the ActNorm and the 1x1 are not looked at here -- kept as found)
            return s if s is not None and _unhooked(backward=(s[2], )) else None
        run = self._collect(i, z, -1, 3, member)
        if run and FUSED.glow_inverse_usable(z, run):
            return (*FUSED.glow_flow_vec_inverse(z, ld, run), 3 * len(run))

    def _realnvp_inverse(self, i, z, ld):
        run = self._collect(i, z, -1, 2, self._realnvp_any_mode_at)
        if run and FUSED.realnvp_inverse_usable(z, run):
            return (*FUSED.realnvp_flow_vec_inverse(z, ld, run), 2 * len(run))

    def _maf_inverse(self, i, z, ld):
        m = self._bn_pair_at(i - 1, z, False, _autoregressive)
        if m is not None and FUSED.maf_step_inverse_usable(z, *m):
            # one launch per step; with device draws it reads a mask set per pass (the two names are the two mask sources of one body)
            inverse = FUSED.maf_step_inverse_drawn if FUSED.maf_device_draws(m[1]) else FUSED.maf_step_inverse
            return (*inverse(z, ld, *m), 2)

    def _layer_inverse(self, i, z, ld):
        return (*self.layers[i].backward(z, ld), 1)

    _INVERSE = (_planar_inverse, _resflow_inverse, _glow_inverse, _realnvp_inverse, _maf_inverse, _layer_inverse)

    def backward(self, z, log_df_dz):
        """INVERSE flow (sampling).  The sampling kernels build no autograd graph: without a request for one the whole pass runs under
        no_grad (the reference's ``sample_y``, main.py:113, leaves autograd on and never uses the graph).  An input that requires grad --
        or the ``differentiable_inverse()`` context, for gradients of the parameters alone -- takes the graph-building form of every
        layer's inverse instead (inverse_grad.py: the reference's formulas over the engine's own conditioners and gathers).
        Invariant: past the first branch below grad is off, so no inverse route has an autograd case to tell apart."""
        if torch.is_grad_enabled():
            from . import inverse_grad as IG
            if IG.wanted(z, log_df_dz):
                return IG.layer_inverse(self, z, log_df_dz)
            with torch.no_grad():
                return self.backward(z, log_df_dz)
        i = len(self.layers) - 1
        while i >= 0:
            for route in self._INVERSE:
                out = route(self, i, z, log_df_dz)
                if out is not None:
                    z, log_df_dz, used = out
                    i -= used
                    break
        return z, log_df_dz


class Logit(nn.Module):
    """flows/modules.py:141-156"""

    def __init__(self, eps=1.0e-5):
        super().__init__()
        self.eps = eps

    def forward(self, x, log_df_dz):
        return NF.logit(x, log_df_dz, self.eps)

    def backward(self, x, log_df_dz):
        return NF.logit(x, log_df_dz, self.eps, inverse=True)


class Sigmoid(nn.Module):
    """flows/modules.py:125-138"""

    def forward(self, x, log_df_dz):
        return NF.bijector(x, log_df_dz, NF.BIJ_SIGMOID)

    def backward(self, x, log_df_dz):
        return NF.bijector(x, log_df_dz, NF.BIJ_SIGMOID_INV)


class Tanh(nn.Module):
    """flows/modules.py:158-170"""

    def forward(self, x, log_df_dz):
        return NF.bijector(x, log_df_dz, NF.BIJ_TANH)

    def backward(self, x, log_df_dz):
        with torch.no_grad():
            return NF.bijector(x, log_df_dz, NF.BIJ_ARCTANH)


class Arctanh(nn.Module):
    """flows/modules.py:173-183 (its log-det sums over dim 1: vector data)"""

    def forward(self, x, log_df_dz):
        return NF.bijector(x, log_df_dz, NF.BIJ_ARCTANH)

    def backward(self, x, log_df_dz):
        with torch.no_grad():
            return NF.bijector(x, log_df_dz, NF.BIJ_TANH)


class Squeeze1d(nn.Module):
    """flows/squeeze.py:114-132: the alternating entries of a vector as two concatenated halves"""

    def __init__(self, odd=False):
        super().__init__()
        self.odd = bool(odd)

    def forward(self, z, log_df_dz):
        return NF.squeeze1d(z, self.odd), log_df_dz

    def backward(self, z, log_df_dz):
        return NF.squeeze1d(z, self.odd, inverse=True), log_df_dz


class Unsqueeze1d(nn.Module):
    """flows/squeeze.py:135-151: the inverse map of Squeeze1d as a forward layer"""

    def __init__(self, odd=False):
        super().__init__()
        self.odd = bool(odd)

    def forward(self, z, log_df_dz):
        return NF.squeeze1d(z, self.odd, inverse=True), log_df_dz

    def backward(self, z, log_df_dz):
        return NF.squeeze1d(z, self.odd), log_df_dz


class MixLogCDF(nn.Module):
    """flows/modules.py:186-212: CDF of a mixture of logistics as a bijector of x given (log_pi, mu, s); the inverse is the
    reference's bisection (25 or 100 iterations by its batch-global exit rule).  One HIP launch forward, two inverse."""

    def forward(self, x, log_pi, mu, s, log_df_dz):
        return NF.mixlogcdf(x, log_pi, mu, s, log_df_dz)

    def backward(self, x, log_pi, mu, s, log_df_dz):
        return NF.mixlogcdf(x, log_pi, mu, s, log_df_dz, inverse=True)


class PlanarTransform(nn.Module):
    """flows/planar.py:9-68.  Same parameters (u, w of shape (1, dim), b of shape (1,)), same construction draws and projection; the
    forward projects u in place on the GPU (no ``.item()`` host sync) and a Compose runs a whole stack of these in one launch per
    direction (functional.planar_flow / planar_inverse)."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        u = torch.randn(1, self.dim) * 0.01
        w = torch.randn(1, self.dim) * 0.01
        b = torch.randn(1) * 0.01
        self.register_parameter('u', nn.Parameter(u))
        self.register_parameter('w', nn.Parameter(w))
        self.register_parameter('b', nn.Parameter(b))
        self._make_invertible()

    def _make_invertible(self):
        """planar.py:23-33 with torch ops where the parameters live (construction: the CPU, as the reference); the flow itself
        projects in its forward launch sequence (functional.planar_project_)"""
        if self.u.is_cuda:
            NF.planar_project_([self])
            return
        with torch.no_grad():
            w_dot_u = torch.mm(self.u, self.w.t())
            if w_dot_u.item() >= -1.0:
                return
            norm_w = self.w / torch.norm(self.w, p=2, dim=1)**2
            bias = -1.0 + F.softplus(w_dot_u)
            self.u.data = self.u + (bias - w_dot_u) * norm_w

    def forward(self, z, log_df_dz):
        return NF.planar_flow(z, log_df_dz, [self])

    def backward(self, z, log_df_dz):
        z, log_df_dz, _ = NF.planar_inverse(z, log_df_dz, [self])
        return z, log_df_dz


class ConcatLinear(nn.Module):
    """flows/cnf.py:40-51: a Linear on [t, x]; column 0 of the weight multiplies t.  A parameter holder here: the field runs inside the
    CNF kernels (functional.cnf_flow), never layer by layer."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.linear = nn.Linear(in_features + 1, out_features)

    def forward(self, t, x):
        raise NotImplementedError('the engine evaluates the field inside the CNF integration kernels (csrc/cnf.hip); call CNF / '
                                  'flows.odeint.odeint on the ODENet instead of its layers')


class ODENet(nn.Module):
    """flows/cnf.py:68-121 for density data: three ConcatLinear layers dims[0]+1 -> 32 -> 32 -> dims[0] with softplus between them, same
    construction draws and parameter names.  ``noise_on_cpu`` (default False: the Hutchinson noise is drawn in the kernel, Philox keyed
    by torch.initial_seed() and a per-pass stream offset): True draws it per evaluation from the CPU default generator in float32,
    in the reference's order (cnf.py:29), the backward pass's draws included, and ships a pass's draws in one copy.
    ``noise_source`` (tests): a callable (E, B, S, D) -> float32 tensor that replaces the draws of every pass."""

    def __init__(self, dims, base_filters=32, n_layers=2, trace_estimator='hutchinson', noise_on_cpu=False):
        super().__init__()
        self.estimator = trace_estimator
        self.noise_on_cpu = bool(noise_on_cpu)
        self.noise_source = None
        self._seed = None
        if len(dims) == 3:
            raise NotImplementedError('Sorry, FFJORD for image generation is not supported!')
        if len(dims) != 1:
            raise Exception('unsupported target dimension: %s' % (str(dims)))
        hidden_dims = [dims[0]] + [base_filters] * n_layers + [dims[0]]
        self.layers = nn.ModuleList([ConcatLinear(i, o) for i, o in zip(hidden_dims[:-1], hidden_dims[1:])])

    def trace_mode(self):
        """(trace, samples) as ODENet._get_trace_estimator picks them (cnf.py:92-105): training forces Hutchinson with one sample"""
        if self.training:
            return 'hutchinson', 1
        if self.estimator == 'exact':
            return 'exact', 1
        if self.estimator == 'hutchinson':
            return 'hutchinson', 4
        raise RuntimeError('unknown trace estimator %r' % (self.estimator, ))

    def field_params(self):
        return [p for m in self.layers for p in (m.linear.weight, m.linear.bias)]

    def draw(self, E, B, S, D, device):
        """the noise of one pass, (E, B, S, D) float32 on ``device``, or None for in-kernel draws"""
        if self.noise_source is not None:
            return self.noise_source(E, B, S, D).to(device=device, dtype=torch.float32)
        if not self.noise_on_cpu:
            return None
        w = torch.stack([torch.randn([B, S, D]) for _ in range(E)])        # cnf.py:29, one draw per field evaluation
        return w.to(device, non_blocking=True)

    def seed(self, device):
        """device int64[2] (seed, stream offset) of the in-kernel noise; the offset moves on with every pass"""
        if self._seed is None or self._seed.device != device:
            self._seed = torch.tensor([torch.initial_seed() & 0x7fffffffffffffff, 0], dtype=torch.int64, device=device)
        self._seed[1] += 1
        return self._seed

    def forward(self, t, states):
        raise NotImplementedError('the engine evaluates the field inside the CNF integration kernels (csrc/cnf.hip); use CNF or '
                                  'flows.odeint.odeint(func, states, times, method)')


def odeint(func, x, times, method, noise=None, noise_bwd=None):
    """flows/odeint.py:201-214 and :217-224 on the engine's ODENet: the whole integration in one launch; with autograd on and a gradient
    wanted it is the adjoint form (the only one the engine has).  x: (z, log_df_dz); returns the pair at times[-1]."""
    if not isinstance(func, ODENet):
        raise TypeError('the engine integrates its own ODENet only, got %s' % type(func).__name__)
    if isinstance(x, torch.Tensor) or not isinstance(x, tuple) or len(x) != 2:
        raise Exception('"odeint" input must be the tuple (z, log_df_dz)')
    z, ld = x
    params = func.field_params()
    if not z.is_cuda:
        N.ptr(z)
    trace, S = func.trace_mode()
    dev = z.device
    times = torch.as_tensor(times).detach()
    sched, steps = NF.cnf_pack_schedule(times, method, dev)
    sched_rev, steps_rev = NF.cnf_pack_schedule(torch.flip(times, dims=[0]), method, dev)
    B, D = z.shape
    cfg = (sched, steps, sched_rev, steps_rev, method, trace, S,
           lambda E: func.draw(E, B, S, D, dev))
    if noise is None and trace == 'hutchinson':
        noise = func.draw(steps * NF.CNF_STAGES[NF.CNF_METHODS[method]], B, S, D, dev)
    seed = func.seed(dev) if trace == 'hutchinson' and not func.noise_on_cpu and func.noise_source is None else None
    return NF.cnf_flow(z, ld, params, cfg, noise, noise_bwd, seed)


odeint_adjoint = odeint


class CNF(nn.Module):
    """flows/cnf.py:124-173.  Same constructor, attributes, float64 field parameters and ``times`` buffer; ``forward`` integrates over
    the flipped times, ``backward`` over the times as stored, each in one launch (functional.cnf_flow) with the adjoint gradient of
    odeint.py:250-284.  ``backprop='normal'`` constructs and raises NotImplementedError when run.  ``noise`` / ``noise_bwd``: explicit
    Hutchinson noise of the pass and of its backward pass, float32 (E, B, S, D) in evaluation order (tests)."""

    def __init__(self, dims, times, solver_type, trace_estimator='hutchinson', backprop='adjoint', dtype=torch.float64,
                 noise_on_cpu=False):
        super().__init__()
        assert backprop in ['normal', 'adjoint'], 'unsupported backprop type "%s"' % (backprop)
        self.dims = dims
        self.dtype = dtype
        self.func = ODENet(dims, trace_estimator=trace_estimator, noise_on_cpu=noise_on_cpu).type(self.dtype)
        self.method = solver_type
        self.backprop = backprop
        self.register_buffer('times', times.type(self.dtype))
        self._sched = {}

    @property
    def noise_on_cpu(self):
        return self.func.noise_on_cpu

    @noise_on_cpu.setter
    def noise_on_cpu(self, v):
        self.func.noise_on_cpu = bool(v)

    def _schedules(self, flipped, device):
        """the packed device schedules of this direction and of its adjoint, rebuilt when ``times`` or the method changed"""
        key = (bool(flipped), str(device))
        tag = (self.times.data_ptr(), self.times._version, self.method)
        hit = self._sched.get(key)
        if hit is None or hit[0] != tag:
            t = self.times.detach().cpu()
            a, b = (torch.flip(t, dims=[0]), t) if flipped else (t, torch.flip(t, dims=[0]))
            hit = self._sched[key] = (tag, NF.cnf_pack_schedule(a, self.method, device), NF.cnf_pack_schedule(b, self.method, device))
        return hit[1], hit[2]

    def _run(self, z, log_df_dz, flipped, noise, noise_bwd):
        if not z.is_cuda:
            N.ptr(z)                                                        # the engine's "no CPU path" error
        if self.backprop == 'normal':
            raise NotImplementedError('CNF(backprop="normal") is not served by the engine: the kernels implement the adjoint form '
                                      '(flows/odeint.py:250-284), the only one Ffjord can select')
        if self.dtype != torch.float64:
            raise NotImplementedError('the CNF kernels integrate in float64 (the reference\'s default), got dtype=%s' % self.dtype)
        func, dev = self.func, z.device
        (sched, steps), (sched_rev, steps_rev) = self._schedules(flipped, dev)
        trace, S = func.trace_mode()
        B, D = z.shape[0], z.shape[-1]
        cfg = (sched, steps, sched_rev, steps_rev, self.method, trace, S, lambda E: func.draw(E, B, S, D, dev))
        seed = None
        if trace == 'hutchinson':
            if noise is None:
                noise = func.draw(steps * NF.CNF_STAGES[NF.CNF_METHODS[self.method]], B, S, D, dev)
            if not func.noise_on_cpu and func.noise_source is None:
                seed = func.seed(dev)
        return NF.cnf_flow(z, log_df_dz, func.field_params(), cfg, noise, noise_bwd, seed)

    def forward(self, z, log_df_dz, noise=None, noise_bwd=None):
        return self._run(z, log_df_dz, True, noise, noise_bwd)

    def backward(self, z, log_df_dz, noise=None, noise_bwd=None):
        return self._run(z, log_df_dz, False, noise, noise_bwd)


def _param_shape(num_features):
    dims = [1] + [1 for _ in num_features]
    dims[1] = num_features[0]
    return dims


class ActNorm(nn.Module):
    """flows/modules.py:225-256.  ``initialized`` is a plain attribute exactly like the reference's (it is not in
    the state_dict, so the first batch after ``load_state_dict`` re-initialises -- appendix D Q2); set it to True to
    keep loaded values."""

    def __init__(self, num_features, eps=1.0e-5):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.dimensions = _param_shape(num_features)
        self.log_scale = nn.Parameter(torch.zeros(self.dimensions))
        self.bias = nn.Parameter(torch.zeros(self.dimensions))
        self.initialized = False

    def forward(self, z, log_df_dz):
        if not self.initialized:
            from . import dist as nfdist
            if nfdist.sync_stats_active():              # parity mode: the initialisation statistics of the GLOBAL batch
                with torch.no_grad():
                    mean, var, n = nfdist.global_moments(z)
                    std = torch.sqrt(var * (n / (n - 1.0)))                  # unbiased, modules.py:240
                    self.log_scale.data.copy_(torch.log(std + self.eps).view(self.dimensions))
                    self.bias.data.copy_(mean.view(self.dimensions))
            else:
                NF.actnorm_init_(z, self.log_scale, self.bias, self.eps)
            self.initialized = True
        return NF.chan_affine(N.OP_ACTNORM, z, log_df_dz, self.log_scale, self.bias)

    def backward(self, y, log_df_dz):
        return NF.chan_affine(N.OP_ACTNORM, y, log_df_dz, self.log_scale, self.bias, inverse=True)


class BatchNorm(nn.Module):
    """flow BatchNorm, flows/modules.py:259-322: batch statistics are constants for autograd; biased variance
    with eps stored inside; inverse uses the batch buffers in train mode."""

    def __init__(self, num_features, momentum=0.1, eps=1.0e-5, affine=True):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.dimensions = _param_shape(num_features)
        if affine:
            self.log_gamma = nn.Parameter(torch.zeros(self.dimensions))
            self.beta = nn.Parameter(torch.zeros(self.dimensions))
        else:
            self.register_buffer('log_gamma', torch.zeros(self.dimensions))
            self.register_buffer('beta', torch.zeros(self.dimensions))
        self.register_buffer('running_mean', torch.zeros(self.dimensions))
        self.register_buffer('running_var', torch.ones(self.dimensions))
        self.register_buffer('batch_mean', torch.zeros(self.dimensions))
        self.register_buffer('batch_var', torch.ones(self.dimensions))

    def _stats(self):
        if self.training:
            return self.batch_mean, self.batch_var
        return self.running_mean, self.running_var

    def forward(self, x, log_det_jacob):
        from . import dist as nfdist
        if self.training and nfdist.sync_stats_active():    # parity mode: statistics of the GLOBAL batch (modules.py:284-294)
            with torch.no_grad():
                mean, var, _ = nfdist.global_moments(x)
                self.batch_mean.copy_(mean.view(self.dimensions))
                self.batch_var.copy_((var + self.eps).view(self.dimensions))
                self.running_mean.mul_(1.0 - self.momentum).add_(self.batch_mean * self.momentum)
                self.running_var.mul_(1.0 - self.momentum).add_(self.batch_var * self.momentum)
        elif self.training:
            NF.flowbn_update_(x, self.batch_mean, self.batch_var, self.running_mean, self.running_var, self.eps,
                              self.momentum)
        mean, var = self._stats()
        return NF.chan_affine(N.OP_FLOWBN, x, log_det_jacob, mean, var, self.log_gamma, self.beta)

    def backward(self, x, log_det_jacob):
        mean, var = self._stats()
        return NF.chan_affine(N.OP_FLOWBN, x, log_det_jacob, mean, var, self.log_gamma, self.beta, inverse=True)


class InvertibleConv1x1(nn.Module):
    """Glow's PLU-parameterised 1x1 convolution, flows/modules.py:441-497.  Frozen constants are
    ``nn.Parameter(requires_grad=False)`` like the reference, so they appear in the state_dict (appendix D Q3)."""

    def __init__(self, in_out_channels):
        super().__init__()
        C = in_out_channels
        W = torch.zeros((C, C), dtype=torch.float32)
        nn.init.orthogonal_(W)
        LU, pivots = torch.linalg.lu_factor(W)
        P, L, U = torch.lu_unpack(LU, pivots)
        self.P = nn.Parameter(P, requires_grad=False)
        self.L = nn.Parameter(L, requires_grad=True)
        self.U = nn.Parameter(U, requires_grad=True)
        self.I = nn.Parameter(torch.eye(C), requires_grad=False)
        self.pivots = nn.Parameter(pivots, requires_grad=False)
        L_mask = np.tril(np.ones((C, C), dtype='float32'), k=-1)
        self.L_mask = nn.Parameter(torch.from_numpy(L_mask), requires_grad=False)
        self.U_mask = nn.Parameter(torch.from_numpy(L_mask.T.copy()), requires_grad=False)
        s = torch.diag(U)
        self.log_s = nn.Parameter(torch.log(torch.abs(s)), requires_grad=True)
        self.sign_s = nn.Parameter(torch.sign(s), requires_grad=False)
        self._perm_cache = None

    def weight(self):
        """W = P (L o L_mask + I) (U o U_mask + diag(sign_s exp(log_s)))   (modules.py:471-473)"""
        Lp = self.L * self.L_mask + self.I
        Up = self.U * self.U_mask + torch.diag(self.sign_s * torch.exp(self.log_s))
        return self.P @ Lp @ Up

    def _pivot_matrix(self):
        """row-swap matrix of the stored LAPACK pivots (what torch.lu_solve applies to its right-hand side)."""
        key = (self.pivots._version, self.pivots.device)
        if self._perm_cache is None or self._perm_cache[0] != key:
            piv = self.pivots.detach().cpu().numpy().astype(np.int64) - 1
            perm = np.arange(piv.size)
            for i, p in enumerate(piv):
                perm[[i, p]] = perm[[p, i]]
            M = torch.zeros(piv.size, piv.size)
            M[torch.arange(piv.size), torch.from_numpy(perm)] = 1.0
            self._perm_cache = (key, M.to(self.pivots.device))
        return self._perm_cache[1]

    def inverse_weight(self):
        """W^-1 = U'^-1 L'^-1 Pp from the same LU factors / pivots the reference feeds torch.lu_solve
        (modules.py:485-492)."""
        Lp = self.L * self.L_mask + self.I
        Up = self.U * self.U_mask + torch.diag(self.sign_s * torch.exp(self.log_s))
        X = torch.linalg.solve_triangular(Lp, self._pivot_matrix(), upper=False, unitriangular=True)
        return torch.linalg.solve_triangular(Up, X, upper=True)

    _W_eff = None      # (W, holder, index): set for the duration of ONE model forward by fused.plu_weights_all

    def forward(self, z, log_df_dz):
        if self._W_eff is not None and z.is_cuda:
            W, holder, idx = self._W_eff
            return NF.invconv_apply_w(z, log_df_dz, W, self.log_s, holder, idx)
        if z.shape[1] <= NF.PLU_MAX_C:
            return NF.invconv_plu(z, log_df_dz, self.P, self.L, self.U, self.L_mask, self.U_mask, self.sign_s,
                                  self.log_s)
        return NF.invconv(z, self.weight(), log_df_dz, self.log_s)

    _W_inv = None      # set for the duration of ONE model inverse pass by models._inverse_weights_all (all layers of a width at once)

    def backward(self, y, log_df_dz):
        with torch.no_grad():
            W_inv = self._W_inv if (self._W_inv is not None and y.is_cuda) else self.inverse_weight()
            return NF.invconv_inverse(y, W_inv, log_df_dz, self.log_s)


# ---- squeeze family (flows/squeeze.py:114-189) ---------------------------------------------------------------------

def _swap_halves(z):
    h = z.shape[1] // 2
    return torch.cat([z[:, h:], z[:, :h]], dim=1)


class Squeeze2d(nn.Module):
    """flows/squeeze.py:153-170: space-to-depth, channel order k = 4 c + 2 dy + dx; ``odd`` swaps the two channel halves of the result
    (squeeze.py:94-95; no reference model builds it: one extra copy here)."""

    def __init__(self, odd=False):
        super().__init__()
        self.odd = bool(odd)

    def forward(self, z, log_df_dz):
        out = NF.squeeze2d(z)
        return (_swap_halves(out) if self.odd else out), log_df_dz

    def backward(self, z, log_df_dz):
        return NF.unsqueeze2d(_swap_halves(z) if self.odd else z), log_df_dz


class Unsqueeze2d(nn.Module):
    """flows/squeeze.py:173-189: the inverse map of Squeeze2d as a forward layer."""

    def __init__(self, odd=False):
        super().__init__()
        self.odd = bool(odd)

    def forward(self, z, log_df_dz):
        return NF.unsqueeze2d(_swap_halves(z) if self.odd else z), log_df_dz

    def backward(self, z, log_df_dz):
        out = NF.squeeze2d(z)
        return (_swap_halves(out) if self.odd else out), log_df_dz


# ---- coupling layers (flows/coupling.py) -----------------------------------------------------------------------------

class AbstractCoupling(nn.Module):
    def __init__(self, dims, masking='checkerboard', odd=False):
        super().__init__()
        self.dims = dims
        self.odd = bool(odd)
        if len(dims) == 1:
            if dims[0] % 2 != 0:
                raise Exception('coupling layers need an even feature count, got %s (flows/squeeze.py:67)' % str(dims))
            self.mode = N.SPLIT_1D
        elif len(dims) == 3 and masking == 'checkerboard':
            self.mode = N.SPLIT_CHECKER
        elif len(dims) == 3 and masking == 'channelwise':
            self.mode = N.SPLIT_CHANNEL
        else:
            raise Exception('unsupported combination of masking and dimension: %s, %s' % (masking, str(dims)))

    def squeeze(self, z):
        return NF.half_gather(z, 0, self.mode, self.odd), NF.half_gather(z, 1, self.mode, self.odd)

    def conditioner_input(self, z):
        return NF.half_gather(z, 1, self.mode, self.odd)


class AdditiveCoupling(AbstractCoupling):
    """NICE additive coupling, flows/coupling.py:52-79 (no reference model builds it): z0 <- z0 + net_t(z1), log-det unchanged.
    Runs on the affine coupling kernels with the scale pinned to zero (s = 0 * tanh(0) + 0): split + shift + merge in one launch.
    The conditioner's widths are the reference's -- including its checkerboard width (dims[0] instead of 2 * dims[0]), which cannot run
    on image data there either."""

    def __init__(self, dims, masking='checkerboard', odd=False):
        super().__init__(dims, masking, odd)
        if len(dims) == 1:
            in_chs = dims[0] // 2 if not odd else (dims[0] + 1) // 2
            self.net_t = MLP(in_chs, dims[0] - in_chs)
        else:
            in_out_chs = dims[0] if masking == 'checkerboard' else dims[0] // 2
            self.net_t = ConvNet(in_out_chs, in_out_chs)
        self.register_buffer('_zero', torch.zeros(1), persistent=False)

    def _params(self, z):
        t = self.net_t(self.conditioner_input(z))
        return torch.cat([t, torch.zeros_like(t)], dim=1)         # [shift | raw scale = 0]

    def forward(self, z, log_df_dz):
        return NF.affine_coupling(z, self._params(z), self._zero, self._zero, log_df_dz, self.mode, self.odd)

    def backward(self, y, log_df_dz):
        return NF.affine_coupling(y, self._params(y), self._zero, self._zero, log_df_dz, self.mode, self.odd, inverse=True)


class AffineCoupling(AbstractCoupling):
    """RealNVP / Glow affine coupling, flows/coupling.py:82-122; split + transform + merge + log-det are ONE kernel."""

    def __init__(self, dims, masking='checkerboard', odd=False):
        super().__init__(dims, masking, odd)
        self.s_log_scale = nn.Parameter(torch.randn(1) * 0.01)
        self.s_bias = nn.Parameter(torch.randn(1) * 0.01)
        if len(dims) == 1:
            in_chs = dims[0] // 2 if not odd else (dims[0] + 1) // 2
            self.out_chs = dims[0] - in_chs
            self.net = MLP(in_chs, self.out_chs * 2)
        else:
            in_out_chs = dims[0] * 2 if masking == 'checkerboard' else dims[0] // 2
            self.out_chs = in_out_chs
            self.net = ConvNet(in_out_chs, in_out_chs * 2)

    def couple(self, z, x, log_df_dz, inverse=False):
        """the coupling given the conditioner's input ``x`` (the untouched half of z; None = gather it here).  Image models whose
        conditioner runs as the persistent chain kernel take conditioner + transform + merge + log-det in ONE launch per direction;
        the gradient of x is then part of the gradient of z (the gather here is done outside the graph)."""
        if z.dim() == 4 and z.is_cuda and isinstance(self.net, ConvNet):
            from . import fused_conv as FC
            z = z.contiguous()
            if FC.coupling_fusable(self.net, z, self.mode):
                if x is None:
                    x = self.conditioner_input(z.detach())
                return FC.convnet_coupling(self.net, x, z, NF._owned_ld(log_df_dz), self.s_log_scale, self.s_bias, self.mode,
                                           self.odd, inverse=inverse)
        if x is None:
            x = self.conditioner_input(z)
        return NF.affine_coupling(z, self.net(x), self.s_log_scale, self.s_bias, log_df_dz, self.mode, self.odd, inverse=inverse)

    def forward(self, z, log_df_dz):
        return self.couple(z, None, log_df_dz)

    def backward(self, y, log_df_dz):
        return self.couple(y, None, log_df_dz, inverse=True)


class MixLogAttnCoupling(AbstractCoupling):
    """Flow++ mixture-of-logistics coupling with the gated-attention conditioner, flows/coupling.py:125-210.
    CDF -> logit -> affine and all three log-det terms are ONE kernel; the inverse bisection is two launches."""

    def __init__(self, dims, masking='checkerboard', odd=False, base_filters=32, n_mixtures=4):
        super().__init__(dims, masking, odd)
        self.n_mixtures = n_mixtures
        self.a_log_scale = nn.Parameter(torch.randn(1) * 0.01)
        self.a_bias = nn.Parameter(torch.randn(1) * 0.01)
        if len(dims) == 1:
            in_chs = dims[0] // 2 if not odd else (dims[0] + 1) // 2
            out_chs = dims[0] - in_chs
            mid_shape = (base_filters, ) + tuple(d // 2 for d in dims[1:])
        elif masking == 'checkerboard':
            in_chs = out_chs = dims[0] * 2
            mid_shape = (base_filters, ) + tuple(d // 2 for d in dims[1:])
        else:
            in_chs = out_chs = dims[0] // 2
            mid_shape = (base_filters, ) + tuple(dims[1:])
        self.sections = [out_chs] * 2 + [out_chs * n_mixtures] * 3
        self.net = flowpp_conditioner(in_chs, sum(self.sections), mid_shape, base_filters, conv=(len(dims) == 3))
        self.logit_eps = 1.0e-5                      # Logit() default inside the coupling (coupling.py:169)

    def conditioner(self, z):
        """coupling parameters from the untouched half; density data runs the whole gated-attention stack as one
        launch per direction (csrc/flowpp_cond.hip), image data on the per-sample kernels of csrc/flowpp_img.hip (4 launches
        forward, 9 backward); the module stack remains for shapes neither takes and off the GPU."""
        return self.conditioner_of(self.conditioner_input(z))

    def couple(self, z, x, log_df_dz):
        """the coupling given the conditioner's input ``x`` (the untouched half of z, gathered by the fused head of the step)"""
        return NF.mixlog_coupling(z, self.conditioner_of(x), self.a_log_scale, self.a_bias, log_df_dz, self.n_mixtures, self.mode,
                                  self.odd, logit_eps=self.logit_eps)

    def conditioner_of(self, x):
        if FUSED.flowpp_cond_fusable(self.net, x):
            return FUSED.flowpp_cond_forward(self.net, x)
        if FPI.flowpp_img_fusable(self.net, x):
            return FPI.flowpp_img_forward(self.net, x)
        return self.net(x)

    def forward(self, z, log_df_dz):
        if (self.mode == N.SPLIT_1D and z.is_cuda and z.dim() == 2 and z.dtype == torch.float32 and z.shape[0] > 0
                and FUSED.flowpp_cond_fusable(self.net, z[:, :z.shape[1] // 2])):
            return FUSED.flowpp_coupling_vec(z, log_df_dz, self)          # conditioner + coupling, no gather / scatter
        params = self.conditioner(z)
        return NF.mixlog_coupling(z, params, self.a_log_scale, self.a_bias, log_df_dz, self.n_mixtures, self.mode,
                                  self.odd, logit_eps=self.logit_eps)

    def backward(self, z, log_df_dz):
        params = self.conditioner(z)
        return NF.mixlog_coupling(z, params, self.a_log_scale, self.a_bias, log_df_dz, self.n_mixtures, self.mode,
                                  self.odd, inverse=True)


class RQSplineCoupling(AbstractCoupling):
    """monotone rational-quadratic spline coupling of Neural Spline Flows (Durkan et al. 2019; no reference counterpart): the transformed
    half goes through a ``bins``-piece spline on (-tail_bound, tail_bound) with linear tails, its 3 bins - 1 parameters per element come
    from the conditioner of the affine coupling at that width.  Split + spline + merge + log-det are ONE kernel per direction, and the
    inverse is closed-form.  The layer has no parameters of its own."""

    def __init__(self, dims, masking='checkerboard', odd=False, bins=8, tail_bound=3.0):
        super().__init__(dims, masking, odd)
        if bins not in NF.RQS_BINS:
            raise ValueError('RQSplineCoupling: bins must be one of %s, got %r' % (NF.RQS_BINS, bins))
        if not float(tail_bound) > 0.0:
            raise ValueError('RQSplineCoupling: tail_bound must be positive, got %r' % tail_bound)
        self.bins, self.tail_bound = int(bins), float(tail_bound)
        if len(dims) == 1:
            in_chs = dims[0] // 2 if not odd else (dims[0] + 1) // 2
            self.out_chs = dims[0] - in_chs
            self.net = MLP(in_chs, self.out_chs * (3 * self.bins - 1))
        else:
            in_out_chs = dims[0] * 2 if masking == 'checkerboard' else dims[0] // 2
            self.out_chs = in_out_chs
            self.net = ConvNet(in_out_chs, in_out_chs * (3 * self.bins - 1))

    def _couple(self, z, log_df_dz, inverse):
        params = self.net(self.conditioner_input(z))
        return NF.rqs_coupling(z, params, log_df_dz, self.bins, self.tail_bound, self.mode, self.odd, inverse=inverse)

    def forward(self, z, log_df_dz):
        return self._couple(z, log_df_dz, False)

    def backward(self, y, log_df_dz):
        return self._couple(y, log_df_dz, True)


# ---- MAF (flows/maf.py) -------------------------------------------------------------------------------------------------

class MADE(nn.Module):
    """masked autoencoder conditioner, flows/maf.py:9-85.  Same parameter containers (weights / bnorms / biases).
    Masks follow the reference's rule, including its re-draw from the global ``np.random`` on every call
    (degenerate, i.e. constant, for D == 2 -- appendix D Q4).  ``draws = 'device'`` (set through ``MAF.draws``) takes every draw from
    csrc/made_masks.hip instead: same rule, Philox in place of np.random, nothing from the host."""

    draws = 'host'                  # (MAF.draws: where the masks are drawn)
    _seed = None                    # (MAF.seed: device int64[2], the seed words of draws = 'device')

    def __init__(self, in_out_features, num_hidden=2, base_filters=32, use_companion=False):
        super().__init__()
        if use_companion:
            raise NotImplementedError('use_companion=True is never built by the reference models')
        self.in_out_chs = in_out_features
        self.num_hidden = num_hidden
        self.base_filters = base_filters
        self.masks = None
        # the draw changes from call to call for D > 2 (constant for D == 2): a captured graph would freeze a host draw -- FlowTrainer
        # then switches a MAF on the GPU to device draws and keeps any other such model on eager launches (train.py)
        self.masks_redrawn_per_call = in_out_features > 2
        weights, biases, bnorms = [], [], []
        widths = [in_out_features] + [base_filters] * num_hidden
        for i, o in zip(widths[:-1], widths[1:]):
            scale = np.sqrt(2.0 / (o + i))
            weights.append(nn.Parameter(torch.randn(o, i) * scale))
            torch.randn(o, i)                        # the reference also draws the unused companion matrix U
            biases.append(nn.Parameter(torch.randn(o) * 0.01))
            bnorms.append(nn.BatchNorm1d(o))
        scale = np.sqrt(2.0 / (in_out_features + widths[-1]))
        weights.append(nn.Parameter(torch.randn(in_out_features, widths[-1]) * scale))
        torch.randn(in_out_features, widths[-1])
        biases.append(nn.Parameter(torch.randn(in_out_features) * 0.01))
        self.weights = nn.ParameterList(weights)
        self.bnorms = nn.ModuleList(bnorms)
        self.biases = nn.ParameterList(biases)

    def draw_masks(self, device):
        """draws the masks like the reference does on every call; the device copies are re-used while the draw is
        unchanged (always, for D == 2), so the steady state has no host-to-device traffic.  draws = 'device': one launch, one draw,
        into a tensor of its own."""
        if self.draws == 'device':
            self.masks = NF.made_draw_masks(made_seed_words(self, device), 1, self.in_out_chs, advance=True)[0]
            return self.masks
        m = made_degrees_to_masks(self.in_out_chs, self.num_hidden, self.base_filters, np.random)
        c = getattr(self, '_mask_cache', None)
        if c is None or c[0] != device or not all(np.array_equal(a, b) for a, b in zip(c[1], m)):
            self._mask_cache = (device, m, [torch.from_numpy(a).to(device) for a in m])
        self.masks = self._mask_cache[2]
        return self.masks

    def forward(self, z):
        masks = self.draw_masks(z.device)
        h = z
        from . import dist as nfdist
        sync = nfdist.sync_stats_active()
        for i in range(self.num_hidden):
            pre = F.linear(h, self.weights[i] * masks[i], self.biases[i])
            h = torch.relu(nfdist.sync_batch_norm(self.bnorms[i], pre) if (sync and self.bnorms[i].training) else self.bnorms[i](pre))
        return F.linear(h, self.weights[-1] * masks[-1], self.biases[-1])


def made_seed_words(net, device):
    """the seed words a MADE in draws = 'device' mode draws from"""
    if net.num_hidden != 3 or net.base_filters != 32:
        raise RuntimeError("draws='device' serves MADEs of three hidden layers of 32 units (csrc/made_masks.hip)")
    if net._seed is None or net._seed.device != device or not net._seed.is_cuda:
        raise RuntimeError("draws='device' needs the model's seed words on the input's GPU (set it through MAF.draws and call the MAF "
                           "model; got seed on %s, input on %s)" % (None if net._seed is None else net._seed.device, device))
    return net._seed


class AutoregressiveTransfrom(nn.Module):
    """masked autoregressive affine transform (the reference's spelling), flows/maf.py:88-119."""

    def __init__(self, in_out_features, num_hidden=3, base_filters=32):
        super().__init__()
        self.in_out_chs = in_out_features
        self.register_buffer('perm', torch.eye(in_out_features)[:, torch.randperm(in_out_features)])
        self.net_s = MADE(in_out_features, num_hidden, base_filters)
        self.net_t = MADE(in_out_features, num_hidden, base_filters)
        self.s_log_scale = nn.Parameter(torch.randn(1) * 0.01)
        self.s_bias = nn.Parameter(torch.randn(1) * 0.01)

    def draw_pair(self, device):
        """(masks of net s, masks of net t) of one call, in the reference's RNG order: s-net, then t-net; draws = 'device': both from
        one launch"""
        if self.net_s.draws == 'device' and self.net_t.draws == 'device' and self.net_s._seed is self.net_t._seed:
            self.net_s.masks, self.net_t.masks = NF.made_draw_masks(made_seed_words(self.net_s, device), 2, self.in_out_chs, advance=True)
        else:
            self.net_s.draw_masks(device)
            self.net_t.draw_masks(device)
        return self.net_s.masks, self.net_t.masks

    def conditioners(self, z):
        """(s_raw, t) = (net_s(z), net_t(z)); on the GPU both MADEs run in the same fp32-MFMA launches."""
        from . import dist as nfdist
        if (z.is_cuda and self.in_out_chs <= 32 and self.net_s.base_filters == 32 and z.dtype == torch.float32
                and not nfdist.sync_stats_active()):
            from .fused import made_pair_forward
            ms, mt = self.draw_pair(z.device)
            return made_pair_forward(self.net_s, self.net_t, z, ms, mt)
        return self.net_s(z), self.net_t(z)

    def forward(self, z, log_df_dz):
        z = torch.mm(z, self.perm)
        s_raw, t = self.conditioners(z)
        return NF.affine_transform(z, s_raw, t, self.s_log_scale, self.s_bias, log_df_dz)

    def backward(self, z, log_df_dz):
        """D sequential passes; unlike the reference (maf.py:114) the caller's tensor is NOT mutated (appendix D Q5)."""
        z = z.clone()
        for i in range(self.in_out_chs):
            s_raw, t = self.conditioners(z)
            ld_i = log_df_dz.clone()
            cand, ld_all = NF.affine_transform(z, s_raw, t, self.s_log_scale, self.s_bias, ld_i, inverse=True)
            # only column i is taken from this pass (maf.py:114-115)
            s = torch.tanh(s_raw[:, i]) * self.s_log_scale + self.s_bias
            z[:, i] = cand[:, i]
            log_df_dz = log_df_dz - s
        return torch.mm(z, self.perm.t()), log_df_dz


# ---- masked-autoregressive spline (RQ-NSF (AR), Durkan et al. 2019; no reference counterpart) ----------------------------------------

class AutoregressiveSpline(nn.Module):
    """masked autoregressive rational-quadratic spline transform: feature i of the permuted input goes through a ``bins``-piece monotone
    spline on (-tail_bound, tail_bound) with linear tails whose 3 bins - 1 parameters are a MADE-style function of the features before it.
    The conditioner is ``num_hidden`` masked linear layers with ReLU (no BatchNorm: the conditioner is a per-row function, so the
    column-by-column inverse sees the same function in every pass) and a masked output layer that is fused with the spline into one
    kernel per direction (functional.ars_head): the (B, (3 bins - 1) D) parameter tensor never exists.

    The masks are FIXED at construction (hidden degrees ``arange(base_filters) % max(1, D - 1)``, registered as buffers): no draw per
    call, so a captured training step replays the same function.  The head starts at zero: the layer starts as the identity.
    Not a subclass of AutoregressiveTransfrom: Compose serves it through the layer's own calls."""

    masks_redrawn_per_call = False

    def __init__(self, in_out_features, bins=8, tail_bound=3.0, num_hidden=3, base_filters=32):
        super().__init__()
        D = int(in_out_features)
        if bins not in NF.RQS_BINS:
            raise ValueError('AutoregressiveSpline: bins must be one of %s, got %r' % (NF.RQS_BINS, bins))
        if not float(tail_bound) > 0.0:
            raise ValueError('AutoregressiveSpline: tail_bound must be positive, got %r' % tail_bound)
        if not 1 <= D <= NF.ARS_MAX_D:
            raise ValueError('AutoregressiveSpline: the fused head serves 1 <= in_out_features <= %d, got %r' % (NF.ARS_MAX_D, in_out_features))
        if base_filters != NF.ARS_HIDDEN or num_hidden < 1:
            raise ValueError('AutoregressiveSpline: the fused head is built for base_filters = %d and at least one hidden layer, got '
                             'base_filters = %r, num_hidden = %r' % (NF.ARS_HIDDEN, base_filters, num_hidden))
        self.in_out_chs, self.bins, self.tail_bound = D, int(bins), float(tail_bound)
        self.num_hidden, self.base_filters = int(num_hidden), int(base_filters)
        self.register_buffer('perm', torch.eye(D)[:, torch.randperm(D)])
        masks = made_masks_from_degrees(D, self.degrees())
        for i, m in enumerate(masks[:-1]):
            self.register_buffer('mask%d' % i, torch.from_numpy(m))
        self.register_buffer('head_mask', torch.from_numpy(masks[-1]))       # (D, base_filters): row d serves the 3 bins - 1 rows of feature d
        weights, biases = [], []
        widths = [D] + [base_filters] * num_hidden
        for i, o in zip(widths[:-1], widths[1:]):                            # MADE's initialisation (flows/maf.py:28-33)
            weights.append(nn.Parameter(torch.randn(o, i) * np.sqrt(2.0 / (o + i))))
            biases.append(nn.Parameter(torch.randn(o) * 0.01))
        self.weights = nn.ParameterList(weights)
        self.biases = nn.ParameterList(biases)
        self.head_weight = nn.Parameter(torch.zeros((3 * self.bins - 1) * D, base_filters))     # row p D + d: parameter p of feature d
        self.head_bias = nn.Parameter(torch.zeros((3 * self.bins - 1) * D))

    def degrees(self):
        """the hidden units' degrees, one vector per hidden layer"""
        return [np.arange(self.base_filters) % max(1, self.in_out_chs - 1)] * self.num_hidden

    @property
    def masks(self):
        """[hidden masks ..., head mask (D, base_filters)]: made_masks_from_degrees(D, self.degrees())"""
        return [getattr(self, 'mask%d' % i) for i in range(self.num_hidden)] + [self.head_mask]

    def trunk(self, z):
        """the activated last hidden layer (B, base_filters) of the permuted input; framework ops"""
        h = z
        for i in range(self.num_hidden):
            h = torch.relu(F.linear(h, self.weights[i] * getattr(self, 'mask%d' % i), self.biases[i]))
        return h

    def forward(self, z, log_df_dz):
        z = torch.mm(z, self.perm)
        return NF.ars_head(self.trunk(z), self.head_weight, self.head_bias, self.head_mask, z, log_df_dz, self.bins, self.tail_bound)

    def backward(self, z, log_df_dz):
        """D sequential passes of trunk + head, pass i inverting column i in place in ONE clone (column i depends on the recovered
        columns before it alone); the caller's tensor is not mutated.  No graph is built."""
        with torch.no_grad():
            x = z.clone()
            for i in range(self.in_out_chs):
                _, log_df_dz = NF.ars_head(self.trunk(x), self.head_weight, self.head_bias, self.head_mask, x, log_df_dz, self.bins,
                                           self.tail_bound, inverse=True, col=i, out=x)
            return torch.mm(x, self.perm.t()), log_df_dz
