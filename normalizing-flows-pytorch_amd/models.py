"""
Layer stacks with the reference's constructor and call surface:

    net = Glow(dims, datatype, cfg)      cfg.layers (all), cfg.mixtures (Flowpp)
    z, log_df_dz = net(y)                forward flow, log_df_dz of shape (B,)
    y, log_df_dz = net.backward(z)       inverse flow (sampling)

Reference: flows/realnvp.py:9-63, flows/glow.py:10-68, flows/flowpp.py:9-78, flows/maf.py:122-148.
The multi-scale image recipe (shared by RealNVP / Glow / Flow++) is written once here.
"""
import numpy as np
import torch
import torch.nn as nn

from .layers import (CNF, ActNorm, AffineCoupling, AutoregressiveSpline, AutoregressiveTransfrom, BatchNorm, Compose, InvertibleConv1x1, Logit,
                     MixLogAttnCoupling, PlanarTransform, RQSplineCoupling, Squeeze2d, Unsqueeze2d)


class _FlowModel(nn.Module):
    def __init__(self, dims, datatype=None, cfg=None):
        super().__init__()
        self.dims = tuple(dims)
        self.n_layers = cfg.layers
        self.net = Compose(self._build(self.dims, datatype, cfg))

    # one "flow step" = normalisation (+ 1x1 conv) + coupling; supplied by the subclass
    def _step(self, dims, masking, odd, cfg):
        raise NotImplementedError

    def _build(self, dims, datatype, cfg):
        K = self.n_layers
        layers = []
        if datatype == 'image':
            layers.append(Logit(eps=0.01))
            mid = dims
            while max(mid[1], mid[2]) > 8:
                for i in range(K):
                    layers += self._step(mid, 'checkerboard', i % 2 != 0, cfg)
                layers.append(Squeeze2d(odd=False))
                mid = (mid[0] * 4, mid[1] // 2, mid[2] // 2)
                for i in range(K):
                    layers += self._step(mid, 'channelwise', i % 2 != 0, cfg)
            for i in range(K + 1):
                layers += self._step(mid, 'checkerboard', i % 2 != 0, cfg)
            while mid[1] != dims[1] or mid[2] != dims[2]:
                layers.append(Unsqueeze2d(odd=False))
                mid = (mid[0] // 4, mid[1] * 2, mid[2] * 2)
        else:
            for i in range(K):
                layers += self._step(dims, 'checkerboard', i % 2 != 0, cfg)
        return layers

    def _zero_ld(self, z):
        if z.dtype == torch.float32:
            from .workspace import zeros_owned
            return zeros_owned((z.size(0), ), z.device)      # (inside a trainer step: part of the step's one memset, no fill launch)
        return torch.zeros(z.size(0), dtype=z.dtype, device=z.device)

    def _wn_convs(self):
        """the weight-normed convolutions of the image conditioners (their weight-norm arithmetic is batched per pass)."""
        c = getattr(self, '_wn_cache', None)
        if c is None:
            from .conditioners import WeightNorm
            c = self._wn_cache = [m for m in self.modules() if isinstance(m, WeightNorm) and m._conv]
        return c

    def _plu_convs(self):
        """the invertible 1x1 convolutions that run as modules in the forward direction (more than NF.HEAD_MAX_C channels: the
        smaller ones are inside the fused Glow head): their PLU weights are computed in batched launches per pass."""
        c = getattr(self, '_plu_cache', None)
        if c is None:
            from .layers import InvertibleConv1x1
            from . import functional as NF
            c = self._plu_cache = [m for m in self.modules() if isinstance(m, InvertibleConv1x1)
                                   and NF.HEAD_MAX_C < m.L.shape[0] <= NF.PLU_MAX_C]
        return c

    def _inverse_weights_all(self):
        """W^-1 = U'^-1 L'^-1 Pp of every invertible 1x1 convolution of an image model (modules.py:485-492), the layers of one
        width solved as ONE batch: two triangular solves per width instead of two per layer (~10 small launches each, 129
        layers in the CIFAR Glow).  Stashed on the modules for the inverse pass under way."""
        from .layers import InvertibleConv1x1
        convs = getattr(self, '_inv_cache', None)
        if convs is None:
            convs = self._inv_cache = [m for m in self.modules() if isinstance(m, InvertibleConv1x1)]
        groups = {}
        for m in convs:
            groups.setdefault(m.L.shape[0], []).append(m)
        with torch.no_grad():
            for C, ms in groups.items():
                L = torch.stack([m.L for m in ms]) * torch.stack([m.L_mask for m in ms])
                U = torch.stack([m.U for m in ms]) * torch.stack([m.U_mask for m in ms])
                d = torch.stack([m.sign_s * torch.exp(m.log_s) for m in ms])
                Lp = L + torch.eye(C, dtype=L.dtype, device=L.device)
                Up = U + torch.diag_embed(d)
                Pp = torch.stack([m._pivot_matrix() for m in ms])
                X = torch.linalg.solve_triangular(Lp, Pp, upper=False, unitriangular=True)
                Winv = torch.linalg.solve_triangular(Up, X, upper=True)
                for i, m in enumerate(ms):
                    m._W_inv = Winv[i]
        return convs

    def _with_weight_norms(self, fn, z):
        wns = self._wn_convs() if z.is_cuda else []
        plus = self._plu_convs() if (z.is_cuda and z.dim() == 4 and fn == self.net) else []
        invs = self._inverse_weights_all() if (z.is_cuda and z.dim() == 4 and fn != self.net) else []
        if not wns and not plus and not invs:
            return fn(z, self._zero_ld(z))
        from . import fused as FUSED
        FUSED.weight_norm_all(wns)
        FUSED.plu_weights_all(plus)
        try:
            return fn(z, self._zero_ld(z))
        finally:
            for m in wns:
                m._w_eff = None
            for m in plus:
                m._W_eff = None
            for m in invs:
                m._W_inv = None

    def forward_slice(self, z, log_df_dz, a, b):
        """layers[a:b] of the stack in the forward direction on (z, log_df_dz) -- the same Compose peepholes, weight-norm and PLU
        pre-passes as a whole forward, restricted to those layers (they share this model's parameters).  Lets a test feed a
        slice of a full-size model with the oracle's activations at that depth (tests/test_gpu_slices.py)."""
        sub = Compose(list(self.net.layers[a:b]))
        if not z.is_cuda:
            return sub(z, log_df_dz)
        from . import functional as NF
        from . import fused as FUSED
        from .conditioners import WeightNorm
        from .layers import InvertibleConv1x1
        wns = [m for m in sub.modules() if isinstance(m, WeightNorm) and m._conv]
        plus = [m for m in sub.modules() if isinstance(m, InvertibleConv1x1)
                and NF.HEAD_MAX_C < m.L.shape[0] <= NF.PLU_MAX_C] if z.dim() == 4 else []
        FUSED.weight_norm_all(wns)
        FUSED.plu_weights_all(plus)
        try:
            return sub(z, log_df_dz)
        finally:
            for m in wns:
                m._w_eff = None
            for m in plus:
                m._W_eff = None

    def forward(self, z):
        if z.is_cuda and z.device.index != torch.cuda.current_device():
            with torch.cuda.device(z.device):      # (a model on another GPU than the current one: launch on ITS device, as torch's own ops do)
                return self._with_weight_norms(self.net, z)
        return self._with_weight_norms(self.net, z)

    def backward(self, z):
        if z.is_cuda and z.device.index != torch.cuda.current_device():
            with torch.cuda.device(z.device):
                return self._with_weight_norms(self.net.backward, z)
        return self._with_weight_norms(self.net.backward, z)


class RealNVP(_FlowModel):
    def _step(self, dims, masking, odd, cfg):
        return [BatchNorm(dims, affine=False), AffineCoupling(dims, masking=masking, odd=odd)]


class Glow(_FlowModel):
    def _step(self, dims, masking, odd, cfg):
        return [ActNorm(dims), InvertibleConv1x1(dims[0]), AffineCoupling(dims, masking=masking, odd=odd)]


class Flowpp(_FlowModel):
    """flows/flowpp.py:9-78: image steps are ActNorm + inv-1x1 + mixture coupling, density steps have no inv-1x1."""

    def _step(self, dims, masking, odd, cfg):
        layers = [ActNorm(dims)]
        if len(dims) == 3:
            layers.append(InvertibleConv1x1(dims[0]))
        layers.append(MixLogAttnCoupling(dims, masking=masking, odd=odd, n_mixtures=cfg.mixtures))
        return layers


class SplineFlow(_FlowModel):
    """Neural spline flow (Durkan et al. 2019; no reference counterpart): Glow's step with the affine coupling replaced by the
    rational-quadratic spline coupling.  cfg.bins (default 8) and cfg.tail_bound (default 3.0) are optional.  Vector data is the supported
    workload; the image layout is the shared multi-scale recipe."""

    def _step(self, dims, masking, odd, cfg):
        return [ActNorm(dims), InvertibleConv1x1(dims[0]),
                RQSplineCoupling(dims, masking=masking, odd=odd, bins=getattr(cfg, 'bins', 8), tail_bound=getattr(cfg, 'tail_bound', 3.0))]


class MAF(_FlowModel):
    """flows/maf.py:122-148: [flow BatchNorm, autoregressive transform] x layers; density data only."""

    def _build(self, dims, datatype, cfg):
        if datatype == 'image':
            raise NotImplementedError('Sorry, MAF for image generation is not supported!')   # reference forgets to raise
        layers = []
        for _ in range(self.n_layers):
            layers.append(BatchNorm(dims, affine=False))
            layers.append(AutoregressiveTransfrom(dims[0]))
        return layers

    def __init__(self, dims, datatype=None, cfg=None):
        super().__init__(dims, datatype, cfg)
        # seed words of the device-side mask draws (draws = 'device'): seed, stream offset; not in the state_dict
        self.register_buffer('seed', torch.tensor([torch.initial_seed() & 0x7fffffffffffffff, 0], dtype=torch.int64), persistent=False)

    def _mades(self):
        return [n for m in self.net.layers if isinstance(m, AutoregressiveTransfrom) for n in (m.net_s, m.net_t)]

    @property
    def draws(self):
        """'host' (default): the MADE masks are redrawn from np.random on every call, in the reference's order (maf.py:50,66-85);
        'device': drawn by csrc/made_masks.hip from ``seed`` with the same rule (what a captured training step needs for D > 2: a
        replay draws afresh; and what lets the inverse of a step with D > 2 run as one launch).  D <= 4."""
        return self._mades()[0].draws if self.n_layers > 0 else 'host'

    @draws.setter
    def draws(self, value):
        if value not in ('host', 'device'):
            raise ValueError("draws is 'host' or 'device', got %r" % (value, ))
        if value == 'device' and self.dims[0] > 4:
            raise ValueError("draws = 'device' serves D <= 4 (csrc/made_masks.hip), got D = %d" % self.dims[0])
        for n in self._mades():
            n.draws = value
        self._bind_seed()

    def _bind_seed(self):
        for n in self._mades():                              # (every pass: .to() replaces the buffer)
            n._seed = self.seed

    def forward(self, z):
        self._bind_seed()
        return super().forward(z)

    def backward(self, z):
        self._bind_seed()
        return super().backward(z)


class SplineMAF(_FlowModel):
    """masked-autoregressive neural spline flow (RQ-NSF (AR) of Durkan et al. 2019; no reference counterpart): MAF's stack with the
    affine transform replaced by AutoregressiveSpline -- [flow BatchNorm, autoregressive spline] x layers; density data only, up to eight
    features.  cfg.bins (default 8) and cfg.tail_bound (default 3.0) are optional.  The masks are fixed, so FlowTrainer(graph=True)
    captures the step as it is."""

    def _build(self, dims, datatype, cfg):
        if datatype == 'image':
            raise NotImplementedError('Sorry, SplineMAF for image generation is not supported!')
        layers = []
        for _ in range(self.n_layers):
            layers.append(BatchNorm(dims, affine=False))
            layers.append(AutoregressiveSpline(dims[0], getattr(cfg, 'bins', None) or 8, getattr(cfg, 'tail_bound', None) or 3.0))
        return layers


class PlanarFlow(nn.Module):
    """flows/planar.py:71-94: ``cfg.layers`` PlanarTransforms on the flattened dimension.  The reference also builds a BatchNorm per
    layer and discards it (planar.py:82); that draws no random numbers, so it is left out here.  Only (B, D) input runs: the reference
    constructs an image PlanarFlow but its torch.mm fails on a 4-D batch, this one raises RuntimeError naming the shape."""

    def __init__(self, dims, datatype=None, cfg=None):
        super().__init__()
        self.dims = dims
        self.dim = np.prod(dims)
        self.n_layers = cfg.layers
        self.net = Compose([PlanarTransform(self.dim) for _ in range(self.n_layers)])

    _zero_ld = _FlowModel._zero_ld

    def _run(self, fn, z):
        if z.dim() != 2:
            raise RuntimeError('PlanarFlow takes (B, D) input, got shape %s' % (tuple(z.shape), ))
        if z.is_cuda and z.device.index != torch.cuda.current_device():
            with torch.cuda.device(z.device):
                return fn(z, self._zero_ld(z))
        return fn(z, self._zero_ld(z))

    def forward(self, z):
        return self._run(self.net, z)

    def backward(self, z):
        return self._run(self.net.backward, z)


class Ffjord(nn.Module):
    """flows/ffjord.py:10-42: ``cfg.layers`` x [ActNorm, CNF] on density data, the times ``linspace(t0, t1, steps)`` in float32 (stored
    by each CNF as a float64 buffer of float32 values).  ``cfg.backprop`` is not forwarded, as in the reference: the CNFs use the
    adjoint.  The reference builds an EMPTY flow for images (it constructs the NotImplementedError without raising it, ffjord.py:26);
    this one raises.  ``cfg.noise_on_cpu`` (optional, default False) is handed to the CNFs: True reproduces the reference's CPU draws.
    The model mixes float32 (ActNorm) and float64 (field) parameters: it trains with the reference's own loop (torch.optim.Adam,
    main.py:78-92), not with FlowTrainer, whose gradient bucket is single-dtype."""

    def __init__(self, dims, datatype=None, cfg=None):
        super().__init__()
        self.dims = dims
        self.n_layers = cfg.layers
        self.stepsize = cfg.stepsize
        t0, t1 = cfg.t0, cfg.t1
        steps = int(np.ceil((t1 - t0) / self.stepsize)) + 1
        times = torch.linspace(t0, t1, steps, dtype=torch.float32)
        if datatype == 'image':
            raise NotImplementedError('Sorry, FFJORD for image generation is not supported!')
        layers = []
        for _ in range(self.n_layers):
            layers.append(ActNorm(dims))
            layers.append(CNF(dims, times=times, solver_type=cfg.solver, trace_estimator=cfg.trace,
                              noise_on_cpu=getattr(cfg, 'noise_on_cpu', False)))
        self.net = Compose(layers)

    _zero_ld = _FlowModel._zero_ld

    def _run(self, fn, z):
        if z.is_cuda and z.device.index != torch.cuda.current_device():
            with torch.cuda.device(z.device):
                return fn(z, self._zero_ld(z))
        return fn(z, self._zero_ld(z))

    def forward(self, z):
        return self._run(self.net, z)

    def backward(self, z):
        return self._run(self.net.backward, z)
