"""
Training / evaluation harness: the counterpart of ``Model`` in the reference's main.py:38-124 restricted to what the
hot path needs -- ``train_on_batch`` (main.py:78-92), ``sample_y`` (:109-116), ``log_py`` (:121-124) -- plus what the
reference does not have: data parallelism (dist.GradBucket) and whole-step hipGraph capture.

The prior is N(0, I): ``MultivariateNormal(0, I).log_prob(z) = -0.5 |z|^2 - 0.5 D log(2 pi)`` (main.py:49-51); the
reference materialises a D x D covariance (3072 x 3072 for CIFAR), here it is a reduction.
"""
import math

import os

import torch

from . import dist as nfdist


def standard_normal_logprob(z):
    zf = z.reshape(z.shape[0], -1)
    return -0.5 * (zf * zf).sum(dim=1) - 0.5 * zf.shape[1] * math.log(2.0 * math.pi)


def nll_loss(z, log_det_jacobian):
    """loss = -mean(log N(z; 0, I) + log_det_jacobian)   (main.py:85); one HIP reduction on the GPU."""
    if z.is_cuda and z.dtype == torch.float32 and z.shape[0] > 0:
        from . import functional as NF
        return NF.nll_loss(z, log_det_jacobian)
    return -1.0 * torch.mean(standard_normal_logprob(z) + log_det_jacobian)


def bits_per_dim(loss, dims):
    D = 1
    for d in dims:
        D *= int(d)
    return float(loss) / (D * math.log(2.0))


def _check_ema_decay(d):
    if d is None:
        return None
    d = float(d)
    if not 0.0 <= d < 1.0:
        raise ValueError('ema_decay must lie in [0, 1), got %r' % (d, ))
    return d


class _LrRule:
    """The learning-rate rule of the trainer, stated once for the fused path (whose launch, nf_lr_schedule, restates ``rate``) and the
    torch.optim path.  With ``pos`` the optimizer steps completed under the schedule, W = lr_warmup_steps or 0 and
    t = max(pos - W, 0), the step that follows trains at ``warm(pos) * decay(t)``:
      warm   1 without a warmup, else lr_warmup_start + (1 - lr_warmup_start) min(pos, W) / W -- torch's LinearLR(start_factor, 1, W)
      decay  base | base * decay_ratio ** (t // decay_steps) (StepLR, counted from the warmup's end) |
             lr_min + (base - lr_min)(1 + cos(pi min(t, T) / T)) / 2 with T = cosine_steps.  Past t = T the rate HOLDS at lr_min;
             torch's CosineAnnealingLR swings back up there.
    ``general``: a warmup or a cosine is asked for, what the StepLR launch of ``decay_steps`` alone cannot do."""

    def __init__(self, lr, decay_steps=None, decay_ratio=0.5, lr_warmup_steps=None, lr_warmup_start=1.0 / 3.0, cosine_steps=None,
                 lr_min=0.0):
        self.decay_steps = None if decay_steps is None else int(decay_steps)
        self.decay_ratio = float(decay_ratio)
        self.warmup_steps = None if lr_warmup_steps is None else int(lr_warmup_steps)
        self.warmup_start = float(lr_warmup_start)
        self.cosine_steps = None if cosine_steps is None else int(cosine_steps)
        self.lr_min = float(lr_min)
        if self.decay_steps is not None and self.decay_steps < 1:
            raise ValueError('decay_steps must be a positive number of optimizer steps, got %r' % (decay_steps, ))
        if self.warmup_steps is not None and self.warmup_steps < 1:
            raise ValueError('lr_warmup_steps must be a positive number of optimizer steps, got %r' % (lr_warmup_steps, ))
        if self.cosine_steps is not None and self.cosine_steps < 1:
            raise ValueError('cosine_steps must be a positive number of optimizer steps, got %r' % (cosine_steps, ))
        if self.decay_steps is not None and self.cosine_steps is not None:
            raise ValueError('decay_steps (StepLR) and cosine_steps are two decays of the same rate: give one of them')
        if not 0.0 < self.warmup_start <= 1.0:
            raise ValueError('lr_warmup_start must lie in (0, 1] (torch\'s LinearLR refuses a start factor of 0), got %r' % (lr_warmup_start, ))
        if not 0.0 <= self.lr_min <= float(lr):
            raise ValueError('lr_min must lie in [0, lr = %r], got %r' % (float(lr), lr_min))
        self.general = self.warmup_steps is not None or self.cosine_steps is not None
        self.active = self.general or self.decay_steps is not None

    def rate(self, base, pos):
        base, pos, W = float(base), int(pos), self.warmup_steps or 0
        t = max(pos - W, 0)
        if self.decay_steps is not None:
            d = base * self.decay_ratio ** (t // self.decay_steps)
        elif self.cosine_steps is not None:
            T = self.cosine_steps
            d = self.lr_min if t >= T else self.lr_min + (base - self.lr_min) * (1.0 + math.cos(math.pi * t / T)) / 2.0
        else:
            d = base
        if pos >= W:
            return d
        return (self.warmup_start + (1.0 - self.warmup_start) * pos / W) * d

    def native_args(self):
        """(warmup_steps, warmup_start, kind, span, arg) of nf_lr_schedule"""
        from . import _native as N
        if self.decay_steps is not None:
            tail = (N.header_constant('NF_LR_STEP'), self.decay_steps, self.decay_ratio)
        elif self.cosine_steps is not None:
            tail = (N.header_constant('NF_LR_COSINE'), self.cosine_steps, self.lr_min)
        else:
            tail = (N.header_constant('NF_LR_CONST'), 0, 0.0)
        return (self.warmup_steps or 0, self.warmup_start) + tail


class _HostSchedule:
    """``_LrRule`` on the torch.optim path where torch's StepLR does not cover it (a warmup, a cosine that holds at its floor): the
    surface FlowTrainer uses of a torch scheduler -- ``step()`` after every optimizer step or replay, ``last_epoch`` -- writing the
    group's ``lr`` (in place where it is the device tensor a captured framework optimizer reads) and ``initial_lr``."""

    def __init__(self, optim, rule, base, pos=0):
        self.optim, self.rule, self.base, self.last_epoch = optim, rule, float(base), int(pos)
        self._write()

    def _write(self):
        g = self.optim.param_groups[0]
        lr = self.rule.rate(self.base, self.last_epoch)
        g['initial_lr'] = self.base
        if isinstance(g['lr'], torch.Tensor):
            g['lr'].fill_(lr)
        else:
            g['lr'] = lr
        self._last_lr = [lr]

    def step(self):
        self.last_epoch += 1
        self._write()

    def get_last_lr(self):
        return self._last_lr


class _FlatOptimizer:
    """What the fused optimizers (FlatAdam, FlatRMSprop, FlatAdamax, FlatAdamW) share: ONE fused HIP launch over the flat
    parameter / gradient buffers of a GradBucket, with ``lr`` and the step counter on the device, so that a captured hipGraph keeps working when the rate changes (``set_lr``).

    ``decay_steps`` (None: no schedule, no extra launch) puts torch's StepLR on the device (nf_lr_step_decay, one thread, enqueued
    in front of the optimizer launch and therefore part of a captured step): optimizer step t = 1, 2, ... since construction or the
    last checkpoint load runs at ``base_lr * decay_ratio ** ((t - 1) // decay_steps)``, the rate StepLR gives when scheduler.step()
    follows optim.step() (main.py:89-90).  ``sched_pos`` counts those steps; it is NOT ``step_count``, which a checkpoint carries on
    (Adam's bias correction) while the reference's schedule restarts at every load.  ``lr`` holds the rate in use.

    ``lr_warmup_steps`` / ``lr_warmup_start`` / ``cosine_steps`` / ``lr_min`` (none given: the launches above and nothing else) put
    the whole rule of ``_LrRule`` -- linear warmup times constant, StepLR or cosine decay, DESIGN.md 4.2 -- on the device instead:
    nf_lr_schedule, one thread in the same place, reading the same ``base_lr`` and ``sched_pos``.

    ``max_grad_norm`` / ``skip_nonfinite`` / ``ema_decay`` (all off by default: the launches are then the plain ones) turn the
    optimizer launch into nf_grad_guard + the guarded step (csrc/optim_guard.hip): the gradient's 2-norm in float64,
    torch's clip scale and a skip flag in a device control block, the step reading both from there, the average ``ema`` updated in the
    same pass.  ``step_count`` does not advance on a skipped step; ``sched_pos`` does.  ``guard_state()`` reads the block.  Neither the
    average nor the skip count is torch optimizer state: ``torch_state_dict()`` does not carry them."""

    KIND = None                     # 'Adam' / 'RMSprop' / 'Adamax' / 'AdamW': the torch.optim class whose state_dict format torch_state_dict() speaks
    MOMENTS = ()                    # names of the per-parameter moment buffers, as torch.optim names them

    def _init_common(self, bucket, lr, decay_steps, decay_ratio, max_grad_norm=None, skip_nonfinite=False, ema_decay=None,
                     **schedule_kw):
        self._rule = _LrRule(lr, decay_steps, decay_ratio, **schedule_kw)
        if bucket.flat_params is None:
            raise ValueError('%s needs GradBucket(..., flatten_params=True)' % type(self).__name__)
        from . import _native as N
        self._N = N
        self.bucket = bucket
        dev = bucket.flat.device
        for k in self.MOMENTS:
            setattr(self, k, torch.zeros_like(bucket.flat))
        self.step_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lr = torch.full((1, ), float(lr), dtype=torch.float32, device=dev)
        self._lr_host = float(lr)   # the rate as the caller gave it (a double): what a checkpoint records while ``lr`` still rounds to it
        self.decay_steps, self.decay_ratio = self._rule.decay_steps, self._rule.decay_ratio
        if self._rule.active:
            self.base_lr = torch.full((1, ), float(lr), dtype=torch.float64, device=dev)
            self.sched_pos = torch.zeros(1, dtype=torch.int32, device=dev)
            if self._rule.general:
                self.lr.fill_(self._rule.rate(lr, 0))   # (a warmup starts below the base rate)
        # the guarded step (csrc/optim_guard.hip).  With all three off none of the tensors below exists and _launch() issues the
        # plain nf_adam_step / nf_rmsprop_step; with any of them on it is nf_grad_guard followed by the guarded step
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = _check_ema_decay(ema_decay)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite or self.ema_decay is not None
        self.guard_ctl = self._partials = self.ema = None
        if self.guarded:
            # nf_guard_ctl: float grad_norm, clip_scale; int skip, skipped, ema_count, reserved[3] -- allocated once, a captured step
            # replays on it
            self.guard_ctl = torch.zeros(8, dtype=torch.int32, device=dev)
            self._partials = torch.zeros(N.header_constant('NF_GUARD_MAX_PARTIALS'), dtype=torch.float64, device=dev)
            if self.ema_decay is not None:
                self.ema = bucket.flat_params.detach().clone()      # (the first step that is taken overwrites it with the parameters)

    def _guard(self):
        """nf_grad_guard over the bucket: norm, clip scale and skip flag into the control block; ticks step_count unless it skips"""
        N, b = self._N, self.bucket
        N.call('nf_grad_guard', N.ptr(b.flat), b.numel, 0.0 if self.max_grad_norm is None else self.max_grad_norm,
               1 if self.skip_nonfinite else 0, N.ptr(self._partials, (torch.float64, )), N.ptr(self.guard_ctl),
               N.ptr(self.step_count), N.stream())

    def guard_state(self):
        """{'grad_norm', 'clip_scale'} of the last step, {'skipped', 'steps'}: the steps refused for a non-finite gradient and the steps
        taken since construction (a checkpoint load restores the first and leaves the second at 1 or more).  ONE host read."""
        if not self.guarded:
            raise ValueError('%s was built without max_grad_norm / skip_nonfinite / ema_decay: there is no guard state' % type(self).__name__)
        w = self.guard_ctl.cpu()
        f = w[:2].view(torch.float32)
        return {'grad_norm': float(f[0]), 'clip_scale': float(f[1]), 'skipped': int(w[3]), 'steps': int(w[4])}

    def swap_ema_(self):
        """parameters <-> averaged weights, in place (nf_swap_f32): no temporary, no pointer moves"""
        N, b = self._N, self.bucket
        if self.ema is None:
            raise ValueError('%s was built without ema_decay' % type(self).__name__)
        self._check_homed()
        N.call('nf_swap_f32', N.ptr(b.flat_params), N.ptr(self.ema), b.numel, N.stream())

    def set_lr(self, lr):
        """the rate of a trainer without a schedule, the BASE rate of one with a schedule"""
        self.lr.fill_(float(lr))
        self._lr_host = float(lr)
        if self._rule.active:
            self.base_lr.fill_(float(lr))
            self.lr.fill_(self.scheduled_lr(float(lr), int(self.sched_pos.item())))

    def scheduled_lr(self, base, pos):
        """host restatement of nf_lr_step_decay / nf_lr_schedule (``_LrRule.rate``): the rate of the step that follows ``pos``
        completed ones"""
        return self._rule.rate(base, pos)

    def set_schedule(self, base_lr, pos):
        """restart (pos = 0) or reposition the schedule; the state a captured graph reads is rewritten in place"""
        self.base_lr.fill_(float(base_lr))
        self.sched_pos.fill_(int(pos))
        self.lr.fill_(self.scheduled_lr(base_lr, pos))

    def _check_homed(self):
        # the parameters must still live in the flat buffer (net.to() / .cpu() after construction re-homes p.data silently)
        b = self.bucket
        p0, p1 = b.params[0], b.params[-1]
        if (p0.data_ptr() != b.flat_params.data_ptr()
                or p1.data_ptr() + p1.numel() * 4 != b.flat_params.data_ptr() + b.numel * 4):
            raise RuntimeError('%s: the parameters no longer live in the GradBucket\'s flat buffer (was the model moved '
                               'with .to() / .cpu() after the trainer was built?); build a new FlowTrainer' % type(self).__name__)

    def step(self):
        N = self._N
        self._check_homed()
        if self._rule.general:
            N.call('nf_lr_schedule', N.ptr(self.lr), N.ptr(self.base_lr, (torch.float64, )), N.ptr(self.sched_pos),
                   *self._rule.native_args(), N.stream())
        elif self.decay_steps is not None:
            N.call('nf_lr_step_decay', N.ptr(self.lr), N.ptr(self.base_lr, (torch.float64, )), N.ptr(self.sched_pos),
                   self.decay_steps, self.decay_ratio, N.stream())
        self._launch()

    # -- the private flat format (unchanged) ---------------------------------------------------------------------------------------
    def state_dict(self):
        sd = {k: getattr(self, k) for k in self.MOMENTS}
        sd.update({'step': self.step_count, 'lr': self.lr})
        return sd

    def load_state_dict(self, sd):
        for k, t in self.state_dict().items():
            t.copy_(sd[k])

    # -- torch.optim's format: what the reference's checkpoints hold (main.py:94-107) -----------------------------------------------
    def _hyper(self):
        raise NotImplementedError

    def _torch_group(self, lr):
        """param_groups[0] as the installed torch.optim class of the same hyper-parameters writes it (whatever keys that version
        carries), taken from a throw-away instance over one scalar"""
        cls = getattr(torch.optim, self.KIND)
        group = dict(cls([torch.nn.Parameter(torch.zeros(1))], lr=float(lr), **self._hyper()).state_dict()['param_groups'][0])
        return group

    def torch_state_dict(self):
        """the optimizer state in ``torch.optim.<KIND>.state_dict()`` format: ``state[i]`` keyed by the parameter's position in the
        iterable the bucket was built from (``net.parameters()``; frozen parameters hold a position and no state, as in torch),
        per-parameter ``step`` and moments shaped like the parameter (copies: the flat buffers stay where they are).  An optimizer
        that never stepped has no state entries, like torch's."""
        b = self.bucket
        step = int(self.step_count.item())
        state = {}
        if step > 0:
            o = 0
            for i, p in zip(b.index, b.params):
                n = p.numel()
                e = {'step': torch.tensor(float(step), dtype=torch.float32)}
                for k in self.MOMENTS:
                    e[k] = getattr(self, k)[o:o + n].view_as(p).clone()
                state[i] = e
                o += n
        lr = float(self.lr.item())
        if float(torch.tensor(self._lr_host, dtype=torch.float32)) == lr:
            lr = self._lr_host
        if self._rule.active:                                       # torch's group holds the rate of the NEXT step after scheduler.step()
            lr = self.scheduled_lr(self.base_lr.item(), self.sched_pos.item())
        group = self._torch_group(lr)
        if self._rule.active:
            group['initial_lr'] = float(self.base_lr.item())        # (the key a torch scheduler adds to the group)
        group['params'] = list(range(b.n_all))
        return {'state': state, 'param_groups': [group]}

    def load_torch_state_dict(self, sd):
        """the reverse: moments and step into the flat buffers (in place, a captured graph goes on reading them), ``lr`` from the
        group.  The other hyper-parameters are launch arguments, frozen into a captured graph: they must equal this optimizer's.
        A schedule, if any, restarts at position 0 from the loaded rate, as the reference's does after load_ckpt -- a poor fit for a
        warmup, which then runs again from ``lr_warmup_start`` times the saved rate: ``FlowTrainer.load_ckpt(resume_schedule=True)``
        (or ``set_schedule(base, pos)`` after this call) continues it instead."""
        groups = sd['param_groups']
        if len(groups) != 1:
            raise ValueError('%s holds one parameter group, the state dict has %d' % (type(self).__name__, len(groups)))
        group, b = groups[0], self.bucket
        if len(group['params']) != b.n_all:
            raise ValueError('the state dict covers %d parameters, the model has %d' % (len(group['params']), b.n_all))
        for k, mine in self._hyper().items():
            theirs = group.get(k, mine)
            theirs = tuple(float(x) for x in theirs) if isinstance(theirs, (tuple, list)) else float(theirs)
            mine = tuple(float(x) for x in mine) if isinstance(mine, (tuple, list)) else float(mine)
            if theirs != mine:
                raise ValueError('%s was built with %s = %r, the state dict was written with %r; build the optimizer with the '
                                 'checkpoint\'s hyper-parameters' % (type(self).__name__, k, mine, theirs))
        if bool(group.get('decoupled_weight_decay', False)) != (self.KIND == 'AdamW'):
            raise ValueError('%s was built with decoupled_weight_decay = %r, the state dict was written with %r'
                             % (type(self).__name__, self.KIND == 'AdamW', bool(group.get('decoupled_weight_decay', False))))
        for k in ('amsgrad', 'centered', 'maximize'):
            if group.get(k, False):
                raise ValueError('%s does not implement %s=True' % (type(self).__name__, k))
        if float(group.get('momentum', 0.0)) != 0.0:
            raise ValueError('%s does not implement momentum' % type(self).__name__)
        where = {pid: j for j, pid in enumerate(group['params'])}      # torch keys the state by the ids listed in the group
        state = {where[k]: v for k, v in sd['state'].items()}
        steps = {int(float(e['step'])) for e in state.values()}
        if len(steps) > 1:
            raise ValueError('per-parameter step counts differ (%s): one fused launch keeps one counter' % sorted(steps))
        with torch.no_grad():
            o = 0
            for i, p in zip(b.index, b.params):
                n = p.numel()
                e = state.get(i)
                for k in self.MOMENTS:
                    dst = getattr(self, k)[o:o + n]
                    if e is None:                           # torch keeps no state for a parameter that never saw a gradient
                        dst.zero_()
                    else:
                        dst.copy_(e[k].reshape(-1))
                o += n
            self.step_count.fill_(steps.pop() if steps else 0)
            lr = float(group['lr'])
            self.lr.fill_(lr)
            self._lr_host = lr
            if self._rule.active:
                self.set_schedule(lr, 0)


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam semantics (the reference's optimizer, main.py:56-64) as ONE fused HIP launch over the flat
    parameter / gradient buffers of a GradBucket.  ``lr`` and the step counter live on the device, so a captured
    hipGraph keeps working when a scheduler changes the rate (``set_lr``, or the on-device StepLR of ``decay_steps``)."""

    KIND, MOMENTS = 'Adam', ('exp_avg', 'exp_avg_sq')
    ENTRY = 'nf_adam_step'          # the plain launch; ENTRY + '_guarded' is the guarded one.  FlatAdamax and FlatAdamW differ in these
                                    # three names (and their defaults) alone: the entry points share one argument list

    def __init__(self, bucket, lr=1.0e-4, betas=(0.9, 0.999), eps=1.0e-8, weight_decay=0.0, decay_steps=None, decay_ratio=0.5,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, lr_warmup_steps=None, lr_warmup_start=1.0 / 3.0,
                 cosine_steps=None, lr_min=0.0):
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self._init_common(bucket, lr, decay_steps, decay_ratio, max_grad_norm, skip_nonfinite, ema_decay,
                          lr_warmup_steps=lr_warmup_steps, lr_warmup_start=lr_warmup_start, cosine_steps=cosine_steps, lr_min=lr_min)

    def _hyper(self):
        return {'betas': (float(self.betas[0]), float(self.betas[1])), 'eps': self.eps, 'weight_decay': self.weight_decay}

    def _launch(self):
        N, b = self._N, self.bucket
        m, s = (getattr(self, k) for k in self.MOMENTS)
        if self.guarded:
            self._guard()
            N.call(self.ENTRY + '_guarded', N.ptr(b.flat_params), N.ptr(b.flat), N.ptr(m), N.ptr(s),
                   N.ptr(self.step_count), N.ptr(self.lr), self.betas[0], self.betas[1], self.eps, self.weight_decay,
                   N.ptr(self.guard_ctl), N.ptr(self.ema), self.ema_decay or 0.0, b.numel, N.stream())
            return
        N.call(self.ENTRY, N.ptr(b.flat_params), N.ptr(b.flat), N.ptr(m), N.ptr(s),
               N.ptr(self.step_count), N.ptr(self.lr), self.betas[0], self.betas[1], self.eps, self.weight_decay, 1.0,
               b.numel, N.stream())


class FlatAdamax(FlatAdam):
    """torch.optim.Adamax (Glow's optimizer) as one fused HIP launch, nf_adamax_step: the second buffer is ``exp_inf``, the running
    infinity norm max(beta2 u, |g| + eps), and only the first moment is bias-corrected.  Same surface and checkpoint format code as
    FlatAdam: ``torch_state_dict()`` is what torch.optim.Adamax writes and loads."""

    KIND, MOMENTS, ENTRY = 'Adamax', ('exp_avg', 'exp_inf'), 'nf_adamax_step'

    def __init__(self, bucket, lr=2.0e-3, **kw):
        super().__init__(bucket, lr=lr, **kw)


class FlatAdamW(FlatAdam):
    """torch.optim.AdamW -- Adam with DECOUPLED weight decay: p *= 1 - lr * weight_decay ahead of the update, no L2 term in the
    gradient (which the weight-normed conditioners' ``weight_g`` takes badly) -- as one fused HIP launch, nf_adamw_step.  The group of
    ``torch_state_dict()`` carries ``decoupled_weight_decay``; a guarded step that is skipped does not decay either."""

    KIND, ENTRY = 'AdamW', 'nf_adamw_step'

    def __init__(self, bucket, lr=1.0e-3, weight_decay=1.0e-2, **kw):
        super().__init__(bucket, lr=lr, weight_decay=weight_decay, **kw)


class FlatRMSprop(_FlatOptimizer):
    """torch.optim.RMSprop with momentum 0 and centered False -- the form the reference constructs (main.py:56-59) -- as one fused
    HIP launch (nf_rmsprop_step) over the flat buffers; same surface as FlatAdam."""

    KIND, MOMENTS = 'RMSprop', ('square_avg', )

    def __init__(self, bucket, lr=1.0e-2, alpha=0.99, eps=1.0e-8, weight_decay=0.0, decay_steps=None, decay_ratio=0.5,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, lr_warmup_steps=None, lr_warmup_start=1.0 / 3.0,
                 cosine_steps=None, lr_min=0.0):
        self.alpha, self.eps, self.weight_decay = alpha, eps, weight_decay
        self._init_common(bucket, lr, decay_steps, decay_ratio, max_grad_norm, skip_nonfinite, ema_decay,
                          lr_warmup_steps=lr_warmup_steps, lr_warmup_start=lr_warmup_start, cosine_steps=cosine_steps, lr_min=lr_min)

    def _hyper(self):
        return {'alpha': self.alpha, 'eps': self.eps, 'weight_decay': self.weight_decay}

    def _launch(self):
        N, b = self._N, self.bucket
        if self.guarded:
            self._guard()
            N.call('nf_rmsprop_step_guarded', N.ptr(b.flat_params), N.ptr(b.flat), N.ptr(self.square_avg), N.ptr(self.lr), self.alpha,
                   self.eps, self.weight_decay, N.ptr(self.guard_ctl), N.ptr(self.ema), self.ema_decay or 0.0, b.numel, N.stream())
            return
        N.call('nf_rmsprop_step', N.ptr(b.flat_params), N.ptr(b.flat), N.ptr(self.square_avg), N.ptr(self.step_count),
               N.ptr(self.lr), self.alpha, self.eps, self.weight_decay, 1.0, b.numel, N.stream())


def _to_reference_layout(sd, bucket):
    """a torch.optim state dict over ``bucket.params`` (the trainable parameters only) re-keyed by position in net.parameters(),
    the layout of the reference's ``torch.optim.X(net.parameters())`` (main.py:57-64)"""
    group = dict(sd['param_groups'][0])
    group['params'] = list(range(bucket.n_all))
    group['lr'] = float(group['lr'])                    # (a device tensor under a captured framework optimizer)
    return {'state': {bucket.index[k]: v for k, v in sd['state'].items()}, 'param_groups': [group]}


def _from_reference_layout(sd, bucket):
    group = dict(sd['param_groups'][0])
    if len(group['params']) != bucket.n_all:
        raise ValueError('the state dict covers %d parameters, the model has %d' % (len(group['params']), bucket.n_all))
    back = {i: k for k, i in enumerate(bucket.index)}
    group['params'] = list(range(len(bucket.params)))
    return {'state': {back[i]: v for i, v in sd['state'].items() if i in back}, 'param_groups': [group]}


class _HipStepGraph:
    """one captured piece of a train step: a torch.cuda.CUDAGraph (= hipGraph on ROCm).  ``FlowTrainer(graph_factory=...)`` takes any
    class with the same two methods; the world-size-2 gloo test passes one that re-runs the closure, so that the capture / replay /
    all-reduce-between-two-graphs control flow of the N > 1 path is exercised without a GPU."""

    def __init__(self):
        self.g = torch.cuda.CUDAGraph()

    def capture(self, fn):
        # thread_local: a collective watchdog / other host thread touching the runtime must not invalidate the capture
        with torch.cuda.graph(self.g, capture_error_mode='thread_local'):
            return fn()

    def replay(self):
        self.g.replay()


class _EmaWeights:
    """``with trainer.ema_weights():`` -- two in-place exchanges of parameters and average, the second one in ``__exit__``"""

    def __init__(self, trainer):
        self.trainer = trainer

    def __enter__(self):
        tr = self.trainer
        if tr._in_ema:
            raise RuntimeError('FlowTrainer.ema_weights() does not nest: the parameters already hold the averaged weights')
        tr._swap_ema()
        tr._in_ema = True
        return tr

    def __exit__(self, *exc):
        self.trainer._swap_ema()
        self.trainer._in_ema = False
        return False


class FlowTrainer:
    """Adam (lr 1e-4, betas (0.9, 0.999): configs/default.yaml:13-20) or RMSprop (``optimizer='rmsprop'``, main.py:56-59) on the
    NLL, gradients in one flat bucket.  ``decay_steps`` / ``decay_ratio``: the reference's StepLR (main.py:68-70, :90), on the device
    and inside the captured step with the fused optimizers, torch.optim.lr_scheduler.StepLR on the torch.optim path (CPU, or
    ``fused_adam=False``).  ``save_ckpt`` / ``load_ckpt`` speak the reference's checkpoint format (main.py:94-107).

    Two parts of the published Glow / Flow++ recipes the reference's switch (main.py:56-70) does not offer, both opt-in:
    ``optimizer='adamax' | 'adamw'`` -- FlatAdamax / FlatAdamW, one fused launch each, torch.optim.Adamax / AdamW on the torch.optim
    path; and ``lr_warmup_steps`` / ``lr_warmup_start`` / ``cosine_steps`` / ``lr_min`` -- a linear warmup of the rate (these are NOT
    ``warmup``, the eager steps before capture) times a constant, the StepLR of ``decay_steps`` counted from the warmup's end, or a
    cosine decay to ``lr_min`` that holds there (``_LrRule``).  On the fused path the rule is one one-thread launch
    inside the captured step (nf_lr_schedule); on the torch.optim path it is host code stepped after every step or replay.

    Three options the reference's loop (main.py:78-92) does not have, all off by default -- the step is then what it always was:
    ``max_grad_norm`` clips the global 2-norm of the (all-reduced) gradient as torch.nn.utils.clip_grad_norm_ does;
    ``skip_nonfinite`` leaves parameters, moments, step count and average untouched when that norm is not finite (the schedule
    position still advances); ``ema_decay`` keeps an exponential moving average of the parameters, copied from them at the first
    step taken (after ActNorm's data-dependent initialisation) -- ``ema_weights()``, ``evaluate(ema=True)``, ``report(ema=True)``.
    With the fused optimizers all three run on the device inside the (captured) step, without a host read (csrc/optim_guard.hip,
    ``guard_state()``); on the torch.optim path they are clip_grad_norm_, a host isfinite check and _foreach_lerp_.  Known limit: a
    non-finite FORWARD has written NaN into BatchNorm running statistics before the guard sees the gradient; running statistics
    are not snapshotted, and ``guard_state()['skipped']`` rising is the signal to reload a checkpoint.

    ``graph=True`` captures zero-grad + forward + backward into one hipGraph and the optimizer step into a second one
    (the gradient all-reduce runs between the two replays; a single process captures both into ONE graph), after
    ``warmup`` eager steps that also perform the data-dependent ActNorm initialisation.  The batch shape is then fixed.
    The call that captures also takes one extra eager step on its batch (allocator warm-up on the capture stream)."""

    TRAIN_MODE_RECHECK = 256        # calls of train_on_batch between two walks over the submodules' training flags

    def __init__(self, net, lr=1.0e-4, betas=(0.9, 0.999), weight_decay=0.0, graph=False, warmup=3, process_group=None,
                 fused_adam=True, sampler=None, sync_stats=False, graph_factory=None, one_graph=None, optimizer='adam',
                 decay_steps=None, decay_ratio=0.5, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, lr_warmup_steps=None,
                 lr_warmup_start=1.0 / 3.0, cosine_steps=None, lr_min=0.0):
        if optimizer not in ('adam', 'rmsprop', 'adamax', 'adamw'):
            raise Exception('optimizer "%s" is currently not supported' % (optimizer, ))       # (the reference's words, main.py:66)
        sched_kw = dict(lr_warmup_steps=lr_warmup_steps, lr_warmup_start=lr_warmup_start, cosine_steps=cosine_steps, lr_min=lr_min)
        self._rule = _LrRule(lr, decay_steps, decay_ratio, **sched_kw)
        self.net = net
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = _check_ema_decay(ema_decay)
        guard_kw = dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay)
        self._guarded = self.max_grad_norm is not None or self.skip_nonfinite or self.ema_decay is not None
        self._in_ema = False        # inside ``with trainer.ema_weights():`` the parameters hold the average
        # the torch.optim path's guard state (host side; the fused optimizers keep theirs in the device control block)
        self._ema = None            # one tensor per bucketed parameter
        self._ema_count = self._skipped = 0
        self._last_norm = None
        self.one_graph = (os.environ.get('NF_DP_ONE_GRAPH', '0') == '1') if one_graph is None else bool(one_graph)
        self._g_whole = False
        # parity mode: every batch statistic over the GLOBAL batch -- W-way data parallelism then reproduces
        # the single-process result on the concatenated batch.  Layer-by-layer launches with collectives in between: no hipGraph.
        self.sync_stats = bool(sync_stats)
        if self.sync_stats:
            graph = False
        self.sampler = sampler      # data.DeviceSampler / data.DeviceDataset (next(), .out, .step): train_on_batch() without a batch draws or
                                    # gathers one on the device, inside the graph
        on_gpu = next(net.parameters()).is_cuda
        if graph and any(getattr(m_, 'masks_redrawn_per_call', False) and getattr(m_, 'draws', 'host') != 'device' for m_ in net.modules()):
            # MADE re-draws its masks from the host's np.random on every call (flows/maf.py:50,72); for D > 2 the draw varies, and a
            # replayed graph would repeat the masks of the captured step.  A MAF on the GPU draws them on the device instead
            # (MAF.draws = 'device', D <= 4); any other such model trains on eager launches
            from .models import MAF
            if on_gpu and isinstance(net, MAF) and net.dims[0] <= 4:
                net.draws = 'device'
            else:
                graph = False
        if graph and on_gpu:
            # a Residual Flow draws its series lengths and noise from the host generators by default: a captured step would replay one
            # frozen draw (or fail at capture on the host-to-device copies).  Its whole-stack kernels draw on the device instead.
            from . import functional as NF
            from .resflow import ResFlow
            for m_ in net.modules():
                if isinstance(m_, ResFlow) and NF.RESFLOW_STACK:
                    m_.draws = 'device'
        fused_adam = bool(fused_adam) and on_gpu
        self.bucket = nfdist.GradBucket(net.parameters(), process_group, flatten_params=fused_adam)
        self.graph = bool(graph)
        self._graph_factory = graph_factory or _HipStepGraph
        self.decay_steps = None if decay_steps is None else int(decay_steps)
        self.decay_ratio = float(decay_ratio)
        self._base_lr = float(lr)
        self._sched = None          # the torch.optim path's schedule (host side, stepped after every optimizer step or replay): torch's
                                    # StepLR for decay_steps alone, _HostSchedule for a rule with a warmup or a cosine
        if fused_adam:
            if optimizer == 'rmsprop':
                self.optim = FlatRMSprop(self.bucket, lr=lr, weight_decay=weight_decay, decay_steps=decay_steps,
                                         decay_ratio=decay_ratio, **guard_kw, **sched_kw)
            else:
                flat_cls = {'adam': FlatAdam, 'adamax': FlatAdamax, 'adamw': FlatAdamW}[optimizer]
                self.optim = flat_cls(self.bucket, lr=lr, betas=betas, weight_decay=weight_decay, decay_steps=decay_steps,
                                      decay_ratio=decay_ratio, **guard_kw, **sched_kw)
        else:
            capturable = self.graph and on_gpu
            if capturable and self.skip_nonfinite:
                raise ValueError('skip_nonfinite=True with a captured torch.optim optimizer (graph=True, fused_adam=False) would need a '
                                 'host read between backward and the optimizer inside the hipGraph; train with the fused optimizers '
                                 '(fused_adam=True) or without graph=True')
            if self.ema_decay is not None:
                self._ema = [p.detach().clone() for p in self.bucket.params]
            if capturable and self._rule.active:
                # a captured framework optimizer reads a python-float rate once, at capture: the scheduler needs a device tensor to fill
                lr = torch.tensor(float(lr), dtype=torch.float32, device=next(net.parameters()).device)
            if optimizer == 'rmsprop':
                self.optim = torch.optim.RMSprop(self.bucket.params, lr=lr, weight_decay=weight_decay, capturable=capturable,
                                                 foreach=True)
            else:
                torch_cls = {'adam': torch.optim.Adam, 'adamax': torch.optim.Adamax, 'adamw': torch.optim.AdamW}[optimizer]
                self.optim = torch_cls(self.bucket.params, lr=lr, betas=betas, weight_decay=weight_decay,
                                       capturable=capturable, foreach=True)
            if self._rule.general:
                self._sched = _HostSchedule(self.optim, self._rule, self._base_lr)
            elif decay_steps is not None:
                self._sched = torch.optim.lr_scheduler.StepLR(self.optim, step_size=self.decay_steps, gamma=self.decay_ratio)
        self.warmup = warmup
        self._eager_steps = 0
        self._replicas_synced = False
        self._g_fb = self._g_opt = None
        self._static_y = self._static_z = self._static_loss = None
        # parameters whose gradient arrives from framework autograd (convolutions, BatchNorm2d ...) rather than from a kernel
        # writing into the bucket: found in the first eager step, afterwards their AccumulateGrad adds (one launch per
        # parameter) are replaced by one gather launch per 128 tensors
        self._gather = on_gpu
        self._indirect = None
        self._calls_since_mode_walk = self.TRAIN_MODE_RECHECK          # the first call walks the tree
        self._captured_det = None

    # -- one step, eager --------------------------------------------------------------------------------------------
    def _forward_backward(self, y):
        if y is None:                                   # on-device data: the draw is part of the step (and of its hipGraph)
            y = self.sampler.next()
        if self.sync_stats:
            with nfdist.sync_statistics(self.bucket.group):
                return self._run_step(y.device, lambda: self._forward_loss(y))
        return self._run_step(y.device, lambda: self._forward_loss(y))

    def _forward_loss(self, y):
        z, ld = self.net(y)
        return z, nll_loss(z, ld)

    def _run_step(self, device, forward_loss):
        """zero the bucket, open the step's scratch arena and the deferred-work queues, run ``forward_loss() -> (z, loss)`` and
        ``loss.backward()``, flush.  ``_forward_backward`` is this with the whole model; tests run slices of a model through it."""
        from .workspace import ARENA
        self.bucket.zero_()
        hooks, seen = [], set()
        if self._gather and self._indirect is None:     # first step: watch which parameters autograd itself produces
            for i, p in enumerate(self.bucket.params):
                # (a tensor hook also fires, with None, when a hand-written backward wrote into the bucket and returned nothing)
                hooks.append(p.register_hook(lambda g, i=i: seen.add(i) if g is not None else None))
        elif self._indirect:
            for i in self._indirect:
                self.bucket.params[i].grad = None       # AccumulateGrad then keeps the incoming tensor: no add launch
        from .fused import FPP_DEFER
        from .fused_conv import CONV_DEFER
        ARENA.begin(device)                             # one memset for every zero-initialised accumulator of the step
        FPP_DEFER.begin()                               # the Flow++ steps' slab finalizes: all of them in one go after backward
        from .fused_flowpp_img import FPP_IMG_DEFER
        FPP_IMG_DEFER.begin()                           # the image Flow++ conditioners' weight gradients: sixteen convolutions per launch
        CONV_DEFER.begin()                              # the image conditioners' weight-gradient passes: sixteen layers per launch
        try:
            z, loss = forward_loss()
            loss.backward()
        finally:
            FPP_DEFER.flush()
            FPP_IMG_DEFER.flush()
            CONV_DEFER.flush()
            ARENA.end()
            for h in hooks:
                h.remove()
        if hooks:
            self._indirect = sorted(seen)
        elif self._indirect:
            self._gather_indirect()
        from .workspace import _capturing, in_arena
        if not _capturing() and isinstance(loss, torch.Tensor) and in_arena(loss):
            loss = loss.clone()                         # (the arena is zeroed again when the next step begins; inside a capture the loss is
        return z, loss                                  #  the graph's static output, rewritten by every replay)

    def _gather_indirect(self):
        """copy the framework-produced gradients into their bucket slots (nf_multi_copy) and re-attach the views."""
        import ctypes
        from . import _native as N
        from .fused import CopyDesc
        descs = []
        for i in self._indirect:
            p, view = self.bucket.params[i], self.bucket.views[i]
            g = p.grad
            if g is not None and g.data_ptr() != view.data_ptr():
                g = g.contiguous()
                descs.append((g, view))
            p.grad = view
        for k0 in range(0, len(descs), 128):
            chunk = descs[k0:k0 + 128]
            arr = (CopyDesc * len(chunk))(*[CopyDesc(g.data_ptr(), v.data_ptr(), g.numel()) for g, v in chunk])
            N.call('nf_multi_copy', ctypes.addressof(arr), len(chunk), N.stream())

    def _optim_step(self):
        """one eager optimizer step.  The fused optimizers carry their schedule inside ``step()``; the torch.optim path's StepLR is
        host code and follows it here -- and every graph replay in train_on_batch, never inside a capture."""
        self._optim_only()
        if self._sched is not None:
            self._sched.step()

    def _optim_only(self):
        """the optimizer's own step: what a capture records.  The fused optimizers carry clipping, the non-finite guard and the
        average inside ``step()`` (csrc/optim_guard.hip); on the torch.optim path they take their host forms here:
        clip_grad_norm_, an isfinite check of its norm that skips ``optim.step()`` (a host read: never under a real capture, the
        constructor refuses that), and ``_foreach_lerp_`` for the average -- a copy at the first update that is taken."""
        if self._fused or not self._guarded:
            self.optim.step()
            return
        params = self.bucket.params
        if self.max_grad_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
        else:
            norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm([p.grad for p in params])))
        self._last_norm = norm
        if self.skip_nonfinite and not bool(torch.isfinite(norm)):
            self._skipped += 1
            return
        self.optim.step()
        self._ema_count += 1
        if self._ema is not None:
            with torch.no_grad():
                if self._ema_count == 1:
                    torch._foreach_copy_(self._ema, [p.detach() for p in params])
                else:
                    torch._foreach_lerp_(self._ema, [p.detach() for p in params], 1.0 - self.ema_decay)

    def guard_state(self):
        """{'grad_norm', 'clip_scale'} of the last step, 'skipped' (steps refused for a non-finite gradient) and 'steps' (steps taken);
        one host read on the fused path.  ``skipped`` rising is the signal to reload a checkpoint: the guard keeps parameters,
        moments, step count and average clean, but a non-finite FORWARD has already written into the running statistics."""
        if not self._guarded:
            raise ValueError('FlowTrainer was built without max_grad_norm / skip_nonfinite / ema_decay: there is no guard state')
        if self._fused:
            return self.optim.guard_state()
        norm = float('nan') if self._last_norm is None else float(self._last_norm)
        scale = 1.0 if self.max_grad_norm is None else min(1.0, self.max_grad_norm / (norm + 1.0e-6))
        return {'grad_norm': norm, 'clip_scale': scale, 'skipped': self._skipped, 'steps': self._ema_count}

    def ema_weights(self):
        """context manager: inside it the parameters hold the averaged weights (swapped in place: nf_swap_f32 on the fused path, so a
        captured graph's pointers stay valid and no copy of the bucket is made); on exit -- also by an exception -- the iterate is
        back, bit for bit.  Buffers (running statistics) are not averaged and stay the live ones.  No training inside the block."""
        if self.ema_decay is None:
            raise ValueError('FlowTrainer.ema_weights() needs FlowTrainer(..., ema_decay=d)')
        return _EmaWeights(self)

    def _swap_ema(self):
        if self._fused:
            self.optim.swap_ema_()
        else:
            with torch.no_grad():
                params = [p.detach() for p in self.bucket.params]
                tmp = [p.clone() for p in params]
                torch._foreach_copy_(params, self._ema)
                torch._foreach_copy_(self._ema, tmp)

    def _capture(self, y):
        self._static_y = y.clone() if y is not None else None
        if torch.cuda.is_available() and (y is None or y.is_cuda):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):               # one more eager step on the side stream (capture etiquette)
                self._forward_backward(self._static_y)
                self.bucket.all_reduce_mean_()
                self._optim_step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
        else:                                           # (a CPU stand-in graph factory: the same extra eager step, no streams)
            self._forward_backward(self._static_y)
            self.bucket.all_reduce_mean_()
            self._optim_step()
        single = not self.bucket.collective            # no all-reduce between backward and Adam: one graph, one replay
        # N > 1 with one_graph: the flat bucket's all-reduce is captured BETWEEN backward and Adam (ProcessGroupNCCL enqueues the RCCL
        # kernel on the capturing stream): one replay per step instead of two graph launches and an eager collective in between.
        # Opt-in (FlowTrainer(one_graph=True) / NF_DP_ONE_GRAPH=1): no multi-GPU node was available to measure it; a capture that
        # fails falls back to the two-graph form below.
        whole = single

        def forward_backward():
            z, loss = self._forward_backward(self._static_y)
            if whole:
                self.bucket.all_reduce_mean_()          # (no-op at world size 1)
                self._optim_only()
            return z.detach(), loss.detach()
        g_fb = None
        if not single and self.one_graph:
            whole = True
            try:
                g_fb = self._graph_factory()
                self._static_z, self._static_loss = g_fb.capture(forward_backward)
            except Exception as e:
                import warnings
                warnings.warn('the data-parallel step could not be captured as ONE hipGraph (%s: %s); two graphs with the all-reduce '
                              'between them' % (type(e).__name__, e))
                g_fb, whole = None, False
                if torch.cuda.is_available():
                    torch.cuda.synchronize()
        if g_fb is None:
            g_fb = self._graph_factory()
            self._static_z, self._static_loss = g_fb.capture(forward_backward)
        g_opt = None
        if not whole:                                   # N > 1: graph A, the flat bucket's all-reduce (eager, RCCL), graph B = Adam
            g_opt = self._graph_factory()
            g_opt.capture(self._optim_only)
        self._g_fb, self._g_opt = g_fb, g_opt
        self._g_whole = whole
        from . import _native as N_
        self._captured_det = N_.deterministic()

    def train_on_batch(self, y=None):
        """returns (z, loss) like main.py:78-92; with graph=True the returned tensors are the graph's static outputs.
        Raises _native.PersistentKernelTimeout as soon as the host sees that a persistent kernel of an EARLIER launch gave up on
        a grid exchange (sticky pinned error word, no synchronisation: at most one step late)."""
        from . import _native as N
        if self._in_ema:
            raise RuntimeError('FlowTrainer.train_on_batch inside `with trainer.ema_weights():` -- the parameters hold the averaged '
                               'weights there; leave the block before training')
        if y is None and self.sampler is None:
            raise ValueError('train_on_batch() without a batch needs FlowTrainer(..., sampler=data.DeviceSampler(...) or data.DeviceDataset(...))')
        if y is not None and y.is_cuda and y.device.index != torch.cuda.current_device():
            # a model / batch on another GPU than the current one (net.to('cuda:1') without torch.cuda.set_device works in the reference):
            # the launches must go to THAT device's stream and read its copy of the library's globals
            with torch.cuda.device(y.device):
                return self.train_on_batch(y)
        if y is None or y.is_cuda:
            N.check_persistent()
        # Module.train() walks every submodule: 1.24 ms of host time per call on C1's ~1 000 modules -- more than the 1.05 ms the whole
        # step takes on the device.  The root's flag answers for the tree on most calls; a CHILD put into eval() on its own (the root stays
        # in training mode) is found by a walk on the first call and every TRAIN_MODE_RECHECK calls after it
        self._calls_since_mode_walk += 1
        if not self.net.training:
            # the state log_py() / sample_y() / net.eval() leave (main.py alternates train() and eval() at every report, :73-76, :327):
            # Module.train() puts the whole tree back, graph or no graph -- a replay launches what was captured whatever the flags say
            self.net.train()
            self._calls_since_mode_walk = 0
        elif self._calls_since_mode_walk >= self.TRAIN_MODE_RECHECK:
            if any(not m_.training for m_ in self.net.modules()):
                if self._g_fb is not None:
                    raise RuntimeError('FlowTrainer: a submodule was switched to eval() after the step was captured in a hipGraph (the graph '
                                       'replays training-mode launches); build a new FlowTrainer')
                self.net.train()
            self._calls_since_mode_walk = 0
        if self._g_fb is not None and self._captured_det != N.deterministic():
            raise RuntimeError('FlowTrainer: _native.deterministic() was switched after the step was captured in a hipGraph -- the graph holds '
                               'the launch shapes of the mode it was captured in; build a new FlowTrainer')
        if self.graph and self._g_fb is None and self._eager_steps >= self.warmup:
            try:
                self._capture(y)
            except Exception as e:                      # keep training eagerly rather than dying on a capture problem
                import warnings
                warnings.warn('hipGraph capture failed (%s: %s); continuing with eager launches' % (type(e).__name__, e))
                self.graph = False
                self._g_fb = self._g_opt = None
                if torch.cuda.is_available():
                    torch.cuda.synchronize()
        if self._g_fb is not None:
            if not self._replicas_synced:               # warmup=0: no eager step ran before the capture
                self._sync_replicas_after_first_step()
            if self._static_y is not None:
                self._static_y.copy_(y, non_blocking=True)
            self._g_fb.replay()                         # (world size 1, or one_graph: the whole step)
            if self._g_opt is not None:
                self.bucket.all_reduce_mean_()
                self._g_opt.replay()
            if self._sched is not None:
                self._sched.step()
            return self._static_z, self._static_loss
        z, loss = self._forward_backward(y)
        self.bucket.all_reduce_mean_()
        self._optim_step()
        self._eager_steps += 1
        if not self._replicas_synced:
            self._sync_replicas_after_first_step()
        return z.detach(), loss.detach()

    def _sync_replicas_after_first_step(self):
        """The first forward performs the data-dependent ActNorm initialisation (modules.py:238-244) on each replica's OWN
        shard, so the replicas' log_scale / bias differ after step 1.  Data parallelism needs identical replicas:
        rank 0's parameters and buffers win (policy 2); afterwards running statistics evolve per replica
        unless the trainer runs in sync-statistics mode."""
        self._replicas_synced = True
        if self.bucket.collective:
            # every parameter AND buffer: the frozen PLU constants (P, pivots, sign_s), MAF's perm and the running statistics
            # too, so that replicas built from different seeds cannot keep private copies of those
            nfdist.broadcast_parameters(self.net, src=0, group=self.bucket.group, force=True)

    # -- the reference's configuration and checkpoints ------------------------------------------------------------------------------
    @classmethod
    def from_cfg(cls, net, cfg, **kw):
        """``cfg``: the reference's ``cfg.optimizer`` node (configs/default.yaml: name, lr, beta1, beta2, weight_decay, decay_steps,
        decay_ratio), read as main.py:56-70 reads it; ``kw`` goes to the constructor (graph, sampler, ...)."""
        return cls(net, lr=cfg.lr, betas=(cfg.beta1, cfg.beta2), weight_decay=cfg.weight_decay, optimizer=cfg.name,
                   decay_steps=cfg.decay_steps, decay_ratio=cfg.decay_ratio, **kw)

    @property
    def _fused(self):
        return isinstance(self.optim, _FlatOptimizer)

    def current_lr(self):
        """the rate the next optimizer step runs at (synchronises on the fused path)"""
        if self._fused:
            o = self.optim
            return o.scheduled_lr(o.base_lr.item(), o.sched_pos.item()) if o._rule.active else float(o.lr.item())
        return float(self.optim.param_groups[0]['lr'])

    def save_ckpt(self, step, filename):
        """{'net', 'optim', 'step'} with ``optim`` in torch.optim's format over net.parameters(): main.py:94-100.  With ``ema_decay``
        also 'ema' and 'skipped'; without it the file is exactly the reference's."""
        optim = self.optim.torch_state_dict() if self._fused else _to_reference_layout(self.optim.state_dict(), self.bucket)
        ckpt = {'net': self.net.state_dict(), 'optim': optim, 'step': step}
        if self.ema_decay is not None:
            # two keys the reference's load_ckpt (main.py:102-107) never reads: the averaged TRAINABLE parameters by name, shaped like
            # net.state_dict()'s entries, and the count of refused steps
            if self._in_ema:
                raise RuntimeError('FlowTrainer.save_ckpt inside `with trainer.ema_weights():` would save the average as the model')
            ckpt['ema'] = {k: v.clone() for k, v in zip(self._ema_names(), self._ema_views())}
            ckpt['skipped'] = self.guard_state()['skipped']
        torch.save(ckpt, filename)

    def _ema_names(self):
        ids = {id(p): k for k, p in self.net.named_parameters()}
        return [ids[id(p)] for p in self.bucket.params]

    def _ema_views(self):
        """the average as one tensor per bucketed parameter (views of the fused optimizer's flat buffer)"""
        if not self._fused:
            return self._ema
        out, o = [], 0
        for p in self.bucket.params:
            out.append(self.optim.ema[o:o + p.numel()].view_as(p))
            o += p.numel()
        return out

    def load_ckpt(self, filename, resume_schedule=False):
        """main.py:102-107; returns the saved step.  Everything is copied INTO the tensors the trainer already holds, so a step that
        is captured in a hipGraph goes on replaying.  The reference saves no scheduler state: after a load its StepLR restarts at
        position 0 from the saved (already decayed) rate, and so does this one by default.  ``resume_schedule=True`` continues the
        schedule instead: position ``ckpt['step']``, base rate the group's ``initial_lr`` (else the rate this trainer was built with).
        A restart is a poor fit for a rule with a warmup (``lr_warmup_steps``): the warmup runs again, from ``lr_warmup_start`` times
        the saved rate -- which is itself mid-schedule.  Load such a run with ``resume_schedule=True``."""
        if not self._fused and isinstance(self._g_fb, _HipStepGraph):
            raise RuntimeError('FlowTrainer: torch.optim.load_state_dict re-binds the state tensors a captured hipGraph reads; load the '
                               'checkpoint before the step is captured, or train with the fused optimizers (fused_adam=True)')
        ckpt = torch.load(filename, map_location=next(self.net.parameters()).device)
        self.net.load_state_dict(ckpt['net'])
        step = ckpt['step']
        group = ckpt['optim']['param_groups'][0]
        lr = float(group['lr'])
        base = float(group.get('initial_lr', self._base_lr)) if resume_schedule else lr
        pos = int(step) if resume_schedule else 0
        if self._fused:
            self.optim.load_torch_state_dict(ckpt['optim'])
            if self._rule.active:
                self.optim.set_schedule(base, pos)
        else:
            lr_slot = self.optim.param_groups[0]['lr']          # (a device tensor when the framework optimizer is captured)
            self.optim.load_state_dict(_from_reference_layout(ckpt['optim'], self.bucket))
            g = self.optim.param_groups[0]
            if self._rule.active:
                lr = self._rule.rate(base, pos)
            if isinstance(lr_slot, torch.Tensor):
                g['lr'] = lr_slot.fill_(lr)
            else:
                g['lr'] = lr
            if self._rule.general:
                self._sched = _HostSchedule(self.optim, self._rule, base, pos)
            elif self.decay_steps is not None:
                g['initial_lr'] = base
                self._sched = torch.optim.lr_scheduler.StepLR(self.optim, step_size=self.decay_steps, gamma=self.decay_ratio)
                self._sched.last_epoch = pos
                self._sched._last_lr = [lr]
            else:
                g.pop('initial_lr', None)
        if self.ema_decay is not None:
            # into the tensors that exist (a captured step goes on).  A file without 'ema' seeds the average from the loaded
            # parameters; either way the next update blends instead of copying (ema_count >= 1 before it)
            with torch.no_grad():
                views = self._ema_views()
                if 'ema' in ckpt:
                    for k, v in zip(self._ema_names(), views):
                        v.copy_(ckpt['ema'][k])
                else:
                    for p, v in zip(self.bucket.params, views):
                        v.copy_(p.detach())
                skipped = int(ckpt.get('skipped', 0))
                if self._fused:
                    self.optim.guard_ctl[3].fill_(skipped)
                    self.optim.guard_ctl[4].clamp_(min=1)
                else:
                    self._skipped, self._ema_count = skipped, max(self._ema_count, 1)
        return step

    # -- evaluation -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def log_py(self, y):
        self.net.eval()
        z, ld = self.net(y)
        return standard_normal_logprob(z) + ld

    @torch.no_grad()
    def evaluate(self, dataset, graph=False, keep_rows=False, ema=False):
        """held-out score of the model over a whole device-resident set: main.py:121-127 taken over every sample exactly once.

        ``dataset``  a data.DeviceDataset on the SWEEP schedule (``train_set.sweep_view()`` or ``DeviceDataset(..., sweep=True)``).
        Returns {'n', 'nll' (nats per sample, -sum log p / n), 'stderr' (of nll, from the second moment), 'bits_per_dim'} and, for a
        dequantised image set, 'bits_per_dim_pixel' = bits_per_dim + 8: the density is that of pixel / 256 in [0, 1), 8 bits per
        dimension away from the density of the 0..255 pixel.  D is the size of what the model sees, so with a pad ring it is the PADDED
        size throughout (the ring's constant zeros are scored as data, as the reference's padded MNIST is).
        The model goes to eval() under no_grad; the accumulator and the set's step counter are zeroed, then every step launches
        gather -> net(y) -> nf_logp_accumulate -> advance with NO host synchronisation between batches; the three float64 sums are read
        once at the end (after one all-reduce under an initialised process group, where each rank sweeps its own positions).  Zeroing
        the step makes two calls on the same weights return the same bits, dequantisation noise included.
        ``keep_rows``  also returns 'rows': the float64 log p of this rank's valid samples in the order served (the data-set order for
        the identity order at world size 1).
        ``graph``  one step's launches are captured once and replayed for every step; a capture that raises warns and the sweep runs on
        eager launches.  The model is left in eval(): the next train_on_batch() puts it back, captured or not.
        ``ema``    score the averaged weights (``ema_decay``): the sweep runs inside ``ema_weights()``.  Running statistics (BatchNorm, flow
        BatchNorm) are buffers, not parameters: they are not averaged and stay the live ones."""
        if ema:
            with self.ema_weights():
                return self.evaluate(dataset, graph=graph, keep_rows=keep_rows)
        from . import _native as N
        from .models import Ffjord
        if not getattr(dataset, 'sweep', False):
            raise ValueError('FlowTrainer.evaluate scores every sample exactly once: it takes a sweep-schedule data set, and this one '
                             'follows the loader (which drops the tail) -- pass dataset.sweep_view()')
        if isinstance(self.net, Ffjord):
            raise NotImplementedError('FlowTrainer.evaluate does not serve FFJORD (float64 states, adaptive integration)')
        if dataset.data is None:
            raise RuntimeError('this DeviceDataset was built with device=None: it has no device copy to gather from')
        self.net.eval()
        dev = dataset.data.device
        S, B, D = dataset.steps_per_epoch, dataset.batch, 1
        for d_ in dataset.dims:
            D *= int(d_)
        acc = torch.zeros(3, dtype=torch.float64, device=dev)
        row = torch.empty(B, dtype=torch.float64, device=dev)
        rows_all = torch.empty(S * B, dtype=torch.float64, device=dev) if keep_rows else None

        def one_step():
            y = dataset.gather()
            z, ld = self.net(y)
            if z.dtype != torch.float32 or ld.dtype != torch.float32:
                raise NotImplementedError('FlowTrainer.evaluate takes float32 models, got z %s, ld %s' % (z.dtype, ld.dtype))
            z, ld = z.contiguous(), ld.contiguous()
            N.call('nf_logp_accumulate', N.ptr(z), N.ptr(ld), row.data_ptr(), None, None if rows_all is None else rows_all.data_ptr(),
                   acc.data_ptr(), B, D, dataset.n, dataset.stride, dataset.offset, dataset.step.data_ptr(), N.stream())
            dataset.advance()                           # AFTER the fold has read the step

        g = None
        if graph:
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):           # one eager step on the side stream (capture etiquette); its sums are zeroed below
                    one_step()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                g = self._graph_factory()
                g.capture(one_step)
            except Exception as e:
                import warnings
                warnings.warn('hipGraph capture of the evaluation step failed (%s: %s); continuing with eager launches' % (type(e).__name__, e))
                g = None
                torch.cuda.synchronize()
        acc.zero_()
        dataset.step.zero_()
        for _ in range(S):
            if g is not None:
                g.replay()
            else:
                one_step()
        import torch.distributed as _d
        if _d.is_available() and _d.is_initialized():
            _d.all_reduce(acc, op=_d.ReduceOp.SUM, group=self.bucket.group)
        s1, s2, n = (float(v) for v in acc.cpu())       # the one read of the sweep
        n_i = int(round(n))
        nll = -s1 / n
        var = max(s2 / n - (s1 / n) ** 2, 0.0) * (n / (n - 1.0)) if n_i > 1 else 0.0
        res = {'n': n_i, 'nll': nll, 'stderr': math.sqrt(var / n), 'bits_per_dim': bits_per_dim(nll, dataset.dims)}
        if dataset.image and dataset.dequantize:
            res['bits_per_dim_pixel'] = res['bits_per_dim'] + 8.0
        if keep_rows:
            all_rows = rows_all.cpu().reshape(S, B)
            res['rows'] = torch.cat([all_rows[s, :dataset.valid(s)] for s in range(S)])
        return res

    @torch.no_grad()
    def report(self, y_data, n_samples=None, graph=False, generator=None, map_size=256, canvas=512, radius=2, ema=False):
        """what Model.report computes before matplotlib, tensorboard and the jpg writer take over (main.py:135-284), as numpy arrays
        from ONE host read: everything is queued on the current stream, copied to pinned memory, and synchronised once.  The panels
        (``*_rgb``, ``*_grid``) are uint8 HWC images rasterised on the device (csrc/report.hip) -- the data area alone, no axes, ticks,
        titles or colour bars -- that PIL.Image.fromarray or SummaryWriter.add_image(..., dataformats='HWC') take as they are.
        By the case of main.py:142-147:
          (n, 2)   'z', 'pz', 'y_sample', 'py_sample' (float32); 'z_rgb', 'y_rgb' (canvas, canvas, 3): jet over the finite range of pz /
                   py_sample; 'y_data_rgb': the batch in one colour (jet[0]); 'py_map' (map_size, map_size) float32: the density of the
                   grid of main.py:199-206 through the whole flow; 'py_map_rgb': inferno over (0, 1), image_plot's defaults
          (n, 3)   the same without the map; the scatters are seen through report.view_matrix() (elev 10, azim -80)
          images   'data_grid', 'sample_grid': make_grid(clamp(., 0, 1), nrow=8, pad_value=1) as uint8 HWC, the second over 'y_sample',
                   the first 64 of the samples drawn
        ``n_samples``  default: the reference's max(100, n) for vectors, max(64, n) for images.  ``generator``: of the latent draw.
        ``graph``      (2-D) the chain grid -> net(y) -> log p -> colours is captured once per map_size and replayed by later calls: its
                       input is a constant.  A capture that raises warns and the call continues eagerly, as in ``evaluate``.
        ``ema``        draw and score with the averaged weights (``ema_decay``): the call runs inside ``ema_weights()``; running statistics
                       are buffers and stay the live ones.
        The model is left in eval(), like log_py(): the next train_on_batch() puts it back, captured or not."""
        if ema:
            with self.ema_weights():
                return self.report(y_data, n_samples=n_samples, graph=graph, generator=generator, map_size=map_size, canvas=canvas,
                                   radius=radius)
        from . import report as _report
        return _report.report(self, y_data, n_samples=n_samples, graph=graph, generator=generator, map_size=map_size, canvas=canvas,
                              radius=radius)

    @torch.no_grad()
    def sample_y(self, n, dims, generator=None):
        self.net.eval()
        dev = next(self.net.parameters()).device
        z = torch.randn((n, ) + tuple(dims), device=dev, generator=generator)
        y, ld = self.net.backward(z)
        return y, torch.exp(standard_normal_logprob(z) - ld)
