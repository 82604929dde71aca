"""A compact restatement of the reference's FFJORD (flows/ffjord.py, flows/cnf.py, flows/odeint.py) in plain torch, for any dtype and
device: the yardstick of tests/test_ffjord_host.py and tests/test_gpu_ffjord.py.

  * the field in FORWARD mode: value and tangents in one pass, the softplus derivative written out with F.softplus's threshold rule;
  * the four solvers' host loops, operation by operation (the "adaptive" ones discard their step proposal, odeint.py:80);
  * the adjoint (odeint.py:217-284) with torch.autograd.grad on the forward-mode expression, fresh noise per backward evaluation.

The field's parameters are a list [W1, b1, W2, b2, W3, b3]; noise is a list of (B, S, D) tensors, one per field evaluation in evaluation
order (ignored by the exact trace)."""
import numpy as np
import torch
import torch.nn.functional as F

STAGES = {'midpoint': 2, 'rk4': 4, 'bosha3': 5, 'dopri5': 7}

ADAPTIVE = {                                                               # odeint.py:114-160
    'bosha3': (3, [1.0 / 2.0, 3.0 / 4.0, 1.0, 1.0],
               [[1.0 / 2.0], [0.0, 3.0 / 4.0], [2.0 / 9.0, 1.0 / 3.0, 4.0 / 9.0], [2.0 / 9.0, 1.0 / 3.0, 4.0 / 9.0, 0.0]]),
    'dopri5': (5, [1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0, 1.0],
               [[1.0 / 5.0], [3.0 / 40.0, 9.0 / 40.0], [44.0 / 45.0, -56.0 / 15.0, 32.0 / 9.0],
                [19372.0 / 6561.0, -25360.0 / 2187.0, 64448.0 / 6561.0, -212.0 / 729.0],
                [9017.0 / 3168.0, -355.0 / 33.0, 46732.0 / 5247.0, 49.0 / 176.0, -5103.0 / 18656.0],
                [35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0]]),
}


def softplus_pair(x):
    """F.softplus (beta 1, threshold 20) and its derivative as autograd computes it: e^x / (e^x + 1), 1 above the threshold"""
    e = torch.exp(torch.where(x > 20.0, torch.zeros_like(x), x))          # (no inf / inf in the branch that is not taken)
    return F.softplus(x), torch.where(x > 20.0, torch.ones_like(x), e / (e + 1.0))


def field(params, t, z, w, trace, pre=None):
    """ODENet.forward (cnf.py:107-121): (f, trace estimate).  trace 'hutchinson': w (B, S, D), mean_s w_s^T J w_s; 'exact': sum_i J_ii.
    ``pre`` (a list) receives the two pre-activations."""
    W1, b1, W2, b2, W3, b3 = params
    tt = torch.ones_like(z[:, :1]) * t
    h1 = F.linear(torch.cat([tt, z], dim=1), W1, b1)
    a1, s1 = softplus_pair(h1)
    h2 = F.linear(torch.cat([tt, a1], dim=1), W2, b2)
    a2, s2 = softplus_pair(h2)
    f = F.linear(torch.cat([tt, a2], dim=1), W3, b3)
    if pre is not None:
        pre += [h1, h2]
    D = z.shape[1]
    if trace == 'exact':
        tangents, scale = [torch.eye(D, dtype=z.dtype, device=z.device)[i].expand_as(z) for i in range(D)], 1.0
    else:
        w = w.to(z.dtype)
        tangents, scale = [w[:, s, :] for s in range(w.shape[1])], 1.0 / w.shape[1]
    quads = []
    for v in tangents:
        d = (((v @ W1[:, 1:].t()) * s1) @ W2[:, 1:].t() * s2) @ W3[:, 1:].t()
        quads.append(torch.sum(d * v, dim=1))
    return f, torch.stack(quads, dim=1).sum(dim=1) * scale


def stage_times_and_states(func, x, times, method):
    """``odeint`` (odeint.py:201-214) on a TUPLE state: func(t, state) -> tuple of derivatives.  Returns the final state."""
    add = lambda a, b: tuple(p + q for p, q in zip(a, b))                  # noqa: E731
    mul = lambda a, c: tuple(p * c for p in a)                              # noqa: E731
    if method in ('midpoint', 'rk4'):                                       # odeint.py:13-52
        for t0, t1 in zip(times[:-1], times[1:]):
            dt = t1 - t0
            k1 = mul(func(t0, x), dt)
            if method == 'midpoint':
                dx = mul(func(t0 + 0.5 * dt, add(x, mul(k1, 0.5))), dt)
            else:
                k2 = mul(func(t0 + 0.5 * dt, add(x, mul(k1, 0.5))), dt)
                k3 = mul(func(t0 + 0.5 * dt, add(x, mul(k2, 0.5))), dt)
                k4 = mul(func(t0 + dt, add(x, k3)), dt)
                dx = tuple((a + 2.0 * b + 2.0 * c + d) / 6.0 for a, b, c, d in zip(k1, k2, k3, k4))
            x = add(x, dx)
        return x
    order, c_t, c_x = ADAPTIVE[method]                                      # odeint.py:68-111
    t_start, t_end = times[0], times[-1]
    dt = (t_end - t_start) / (len(times) - 1)
    dt_min, dt_max = torch.abs(dt) * 0.2, torch.abs(dt) * 5.0
    x0, x1, t0, t1 = x, x, t_start, t_start
    while abs(t1 - t_end) > 1.0e-4:
        ks = [mul(func(t1, x1), dt)]
        for i in range(order + 1):
            kx = tuple(sum([k[c] * cc for k, cc in zip(ks, c_x[i])]) for c in range(len(x1)))
            ks.append(mul(func(t1 + c_t[i] * dt, add(x1, kx)), dt))
        dx = tuple(sum([k[c] * cc for k, cc in zip(ks, c_x[-1])]) for c in range(len(x1)))
        dt = torch.clamp(torch.abs(dt), dt_min, dt_max) * torch.sign(dt)
        if (t_start - (t1 + dt)) * (t_end - (t1 + dt)) > 0.0:
            dt = t_end - t1
        x0, t0 = x1, t1
        x1, t1 = add(x1, dx), t1 + dt
    slope = (t_end - t0) / (t1 - t0)
    return tuple(a + (b - a) * slope for a, b in zip(x0, x1))


def evaluations(times, method):
    """number of field evaluations of one integration (the length of the noise list it consumes)"""
    n = [0]

    def f(t, x):
        n[0] += 1
        return (torch.zeros(()), )
    stage_times_and_states(f, (torch.zeros(()), ), times, method)
    return n[0]


def stage_times(times, method):
    """the t handed to the field, in evaluation order (float64 values)"""
    out = []

    def f(t, x):
        out.append(float(t))
        return (torch.zeros((), dtype=torch.float64), )
    stage_times_and_states(f, (torch.zeros((), dtype=torch.float64), ), times, method)
    return out


def integrate(params, z, ld, times, method, trace, noise):
    """odeint of (z, ld) without a graph; noise: list consumed in evaluation order"""
    it = iter(noise if noise is not None else [])

    def f(t, x):
        return field(params, t, x[0], None if trace == 'exact' else next(it), trace)
    with torch.no_grad():
        return stage_times_and_states(f, (z, ld), times, method)


def adjoint(params, z_end, ld_end, g_z, g_ld, times, method, trace, noise):
    """OdeIntAdjoint.backward (odeint.py:266-284): integrates (a_z, a_ld, z, ld, g_theta) over reversed(times) from the saved final state;
    returns (grad z, grad ld, [grad of each parameter]).  noise: the backward pass's own draws."""
    it = iter(noise if noise is not None else [])

    def aug(t, s):
        a_z, a_ld, z = s[0], s[1], s[2]
        with torch.enable_grad():
            zz = z.detach().requires_grad_(True)
            pp = [p.detach().requires_grad_(True) for p in params]
            f, tr = field(pp, t.detach(), zz, None if trace == 'exact' else next(it), trace)
            vj = torch.autograd.grad((f, tr), [zz] + pp, grad_outputs=(-1.0 * a_z, -1.0 * a_ld), allow_unused=True)
        vj = [torch.zeros_like(q) if v is None else v for v, q in zip(vj, [zz] + pp)]
        return (vj[0], torch.zeros_like(a_ld), f.detach(), tr.detach()) + tuple(vj[1:])
    with torch.no_grad():
        s0 = (g_z, g_ld, z_end, ld_end) + tuple(torch.zeros_like(p) for p in params)
        out = stage_times_and_states(aug, s0, torch.flip(times, dims=[0]), method)
    return out[0], out[1], list(out[4:])


class _Adjoint(torch.autograd.Function):
    """the autograd node of one CNF direction, float64 inside (cnf.py:145-173)"""

    @staticmethod
    def forward(ctx, z, ld, times, method, trace, noise, noise_bwd, *params):
        z1, ld1 = integrate([p.detach() for p in params], z.detach(), ld.detach(), times, method, trace, noise)
        ctx.cfg = (times, method, trace, noise_bwd)
        ctx.save_for_backward(z1, ld1, *params)
        return z1, ld1

    @staticmethod
    def backward(ctx, g_z, g_ld):
        z1, ld1, *params = ctx.saved_tensors
        times, method, trace, noise_bwd = ctx.cfg
        a_z, a_ld, gp = adjoint([p.detach() for p in params], z1, ld1, g_z, g_ld, times, method, trace, noise_bwd)
        return (a_z, a_ld, None, None, None, None, None) + tuple(gp)


def cnf(params, z, ld, times, method, trace, noise, noise_bwd, flipped):
    """CNF.forward (flipped=True: over the flipped times) / CNF.backward (times as stored) with the casts of cnf.py:146-158"""
    org = z.dtype
    tt = torch.flip(times, dims=[0]) if flipped else times
    z1, ld1 = _Adjoint.apply(z.double(), ld.double(), tt, method, trace, noise, noise_bwd, *params)
    return z1.to(org), ld1.to(org)


def actnorm(z, ld, log_scale, bias, inverse=False):
    """modules.py:246-256 (initialised)"""
    if inverse:
        return z * torch.exp(log_scale) + bias, ld + torch.sum(log_scale)
    return (z - bias) / torch.exp(log_scale), ld - torch.sum(log_scale)


def actnorm_init(z, eps=1.0e-5):
    """modules.py:239-243: (log_scale, bias) of the first batch"""
    return torch.log(torch.std(z, dim=0) + eps).view(1, -1), torch.mean(z, dim=0).view(1, -1)


def model_params(sd, layers, requires_grad=False):
    """[(log_scale, bias, [W1, b1, W2, b2, W3, b3])] of an Ffjord state_dict, dtypes as stored"""
    out = []
    for i in range(layers):
        t = [sd['net.layers.%d.%s' % (2 * i, n)] for n in ('log_scale', 'bias')]
        t += [sd['net.layers.%d.func.layers.%d.linear.%s' % (2 * i + 1, j, n)] for j in range(3) for n in ('weight', 'bias')]
        t = [x.detach().clone().requires_grad_(requires_grad) for x in t]
        out.append((t[0], t[1], t[2:]))
    return out


def model_forward(layers, y, times, method, trace, noises, noises_bwd, init=False):
    """Ffjord.forward (ffjord.py:36-38).  noises[i] / noises_bwd[i]: the evaluation lists of CNF i and of its backward pass"""
    z, ld = y, torch.zeros(y.shape[0], dtype=y.dtype, device=y.device)
    for i, (ls, b, p) in enumerate(layers):
        if init:
            with torch.no_grad():
                a, c = actnorm_init(z)
                ls.copy_(a)
                b.copy_(c)
        z, ld = actnorm(z, ld, ls, b)
        z, ld = cnf(p, z, ld, times, method, trace, noises[i] if noises else None, noises_bwd[i] if noises_bwd else None, True)
    return z, ld


def model_inverse(layers, z, times, method, trace, noises, noises_bwd=None):
    """Ffjord.backward (ffjord.py:40-42): layers last to first; noises[i] belongs to CNF i"""
    ld = torch.zeros(z.shape[0], dtype=z.dtype, device=z.device)
    for i in range(len(layers) - 1, -1, -1):
        ls, b, p = layers[i]
        z, ld = cnf(p, z, ld, times, method, trace, noises[i] if noises else None, noises_bwd[i] if noises_bwd else None, False)
        z, ld = actnorm(z, ld, ls, b, inverse=True)
    return z, ld


def nll(z, ld):
    """main.py:85 with the standard-normal prior of main.py:49-51"""
    D = z.shape[1]
    logp = -0.5 * torch.sum(z * z, dim=1) - 0.5 * D * float(np.log(2.0 * np.pi))
    return -1.0 * torch.mean(logp + ld)
