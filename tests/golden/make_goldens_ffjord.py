"""
Generates the FFJORD goldens by RUNNING THE UPSTREAM REFERENCE (flows/ffjord.py, flows/cnf.py, flows/odeint.py, imported under the alias
``ref_flows``) on the CPU with seeded inputs.  Data only: parameters, inputs, noise, expected outputs and gradients.

    python tests/golden/make_goldens_ffjord.py          # only where the reference checkout exists

The Hutchinson noise is recorded by wrapping ``torch.randn`` while the reference runs.  Recorded noise does not compress, and a committed
file stays under 1 MiB, so the training noise lives in two files of its own; the S = 4 evaluation noise (another 1.4 MB) is not stored:
those cases record the seed set before the call, the first draw and the sum of all draws, and a test regenerates the draws with
``torch.manual_seed`` and checks both before it uses them.

tests/golden/model_ffjord.npz (L = 2 layers, B = 64, shipped times t0 = 0, t1 = 1, stepsize 0.1):
  d<D>/sd0/<key>                      construction state_dict under torch.manual_seed(100), D = 2 and 3 (float32 ActNorm, float64 field)
  d<D>/y                              input batch (randn * 0.5 from a generator seeded 101)
  d<D>/<solver>/an/<key>              the ActNorm parameters after the first forward's data-dependent initialisation
  d<D>/<solver>/z, /ld, /loss         training-mode forward and main.py's loss (main.py:85), solver in midpoint rk4 bosha3 dopri5
  d<D>/<solver>/grad/<param>          every parameter's gradient of that loss (adjoint: fresh noise in the backward pass)
  d<D>/eval/sd/<key>                  the state the evaluation cases run on (dopri5's state after its training forward)
  d<D>/eval/<trace>/fwd/z, /ld        net.eval(); net(y), trace in exact hutchinson
  d<D>/eval/<trace>/inv/u, /x, /ld    net.backward(u), u = randn * 0.5 from a generator seeded 102
  d<D>/eval/hutchinson/<dir>/seed, /first, /sum     torch.manual_seed(seed) precedes the call; the first draw (B, 4, D); sum of all draws
  main/sd0/<key>, main/noise_seed, main/step<s>/y, /z, /loss, main/sdN/<key>
                                      main.py's train_on_batch (Adam lr 1e-4, StepLR) for 2 steps, D = 2, dopri5; torch.manual_seed(
                                      noise_seed) once before the first step, the draws come from the CPU default generator
tests/golden/model_ffjord_noise_d<D>.npz:
  <solver>/fwd, /bwd                  (L, E, B, 1, D) float32: the draws of CNF i's forward integration / of its backward pass, evaluation order
"""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests._ref import load_reference  # noqa: E402

L, B = 2, 64
SOLVERS = ('midpoint', 'rk4', 'bosha3', 'dopri5')


def cfg_of(solver, trace='hutchinson'):
    return NS(layers=L, stepsize=0.1, t0=0.0, t1=1.0, solver=solver, trace=trace, backprop='adjoint')


def npy(t):
    return t.detach().cpu().numpy().copy()


def loss_of(z, ld):
    D = z.shape[1]
    mvn = torch.distributions.MultivariateNormal(torch.zeros(D), torch.eye(D))
    return -1.0 * torch.mean(mvn.log_prob(z) + ld)                 # main.py:85


class Recorder:
    """torch.randn, recording every draw while installed"""

    def __init__(self):
        self.orig, self.draws = torch.randn, []

    def __call__(self, *a, **k):
        t = self.orig(*a, **k)
        self.draws.append(t.clone())
        return t

    def __enter__(self):
        torch.randn = self
        return self

    def __exit__(self, *exc):
        torch.randn = self.orig
        return False


def per_layer(draws, reverse):
    """(L, E, B, S, D): the draws of one pass split by CNF layer (the backward pass visits the layers last to first)"""
    E = len(draws) // L
    assert E * L == len(draws)
    parts = [torch.stack(draws[i * E:(i + 1) * E]) for i in range(L)]
    return torch.stack(parts[::-1] if reverse else parts)


def main():
    ref = load_reference()
    if ref is None:
        sys.exit('reference not available: goldens can only be generated where the reference checkout exists')
    out = {}
    for D in (2, 3):
        noise = {}
        y = torch.randn(B, D, generator=torch.Generator().manual_seed(101)) * 0.5
        u = torch.randn(B, D, generator=torch.Generator().manual_seed(102)) * 0.5
        out['d%d/y' % D] = npy(y)
        for solver in SOLVERS:
            torch.manual_seed(100)
            net = ref.Ffjord((D, ), '2d', cfg_of(solver))
            if solver == SOLVERS[0]:
                for k, v in net.state_dict().items():
                    out['d%d/sd0/%s' % (D, k)] = npy(v)
            torch.manual_seed(200 + D)
            with Recorder() as rec:
                z, ld = net(y.clone())
            noise[solver + '/fwd'] = npy(per_layer(rec.draws, False))
            loss = loss_of(z, ld)
            with Recorder() as rec:
                loss.backward()
            noise[solver + '/bwd'] = npy(per_layer(rec.draws, True))
            p = 'd%d/%s/' % (D, solver)
            out[p + 'z'], out[p + 'ld'], out[p + 'loss'] = npy(z), npy(ld), npy(loss)
            for k, v in net.state_dict().items():
                if k.endswith('log_scale') or k.endswith('.bias') and 'func' not in k:
                    out[p + 'an/' + k] = npy(v)
            for k, q in net.named_parameters():
                out[p + 'grad/' + k] = npy(q.grad)
        path = os.path.join(HERE, 'model_ffjord_noise_d%d.npz' % D)
        np.savez_compressed(path, **noise)
        print('%s: %d arrays, %.1f KB' % (path, len(noise), os.path.getsize(path) / 1024))

        # evaluation mode on the state dopri5's training forward left (ActNorm initialised)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        for k, v in sd.items():
            out['d%d/eval/sd/%s' % (D, k)] = npy(v)
        for trace in ('exact', 'hutchinson'):
            net = ref.Ffjord((D, ), '2d', cfg_of('dopri5', trace))
            net.load_state_dict(sd)
            for m in net.net.layers:
                m.initialized = True
            net.eval()
            for direction, x in (('fwd', y), ('inv', u)):
                p = 'd%d/eval/%s/%s/' % (D, trace, direction)
                seed = 400 + 10 * D + (1 if direction == 'inv' else 0)
                torch.manual_seed(seed)
                with Recorder() as rec:
                    a, b = (net if direction == 'fwd' else net.backward)(x.clone())
                if direction == 'fwd':
                    out[p + 'z'], out[p + 'ld'] = npy(a), npy(b)
                else:
                    out[p + 'u'], out[p + 'x'], out[p + 'ld'] = npy(x), npy(a), npy(b)
                if trace == 'hutchinson':
                    out[p + 'seed'] = np.array(seed, dtype=np.int64)
                    out[p + 'first'] = npy(rec.draws[0])
                    out[p + 'sum'] = np.array(float(torch.stack(rec.draws).double().sum()), dtype=np.float64)
                else:
                    assert not rec.draws

    # main.py's train_on_batch (:78-92) with its optimizer set-up (:56-71, configs/default.yaml)
    torch.manual_seed(300)
    net = ref.Ffjord((2, ), '2d', cfg_of('dopri5'))
    for k, v in net.state_dict().items():
        out['main/sd0/' + k] = npy(v)
    optim = torch.optim.Adam(net.parameters(), lr=1.0e-4, betas=(0.9, 0.999), weight_decay=0.0)
    sched = torch.optim.lr_scheduler.StepLR(optim, step_size=10000, gamma=0.5)
    g = torch.Generator().manual_seed(301)
    out['main/noise_seed'] = np.array(302, dtype=np.int64)
    torch.manual_seed(302)
    for s in range(2):
        y = torch.randn(B, 2, generator=g) * 0.5
        z, ld = net(y.contiguous())
        loss = loss_of(z.view(B, -1), ld)
        optim.zero_grad()
        loss.backward()
        optim.step()
        sched.step()
        out['main/step%d/y' % s], out['main/step%d/z' % s], out['main/step%d/loss' % s] = npy(y), npy(z), npy(loss)
    for k, v in net.state_dict().items():
        out['main/sdN/' + k] = npy(v)
    path = os.path.join(HERE, 'model_ffjord.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %.1f KB' % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
