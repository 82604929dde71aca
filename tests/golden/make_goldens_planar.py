"""
Generates tests/golden/model_planar.npz by RUNNING THE UPSTREAM REFERENCE's planar flow (flows/planar.py, imported under the alias
``ref_flows``) on seeded inputs.  Data only: parameters, inputs, expected outputs and gradients.

    python tests/golden/make_goldens_planar.py          # only where the reference checkout exists

Keys (fp32):
  d<D>/sd0/<param>          the construction state_dict under torch.manual_seed(100), D = 2 and 3, K = 4 layers
  d<D>/y                    input batch (B = 64, randn * 0.5 from a generator seeded 101)
  d<D>/z, /ld, /loss        forward and main.py's loss (main.py:85)
  d<D>/grad/<param>         every parameter's gradient of that loss
  d<D>/x_inv, /ld_inv       net.backward(z) of the forward's z
  proj/sd0/<param>          D = 2 state whose layer 1 has w.u < -1 (u projected by the forward), proj/y, proj/z, proj/ld,
  proj/sd1/<param>          ... and the state after the forward (the projected u)
  main/sd0/<param>, main/step<s>/y, /z, /loss, main/sdN/<param>
                            main.py's train_on_batch (Adam lr 1e-4, StepLR) for 3 steps, D = 2, K = 4, B = 64
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

K, B = 4, 64


def npy(t):
    return t.detach().cpu().numpy().copy()


def loss_of(z, ld):
    D = z.shape[1]
    mvn = torch.distributions.MultivariateNormal(torch.zeros(D), torch.eye(D))
    return -1.0 * torch.mean(mvn.log_prob(z) + ld)                 # main.py:85


def main():
    ref = load_reference()
    if ref is None:
        sys.exit('reference not available: goldens can only be generated where the reference checkout exists')
    out = {}
    for D in (2, 3):
        torch.manual_seed(100)
        net = ref.PlanarFlow((D, ), '2d', NS(layers=K))
        for k, v in net.state_dict().items():
            out['d%d/sd0/%s' % (D, k)] = npy(v)
        y = torch.randn(B, D, generator=torch.Generator().manual_seed(101)) * 0.5
        z, ld = net(y.clone())
        loss = loss_of(z, ld)
        loss.backward()
        out['d%d/y' % D], out['d%d/z' % D], out['d%d/ld' % D], out['d%d/loss' % D] = npy(y), npy(z), npy(ld), npy(loss)
        for k, p in net.named_parameters():
            out['d%d/grad/%s' % (D, k)] = npy(p.grad)
        with torch.no_grad():
            x, ldi = net.backward(z.detach().clone())
        out['d%d/x_inv' % D], out['d%d/ld_inv' % D] = npy(x), npy(ldi)

    # a layer whose forward projects u (planar.py:27-33)
    torch.manual_seed(200)
    net = ref.PlanarFlow((2, ), '2d', NS(layers=K))
    with torch.no_grad():
        net.net.layers[1].w.copy_(torch.tensor([[0.8, -0.6]]))
        net.net.layers[1].u.copy_(torch.tensor([[-1.5, 0.7]]))     # w.u = -1.62
    for k, v in net.state_dict().items():
        out['proj/sd0/' + k] = npy(v)
    y = torch.randn(B, 2, generator=torch.Generator().manual_seed(201)) * 0.5
    z, ld = net(y.clone())
    out['proj/y'], out['proj/z'], out['proj/ld'] = npy(y), npy(z), npy(ld)
    for k, v in net.state_dict().items():
        out['proj/sd1/' + k] = npy(v)
    assert not np.array_equal(out['proj/sd1/net.layers.1.u'], out['proj/sd0/net.layers.1.u'])

    # main.py's train_on_batch (:78-92) with its optimizer set-up (:56-71, configs/default.yaml)
    torch.manual_seed(300)
    net = ref.PlanarFlow((2, ), '2d', NS(layers=K))
    for k, v in net.state_dict().items():
        out['main/sd0/' + k] = npy(v)
    optim = torch.optim.Adam(net.parameters(), lr=1.0e-4, betas=(0.9, 0.999), weight_decay=0.0)
    sched = torch.optim.lr_scheduler.StepLR(optim, step_size=10000, gamma=0.5)
    g = torch.Generator().manual_seed(301)
    for s in range(3):
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
    path = os.path.join(HERE, 'model_planar.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %.1f KB' % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
