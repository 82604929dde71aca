"""What the fused-optimizer tests on the device share (tests/test_gpu_optim.py, test_gpu_trainer_guard.py, test_gpu_optim_recipes.py,
test_gpu_optim_entries.py): the project's optimizer bar, 2e-6 + 2e-6 |x| per entry, and parameters in a flat bucket beside their clones
for torch.optim, fed the same gradient."""
import torch

DEV = 'cuda'
SPECIAL = [0.0, 1e-12, -1e-9, 1e-6, 3e4]


def _close(a, b, what):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    assert bool(torch.isfinite(a).all()), what
    ratio = float(((a - b).abs() / (2e-6 + 2e-6 * b.abs())).max())
    print('%s: %.3f of the bar' % (what, ratio))
    assert ratio <= 1.0, '%s: %.3f of the bar 2e-6 + 2e-6 |x|' % (what, ratio)


def _pair(mods, shapes, seed=0):
    """parameters in a flat bucket and their clones for torch.optim; mods = (the train module, the dist module)"""
    _, nfdist = mods
    g = torch.Generator(device=DEV).manual_seed(seed)
    pa = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=g)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    return pa, pb, nfdist.GradBucket(pa, flatten_params=True), g


def _feed(bucket, pb, flat):
    """the same gradient into the bucket and into the clones' .grad"""
    bucket.flat.copy_(flat)
    o = 0
    for b in pb:
        b.grad = flat[o:o + b.numel()].view_as(b).clone()
        o += b.numel()


def _fresh(bucket, g, special=False):
    flat = torch.randn(bucket.numel, device=DEV, generator=g)
    if special:
        flat[:len(SPECIAL)] = torch.tensor(SPECIAL, device=DEV)
    return flat
