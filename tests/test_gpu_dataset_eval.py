"""
Dequantised batches, the sweep schedule, the log-likelihood accumulator and FlowTrainer.evaluate on the GPU (csrc/dataset.hip, csrc/logp.hip)
against their numpy restatements (data.DeviceDataset.host_batch / indices / valid, held to their rules by tests/test_dataset_eval_host.py):
gathered batches are BIT-equal, noise included; the accumulator agrees with float64 numpy; evaluate agrees with log_py, repeats its bits and
leaves a captured training step working.  Needs a real MI355X.
"""
import importlib
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BADARG = 10001


def _data(pkg):
    return importlib.import_module(pkg.__name__ + '.data')


def _train(pkg):
    return importlib.import_module(pkg.__name__ + '.train')


def _every_byte(shape, seed=5):
    n_bytes = int(np.prod(shape))
    return (np.random.default_rng(seed).permutation(n_bytes) % 256).astype(np.uint8).reshape(shape)


def _check_step(ds):
    """one next() of ``ds`` against the host, at whatever step the device counter holds"""
    step = int(ds.step.item())
    ds.out.fill_(7.0)                                        # an unwritten pad ring or tail would keep the 7
    ds.last_indices.fill_(-1)
    out = ds.next()
    torch.cuda.synchronize()
    assert int(ds.step.item()) == step + 1
    idx = ds.indices(step)
    assert np.array_equal(ds.last_indices.cpu().numpy(), idx)
    want = ds.host_batch(step)
    assert out.shape == want.shape == (ds.batch, ) + ds.dims
    assert torch.equal(out.cpu(), want), 'step %d: %d elements differ' % (step, int((out.cpu() != want).sum()))
    return idx


# ---- 1. dequantised batches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,batch,pad', [((37, 5, 7, 3), 8, 0), ((37, 5, 7, 3), 8, 3),         # byte-load path, 105 bytes per sample
                                              ((300, 32, 32, 3), 64, 0),                            # 16-byte path, four slices
                                              ((300, 28, 28), 64, 2),                               # MNIST shape
                                              ((600, 8, 8, 3), 512, 0),                             # two slices
                                              ((1100, 7, 8, 3), 1024, 1)])                          # one slice
def test_dequantised_batches_are_bit_equal(pkg, shape, batch, pad):
    D = _data(pkg)
    arr = _every_byte(shape)
    ds = D.DeviceDataset(arr, batch, pad=pad, seed=3, device=DEV, dequantize=True)
    for _ in range(ds.steps_per_epoch + 1):                  # across the epoch boundary
        _check_step(ds)
    x = ds.out.cpu()
    inner = x[:, :, pad:pad + shape[1], pad:pad + shape[2]]
    assert bool((inner > 0).all()) and bool((inner < 1).all())
    v = arr.reshape(arr.shape + (1, ))[ds.indices(ds.steps_per_epoch)] if arr.ndim == 3 else arr[ds.indices(ds.steps_per_epoch)]
    assert np.array_equal(np.floor(inner.numpy().astype(np.float64) * 256.0), np.transpose(v, (0, 3, 1, 2)))
    if shape[0] == 37 and pad == 0:
        ds.step.fill_((1 << 33) + 5)                         # the step's high word is part of the noise counter and of the epoch
        _check_step(ds)
        assert not torch.equal(ds.host_batch((1 << 33) + 5), ds.host_batch(5))


def test_plain_entry_points_are_what_they_were(pkg):
    """dequant = 0, sweep = 0 through the extended entry point: the bits of nf_dataset_gather_u8"""
    D, N = _data(pkg), pkg._native
    arr = _every_byte((300, 32, 32, 3))
    ds = D.DeviceDataset(arr, 64, seed=3, device=DEV)
    want = ds.next().clone()
    out = torch.full_like(want, 7.0)
    N.call('nf_dataset_gather_u8_x', ds.data.data_ptr(), out.data_ptr(), 300, 32, 32, 3, 0, 64, 64, 0, ds.steps_per_epoch, ds.seed, 1, 0, 0,
           None, None, N.stream())
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(want.cpu(), ds.host_batch(0))


# ---- 2. sweep batches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shuffle', [False, True])
@pytest.mark.parametrize('n', [37, 5])
@pytest.mark.parametrize('kind', ['image', 'image_dq', 2, 3, 5])
def test_sweep_batches(pkg, kind, n, shuffle):
    D = _data(pkg)
    if isinstance(kind, int):
        src = np.random.default_rng(kind).normal(size=(n, kind)).astype(np.float32)
        ds = D.DeviceDataset(src, 8, seed=8, shuffle=shuffle, device=DEV, sweep=True)
    else:
        src = _every_byte((n, 5, 7, 3))
        ds = D.DeviceDataset(src, 8, pad=1, seed=8, shuffle=shuffle, device=DEV, sweep=True, dequantize=kind == 'image_dq')
    S = ds.steps_per_epoch
    assert S == -(-n // 8)
    for p in range(2):                                       # the counter wraps to a second pass
        served = []
        for k in range(S):
            idx, v = _check_step(ds), ds.valid(p * S + k)
            assert (idx[v:] == n - 1).all()
            if v < 8:                                        # the tail rows hold sample N - 1
                tail = ds.out[v:].cpu()
                assert torch.equal(tail, tail[:1].expand_as(tail))
                if isinstance(kind, int):
                    assert np.array_equal(tail[0].numpy(), src[n - 1])
            served.append(idx[:v])
        assert np.array_equal(np.sort(np.concatenate(served)), np.arange(n))


# ---- 3. bad arguments -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(pkg):
    N = pkg._native
    lib = N.load()
    data8 = torch.zeros((100, 4, 4, 3), dtype=torch.uint8, device=DEV)
    dataf = torch.zeros((100, 2), dtype=torch.float32, device=DEV)
    out = torch.full((8, 3, 4, 4), 7.0, device=DEV)
    idx = torch.full((8, ), -1, dtype=torch.int64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)

    def u8(data=data8.data_ptr(), o=out.data_ptr(), N_=100, B=8, stride=8, offset=0, E=13, dq=1, sweep=1):
        return lib.nf_dataset_gather_u8_x(data, o, N_, 4, 4, 3, 0, B, stride, offset, E, 1, 1, dq, sweep, step.data_ptr(), idx.data_ptr(),
                                          N.stream())

    def f32(data=dataf.data_ptr(), o=out.data_ptr(), N_=100, B=8, stride=8, offset=0, E=13, sweep=1):
        return lib.nf_dataset_gather_f32_x(data, o, N_, 2, B, stride, offset, E, 1, 1, sweep, step.data_ptr(), idx.data_ptr(), N.stream())
    for kw in (dict(data=None), dict(o=None), dict(N_=0), dict(N_=-3), dict(N_=1 << 31), dict(B=0), dict(E=0), dict(E=14),
               dict(stride=16, offset=9, E=7), dict(offset=-1), dict(sweep=2), dict(sweep=-1), dict(sweep=0)):   # (E = 13 > 99 / 8 on the loader's)
        assert u8(**kw) == BADARG, kw
        assert f32(**kw) == BADARG, kw
    for kw in (dict(dq=2), dict(dq=-1)):
        assert u8(**kw) == BADARG, kw
    z = torch.zeros((8, 2), device=DEV)
    ld = torch.zeros(8, device=DEV)
    row = torch.full((8, ), 7.0, dtype=torch.float64, device=DEV)
    acc = torch.full((3, ), 7.0, dtype=torch.float64, device=DEV)

    def lp(z_=z.data_ptr(), ld_=ld.data_ptr(), row_=row.data_ptr(), acc_=acc.data_ptr(), B=8, D_=2, N_=100, stride=8, offset=0):
        return lib.nf_logp_accumulate(z_, ld_, row_, None, None, acc_, B, D_, N_, stride, offset, step.data_ptr(), N.stream())
    for kw in (dict(z_=None), dict(ld_=None), dict(row_=None), dict(acc_=None), dict(B=0), dict(D_=0), dict(N_=0), dict(stride=0),
               dict(stride=16, offset=9), dict(offset=-1), dict(N_=1 << 31), dict(stride=1 << 31)):
        assert lp(**kw) == BADARG, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((idx == -1).all()) and bool((row == 7.0).all()) and bool((acc == 7.0).all())
    assert u8() == 0 and f32() == 0 and lp() == 0             # the defaults of this test are valid calls
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        _data(pkg).DeviceDataset(np.zeros((96, 2), dtype=np.float32), 96, device=DEV, dequantize=True)


# ---- 4. accumulator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,D_', [(b, d) for b in (1, 63, 64, 65, 4097) for d in (2, 3, 5)] + [(65, 3072)])
def test_logp_accumulator(pkg, B, D_):
    """random z; ld = normal - 3, so that log p <= -1/2 D log 2 pi - 3 + max(normal) < -1 has no cancellation and a RELATIVE bound on a row
    means something.  Float64 rows and sums within 1e-12 relative (summation order in float64: <= n * 2^-53 ~ 5e-13 at n = 4097 + 3 D
    terms), the float32 copy within one rounding of the float64 value."""
    N = pkg._native
    rng = np.random.default_rng(B * 31 + D_)
    n_set = 2 * B + B // 3 if B > 1 else 2                   # stride = B: steps 0, 1 full, step 2 holds B // 3 rows (B = 1: step 2 wraps to 0)
    S = -(-n_set // B)
    z = rng.normal(size=(3, B, D_)).astype(np.float32)
    ld = (rng.normal(size=(3, B)) - 3.0).astype(np.float32)
    valid = [int(min(max(n_set - (s % S) * B, 0), B)) for s in range(3)]
    assert valid[0] == B and (B == 1 or valid[2] == B // 3)
    for s in range(3):
        z[s, valid[s]:] = np.inf                             # rows at and beyond `valid` must not count
    want_rows = -0.5 * (z.astype(np.float64) ** 2).sum(axis=2) - 0.5 * D_ * math.log(2.0 * math.pi) + ld.astype(np.float64)
    good = [want_rows[s, :valid[s]] for s in range(3)]
    want_acc = np.array([sum(g.sum() for g in good), sum((g * g).sum() for g in good), float(sum(valid))])
    zd, ldd = torch.from_numpy(z).to(DEV), torch.from_numpy(ld).to(DEV)

    def run():
        acc = torch.zeros(3, dtype=torch.float64, device=DEV)
        rows = torch.zeros((3, B), dtype=torch.float64, device=DEV)
        rows32 = torch.zeros((3, B), dtype=torch.float32, device=DEV)
        rows_all = torch.zeros(S * B, dtype=torch.float64, device=DEV)
        step = torch.zeros(1, dtype=torch.int64, device=DEV)
        parts = []
        for s in range(3):
            N.call('nf_logp_accumulate', zd[s].data_ptr(), ldd[s].data_ptr(), rows[s].data_ptr(), rows32[s].data_ptr(), rows_all.data_ptr(),
                   acc.data_ptr(), B, D_, n_set, B, 0, step.data_ptr(), N.stream())
            N.call('nf_sample_advance', step.data_ptr(), N.stream())
            parts.append(acc.clone())
        torch.cuda.synchronize()
        return acc.cpu().numpy(), rows.cpu().numpy(), rows32.cpu().numpy(), rows_all.cpu().numpy().reshape(S, B), [p.cpu().numpy() for p in parts]

    acc, rows, rows32, rows_all, parts = run()
    assert acc[2] == sum(valid) and np.isfinite(acc).all()
    assert np.all(np.abs(acc - want_acc) <= 1e-12 * np.abs(want_acc)), (acc, want_acc)
    for s in range(3):
        g, w = rows[s, :valid[s]], good[s]
        assert np.all(np.abs(g - w) <= 1e-12 * np.abs(w))
        assert np.all(np.abs(rows32[s, :valid[s]].astype(np.float64) - w) <= 2.0 ** -23 * np.abs(w))
        assert np.all(np.isneginf(rows[s, valid[s]:]))       # computed, filed, never summed
    filed = {s % S: rows[s] for s in range(3)}               # rows_all[(step % S) * B + j]: the last writer of a slot stays
    for k, r in filed.items():
        assert np.array_equal(rows_all[k], r)
    # three accumulating calls equal the sum of three: each call adds its own step's sums to what the accumulator held
    one = [np.array([good[s].sum(), (good[s] * good[s]).sum(), float(valid[s])]) for s in range(3)]
    prev = np.zeros(3)
    for s in range(3):
        assert np.all(np.abs((parts[s] - prev) - one[s]) <= 1e-12 * np.abs(want_acc) + 1e-300)
        prev = parts[s]
    again = run()
    assert acc.tobytes() == again[0].tobytes() and rows.tobytes() == again[1].tobytes() and rows32.tobytes() == again[2].tobytes()
    was = N.deterministic()
    try:
        N.deterministic(True)
        det = run()
        N.deterministic(False)
        fast = run()
    finally:
        N.deterministic(was)
    for other in (det, fast):
        assert acc.tobytes() == other[0].tobytes() and rows.tobytes() == other[1].tobytes() and rows32.tobytes() == other[2].tobytes()


# ---- 5. - 7. evaluate -----------------------------------------------------------------------------------------------------------------
def _close(a, b):
    """the project's op tolerance: 1e-5 * max(1, |value|)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= 1e-5 * np.maximum(1.0, np.abs(b))))


def _evaluate_checks(pkg, trainer, ev, n, want_rows):
    N = pkg._native
    res = trainer.evaluate(ev, keep_rows=True)
    rows = res['rows'].numpy()
    assert res['n'] == n and rows.shape == (n, ) and rows.dtype == np.float64
    assert abs(res['nll'] + rows.mean()) <= 1e-12 * abs(rows.mean())
    assert res['stderr'] > 0 and abs(res['stderr'] - rows.std(ddof=1) / math.sqrt(n)) <= 1e-6 * res['stderr']
    assert abs(res['bits_per_dim'] - res['nll'] / (np.prod(ev.dims) * math.log(2.0))) < 1e-12
    for name, want in want_rows.items():
        diff = np.abs(rows - want) / np.maximum(1.0, np.abs(want))
        print('evaluate rows against %s: max scaled difference %.3e' % (name, diff.max()))
        assert _close(rows, want), name
    again = trainer.evaluate(ev, keep_rows=True)
    assert again['rows'].numpy().tobytes() == rows.tobytes() and again['nll'] == res['nll'] and again['stderr'] == res['stderr']
    plain = trainer.evaluate(ev)
    assert 'rows' not in plain and plain['nll'] == res['nll'] and plain['n'] == n
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='hipGraph capture of the evaluation step failed')    # a fall-back to eager is a failure here
        g = trainer.evaluate(ev, graph=True, keep_rows=True)
    assert g['n'] == n and _close(g['rows'].numpy(), rows) and _close(g['nll'], res['nll'])
    was = N.deterministic()
    try:
        N.deterministic(True)
        d_eager = trainer.evaluate(ev, keep_rows=True)
        d_graph = trainer.evaluate(ev, graph=True, keep_rows=True)
    finally:
        N.deterministic(was)
    assert d_graph['rows'].numpy().tobytes() == d_eager['rows'].numpy().tobytes() and d_graph['nll'] == d_eager['nll']
    assert not trainer.net.training
    return res


def test_evaluate_vector_model(pkg):
    D, T = _data(pkg), _train(pkg)
    torch.manual_seed(0)
    rows = D.moons(1000, np.random.default_rng(1))
    net = pkg.RealNVP((2, ), '2d', NS(layers=4, mixtures=None)).to(DEV)
    ds = D.DeviceDataset(rows, 96, seed=1, device=DEV)
    trainer = T.FlowTrainer(net, sampler=ds)
    for _ in range(4):                                       # every data-dependent initialisation has happened
        trainer.train_on_batch()
    ev = ds.sweep_view()
    assert ev.steps_per_epoch == 11 and ev.valid(10) == 40 and ev.data.data_ptr() == ds.data.data_ptr()
    y = torch.from_numpy(rows).to(DEV)
    want = {'log_py, one batch': trainer.log_py(y).double().cpu().numpy(),
            'log_py, batches of 250': torch.cat([trainer.log_py(y[i:i + 250]) for i in range(0, 1000, 250)]).double().cpu().numpy()}
    res = _evaluate_checks(pkg, trainer, ev, 1000, want)
    assert 'bits_per_dim_pixel' not in res
    with pytest.raises(ValueError, match='sweep_view'):
        trainer.evaluate(ds)
    z, loss = trainer.train_on_batch()
    assert net.training and bool(torch.isfinite(loss))


@pytest.fixture(scope='module')
def glow_set():
    return np.random.default_rng(4).integers(0, 256, size=(70, 32, 32, 3), dtype=np.uint8)


def test_evaluate_image_model(pkg, glow_set):
    D, T = _data(pkg), _train(pkg)
    torch.manual_seed(0)
    net = pkg.Glow((3, 32, 32), 'image', NS(layers=2, mixtures=None)).to(DEV)
    ds = D.DeviceDataset(glow_set, 32, seed=1, device=DEV, dequantize=True)
    trainer = T.FlowTrainer(net, sampler=ds)
    for _ in range(4):
        trainer.train_on_batch()
    ev = ds.sweep_view()
    assert ev.data.data_ptr() == ds.data.data_ptr() and ev.dequantize and ev.steps_per_epoch == 3 and ev.valid(2) == 6
    want = torch.cat([trainer.log_py(ev.host_batch(s).to(DEV))[:ev.valid(s)] for s in range(3)]).double().cpu().numpy()
    res = _evaluate_checks(pkg, trainer, ev, 70, {'log_py(host_batch(step))': want})
    assert abs(res['bits_per_dim_pixel'] - res['bits_per_dim'] - 8.0) < 1e-12
    assert int(ds.step.item()) == 4                          # the view has its own step counter


def test_captured_training_on_dequantised_batches(pkg, glow_set):
    D, T = _data(pkg), _train(pkg)
    torch.manual_seed(0)
    net = pkg.Glow((3, 32, 32), 'image', NS(layers=2, mixtures=None)).to(DEV)
    ds = D.DeviceDataset(glow_set, 32, seed=1, shuffle=False, device=DEV, dequantize=True)
    trainer = T.FlowTrainer(net, graph=True, warmup=2, sampler=ds)
    for _ in range(3):                                       # two eager steps, then the capture (with its extra step) and a first replay
        trainer.train_on_batch()
    assert trainer._g_fb is not None
    losses, outs = [], []
    for _ in range(3):
        z, loss = trainer.train_on_batch()
        torch.cuda.synchronize()
        step = int(ds.step.item()) - 1
        assert torch.equal(ds.out.cpu(), ds.host_batch(step)), 'batch of step %d' % step     # fresh noise, the same floor, no host work
        outs.append(ds.out.clone())
        losses.append(float(loss))
    assert not torch.equal(outs[0], outs[2])                 # steps two apart: the same samples (E = 2), other noise
    assert torch.equal(torch.floor(outs[0] * 256), torch.floor(outs[2] * 256))
    res = trainer.evaluate(ds.sweep_view())
    assert res['n'] == 70 and math.isfinite(res['nll']) and not net.training
    z, loss = trainer.train_on_batch()                       # the captured step goes on; the model is back in training mode
    assert net.training and trainer._g_fb is not None
    losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses)
