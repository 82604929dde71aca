"""
Seeded synthetic inputs of the benchmark configurations.  The reference's data code (flows/dataset.py) needs
hydra / torchvision / sklearn tables and cannot travel; these are numpy restatements of the same distributions that
take the sample count ``n`` directly (flows/dataset.py:13-50; sklearn.datasets.make_moons / make_circles / make_swiss_roll /
make_s_curve geometry).
"""
import numpy as np
import torch


def moons(n, rng, noise=0.08):
    """two interleaving half circles + gaussian noise, then (x - 0.5) / 2   (dataset.py:18-21)"""
    n_out = n // 2
    n_in = n - n_out
    t_out = np.linspace(0.0, np.pi, n_out)
    t_in = np.linspace(0.0, np.pi, n_in)
    x = np.concatenate([np.cos(t_out), 1.0 - np.cos(t_in)])
    y = np.concatenate([np.sin(t_out), 1.0 - np.sin(t_in) - 0.5])
    pts = np.stack([x, y], axis=1)
    pts = pts[rng.permutation(n)]
    pts = pts + rng.normal(scale=noise, size=pts.shape)
    return ((pts - 0.5) / 2.0).astype(np.float32)


def circles(n, rng, noise=0.08, factor=0.5):
    """two concentric circles (radii 1 and `factor`) + noise, scaled by 0.6   (dataset.py:13-15)"""
    n_out = n // 2
    n_in = n - n_out
    t_out = np.linspace(0.0, 2.0 * np.pi, n_out, endpoint=False)
    t_in = np.linspace(0.0, 2.0 * np.pi, n_in, endpoint=False)
    x = np.concatenate([np.cos(t_out), np.cos(t_in) * factor])
    y = np.concatenate([np.sin(t_out), np.sin(t_in) * factor])
    pts = np.stack([x, y], axis=1)
    pts = pts[rng.permutation(n)]
    pts = pts + rng.normal(scale=noise, size=pts.shape)
    return (pts * 0.6).astype(np.float32)


def normals(n, rng, radius=0.7, n_normals=8):
    """8 gaussians (sigma 0.1) on a circle of radius 0.7   (dataset.py:24-34)"""
    k = rng.integers(n_normals, size=(n, ))
    cx = radius * np.cos(2.0 * np.pi * k / n_normals)
    cy = radius * np.sin(2.0 * np.pi * k / n_normals)
    d = rng.normal(size=(2, n)) * 0.1
    return np.stack([cx + d[0], cy + d[1]], axis=1).astype(np.float32)


def cifar_like(n, rng, dims=(3, 32, 32)):
    """uniform uint8 pixels / 255 (the reference feeds uint8/255 without dequantisation noise, dataset.py:120)"""
    return (rng.integers(0, 256, size=(n, ) + tuple(dims), dtype=np.uint8).astype(np.float32) / 255.0)


def swiss(n, rng, noise=0.08):
    """sklearn make_swiss_roll: t = 1.5 pi (1 + 2u), (t cos t, 21 u2, t sin t) + gaussian noise, then x * 0.07, y * 0.07 - 1,
    z * 0.07   (dataset.py:37-42)"""
    t = 1.5 * np.pi * (1.0 + 2.0 * rng.random(n))
    pts = np.stack([t * np.cos(t), 21.0 * rng.random(n), t * np.sin(t)], axis=1)
    pts = pts + rng.normal(scale=noise, size=pts.shape)
    return (pts * 0.07 - np.array([0.0, 1.0, 0.0])).astype(np.float32)


def s_curve(n, rng, noise=0.08):
    """sklearn make_s_curve: t = 3 pi (u - 1/2), (sin t, 2 u2, sign(t) (cos t - 1)) + gaussian noise, then x * 0.7, (y - 1) * 0.7,
    z * 0.35   (dataset.py:45-50)"""
    t = 3.0 * np.pi * (rng.random(n) - 0.5)
    pts = np.stack([np.sin(t), 2.0 * rng.random(n), np.sign(t) * (np.cos(t) - 1.0)], axis=1)
    pts = pts + rng.normal(scale=noise, size=pts.shape)
    return ((pts - np.array([0.0, 1.0, 0.0])) * np.array([0.7, 0.7, 0.35])).astype(np.float32)


GENERATORS = {'moons': moons, 'circles': circles, 'normals': normals, 'cifar': cifar_like, 'swiss': swiss, 's_curve': s_curve}


def sample(name, n, seed):
    return torch.from_numpy(GENERATORS[name](n, np.random.default_rng(seed)))


# ---- on-device generation (csrc/datagen.hip): same distributions, drawn where they are consumed --------------------------------------
KINDS = {'moons': 0, 'circles': 1, 'normals': 2, 'cifar': 3, 'swiss': 4, 's_curve': 5}


class DeviceSampler:
    """A stream of synthetic batches generated ON the GPU: ``next()`` fills (and returns) one static tensor with a fresh batch.
    The step counter lives in device memory and the draw is a pure function of (seed, step, sample index), so the two launches
    can be captured into a hipGraph (FlowTrainer(sampler=...)): every replay trains on a new batch without any host-to-device
    copy -- the reference copies each batch from the host (main.py:79).

    ``rank``: under data parallelism every replica must draw a DIFFERENT shard of the global batch; the rank (default: the
    process group's, 0 without one) is folded into the Philox key, so W replicas built with the same seed see W distinct
    streams and the effective global batch is B * W."""

    def __init__(self, name, batch, dims, seed=0, device='cuda', rank=None):
        import torch as _t
        from . import _native as N
        self._N = N
        self.kind = KINDS[name]
        self.batch = int(batch)
        self.dims = tuple(dims)
        per = 1
        for d_ in self.dims:
            per *= int(d_)
        if self.kind in (4, 5):
            if self.dims != (3, ):
                raise ValueError('%s is a 3-D data set' % name)
        elif self.kind != 3 and per != 2:
            raise ValueError('%s is a 2-D data set' % name)
        self.per = per
        if rank is None:
            import torch.distributed as _d
            rank = _d.get_rank() if _d.is_available() and _d.is_initialized() else 0
        self.rank = int(rank)
        self.seed = (int(seed) ^ (self.rank * 0x9E3779B97F4A7C15)) & 0x7FFFFFFFFFFFFFFF    # 63-bit key, distinct per rank
        self.out = _t.empty((self.batch, ) + self.dims, dtype=_t.float32, device=device)
        self.step = _t.zeros(1, dtype=_t.int64, device=device)

    def next(self):
        N = self._N
        N.call('nf_sample_data', self.kind, self.out.data_ptr(), self.batch, self.per, self.seed, self.step.data_ptr(), N.stream())
        N.call('nf_sample_advance', self.step.data_ptr(), N.stream())
        return self.out


# ---- device-resident data sets (csrc/dataset.hip): the reference loader's batch sequence, gathered where it is consumed ---------------
N_DATASET_SIZE = 65536          # dataset.py:10: the fixed size of the reference's toy sets
DS_ROUNDS = 8                   # Feistel rounds (csrc/dataset.hip NF_DS_ROUNDS)
DS_WALK = 155                   # bound of the cycle walk: (3/4)^155 < 2^-64 (NF_DS_WALK); beyond it the position itself is served
DS_KEY = 0x510e527f             # key constant that sets the permutation's Philox stream apart (NF_DS_KEY)


DQ_KEY = 0x9b05688c             # key constant of the dequantisation noise's Philox stream (NF_DQ_KEY)


def _philox_words(c0, c1, c2, c3, k0, k1):
    """the four words of Philox4x32-10 (csrc/nf_philox.h) on uint64 arrays / scalars holding 32-bit words"""
    M0, M1, W0, W1, m32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85, np.uint64(0xFFFFFFFF)
    shape = np.broadcast(*(np.asarray(c) for c in (c0, c1, c2, c3))).shape
    c0, c1, c2, c3 = (np.broadcast_to(np.asarray(c, dtype=np.uint64), shape) for c in (c0, c1, c2, c3))
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2
        ka, kb = np.uint64((k0 + r * W0) & 0xFFFFFFFF), np.uint64((k1 + r * W1) & 0xFFFFFFFF)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ ka, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ kb, p0 & m32
    return c0, c1, c2, c3


def _philox_word0(c0, c1, c2, c3, k0, k1):
    """word 0 of Philox4x32-10 (csrc/nf_philox.h) on uint64 arrays / scalars holding 32-bit words"""
    return _philox_words(c0, c1, c2, c3, k0, k1)[0]


def dequant_words(seed, step, idx, n_bytes):
    """the 32-bit noise words of the dequantising gather (csrc/dataset.hip, the DQ arm), uint32 of shape ``idx.shape + (n_bytes, )``:
    byte b of data-set sample idx at device step ``step`` gets word b & 3 of Philox4x32-10(counter (b >> 2, idx, step lo, step hi),
    key (seed lo, seed hi ^ DQ_KEY)); its top 15 bits are the noise below the byte.  ``seed`` as DeviceDataset stores it."""
    seed, step, n_bytes = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(n_bytes)
    idx = np.asarray(idx, dtype=np.int64)
    quads = np.arange((n_bytes + 3) // 4, dtype=np.uint64)
    w = _philox_words(quads, idx.astype(np.uint64)[..., None], step & 0xFFFFFFFF, step >> 32, seed & 0xFFFFFFFF, (seed >> 32) ^ DQ_KEY)
    return np.stack(w, axis=-1).reshape(idx.shape + (-1, ))[..., :n_bytes].astype(np.uint32)


def dataset_perm(seed, epoch, pos, N, rounds=DS_ROUNDS):
    """index in [0, N) served at position ``pos`` of pass ``epoch`` (ints, or arrays that broadcast): for every (seed, epoch) a bijection
    of [0, N).
    A balanced Feistel network over 2h bits, h = max(1, ceil(bits(N - 1) / 2)): (L, R) -> (R, L ^ F(R, round)) with F = word 0 of
    Philox4x32-10(counter (R, round, epoch lo, epoch hi), key (seed lo, seed hi ^ DS_KEY)) masked to h bits, applied again while the
    result is >= N (cycle walking, at most DS_WALK further times).  Integers only: the same function as nf_ds_index of
    csrc/dataset.hip, bit for bit.  ``rounds`` exists for the tests that tell 8 rounds from fewer."""
    N = int(N)
    if not 0 < N < 1 << 31:
        raise ValueError('dataset_perm: N must lie in [1, 2^31), got %d' % N)
    pos = np.asarray(pos, dtype=np.int64)
    if pos.size and (pos.min() < 0 or pos.max() >= N):
        raise ValueError('dataset_perm: positions must lie in [0, N)')
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    epoch = np.asarray(epoch).astype(np.uint64) if isinstance(epoch, np.ndarray) else np.uint64(int(epoch) & 0xFFFFFFFFFFFFFFFF)
    shape = np.broadcast(pos, epoch).shape
    start = np.broadcast_to(pos, shape).astype(np.uint64).reshape(-1)
    epoch = np.broadcast_to(epoch, shape).reshape(-1)
    bits = (N - 1).bit_length()
    h = 1 if bits < 2 else (bits + 1) // 2
    mask, hh = np.uint64((1 << h) - 1), np.uint64(h)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) ^ DS_KEY

    def feistel(x, e):
        L, R, e_lo, e_hi = x >> hh, x & mask, e & np.uint64(0xFFFFFFFF), e >> np.uint64(32)
        for r in range(rounds):
            L, R = R, L ^ (_philox_word0(R, r, e_lo, e_hi, k0, k1) & mask)
        return (L << hh) | R
    x = feistel(start, epoch)
    for _ in range(DS_WALK):
        out = np.nonzero(x >= np.uint64(N))[0]
        if out.size == 0:
            break
        x[out] = feistel(x[out], epoch[out])
    x = np.where(x >= np.uint64(N), start, x)
    return x.astype(np.int64).reshape(shape)


class DeviceDataset:
    """A data set held in DEVICE memory that serves the reference loader's batch sequence (flows/dataset.py:53-127) with no host work
    per step: ``next()`` gathers this rank's batch of the current step into one static tensor and advances the step, two launches that
    a hipGraph can capture (FlowTrainer(sampler=...)); a replay walks through the batches and the epochs by itself.

    ``source``  uint8 (N, H, W) or (N, H, W, C), array or tensor: the image form -- out (B, C, H + 2 pad, W + 2 pad) = uint8 / 255, HWC ->
                CHW, a zero ring of ``pad`` pixels (MNIST: pad = 2), dims = (C, H + 2 pad, W + 2 pad), dtype 'image' (dataset.py:67-79,
                :119-122);  float32 (N, D): the row form -- out (B, D), dims = (D, ), dtype '2d' / '3d' (dataset.py:80-99, :124-125).
                Uploaded once.
    Schedule    dataset.py:111-117: a pass has steps_per_epoch = (N - 1) // (world * batch) steps (the tail is dropped, and the last full
                batch where world * batch divides N); step s is step s % E of pass s // E; rank r takes positions
                k * world * batch + r * batch + j of the pass's order, so the ranks of one step hold disjoint samples of ONE permutation
                (the rank is not folded into the seed).  N <= world * batch is refused.
    Order       ``shuffle``: index = dataset_perm(seed, pass, position), evaluated in the gather kernel -- no index array, no reshuffle
                launch (the reference: np.random.shuffle per pass); otherwise the identity.
    ``device``  None builds a host-only object: ``indices`` / ``host_batch`` work, ``next()`` does not.
    ``dequantize``  images only, off by default (the reference feeds uint8 / 255, dataset.py:120): out = (v + u) / 256 with 15 bits of
                uniform noise u drawn in the gather kernel -- ((v * 2^15 + (w >> 17)) + 0.5) * 2^-23, w = dequant_words(seed, step, index,
                bytes): strictly inside (0, 1), floor(256 x) == v, a pure function of (seed, step, sample, byte), so a captured step draws
                fresh noise on every replay and ``host_batch(step)`` restates it bit for bit.  The pad ring stays 0.
    ``sweep``   the schedule of a held-out score (FlowTrainer.evaluate): steps_per_epoch = ceil(N / (world * batch)), every sample is
                served exactly once per pass; a position >= N is served sample N - 1 and is not valid (``valid(step)`` counts the real
                rows).  N <= world * batch is allowed.  ``sweep_view()`` builds such a set over the device copy of this one."""

    def __init__(self, source, batch, pad=0, seed=0, shuffle=True, device='cuda', rank=None, world=None, dequantize=False, sweep=False,
                 _share=None):
        arr = source.detach().cpu().numpy() if isinstance(source, torch.Tensor) else np.asarray(source)
        if arr.dtype == np.uint8 and arr.ndim in (3, 4):
            arr = arr.reshape(arr.shape + (1, )) if arr.ndim == 3 else arr
            self.image = True
        elif arr.dtype == np.float32 and arr.ndim == 2:
            self.image = False
        else:
            raise ValueError('DeviceDataset takes uint8 (N, H, W[, C]) images or float32 (N, D) rows, got %s %s' % (arr.dtype, arr.shape))
        if min(arr.shape) < 1:
            raise ValueError('DeviceDataset: empty source %s' % (arr.shape, ))
        self.host = np.ascontiguousarray(arr)
        self.n, self.batch, self.pad = int(arr.shape[0]), int(batch), int(pad)
        if self.pad < 0 or (self.pad and not self.image):
            raise ValueError('pad is a non-negative ring of pixels around images')
        if rank is None or world is None:
            import torch.distributed as _d
            on = _d.is_available() and _d.is_initialized()
            rank = (_d.get_rank() if on else 0) if rank is None else rank
            world = (_d.get_world_size() if on else 1) if world is None else world
        self.rank, self.world = int(rank), int(world)
        if self.batch < 1 or self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError('DeviceDataset: batch %d, rank %d of %d' % (self.batch, self.rank, self.world))
        self.stride, self.offset = self.world * self.batch, self.rank * self.batch
        if self.n >= 1 << 31:
            raise ValueError('DeviceDataset holds fewer than 2^31 samples')
        self.dequantize, self.sweep = bool(dequantize), bool(sweep)
        if self.dequantize and not self.image:
            raise ValueError('dequantize=True is for uint8 images: float32 rows hold no quantisation step to fill')
        if self.sweep:
            if self.stride >= 1 << 31:
                raise ValueError('DeviceDataset(sweep=True): world * batch must stay below 2^31')
            self.steps_per_epoch = -(-self.n // self.stride)
        else:
            if self.n <= self.stride:
                raise ValueError('a data set of %d samples serves no batch of %d x %d: the loader needs N > world * batch (dataset.py:113)'
                                 % (self.n, self.world, self.batch))
            self.steps_per_epoch = (self.n - 1) // self.stride
        self.seed, self.shuffle = int(seed) & 0x7FFFFFFFFFFFFFFF, bool(shuffle)
        if self.image:
            _, H, W, C = arr.shape
            self.dims, self.dtype = (C, H + 2 * self.pad, W + 2 * self.pad), 'image'
        else:
            self.dims, self.dtype = (int(arr.shape[1]), ), '%dd' % arr.shape[1]
        self.data = self.out = self.step = self.last_indices = None
        if _share is not None:                               # sweep_view(): the parent's device copy, no second upload
            device = _share.device
        if device is not None:
            from . import _native as N
            self._N = N
            self.data = _share if _share is not None else torch.from_numpy(self.host).to(device)
            self.out = torch.empty((self.batch, ) + self.dims, dtype=torch.float32, device=device)
            self.step = torch.zeros(1, dtype=torch.int64, device=device)
            self.last_indices = torch.zeros(self.batch, dtype=torch.int64, device=device)

    @classmethod
    def toy(cls, name, batch, seed=0, n=N_DATASET_SIZE, **kw):
        """the reference's fixed toy set of N_DATASET_SIZE points (dataset.py:10-50, :80-99), built ONCE from data.GENERATORS[name] --
        the reference draws it again at every pass (:113-114 call _initialize) --; ``seed`` seeds the points and the order alike."""
        if name not in GENERATORS or name == 'cifar':
            raise ValueError('no toy set named %r' % (name, ))
        return cls(GENERATORS[name](int(n), np.random.default_rng(seed)), batch, seed=seed, **kw)

    @classmethod
    def from_npz(cls, path, key, batch, **kw):
        """an array a user has on disk: ``np.load(path)[key]``, uint8 images or float32 rows"""
        with np.load(path) as f:
            return cls(f[key], batch, **kw)

    def sweep_view(self, batch=None, dequantize=None, shuffle=False):
        """a sweep-schedule data set over the SAME device copy (no second upload) with its own step counter, batch tensor and -- by
        default -- the identity order: what FlowTrainer.evaluate takes.  ``batch`` / ``dequantize`` default to this set's."""
        return DeviceDataset(self.host, self.batch if batch is None else batch, pad=self.pad, seed=self.seed, shuffle=shuffle, device=None,
                             rank=self.rank, world=self.world, dequantize=self.dequantize if dequantize is None else dequantize,
                             sweep=True, _share=self.data)

    def gather(self):
        """one launch: this rank's batch of the step in device memory -> ``out`` (the step stays; ``advance()`` moves it on)"""
        if self.data is None:
            raise RuntimeError('this DeviceDataset was built with device=None: it has no device copy to gather from')
        N, a = self._N, (self.n, ) + (self.host.shape[1:] if self.image else (self.host.shape[1], ))
        head = (self.batch, self.stride, self.offset, self.steps_per_epoch, self.seed, int(self.shuffle))
        tail = (self.step.data_ptr(), self.last_indices.data_ptr(), N.stream())
        extra = self.dequantize or self.sweep
        if self.image and extra:
            N.call('nf_dataset_gather_u8_x', self.data.data_ptr(), self.out.data_ptr(), a[0], a[1], a[2], a[3], self.pad, *head,
                   int(self.dequantize), int(self.sweep), *tail)
        elif self.image:
            N.call('nf_dataset_gather_u8', self.data.data_ptr(), self.out.data_ptr(), a[0], a[1], a[2], a[3], self.pad, *head, *tail)
        elif extra:
            N.call('nf_dataset_gather_f32_x', self.data.data_ptr(), self.out.data_ptr(), a[0], a[1], *head, int(self.sweep), *tail)
        else:
            N.call('nf_dataset_gather_f32', self.data.data_ptr(), self.out.data_ptr(), a[0], a[1], *head, *tail)
        return self.out

    def advance(self):
        self._N.call('nf_sample_advance', self.step.data_ptr(), self._N.stream())

    def next(self):
        out = self.gather()
        self.advance()
        return out

    def _positions(self, step):
        epoch, k = divmod(int(step), self.steps_per_epoch)
        return epoch, k * self.stride + self.offset + np.arange(self.batch, dtype=np.int64)

    def valid(self, step):
        """the number of real rows in the batch of ``step``: ``batch`` on the loader's schedule, fewer in a sweep's last steps"""
        if not self.sweep:
            return self.batch
        return int(min(max(self.n - self._positions(step)[1][0], 0), self.batch))

    def indices(self, step):
        """(batch, ) int64: the samples this rank is served at ``step`` (numpy; what the kernel writes to ``last_indices``); a sweep's
        positions beyond the set are clamped to sample N - 1"""
        epoch, pos = self._positions(step)
        if not self.sweep:
            return dataset_perm(self.seed, epoch, pos, self.n) if self.shuffle else pos
        idx, ok = np.full(self.batch, self.n - 1, dtype=np.int64), pos < self.n
        idx[ok] = dataset_perm(self.seed, epoch, pos[ok], self.n) if self.shuffle else pos[ok]
        return idx

    def host_batch(self, step):
        """the batch of ``step`` as the reference builds it on the host (dataset.py:116-125), a float32 torch tensor; with
        ``dequantize`` the kernel's noise restated in numpy (every operation is exact in float32)"""
        idx = self.indices(step)
        rows = self.host[idx]
        if not self.image:
            return torch.from_numpy(rows)
        if self.dequantize:
            w = dequant_words(self.seed, step, idx, rows[0].size).reshape(rows.shape)
            q = (rows.astype(np.uint32) << np.uint32(15)) | (w >> np.uint32(17))
            x = (q.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
        else:
            x = rows.astype('float32') / 255.0
        x, p = np.transpose(x, (0, 3, 1, 2)), self.pad
        return torch.from_numpy(np.ascontiguousarray(np.pad(x, ((0, 0), (0, 0), (p, p), (p, p))).astype(np.float32)))
