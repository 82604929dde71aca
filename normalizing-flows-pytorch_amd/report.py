"""
What the reference's ``Model.report`` (main.py:135-284) computes on its way to matplotlib, tensorboard and the jpg writer, without the
figure library: the latent positions and p(z) of a batch, samples with their density, the density of the 65 536 grid points through the
whole flow (main.py:198-211) and the clamped 8-per-row image grids (main.py:258-278), each as numpy arrays and as uint8 RGB panels that
``PIL.Image.fromarray`` or ``SummaryWriter.add_image(..., dataformats='HWC')`` take as they are.  Axes, ticks, titles and colour bars are
NOT drawn: a panel is the data area alone.

Three layers:
    *_host      numpy restatements of the kernels in csrc/report.hip, bit for bit (they need no GPU: the yardsticks of the GPU tests)
    grid, minmax, colorize, scatter, image_grid
                the device wrappers: CUDA tensors in, CUDA tensors out, launches on the current stream, no synchronisation
    report      FlowTrainer.report (train.py): everything queued, ONE host read

Exactness: every number that decides a pixel or a table index is a double built from separately rounded
operations on both sides (numpy ufuncs never contract a multiply and an add; the kernels are compiled with contraction off), and the
colour is a function of the STORED float32 value, so exp() may differ in the last place between the two without moving a pixel.
"""
import ctypes
import math
import warnings

import numpy as np

CMAPS = {'inferno': 0, 'jet': 1}                # NF_CMAP_* of include/nfhip.h
MAX_CANVAS, MAX_RADIUS = 4096, 8
_tables = {}
_one_colour = {}                                # device -> (1, 3) uint8 jet[0], the colour of the data panel


def _cmap_id(cmap):
    if cmap in CMAPS:
        return CMAPS[cmap]
    if cmap in CMAPS.values() and not isinstance(cmap, bool):
        return int(cmap)
    raise ValueError('colour map %r: the tables hold %s' % (cmap, ' and '.join(sorted(CMAPS))))


def cmap_table(name):
    """(256, 3) uint8: the table the kernels index, read from the library (nf_report_cmap, host only -- no GPU needed)"""
    cid = _cmap_id(name)
    if cid not in _tables:
        from . import _native as N
        buf = (ctypes.c_uint8 * 768)()
        rc = N.load().nf_report_cmap(cid, ctypes.addressof(buf))
        if rc != 0:
            raise N.NativeLibraryError('nf_report_cmap failed with code %d' % rc)
        t = np.frombuffer(buf, dtype=np.uint8).reshape(256, 3).copy()
        t.setflags(write=False)
        _tables[cid] = t
    return _tables[cid]


# -- host restatements -------------------------------------------------------------------------------------------------------------------
def grid_host(map_size):
    """main.py:199-206, literally: (map_size^2, 2) float32"""
    ix = (np.arange(map_size) + 0.5) / map_size * 2.0 - 1.0
    iy = (np.arange(map_size) + 0.5) / map_size * -2.0 + 1.0
    ix, iy = np.meshgrid(ix, iy)
    return np.stack([ix.reshape(-1), iy.reshape(-1)], axis=1).astype(np.float32)


def minmax_host(v):
    """(min, max) over the finite values as floats; (0.0, 1.0) when there is none"""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    f = v[np.isfinite(v)]
    if f.size == 0:
        return 0.0, 1.0
    return float(f.min()), float(f.max())


def colorize_host(p, lo, hi, cmap):
    """p float32 (any shape) -> uint8 p.shape + (3, ): index 0 if x < 0 or hi == lo, 255 if x >= 1, else floor(x * 256) with
    x = (double(p) - lo) / (hi - lo); NaN -> (0, 0, 0).  What matplotlib's cmap(Normalize(lo, hi)(p), bytes=True)[..., :3] gives."""
    p = np.asarray(p, dtype=np.float32)
    tab = cmap_table(cmap)
    lo, hi = float(lo), float(hi)
    nan = np.isnan(p)
    if hi == lo:
        idx = np.zeros(p.shape, dtype=np.int64)
    else:
        with np.errstate(invalid='ignore', over='ignore'):
            x = (np.where(nan, 0.0, p).astype(np.float64) - lo) / (hi - lo)
            inside = (x >= 0.0) & (x < 1.0)
            idx = np.where(inside, np.floor(np.where(inside, x, 0.0) * 256.0), np.where(x >= 1.0, 255.0, 0.0)).astype(np.int64)
    rgb = tab[idx]
    rgb[nan] = 0
    return rgb


def view_matrix(elev=10.0, azim=-80.0):
    """row-major 3 x 3 double: (u, v, depth) = M @ (x, y, z) for an orthographic camera at elevation ``elev`` and azimuth ``azim`` degrees
    looking at the origin, z up (the reference's ax.view_init(elev=10.0, azim=-80.0), common/utils.py:24): u to the right, v up,
    depth towards the viewer (larger = nearer)."""
    e, a = math.radians(float(elev)), math.radians(float(azim))
    ce, se, ca, sa = math.cos(e), math.sin(e), math.cos(a), math.sin(a)
    return np.array([[-sa, ca, 0.0],
                     [-se * ca, -se * sa, ce],
                     [ce * ca, ce * sa, se]], dtype=np.float64)


def scatter_host(pts, rgb_pt, S, radius, view=None):
    """the scatter panel of nf_report_scatter in numpy and a python loop over the points: (S, S, 3) uint8.  ``view`` (3 x 3) is needed
    for (n, 3) points and ignored for (n, 2)."""
    pts = np.asarray(pts, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] not in (2, 3):
        raise ValueError('scatter panels take (n, 2) or (n, 3) points, got %s' % (pts.shape, ))
    n, D = pts.shape
    S, radius = int(S), int(radius)
    if not (1 <= S <= MAX_CANVAS and 0 <= radius <= MAX_RADIUS):
        raise ValueError('canvas %d (1..%d) / radius %d (0..%d)' % (S, MAX_CANVAS, radius, MAX_RADIUS))
    rgb_pt = np.asarray(rgb_pt, dtype=np.uint8).reshape(n, 3)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        if D == 3:
            M = np.asarray(view, dtype=np.float64).reshape(3, 3)
            z = pts[:, 2].astype(np.float64)
            u = (M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z           # (elementwise: every operation rounded on its own, as in the kernel)
            w = (M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z
            depth = (M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z
        else:
            u, w, depth = x, y, np.zeros(n)
        ok = np.isfinite(u) & np.isfinite(w) & np.isfinite(depth)
        cx = np.floor((u + 1.0) * 0.5 * float(S))
        cy = np.floor((1.0 - w) * 0.5 * float(S))
        ok &= ~((cx + radius < 0.0) | (cx - radius >= S) | (cy + radius < 0.0) | (cy - radius >= S))
        dq = np.floor(np.clip((depth + 2.0) / 4.0, 0.0, 1.0) * 1048575.0)
    keys = np.zeros((S, S), dtype=np.uint64)
    offs = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if dx * dx + dy * dy <= radius * radius]
    for i in np.nonzero(ok)[0]:
        key = np.uint64((int(dq[i]) << 32) | (int(i) + 1))
        px, py = int(cx[i]), int(cy[i])
        for dy, dx in offs:
            qx, qy = px + dx, py + dy
            if 0 <= qx < S and 0 <= qy < S and keys[qy, qx] < key:
                keys[qy, qx] = key
    out = np.full((S, S, 3), 255, dtype=np.uint8)
    hit = keys != 0
    out[hit] = rgb_pt[(keys[hit] & np.uint64(0xffffffff)).astype(np.int64) - 1]
    return out


def _grid_shape(n, H, W, nrow, padding):
    xmaps = min(int(nrow), int(n))
    ymaps = -(-int(n) // xmaps)
    return xmaps, ymaps, (H + padding) * ymaps + padding, (W + padding) * xmaps + padding


def _to_byte_host(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        c = np.where(x > 0, np.where(x < 1, x, np.float32(1.0)), np.float32(0.0)).astype(np.float32)     # NaN -> 0
    return (c * np.float32(255.0)).astype(np.uint8)


def image_grid_host(x, nrow=8, padding=2, pad_value=1.0):
    """torchvision's make_grid(clamp(x, 0, 1), nrow, padding, pad_value).permute(1, 2, 0) through save_image's
    (image * 255.0).astype('uint8') (main.py:258-263, common/utils.py:76-78): x (n, C, H, W), C in {1, 3} -> (Hout, Wout, 3) uint8.
    n = 1 gets its border like any other n (torchvision returns the bare image there)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 4 or x.shape[0] < 1 or x.shape[1] not in (1, 3) or nrow < 1 or padding < 0:
        raise ValueError('image_grid takes (n >= 1, C in {1, 3}, H, W), nrow >= 1, padding >= 0; got %s, %r, %r' % (x.shape, nrow, padding))
    n, C, H, W = x.shape
    xmaps, ymaps, Hout, Wout = _grid_shape(n, H, W, nrow, padding)
    out = np.empty((Hout, Wout, 3), dtype=np.uint8)
    out[...] = _to_byte_host(np.float32(pad_value))
    b = _to_byte_host(x)
    for k in range(n):
        r, c = divmod(k, xmaps)
        y0, x0 = r * (H + padding) + padding, c * (W + padding) + padding
        out[y0:y0 + H, x0:x0 + W, :] = np.transpose(b[k] if C == 3 else np.repeat(b[k], 3, axis=0), (1, 2, 0))
    return out


# -- device wrappers -----------------------------------------------------------------------------------------------------------------------
def _f32(t, what):
    import torch
    from . import _native as N
    if t.dtype != torch.float32:
        raise N.NativeLibraryError('%s takes float32, got %s' % (what, t.dtype))
    return N.ptr(t.contiguous())


def grid(map_size, device='cuda'):
    """(map_size^2, 2) float32 on ``device``: nf_report_grid"""
    import torch
    from . import _native as N
    y = torch.empty((int(map_size) * int(map_size), 2), dtype=torch.float32, device=device)
    with torch.cuda.device(y.device):
        N.call('nf_report_grid', N.ptr(y), int(map_size), N.stream())
    return y


def minmax(v, out=None):
    """float64 tensor [min, max] over the finite values of ``v`` ([0, 1] when there is none), on the device, no synchronisation"""
    import torch
    from . import _native as N
    v = v.contiguous()
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=v.device)
    N.call('nf_report_minmax', _f32(v, 'minmax'), v.numel(), out.data_ptr(), N.stream())
    return out


def colorize(v, lo=0.0, hi=1.0, cmap='inferno', is_log=False, range_dev=None, p_out=None, rgb=True):
    """uint8 v.shape + (3, ) colours of p = exp(v) (``is_log``) or v, over (lo, hi) or the device pair ``range_dev`` (minmax()).
    ``p_out`` (float32, v's shape; may be v itself) receives p; ``rgb=False`` computes p_out alone and returns it."""
    import torch
    from . import _native as N
    v = v.contiguous()
    out = torch.empty(tuple(v.shape) + (3, ), dtype=torch.uint8, device=v.device) if rgb else None
    if p_out is not None and (p_out.dtype != torch.float32 or not p_out.is_contiguous() or p_out.numel() != v.numel()):
        raise N.NativeLibraryError('colorize: p_out must be a contiguous float32 tensor of v\'s size')
    if v.numel() > 0:
        N.call('nf_report_colorize', _f32(v, 'colorize'), v.numel(), 1 if is_log else 0,
               None if range_dev is None else N.ptr(range_dev, (torch.float64, )), float(lo), float(hi), _cmap_id(cmap),
               None if p_out is None else N.ptr(p_out), None if out is None else out.data_ptr(), N.stream())
    return out if rgb else p_out


def scatter(pts, rgb_pt, S, radius, view=None):
    """(S, S, 3) uint8 panel of the (n, 2) or (n, 3) float32 points with colours rgb_pt (n, 3) uint8: nf_report_scatter"""
    import torch
    from . import _native as N
    n, D = int(pts.shape[0]), int(pts.shape[1])
    pts, rgb_pt = pts.contiguous(), rgb_pt.contiguous()
    if rgb_pt.dtype != torch.uint8 or rgb_pt.numel() != 3 * n:
        raise N.NativeLibraryError('scatter: rgb_pt must be (n, 3) uint8')
    keys = torch.empty(int(S) * int(S), dtype=torch.int64, device=pts.device)          # (the kernels read it as uint64)
    out = torch.empty((int(S), int(S), 3), dtype=torch.uint8, device=pts.device)
    v9 = None
    if D == 3:
        v9 = np.ascontiguousarray(view_matrix() if view is None else view, dtype=np.float64).reshape(9)
    N.call('nf_report_scatter', _f32(pts, 'scatter') if n else None, rgb_pt.data_ptr() if n else None, n, D,
           None if v9 is None else v9.ctypes.data, int(S), int(radius), keys.data_ptr(), out.data_ptr(), N.stream())
    return out


def image_grid(x, nrow=8, padding=2, pad_value=1.0):
    """(Hout, Wout, 3) uint8 grid of the (n, C, H, W) float32 images: nf_report_image_grid"""
    import torch
    from . import _native as N
    x = x.contiguous()
    if x.dim() != 4:
        raise N.NativeLibraryError('image_grid takes (n, C, H, W), got %s' % (tuple(x.shape), ))
    n, C, H, W = (int(s) for s in x.shape)
    if n < 1 or nrow < 1 or padding < 0:
        raise N.NativeLibraryError('image_grid: n, nrow >= 1 and padding >= 0, got %d, %r, %r' % (n, nrow, padding))
    _, _, Hout, Wout = _grid_shape(n, H, W, nrow, padding)
    out = torch.empty((Hout, Wout, 3), dtype=torch.uint8, device=x.device)
    N.call('nf_report_image_grid', _f32(x, 'image_grid'), n, C, H, W, int(nrow), int(padding), float(pad_value), out.data_ptr(), N.stream())
    return out


# -- FlowTrainer.report --------------------------------------------------------------------------------------------------------------------
class _MapChain:
    """the density map of one (trainer, map_size): grid -> net(y) -> log p -> exp + inferno, with every tensor it writes held here so
    that a captured hipGraph of ``run`` can be replayed (main.py:198-213)"""

    def __init__(self, trainer, map_size, device):
        import torch
        self.net, self.m, B = trainer.net, int(map_size), int(map_size) * int(map_size)
        self.y = torch.empty((B, 2), dtype=torch.float32, device=device)
        self.row = torch.empty(B, dtype=torch.float64, device=device)
        self.acc = torch.zeros(3, dtype=torch.float64, device=device)
        self.logp = torch.empty(B, dtype=torch.float32, device=device)
        self.p = torch.empty(B, dtype=torch.float32, device=device)
        self.rgb = torch.empty((B, 3), dtype=torch.uint8, device=device)
        self.graph, self.det = None, None

    def run(self):
        import torch
        from . import _native as N
        B = self.m * self.m
        N.call('nf_report_grid', N.ptr(self.y), self.m, N.stream())
        z, ld = self.net(self.y)
        z, ld = z.reshape(B, -1), ld.reshape(B)
        if z.dtype != torch.float32 or ld.dtype != torch.float32:       # FFJORD: float64 states, served through a torch cast
            z, ld = z.float(), ld.float()
        z, ld = z.contiguous(), ld.contiguous()
        # the evaluation fold with N = stride = B, offset 0 and no step: every row valid, the float32 row is what report needs
        N.call('nf_logp_accumulate', N.ptr(z), N.ptr(ld), self.row.data_ptr(), N.ptr(self.logp), None, self.acc.data_ptr(), B, int(z.shape[1]),
               B, B, 0, None, N.stream())
        N.call('nf_report_colorize', N.ptr(self.logp), B, 1, None, 0.0, 1.0, CMAPS['inferno'], N.ptr(self.p), self.rgb.data_ptr(), N.stream())


def _density_map(trainer, map_size, device, graph):
    import torch
    chains = trainer.__dict__.setdefault('_report_maps', {})
    ch = chains.get(int(map_size))
    if ch is None:
        ch = chains[int(map_size)] = _MapChain(trainer, map_size, device)
    from . import _native as N
    if ch.graph is not None and ch.det != N.deterministic():
        ch.graph = None                                     # (a graph holds the launch shapes of the mode it was captured in)
    if graph and ch.graph is None:
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                   # one eager pass on the side stream (capture etiquette)
                ch.run()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = trainer._graph_factory()
            g.capture(ch.run)
            ch.graph, ch.det = g, N.deterministic()
        except Exception as e:
            warnings.warn('hipGraph capture of the density map failed (%s: %s); continuing with eager launches' % (type(e).__name__, e))
            ch.graph = None
            torch.cuda.synchronize()
    if graph and ch.graph is not None:
        ch.graph.replay()
    else:
        ch.run()
    return ch


def _points_panel(pts, values, canvas, radius, view):
    """jet over the finite range of ``values`` (matplotlib's autoscale of scatter(c=...), common/utils.py:19), painted at ``pts``"""
    rng = minmax(values)
    return scatter(pts, colorize(values, cmap='jet', range_dev=rng), canvas, radius, view)


def report(trainer, y_data, n_samples=None, graph=False, generator=None, map_size=256, canvas=512, radius=2):
    """FlowTrainer.report: see train.py"""
    import torch
    from .train import standard_normal_logprob
    net = trainer.net
    net.eval()
    dev = next(net.parameters()).device
    if not y_data.is_cuda:
        y_data = y_data.to(dev)
    with torch.cuda.device(y_data.device):
        return _report(trainer, net, y_data.contiguous(), n_samples, graph, generator, map_size, canvas, radius, standard_normal_logprob)


def _report(trainer, net, y_data, n_samples, graph, generator, map_size, canvas, radius, logprob):
    import torch
    n, dev = int(y_data.shape[0]), y_data.device
    vec = y_data.dim() == 2 and y_data.shape[1] in (2, 3)                       # main.py:142-147
    if n_samples is None:
        n_samples = max(100, n) if vec else max(64, n)
    out = {}
    if vec:
        D = int(y_data.shape[1])
        view = view_matrix() if D == 3 else None
        y32 = y_data.float()
        # latent positions and p(z)  (main.py:166-173, :224-232)
        z, _ = net(y_data)
        z = z.reshape(n, -1).float().contiguous()
        pz = colorize(logprob(z).float(), is_log=True, p_out=torch.empty(n, dtype=torch.float32, device=dev), rgb=False)
        out['z'], out['pz'], out['z_rgb'] = z, pz, _points_panel(z, pz, canvas, radius, view)
        # samples with their density  (main.py:183-189, :242-249)
        zs = torch.randn((n_samples, ) + tuple(net.dims), device=dev, generator=generator)
        ys, ld = net.backward(zs)
        ys = ys.reshape(n_samples, -1).float().contiguous()
        py = colorize((logprob(zs) - ld).float(), is_log=True, p_out=torch.empty(n_samples, dtype=torch.float32, device=dev), rgb=False)
        out['y_sample'], out['py_sample'], out['y_rgb'] = ys, py, _points_panel(ys, py, canvas, radius, view)
        # the data, in one colour  (main.py:154-157; matplotlib's default blue there, the first entry of the same map here)
        one = _one_colour.get(dev)
        if one is None:                                     # (uploaded once per device: no host-to-device copy in later reports)
            one = _one_colour[dev] = torch.from_numpy(cmap_table('jet')[:1].copy()).to(dev)
        out['y_data_rgb'] = scatter(y32.contiguous(), one.expand(n, 3).contiguous(), canvas, radius, view)
        if D == 2:
            ch = _density_map(trainer, map_size, dev, graph)
            out['py_map'], out['py_map_rgb'] = ch.p.view(ch.m, ch.m), ch.rgb.view(ch.m, ch.m, 3)
    else:
        # the clamped 8-per-row grids  (main.py:258-278)
        out['data_grid'] = image_grid(y_data.float())
        zs = torch.randn((n_samples, ) + tuple(net.dims), device=dev, generator=generator)
        ys, _ = net.backward(zs)
        ys = ys[:64].float().contiguous()
        out['y_sample'], out['sample_grid'] = ys, image_grid(ys)
    # everything above is queued; one host read
    host = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in out.items()}
    for k, t in out.items():
        host[k].copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return {k: h.numpy().copy() for k, h in host.items()}
