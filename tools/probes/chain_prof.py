"""phase stamps of workgroup 0 of the persistent ConvNet kernel (csrc/conv_chain.hip built with -DNF_CC_PROF=1 into build/).
   python tools/probes/chain_prof.py --build ;  python tools/probes/chain_prof.py I O H W [B]
   --arrivals (with --cpl): the census of the build with -DNF_CC_PROF=2 -- no phase stamps, nothing that only workgroup 0 does; every
   workgroup records when it reaches the poll of every exchange round, forward and backward.  Printed per round, as medians over
   the launches: which workgroup came last most often, how far the last one lags the median, and the lag of workgroup 0.
   --lib=PATH: another build of the probe library (e.g. of an older conv_chain.hip)"""
import ctypes, importlib, os, subprocess, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
pkg = importlib.import_module('normalizing-flows-pytorch_amd')
N = importlib.import_module('normalizing-flows-pytorch_amd._native')
cond = importlib.import_module('normalizing-flows-pytorch_amd.conditioners')
here = os.path.dirname(os.path.abspath(pkg.__file__))
ARRIVALS = '--arrivals' in sys.argv
lib_path = os.path.join(here, 'build', 'libccprof2.so' if ARRIVALS else 'libccprof.so')
if '--build' in sys.argv:
    os.makedirs(os.path.join(here, 'build'), exist_ok=True)
    for mode, name in ((1, 'libccprof.so'), (2, 'libccprof2.so')):
        out = os.path.join(here, 'build', name)
        subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=on',
                               '-DNF_CC_PROF=%d' % mode, '-shared', '-o', out, os.path.join(here, 'csrc', 'conv_chain.hip')])
        print('built', out)
    sys.exit(0)
for a_ in sys.argv:
    if a_.startswith('--lib='):
        lib_path = os.path.abspath(a_[6:])
prof = ctypes.CDLL(lib_path)
real = N.load()
for name in ('nf_convnet_chain_fwd', 'nf_convnet_chain_bwd', 'nf_convnet_chain_usable', 'nf_convnet_chain_ws_floats', 'nf_conv_weight_pack', 'nf_conv_weight_pack_images'):
    fn = getattr(real, name)
    pf = getattr(prof, name)
    pf.argtypes, pf.restype = fn.argtypes, fn.restype
    setattr(real, name, pf)
I, O, H, W = [int(v) for v in sys.argv[1:5]]
B = int(sys.argv[5]) if len(sys.argv) > 5 else 64
net = cond.ConvNet(I, O).cuda().train()
net.fused = True
fc = importlib.import_module('normalizing-flows-pytorch_amd.fused_conv')
if '--nopack' not in sys.argv:                       # the path a model takes: weight images written once, streamed by the kernel
    wns = [m for m in net.modules() if isinstance(m, cond.WeightNorm)]
    with torch.no_grad():
        for m in wns:
            m._w_eff = m.effective_weight().contiguous()
    fc.pack_conv_weights(wns, [m._w_eff for m in wns])
    assert fc._convnet_packs(net) is not None
x = torch.randn(B, I, H, W, device='cuda')
CPL = '--cpl' in sys.argv                           # with the fused coupling: the launch a model makes (checkerboard split of (I/2, 2H, 2W))
if CPL:
    NF = importlib.import_module('normalizing-flows-pytorch_amd.functional')
    z = torch.randn(B, I // 2, 2 * H, 2 * W, device='cuda')
    a, c = torch.full((1, ), 0.5, device='cuda'), torch.zeros(1, device='cuda')
    BWD = '--bwd' in sys.argv or ARRIVALS             # (the census takes both directions)
    HEAD = '--head' in sys.argv                      # the next step's head transposed in the backward launch's prologue (nf_cc_head_bwd)
    Cf = I // 2
    hW, hls = torch.randn(Cf, Cf, device='cuda') / Cf ** 0.5, torch.randn(Cf, device='cuda') * 0.1

    class FakeHead(torch.autograd.Function):
        @staticmethod
        def forward(ctx, y):
            return y.clone()

        @staticmethod
        def backward(ctx, g_h):
            g_x = torch.empty_like(g_h)
            NF.PENDING_HEAD_BWD[g_x.data_ptr()] = (g_h.contiguous(), hls, hW, g_x, None if Cf >= 9 else (N.SPLIT_CHECKER, 0))
            return g_x
    from types import SimpleNamespace as NS
    holder = NS(meta={}, pending=[], g_ld={})
    h_b, h_logs = torch.randn(Cf, device='cuda') * 0.1, torch.randn(Cf, device='cuda') * 0.1
    FWD_HEAD = HEAD and not BWD and 9 <= Cf <= 64    # the step's head in the forward launch's prologue (nf_cc_head_fwd)

    def launch_pair():
        with torch.set_grad_enabled(BWD):
            zz = z.clone().requires_grad_(BWD)
            ld = torch.zeros(B, device='cuda')
            if FWD_HEAD:
                zz, xx, ld = NF.glow_head_w(zz, ld, hls, h_b, hW, h_logs, holder, 0, N.SPLIT_CHECKER, 0, defer=True)
            else:
                xx = NF.half_gather(zz.detach(), 1, N.SPLIT_CHECKER, 0)
            y, ld2 = fc.convnet_coupling(net, xx, zz, ld, a, c, N.SPLIT_CHECKER, 0)
            assert not NF.PENDING_HEADS
            if BWD:
                if HEAD:
                    y = FakeHead.apply(y)
                (y.square().sum() * 1e-3 + ld2.sum()).backward()
                assert not NF.PENDING_HEAD_BWD
    for _ in range(3):
        launch_pair()
else:
    with torch.no_grad():
        for _ in range(3):
            y = net(x)
torch.cuda.synchronize()
G = int(real.nf_convnet_chain_blocks(B, I, O, H, W))    # the workgroups of a launch
if ARRIVALS:
    assert CPL, '--arrivals goes with --cpl'
    import statistics
    NR, MAXB, NLAUNCH = 5, 128, 20
    lag_last = [[] for _ in range(2 * NR)]
    lag0 = [[] for _ in range(2 * NR)]
    who = [[0] * G for _ in range(2 * NR)]
    arr = (ctypes.c_longlong * (2 * NR * MAXB))()
    for _ in range(NLAUNCH):
        launch_pair()
        torch.cuda.synchronize()
        prof.nf_cc_arrive_read(arr)
        for r in range(2 * NR):
            ts = [arr[r * MAXB + i] / 100.0 for i in range(G)]
            med = statistics.median(ts)
            last = max(range(G), key=lambda i: ts[i])
            who[r][last] += 1
            lag_last[r].append(ts[last] - med)
            lag0[r].append(ts[0] - med)
    print('B %d  %d -> %d  %d x %d   %d workgroups, %d launches; us behind the median arrival at the poll (medians over the launches)' % (B, I, O, H, W, G, NLAUNCH))
    for r in range(2 * NR):
        top = max(range(G), key=lambda i: who[r][i])
        print('  %s round %d: last most often workgroup %3d (%2d of %d; workgroup 0 last in %2d) | last lags %.2f | workgroup 0 lags %+.2f'
              % ('forward ' if r < NR else 'backward', r % NR, top, who[r][top], NLAUNCH, who[r][0], statistics.median(lag_last[r]), statistics.median(lag0[r])))
    assert N.persistent_timeouts() == 0
    sys.exit(0)
buf = (ctypes.c_longlong * 128)()
prof.nf_cc_prof_read(buf)
t = [v / 100.0 for v in buf]   # us
print('B %d  %d -> %d  %d x %d   total %.1f us: zero+conv0 %.1f' % (B, I, O, H, W, t[51] - t[0], t[1] - t[0]))
for l in range(5):
    o = 8 * l
    print('  layer %d: wait/sync %.1f | k-split %.1f | finish+tile stats %.1f | grid exchange %.1f | consts %.1f | normalise+weights %.1f | K loop %.1f'
          % (l, t[2 + o] - (t[1] if l == 0 else t[8 + o - 8]), t[3 + o] - t[2 + o], t[4 + o] - t[3 + o], t[5 + o] - t[4 + o], t[6 + o] - t[5 + o],
             (t[7 + o] - t[6 + o]) if l < 4 else 0.0, (t[8 + o] - t[7 + o]) if l < 4 else 0.0))
print('  1x1 out conv %.1f' % (t[51] - t[50]))
print('  exchange of layer 1: sync %.1f | combine+publish %.1f | poll %.1f | sync %.1f | merge %.1f' % (
    t[56] - t[12], t[57] - t[56], t[58] - t[57], t[59] - t[58], t[13] - t[59]))
if '--head' in sys.argv and '--bwd' not in sys.argv:
    print('  prologue: requests %.1f | zero %.1f | head %.1f [W, An to LDS %.1f | barrier %.1f | blocks %.1f (loads %.1f, normalise + MFMA %.1f, outputs %.1f) | barrier %.1f] | rest of conv0 %.1f'
          % (t[105] - t[0], t[106] - t[105], t[107] - t[106], t[108] - t[106], t[109] - t[108], t[110] - t[109], t[111] - t[109], t[112] - t[111], t[110] - t[112], t[107] - t[110], t[1] - t[107]))
if '--bwd' in sys.argv:
    print('backward total %.1f us: zero + 1x1^T (coupling backward on the fly) %.1f' % (t[97] - t[64], t[65] - t[64]))
    for l in range(4, -1, -1):
        o = 66 + 6 * (4 - l)
        prev = t[65] if l == 4 else t[o - 1]
        print('  layer %d: loads+sync %.1f | k-split %.1f | gn, sums, exchange %.1f | G -> frame %.1f | weights wait+sync %.1f | K loop %.1f'
              % (l, t[o] - prev, t[o + 1] - t[o], t[o + 2] - t[o + 1], t[o + 3] - t[o + 2], (t[o + 4] - t[o + 3]) if l >= 1 else 0.0,
                 (t[o + 5] - t[o + 4]) if l >= 1 else 0.0))
    print('  conv0^T chunks + stores %.1f' % (t[97] - t[96]))
    print('  prologue: start -> head (zero, requests) %.1f | head %.1f [W to LDS %.1f | barrier %.1f | items %.1f | barrier %.1f] | 1x1^T %.1f'
          % (t[100] - t[64], t[101] - t[100], t[102] - t[100], t[103] - t[102], t[104] - t[103], t[101] - t[104], t[65] - t[101]))
arr = (ctypes.c_longlong * (2 * 5 * 128))()
prof.nf_cc_arrive_read(arr)
a = [arr[1 * 128 + i] / 100.0 for i in range(G)]          # [direction 0][round 1][workgroup]
print('  arrival of the workgroups at the poll of layer 1, us after the first: ' + ' '.join('%.1f' % (v - min(a)) for v in a))
if I > 32:
    print('  chunk 1 of conv0: weights requested, barrier %.1f | weights to LDS %.1f | frame loads + stores %.1f | barrier %.1f | K loop %.1f   (chunk 0 began %.1f us before)'
          % (t[53] - t[52], t[54] - t[53], t[55] - t[54], t[60] - t[55], t[61] - t[60], t[52] - t[0]))
