// The fused optimizer steps over flat parameter / gradient / state buffers: the whole step is ONE launch (+ a 1-thread step-counter
// bump on the plain path), instead of the thousands of per-parameter scalar kernels a capturable framework optimizer issues for the
// ~1100 small tensors of a 32-step flow.  Four recipes -- Adam and RMSprop, which the reference trains with (main.py:56-64,
// configs/default.yaml:13-20), Adamax and AdamW (Glow's and the weight-normed conditioners') -- whose element arithmetic is
// csrc/nf_optim_recipes.h, in ONE kernel body, k_optim_step<R, VEC, MODE>, behind ONE launcher and eight entry points:
//   nf_X_step           plain: step[0] += 1 (k_adam_tick), then the stream with grad_scale as the caller gives it;
//   nf_X_step_guarded   after nf_grad_guard (csrc/optim_guard.hip, which ticks): grad_scale = ctl->clip_scale, nothing touched when
//                       ctl->skip is set -- AdamW's decoupled decay included, it is part of the element's update behind the same early
//                       return --, and with ema != NULL the averaged weights updated in the same pass from the new parameter.
// `step` and `lr` live in device memory so that a captured hipGraph replays with the right values.
// Below them the schedules as one-thread launches: StepLR (nf_lr_step_decay) and linear warmup times constant / step / cosine decay
// (nf_lr_schedule); and nf_multi_copy.
#include <math.h>

#include "nf_common.h"
#include "nf_optim_recipes.h"

__global__ void k_adam_tick(int* __restrict__ step) { step[0] += 1; }

// ema = p_new on the first update that is taken (ActNorm initialises in the first forward), d ema + (1 - d) p_new afterwards
__device__ __forceinline__ float nf_ema_one(float e, float p, float d) { return fmaf(d, e, (1.f - d) * p); }

// A pure stream: per element 4 B of gradient read, 4 B of parameter and of each of the recipe's R::STATES buffers read and written (28 B
// for the Adam family, 20 B for RMSprop, whose m is NULL and never formed into an address that is used), and 8 B more for the average
// (4 B on the step that copies).  VEC: every buffer sits on 16 bytes, the body moves float4s and the last n % 4 elements take the scalar
// form in the same launch; otherwise every element does.
enum { NF_STEP_PLAIN, NF_STEP_GUARDED, NF_STEP_GUARDED_EMA };

template <class R, bool VEC, int MODE>
__global__ void __launch_bounds__(NF_BLOCK) k_optim_step(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ s, const int* __restrict__ step,
                                                         const float* __restrict__ lr, NfOptimHyper h, float grad_scale,
                                                         const nf_guard_ctl* __restrict__ ctl, float* __restrict__ ema, float ema_decay,
                                                         int64_t n) {
    constexpr bool TWO = R::STATES == 2, EMA = MODE == NF_STEP_GUARDED_EMA;
    bool first = false;
    if (MODE != NF_STEP_PLAIN) {                              // (the plain form does not read the control block)
        if (ctl->skip != 0) return;                           // uniform over the grid: nothing is touched
        grad_scale = ctl->clip_scale;
        first = ctl->ema_count == 1;
    }
    const typename R::Consts c = R::consts(step, lr, h);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;                                         // elements [0, done) are covered by the float4 body
    if (VEC) {
        const int64_t n4 = n / 4;
        float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
        float4* __restrict__ s4 = reinterpret_cast<float4*>(s);
        float4* __restrict__ e4 = reinterpret_cast<float4*>(ema);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        for (int64_t i = tid; i < n4; i += gstride) {
            float4 pi = p4[i], si = s4[i], mi = {};
            if constexpr (TWO) mi = m4[i];
            const float4 gi = g4[i];
            R::one(pi.x, gi.x, mi.x, si.x, c, grad_scale);
            R::one(pi.y, gi.y, mi.y, si.y, c, grad_scale);
            R::one(pi.z, gi.z, mi.z, si.z, c, grad_scale);
            R::one(pi.w, gi.w, mi.w, si.w, c, grad_scale);
            if constexpr (TWO) m4[i] = mi;
            s4[i] = si;
            p4[i] = pi;
            if (EMA) {
                float4 ei = pi;
                if (!first) {
                    ei = e4[i];
                    ei.x = nf_ema_one(ei.x, pi.x, ema_decay);
                    ei.y = nf_ema_one(ei.y, pi.y, ema_decay);
                    ei.z = nf_ema_one(ei.z, pi.z, ema_decay);
                    ei.w = nf_ema_one(ei.w, pi.w, ema_decay);
                }
                e4[i] = ei;
            }
        }
        done = 4 * n4;
    }
    for (int64_t i = done + tid; i < n; i += gstride) {
        float pi = p[i], si = s[i], mi = 0.f;
        if constexpr (TWO) mi = m[i];
        R::one(pi, g[i], mi, si, c, grad_scale);
        if constexpr (TWO) m[i] = mi;
        s[i] = si;
        p[i] = pi;
        if (EMA) ema[i] = first ? pi : nf_ema_one(ema[i], pi, ema_decay);
    }
}

template <class R, int MODE>
static auto nf_step_kernel(bool vec) { return vec ? k_optim_step<R, true, MODE> : k_optim_step<R, false, MODE>; }

// The launcher of all eight entry points.  m is the first moment (NULL for a one-state recipe), s the second buffer; guarded: ctl is
// read and ema may be given, step has been ticked by nf_grad_guard; plain: ctl and ema are NULL and step is ticked here.
template <class R>
static int nf_optim_step(bool guarded, float* param, const float* grad, float* m, float* s, const int* step, const float* lr,
                         const NfOptimHyper& h, float grad_scale, const nf_guard_ctl* ctl, float* ema, float ema_decay, int64_t n,
                         nf_stream_t stream) {
    if (n < 0 || (guarded && ctl == nullptr)) return NF_E_BADARG;
    if (n == 0) return 0;
    if (param == nullptr || grad == nullptr || s == nullptr || lr == nullptr) return NF_E_BADARG;
    if ((R::STATES == 2 && m == nullptr) || ((R::USES_STEP || !guarded) && step == nullptr)) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (!guarded) {
        hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, st, const_cast<int*>(step));      // (a plain entry point's step is int*)
        NF_CHECK_LAUNCH();
    }
    const bool vec = n >= 4 && (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)s | (uintptr_t)ema) & 15) == 0;      // (NULL counts as aligned)
    const auto kernel = !guarded ? nf_step_kernel<R, NF_STEP_PLAIN>(vec)
                                 : ema != nullptr ? nf_step_kernel<R, NF_STEP_GUARDED_EMA>(vec) : nf_step_kernel<R, NF_STEP_GUARDED>(vec);
    hipLaunchKernelGGL(kernel, dim3(nf_grid_for(vec ? n / 4 : n)), dim3(NF_BLOCK), 0, st, param, grad, m, s, step, lr, h,
                       grad_scale, ctl, ema, ema_decay, n);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int* step, const float* lr,
                            float beta1, float beta2, float eps, float weight_decay, float grad_scale, int64_t n,
                            nf_stream_t stream) {
    return nf_optim_step<NfAdam>(false, param, grad, exp_avg, exp_avg_sq, step, lr, nf_adam_hyper(beta1, beta2, eps, weight_decay), grad_scale,
                                 nullptr, nullptr, 0.f, n, stream);
}

extern "C" int nf_rmsprop_step(float* param, const float* grad, float* square_avg, int* step, const float* lr, float alpha,
                               float eps, float weight_decay, float grad_scale, int64_t n, nf_stream_t stream) {
    return nf_optim_step<NfRmsprop>(false, param, grad, nullptr, square_avg, step, lr, nf_rmsprop_hyper(alpha, eps, weight_decay), grad_scale,
                                    nullptr, nullptr, 0.f, n, stream);
}

extern "C" int nf_adamax_step(float* param, const float* grad, float* exp_avg, float* exp_inf, int* step, const float* lr, float beta1,
                              float beta2, float eps, float weight_decay, float grad_scale, int64_t n, nf_stream_t stream) {
    return nf_optim_step<NfAdamax>(false, param, grad, exp_avg, exp_inf, step, lr, nf_adam_hyper(beta1, beta2, eps, weight_decay), grad_scale,
                                   nullptr, nullptr, 0.f, n, stream);
}

extern "C" int nf_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int* step, const float* lr, float beta1,
                             float beta2, float eps, float weight_decay, float grad_scale, int64_t n, nf_stream_t stream) {
    return nf_optim_step<NfAdamW>(false, param, grad, exp_avg, exp_avg_sq, step, lr, nf_adam_hyper(beta1, beta2, eps, weight_decay), grad_scale,
                                  nullptr, nullptr, 0.f, n, stream);
}

extern "C" int nf_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int* step,
                                    const float* lr, float beta1, float beta2, float eps, float weight_decay, const nf_guard_ctl* ctl,
                                    float* ema, float ema_decay, int64_t n, nf_stream_t stream) {
    return nf_optim_step<NfAdam>(true, param, grad, exp_avg, exp_avg_sq, step, lr,
                                 nf_adam_hyper(beta1, beta2, eps, weight_decay), 1.f, ctl, ema, ema_decay, n, stream);
}

extern "C" int nf_rmsprop_step_guarded(float* param, const float* grad, float* square_avg, const float* lr, float alpha, float eps,
                                       float weight_decay, const nf_guard_ctl* ctl, float* ema, float ema_decay, int64_t n,
                                       nf_stream_t stream) {
    return nf_optim_step<NfRmsprop>(true, param, grad, nullptr, square_avg, nullptr, lr, nf_rmsprop_hyper(alpha, eps, weight_decay), 1.f, ctl,
                                    ema, ema_decay, n, stream);
}

extern "C" int nf_adamax_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_inf, const int* step, const float* lr,
                                      float beta1, float beta2, float eps, float weight_decay, const nf_guard_ctl* ctl, float* ema,
                                      float ema_decay, int64_t n, nf_stream_t stream) {
    return nf_optim_step<NfAdamax>(true, param, grad, exp_avg, exp_inf, step, lr,
                                   nf_adam_hyper(beta1, beta2, eps, weight_decay), 1.f, ctl, ema, ema_decay, n, stream);
}

extern "C" int nf_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int* step, const float* lr,
                                     float beta1, float beta2, float eps, float weight_decay, const nf_guard_ctl* ctl, float* ema,
                                     float ema_decay, int64_t n, nf_stream_t stream) {
    return nf_optim_step<NfAdamW>(true, param, grad, exp_avg, exp_avg_sq, step, lr,
                                  nf_adam_hyper(beta1, beta2, eps, weight_decay), 1.f, ctl, ema, ema_decay, n, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// StepLR on the device (main.py:68-70, :90: scheduler.step() after every optim.step()): one thread, enqueued BEFORE the
// optimizer launch of the same step, so that it is part of the captured graph and replays decay without host work.
// pos[0] counts the optimizer steps taken under the schedule; step number pos + 1 trains at
//   lr = base_lr * decay_ratio ^ (pos / decay_steps)
// formed in double from the base rate and the INTEGER exponent (repeated squaring) and rounded to float once -- multiplying
// a float by the ratio at every boundary would drift from torch's double-precision StepLR.
// ---------------------------------------------------------------------------------------------------------------
__global__ void k_lr_step_decay(float* __restrict__ lr, const double* __restrict__ base_lr, int* __restrict__ pos, int decay_steps,
                                double decay_ratio) {
    const int t = pos[0];
    int e = t / decay_steps;
    double f = 1.0, b = decay_ratio;
    while (e > 0) {
        if (e & 1) f *= b;
        b *= b;
        e >>= 1;
    }
    lr[0] = (float)(base_lr[0] * f);
    pos[0] = t + 1;
}

extern "C" int nf_lr_step_decay(float* lr, const double* base_lr, int* pos, int decay_steps, double decay_ratio, nf_stream_t stream) {
    if (lr == nullptr || base_lr == nullptr || pos == nullptr || decay_steps < 1) return NF_E_BADARG;
    hipLaunchKernelGGL(k_lr_step_decay, dim3(1), dim3(1), 0, (hipStream_t)stream, lr, base_lr, pos, decay_steps, decay_ratio);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Linear warmup times a decay, on the device (torch's SequentialLR([LinearLR, CosineAnnealingLR | StepLR], milestones=[W]) stepped
// after every optim.step(): main.py:89-90 with the schedules Glow and Flow++ are published with instead of the bare StepLR of
// main.py:68-70).  One thread, enqueued where k_lr_step_decay is.  With p = pos[0], W = warmup_steps, t = max(p - W, 0):
//   warm  = 1 for p >= W, else warmup_start + (1 - warmup_start) p / W
//   decay = base                                                      NF_LR_CONST
//         = base * arg ^ (t / span)            (integer power)        NF_LR_STEP    (arg: the ratio)
//         = arg + (base - arg) (1 + cos(pi t / span)) / 2, t < span   NF_LR_COSINE  (arg: the floor; AT and PAST t = span the rate
//                                                                     IS arg -- it holds, torch's CosineAnnealingLR swings back up)
// lr[0] = (float)(warm * decay), everything in double and rounded once; pos[0] = p + 1.
// ---------------------------------------------------------------------------------------------------------------
__global__ void k_lr_schedule(float* __restrict__ lr, const double* __restrict__ base_lr, int* __restrict__ pos, int warmup_steps,
                              double warmup_start, int kind, int span, double arg) {
    const int p = pos[0];
    const double base = base_lr[0];
    const double warm = p >= warmup_steps ? 1.0 : warmup_start + (1.0 - warmup_start) * (double)p / (double)warmup_steps;
    const int t = p > warmup_steps ? p - warmup_steps : 0;
    double d = base;
    if (kind == NF_LR_STEP) {
        int e = t / span;
        double f = 1.0, b = arg;
        while (e > 0) {
            if (e & 1) f *= b;
            b *= b;
            e >>= 1;
        }
        d = base * f;
    } else if (kind == NF_LR_COSINE) {
        d = t >= span ? arg : arg + (base - arg) * (1.0 + cos(M_PI * (double)t / (double)span)) / 2.0;
    }
    lr[0] = (float)(warm * d);
    pos[0] = p + 1;
}

extern "C" int nf_lr_schedule(float* lr, const double* base_lr, int* pos, int warmup_steps, double warmup_start, int kind, int span,
                              double arg, nf_stream_t stream) {
    if (lr == nullptr || base_lr == nullptr || pos == nullptr || warmup_steps < 0) return NF_E_BADARG;
    if (warmup_steps > 0 && !(warmup_start > 0.0 && warmup_start <= 1.0)) return NF_E_BADARG;
    if (kind != NF_LR_CONST && kind != NF_LR_STEP && kind != NF_LR_COSINE) return NF_E_BADARG;
    if (kind != NF_LR_CONST && span < 1) return NF_E_BADARG;
    if (kind == NF_LR_COSINE && !(arg >= 0.0)) return NF_E_BADARG;
    hipLaunchKernelGGL(k_lr_schedule, dim3(1), dim3(1), 0, (hipStream_t)stream, lr, base_lr, pos, warmup_steps, warmup_start, kind, span,
                       arg);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// gather of many small gradient tensors into the flat bucket: one launch per NF_COPY_MAX tensors instead of one
// AccumulateGrad add per parameter (an image Glow has ~2 600 framework-produced parameter gradients: 12 ms of adds)
// ---------------------------------------------------------------------------------------------------------------
struct NfCopyArgs { nf_copy_desc d[NF_COPY_MAX]; };

__global__ void __launch_bounds__(NF_BLOCK) k_multi_copy(NfCopyArgs args) {
    const nf_copy_desc& d = args.d[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += (int64_t)gridDim.x * blockDim.x) d.dst[i] = d.src[i];
}

extern "C" int nf_multi_copy(const nf_copy_desc* descs, int n_tensors, nf_stream_t stream) {
    if (descs == nullptr || n_tensors < 1 || n_tensors > NF_COPY_MAX) return NF_E_BADARG;
    NfCopyArgs args;
    int64_t maxn = 1;
    for (int i = 0; i < n_tensors; ++i) {
        if (descs[i].n < 0 || (descs[i].n > 0 && (descs[i].src == nullptr || descs[i].dst == nullptr))) return NF_E_BADARG;
        args.d[i] = descs[i];
        if (descs[i].n > maxn) maxn = descs[i].n;
    }
    int64_t gx = (maxn + NF_BLOCK - 1) / NF_BLOCK;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_multi_copy, dim3((unsigned)gx, (unsigned)n_tensors), dim3(NF_BLOCK), 0, (hipStream_t)stream, args);
    NF_CHECK_LAUNCH();
    return 0;
}
