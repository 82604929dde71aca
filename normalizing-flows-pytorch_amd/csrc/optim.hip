// Fused Adam over flat parameter / gradient / moment buffers: the whole optimizer step is ONE launch (+ a 1-thread
// step-counter bump), instead of the thousands of per-parameter scalar kernels a capturable framework Adam issues for
// the ~1100 small tensors of a 32-step flow.  Semantics = torch.optim.Adam (no amsgrad), which is what the reference
// trains with (main.py:56-64, configs/default.yaml:13-20):
//   g += wd * p ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// `step` and `lr` live in device memory so that a captured hipGraph replays with the right values.
// Below it: the same for RMSprop (nf_rmsprop_step), Adamax and AdamW (nf_adamax_step, nf_adamw_step), and the schedules as one-thread
// launches: StepLR (nf_lr_step_decay) and linear warmup times constant / step / cosine decay (nf_lr_schedule).
#include <math.h>

#include "nf_common.h"
#include "nf_optim_recipes.h"

__global__ void k_adam_tick(int* __restrict__ step) { step[0] += 1; }

__global__ void __launch_bounds__(NF_BLOCK) k_adam_step(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        const int* __restrict__ step, const float* __restrict__ lr,
                                                        float b1, float b2, float eps, float wd, float grad_scale,
                                                        int64_t n) {
    const float t = (float)step[0];
    const float bc1 = 1.f - powf(b1, t);
    const float bc2_sqrt = sqrtf(1.f - powf(b2, t));
    const float step_size = lr[0] / bc1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float gi = g[i] * grad_scale;
        const float pi = p[i];
        if (wd != 0.f) gi = fmaf(wd, pi, gi);
        const float mi = fmaf(b1, m[i], (1.f - b1) * gi);
        const float vi = fmaf(b2, v[i], (1.f - b2) * gi * gi);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    }
}

extern "C" int nf_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int* step,
                            const float* lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                            int64_t n, nf_stream_t stream) {
    if (n < 0) return NF_E_BADARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, st, step);
    NF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_adam_step, dim3(nf_grid_for(n)), dim3(NF_BLOCK), 0, st, param, grad, exp_avg, exp_avg_sq, step, lr,
                       beta1, beta2, eps, weight_decay, grad_scale, n);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Fused RMSprop over the same flat buffers: torch.optim.RMSprop with momentum = 0 and centered = False, the only form the
// reference constructs (main.py:56-59):
//   g += wd * p ; v = alpha v + (1 - alpha) g^2 ; p -= lr * g / (sqrt(v) + eps)
// A pure stream, 12 B read and 8 B written per element.  Where the three flat buffers and the gradient are 16-byte aligned the
// body moves float4s (VEC) and the last n % 4 elements take the scalar form in the same launch; otherwise every element does.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void nf_rmsprop_one(float& p, float g, float& v, float lr, float alpha, float eps, float wd,
                                               float grad_scale) {
    float gi = g * grad_scale;
    if (wd != 0.f) gi = fmaf(wd, p, gi);
    v = fmaf(alpha, v, (1.f - alpha) * gi * gi);
    p = p - lr * (gi / (sqrtf(v) + eps));
}

template <bool VEC>
__global__ void __launch_bounds__(NF_BLOCK) k_rmsprop_step(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ v, const float* __restrict__ lr_ptr, float alpha,
                                                           float eps, float wd, float grad_scale, int64_t n) {
    const float lr = lr_ptr[0];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;                                     // elements [0, done) are covered by the float4 body
    if (VEC) {
        const int64_t n4 = n / 4;
        float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
        float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        for (int64_t i = tid; i < n4; i += gstride) {
            float4 pi = p4[i], vi = v4[i];
            const float4 gi = g4[i];
            nf_rmsprop_one(pi.x, gi.x, vi.x, lr, alpha, eps, wd, grad_scale);
            nf_rmsprop_one(pi.y, gi.y, vi.y, lr, alpha, eps, wd, grad_scale);
            nf_rmsprop_one(pi.z, gi.z, vi.z, lr, alpha, eps, wd, grad_scale);
            nf_rmsprop_one(pi.w, gi.w, vi.w, lr, alpha, eps, wd, grad_scale);
            v4[i] = vi;
            p4[i] = pi;
        }
        done = 4 * n4;
    }
    for (int64_t i = done + tid; i < n; i += gstride) {
        float pi = p[i], vi = v[i];
        nf_rmsprop_one(pi, g[i], vi, lr, alpha, eps, wd, grad_scale);
        v[i] = vi;
        p[i] = pi;
    }
}

extern "C" int nf_rmsprop_step(float* param, const float* grad, float* square_avg, int* step, const float* lr, float alpha,
                               float eps, float weight_decay, float grad_scale, int64_t n, nf_stream_t stream) {
    if (n < 0) return NF_E_BADARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, st, step);
    NF_CHECK_LAUNCH();
    const bool vec = n >= 4 && (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)square_avg) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_rmsprop_step<true>, dim3(nf_grid_for(n / 4)), dim3(NF_BLOCK), 0, st, param, grad, square_avg, lr, alpha,
                           eps, weight_decay, grad_scale, n);
    else
        hipLaunchKernelGGL(k_rmsprop_step<false>, dim3(nf_grid_for(n)), dim3(NF_BLOCK), 0, st, param, grad, square_avg, lr, alpha,
                           eps, weight_decay, grad_scale, n);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Fused Adamax and AdamW over the same flat buffers (torch.optim.Adamax, torch.optim.AdamW; the reference's optimizer switch,
// main.py:56-66, names neither -- Adamax is what Glow trains with, decoupled decay what the weight-normed conditioners want).
// The element's arithmetic is nf_optim_recipes.h; both are 28-byte-per-element streams like k_adam_step (16 B read, 12 B written)
// in k_rmsprop_step's shape: float4 lanes with the scalar tail in the same launch where all four buffers sit on 16 bytes.
// ---------------------------------------------------------------------------------------------------------------
template <bool VEC, class R>
__global__ void __launch_bounds__(NF_BLOCK) k_recipe_step(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ s, const int* __restrict__ step,
                                                          const float* __restrict__ lr, NfRecipeHyper h, float grad_scale, int64_t n) {
    const typename R::Consts c = R::consts(step, lr, h);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;                                     // elements [0, done) are covered by the float4 body
    if (VEC) {
        const int64_t n4 = n / 4;
        float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
        float4* __restrict__ s4 = reinterpret_cast<float4*>(s);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        for (int64_t i = tid; i < n4; i += gstride) {
            float4 pi = p4[i], mi = m4[i], si = s4[i];
            const float4 gi = g4[i];
            R::one(pi.x, gi.x, mi.x, si.x, c, grad_scale);
            R::one(pi.y, gi.y, mi.y, si.y, c, grad_scale);
            R::one(pi.z, gi.z, mi.z, si.z, c, grad_scale);
            R::one(pi.w, gi.w, mi.w, si.w, c, grad_scale);
            m4[i] = mi;
            s4[i] = si;
            p4[i] = pi;
        }
        done = 4 * n4;
    }
    for (int64_t i = done + tid; i < n; i += gstride) {
        float pi = p[i], mi = m[i], si = s[i];
        R::one(pi, g[i], mi, si, c, grad_scale);
        m[i] = mi;
        s[i] = si;
        p[i] = pi;
    }
}

template <class R>
static int nf_recipe_step(float* param, const float* grad, float* m, float* s, int* step, const float* lr, float beta1, float beta2,
                          float eps, float weight_decay, float grad_scale, int64_t n, nf_stream_t stream) {
    if (n < 0) return NF_E_BADARG;
    if (n == 0) return 0;
    if (param == nullptr || grad == nullptr || m == nullptr || s == nullptr || step == nullptr || lr == nullptr) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, st, step);
    NF_CHECK_LAUNCH();
    const bool vec = n >= 4 && (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)s) & 15) == 0;
    const NfRecipeHyper h = nf_recipe_hyper(beta1, beta2, eps, weight_decay);
    if (vec)
        hipLaunchKernelGGL((k_recipe_step<true, R>), dim3(nf_grid_for(n / 4)), dim3(NF_BLOCK), 0, st, param, grad, m, s, step, lr, h,
                           grad_scale, n);
    else
        hipLaunchKernelGGL((k_recipe_step<false, R>), dim3(nf_grid_for(n)), dim3(NF_BLOCK), 0, st, param, grad, m, s, step, lr, h,
                           grad_scale, n);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_adamax_step(float* param, const float* grad, float* exp_avg, float* exp_inf, int* step, const float* lr, float beta1,
                              float beta2, float eps, float weight_decay, float grad_scale, int64_t n, nf_stream_t stream) {
    return nf_recipe_step<NfAdamax>(param, grad, exp_avg, exp_inf, step, lr, beta1, beta2, eps, weight_decay, grad_scale, n, stream);
}

extern "C" int nf_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int* step, const float* lr, float beta1,
                             float beta2, float eps, float weight_decay, float grad_scale, int64_t n, nf_stream_t stream) {
    return nf_recipe_step<NfAdamW>(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, grad_scale, n, stream);
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
