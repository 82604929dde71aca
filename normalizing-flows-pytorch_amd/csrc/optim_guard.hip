// The guarded optimizer step: global-norm gradient clipping (torch.nn.utils.clip_grad_norm_), a skip of the whole step when the
// gradient is not finite, and an exponential moving average of the parameters -- all inside the train step (main.py:78-92), with
// every decision taken on the device so that a captured hipGraph replays it without a host read.
//
//   nf_grad_guard            two launches over the flat gradient:
//       k_guard_partials     grid-stride sum of squares in float64, ONE partial per workgroup in a fixed slab (no atomics);
//       k_guard_finalise     one workgroup, after the kernel boundary that makes the slab visible: the partials are added in index
//                            order by one thread, then norm, clip scale and skip flag go into the control block and the counters
//                            tick -- the optimizer's step and ema_count on a step that is taken, `skipped` on one that is not.
//   nf_adam_step_guarded     k_adam_step's / nf_rmsprop_one's arithmetic (csrc/optim.hip) with grad_scale = ctl->clip_scale, nothing
//   nf_rmsprop_step_guarded  touched when ctl->skip is set, and the average updated in the same pass from the new parameter.
//   nf_adamax_step_guarded   the same for Adamax and AdamW (the element arithmetic of nf_optim_recipes.h, shared with csrc/optim.hip);
//   nf_adamw_step_guarded    a skipped AdamW step does not apply the decoupled decay either.
//   nf_swap_f32              in-place exchange of two flat buffers (the averaged weights into the parameters and back).
// The result of the reduction depends on n and on the gradient's 16-byte alignment alone: the grid, the elements a thread takes and
// the order of every addition are fixed by them, so two runs give the same bits whatever NF_DETERMINISTIC says.
#include <math.h>

#include "nf_common.h"
#include "nf_optim_recipes.h"

static inline unsigned nf_guard_grid(int64_t work_items) {
    int64_t g = (work_items + NF_BLOCK - 1) / NF_BLOCK;
    if (g < 1) g = 1;
    if (g > NF_GUARD_MAX_PARTIALS) g = NF_GUARD_MAX_PARTIALS;
    return (unsigned)g;
}

__device__ __forceinline__ double nf_sq(float x) { return (double)x * (double)x; }

template <bool VEC>
__global__ void __launch_bounds__(NF_BLOCK) k_guard_partials(const float* __restrict__ g, int64_t n, double* __restrict__ partials) {
    __shared__ double wave_sums[NF_BLOCK / NF_WAVE];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    int64_t done = 0;
    if (VEC) {
        const int64_t n4 = n / 4;
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        for (int64_t i = tid; i < n4; i += gstride) {
            const float4 v = g4[i];
            acc += (nf_sq(v.x) + nf_sq(v.y)) + (nf_sq(v.z) + nf_sq(v.w));
        }
        done = 4 * n4;
    }
    for (int64_t i = done + tid; i < n; i += gstride) acc += nf_sq(g[i]);
    // fixed-order block sum: lanes by shuffle, then the four wave sums by thread 0 in wave order
#pragma unroll
    for (int off = NF_WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, NF_WAVE);
    if ((threadIdx.x & (NF_WAVE - 1)) == 0) wave_sums[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sums[0];
        for (int w = 1; w < NF_BLOCK / NF_WAVE; ++w) s += wave_sums[w];
        partials[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(NF_BLOCK) k_guard_finalise(const double* __restrict__ partials, int n_partials, float max_norm,
                                                             int skip_nonfinite, nf_guard_ctl* __restrict__ ctl, int* __restrict__ step) {
    __shared__ double part[NF_GUARD_MAX_PARTIALS];
    for (int i = threadIdx.x; i < n_partials; i += blockDim.x) part[i] = partials[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < n_partials; ++i) sum += part[i];          // index order
    const double norm = sqrt(sum);
    const bool finite = isfinite(sum);
    double scale = 1.0;
    if (max_norm > 0.f) {                                         // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1)
        scale = (double)max_norm / (norm + 1.0e-6);
        if (scale > 1.0) scale = 1.0;                             // (a NaN stays a NaN, as torch's clamp leaves it)
    }
    const int skip = (skip_nonfinite != 0 && !finite) ? 1 : 0;
    ctl->grad_norm = (float)norm;
    ctl->clip_scale = (float)scale;
    ctl->skip = skip;
    if (skip) {
        ctl->skipped += 1;
    } else {
        if (step != nullptr) step[0] += 1;
        ctl->ema_count += 1;
    }
}

extern "C" int nf_grad_guard(const float* grad, int64_t n, float max_norm, int skip_nonfinite, double* partials, nf_guard_ctl* ctl,
                             int* step, nf_stream_t stream) {
    if (n < 0 || ctl == nullptr) return NF_E_BADARG;
    if (n == 0) return 0;
    if (grad == nullptr || partials == nullptr) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n >= 4 && ((uintptr_t)grad & 15) == 0;
    const unsigned grid = nf_guard_grid(vec ? n / 4 : n);
    if (vec)
        hipLaunchKernelGGL(k_guard_partials<true>, dim3(grid), dim3(NF_BLOCK), 0, st, grad, n, partials);
    else
        hipLaunchKernelGGL(k_guard_partials<false>, dim3(grid), dim3(NF_BLOCK), 0, st, grad, n, partials);
    NF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_guard_finalise, dim3(1), dim3(NF_BLOCK), 0, st, partials, (int)grid, max_norm, skip_nonfinite, ctl, step);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the guarded steps.  One element: the arithmetic of k_adam_step / nf_rmsprop_one, then the average from the NEW parameter.
// (optim.hip's device functions are local to its translation unit -- no -fgpu-rdc -- so the two expressions are restated here,
// operation for operation; tests/test_gpu_trainer_guard.py holds both to torch.optim at the bar the plain kernels meet.)
// ---------------------------------------------------------------------------------------------------------------
struct NfAdamConsts { float b1, b2, eps, wd, bc2_sqrt, step_size; };

__device__ __forceinline__ void nf_adam_one(float& p, float g, float& m, float& v, const NfAdamConsts& c, float grad_scale) {
    float gi = g * grad_scale;
    if (c.wd != 0.f) gi = fmaf(c.wd, p, gi);
    m = fmaf(c.b1, m, (1.f - c.b1) * gi);
    v = fmaf(c.b2, v, (1.f - c.b2) * gi * gi);
    p = p - c.step_size * (m / (sqrtf(v) / c.bc2_sqrt + c.eps));
}

__device__ __forceinline__ void nf_rmsprop_one_g(float& p, float g, float& v, float lr, float alpha, float eps, float wd,
                                                 float grad_scale) {
    float gi = g * grad_scale;
    if (wd != 0.f) gi = fmaf(wd, p, gi);
    v = fmaf(alpha, v, (1.f - alpha) * gi * gi);
    p = p - lr * (gi / (sqrtf(v) + eps));
}

// ema = p_new on the first update that is taken (ActNorm initialises in the first forward), d ema + (1 - d) p_new afterwards
__device__ __forceinline__ float nf_ema_one(float e, float p, float d, bool first) { return first ? p : fmaf(d, e, (1.f - d) * p); }

template <bool VEC, bool EMA>
__global__ void __launch_bounds__(NF_BLOCK) k_adam_step_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, const int* __restrict__ step,
                                                                const float* __restrict__ lr, float b1, float b2, float eps, float wd,
                                                                const nf_guard_ctl* __restrict__ ctl, float* __restrict__ ema,
                                                                float ema_decay, int64_t n) {
    if (ctl->skip != 0) return;                                    // uniform over the grid: nothing is touched
    const float grad_scale = ctl->clip_scale;
    const bool first = ctl->ema_count == 1;
    const float t = (float)step[0];
    NfAdamConsts c;
    c.b1 = b1; c.b2 = b2; c.eps = eps; c.wd = wd;
    c.bc2_sqrt = sqrtf(1.f - powf(b2, t));
    c.step_size = lr[0] / (1.f - powf(b1, t));
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if (VEC) {
        const int64_t n4 = n / 4;
        float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
        float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
        float4* __restrict__ e4 = reinterpret_cast<float4*>(ema);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        for (int64_t i = tid; i < n4; i += gstride) {
            float4 pi = p4[i], mi = m4[i], vi = v4[i];
            const float4 gi = g4[i];
            nf_adam_one(pi.x, gi.x, mi.x, vi.x, c, grad_scale);
            nf_adam_one(pi.y, gi.y, mi.y, vi.y, c, grad_scale);
            nf_adam_one(pi.z, gi.z, mi.z, vi.z, c, grad_scale);
            nf_adam_one(pi.w, gi.w, mi.w, vi.w, c, grad_scale);
            m4[i] = mi;
            v4[i] = vi;
            p4[i] = pi;
            if (EMA) {
                float4 ei = pi;
                if (!first) {
                    ei = e4[i];
                    ei.x = nf_ema_one(ei.x, pi.x, ema_decay, false);
                    ei.y = nf_ema_one(ei.y, pi.y, ema_decay, false);
                    ei.z = nf_ema_one(ei.z, pi.z, ema_decay, false);
                    ei.w = nf_ema_one(ei.w, pi.w, ema_decay, false);
                }
                e4[i] = ei;
            }
        }
        done = 4 * n4;
    }
    for (int64_t i = done + tid; i < n; i += gstride) {
        float pi = p[i], mi = m[i], vi = v[i];
        nf_adam_one(pi, g[i], mi, vi, c, grad_scale);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        if (EMA) ema[i] = first ? pi : nf_ema_one(ema[i], pi, ema_decay, false);
    }
}

template <bool VEC, bool EMA>
__global__ void __launch_bounds__(NF_BLOCK) k_rmsprop_step_guarded(float* __restrict__ p, const float* __restrict__ g,
                                                                   float* __restrict__ v, const float* __restrict__ lr_ptr, float alpha,
                                                                   float eps, float wd, const nf_guard_ctl* __restrict__ ctl,
                                                                   float* __restrict__ ema, float ema_decay, int64_t n) {
    if (ctl->skip != 0) return;
    const float grad_scale = ctl->clip_scale;
    const bool first = ctl->ema_count == 1;
    const float lr = lr_ptr[0];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if (VEC) {
        const int64_t n4 = n / 4;
        float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
        float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
        float4* __restrict__ e4 = reinterpret_cast<float4*>(ema);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        for (int64_t i = tid; i < n4; i += gstride) {
            float4 pi = p4[i], vi = v4[i];
            const float4 gi = g4[i];
            nf_rmsprop_one_g(pi.x, gi.x, vi.x, lr, alpha, eps, wd, grad_scale);
            nf_rmsprop_one_g(pi.y, gi.y, vi.y, lr, alpha, eps, wd, grad_scale);
            nf_rmsprop_one_g(pi.z, gi.z, vi.z, lr, alpha, eps, wd, grad_scale);
            nf_rmsprop_one_g(pi.w, gi.w, vi.w, lr, alpha, eps, wd, grad_scale);
            v4[i] = vi;
            p4[i] = pi;
            if (EMA) {
                float4 ei = pi;
                if (!first) {
                    ei = e4[i];
                    ei.x = nf_ema_one(ei.x, pi.x, ema_decay, false);
                    ei.y = nf_ema_one(ei.y, pi.y, ema_decay, false);
                    ei.z = nf_ema_one(ei.z, pi.z, ema_decay, false);
                    ei.w = nf_ema_one(ei.w, pi.w, ema_decay, false);
                }
                e4[i] = ei;
            }
        }
        done = 4 * n4;
    }
    for (int64_t i = done + tid; i < n; i += gstride) {
        float pi = p[i], vi = v[i];
        nf_rmsprop_one_g(pi, g[i], vi, lr, alpha, eps, wd, grad_scale);
        v[i] = vi;
        p[i] = pi;
        if (EMA) ema[i] = first ? pi : nf_ema_one(ema[i], pi, ema_decay, false);
    }
}

static inline bool nf_all_aligned16(const void* a, const void* b, const void* c, const void* d, const void* e) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;       // (NULL counts as aligned)
}

extern "C" int nf_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int* step,
                                    const float* lr, float beta1, float beta2, float eps, float weight_decay, const nf_guard_ctl* ctl,
                                    float* ema, float ema_decay, int64_t n, nf_stream_t stream) {
    if (n < 0 || ctl == nullptr) return NF_E_BADARG;
    if (n == 0) return 0;
    if (param == nullptr || grad == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr || step == nullptr || lr == nullptr)
        return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n >= 4 && nf_all_aligned16(param, grad, exp_avg, exp_avg_sq, ema);
    const dim3 grid(nf_grid_for(vec ? n / 4 : n)), block(NF_BLOCK);
#define NF_LAUNCH_ADAM_G(V, E)                                                                                                       \
    hipLaunchKernelGGL((k_adam_step_guarded<V, E>), grid, block, 0, st, param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, \
                       weight_decay, ctl, ema, ema_decay, n)
    if (vec) {
        if (ema != nullptr) NF_LAUNCH_ADAM_G(true, true); else NF_LAUNCH_ADAM_G(true, false);
    } else {
        if (ema != nullptr) NF_LAUNCH_ADAM_G(false, true); else NF_LAUNCH_ADAM_G(false, false);
    }
#undef NF_LAUNCH_ADAM_G
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_rmsprop_step_guarded(float* param, const float* grad, float* square_avg, const float* lr, float alpha, float eps,
                                       float weight_decay, const nf_guard_ctl* ctl, float* ema, float ema_decay, int64_t n,
                                       nf_stream_t stream) {
    if (n < 0 || ctl == nullptr) return NF_E_BADARG;
    if (n == 0) return 0;
    if (param == nullptr || grad == nullptr || square_avg == nullptr || lr == nullptr) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n >= 4 && nf_all_aligned16(param, grad, square_avg, ema, nullptr);
    const dim3 grid(nf_grid_for(vec ? n / 4 : n)), block(NF_BLOCK);
#define NF_LAUNCH_RMS_G(V, E)                                                                                                       \
    hipLaunchKernelGGL((k_rmsprop_step_guarded<V, E>), grid, block, 0, st, param, grad, square_avg, lr, alpha, eps, weight_decay, ctl, \
                       ema, ema_decay, n)
    if (vec) {
        if (ema != nullptr) NF_LAUNCH_RMS_G(true, true); else NF_LAUNCH_RMS_G(true, false);
    } else {
        if (ema != nullptr) NF_LAUNCH_RMS_G(false, true); else NF_LAUNCH_RMS_G(false, false);
    }
#undef NF_LAUNCH_RMS_G
    NF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the guarded Adamax and AdamW steps: the element arithmetic of nf_optim_recipes.h (what k_recipe_step of csrc/optim.hip runs) in
// the template shape of the two kernels above.  A skipped step touches nothing -- AdamW's decoupled decay included: it is part of
// the element's update, behind the same early return.
// ---------------------------------------------------------------------------------------------------------------
template <bool VEC, bool EMA, class R>
__global__ void __launch_bounds__(NF_BLOCK) k_recipe_step_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                  float* __restrict__ s, const int* __restrict__ step,
                                                                  const float* __restrict__ lr, NfRecipeHyper h,
                                                                  const nf_guard_ctl* __restrict__ ctl, float* __restrict__ ema,
                                                                  float ema_decay, int64_t n) {
    if (ctl->skip != 0) return;                                    // uniform over the grid: nothing is touched
    const float grad_scale = ctl->clip_scale;
    const bool first = ctl->ema_count == 1;
    const typename R::Consts c = R::consts(step, lr, h);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if (VEC) {
        const int64_t n4 = n / 4;
        float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
        float4* __restrict__ s4 = reinterpret_cast<float4*>(s);
        float4* __restrict__ e4 = reinterpret_cast<float4*>(ema);
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
            if (EMA) {
                float4 ei = pi;
                if (!first) {
                    ei = e4[i];
                    ei.x = nf_ema_one(ei.x, pi.x, ema_decay, false);
                    ei.y = nf_ema_one(ei.y, pi.y, ema_decay, false);
                    ei.z = nf_ema_one(ei.z, pi.z, ema_decay, false);
                    ei.w = nf_ema_one(ei.w, pi.w, ema_decay, false);
                }
                e4[i] = ei;
            }
        }
        done = 4 * n4;
    }
    for (int64_t i = done + tid; i < n; i += gstride) {
        float pi = p[i], mi = m[i], si = s[i];
        R::one(pi, g[i], mi, si, c, grad_scale);
        m[i] = mi;
        s[i] = si;
        p[i] = pi;
        if (EMA) ema[i] = first ? pi : nf_ema_one(ema[i], pi, ema_decay, false);
    }
}

template <class R>
static int nf_recipe_step_guarded(float* param, const float* grad, float* m, float* s, const int* step, const float* lr, float beta1,
                                  float beta2, float eps, float weight_decay, const nf_guard_ctl* ctl, float* ema, float ema_decay,
                                  int64_t n, nf_stream_t stream) {
    if (n < 0 || ctl == nullptr) return NF_E_BADARG;
    if (n == 0) return 0;
    if (param == nullptr || grad == nullptr || m == nullptr || s == nullptr || step == nullptr || lr == nullptr) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n >= 4 && nf_all_aligned16(param, grad, m, s, ema);
    const dim3 grid(nf_grid_for(vec ? n / 4 : n)), block(NF_BLOCK);
    const NfRecipeHyper h = nf_recipe_hyper(beta1, beta2, eps, weight_decay);
#define NF_LAUNCH_RECIPE_G(V, E) \
    hipLaunchKernelGGL((k_recipe_step_guarded<V, E, R>), grid, block, 0, st, param, grad, m, s, step, lr, h, ctl, ema, ema_decay, n)
    if (vec) {
        if (ema != nullptr) NF_LAUNCH_RECIPE_G(true, true); else NF_LAUNCH_RECIPE_G(true, false);
    } else {
        if (ema != nullptr) NF_LAUNCH_RECIPE_G(false, true); else NF_LAUNCH_RECIPE_G(false, false);
    }
#undef NF_LAUNCH_RECIPE_G
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_adamax_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_inf, const int* step, const float* lr,
                                      float beta1, float beta2, float eps, float weight_decay, const nf_guard_ctl* ctl, float* ema,
                                      float ema_decay, int64_t n, nf_stream_t stream) {
    return nf_recipe_step_guarded<NfAdamax>(param, grad, exp_avg, exp_inf, step, lr, beta1, beta2, eps, weight_decay, ctl, ema, ema_decay,
                                            n, stream);
}

extern "C" int nf_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int* step, const float* lr,
                                     float beta1, float beta2, float eps, float weight_decay, const nf_guard_ctl* ctl, float* ema,
                                     float ema_decay, int64_t n, nf_stream_t stream) {
    return nf_recipe_step_guarded<NfAdamW>(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, ctl, ema,
                                           ema_decay, n, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// a <-> b over n floats, in place: every element is read into registers from both sides before either side is written, and no
// element is touched by two threads, so the buffers need no temporary.  They must not overlap.
// ---------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(NF_BLOCK) k_swap_f32(float* __restrict__ a, float* __restrict__ b, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if (VEC) {
        const int64_t n4 = n / 4;
        float4* __restrict__ a4 = reinterpret_cast<float4*>(a);
        float4* __restrict__ b4 = reinterpret_cast<float4*>(b);
        for (int64_t i = tid; i < n4; i += gstride) {
            const float4 x = a4[i], y = b4[i];
            a4[i] = y;
            b4[i] = x;
        }
        done = 4 * n4;
    }
    for (int64_t i = done + tid; i < n; i += gstride) {
        const float x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

extern "C" int nf_swap_f32(float* a, float* b, int64_t n, nf_stream_t stream) {
    if (n < 0) return NF_E_BADARG;
    if (n == 0) return 0;
    if (a == nullptr || b == nullptr) return NF_E_BADARG;
    if (a == b) return 0;
    if ((a < b && a + n > b) || (b < a && b + n > a)) return NF_E_BADARG;       // overlapping ranges
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n >= 4 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_swap_f32<true>, dim3(nf_grid_for(n / 4)), dim3(NF_BLOCK), 0, st, a, b, n);
    else
        hipLaunchKernelGGL(k_swap_f32<false>, dim3(nf_grid_for(n)), dim3(NF_BLOCK), 0, st, a, b, n);
    NF_CHECK_LAUNCH();
    return 0;
}
