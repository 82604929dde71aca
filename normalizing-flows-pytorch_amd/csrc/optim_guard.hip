// What the guarded optimizer step needs beside the step itself: global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) and the
// skip of the whole step when the gradient is not finite, decided on the device so that a captured hipGraph replays the decision without
// a host read (main.py:78-92 has neither), and the exchange that puts the averaged weights to use.
//
//   nf_grad_guard            two launches over the flat gradient:
//       k_guard_partials     grid-stride sum of squares in float64, ONE partial per workgroup in a fixed slab (no atomics);
//       k_guard_finalise     one workgroup, after the kernel boundary that makes the slab visible: the partials are added in index
//                            order by one thread, then norm, clip scale and skip flag go into the control block and the counters
//                            tick -- the optimizer's step and ema_count on a step that is taken, `skipped` on one that is not.
//   nf_swap_f32              in-place exchange of two flat buffers (the averaged weights into the parameters and back).
// The steps that read the control block, nf_X_step_guarded, are the guarded modes of the one kernel body of csrc/optim.hip.
// The result of the reduction depends on n and on the gradient's 16-byte alignment alone: the grid, the elements a thread takes and
// the order of every addition are fixed by them, so two runs give the same bits whatever NF_DETERMINISTIC says.
#include <math.h>

#include "nf_common.h"

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
