// Log-likelihood accumulator of a held-out sweep (main.py:121-127: log p(y) = log N(z; 0, I) + log|det J|, there for one host batch):
//   log p(y_b) = -1/2 |z_b|^2 - 1/2 D log(2 pi) + ld_b      from float32 z (B, D) and ld (B)
// with the row's sum of squares and log p itself in FLOAT64 -- the pass is bandwidth-bound and fp64 FMA runs at full rate on gfx950, so
// no summation-order term enters a tolerance.  Two launches in stream order, no spin loop, no float atomic, no grid exchange:
//   k_logp_rows   one thread per row for D <= 4; above, one wave per row: lane-strided float64 partials, a fixed xor tree
//   k_logp_fold   ONE workgroup: reads the device step, valid = clamp(N - ((step % S) * stride + offset), 0, B) (the sweep schedule of
//                 dataset.hip), sums rows < valid in a fixed order (thread t takes rows t, t + 256, ...; a fixed LDS tree) and adds
//                 {sum log p, sum (log p)^2, count} to acc[3]; optionally files the step's rows at rows_all[(step % S) * B + j]
// Every order is fixed, so two runs give the same bits in either NF_DETERMINISTIC mode.
#include "nf_common.h"

#define NF_LOG_2PI 1.8378770664093454835606594728112

__device__ __forceinline__ double nf_wave_xor_sum(double v) {
#pragma unroll
    for (int off = NF_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, NF_WAVE);
    return v;
}

__global__ void __launch_bounds__(NF_BLOCK) k_logp_rows(const float* __restrict__ z, const float* __restrict__ ld, double* __restrict__ logp,
                                                        float* __restrict__ logp_f32, int64_t B, int64_t D) {
    const double c = -0.5 * (double)D * NF_LOG_2PI;
    if (D <= 4) {
        const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
        for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gstride) {
            double ss = 0.0;
            for (int64_t d = 0; d < D; ++d) {
                const double v = (double)z[b * D + d];
                ss += v * v;
            }
            const double lp = -0.5 * ss + c + (double)ld[b];
            logp[b] = lp;
            if (logp_f32 != nullptr) logp_f32[b] = (float)lp;
        }
        return;
    }
    const int lane = threadIdx.x & (NF_WAVE - 1), waves = NF_BLOCK / NF_WAVE;
    for (int64_t b = (int64_t)blockIdx.x * waves + (threadIdx.x >> 6); b < B; b += (int64_t)gridDim.x * waves) {
        const float* __restrict__ row = z + b * D;
        double ss = 0.0;
        for (int64_t d = lane; d < D; d += NF_WAVE) {
            const double v = (double)row[d];
            ss += v * v;
        }
        ss = nf_wave_xor_sum(ss);
        if (lane == 0) {
            const double lp = -0.5 * ss + c + (double)ld[b];
            logp[b] = lp;
            if (logp_f32 != nullptr) logp_f32[b] = (float)lp;
        }
    }
}

__global__ void __launch_bounds__(NF_BLOCK) k_logp_fold(const double* __restrict__ logp, double* __restrict__ rows_all,
                                                        double* __restrict__ acc, int64_t B, int64_t N, int64_t stride, int64_t offset,
                                                        int64_t S, const int64_t* __restrict__ step_ptr) {
    __shared__ double s_a[NF_BLOCK], s_b[NF_BLOCK];
    const unsigned long long step = step_ptr != nullptr ? (unsigned long long)step_ptr[0] : 0ull;
    const int64_t k = (int64_t)(step % (unsigned long long)S);
    int64_t valid = N - (k * stride + offset);
    valid = valid < 0 ? 0 : (valid > B ? B : valid);
    double a = 0.0, b = 0.0;
    for (int64_t j = threadIdx.x; j < valid; j += NF_BLOCK) {
        const double v = logp[j];
        a += v;
        b += v * v;
    }
    if (rows_all != nullptr)
        for (int64_t j = threadIdx.x; j < B; j += NF_BLOCK) rows_all[k * B + j] = logp[j];
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
#pragma unroll
    for (int w = NF_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_a[threadIdx.x] += s_a[threadIdx.x + w];
            s_b[threadIdx.x] += s_b[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {                               // the one writer of acc: launches on one stream are ordered
        acc[0] += s_a[0];
        acc[1] += s_b[0];
        acc[2] += (double)valid;
    }
}

extern "C" int nf_logp_accumulate(const float* z, const float* ld, double* logp_row, float* logp_f32, double* rows_all, double* acc,
                                  int64_t B, int64_t D, int64_t N, int64_t stride, int64_t offset, const int64_t* step,
                                  nf_stream_t stream) {
    if (z == nullptr || ld == nullptr || logp_row == nullptr || acc == nullptr) return NF_E_BADARG;
    if (B <= 0 || D <= 0 || N <= 0 || N >= ((int64_t)1 << 31) || stride <= 0 || stride >= ((int64_t)1 << 31) || offset < 0 ||
        offset + B > stride)
        return NF_E_BADARG;
    const int64_t S = (N + stride - 1) / stride;
    hipLaunchKernelGGL(k_logp_rows, dim3(D <= 4 ? nf_grid_for(B) : nf_grid_for(B, NF_BLOCK / NF_WAVE)), dim3(NF_BLOCK), 0,
                       (hipStream_t)stream, z, ld, logp_row, logp_f32, B, D);
    NF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_logp_fold, dim3(1), dim3(NF_BLOCK), 0, (hipStream_t)stream, logp_row, rows_all, acc, B, N, stride, offset, S, step);
    NF_CHECK_LAUNCH();
    return 0;
}
