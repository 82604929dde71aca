// Monotone rational-quadratic spline coupling (Durkan et al. 2019, "Neural Spline Flows"): split + spline + merge + log-det in one launch
// per direction, the closed-form inverse (one quadratic solve) and the analytic backward.  The element arithmetic is nf_rqs_elem.h.
//
// params is the conditioner output (B, (3K-1)*Ch, h, w): parameter p of half-element e = (m*h+i)*w+j of sample b at
// params[b*PS + p*nh + e], nh = Ch*h*w, PS = (3K-1)*nh (the convention of the mixture coupling: every parameter plane is contiguous in e).
//
// Two launch shapes per direction:
//   rows    vector data (h = w = 1) whose parameter row fits the LDS tile: ONE THREAD PER SAMPLE.  A workgroup's parameter rows are one
//           contiguous span of global memory; it is staged through LDS with coalesced accesses (row stride odd: conflict-free per-thread
//           reads), the backward overwrites its own row with the gradients and the tile leaves the same way.  The thread adds the log-det
//           terms of its sample's elements in order.
//   sample  everything else: ONE WORKGROUP PER SAMPLE walks the sample's elements (the parameter planes are coalesced along e), the
//           log-det terms are folded through the wave shuffles and LDS in a fixed order.  The backward has nothing to reduce (the
//           coupling has no parameters of its own): one thread per element over the whole batch.
// No float atomics anywhere: two runs give the same bits, and the deterministic mode has no case for this file.
#include "nf_common.h"
#include "nf_rqs_elem.h"

#define NF_RQS_TILE_WORDS 12288        // 48 KB of LDS per workgroup of the rows kernels

// odd row stride of the LDS tile
static inline int nf_rqs_stride(int PS) { return PS | 1; }
// threads (= rows) of a rows workgroup: 256, 128 or 64 so that the tile fits; 0: the row is too long for this form
static inline int nf_rqs_rows_threads(const NfSplit& s, int K) {
    if (s.h * s.w != 1) return 0;
    const int64_t RS = nf_rqs_stride((3 * K - 1) * s.n_half);
    for (int th = NF_BLOCK; th >= NF_WAVE; th >>= 1)
        if (th * RS <= NF_RQS_TILE_WORDS) return th;
    return 0;
}

// e / PS by a multiply: magic = ceil(2^32 / PS) is exact while e * PS < 2^32 (a tile holds at most NF_RQS_TILE_WORDS elements, PS <= 191;
// PS = (3K-1) Ch is never a power of two, so the magic fits 32 bits)
static inline unsigned nf_rqs_magic(int PS) { return (unsigned)((0x100000000ULL + (unsigned)PS - 1) / (unsigned)PS); }

// rows [row0, row0 + blockDim.x) of a (B, PS) tensor <-> the tile (row stride RS = PS or PS + 1).  The span is contiguous in global memory:
// 16-byte accesses when it is whole quads and aligned (every full tile of an aligned tensor), 4-byte accesses otherwise.  A quad starts in
// row r at column c and runs into the next row at most once (PS >= 11).
template <bool OUT>
__device__ __forceinline__ void nf_rqs_stage(float* __restrict__ g, float* __restrict__ tile, int64_t row0, int64_t B, int PS, int RS,
                                             unsigned magic) {
    if (OUT) __syncthreads();
    const int rows = (int)min((int64_t)blockDim.x, B - row0);
    const int total = rows * PS, pad = RS - PS;
    float* span = g + row0 * PS;
    if ((total & 3) == 0 && (reinterpret_cast<uintptr_t>(span) & 15) == 0) {
        for (int q = threadIdx.x; q < (total >> 2); q += blockDim.x) {
            const int e = 4 * q;
            const int r = (int)__umulhi((unsigned)e, magic), c = e - r * PS;
            const int i0 = r * RS + c;
            const int i1 = i0 + 1 + (c + 1 >= PS ? pad : 0), i2 = i0 + 2 + (c + 2 >= PS ? pad : 0), i3 = i0 + 3 + (c + 3 >= PS ? pad : 0);
            if (!OUT) {
                const float4 v = reinterpret_cast<const float4*>(span)[q];
                tile[i0] = v.x; tile[i1] = v.y; tile[i2] = v.z; tile[i3] = v.w;
            } else {
                float4 v;
                v.x = tile[i0]; v.y = tile[i1]; v.z = tile[i2]; v.w = tile[i3];
                reinterpret_cast<float4*>(span)[q] = v;
            }
        }
    } else {
        for (int e = threadIdx.x; e < total; e += blockDim.x) {
            const int r = (int)__umulhi((unsigned)e, magic);
            const int i = r * RS + (e - r * PS);
            if (!OUT) tile[i] = span[e];
            else span[e] = tile[i];
        }
    }
    __syncthreads();
}

// ---- forward / inverse ------------------------------------------------------------------------------------------------------------
template <int K, bool INV>
__global__ void __launch_bounds__(NF_BLOCK) k_rqs_rows(const float* __restrict__ z, const float* __restrict__ prm, float* __restrict__ y,
                                                       float* __restrict__ ld, NfSplit s, float bound, int64_t B, int RS, unsigned magic) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int PS = (3 * K - 1) * s.n_half;
    for (int64_t row0 = (int64_t)blockIdx.x * blockDim.x; row0 < B; row0 += (int64_t)gridDim.x * blockDim.x) {
        nf_rqs_stage<false>(const_cast<float*>(prm), tile, row0, B, PS, RS, magic);
        const int64_t b = row0 + threadIdx.x;
        if (b < B) {
            const float* zb = z + b * s.n_full;
            float* yb = y + b * s.n_full;
            const float* row = tile + threadIdx.x * RS;
            float acc = 0.f;
            for (int e = 0; e < s.n_half; ++e) {
                const int o0 = nf_half_to_full(s, 0, e), o1 = nf_half_to_full(s, 1, e);
                const float v = zb[o0];
                yb[o0] = nf_rqs_inside(v, bound) ? nf_rqs_elem<K, INV>(row + e, s.n_half, bound, v, acc) : v;
                yb[o1] = zb[o1];
            }
            ld[b] += acc;
        }
        __syncthreads();
    }
}

template <int K, bool INV>
__global__ void __launch_bounds__(NF_BLOCK) k_rqs_sample(const float* __restrict__ z, const float* __restrict__ prm, float* __restrict__ y,
                                                         float* __restrict__ ld, NfSplit s, float bound) {
    __shared__ float scratch[NF_BLOCK / NF_WAVE];
    const int64_t b = blockIdx.x;
    const float* zb = z + b * s.n_full;
    float* yb = y + b * s.n_full;
    const float* pb = prm + b * (3 * K - 1) * (int64_t)s.n_half;
    float acc = 0.f;
    for (int e = threadIdx.x; e < s.n_half; e += blockDim.x) {
        const int o0 = nf_half_to_full(s, 0, e), o1 = nf_half_to_full(s, 1, e);
        const float v = zb[o0];
        yb[o0] = nf_rqs_inside(v, bound) ? nf_rqs_elem<K, INV>(pb + e, s.n_half, bound, v, acc) : v;
        yb[o1] = zb[o1];
    }
    const float tot = nf_block_sum(acc, scratch);        // shuffle tree, then the waves in order: the same sum every run
    if (threadIdx.x == 0) ld[b] += tot;
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
template <int K>
__global__ void __launch_bounds__(NF_BLOCK) k_rqs_rows_bwd(const float* __restrict__ gy, const float* __restrict__ gld, const float* __restrict__ z,
                                                           const float* __restrict__ prm, float* __restrict__ gz, float* __restrict__ gprm,
                                                           NfSplit s, float bound, int64_t B, int RS, unsigned magic) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int PS = (3 * K - 1) * s.n_half;
    for (int64_t row0 = (int64_t)blockIdx.x * blockDim.x; row0 < B; row0 += (int64_t)gridDim.x * blockDim.x) {
        nf_rqs_stage<false>(const_cast<float*>(prm), tile, row0, B, PS, RS, magic);
        const int64_t b = row0 + threadIdx.x;
        if (b < B) {
            const int64_t fb = b * s.n_full;
            float* row = tile + threadIdx.x * RS;
            const float gl = gld[b];
            for (int e = 0; e < s.n_half; ++e) {
                const int o0 = nf_half_to_full(s, 0, e), o1 = nf_half_to_full(s, 1, e);
                // the gradients overwrite this element's own parameters in the tile (all of them are in registers before the first store)
                gz[fb + o0] = nf_rqs_bwd_elem<K>(row + e, s.n_half, row + e, s.n_half, bound, z[fb + o0], gy[fb + o0], gl);
                gz[fb + o1] = gy[fb + o1];
            }
        }
        nf_rqs_stage<true>(gprm, tile, row0, B, PS, RS, magic);
    }
}

template <int K>
__global__ void __launch_bounds__(NF_BLOCK) k_rqs_bwd(const float* __restrict__ gy, const float* __restrict__ gld, const float* __restrict__ z,
                                                      const float* __restrict__ prm, float* __restrict__ gz, float* __restrict__ gprm, NfSplit s,
                                                      float bound, int64_t total) {
    const int64_t PS = (int64_t)(3 * K - 1) * s.n_half;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / s.n_half;
        const int e = (int)(t - b * s.n_half);
        const int64_t fb = b * s.n_full;
        const int o0 = nf_half_to_full(s, 0, e), o1 = nf_half_to_full(s, 1, e);
        gz[fb + o0] = nf_rqs_bwd_elem<K>(prm + b * PS + e, s.n_half, gprm + b * PS + e, s.n_half, bound, z[fb + o0], gy[fb + o0], gld[b]);
        gz[fb + o1] = gy[fb + o1];
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static inline int nf_rqs_args(NfSplit& s, int K, float bound, int mode, int odd, int64_t B, int C, int H, int W) {
    if (K != 4 && K != 8 && K != 16) return NF_E_UNSUPPORTED;
    if (!(bound > 0.f) || B < 0 || B > 0x7fffffffLL || C < 1 || H < 1 || W < 1) return NF_E_BADARG;
    if (mode == NF_SPLIT_NONE || !nf_make_split(s, mode, odd, C, H, W)) return NF_E_BADARG;
    return 0;
}

#define NF_RQS_DISPATCH(K, CALL) \
    do {                         \
        if (K == 4) { CALL(4); } \
        else if (K == 8) { CALL(8); } \
        else { CALL(16); }       \
    } while (0)

extern "C" int nf_rqs_coupling_fwd(const float* z, const float* params, float* y, float* ld, int K, float bound, int mode, int odd, int inverse,
                                   int64_t B, int C, int H, int W, nf_stream_t stream) {
    NfSplit s;
    const int rc = nf_rqs_args(s, K, bound, mode, odd, B, C, H, W);
    if (rc != 0) return rc;
    if (B == 0 || s.n_half == 0) return 0;
    if (z == nullptr || params == nullptr || y == nullptr || ld == nullptr) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int th = nf_rqs_rows_threads(s, K);
    if (th > 0) {
        const int RS = nf_rqs_stride((3 * K - 1) * s.n_half);
        const unsigned magic = nf_rqs_magic((3 * K - 1) * s.n_half);
        const dim3 grid(nf_grid_for(B, th));
        const size_t lds = (size_t)th * RS * sizeof(float);
#define CALL(KT)                                                                                                             \
    if (inverse) hipLaunchKernelGGL((k_rqs_rows<KT, true>), grid, dim3(th), lds, st, z, params, y, ld, s, bound, B, RS, magic);      \
    else hipLaunchKernelGGL((k_rqs_rows<KT, false>), grid, dim3(th), lds, st, z, params, y, ld, s, bound, B, RS, magic)
        NF_RQS_DISPATCH(K, CALL);
#undef CALL
    } else {
        const int bt = min(NF_BLOCK, (s.n_half + NF_WAVE - 1) / NF_WAVE * NF_WAVE);
#define CALL(KT)                                                                                                             \
    if (inverse) hipLaunchKernelGGL((k_rqs_sample<KT, true>), dim3((unsigned)B), dim3(bt), 0, st, z, params, y, ld, s, bound); \
    else hipLaunchKernelGGL((k_rqs_sample<KT, false>), dim3((unsigned)B), dim3(bt), 0, st, z, params, y, ld, s, bound)
        NF_RQS_DISPATCH(K, CALL);
#undef CALL
    }
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_rqs_coupling_bwd(const float* g_y, const float* g_ld, const float* z, const float* params, float* g_z, float* g_params, int K,
                                   float bound, int mode, int odd, int64_t B, int C, int H, int W, nf_stream_t stream) {
    NfSplit s;
    const int rc = nf_rqs_args(s, K, bound, mode, odd, B, C, H, W);
    if (rc != 0) return rc;
    if (B == 0 || s.n_half == 0) return 0;
    if (g_y == nullptr || g_ld == nullptr || z == nullptr || params == nullptr || g_z == nullptr || g_params == nullptr) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int th = nf_rqs_rows_threads(s, K);
    if (th > 0) {
        const int RS = nf_rqs_stride((3 * K - 1) * s.n_half);
        const unsigned magic = nf_rqs_magic((3 * K - 1) * s.n_half);
        const dim3 grid(nf_grid_for(B, th));
        const size_t lds = (size_t)th * RS * sizeof(float);
#define CALL(KT) hipLaunchKernelGGL(k_rqs_rows_bwd<KT>, grid, dim3(th), lds, st, g_y, g_ld, z, params, g_z, g_params, s, bound, B, RS, magic)
        NF_RQS_DISPATCH(K, CALL);
#undef CALL
    } else {
        const int64_t total = B * s.n_half;
        const dim3 grid(nf_grid_for(total));
#define CALL(KT) hipLaunchKernelGGL(k_rqs_bwd<KT>, grid, dim3(NF_BLOCK), 0, st, g_y, g_ld, z, params, g_z, g_params, s, bound, total)
        NF_RQS_DISPATCH(K, CALL);
#undef CALL
    }
    NF_CHECK_LAUNCH();
    return 0;
}
