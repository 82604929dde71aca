// Autoregressive spline head: the masked output layer of a MADE-style conditioner fused with the rational-quadratic spline it
// parameterises (the masked-autoregressive form of Neural Spline Flows, Durkan et al. 2019).  The (B, (3K-1) D) parameter tensor and its
// gradient are never written to memory: a thread forms the 3K-1 parameters of one feature of its row from the row's hidden vector,
// applies the spline at once (nf_rqs_elem.h, unchanged), and in the backward turns the parameter gradients straight into g_a and into
// the workgroup's weight- and bias-gradient slabs.
//
//     P[p] = bias[p D + d] + sum_i a[i] weight[p D + d, i] mask[d, i],     y_d = rqs(z_d; P),     ld += log dy_d / dz_d
//
// Launch shape: ONE THREAD PER ROW, NF_ARS_ROWS rows per workgroup, grid-stride over the row tiles.  Per tile the hidden rows are staged
// through LDS (coalesced global accesses, row stride 33: conflict-free per-thread reads) and stay there; per feature the workgroup stages
// that feature's masked weight rows TRANSPOSED, wT[i][p] (row stride 3K: whole 16-byte reads along p, the same address in every lane -- a
// broadcast), so the LDS footprint does not depend on D.  The thread's 3K-1 parameters are a fully unrolled local array (registers),
// which is what the element functions read (P[p * 1]); the loop over the 32 hidden units is NOT unrolled (it walks LDS, not a
// register array): unrolled, the compiler scheduled all 32 rows' reads and FMA chains together and K = 16 went to scratch.
//
// Backward: the element function writes the parameter gradients into a second local array; the thread leaves them in an LDS tile (row
// stride 3K-1, odd) and adds g_a[i] += sum_p gP[p] wT[i][p] into its row of a g_a tile, which leaves coalesced.  An element in a linear
// tail skips all of that (zeros in the tile, g_z = g_y).  The weight gradient of the feature is the (3K-1) x rows by rows x 32 product of
// the gradient tile with the hidden tile: plain fp32 FMAs, thread t owns column i = t & 31 and the rows r = (t >> 5), (t >> 5) + 4, ...:
// one hidden value and 3K/4 16-byte reads of the gradient row (the same address in 32 lanes) feed 3K FMAs; the four row groups' partial
// sums meet in LDS (the gradient tile's own words) and are added in group order.  Element o of the block is added to the workgroup's
// slab by thread o % 128 (written by the first tile, read back and added to by the same thread for the later ones: no other thread ever
// touches it).  nf_slab_sum folds the slabs in slab order.  No float atomics anywhere: two runs give the same bits, and the
// deterministic mode has no case for this file.
#include "nf_common.h"
#include "nf_rqs_elem.h"

#define NF_ARS_H 32                       // hidden width the kernels are built for
#define NF_ARS_AS (NF_ARS_H + 1)          // row stride of the hidden tile

static_assert(NF_ARS_ROWS == 128, "the weight-gradient product maps 128 threads to 32 columns x 4 row groups");

// rows [row0, row0 + rows) of the (B, 32) tensor g <-> the hidden tile
template <bool OUT>
__device__ __forceinline__ void nf_ars_rows(float* __restrict__ g, float* __restrict__ at, int64_t row0, int rows) {
    float* span = g + row0 * NF_ARS_H;
    for (int e = threadIdx.x; e < rows * NF_ARS_H; e += NF_ARS_ROWS) {
        const int i = (e >> 5) * NF_ARS_AS + (e & (NF_ARS_H - 1));
        if (!OUT) at[i] = span[e];
        else span[e] = at[i];
    }
}

// feature d's masked weight rows, transposed: wT[i * PSP + p] = weight[p D + d, i] mask[d, i] (column PS is padding), bt[p] = bias[p D + d]
template <int K>
__device__ __forceinline__ void nf_ars_stage(const float* __restrict__ weight, const float* __restrict__ bias, const float* __restrict__ mask,
                                             int D, int d, float* __restrict__ wT, float* __restrict__ bt) {
    constexpr int PS = 3 * K - 1, PSP = PS + 1;
    for (int e = threadIdx.x; e < PS * NF_ARS_H; e += NF_ARS_ROWS) {
        const int p = e >> 5, i = e & (NF_ARS_H - 1);
        wT[i * PSP + p] = weight[(int64_t)(p * D + d) * NF_ARS_H + i] * mask[d * NF_ARS_H + i];
    }
    if (threadIdx.x < NF_ARS_H) wT[threadIdx.x * PSP + PS] = 0.f;
    if (threadIdx.x < PSP) bt[threadIdx.x] = threadIdx.x < PS ? bias[threadIdx.x * D + d] : 0.f;
}

// P[p] = bt[p] + sum_i a[i] wT[i][p], the terms added in the order of i
template <int K>
__device__ __forceinline__ void nf_ars_params(const float* a, const float* wT, const float* bt, float (&P)[3 * K - 1]) {
    constexpr int PS = 3 * K - 1, PSP = PS + 1;
#pragma unroll
    for (int p = 0; p < PS; ++p) P[p] = bt[p];
#pragma unroll 1                // (unrolled, the 32 rows' LDS reads and FMA chains were scheduled together: hundreds of live registers, scratch)
    for (int i = 0; i < NF_ARS_H; ++i) {
        const float ai = a[i];
#pragma unroll
        for (int q = 0; q < PSP / 4; ++q) {
            const float4 w = *reinterpret_cast<const float4*>(wT + i * PSP + 4 * q);
            P[4 * q] = fmaf(ai, w.x, P[4 * q]);
            P[4 * q + 1] = fmaf(ai, w.y, P[4 * q + 1]);
            P[4 * q + 2] = fmaf(ai, w.z, P[4 * q + 2]);
            if (4 * q + 3 < PS) P[4 * q + 3] = fmaf(ai, w.w, P[4 * q + 3]);
        }
    }
}

// ---- forward / column inverse -----------------------------------------------------------------------------------------------------
// z and y may be the same tensor: an element is read before it is written, by the one thread that touches it
template <int K, bool INV>
__global__ void __launch_bounds__(NF_ARS_ROWS) k_ars_head(const float* __restrict__ a, const float* __restrict__ weight,
                                                          const float* __restrict__ bias, const float* __restrict__ mask, const float* z,
                                                          float* y, float* __restrict__ ld, float bound, int col, int64_t B, int D) {
    constexpr int PS = 3 * K - 1, PSP = PS + 1;
    __shared__ __attribute__((aligned(16))) float wT[NF_ARS_H * PSP];
    __shared__ float bt[PSP];
    __shared__ float at[NF_ARS_ROWS * NF_ARS_AS];
    const int d0 = INV ? col : 0, d1 = INV ? col + 1 : D;
    for (int64_t row0 = (int64_t)blockIdx.x * NF_ARS_ROWS; row0 < B; row0 += (int64_t)gridDim.x * NF_ARS_ROWS) {
        const int rows = (int)min((int64_t)NF_ARS_ROWS, B - row0);
        const int64_t b = row0 + threadIdx.x;
        const bool ok = threadIdx.x < rows;
        __syncthreads();                                   // (the previous tile's reads of the hidden tile)
        nf_ars_rows<false>(const_cast<float*>(a), at, row0, rows);
        __syncthreads();
        float acc = 0.f;
        for (int d = d0; d < d1; ++d) {
            __syncthreads();                               // (the previous feature's reads of wT / bt)
            nf_ars_stage<K>(weight, bias, mask, D, d, wT, bt);
            __syncthreads();
            if (ok) {
                const float v = z[b * D + d];
                float out = v;
                if (nf_rqs_inside(v, bound)) {
                    float P[PS];
                    nf_ars_params<K>(at + threadIdx.x * NF_ARS_AS, wT, bt, P);
                    out = nf_rqs_elem<K, INV>(P, 1, bound, v, acc);
                }
                y[b * D + d] = out;
            }
        }
        if (ok) ld[b] += acc;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
template <int K>
__global__ void __launch_bounds__(NF_ARS_ROWS) k_ars_head_bwd(const float* __restrict__ gy, const float* __restrict__ gld,
                                                              const float* __restrict__ a, const float* __restrict__ weight,
                                                              const float* __restrict__ bias, const float* __restrict__ mask,
                                                              const float* __restrict__ z, float* __restrict__ ga, float* __restrict__ gz,
                                                              float* __restrict__ gw_slabs, float* __restrict__ gb_slabs, float bound,
                                                              int64_t B, int D) {
    constexpr int PS = 3 * K - 1, PSP = PS + 1, NQ = PSP / 4;
    __shared__ __attribute__((aligned(16))) float wT[NF_ARS_H * PSP];
    __shared__ float bt[PSP];
    __shared__ float at[NF_ARS_ROWS * NF_ARS_AS];
    __shared__ float gat[NF_ARS_ROWS * NF_ARS_AS];
    // the parameter-gradient tile, row stride PSP (16-byte reads along p; column PS is padding, zero); after the product the same words
    // hold the four row groups' partial sums, [group][p][column]
    __shared__ __attribute__((aligned(16))) float gp[NF_ARS_ROWS * PSP];
    float* slab_w = gw_slabs + (int64_t)blockIdx.x * PS * D * NF_ARS_H;       // this workgroup's slabs
    float* slab_b = gb_slabs + (int64_t)blockIdx.x * PS * D;
    const int ci = threadIdx.x & (NF_ARS_H - 1), cg = threadIdx.x >> 5;      // the weight-gradient product: column and row group
    bool first = true;
    for (int64_t row0 = (int64_t)blockIdx.x * NF_ARS_ROWS; row0 < B; row0 += (int64_t)gridDim.x * NF_ARS_ROWS) {
        const int rows = (int)min((int64_t)NF_ARS_ROWS, B - row0);
        const int64_t b = row0 + threadIdx.x;
        const bool ok = threadIdx.x < rows;
        __syncthreads();                                   // (the previous tile's reads of the hidden tile and its store out of the g_a tile)
        nf_ars_rows<false>(const_cast<float*>(a), at, row0, rows);
        float* gar = gat + threadIdx.x * NF_ARS_AS;        // this thread's row of g_a: nobody else touches it before the store below
#pragma unroll 1
        for (int i = 0; i < NF_ARS_H; ++i) gar[i] = 0.f;
        const float gl = ok ? gld[b] : 0.f;
        for (int d = 0; d < D; ++d) {
            __syncthreads();                               // (the hidden tile is in place; the previous feature's reads of wT / bt / gp)
            nf_ars_stage<K>(weight, bias, mask, D, d, wT, bt);
            __syncthreads();
            if (ok) {
                const float x = z[b * D + d], g = gy[b * D + d];
                float4* grow = reinterpret_cast<float4*>(gp + threadIdx.x * PSP);
                if (nf_rqs_inside(x, bound)) {
                    float P[PS], G[PS];
                    nf_ars_params<K>(at + threadIdx.x * NF_ARS_AS, wT, bt, P);
                    gz[b * D + d] = nf_rqs_bwd_elem<K>(P, 1, G, 1, bound, x, g, gl);
#pragma unroll
                    for (int q = 0; q < NQ; ++q) grow[q] = make_float4(G[4 * q], G[4 * q + 1], G[4 * q + 2], 4 * q + 3 < PS ? G[4 * q + 3] : 0.f);
#pragma unroll 1
                    for (int i = 0; i < NF_ARS_H; ++i) {
                        float s = 0.f;
#pragma unroll
                        for (int q = 0; q < NQ; ++q) {
                            const float4 w = *reinterpret_cast<const float4*>(wT + i * PSP + 4 * q);
                            s = fmaf(G[4 * q], w.x, s);
                            s = fmaf(G[4 * q + 1], w.y, s);
                            s = fmaf(G[4 * q + 2], w.z, s);
                            if (4 * q + 3 < PS) s = fmaf(G[4 * q + 3], w.w, s);
                        }
                        gar[i] += s;
                    }
                } else {                                   // a linear tail: no parameter gradient, g_z = g_y
                    gz[b * D + d] = g;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) grow[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            __syncthreads();
            // g_weight[p D + d, i] += sum_r gP[r][p] a[r][i] over the tile's rows: row group cg takes the rows r = cg, cg + 4, ... in order
            // for every p of its column (one hidden value and NQ 16-byte reads per 4 NQ FMAs), the four groups meet in LDS in group order
            float acc[PSP];
#pragma unroll
            for (int p = 0; p < PSP; ++p) acc[p] = 0.f;
#pragma unroll 1
            for (int r = cg; r < rows; r += NF_ARS_ROWS / NF_ARS_H) {
                const float av = at[r * NF_ARS_AS + ci];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const float4 w = *reinterpret_cast<const float4*>(gp + r * PSP + 4 * q);
                    acc[4 * q] = fmaf(w.x, av, acc[4 * q]);
                    acc[4 * q + 1] = fmaf(w.y, av, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(w.z, av, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(w.w, av, acc[4 * q + 3]);
                }
            }
            float bs = 0.f;                                // g_bias[p D + d]: thread p adds its column of the tile in row order
            if (threadIdx.x < PS)
                for (int r = 0; r < rows; ++r) bs += gp[r * PSP + threadIdx.x];
            __syncthreads();                               // (every read of the gradient tile is done: its words take the partial sums)
#pragma unroll
            for (int p = 0; p < PSP; ++p) gp[(cg * PSP + p) * NF_ARS_H + ci] = acc[p];
            __syncthreads();
            // element o of the feature's (3K-1) x 32 block always belongs to thread o % NF_ARS_ROWS: its slab word has one writer.
            // The mask entry multiplies the sum (0: exactly 0)
            for (int o = threadIdx.x; o < PS * NF_ARS_H; o += NF_ARS_ROWS) {
                const int p = o >> 5, i = o & (NF_ARS_H - 1);
                constexpr int GS = PSP * NF_ARS_H;
                const float v = (((gp[o] + gp[GS + o]) + gp[2 * GS + o]) + gp[3 * GS + o]) * mask[d * NF_ARS_H + i];
                const int64_t w = (int64_t)(p * D + d) * NF_ARS_H + i;
                slab_w[w] = first ? v : slab_w[w] + v;
            }
            if (threadIdx.x < PS) {
                const int o = threadIdx.x * D + d;
                slab_b[o] = first ? bs : slab_b[o] + bs;
            }
        }
        __syncthreads();                                   // (every row of g_a is complete)
        nf_ars_rows<true>(ga, gat, row0, rows);
        first = false;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
extern "C" int nf_arspline_usable(int D, int K, int H) {
    return (D >= 1 && D <= 8 && (K == 4 || K == 8 || K == 16) && H == NF_ARS_H) ? 1 : 0;
}

extern "C" int nf_arspline_head_slabs(int64_t B) {
    if (B <= 0) return 0;
    const int64_t tiles = (B + NF_ARS_ROWS - 1) / NF_ARS_ROWS;
    return (int)(tiles < NF_ARS_MAX_SLABS ? tiles : NF_ARS_MAX_SLABS);
}

static inline int nf_ars_args(int K, float bound, int64_t B, int D, int H) {
    if (!nf_arspline_usable(D, K, H)) return NF_E_UNSUPPORTED;
    if (!(bound > 0.f) || B < 0 || B > 0x7fffffffLL) return NF_E_BADARG;
    return 0;
}

#define NF_ARS_DISPATCH(K, CALL) \
    do {                         \
        if (K == 4) { CALL(4); } \
        else if (K == 8) { CALL(8); } \
        else { CALL(16); }       \
    } while (0)

extern "C" int nf_arspline_head_fwd(const float* a, const float* weight, const float* bias, const float* mask, const float* z, float* y, float* ld,
                                    int K, float bound, int inverse, int col, int64_t B, int D, int H, nf_stream_t stream) {
    const int rc = nf_ars_args(K, bound, B, D, H);
    if (rc != 0) return rc;
    if (inverse ? (col < 0 || col >= D) : col != -1) return NF_E_BADARG;
    if (B == 0) return 0;
    if (a == nullptr || weight == nullptr || bias == nullptr || mask == nullptr || z == nullptr || y == nullptr || ld == nullptr) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(nf_grid_for(B, NF_ARS_ROWS));
#define CALL(KT)                                                                                                                          \
    if (inverse) hipLaunchKernelGGL((k_ars_head<KT, true>), grid, dim3(NF_ARS_ROWS), 0, st, a, weight, bias, mask, z, y, ld, bound, col, B, D); \
    else hipLaunchKernelGGL((k_ars_head<KT, false>), grid, dim3(NF_ARS_ROWS), 0, st, a, weight, bias, mask, z, y, ld, bound, col, B, D)
    NF_ARS_DISPATCH(K, CALL);
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_arspline_head_bwd(const float* g_y, const float* g_ld, const float* a, const float* weight, const float* bias, const float* mask,
                                    const float* z, float* g_a, float* g_z, float* g_w_slabs, float* g_b_slabs, int K, float bound, int64_t B,
                                    int D, int H, nf_stream_t stream) {
    const int rc = nf_ars_args(K, bound, B, D, H);
    if (rc != 0) return rc;
    if (B == 0) return 0;
    if (g_y == nullptr || g_ld == nullptr || a == nullptr || weight == nullptr || bias == nullptr || mask == nullptr || z == nullptr ||
        g_a == nullptr || g_z == nullptr || g_w_slabs == nullptr || g_b_slabs == nullptr)
        return NF_E_BADARG;
    const dim3 grid((unsigned)nf_arspline_head_slabs(B));                      // one slab per workgroup
#define CALL(KT)                                                                                                                      \
    hipLaunchKernelGGL(k_ars_head_bwd<KT>, grid, dim3(NF_ARS_ROWS), 0, (hipStream_t)stream, g_y, g_ld, a, weight, bias, mask, z, g_a, g_z, \
                       g_w_slabs, g_b_slabs, bound, B, D)
    NF_ARS_DISPATCH(K, CALL);
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}
