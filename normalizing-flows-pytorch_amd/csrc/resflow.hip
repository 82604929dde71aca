// Residual Flow, whole stack per launch: [ActNorm, InvertibleResLinear] x L on (B, D <= 4) data (flows/resflow.py:9-38, flows/iresblock.py,
// flows/spectral_norm.py, flows/modules.py:225-256).  Rows of a ResFlow never couple, except through (1) the ActNorm initialisation
// (stays on the per-layer path), (2) the batch-global exit of the fixed-point inverse (one workgroup: __syncthreads_or), (3) the parameter
// gradient sums (per-workgroup slabs folded in a fixed order) and (4) the reference's use of d_ld[0] for the whole batch (read once).
//   nf_resflow_spectral      power iteration + scaling of all 3 L matrices, one workgroup each; the stack's parameters land in ONE packed
//                            buffer (L, n_tot) that the other kernels stage from:  W1 | b1 | W2 | b2 | W3 | b3 | beta1 beta2 | log_scale | bias
//   nf_resflow_fwd           one row per thread, layer loop outside, the layer's weights re-staged in LDS; z and ld carried in registers
//   nf_resflow_bwd           lane = (sample slot, hidden unit) as k_resmlp_train_bwd; a wave owns its rows through all layers
//   nf_resflow_spectral_bwd  fold of the slabs + autograd of the spectral normalisation + every other parameter's total, added to the sinks
//   nf_resflow_inv           the whole inverse stack in one workgroup of 512 threads, rows in registers
//   nf_resflow_draws         the series lengths and the noise the kernels draw for given seed words
// No software grid barrier, no spin loop, no cooperative launch: every loop has a compile-time or argument bound.
#include "nf_common.h"
#include "nf_philox.h"
#include "nf_resmlp_core.h"

#define NF_RF_TAB 16            // pointers per layer: Wbar[3] u[3] v[3] b[3] beta[2] log_scale bias
#define NF_RF_GTAB 10           // gradient sinks per layer: gWbar[3] gb[3] gbeta[2] g_log_scale g_bias
#define NF_RF_BWD_MAX_GRID 64   // workgroups of nf_resflow_bwd: the slab is grid * L * n_tot floats (10 MB at L = 32)

struct NfRfOff { int W1, b1, W2, b2, W3, b3, be, ls, bi, tot; };
__host__ __device__ constexpr NfRfOff nf_rf_off(int D) {
    NfRfOff o{};
    o.W1 = 0;
    o.b1 = NF_RES_H * D;
    o.W2 = o.b1 + NF_RES_H;
    o.b2 = o.W2 + NF_RES_H * NF_RES_H;
    o.W3 = o.b2 + NF_RES_H;
    o.b3 = o.W3 + D * NF_RES_H;
    o.be = o.b3 + D;
    o.ls = o.be + 2;
    o.bi = o.ls + D;
    o.tot = o.bi + D;
    return o;
}
__device__ __forceinline__ NfResW nf_rf_weights(const float* P, const NfRfOff& o) {
    return NfResW{P + o.W1, P + o.b1, P + o.W2, P + o.b2, P + o.W3, P + o.b3, P + o.be, P + o.be + 1};
}

// ---- draws: Philox4x32-10 keyed by the seed words, counter = (row, layer, slot, sample, stream offset) --------------------------------------
struct NfRfKey { unsigned k0, k1, c3; };
__device__ __forceinline__ NfRfKey nf_rf_key(const int64_t* seed) {
    const uint64_t s = (uint64_t)seed[0], o = (uint64_t)seed[1];
    return NfRfKey{(unsigned)s, (unsigned)(s >> 32) ^ (unsigned)(o >> 32), (unsigned)o};
}
__device__ __forceinline__ unsigned nf_rf_c2(int layer, int slot, int s) { return ((unsigned)layer << 8) | ((unsigned)slot << 4) | (unsigned)s; }
// one length per (layer, slot, sample) for the whole batch (iresblock.py:66, :90: np.random.geometric once per call):
// n = n_exact + ceil(log(u) / log(1 - p)), a geometric(p) on {1, 2, ..}
__device__ __forceinline__ int nf_rf_length(const NfRfKey& k, int layer, int slot, int s, int n_exact, float p) {
    const NfPhilox r = nf_philox(0xFFFFFFFFu, 0xFFFFFFFFu, nf_rf_c2(layer, slot, s), k.c3, k.k0, k.k1);
    const float g = ceilf(logf(nf_u01(r.c[0])) / logf(1.f - p));
    const int n = n_exact + (int)fminf(fmaxf(g, 1.f), (float)NF_RES_MAXK);
    return n > NF_RES_MAXK ? NF_RES_MAXK : n;
}
template <int D>
__device__ __forceinline__ void nf_rf_noise(const NfRfKey& k, int layer, int slot, int s, int64_t row, float (&v)[D]) {
    const NfPhilox r = nf_philox((unsigned)row, (unsigned)((uint64_t)row >> 32), nf_rf_c2(layer, slot, s), k.c3, k.k0, k.k1);
    float n[4];
    nf_box_muller(r.c[0], r.c[1], n[0], n[1]);
    if (D > 2) nf_box_muller(r.c[2], r.c[3], n[2], n[3]);
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = n[d];
}
// the length of (layer, slot, sample): a fixed one (the `fixed` estimator), an explicit one, or a drawn one
__device__ __forceinline__ int nf_rf_n(const int* n_terms, const int64_t* seed, int fixed_n, int l, int layer0, int slot, int slots, int s, int S,
                                       int n_exact, float p) {
    int n;
    if (fixed_n > 0) n = fixed_n;
    else if (n_terms != nullptr) n = n_terms[(l * slots + (slots == 1 ? 0 : slot)) * S + s];
    else n = nf_rf_length(nf_rf_key(seed), layer0 + l, slot, s, n_exact, p);
    return n < 0 ? 0 : (n > NF_RES_MAXK ? NF_RES_MAXK : n);
}
// coefficients from (n_exact, p), k = 1, 2, .. in order (iresblock.py:59-81 value, :84-109 Neumann): pw = (1 - p)^max(0, k - n_exact - 1)
struct NfRfValueCoef {
    int n_exact; float q, pw;
    __device__ __forceinline__ float operator()(int k) {
        if (k - n_exact - 1 > 0) pw *= q;
        return ((k & 1) ? 1.f : -1.f) / ((float)k * pw);
    }
};
struct NfRfNeumannCoef {
    int n_exact; float q, pw;
    __device__ __forceinline__ float operator()(int k) {
        if (k - n_exact - 1 > 0) pw *= q;
        return ((k & 1) ? -1.f : 1.f) / pw;
    }
};

// log-det estimate of one row: mode 1 exact, mode 2 the mean of S series samples (slot 1 draws)
template <int D>
__device__ __forceinline__ float nf_rf_logdet(const float (&J)[D][D], int mode, const int* s_n, const float* noise, const int64_t* seed, int l,
                                              int layer0, int slots, int S, int n_exact, float p, int64_t b, int64_t B) {
    if (mode == 1) return logf(fabsf(nf_det_I_plus<D>(J)));
    float total = 0.f;
    for (int s = 0; s < S; ++s) {
        float vv[D];
        if (noise != nullptr) {
            const float* v = noise + ((((int64_t)l * slots + (slots - 1)) * B + b) * S + s) * D;
#pragma unroll
            for (int d = 0; d < D; ++d) vv[d] = v[d];
        } else {
            nf_rf_noise<D>(nf_rf_key(seed), layer0 + l, 1, s, b, vv);
        }
        nf_res_series_acc<D>(J, vv, s_n[s], NfRfValueCoef{n_exact, 1.f - p, 1.f}, total);
    }
    return total / (float)S;
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NF_BLOCK) k_resflow_spectral(const int64_t* __restrict__ tab, float* __restrict__ packed, int D, float coeff,
                                                               float eps) {
    __shared__ NfSnLds sl;
    const int m = blockIdx.x, l = blockIdx.y;
    const NfRfOff o = nf_rf_off(D);
    const int64_t* T = tab + (int64_t)l * NF_RF_TAB;
    float* P = packed + (int64_t)l * o.tot;
    const int H = m == 2 ? D : NF_RES_H, Wd = m == 0 ? D : NF_RES_H;
    const int off = m == 0 ? o.W1 : (m == 1 ? o.W2 : o.W3);
    nf_spectral_body((const float*)T[m], (float*)T[3 + m], (float*)T[6 + m], P + off, H, Wd, coeff, eps, sl);
    const float* bsrc = (const float*)T[9 + m];
    const int boff = m == 0 ? o.b1 : (m == 1 ? o.b2 : o.b3);
    if ((int)threadIdx.x < H) P[boff + threadIdx.x] = bsrc[threadIdx.x];
    if (m == 0 && threadIdx.x < 2) P[o.be + threadIdx.x] = ((const float*)T[12 + threadIdx.x])[0];
    if (m == 2 && (int)threadIdx.x < D) {
        P[o.ls + threadIdx.x] = ((const float*)T[14])[threadIdx.x];
        P[o.bi + threadIdx.x] = ((const float*)T[15])[threadIdx.x];
    }
}

// mode 0: z only.  1: + exact log-det.  2: + series estimator.  save (L, B, D): the block inputs (training), or NULL.
#define NF_RF_FWD_THREADS 64
template <int D>
__global__ void __launch_bounds__(NF_RF_FWD_THREADS) k_resflow_fwd(const float* __restrict__ packed, const float* __restrict__ x,
                                                                   float* __restrict__ y, float* __restrict__ ld, float* __restrict__ save,
                                                                   const int* __restrict__ n_terms, const float* __restrict__ noise,
                                                                   const int64_t* __restrict__ seed, int mode, int S, int n_exact, int fixed_n,
                                                                   float p, int L, int layer0, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ int s_n[NF_RES_MAXS];
    constexpr NfRfOff o = nf_rf_off(D);
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = b < B;
    float z[D], lv = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) z[d] = ok ? x[b * D + d] : 0.f;
    if (ok && mode != 0) lv = ld[b];
    for (int l = 0; l < L; ++l) {                                    // (runtime bound: never unrolled over layers)
        const float* P = packed + (int64_t)l * o.tot;
        __syncthreads();                                             // the previous layer's readers are done with sm / s_n
        if (mode == 2 && (int)threadIdx.x < S) s_n[threadIdx.x] = nf_rf_n(n_terms, seed, fixed_n, l, layer0, 1, 2, threadIdx.x, S, n_exact, p);
        nf_res_stage<D>(nf_rf_weights(P, o), sm);
        const float beta1 = P[o.be], beta2 = P[o.be + 1];
        float lsum = 0.f;                                            // ActNorm (modules.py:246-249), the arithmetic of k_chan_affine_fwd
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float ls = P[o.ls + d];
            z[d] = (z[d] - P[o.bi + d]) / expf(ls);
            lsum += ls;
        }
        lv += -lsum;
        if (save != nullptr && ok) {
#pragma unroll
            for (int d = 0; d < D; ++d) save[((int64_t)l * B + b) * D + d] = z[d];
        }
        float g[D], J[D][D];
        if (mode == 0) nf_res_eval<D, false>(sm, beta1, beta2, z, g, J);
        else nf_res_eval<D, true>(sm, beta1, beta2, z, g, J);
        if (mode != 0 && ok) lv += nf_rf_logdet<D>(J, mode, s_n, noise, seed, l, layer0, 2, S, n_exact, p, b, B);
#pragma unroll
        for (int d = 0; d < D; ++d) z[d] = z[d] + g[d];
    }
    if (ok) {
#pragma unroll
        for (int d = 0; d < D; ++d) y[b * D + d] = z[d];
        if (mode != 0) ld[b] = lv;
    }
}

// ---- backward: the stack in reverse, layer loop outside, the wave's own row pairs inside -----------------------------------------------------
template <int D>
__global__ void __launch_bounds__(NF_RT_THREADS) k_resflow_bwd(const float* __restrict__ packed, const float* __restrict__ save,
                                                               const float* g_y, const float* __restrict__ g_ld, float* d_z,
                                                               const int* __restrict__ n_terms, const float* __restrict__ noise,
                                                               const int64_t* __restrict__ seed, int S, float p, float* __restrict__ slab, int L,
                                                               int layer0, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr NfRfOff o = nf_rf_off(D);
    float* xb = sm + NF_RES_LDS(D) / sizeof(float);
    float* accum = xb + NF_RT_WAVES * 2 * NF_RES_BWD_PER(D);             // n_tot floats: this workgroup's totals of one layer
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, slot = lane >> 5, u = lane & 31;
    float* my = xb + (wid * 2 + slot) * NF_RES_BWD_PER(D);
    const float cs = g_ld[0];                                            // iresblock.py:166: the first row's for the whole batch
    const int64_t pairs = (B + 1) / 2;
    for (int l = L - 1; l >= 0; --l) {
        const float* P = packed + (int64_t)l * o.tot;
        __syncthreads();                                                 // sm and accum of the layer before are read out
        nf_res_stage<D>(nf_rf_weights(P, o), sm);
        const float beta1 = P[o.be], beta2 = P[o.be + 1];
        const int n1 = nf_rf_n(n_terms, seed, 0, l, layer0, 0, 2, 0, S, 1, p);
        const float* src = l == L - 1 ? g_y : d_z;
        float einv[D];
#pragma unroll
        for (int d = 0; d < D; ++d) einv[d] = expf(P[o.ls + d]);
        NfResAcc<D> acc;
        acc.zero();
        float a_ls = 0.f, a_bi = 0.f;                                    // lane u < D: sums of feature u
        for (int64_t pr = (int64_t)blockIdx.x * NF_RT_WAVES + wid; pr < pairs; pr += (int64_t)gridDim.x * NF_RT_WAVES) {
            const int64_t b = 2 * pr + slot;
            const bool ok = b < B;
            float xv[D], vv[D], dg[D], dx[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                xv[d] = ok ? save[((int64_t)l * B + b) * D + d] : 0.f;
                dg[d] = ok ? src[b * D + d] : 0.f;
                vv[d] = 0.f;
            }
            if (ok) {
                if (noise != nullptr) {
#pragma unroll
                    for (int d = 0; d < D; ++d) vv[d] = noise[((((int64_t)l * 2) * B + b) * S) * D + d];
                } else {
                    nf_rf_noise<D>(nf_rf_key(seed), layer0 + l, 0, 0, b, vv);
                }
            }
            nf_res_bwd_pair<D>(sm, my, beta1, beta2, cs, ok, u, xv, vv, dg, n1, NfRfNeumannCoef{1, 1.f - p, 1.f}, acc, dx);
            // residual connection, then the ActNorm in front of the block (the arithmetic of k_chan_affine_bwd)
            const float dl = ok ? g_ld[b] : 0.f;
            float yl = 0.f, dyl = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float dy = dg[d] + dx[d];
                if (u == d) { yl = xv[d]; dyl = dy; }
                if (ok && u == 0) d_z[b * D + d] = dy / einv[d];
            }
            if (ok && u < D) { a_ls += fmaf(dyl, yl, dl); a_bi += dyl; }
        }
        // totals of the workgroup in a fixed order: wave 0 stores, waves 1 .. 3 add in turn (no atomics: the same bits every run)
        for (int w = 0; w < NF_RT_WAVES; ++w) {
            if (wid == w) {
                const bool first = w == 0;
#define NF_PUT(idx, t) accum[idx] = first ? (t) : accum[idx] + (t)
#pragma unroll
                for (int i = 0; i < NF_RES_H; ++i) {
                    const float t = acc.W2[i] + __shfl_xor(acc.W2[i], 32, NF_WAVE);
                    if (slot == 0) NF_PUT(o.W2 + u * NF_RES_H + i, t);
                }
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const float t1 = acc.W1[d] + __shfl_xor(acc.W1[d], 32, NF_WAVE);
                    const float t3 = acc.W3[d] + __shfl_xor(acc.W3[d], 32, NF_WAVE);
                    if (slot == 0) { NF_PUT(o.W1 + u * D + d, t1); NF_PUT(o.W3 + d * NF_RES_H + u, t3); }
                }
                const float tb1 = acc.b1 + __shfl_xor(acc.b1, 32, NF_WAVE);
                const float tb2 = acc.b2 + __shfl_xor(acc.b2, 32, NF_WAVE);
                const float tb3 = acc.b3 + __shfl_xor(acc.b3, 32, NF_WAVE);
                const float tls = a_ls + __shfl_xor(a_ls, 32, NF_WAVE);
                const float tbi = a_bi + __shfl_xor(a_bi, 32, NF_WAVE);
                if (slot == 0) {
                    NF_PUT(o.b1 + u, tb1);
                    NF_PUT(o.b2 + u, tb2);
                    if (u < D) {
                        NF_PUT(o.b3 + u, tb3);
                        float ei = 1.f;
#pragma unroll
                        for (int d = 0; d < D; ++d)
                            if (u == d) ei = einv[d];
                        NF_PUT(o.ls + u, -tls);                          // g_log_scale = -sum g y - sum g_ld
                        NF_PUT(o.bi + u, -tbi / ei);                     // g_bias = -sum g / exp(log_scale)
                    }
                }
                float e1 = nf_half_allsum(acc.be1);
                float e2 = nf_half_allsum(acc.be2);
                e1 += __shfl_xor(e1, 32, NF_WAVE);
                e2 += __shfl_xor(e2, 32, NF_WAVE);
                if (lane == 0) { NF_PUT(o.be, e1); NF_PUT(o.be + 1, e2); }
#undef NF_PUT
            }
            __syncthreads();
        }
        float* dst = slab + ((int64_t)blockIdx.x * L + l) * o.tot;
        for (int i = threadIdx.x; i < o.tot; i += blockDim.x) dst[i] = accum[i];
    }
}

// fold of the slabs in workgroup order + the autograd of the spectral normalisation; every total is ADDED to its sink: gtab's pointer, or
// (gtab == NULL) its place in flat (L, n_tot), laid out as `packed`
__global__ void __launch_bounds__(NF_BLOCK) k_resflow_finish(const int64_t* __restrict__ tab, const int64_t* __restrict__ gtab,
                                                             float* __restrict__ flat, const float* __restrict__ slab, int G, int L, int D,
                                                             float coeff, float eps) {
    __shared__ float gl[NF_RES_H * NF_RES_H];
    __shared__ float scratch[NF_BLOCK / NF_WAVE];
    __shared__ float bc[2];
    const int m = blockIdx.x, l = blockIdx.y;
    const NfRfOff o = nf_rf_off(D);
    const int64_t* T = tab + (int64_t)l * NF_RF_TAB;
    auto sink = [&](int j, int off) { return gtab != nullptr ? (float*)gtab[(int64_t)l * NF_RF_GTAB + j] : flat + (int64_t)l * o.tot + off; };
    const float* S0 = slab + (int64_t)l * o.tot;
    const int64_t gs = (int64_t)L * o.tot;
    auto fold = [&](int idx) {
        float t = 0.f;
        for (int g = 0; g < G; ++g) t += S0[g * gs + idx];
        return t;
    };
    const int R = m == 2 ? D : NF_RES_H, C = m == 0 ? D : NF_RES_H;
    const int off = m == 0 ? o.W1 : (m == 1 ? o.W2 : o.W3);
    for (int e = threadIdx.x; e < R * C; e += blockDim.x) gl[e] = fold(off + e);
    __syncthreads();
    nf_spectral_bwd_body((const float*)T[m], (const float*)T[3 + m], (const float*)T[6 + m], gl, sink(m, off), R, C, coeff, eps, scratch, bc);
    const int boff = m == 0 ? o.b1 : (m == 1 ? o.b2 : o.b3);
    const int nb = m == 2 ? D : NF_RES_H;                                // b1, b2: 32 entries; b3: D
    if ((int)threadIdx.x < nb) sink(3 + m, boff)[threadIdx.x] += fold(boff + threadIdx.x);
    if (m == 0 && threadIdx.x < 2) sink(6 + threadIdx.x, o.be + threadIdx.x)[0] += fold(o.be + threadIdx.x);
    if (m == 2 && (int)threadIdx.x < D) {
        sink(8, o.ls)[threadIdx.x] += fold(o.ls + threadIdx.x);
        sink(9, o.bi)[threadIdx.x] += fold(o.bi + threadIdx.x);
    }
}

// ---- inverse: one workgroup, rows in registers ---------------------------------------------------------------------------------------------
#define NF_RF_INV_THREADS 512
#define NF_RF_INV_ROWS (NF_RESFLOW_INV_WG_MAX_ROWS / NF_RF_INV_THREADS)
#define NF_RF_INV_MAXIT 100     // iresblock.py:243
template <int D>
__global__ void __launch_bounds__(NF_RF_INV_THREADS) k_resflow_inv(const int64_t* __restrict__ tab, float* packed, const float* zin,
                                                                   float* xout, float* __restrict__ ld, int* __restrict__ iters,
                                                                   const int* __restrict__ n_terms, const float* __restrict__ noise,
                                                                   const int64_t* __restrict__ seed, int mode, int S, int n_exact, int fixed_n,
                                                                   float p, float coeff, float eps, float ftol, int L, int layer0, int B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ NfSnLds sl;
    __shared__ float s_u[3][64], s_v[3][64];
    __shared__ int s_n[NF_RES_MAXS];
    constexpr NfRfOff o = nf_rf_off(D);
    const int tid = threadIdx.x;
    float xr[NF_RF_INV_ROWS][D], lr[NF_RF_INV_ROWS];          // x and ld of the thread's rows; a block's z waits in xout (read once per iteration)
#pragma unroll
    for (int r = 0; r < NF_RF_INV_ROWS; ++r) {
        const int b = r * NF_RF_INV_THREADS + tid;
        lr[r] = b < B ? ld[b] : 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) xr[r][d] = b < B ? zin[(int64_t)b * D + d] : 0.f;
    }
    for (int l = L - 1; l >= 0; --l) {
        const int64_t* T = tab + (int64_t)l * NF_RF_TAB;
        float* P = packed + (int64_t)l * o.tot;
        __syncthreads();
        // the block's small parameters and power-iteration vectors
        if (tid < NF_RES_H) { P[o.b1 + tid] = ((const float*)T[9])[tid]; P[o.b2 + tid] = ((const float*)T[10])[tid]; }
        if (tid < D) { P[o.b3 + tid] = ((const float*)T[11])[tid]; P[o.ls + tid] = ((const float*)T[14])[tid]; P[o.bi + tid] = ((const float*)T[15])[tid]; }
        if (tid < 2) P[o.be + tid] = ((const float*)T[12 + tid])[0];
        if (tid < 3 * 64) {
            const int m = tid >> 6, i = tid & 63;
            const int H = m == 2 ? D : NF_RES_H, Wd = m == 0 ? D : NF_RES_H;
            if (i < H) s_u[m][i] = ((const float*)T[3 + m])[i];
            if (i < Wd) s_v[m][i] = ((const float*)T[6 + m])[i];
        }
        __syncthreads();
        const float beta1 = P[o.be], beta2 = P[o.be + 1];
        auto weights = [&]() {                   // one power iteration of the three matrices (spectral_norm.py:26-43 runs per g_fn call) + staging
            nf_spectral_body((const float*)T[0], s_u[0], s_v[0], P + o.W1, NF_RES_H, D, coeff, eps, sl);
            nf_spectral_body((const float*)T[1], s_u[1], s_v[1], P + o.W2, NF_RES_H, NF_RES_H, coeff, eps, sl);
            nf_spectral_body((const float*)T[2], s_u[2], s_v[2], P + o.W3, D, NF_RES_H, coeff, eps, sl);
            __syncthreads();                     // W_eff went through global memory: visible to the workgroup from here
            nf_res_stage<D>(nf_rf_weights(P, o), sm);
        };
#pragma unroll
        for (int r = 0; r < NF_RF_INV_ROWS; ++r) {                       // x starts at z (iresblock.py:240); only this thread reads it back
            const int b = r * NF_RF_INV_THREADS + tid;
#pragma unroll
            for (int d = 0; d < D; ++d)
                if (b < B) xout[(int64_t)b * D + d] = xr[r][d];
        }
        int done = 0;
        for (int it = 0; it < NF_RF_INV_MAXIT; ++it) {
            weights();
            int moving = 0;
#pragma unroll 1
            for (int r = 0; r < NF_RF_INV_ROWS; ++r) {                   // (not unrolled: one evaluation's registers at a time; the rows
                const int b = r * NF_RF_INV_THREADS + tid;               //  are picked by selects, so they stay in registers)
                if (b < B) {
                    float xc[D], zc[D], g[D], J[D][D];
#pragma unroll
                    for (int d = 0; d < D; ++d) zc[d] = xout[(int64_t)b * D + d];
#pragma unroll
                    for (int rr = 0; rr < NF_RF_INV_ROWS; ++rr)
#pragma unroll
                        for (int d = 0; d < D; ++d)
                            if (rr == r) xc[d] = xr[rr][d];
                    nf_res_eval<D, false, true>(sm, beta1, beta2, xc, g, J);
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const float nx = zc[d] - g[d];
                        moving |= !(fabsf(nx - xc[d]) < ftol);           // iresblock.py:248
#pragma unroll
                        for (int rr = 0; rr < NF_RF_INV_ROWS; ++rr)
                            if (rr == r) xr[rr][d] = nx;
                    }
                }
            }
            ++done;
            if (!__syncthreads_or(moving)) break;                        // batch-global exit: every row of the batch is in this workgroup
        }
        if (mode == 2 && tid < S) s_n[tid] = nf_rf_n(n_terms, seed, fixed_n, l, layer0, 1, 1, tid, S, n_exact, p);
        weights();                                                       // the reference's final g_fn(x) (iresblock.py:252)
        float lsum = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) lsum += P[o.ls + d];
#pragma unroll 1
        for (int r = 0; r < NF_RF_INV_ROWS; ++r) {
            const int b = r * NF_RF_INV_THREADS + tid;
            if (b < B) {
                float xc[D], lc = 0.f;
#pragma unroll
                for (int rr = 0; rr < NF_RF_INV_ROWS; ++rr) {
                    if (rr == r) lc = lr[rr];
#pragma unroll
                    for (int d = 0; d < D; ++d)
                        if (rr == r) xc[d] = xr[rr][d];
                }
                if (mode != 0) {
                    float J[D][D];
                    nf_res_jac_cols<D>(sm, beta1, beta2, xc, J);
                    lc += -1.f * nf_rf_logdet<D>(J, mode, s_n, noise, seed, l, layer0, 1, S, n_exact, p, b, B);
                }
                lc += lsum;
#pragma unroll
                for (int rr = 0; rr < NF_RF_INV_ROWS; ++rr) {
                    if (rr == r) lr[rr] = lc;
#pragma unroll
                    for (int d = 0; d < D; ++d)
                        if (rr == r) xr[rr][d] = fmaf(xc[d], expf(P[o.ls + d]), P[o.bi + d]);     // modules.py:253
                }
            }
        }
        __syncthreads();
        if (tid < 3 * 64) {                                              // u / v written back once per block
            const int m = tid >> 6, i = tid & 63;
            const int H = m == 2 ? D : NF_RES_H, Wd = m == 0 ? D : NF_RES_H;
            if (i < H) ((float*)T[3 + m])[i] = s_u[m][i];
            if (i < Wd) ((float*)T[6 + m])[i] = s_v[m][i];
        }
        if (tid == 0) iters[l] = done;
    }
#pragma unroll
    for (int r = 0; r < NF_RF_INV_ROWS; ++r) {
        const int b = r * NF_RF_INV_THREADS + tid;
        if (b < B) {
            ld[b] = lr[r];
#pragma unroll
            for (int d = 0; d < D; ++d) xout[(int64_t)b * D + d] = xr[r][d];
        }
    }
}

// slots = 2: n_terms (L, 2, S), noise (L, 2, B, S, D), slot 0 the Neumann surrogate's (n_exact 1, sample 0 only; the rest is zero), slot 1 the
// value estimator's.  slots = 1 (the inverse): the value estimator's draws alone.
__global__ void __launch_bounds__(NF_BLOCK) k_resflow_draws(int* __restrict__ n_terms, float* __restrict__ noise, const int64_t* __restrict__ seed,
                                                            int slots, int S, int n_exact, int fixed_n, float p, int L, int layer0, int64_t B,
                                                            int D) {
    const NfRfKey key = nf_rf_key(seed);
    const int64_t total = (int64_t)L * slots * B * S;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int s = (int)(t % S);
        const int64_t b = (t / S) % B;
        const int sl = (int)((t / S / B) % slots), l = (int)(t / S / B / slots);
        const int slot = slots == 1 ? 1 : sl;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const bool live = slot == 1 || s == 0;
        if (live) nf_rf_noise<4>(key, layer0 + l, slot, s, b, v);
        for (int d = 0; d < D; ++d) noise[t * D + d] = v[d];
        if (b == 0) {
            int n = 0;
            if (live) n = slot == 1 ? (fixed_n > 0 ? fixed_n : nf_rf_length(key, layer0 + l, 1, s, n_exact, p)) : nf_rf_length(key, layer0 + l, 0, 0, 1, p);
            n_terms[(l * slots + sl) * S + s] = n;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static bool rf_ok(int L, int64_t B, int D) { return L >= 1 && L <= NF_RESFLOW_MAX_LAYERS && D >= 1 && D <= NF_RES_MAXD && B >= 0 && B < ((int64_t)1 << 31); }
static bool rf_series_ok(int mode, int S, int n_exact, int fixed_n, float p, const int* n_terms, const float* noise, const int64_t* seed) {
    if (mode < 0 || mode > 2) return false;
    if (mode != 2) return true;
    if (S < 1 || S > NF_RES_MAXS || n_exact < 0 || n_exact > NF_RES_MAXK || fixed_n < 0 || fixed_n > NF_RES_MAXK || !(p > 0.f && p < 1.f)) return false;
    if (noise == nullptr) return seed != nullptr;                        // in-kernel draws
    return fixed_n > 0 || n_terms != nullptr;
}
static unsigned rf_bwd_grid(int64_t B) {
    const int64_t pairs = (B + 1) / 2;
    int64_t g = (pairs + NF_RT_WAVES - 1) / NF_RT_WAVES;
    if (g < 1) g = 1;
    return (unsigned)(g > NF_RF_BWD_MAX_GRID ? NF_RF_BWD_MAX_GRID : g);
}

extern "C" int nf_resflow_param_floats(int D, int* n_floats) {
    if (D < 1 || D > NF_RES_MAXD || n_floats == nullptr) return NF_E_BADARG;
    *n_floats = nf_rf_off(D).tot;
    return 0;
}

extern "C" int nf_resflow_spectral(const int64_t* table, float* packed, int L, int D, float coeff, float eps, nf_stream_t stream) {
    if (!rf_ok(L, 0, D) || table == nullptr || packed == nullptr) return NF_E_BADARG;
    hipLaunchKernelGGL(k_resflow_spectral, dim3(3, (unsigned)L), dim3(NF_BLOCK), 0, (hipStream_t)stream, table, packed, D, coeff, eps);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_resflow_fwd(const float* x, float* y, float* ld, float* save, const float* packed, const int* n_terms, const float* noise,
                              const int64_t* seed, int mode, int S, int n_exact, int fixed_n, float p, int L, int layer0, int64_t B, int D,
                              nf_stream_t stream) {
    if (!rf_ok(L, B, D) || layer0 < 0 || !rf_series_ok(mode, S, n_exact, fixed_n, p, n_terms, noise, seed)) return NF_E_BADARG;
    if (x == nullptr || y == nullptr || packed == nullptr || (mode != 0 && ld == nullptr)) return NF_E_BADARG;
    if (B == 0) return 0;
    const unsigned g = (unsigned)((B + NF_RF_FWD_THREADS - 1) / NF_RF_FWD_THREADS);
#define CALL(DT) hipLaunchKernelGGL(k_resflow_fwd<DT>, dim3(g), dim3(NF_RF_FWD_THREADS), NF_RES_LDS(DT), (hipStream_t)stream, packed, x, y, ld, save, \
                                    n_terms, noise, seed, mode, S, n_exact, fixed_n, p, L, layer0, B)
    NF_RES_DISPATCH(D, CALL)
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_resflow_bwd_slab_floats(int L, int64_t B, int D, int64_t* n_floats) {
    if (!rf_ok(L, B, D) || n_floats == nullptr) return NF_E_BADARG;
    *n_floats = (int64_t)rf_bwd_grid(B) * L * nf_rf_off(D).tot;
    return 0;
}

extern "C" int nf_resflow_bwd(const float* g_y, const float* g_ld, float* d_z, const float* save, const float* packed, const int* n_terms,
                              const float* noise, const int64_t* seed, int S, float p, float* slab, int L, int layer0, int64_t B, int D,
                              nf_stream_t stream) {
    if (!rf_ok(L, B, D) || layer0 < 0 || B < 1 || S < 1 || S > NF_RES_MAXS || !(p > 0.f && p < 1.f)) return NF_E_BADARG;
    if (g_y == nullptr || g_ld == nullptr || d_z == nullptr || save == nullptr || packed == nullptr || slab == nullptr) return NF_E_BADARG;
    if (noise == nullptr ? seed == nullptr : n_terms == nullptr) return NF_E_BADARG;
    const unsigned g = rf_bwd_grid(B);
#define CALL(DT) hipLaunchKernelGGL(k_resflow_bwd<DT>, dim3(g), dim3(NF_RT_THREADS),                                                              \
                                    NF_RES_LDS(DT) + (NF_RT_WAVES * 2 * NF_RES_BWD_PER(DT) + nf_rf_off(DT).tot) * sizeof(float), (hipStream_t)stream, \
                                    packed, save, g_y, g_ld, d_z, n_terms, noise, seed, S, p, slab, L, layer0, B)
    NF_RES_DISPATCH(D, CALL)
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_resflow_spectral_bwd(const int64_t* table, const int64_t* grads, float* flat, const float* slab, int L, int64_t B, int D,
                                       float coeff, float eps, nf_stream_t stream) {
    if (!rf_ok(L, B, D) || B < 1 || table == nullptr || (grads == nullptr) == (flat == nullptr) || slab == nullptr) return NF_E_BADARG;
    hipLaunchKernelGGL(k_resflow_finish, dim3(3, (unsigned)L), dim3(NF_BLOCK), 0, (hipStream_t)stream, table, grads, flat, slab, (int)rf_bwd_grid(B),
                       L, D, coeff, eps);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_resflow_inv(const float* z, float* x, float* ld, int* iters, const int64_t* table, float* packed, const int* n_terms,
                              const float* noise, const int64_t* seed, int mode, int S, int n_exact, int fixed_n, float p, float coeff, float eps,
                              float ftol, int L, int layer0, int64_t B, int D, nf_stream_t stream) {
    if (!rf_ok(L, B, D) || layer0 < 0 || B > NF_RESFLOW_INV_WG_MAX_ROWS || !rf_series_ok(mode, S, n_exact, fixed_n, p, n_terms, noise, seed))
        return NF_E_BADARG;
    if (z == nullptr || x == nullptr || ld == nullptr || iters == nullptr || table == nullptr || packed == nullptr) return NF_E_BADARG;
    if (B == 0) return 0;
#define CALL(DT) hipLaunchKernelGGL(k_resflow_inv<DT>, dim3(1), dim3(NF_RF_INV_THREADS), NF_RES_LDS(DT), (hipStream_t)stream, table, packed, z, x, ld, \
                                    iters, n_terms, noise, seed, mode, S, n_exact, fixed_n, p, coeff, eps, ftol, L, layer0, (int)B)
    NF_RES_DISPATCH(D, CALL)
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_resflow_draws(int* n_terms, float* noise, const int64_t* seed, int slots, int S, int n_exact, int fixed_n, float p, int L,
                                int layer0, int64_t B, int D, nf_stream_t stream) {
    if (L < 1 || layer0 < 0 || D < 1 || D > NF_RES_MAXD || B < 1 || slots < 1 || slots > 2 || S < 1 || S > NF_RES_MAXS || !(p > 0.f && p < 1.f))
        return NF_E_BADARG;
    if (n_terms == nullptr || noise == nullptr || seed == nullptr || n_exact < 0 || fixed_n < 0) return NF_E_BADARG;
    hipLaunchKernelGGL(k_resflow_draws, dim3(nf_grid_for((int64_t)L * slots * B * S)), dim3(NF_BLOCK), 0, (hipStream_t)stream, n_terms, noise, seed,
                       slots, S, n_exact, fixed_n, p, L, layer0, B, D);
    NF_CHECK_LAUNCH();
    return 0;
}
