// Invertible residual block (Residual Flow) forward / inverse + log-det on the GPU for D <= 4 features:
//   g(x) = W3 lipswish(W2 lipswish(W1 x + b1) + b2) + b3      (flows/iresblock.py:258-278, flows/modules.py:215-222)
// One thread per sample, the three (spectrally normalised) weight matrices broadcast from LDS.  The per-sample Jacobian
// J = W3 D2 W2 D1 W1 (D x D) is formed in forward mode, so every log-det estimator of the reference reduces to a few
// D x D operations per sample instead of nested autograd VJP sweeps:
//   exact  : log |det(I + J)|                                                    (iresblock.py:17-32)
//   series : mean_s sum_k coef[s][k] * v_s^T (J^T)^k v_s   with host-drawn noise v and Russian-roulette lengths
//            (fixed: coef = (-1)^(k+1)/k, iresblock.py:35-56; unbias: / P(N >= k), iresblock.py:59-81)
// Spectral normalisation (flows/spectral_norm.py:26-43) is a separate one-block-per-matrix launch, and the fixed-point
// inverse (iresblock.py:236-255) is a chain of single-iteration launches gated by a device flag that reproduces the
// reference's batch-global exit without a host round trip.
#include "nf_common.h"
#include "nf_det.h"
#include "nf_resmlp_core.h"

NF_DET_STATE(nf_rsm)
NF_DET_HOST_API(nf_rsm)


// mode 0: y = x + g only.  mode 1: + exact log-det.  mode 2: + series estimator with noise v (B, S, D)
template <int D>
__global__ void __launch_bounds__(NF_BLOCK) k_resmlp_fwd(NfResW w, const float* __restrict__ x, float* __restrict__ y,
                                                         float* __restrict__ ld, float ld_sign, int mode,
                                                         const float* __restrict__ v, const float* __restrict__ coef,
                                                         const int* __restrict__ n_terms, int S, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    nf_res_stage<D>(w, sm);
    const float beta1 = w.beta1[0], beta2 = w.beta2[0];
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
        float xv[D], g[D], J[D][D];
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d] = x[b * D + d];
        if (mode == 0) nf_res_eval<D, false>(sm, beta1, beta2, xv, g, J);
        else nf_res_eval<D, true>(sm, beta1, beta2, xv, g, J);
        if (y != nullptr) {
#pragma unroll
            for (int d = 0; d < D; ++d) y[b * D + d] = xv[d] + g[d];
        }
        if (mode == 1) {
            ld[b] += ld_sign * logf(fabsf(nf_det_I_plus<D>(J)));
        } else if (mode == 2) {
            float total = 0.f;
            for (int s = 0; s < S; ++s) {
                float vv[D];
#pragma unroll
                for (int d = 0; d < D; ++d) vv[d] = v[(b * S + s) * D + d];
                const float* cf = coef + s * NF_RES_MAXK;
                nf_res_series_acc<D>(J, vv, n_terms[s], [&](int k) { return cf[k - 1]; }, total);
            }
            ld[b] += ld_sign * total / (float)S;
        }
    }
}

// one fixed-point iteration x <- z - g(x); runs only while the previous iteration left some |dx| >= ftol
template <int D>
__global__ void __launch_bounds__(NF_BLOCK) k_resmlp_fixed_point(NfResW w, const float* __restrict__ z, float* __restrict__ x,
                                                                 int* __restrict__ flags, int it, float ftol, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    if (it > 0 && flags[it - 1] == 0) return;                // converged (or skipped) before: the reference left its loop
    nf_res_stage<D>(w, sm);
    const float beta1 = w.beta1[0], beta2 = w.beta2[0];
    bool moving = false;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
        float xv[D], g[D], J[D][D];
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d] = x[b * D + d];
        nf_res_eval<D, false>(sm, beta1, beta2, xv, g, J);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float nx = z[b * D + d] - g[d];
            moving |= !(fabsf(nx - xv[d]) < ftol);             // iresblock.py:248
            x[b * D + d] = nx;
        }
    }
    if (__any(moving) && (threadIdx.x & (NF_WAVE - 1)) == 0) atomicOr(flags + it, 1);
}

// spectral normalisation of up to 3 matrices (one block each): one power iteration, u / v updated in place,
// W_eff = W_bar * min(coeff / (sigma + eps), 1).  Skipped like the fixed-point step when `flags` says "converged".
struct NfSnArgs {
    const float* Wbar[3];
    float* u[3];
    float* v[3];
    float* Weff[3];
    int h[3];
    int w[3];
};
__global__ void __launch_bounds__(NF_BLOCK) k_spectral_weights(NfSnArgs a, float coeff, float eps, const int* __restrict__ flags,
                                                               int it) {
    __shared__ NfSnLds sl;
    if (flags != nullptr && it > 0 && flags[it - 1] == 0) return;
    const int m = blockIdx.x;
    nf_spectral_body(a.Wbar[m], a.u[m], a.v[m], a.Weff[m], a.h[m], a.w[m], coeff, eps, sl);
}

// ---------------------------------------------------------------------------------------------------------------

extern "C" int nf_resmlp_fwd(const float* x, const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* W3, const float* b3, const float* beta1, const float* beta2, float* y, float* ld,
                             float ld_sign, int mode, const float* noise, const float* coef, const int* n_terms, int S,
                             int64_t B, int D, nf_stream_t stream) {
    if (D < 1 || mode < 0 || mode > 2 || (mode > 0 && ld == nullptr)) return NF_E_BADARG;
    if (mode == 2 && (S < 1 || S > NF_RES_MAXS || noise == nullptr || coef == nullptr || n_terms == nullptr)) return NF_E_BADARG;
    if (B == 0) return 0;
    NfResW w{W1, b1, W2, b2, W3, b3, beta1, beta2};
    unsigned g = nf_grid_for(B, 64);
    if (g > 2048) g = 2048;
#define CALL(DT) hipLaunchKernelGGL(k_resmlp_fwd<DT>, dim3(g), dim3(64), NF_RES_LDS(DT), (hipStream_t)stream, w, x, y, ld, ld_sign, mode, noise, coef, n_terms, S, B)
    NF_RES_DISPATCH(D, CALL)
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_resmlp_fixed_point_step(const float* z, float* x, const float* W1, const float* b1, const float* W2,
                                          const float* b2, const float* W3, const float* b3, const float* beta1,
                                          const float* beta2, int* flags, int iteration, float ftol, int64_t B, int D,
                                          nf_stream_t stream) {
    if (D < 1 || iteration < 0 || flags == nullptr) return NF_E_BADARG;
    if (B == 0) return 0;
    NfResW w{W1, b1, W2, b2, W3, b3, beta1, beta2};
    unsigned g = nf_grid_for(B, 64);
    if (g > 2048) g = 2048;
#define CALL(DT) hipLaunchKernelGGL(k_resmlp_fixed_point<DT>, dim3(g), dim3(64), NF_RES_LDS(DT), (hipStream_t)stream, w, z, x, flags, iteration, ftol, B)
    NF_RES_DISPATCH(D, CALL)
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_spectral_weights(const float* const* W_bar, float* const* u, float* const* v, float* const* W_eff,
                                   const int* rows, const int* cols, int n_mats, float coeff, float eps, const int* flags,
                                   int iteration, nf_stream_t stream) {
    if (n_mats < 1 || n_mats > 3) return NF_E_BADARG;
    NfSnArgs a;
    for (int i = 0; i < n_mats; ++i) {
        if (rows[i] < 1 || cols[i] < 1 || rows[i] > 64 || cols[i] > 64) return NF_E_BADARG;
        a.Wbar[i] = W_bar[i]; a.u[i] = u[i]; a.v[i] = v[i]; a.Weff[i] = W_eff[i]; a.h[i] = rows[i]; a.w[i] = cols[i];
    }
    hipLaunchKernelGGL(k_spectral_weights, dim3((unsigned)n_mats), dim3(NF_BLOCK), 0, (hipStream_t)stream, a, coeff, eps, flags,
                       iteration);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// TRAINING backward of the block (iresblock.py:84-109 Neumann gradient estimator, :112-185 memory-saving autograd Function).
// The reference differentiates, per block and step,
//     L  =  < dL/dg , g(x) >  +  c * S(x, theta),      S = s^T J(x, theta) v,   s = v + sum_k coef_k (J^T)^k v  (held constant),
// where c is the upstream gradient of the log-det taken from the FIRST sample (iresblock.py:166) and v the Hutchinson noise:
// S needs second derivatives of g, which nested autograd sweeps provide there.  For the 2 -> 32 -> 32 -> 2 LipSwish network they
// are closed form.  With h1 = W1 x + b1, a1 = phi(h1), h2 = W2 a1 + b2, a = W1 v, p1 = phi'(h1) a, q = W2 p1, p2 = phi'(h2) q:
//     S = (W3^T s) . p2,   and with r3 = W3^T s, g3 = W3^T dL/dg the combined signals are
//     GQ  = c r3 phi'(h2)                                  (gradient of q)
//     GH2 = g3 phi'(h2) + c r3 phi''(h2) q                 (gradient of h2)
//     GP1 = W2^T GQ,  GA1 = W2^T GH2,  GH1 = GA1 phi'(h1) + GP1 phi''(h1) a   (gradient of h1)
//     dW3 = dL/dg a2^T + c s p2^T,  dW2 = GQ p1^T + GH2 a1^T,  db2 = GH2,  dW1 = GH1 x^T + (GP1 phi'(h1)) v^T,  db1 = GH1,  db3 = dL/dg,
//     dx = W1^T GH1  (the residual connection's identity term is added by the caller), and the two LipSwish slopes beta get
//     dbeta2 = sum g3 dphi/dbeta(h2) + c r3 q dphi'/dbeta(h2),   dbeta1 = sum GA1 dphi/dbeta(h1) + GP1 a dphi'/dbeta(h1).
// Work decomposition: lane = (sample slot, hidden unit): a wave works on TWO samples at a time, every per-unit quantity is one
// register, matrix-vector products read the other units' values as LDS broadcasts; a lane accumulates ITS row of dW2 (32
// registers) and its entries of the other gradients over all the samples of its wave, and the block adds its totals to the
// (zeroed) output with one atomic per entry.

// g_out layout: W1 (32 x D) | b1 (32) | W2 (32 x 32) | b2 (32) | W3 (D x 32) | b3 (D) | beta1 | beta2
template <int D>
__global__ void __launch_bounds__(NF_RT_THREADS) k_resmlp_train_bwd(NfResW w, const float* __restrict__ x, const float* __restrict__ vn,
                                                                    const float* __restrict__ coef, int n_terms,
                                                                    const float* __restrict__ d_g, const float* __restrict__ d_ld,
                                                                    float* __restrict__ d_x, float* __restrict__ g_out, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    nf_res_stage<D>(w, sm);
    float* xb = sm + NF_RES_LDS(D) / sizeof(float);          // per (wave, slot): a1[32] | p1[32] | t1[D][32] | GQ[32] | GH2[32]
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, slot = lane >> 5, u = lane & 31;
    float* my = xb + (wid * 2 + slot) * NF_RES_BWD_PER(D);
    const float beta1 = w.beta1[0], beta2 = w.beta2[0], cs = d_ld[0];
    NfResAcc<D> acc;
    acc.zero();
    const int64_t pairs = (B + 1) / 2;
    for (int64_t pr = (int64_t)blockIdx.x * NF_RT_WAVES + wid; pr < pairs; pr += (int64_t)gridDim.x * NF_RT_WAVES) {
        const int64_t b = 2 * pr + slot;
        const bool ok = b < B;
        float xv[D], vv[D], dg[D], dx[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            xv[d] = ok ? x[b * D + d] : 0.f;
            vv[d] = ok ? vn[b * D + d] : 0.f;
            dg[d] = ok ? d_g[b * D + d] : 0.f;
        }
        nf_res_bwd_pair<D>(sm, my, beta1, beta2, cs, ok, u, xv, vv, dg, n_terms, [&](int k) { return coef[k - 1]; }, acc, dx);
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (ok && u == 0) d_x[b * D + d] = dx[d];
    }
    float (&accW2)[NF_RES_H] = acc.W2;
    float (&accW1)[D] = acc.W1;
    float (&accW3)[D] = acc.W3;
    float &acc_b1 = acc.b1, &acc_b2 = acc.b2, &acc_b3 = acc.b3, &acc_be1 = acc.be1, &acc_be2 = acc.be2;
    // ---- totals: the two slots of a wave, then one atomic per entry and wave ------------------------------------------------------------
    float* gW1 = g_out;
    float* gb1 = gW1 + NF_RES_H * D;
    float* gW2 = gb1 + NF_RES_H;
    float* gb2 = gW2 + NF_RES_H * NF_RES_H;
    float* gW3 = gb2 + NF_RES_H;
    float* gb3 = gW3 + D * NF_RES_H;
    float* gbe = gb3 + D;
    // every wave of every workgroup adds to the same entries: deterministic mode takes the workgroups in block order and, inside one,
    // the waves in wave order (within a wave no two lanes share an address)
    NF_DET_ENTER_ALL(nf_rsm);
    nf_det_waves(nf_det_, NF_RT_WAVES, wid, [&] {
#pragma unroll
        for (int i = 0; i < NF_RES_H; ++i) {
            const float t = accW2[i] + __shfl_xor(accW2[i], 32, NF_WAVE);
            if (slot == 0) atomicAdd(gW2 + u * NF_RES_H + i, t);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float t1 = accW1[d] + __shfl_xor(accW1[d], 32, NF_WAVE);
            const float t3 = accW3[d] + __shfl_xor(accW3[d], 32, NF_WAVE);
            if (slot == 0) { atomicAdd(gW1 + u * D + d, t1); atomicAdd(gW3 + d * NF_RES_H + u, t3); }
        }
        {
            const float tb1 = acc_b1 + __shfl_xor(acc_b1, 32, NF_WAVE);
            const float tb2 = acc_b2 + __shfl_xor(acc_b2, 32, NF_WAVE);
            const float tb3 = acc_b3 + __shfl_xor(acc_b3, 32, NF_WAVE);
            if (slot == 0) { atomicAdd(gb1 + u, tb1); atomicAdd(gb2 + u, tb2); if (u < D) atomicAdd(gb3 + u, tb3); }
            float e1 = nf_half_allsum(acc_be1);
            float e2 = nf_half_allsum(acc_be2);
            e1 += __shfl_xor(e1, 32, NF_WAVE);
            e2 += __shfl_xor(e2, 32, NF_WAVE);
            if (lane == 0) { atomicAdd(gbe, e1); atomicAdd(gbe + 1, e2); }
        }
    });
    NF_DET_LEAVE_ALL(nf_rsm);
}

extern "C" int nf_resmlp_train_bwd(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                                   const float* b3, const float* beta1, const float* beta2, const float* noise, const float* coef,
                                   int n_terms, const float* d_g, const float* d_ld, float* d_x, float* g_params, int64_t B, int D,
                                   nf_stream_t stream) {
    if (D < 1 || D > NF_RES_MAXD || n_terms < 0 || n_terms > NF_RES_MAXK || B < 0) return NF_E_BADARG;
    if (B == 0) return 0;
    NfResW w = {W1, b1, W2, b2, W3, b3, beta1, beta2};
    int64_t pairs = (B + 1) / 2;
    unsigned grid = (unsigned)((pairs + NF_RT_WAVES - 1) / NF_RT_WAVES);
    if (grid > 256) grid = 256;
    hipStream_t st = (hipStream_t)stream;
#define NF_L(D_)                                                                                                              \
    hipLaunchKernelGGL(k_resmlp_train_bwd<D_>, dim3(grid), dim3(NF_RT_THREADS),                                               \
                       NF_RES_LDS(D_) + NF_RT_WAVES * 2 * (4 + D_) * NF_RES_H * sizeof(float), st, w, x, noise, coef, n_terms, d_g, \
                       d_ld, d_x, g_params, B)
    switch (D) {
        case 1: NF_L(1); break;
        case 2: NF_L(2); break;
        case 3: NF_L(3); break;
        default: NF_L(4); break;
    }
#undef NF_L
    NF_CHECK_LAUNCH();
    return 0;
}

// autograd of nf_spectral_weights (spectral_norm.py:36-43): W_eff = W_bar * min(coeff / (sigma + eps), 1), sigma = u^T W_bar v with the
// power-iteration vectors held constant.  g_W_bar += g_W_eff * scale  -  [scale < 1] <g_W_eff, W_bar> coeff / (sigma + eps)^2 * u v^T
struct NfSnBwdArgs {
    const float* Wbar[3];
    const float* u[3];
    const float* v[3];
    const float* gWeff[3];
    float* gWbar[3];
    int h[3];
    int w[3];
};
__global__ void __launch_bounds__(NF_BLOCK) k_spectral_bwd(NfSnBwdArgs a, float coeff, float eps) {
    __shared__ float scratch[NF_BLOCK / NF_WAVE];
    __shared__ float bc[2];
    const int m = blockIdx.x;
    nf_spectral_bwd_body(a.Wbar[m], a.u[m], a.v[m], a.gWeff[m], a.gWbar[m], a.h[m], a.w[m], coeff, eps, scratch, bc);
}
extern "C" int nf_spectral_weights_bwd(const float* const* W_bar, const float* const* u, const float* const* v,
                                       const float* const* g_W_eff, float* const* g_W_bar, const int* rows, const int* cols, int n_mats,
                                       float coeff, float eps, nf_stream_t stream) {
    if (n_mats < 1 || n_mats > 3) return NF_E_BADARG;
    NfSnBwdArgs a;
    for (int i = 0; i < n_mats; ++i) {
        if (rows[i] < 1 || cols[i] < 1 || rows[i] > 64 || cols[i] > 64) return NF_E_BADARG;
        a.Wbar[i] = W_bar[i]; a.u[i] = u[i]; a.v[i] = v[i]; a.gWeff[i] = g_W_eff[i]; a.gWbar[i] = g_W_bar[i]; a.h[i] = rows[i]; a.w[i] = cols[i];
    }
    hipLaunchKernelGGL(k_spectral_bwd, dim3((unsigned)n_mats), dim3(NF_BLOCK), 0, (hipStream_t)stream, a, coeff, eps);
    NF_CHECK_LAUNCH();
    return 0;
}
