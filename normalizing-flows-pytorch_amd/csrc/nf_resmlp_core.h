// Device functions of the invertible residual block shared by its per-block kernels (resmlp.hip) and the whole-stack kernels
// (resflow.hip): weight staging, g(x) with its Jacobian, the log-det estimators, the closed-form training backward of one sample
// pair, and the spectral normalisation of one matrix with its autograd.
#pragma once
#include "nf_common.h"

#define NF_RES_H 32
#define NF_RES_MAXD 4
#define NF_RES_MAXS 4
#define NF_RES_MAXK 64

__device__ __forceinline__ float nf_lipswish(float x, float beta, float& dx) {
    const float s = 1.f / (1.f + expf(-beta * x));
    dx = (s + beta * x * s * (1.f - s)) * (1.f / 1.1f);     // d/dx [ x sigmoid(beta x) / 1.1 ]
    return x * s * (1.f / 1.1f);
}

struct NfResW {
    const float *W1, *b1, *W2, *b2, *W3, *b3, *beta1, *beta2;
};

// weights -> LDS: W1 (H x D), W2 (H x H, row stride H+1), W3 (D x H), biases, betas
template <int D>
__device__ __forceinline__ void nf_res_stage(const NfResW& w, float* sm) {
    float* W1 = sm;
    float* b1 = W1 + NF_RES_H * D;
    float* W2 = b1 + NF_RES_H;
    float* b2 = W2 + NF_RES_H * (NF_RES_H + 1);
    float* W3 = b2 + NF_RES_H;
    float* b3 = W3 + D * NF_RES_H;
    for (int i = threadIdx.x; i < NF_RES_H * D; i += blockDim.x) W1[i] = w.W1[i];
    for (int i = threadIdx.x; i < NF_RES_H * NF_RES_H; i += blockDim.x) W2[(i / NF_RES_H) * (NF_RES_H + 1) + (i % NF_RES_H)] = w.W2[i];
    for (int i = threadIdx.x; i < D * NF_RES_H; i += blockDim.x) W3[i] = w.W3[i];
    for (int i = threadIdx.x; i < NF_RES_H; i += blockDim.x) { b1[i] = w.b1[i]; b2[i] = w.b2[i]; }
    for (int i = threadIdx.x; i < D; i += blockDim.x) b3[i] = w.b3[i];
    __syncthreads();
}
#define NF_RES_LDS(D) ((NF_RES_H * (D) + NF_RES_H + NF_RES_H * (NF_RES_H + 1) + NF_RES_H + (D) * NF_RES_H + (D)) * sizeof(float))

// g(x) and, if JAC, the Jacobian columns J[:, d] = W3 (D2 (W2 (D1 W1[:, d])))
// LEAN: the loop over the second layer's units is not unrolled (for kernels that run under a 128-register budget; same arithmetic)
template <int D, bool JAC, bool LEAN = false>
__device__ __forceinline__ void nf_res_eval(const float* sm, float beta1, float beta2, const float (&x)[D], float (&g)[D],
                                            float (&J)[D][D]) {
    const float* W1 = sm;
    const float* b1 = W1 + NF_RES_H * D;
    const float* W2 = b1 + NF_RES_H;
    const float* b2 = W2 + NF_RES_H * (NF_RES_H + 1);
    const float* W3 = b2 + NF_RES_H;
    const float* b3 = W3 + D * NF_RES_H;
    float a1[NF_RES_H], t1[JAC ? D : 1][NF_RES_H];
#pragma unroll
    for (int o = 0; o < NF_RES_H; ++o) {
        float h = b1[o];
#pragma unroll
        for (int d = 0; d < D; ++d) h = fmaf(W1[o * D + d], x[d], h);
        float dh;
        a1[o] = nf_lipswish(h, beta1, dh);
        if (JAC) {
#pragma unroll
            for (int d = 0; d < D; ++d) t1[d][o] = dh * W1[o * D + d];
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        g[d] = b3[d];
        if (JAC) {
#pragma unroll
            for (int e = 0; e < D; ++e) J[d][e] = 0.f;
        }
    }
    auto unit = [&](int o) {
        float h = b2[o];
        float jt[JAC ? D : 1];
        if (JAC) {
#pragma unroll
            for (int d = 0; d < D; ++d) jt[d] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < NF_RES_H; ++i) {
            const float w = W2[o * (NF_RES_H + 1) + i];
            h = fmaf(w, a1[i], h);
            if (JAC) {
#pragma unroll
                for (int d = 0; d < D; ++d) jt[d] = fmaf(w, t1[d][i], jt[d]);
            }
        }
        float dh;
        const float a2 = nf_lipswish(h, beta2, dh);
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const float w3 = W3[r * NF_RES_H + o];
            g[r] = fmaf(w3, a2, g[r]);
            if (JAC) {
#pragma unroll
                for (int d = 0; d < D; ++d) J[r][d] = fmaf(w3, dh * jt[d], J[r][d]);
            }
        }
    };
    if (LEAN) {
#pragma unroll 1
        for (int o = 0; o < NF_RES_H; ++o) unit(o);             // one output unit at a time: ~100 registers
    } else {
        for (int o = 0; o < NF_RES_H; ++o) unit(o);
    }
}

// the Jacobian alone, one COLUMN per pass over the network (64 live registers instead of 32 (D + 1); the entries are the bits nf_res_eval gives)
template <int D>
__device__ __forceinline__ void nf_res_jac_cols(const float* sm, float beta1, float beta2, const float (&x)[D], float (&J)[D][D]) {
    const float* W1 = sm;
    const float* b1 = W1 + NF_RES_H * D;
    const float* W2 = b1 + NF_RES_H;
    const float* b2 = W2 + NF_RES_H * (NF_RES_H + 1);
    const float* W3 = b2 + NF_RES_H;
#pragma unroll 1
    for (int c = 0; c < D; ++c) {
        float a1[NF_RES_H], t[NF_RES_H], col[D];
#pragma unroll
        for (int o = 0; o < NF_RES_H; ++o) {
            float h = b1[o];
#pragma unroll
            for (int d = 0; d < D; ++d) h = fmaf(W1[o * D + d], x[d], h);
            float dh;
            a1[o] = nf_lipswish(h, beta1, dh);
            t[o] = dh * W1[o * D + c];
        }
#pragma unroll
        for (int r = 0; r < D; ++r) col[r] = 0.f;
#pragma unroll 1
        for (int o = 0; o < NF_RES_H; ++o) {
            float h = b2[o], jt = 0.f;
#pragma unroll
            for (int i = 0; i < NF_RES_H; ++i) {
                const float w = W2[o * (NF_RES_H + 1) + i];
                h = fmaf(w, a1[i], h);
                jt = fmaf(w, t[i], jt);
            }
            float dh;
            nf_lipswish(h, beta2, dh);
#pragma unroll
            for (int r = 0; r < D; ++r) col[r] = fmaf(W3[r * NF_RES_H + o], dh * jt, col[r]);
        }
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int d = 0; d < D; ++d)
                if (d == c) J[r][d] = col[r];
    }
}

template <int D>
__device__ __forceinline__ float nf_det_I_plus(const float (&J)[D][D]) {
    float A[D][D];
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int c = 0; c < D; ++c) A[r][c] = J[r][c] + (r == c ? 1.f : 0.f);
    float det = 1.f;                          // Gaussian elimination without pivoting: I + J is near identity (Lip(g) < 1)
#pragma unroll
    for (int k = 0; k < D; ++k) {
        det *= A[k][k];
#pragma unroll
        for (int r = k + 1; r < D; ++r) {
            const float f = A[r][k] / A[k][k];
#pragma unroll
            for (int c = k + 1; c < D; ++c) A[r][c] -= f * A[k][c];
        }
    }
    return det;
}

struct NfLipD { float f, d1, d2, db, d1b; };              // phi, phi', phi'', dphi/dbeta, dphi'/dbeta
__device__ __forceinline__ NfLipD nf_lipswish_all(float h, float beta) {
    const float u = beta * h;
    const float s = 1.f / (1.f + expf(-u));
    const float sp = s * (1.f - s), spp = sp * (1.f - 2.f * s);
    const float k = 1.f / 1.1f;
    NfLipD r;
    r.f = h * s * k;
    r.d1 = (s + u * sp) * k;
    r.d2 = (2.f * beta * sp + beta * u * spp) * k;
    r.db = h * h * sp * k;
    r.d1b = h * (2.f * sp + u * spp) * k;
    return r;
}
__device__ __forceinline__ float nf_half_allsum(float v) {     // sum over the 32 lanes of a wave half, result in every lane
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, NF_WAVE);
    return v;
}
#define NF_RT_WAVES 4
#define NF_RT_THREADS (NF_RT_WAVES * NF_WAVE)

#define NF_RES_DISPATCH(D, CALL) \
    switch (D) { case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; default: return NF_E_UNSUPPORTED; }

// ---- series estimator: total += sum_{k=1..n} coef(k) * v^T (J^T)^k v  (one Hutchinson sample; coef(k) is called with k = 1, 2, .. n in order) ----
template <int D, class Coef>
__device__ __forceinline__ void nf_res_series_acc(const float (&J)[D][D], const float (&vv)[D], int n, Coef coef, float& total) {
    float wv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) wv[d] = vv[d];
    for (int k = 1; k <= n; ++k) {           // w <- J^T w  (one vector-Jacobian product), tr = w . v
        float nw[D];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            float a = 0.f;
#pragma unroll
            for (int r = 0; r < D; ++r) a = fmaf(J[r][c], wv[r], a);
            nw[c] = a;
        }
        float tr = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) { wv[d] = nw[d]; tr = fmaf(nw[d], vv[d], tr); }
        total = fmaf(coef(k), tr, total);
    }
}

// ---- training backward of ONE sample per wave half (lane = (slot, hidden unit u)); the derivation is at k_resmlp_train_bwd ----------------
template <int D>
struct NfResAcc {
    float W2[NF_RES_H], W1[D], W3[D], b1, b2, b3, be1, be2;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < NF_RES_H; ++i) W2[i] = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) { W1[d] = 0.f; W3[d] = 0.f; }
        b1 = b2 = b3 = be1 = be2 = 0.f;
    }
};
#define NF_RES_BWD_PER(D) ((4 + (D)) * NF_RES_H)          // floats of one (wave, slot) exchange buffer: a1 | p1 | t1[D] | GQ | GH2

// sm: the staged weights; my: this (wave, slot)'s exchange buffer; coef(k), k = 1 .. n_terms in order: the Neumann coefficients.
// dx[d] = (W1^T GH1)[d] in every lane of the half; the accumulators take this sample's contribution when `ok`.
template <int D, class Coef>
__device__ __forceinline__ void nf_res_bwd_pair(const float* sm, float* my, float beta1, float beta2, float cs, bool ok, int u,
                                                const float (&xv)[D], const float (&vv)[D], const float (&dg)[D], int n_terms, Coef coef,
                                                NfResAcc<D>& acc, float (&dx)[D]) {
    const float* W1 = sm;
    const float* b1 = W1 + NF_RES_H * D;
    const float* W2 = b1 + NF_RES_H;
    const float* b2 = W2 + NF_RES_H * (NF_RES_H + 1);
    const float* W3 = b2 + NF_RES_H;
    float* A1 = my;
    float* P1 = my + NF_RES_H;
    float* T1 = my + 2 * NF_RES_H;
    float* GQl = my + (2 + D) * NF_RES_H;
    float* GHl = my + (3 + D) * NF_RES_H;
    // ---- layer 1 (lane = unit u) --------------------------------------------------------------------------------------
    float h1 = b1[u], aV = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) { h1 = fmaf(W1[u * D + d], xv[d], h1); aV = fmaf(W1[u * D + d], vv[d], aV); }
    const NfLipD l1 = nf_lipswish_all(h1, beta1);
    const float p1 = l1.d1 * aV;
    A1[u] = l1.f;
    P1[u] = p1;
#pragma unroll
    for (int d = 0; d < D; ++d) T1[d * NF_RES_H + u] = l1.d1 * W1[u * D + d];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- layer 2 (lane = unit u): h2, q, Jacobian row pieces -----------------------------------------------------------------
    float h2 = b2[u], q = 0.f, jt[D];
#pragma unroll
    for (int d = 0; d < D; ++d) jt[d] = 0.f;
#pragma unroll 8
    for (int i = 0; i < NF_RES_H; ++i) {
        const float wv = W2[u * (NF_RES_H + 1) + i];
        h2 = fmaf(wv, A1[i], h2);
        q = fmaf(wv, P1[i], q);
#pragma unroll
        for (int d = 0; d < D; ++d) jt[d] = fmaf(wv, T1[d * NF_RES_H + i], jt[d]);
    }
    const NfLipD l2 = nf_lipswish_all(h2, beta2);
    float J[D][D];
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int d = 0; d < D; ++d) J[r][d] = nf_half_allsum(W3[r * NF_RES_H + u] * l2.d1 * jt[d]);
    // ---- s = v + sum_k coef_k (J^T)^k v  (every lane, D x D) ----------------------------------------------------------------------
    float sv[D], wv2[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { sv[d] = vv[d]; wv2[d] = vv[d]; }
    for (int k = 1; k <= n_terms; ++k) {
        float nw[D];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            float a = 0.f;
#pragma unroll
            for (int r = 0; r < D; ++r) a = fmaf(J[r][c], wv2[r], a);
            nw[c] = a;
        }
        const float ck = coef(k);
#pragma unroll
        for (int d = 0; d < D; ++d) { wv2[d] = nw[d]; sv[d] = fmaf(ck, nw[d], sv[d]); }
    }
    // ---- signals of layer 2 ------------------------------------------------------------------------------------------------------
    float r3 = 0.f, g3 = 0.f;
#pragma unroll
    for (int r = 0; r < D; ++r) { r3 = fmaf(W3[r * NF_RES_H + u], sv[r], r3); g3 = fmaf(W3[r * NF_RES_H + u], dg[r], g3); }
    const float p2 = l2.d1 * q;
    const float GQ = ok ? cs * r3 * l2.d1 : 0.f;
    const float GH2 = ok ? fmaf(cs * r3 * l2.d2, q, g3 * l2.d1) : 0.f;
    if (ok) {
#pragma unroll
        for (int r = 0; r < D; ++r) acc.W3[r] += fmaf(cs * sv[r], p2, dg[r] * l2.f);
        acc.b2 += GH2;
        acc.be2 += fmaf(cs * r3 * q, l2.d1b, g3 * l2.db);
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (u == d) acc.b3 += dg[d];
    }
#pragma unroll
    for (int i = 0; i < NF_RES_H; ++i) acc.W2[i] += fmaf(GQ, P1[i], GH2 * A1[i]);      // (full unroll: the accumulators stay registers)
    GQl[u] = GQ;
    GHl[u] = GH2;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- back to layer 1 (lane = unit u): W2^T products walk a COLUMN of W2 (row stride 33: conflict-free) --------------------------
    float gp1 = 0.f, ga1 = 0.f;
#pragma unroll 8
    for (int o = 0; o < NF_RES_H; ++o) {
        const float wv = W2[o * (NF_RES_H + 1) + u];
        gp1 = fmaf(wv, GQl[o], gp1);
        ga1 = fmaf(wv, GHl[o], ga1);
    }
    const float GH1 = fmaf(gp1 * l1.d2, aV, ga1 * l1.d1);
    if (ok) {
        acc.b1 += GH1;
        acc.be1 += fmaf(gp1 * aV, l1.d1b, ga1 * l1.db);
#pragma unroll
        for (int d = 0; d < D; ++d) acc.W1[d] += fmaf(gp1 * l1.d1, vv[d], GH1 * xv[d]);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) dx[d] = nf_half_allsum(W1[u * D + d] * GH1);
    __builtin_amdgcn_wave_barrier();                  // the slot buffers are rewritten by the next pair
}

// ---- spectral normalisation of ONE matrix by a workgroup of NF_BLOCK threads (spectral_norm.py:26-43): one power iteration, u / v updated
// in place, W_eff = W_bar * min(coeff / (sigma + eps), 1) ------------------------------------------------------------------------------------
struct NfSnLds {
    float su[64], sv[64], scratch[1024 / NF_WAVE];            // (workgroups of up to 1 024 threads)
    float s_scale;
};
__device__ __forceinline__ void nf_spectral_body(const float* __restrict__ W, float* __restrict__ ug, float* __restrict__ vg,
                                                 float* __restrict__ Weff, int H, int Wd, float coeff, float eps, NfSnLds& s) {
    if ((int)threadIdx.x < H) s.su[threadIdx.x] = ug[threadIdx.x];
    __syncthreads();
    float t = 0.f;                                            // v = l2normalize(W^T u)
    if ((int)threadIdx.x < Wd)
        for (int r = 0; r < H; ++r) t = fmaf(W[r * Wd + threadIdx.x], s.su[r], t);
    float n2 = nf_block_sum((int)threadIdx.x < Wd ? t * t : 0.f, s.scratch);
    if (threadIdx.x == 0) s.s_scale = sqrtf(n2) + 1e-12f;
    __syncthreads();
    if ((int)threadIdx.x < Wd) { s.sv[threadIdx.x] = t / s.s_scale; vg[threadIdx.x] = s.sv[threadIdx.x]; }
    __syncthreads();
    float q = 0.f;                                            // u = l2normalize(W v)
    if ((int)threadIdx.x < H)
        for (int c = 0; c < Wd; ++c) q = fmaf(W[threadIdx.x * Wd + c], s.sv[c], q);
    n2 = nf_block_sum((int)threadIdx.x < H ? q * q : 0.f, s.scratch);
    if (threadIdx.x == 0) s.s_scale = sqrtf(n2) + 1e-12f;
    __syncthreads();
    const float un = (int)threadIdx.x < H ? q / s.s_scale : 0.f;
    if ((int)threadIdx.x < H) ug[threadIdx.x] = un;
    const float sigma = nf_block_sum(un * q, s.scratch);      // u . (W v)
    if (threadIdx.x == 0) s.s_scale = fminf(coeff / (sigma + eps), 1.f);
    __syncthreads();
    for (int i = threadIdx.x; i < H * Wd; i += blockDim.x) Weff[i] = W[i] * s.s_scale;
}

// autograd of it with the power-iteration vectors held constant (spectral_norm.py:36-43):
// g_W_bar += g_W_eff * scale  -  [scale < 1] <g_W_eff, W_bar> coeff / (sigma + eps)^2 * u v^T.   g may live in LDS.
__device__ __forceinline__ void nf_spectral_bwd_body(const float* __restrict__ W, const float* __restrict__ u, const float* __restrict__ v,
                                                     const float* g, float* __restrict__ out, int R, int C, float coeff, float eps,
                                                     float* scratch, float* bc) {
    const int n = R * C;
    float ps = 0.f, pd = 0.f;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int r = e / C, c = e - r * C;
        ps = fmaf(u[r] * v[c], W[e], ps);
        pd = fmaf(g[e], W[e], pd);
    }
    const float sigma = nf_block_sum(ps, scratch);
    const float dot = nf_block_sum(pd, scratch);
    if (threadIdx.x == 0) { bc[0] = sigma; bc[1] = dot; }
    __syncthreads();
    const float sg = bc[0], scale = coeff / (sg + eps);
    const bool active = scale < 1.f;
    const float k2 = active ? -bc[1] * coeff / ((sg + eps) * (sg + eps)) : 0.f;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int r = e / C, c = e - r * C;
        out[e] += (active ? g[e] * scale : g[e]) + k2 * u[r] * v[c];
    }
}
