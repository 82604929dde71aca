// Planar flow (flows/planar.py): the whole K-layer stack per direction, without a host round trip.
//
//   projection  nf_planar_project   every layer's u projected in place where w.u < -1 (planar.py:23-33), a launch of its own so that no
//                                   workgroup of the forward reads a u another one writes
//   forward     nf_planar_fwd       all K layers in one launch, one row per thread; training saves the per-layer inputs z_k (B x K x D)
//   backward    nf_planar_bwd       the layers in reverse per row from the saved z_k: g_z and the per-row u / w / b terms, summed over the
//                                   batch per wave by a fixed shuffle tree into a slab, then a fixed-order fold launch adds the slab into the
//                                   gradient buffers: no float atomics, bit-reproducible whatever the scheduling
//   inverse     nf_planar_inv       the bisection (planar.py:47-68) with the reference's batch-global exit rule: one workgroup of 1024
//                                   threads for B <= NF_PLANAR_INV_WG_MAX_ROWS (the "all closed?" test is a __syncthreads_or per iteration),
//                                   else three launches per layer (28 iterations + open flag, the first all-closed iteration, the finish)
//
// Full-precision tanhf / logf / log1pf / expf throughout: the inverse's bracket is 1e-5 wide.
#include <cstdlib>

#include "nf_common.h"

#define PL_WG 1024                     // threads of the one-workgroup inverse
#define PL_RPT (NF_PLANAR_INV_WG_MAX_ROWS / PL_WG)
#define PL_P1_ITERS 28                 // no bracket closes before iteration 28 unless it collapses: 2000 * 2^-28 < 1e-5 <= 2000 * 2^-27
#define PL_MAX_ITERS 100               // planar.py:57
#define PL_OPEN (PL_MAX_ITERS + 1)

struct NfPlanarPtrs {
    float* p[3 * NF_PLANAR_MAX_LAYERS];   // u_0 .. u_{K-1}, w_0 .. w_{K-1}, b_0 .. b_{K-1}
};

static int nf_pl_mode = 0;             // 0: automatic form selection, 1: grid forms at every B (nf_planar_config)

extern "C" int nf_planar_config(int mode) {
    if (mode >= 0) nf_pl_mode = mode & 1;
    return 0;
}

static bool pl_table(NfPlanarPtrs& t, const int64_t* host, int K, bool need_all) {
    if (host == nullptr) return false;
    for (int i = 0; i < 3 * NF_PLANAR_MAX_LAYERS; ++i) t.p[i] = nullptr;
    for (int i = 0; i < 3 * K; ++i) {
        t.p[i] = (float*)(intptr_t)host[i];
        if (need_all && t.p[i] == nullptr) return false;
    }
    return true;
}

// w.u of layer k as torch.mm(u, w.t()) computes it: one fixed-order dot product (the same in every launch of this file)
__device__ __forceinline__ float pl_dot(const float* __restrict__ a, const float* __restrict__ b, int D) {
    float s = 0.0f;
    for (int d = 0; d < D; ++d) s = fmaf(a[d], b[d], s);
    return s;
}

__device__ __forceinline__ float pl_logdet(float wu, float t) {
    const float det = 1.0f + wu * (1.0f - t * t);                    // deriv_tanh, modules.py:40-43
    return logf(fabsf(det) + 1.0e-5f);
}

__device__ __forceinline__ float pl_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, NF_WAVE);
    return v;
}

__device__ __forceinline__ int pl_wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, NF_WAVE));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// projection (planar.py:23-33): one wave per layer.  u <- u + (-1 + softplus(w.u) - w.u) * w / |w|^2 where w.u < -1.
// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NF_BLOCK) k_planar_project(NfPlanarPtrs t, int K, int D) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int k = wid; k < K; k += NF_BLOCK / NF_WAVE) {
        float* u = t.p[k];
        const float* w = t.p[K + k];
        float su = 0.0f, sw = 0.0f;
        for (int d = lane; d < D; d += NF_WAVE) {
            su = fmaf(u[d], w[d], su);
            sw = fmaf(w[d], w[d], sw);
        }
        const float wu = pl_wave_sum(su), ww = pl_wave_sum(sw);
        if (wu >= -1.0f) continue;                                       // planar.py:27
        const float nrm = sqrtf(ww), nw = nrm * nrm;                     // torch.norm(w, p=2, dim=1) ** 2
        const float sp = wu > 20.0f ? wu : log1pf(expf(wu));             // F.softplus (beta 1, threshold 20)
        const float c = (-1.0f + sp) - wu;
        for (int d = lane; d < D; d += NF_WAVE) u[d] = u[d] + c * (w[d] / nw);
    }
}

// parameters of all layers in LDS: u [K][D], w [K][D], b [K], w.u [K]
template <int DT>
__device__ __forceinline__ void pl_stage(const NfPlanarPtrs& t, int K, float* su, float* sw, float* sb, float* swu) {
    constexpr int DS = DT > 0 ? DT : 1;
    for (int e = threadIdx.x; e < K * DS; e += blockDim.x) {
        const int k = e / DS, d = e - k * DS;
        su[e] = t.p[k][d];
        sw[e] = t.p[K + k][d];
    }
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        sb[k] = t.p[2 * K + k][0];
        swu[k] = pl_dot(t.p[k], t.p[K + k], DS);
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// forward (planar.py:35-45), one row per thread.  DT > 0: the row in registers, parameters in LDS; DT == 0: any D, row in `out`.
// ---------------------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(NF_BLOCK) k_planar_fwd(const float* __restrict__ z, float* __restrict__ out, float* __restrict__ ld,
                                                         float* __restrict__ save, NfPlanarPtrs t, int K, int64_t B, int D) {
    __shared__ float su[NF_PLANAR_MAX_LAYERS * (DT > 0 ? DT : 1)], sw[NF_PLANAR_MAX_LAYERS * (DT > 0 ? DT : 1)];
    __shared__ float sb[NF_PLANAR_MAX_LAYERS], swu[NF_PLANAR_MAX_LAYERS];
    if (DT > 0) {
        pl_stage<DT>(t, K, su, sw, sb, swu);
    } else {
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            sb[k] = t.p[2 * K + k][0];
            swu[k] = pl_dot(t.p[k], t.p[K + k], D);
        }
        __syncthreads();
    }
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float l = ld[b];
    if (DT > 0) {
        float x[DT > 0 ? DT : 1];
#pragma unroll
        for (int d = 0; d < DT; ++d) x[d] = z[b * DT + d];
        for (int k = 0; k < K; ++k) {
            if (save != nullptr) {
#pragma unroll
                for (int d = 0; d < DT; ++d) save[((int64_t)k * B + b) * DT + d] = x[d];
            }
            float a = 0.0f;
#pragma unroll
            for (int d = 0; d < DT; ++d) a = fmaf(x[d], sw[k * DT + d], a);
            const float th = tanhf(a + sb[k]);
#pragma unroll
            for (int d = 0; d < DT; ++d) x[d] = fmaf(su[k * DT + d], th, x[d]);
            l += pl_logdet(swu[k], th);
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) out[b * DT + d] = x[d];
    } else {
        float* x = out + b * D;
        for (int d = 0; d < D; ++d) x[d] = z[b * D + d];
        for (int k = 0; k < K; ++k) {
            if (save != nullptr)
                for (int d = 0; d < D; ++d) save[((int64_t)k * B + b) * D + d] = x[d];
            const float th = tanhf(pl_dot(x, t.p[K + k], D) + sb[k]);
            const float* u = t.p[k];
            for (int d = 0; d < D; ++d) x[d] = fmaf(u[d], th, x[d]);
            l += pl_logdet(swu[k], th);
        }
    }
    ld[b] = l;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// backward: per row, layer k in reverse, with g = dL/dz_{k+1} and c = g_ld * sign(det) / (|det| + 1e-5) (abs: gradient 0 at 0):
//   g_t = g.u - 2 c wu t,  g_a = g_t (1 - t^2);   dL/du_k += g t + c psi w,  dL/dw_k += g_a z_k + c psi u,  dL/db_k += g_a;
//   g <- g + g_a w.    The per-row terms are summed per wave (fixed xor tree) into slab[wave][k][2D + 1].
// ---------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pl_dlogdet(float gl, float det) {
    const float sg = det > 0.0f ? 1.0f : (det < 0.0f ? -1.0f : 0.0f);
    return gl * sg / (fabsf(det) + 1.0e-5f);
}

template <int DT>
__global__ void __launch_bounds__(NF_BLOCK) k_planar_bwd(const float* __restrict__ g_out, const float* __restrict__ g_ld,
                                                         const float* __restrict__ save, float* __restrict__ g_z, float* __restrict__ slab,
                                                         NfPlanarPtrs t, int K, int64_t B, int D) {
    __shared__ float su[NF_PLANAR_MAX_LAYERS * (DT > 0 ? DT : 1)], sw[NF_PLANAR_MAX_LAYERS * (DT > 0 ? DT : 1)];
    __shared__ float sb[NF_PLANAR_MAX_LAYERS], swu[NF_PLANAR_MAX_LAYERS];
    if (DT > 0) {
        pl_stage<DT>(t, K, su, sw, sb, swu);
    } else {
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            sb[k] = t.p[2 * K + k][0];
            swu[k] = pl_dot(t.p[k], t.p[K + k], D);
        }
        __syncthreads();
    }
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = b < B;                       // (dead lanes take part in the wave sums with zeros)
    const int lane = threadIdx.x & 63;
    const int stride = 2 * D + 1;
    float* const my_slab = slab + ((int64_t)blockIdx.x * (NF_BLOCK / NF_WAVE) + (threadIdx.x >> 6)) * K * stride;
    const float gl = live ? g_ld[b] : 0.0f;
    if (DT > 0) {
        float g[DT > 0 ? DT : 1];
#pragma unroll
        for (int d = 0; d < DT; ++d) g[d] = live ? g_out[b * DT + d] : 0.0f;
        for (int k = K - 1; k >= 0; --k) {
            float x[DT > 0 ? DT : 1];
#pragma unroll
            for (int d = 0; d < DT; ++d) x[d] = live ? save[((int64_t)k * B + b) * DT + d] : 0.0f;
            float a = 0.0f, gu = 0.0f;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                a = fmaf(x[d], sw[k * DT + d], a);
                gu = fmaf(g[d], su[k * DT + d], gu);
            }
            const float th = tanhf(a + sb[k]), psi = 1.0f - th * th, wu = swu[k];
            const float c = pl_dlogdet(gl, 1.0f + wu * psi);
            const float ga = live ? (gu - 2.0f * c * wu * th) * psi : 0.0f;
            const float cp = live ? c * psi : 0.0f;
            const float tl = live ? th : 0.0f;
            float* const dst = my_slab + k * stride;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const float vu = pl_wave_sum(g[d] * tl + cp * sw[k * DT + d]);
                const float vw = pl_wave_sum(ga * x[d] + cp * su[k * DT + d]);
                if (lane == 0) {
                    dst[d] = vu;
                    dst[DT + d] = vw;
                }
            }
            const float vb = pl_wave_sum(ga);
            if (lane == 0) dst[2 * DT] = vb;
#pragma unroll
            for (int d = 0; d < DT; ++d) g[d] = fmaf(ga, sw[k * DT + d], g[d]);
        }
        if (live && g_z != nullptr) {
#pragma unroll
            for (int d = 0; d < DT; ++d) g_z[b * DT + d] = g[d];
        }
    } else {
        // g_z is the row's working copy of the gradient (required for the generic form)
        float* const g = g_z + (live ? b : 0) * D;
        if (live)
            for (int d = 0; d < D; ++d) g[d] = g_out[b * D + d];
        for (int k = K - 1; k >= 0; --k) {
            const float* x = save + ((int64_t)k * B + (live ? b : 0)) * D;
            const float* u = t.p[k];
            const float* w = t.p[K + k];
            float a = 0.0f, gu = 0.0f;
            if (live) {
                a = pl_dot(x, w, D);
                gu = pl_dot(g, u, D);
            }
            const float th = tanhf(a + sb[k]), psi = 1.0f - th * th, wu = swu[k];
            const float c = pl_dlogdet(gl, 1.0f + wu * psi);
            const float ga = live ? (gu - 2.0f * c * wu * th) * psi : 0.0f;
            const float cp = live ? c * psi : 0.0f;
            const float tl = live ? th : 0.0f;
            float* const dst = my_slab + k * stride;
            for (int d = 0; d < D; ++d) {
                const float gd = live ? g[d] : 0.0f, xd = live ? x[d] : 0.0f;
                const float vu = pl_wave_sum(gd * tl + cp * w[d]);
                const float vw = pl_wave_sum(ga * xd + cp * u[d]);
                if (lane == 0) {
                    dst[d] = vu;
                    dst[D + d] = vw;
                }
                if (live) g[d] = fmaf(ga, w[d], gd);
            }
            const float vb = pl_wave_sum(ga);
            if (lane == 0) dst[2 * D] = vb;
        }
    }
}

// fold: one wave per gradient element; lane l sums waves l, l + 64, ... in order, then a fixed xor tree; += into the gradient buffer
__global__ void __launch_bounds__(NF_BLOCK) k_planar_fold(const float* __restrict__ slab, int64_t n_waves, NfPlanarPtrs g, int K, int D) {
    const int lane = threadIdx.x & 63;
    const int stride = 2 * D + 1;
    const int64_t n_el = (int64_t)K * stride;
    const int64_t e = (int64_t)blockIdx.x * (NF_BLOCK / NF_WAVE) + (threadIdx.x >> 6);
    if (e >= n_el) return;
    float s = 0.0f;
    for (int64_t w = lane; w < n_waves; w += NF_WAVE) s += slab[w * n_el + e];
    s = pl_wave_sum(s);
    if (lane == 0) {
        const int k = (int)(e / stride), j = (int)(e - (int64_t)k * stride);
        float* dst = j < D ? g.p[k] + j : (j < 2 * D ? g.p[K + k] + (j - D) : g.p[2 * K + k]);
        *dst = *dst + s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// inverse (planar.py:47-68).  One bisection iteration of a row; returns whether the bracket is closed afterwards.
// ---------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pl_bisect(float& lo, float& hi, float wz, float wu, float bb) {
    const float mid = (lo + hi) * 0.5f;
    const float val = mid + wu * tanhf(mid + bb);
    lo = val < wz ? mid : lo;
    hi = val > wz ? mid : hi;
    return fabsf(hi - lo) < 1.0e-5f;
}

__device__ __forceinline__ float pl_row_wz(const float* __restrict__ x, const float* __restrict__ w, int D) { return pl_dot(x, w, D); }

// the finish of a row: a = mid + b, z <- z - u tanh(a), ld -= log|det|
__device__ __forceinline__ void pl_finish(float* __restrict__ x, const float* __restrict__ u, int D, float mid, float bb, float wu,
                                          float& l) {
    const float th = tanhf(mid + bb);
    for (int d = 0; d < D; ++d) x[d] = x[d] - u[d] * th;
    l -= pl_logdet(wu, th);
}

// one workgroup, every layer: rows b = threadIdx.x + PL_WG * s, s < PL_RPT; the batch-global exit is a __syncthreads_or per iteration
template <int DT>
__global__ void __launch_bounds__(PL_WG) k_planar_inv_wg(float* __restrict__ out, float* __restrict__ ld, float* __restrict__ mids,
                                                         int* __restrict__ iters, NfPlanarPtrs t, int K, int64_t B, int D) {
    __shared__ float sb[NF_PLANAR_MAX_LAYERS], swu[NF_PLANAR_MAX_LAYERS];
    __shared__ float sp[2 * NF_PLANAR_MAX_LAYERS * (DT > 0 ? DT : 1)];
    __shared__ float sz[NF_PLANAR_INV_WG_MAX_ROWS];
    const int Dn = DT > 0 ? DT : D;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        sb[k] = t.p[2 * K + k][0];
        swu[k] = pl_dot(t.p[k], t.p[K + k], Dn);                       // planar.py:49 (no projection in the inverse)
    }
    if (DT > 0) {
        for (int e = threadIdx.x; e < K * DT; e += blockDim.x) {
            const int k = e / DT, d = e - k * DT;
            sp[e] = t.p[k][d];
            sp[K * DT + e] = t.p[K + k][d];
        }
    }
    __syncthreads();
    float lo[PL_RPT], hi[PL_RPT];
    float* const swz = sz;                                             // w.z of the rows (LDS: 64 KB at 16 rows per thread)
    for (int k = K - 1; k >= 0; --k) {
        const float* u = DT > 0 ? sp + k * DT : t.p[k];
        const float* w = DT > 0 ? sp + K * DT + k * DT : t.p[K + k];
        const float wu = swu[k], bb = sb[k];
#pragma unroll
        for (int s = 0; s < PL_RPT; ++s) {
            const int64_t b = threadIdx.x + (int64_t)PL_WG * s;
            swz[s * PL_WG + threadIdx.x] = b < B ? pl_row_wz(out + b * Dn, w, Dn) : 0.0f;
            lo[s] = -1.0e3f;
            hi[s] = 1.0e3f;
        }
        int n = PL_MAX_ITERS;
        for (int it = 1; it <= PL_MAX_ITERS; ++it) {
            bool open = false;
#pragma unroll
            for (int s = 0; s < PL_RPT; ++s) {
                if (threadIdx.x + (int64_t)PL_WG * s < B) open |= !pl_bisect(lo[s], hi[s], swz[s * PL_WG + threadIdx.x], wu, bb);
            }
            if (!__syncthreads_or(open)) {                             // planar.py:60: every row of the batch closed
                n = it;
                break;
            }
        }
#pragma unroll
        for (int s = 0; s < PL_RPT; ++s) {
            const int64_t b = threadIdx.x + (int64_t)PL_WG * s;
            if (b < B) {
                const float mid = (lo[s] + hi[s]) * 0.5f;
                if (mids != nullptr) mids[(int64_t)k * B + b] = mid;
                float l = ld[b];
                pl_finish(out + b * Dn, u, Dn, mid, bb, wu, l);
                ld[b] = l;
            }
        }
        if (threadIdx.x == 0) iters[k] = n;
    }
}

// grid form, layer k, phase 1: 28 iterations from the initial bracket; ctl[2k] = max over rows of the first-close iteration (PL_OPEN: open)
__global__ void __launch_bounds__(NF_BLOCK) k_planar_inv_p1(const float* __restrict__ out, float* __restrict__ lohi, int* __restrict__ ctl,
                                                            NfPlanarPtrs t, int k, int K, int64_t B, int D) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int fc = 0;
    if (b < B) {
        const float wu = pl_dot(t.p[k], t.p[K + k], D), bb = t.p[2 * K + k][0];
        const float wz = pl_row_wz(out + b * D, t.p[K + k], D);
        float lo = -1.0e3f, hi = 1.0e3f;
        for (int it = 1; it <= PL_P1_ITERS; ++it)
            if (pl_bisect(lo, hi, wz, wu, bb) && fc == 0) fc = it;
        lohi[b] = lo;
        lohi[B + b] = hi;
        if (fc == 0) fc = PL_OPEN;
    }
    fc = pl_wave_max(fc);
    if ((threadIdx.x & 63) == 0 && fc > 0) atomicMax(ctl + 2 * k, fc);
}

// phase 2 (only when some bracket is still open after 28): the first iteration <= 100 at which each open row closes -> ctl[2k + 1]
__global__ void __launch_bounds__(NF_BLOCK) k_planar_inv_p2(const float* __restrict__ out, const float* __restrict__ lohi, int* __restrict__ ctl,
                                                            NfPlanarPtrs t, int k, int K, int64_t B, int D) {
    if (ctl[2 * k] <= PL_P1_ITERS) return;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int fc = 0;
    if (b < B) {
        float lo = lohi[b], hi = lohi[B + b];
        if (!(fabsf(hi - lo) < 1.0e-5f)) {
            const float wu = pl_dot(t.p[k], t.p[K + k], D), bb = t.p[2 * K + k][0];
            const float wz = pl_row_wz(out + b * D, t.p[K + k], D);
            fc = PL_MAX_ITERS;
            for (int it = PL_P1_ITERS + 1; it <= PL_MAX_ITERS; ++it)
                if (pl_bisect(lo, hi, wz, wu, bb)) {
                    fc = it;
                    break;
                }
        }
    }
    fc = pl_wave_max(fc);
    if ((threadIdx.x & 63) == 0 && fc > 0) atomicMax(ctl + 2 * k + 1, fc);
}

// finish: N = the first iteration at which every bracket was closed (100 at most); each row's bracket after exactly N iterations
__global__ void __launch_bounds__(NF_BLOCK) k_planar_inv_fin(float* __restrict__ out, float* __restrict__ ld, float* __restrict__ mids,
                                                             int* __restrict__ iters, const float* __restrict__ lohi, const int* __restrict__ ctl,
                                                             NfPlanarPtrs t, int k, int K, int64_t B, int D) {
    const int n1 = ctl[2 * k];
    const int n = n1 <= PL_P1_ITERS ? n1 : ctl[2 * k + 1];
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) iters[k] = n;
    if (b >= B) return;
    const float wu = pl_dot(t.p[k], t.p[K + k], D), bb = t.p[2 * K + k][0];
    float* x = out + b * D;
    float lo, hi;
    if (n < PL_P1_ITERS) {                                             // (a batch of collapsed brackets: re-run from the start)
        const float wz = pl_row_wz(x, t.p[K + k], D);
        lo = -1.0e3f;
        hi = 1.0e3f;
        for (int it = 1; it <= n; ++it) pl_bisect(lo, hi, wz, wu, bb);
    } else {
        lo = lohi[b];
        hi = lohi[B + b];
        if (n > PL_P1_ITERS) {
            const float wz = pl_row_wz(x, t.p[K + k], D);
            for (int it = PL_P1_ITERS + 1; it <= n; ++it) pl_bisect(lo, hi, wz, wu, bb);
        }
    }
    const float mid = (lo + hi) * 0.5f;
    if (mids != nullptr) mids[(int64_t)k * B + b] = mid;
    float l = ld[b];
    pl_finish(x, t.p[k], D, mid, bb, wu, l);
    ld[b] = l;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------------------------------------------------------------------
#define PL_DISPATCH(D, CALL) \
    switch (D) {             \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
        case 5: CALL(5); break; \
        case 6: CALL(6); break; \
        case 7: CALL(7); break; \
        case 8: CALL(8); break; \
        default: CALL(0); break; \
    }

static bool pl_shape_ok(int K, int64_t B, int D) { return K >= 1 && K <= NF_PLANAR_MAX_LAYERS && B >= 0 && D >= 1 && B * (int64_t)D < ((int64_t)1 << 40); }

extern "C" int nf_planar_project(const int64_t* params, int K, int D, nf_stream_t stream) {
    NfPlanarPtrs t;
    if (!pl_shape_ok(K, 0, D) || !pl_table(t, params, K, true)) return NF_E_BADARG;
    hipLaunchKernelGGL(k_planar_project, dim3(1), dim3(NF_BLOCK), 0, (hipStream_t)stream, t, K, D);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_planar_fwd(const float* z, float* out, float* ld, float* save, const int64_t* params, int K, int64_t B, int D,
                             nf_stream_t stream) {
    NfPlanarPtrs t;
    if (!pl_shape_ok(K, B, D) || !pl_table(t, params, K, true)) return NF_E_BADARG;
    if (B > 0 && (z == nullptr || out == nullptr || ld == nullptr)) return NF_E_BADARG;
    if (B == 0) return 0;
    const unsigned g = (unsigned)((B + NF_BLOCK - 1) / NF_BLOCK);
#define CALL(DT) hipLaunchKernelGGL(k_planar_fwd<DT>, dim3(g), dim3(NF_BLOCK), 0, (hipStream_t)stream, z, out, ld, save, t, K, B, D)
    PL_DISPATCH(D, CALL);
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_planar_bwd_slab_floats(int K, int64_t B, int D, int64_t* n_floats) {
    if (!pl_shape_ok(K, B, D) || n_floats == nullptr) return NF_E_BADARG;
    const int64_t g = (B + NF_BLOCK - 1) / NF_BLOCK;
    *n_floats = g * (NF_BLOCK / NF_WAVE) * (int64_t)K * (2 * D + 1);
    return 0;
}

extern "C" int nf_planar_bwd(const float* g_out, const float* g_ld, const float* save, const int64_t* params, const int64_t* grads,
                             float* g_z, float* slab, int K, int64_t B, int D, nf_stream_t stream) {
    NfPlanarPtrs t, gp;
    if (!pl_shape_ok(K, B, D) || !pl_table(t, params, K, true) || !pl_table(gp, grads, K, true)) return NF_E_BADARG;
    if (B > 0 && (g_out == nullptr || g_ld == nullptr || save == nullptr || slab == nullptr)) return NF_E_BADARG;
    if (D > 8 && B > 0 && g_z == nullptr) return NF_E_BADARG;               // the generic form keeps the row's gradient there
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t g = (B + NF_BLOCK - 1) / NF_BLOCK;
    if (g > 0x7fffffff) return NF_E_BADARG;
#define CALL(DT) hipLaunchKernelGGL(k_planar_bwd<DT>, dim3((unsigned)g), dim3(NF_BLOCK), 0, st, g_out, g_ld, save, g_z, slab, t, K, B, D)
    PL_DISPATCH(D, CALL);
#undef CALL
    NF_CHECK_LAUNCH();
    const int64_t n_el = (int64_t)K * (2 * D + 1);
    const int64_t fb = (n_el + NF_BLOCK / NF_WAVE - 1) / (NF_BLOCK / NF_WAVE);
    hipLaunchKernelGGL(k_planar_fold, dim3((unsigned)fb), dim3(NF_BLOCK), 0, st, slab, g * (NF_BLOCK / NF_WAVE), gp, K, D);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_planar_inv(const float* z, float* out, float* ld, float* mids, int* iters, float* scratch, int* ctl, const int64_t* params,
                             int K, int64_t B, int D, nf_stream_t stream) {
    NfPlanarPtrs t;
    if (!pl_shape_ok(K, B, D) || !pl_table(t, params, K, true) || iters == nullptr) return NF_E_BADARG;
    if (B > 0 && (z == nullptr || out == nullptr || ld == nullptr)) return NF_E_BADARG;
    const bool wg = nf_pl_mode == 0 && B <= NF_PLANAR_INV_WG_MAX_ROWS;
    if (!wg && (scratch == nullptr || ctl == nullptr)) return NF_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(iters, 0, sizeof(int) * K, st);
    if (e != hipSuccess) return (int)e;
    if (B == 0) return 0;
    if (out != z) {
        e = hipMemcpyAsync(out, z, sizeof(float) * B * D, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    if (wg) {
#define CALL(DT) hipLaunchKernelGGL(k_planar_inv_wg<DT>, dim3(1), dim3(PL_WG), 0, st, out, ld, mids, iters, t, K, B, D)
        PL_DISPATCH(D, CALL);
#undef CALL
        NF_CHECK_LAUNCH();
        return 0;
    }
    e = hipMemsetAsync(ctl, 0, sizeof(int) * 2 * K, st);
    if (e != hipSuccess) return (int)e;
    const int64_t g = (B + NF_BLOCK - 1) / NF_BLOCK;
    if (g > 0x7fffffff) return NF_E_BADARG;
    for (int k = K - 1; k >= 0; --k) {
        hipLaunchKernelGGL(k_planar_inv_p1, dim3((unsigned)g), dim3(NF_BLOCK), 0, st, out, scratch, ctl, t, k, K, B, D);
        hipLaunchKernelGGL(k_planar_inv_p2, dim3((unsigned)g), dim3(NF_BLOCK), 0, st, out, scratch, ctl, t, k, K, B, D);
        hipLaunchKernelGGL(k_planar_inv_fin, dim3((unsigned)g), dim3(NF_BLOCK), 0, st, out, ld, mids, iters, scratch, ctl, t, k, K, B, D);
        NF_CHECK_LAUNCH();
    }
    return 0;
}
