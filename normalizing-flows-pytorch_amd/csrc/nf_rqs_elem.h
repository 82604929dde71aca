// One element of the monotone rational-quadratic spline coupling (Durkan et al. 2019, "Neural Spline Flows", eq. 4-8 and the
// inverse of their appendix A.1), shared by every kernel of rqspline.hip.  Plain C++ without any device intrinsic: the element
// functions also compile for the host (NF_RQS_FN empty), which is how their arithmetic is checked against the float64 restatement.
//
// Raw parameters of one transformed element: rw[0..K) | rh[0..K) | rd[0..K-1), parameter p at P[p * nh].
//   widths   w_j = 2 bound (min + (1 - K min) softmax(rw)_j), heights the same from rh
//   knots    x_0 = y_0 = -bound, x_j = -bound + sum_{i<j} w_i, the last knot exactly +bound; bin sizes are KNOT DIFFERENCES
//   slopes   d_0 = d_K = 1, interior d_j = min + softplus(rd_{j-1} + c), c = log(expm1(1 - min)): zero parameters are the identity
//   inside   -bound < x < bound (strict); outside the element passes through bit for bit with a zero log-det term
//
// No array is indexed by a run-time value: the K-loops are unrolled, one running scan over the knots finds the bin and carries the
// bin's (x_k, y_k, x_{k+1}, y_{k+1}) and its two raw slope parameters along by selects, so everything stays in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef NF_RQS_FN
#define NF_RQS_FN __device__ __forceinline__
#endif

#define NF_RQS_MIN 1.0e-3f            // min_w = min_h = min_d
#define NF_RQS_DC 0.539742417236952f  // log(expm1(1 - min_d))

NF_RQS_FN float nf_rqs_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }      // F.softplus: beta 1, threshold 20
NF_RQS_FN bool nf_rqs_inside(float v, float bound) { return v > -bound && v < bound; }  // (a NaN is outside: it passes through)

// what the scan leaves: the bin's corners, its index, its raw slope parameters, and of the two softmaxes the bin's own
// un-normalised weight and the sum of those before it (for the backward's softmax Jacobians)
struct NfRqsBin {
    float xk, yk, xk1, yk1, rdk, rdk1;
    float ewk, ehk, cew, ceh;
    int k;
};

// exp(r_j - max r) of the width and height logits and their sums.  The sums here and the running sums of the scan are kept in double
// (full rate on this device, a handful of live values): the inverse amplifies a knot's error by dx/dy, which inside a flat bin is in the
// hundreds, so the knots are the correctly rounded sums of the float32 terms instead of carrying K additions' worth of rounding.
template <int K>
NF_RQS_FN void nf_rqs_softmax(const float* P, int64_t nh, float (&ew)[K], float (&eh)[K], double& sw, double& sh) {
    float mw = -INFINITY, mh = -INFINITY;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        ew[j] = P[j * nh];
        eh[j] = P[(K + j) * nh];
        mw = fmaxf(mw, ew[j]);
        mh = fmaxf(mh, eh[j]);
    }
    sw = 0.0; sh = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        ew[j] = expf(ew[j] - mw);
        eh[j] = expf(eh[j] - mh);
        sw += (double)ew[j];
        sh += (double)eh[j];
    }
}

// the running scan: v is compared with the x knots (INV = false) or the y knots (INV = true); bin k = the last knot j <= K - 1 with
// v >= knot_j (the knots increase strictly: every bin is at least 2 bound min wide)
template <int K, bool INV>
NF_RQS_FN void nf_rqs_scan(const float* P, int64_t nh, float bound, float v, const float (&ew)[K], const float (&eh)[K], double sw, double sh,
                           NfRqsBin& b) {
    const double c0 = 2.0 * bound * (double)NF_RQS_MIN, c1 = 2.0 * bound * (1.0 - K * (double)NF_RQS_MIN);
    const double cw = c1 / sw, ch = c1 / sh;
    double cumx = -(double)bound, cumy = -(double)bound;
    float kx = -bound, ky = -bound, rd = 0.f, cew = 0.f, ceh = 0.f;
    b.k = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        cumx += c0 + cw * (double)ew[j];
        cumy += c0 + ch * (double)eh[j];
        const float nx = j == K - 1 ? bound : (float)cumx;
        const float ny = j == K - 1 ? bound : (float)cumy;
        const float rn = j == K - 1 ? 0.f : P[(2 * K + j) * nh];
        const bool sel = j == 0 || (INV ? v >= ky : v >= kx);
        b.xk = sel ? kx : b.xk;   b.yk = sel ? ky : b.yk;
        b.xk1 = sel ? nx : b.xk1; b.yk1 = sel ? ny : b.yk1;
        b.rdk = sel ? rd : b.rdk; b.rdk1 = sel ? rn : b.rdk1;
        b.ewk = sel ? ew[j] : b.ewk; b.ehk = sel ? eh[j] : b.ehk;
        b.cew = sel ? cew : b.cew;   b.ceh = sel ? ceh : b.ceh;
        b.k = sel ? j : b.k;
        kx = nx; ky = ny; rd = rn;
        cew += ew[j]; ceh += eh[j];
    }
}

// y (or the inverse's x) of an element INSIDE the interval; acc += (forward) / -= (inverse) log dy/dx.          eq. 4, 5 and A.1
template <int K, bool INV>
NF_RQS_FN float nf_rqs_elem(const float* P, int64_t nh, float bound, float v, float& acc) {
    float ew[K], eh[K];
    double sw, sh;
    NfRqsBin b;
    nf_rqs_softmax<K>(P, nh, ew, eh, sw, sh);
    nf_rqs_scan<K, INV>(P, nh, bound, v, ew, eh, sw, sh, b);
    const float dk = b.k == 0 ? 1.f : NF_RQS_MIN + nf_rqs_softplus(b.rdk + NF_RQS_DC);
    const float dk1 = b.k == K - 1 ? 1.f : NF_RQS_MIN + nf_rqs_softplus(b.rdk1 + NF_RQS_DC);
    const float W = b.xk1 - b.xk, H = b.yk1 - b.yk, s = H / W, T = dk1 + dk - 2.f * s;
    float th;
    if (!INV) {
        th = (v - b.xk) / W;
    } else {
        const float dy = v - b.yk, t = dy * T;
        const float qa = H * (s - dk) + t, qb = H * dk - t, qc = -s * dy;
        th = 2.f * qc / (-qb - sqrtf(fmaxf(qb * qb - 4.f * qa * qc, 0.f)));      // the root of A.1 in its cancellation-free form
        th = fminf(fmaxf(th, 0.f), 1.f);
    }
    const float q = th * (1.f - th), D = s + T * q;
    const float E = dk1 * th * th + 2.f * s * q + dk * (1.f - th) * (1.f - th);
    const float l = logf(s * s * E) - 2.f * logf(D);
    if (!INV) {
        acc += l;
        return b.yk + H * (s * th * th + dk * q) / D;
    }
    acc -= l;
    return fminf(b.xk + th * W, b.xk1);      // (x_k + W can round one ulp past x_k+1 in a wide bin: the inverse stays inside [-bound, bound])
}

// autograd of the forward direction for one element: returns g_x and WRITES the element's 3K - 1 parameter gradients to GP[p * gnh].
// P may BE GP (a staged row that is overwritten in place): every parameter is read before the first store.
template <int K>
NF_RQS_FN float nf_rqs_bwd_elem(const float* P, int64_t nh, float* GP, int64_t gnh, float bound, float x, float gy, float gl) {
    if (!nf_rqs_inside(x, bound)) {
#pragma unroll
        for (int p = 0; p < 3 * K - 1; ++p) GP[p * gnh] = 0.f;
        return gy;
    }
    float ew[K], eh[K];
    double sw, sh;
    NfRqsBin b;
    nf_rqs_softmax<K>(P, nh, ew, eh, sw, sh);
    nf_rqs_scan<K, false>(P, nh, bound, x, ew, eh, sw, sh, b);
    const bool first = b.k == 0, last = b.k == K - 1;
    const float uk = b.rdk + NF_RQS_DC, uk1 = b.rdk1 + NF_RQS_DC;
    const float dk = first ? 1.f : NF_RQS_MIN + nf_rqs_softplus(uk);
    const float dk1 = last ? 1.f : NF_RQS_MIN + nf_rqs_softplus(uk1);
    const float W = b.xk1 - b.xk, H = b.yk1 - b.yk, rW = 1.f / W, s = H * rW, T = dk1 + dk - 2.f * s;
    const float th = (x - b.xk) * rW, omt = 1.f - th, q = th * omt;
    const float A = s * th * th + dk * q, D = s + T * q, rD = 1.f / D;
    const float E = dk1 * th * th + 2.f * s * q + dk * omt * omt, rE = 1.f / E;
    const float HD2 = H * rD * rD;
    // partial derivatives of y = y_k + H A / D and l = 2 log s + log E - 2 log D with respect to (th, s, d_k, d_k+1), H and y_k explicit
    const float y_th = HD2 * s * E;
    const float y_s = HD2 * q * (th * th * T - dk + 2.f * A);
    const float y_dk = HD2 * q * (s * omt * omt + dk1 * q);
    const float y_dk1 = -HD2 * q * A;
    const float l_th = (2.f * dk1 * th + 2.f * s * (1.f - 2.f * th) - 2.f * dk * omt) * rE - 2.f * T * (1.f - 2.f * th) * rD;
    const float l_s = 2.f / s + 2.f * q * rE - 2.f * (1.f - 2.f * q) * rD;
    const float l_dk = omt * omt * rE - 2.f * q * rD;
    const float l_dk1 = th * th * rE - 2.f * q * rD;
    const float g_th = gy * y_th + gl * l_th, g_s = gy * y_s + gl * l_s;
    const float g_dk = gy * y_dk + gl * l_dk, g_dk1 = gy * y_dk1 + gl * l_dk1;
    // th = (x - x_k) / W, s = H / W, W = x_k+1 - x_k, H = y_k+1 - y_k
    const float g_x = g_th * rW;
    const float g_W = -(g_th * th + g_s * s) * rW;
    const float g_H = gy * A * rD + g_s * rW;
    const float g_xk = -g_x - g_W, g_yk = gy - g_H;
    const float g_xk1 = last ? 0.f : g_W, g_yk1 = last ? 0.f : g_H;       // the last knot is the constant +bound (x_0 = -bound: no width precedes it)
    // knot j >= 1 is -bound + the widths before it: width i receives g_xk if i < k and g_xk1 if i <= k; then w = 2 bound (min + (1 - K min) p),
    // p = softmax: g_r_i = p_i (g_p_i - sum_j p_j g_p_j), the sum from the scan's running totals
    const float cg = 2.f * bound * (1.f - K * NF_RQS_MIN);
    const float rsw = 1.f / (float)sw, rsh = 1.f / (float)sh;
    const float dot_w = cg * (g_xk * b.cew + g_xk1 * (b.cew + b.ewk)) * rsw;
    const float dot_h = cg * (g_yk * b.ceh + g_yk1 * (b.ceh + b.ehk)) * rsh;
    // softplus'(u) = sigmoid(u)
    const float g_rdk = first ? 0.f : g_dk / (1.f + expf(-uk));
    const float g_rdk1 = last ? 0.f : g_dk1 / (1.f + expf(-uk1));
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float gw = cg * ((j < b.k ? g_xk : 0.f) + (j <= b.k ? g_xk1 : 0.f));
        const float gh = cg * ((j < b.k ? g_yk : 0.f) + (j <= b.k ? g_yk1 : 0.f));
        GP[j * gnh] = ew[j] * rsw * (gw - dot_w);
        GP[(K + j) * gnh] = eh[j] * rsh * (gh - dot_h);
        if (j < K - 1) GP[(2 * K + j) * gnh] = (j == b.k - 1 ? g_rdk : 0.f) + (j == b.k ? g_rdk1 : 0.f);
    }
    return g_x;
}
