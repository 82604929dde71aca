// FFJORD (flows/cnf.py, flows/odeint.py): a whole ODE integration of a continuous normalizing flow layer per launch, in fp64.
//
//   schedule   nf_cnf_schedule   HOST: the reference's host loops (odeint.py:13-20, :68-94) turned into the flat list of stage times, the
//                                per-step dt and the final lerp slope, with the same IEEE double operations in the same order
//   forward    nf_cnf_integrate  one row per lane; the state, the hidden activations and the tangents in registers, the stage vectors k_i
//                                in private memory (indexed by the runtime stage), the weights wave-uniform operands from LDS.  The trace
//                                comes from forward-mode tangents in the same pass as the value: one per noise sample (Hutchinson,
//                                cnf.py:22-37) or D unit tangents (exact, cnf.py:10-19).  No autograd.
//   adjoint    nf_cnf_adjoint    (a_z, z, ld) per row over the reversed schedule (odeint.py:266-284); the VJP through value and tangent
//                                passes by hand (second order through softplus).  g_theta feeds nothing back, so it is the sum over steps
//                                and stages of (final-row tableau weight x dt x vjp_theta): every workgroup (one wave, 64 rows) contracts
//                                its rows through LDS into accumulators it owns for the whole integration and writes ONE slab at the end;
//                                a fixed-order fold launch sums the slabs (no float atomics: bit-reproducible).
//
// The "adaptive" solvers of the reference discard their step proposal (odeint.py:80), so all four methods are fixed tableaus here.
#include <cmath>

#include "nf_common.h"
#include "nf_philox.h"

#define CNF_H NF_CNF_HIDDEN
#define CNF_WG 64                      // one wave per workgroup: the contraction's barriers are wave-local, small batches spread over CUs
#define CNF_STAGES 7
#define CNF_LS 33                      // row strides (doubles) of the contraction buffers: odd, so that lanes spread over the banks
#define CNF_RS 35

// ---------------------------------------------------------------------------------------------------------------------------------------
// tableaus: A[m][i][j] multiplies k_j in the argument of stage i, Bw[m][i] in dx; rk4 divides its sum by 6 (odeint.py:51)
// ---------------------------------------------------------------------------------------------------------------------------------------
struct CnfTableau {
    int stages;
    double div;
    double ct[CNF_STAGES];
    double a[CNF_STAGES][CNF_STAGES];
    double b[CNF_STAGES];
};

#define CNF_TABLEAUS \
    /* odeint.py:33-36 */ \
    {2, 1.0, {0.0, 0.5}, {{0.0}, {0.5}}, {0.0, 1.0}}, \
    /* odeint.py:46-52 */ \
    {4, 6.0, {0.0, 0.5, 0.5, 1.0}, {{0.0}, {0.5}, {0.0, 0.5}, {0.0, 0.0, 1.0}}, {1.0, 2.0, 2.0, 1.0}}, \
    /* odeint.py:118-133 (five evaluations; the last enters neither dx nor a later stage) */ \
    {5, \
     1.0, \
     {0.0, 1.0 / 2.0, 3.0 / 4.0, 1.0, 1.0}, \
     {{0.0}, {1.0 / 2.0}, {0.0, 3.0 / 4.0}, {2.0 / 9.0, 1.0 / 3.0, 4.0 / 9.0}, {2.0 / 9.0, 1.0 / 3.0, 4.0 / 9.0, 0.0}}, \
     {2.0 / 9.0, 1.0 / 3.0, 4.0 / 9.0, 0.0, 0.0}}, \
    /* odeint.py:140-160 (seven evaluations) */ \
    {7, \
     1.0, \
     {0.0, 1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0, 1.0}, \
     {{0.0}, \
      {1.0 / 5.0}, \
      {3.0 / 40.0, 9.0 / 40.0}, \
      {44.0 / 45.0, -56.0 / 15.0, 32.0 / 9.0}, \
      {19372.0 / 6561.0, -25360.0 / 2187.0, 64448.0 / 6561.0, -212.0 / 729.0}, \
      {9017.0 / 3168.0, -355.0 / 33.0, 46732.0 / 5247.0, 49.0 / 176.0, -5103.0 / 18656.0}, \
      {35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0}}, \
     {35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0, 0.0}},

static const CnfTableau h_tab[4] = {CNF_TABLEAUS};          // the copy of the host (nf_cnf_schedule)
__constant__ CnfTableau c_tab[4] = {CNF_TABLEAUS};

static bool cnf_method_ok(int m) { return m >= NF_CNF_MIDPOINT && m <= NF_CNF_DOPRI5; }

// ---------------------------------------------------------------------------------------------------------------------------------------
// schedule (host)
// ---------------------------------------------------------------------------------------------------------------------------------------
extern "C" int nf_cnf_schedule(const double* times, int n_times, int method, double* stage_t, double* step_dt, double* slope, int* n_steps,
                               int cap_steps) {
    if (times == nullptr || n_times < 2 || !cnf_method_ok(method) || slope == nullptr || n_steps == nullptr) return NF_E_BADARG;
    if ((stage_t == nullptr) != (step_dt == nullptr) || cap_steps < 0) return NF_E_BADARG;
    for (int i = 0; i < n_times; ++i)
        if (!std::isfinite(times[i])) return NF_E_BADARG;
    const CnfTableau& tb = h_tab[method];
    const bool write = stage_t != nullptr;
    int n = 0;
    if (method == NF_CNF_MIDPOINT || method == NF_CNF_RK4) {               // ODESolver.integrate, odeint.py:13-20
        for (int k = 0; k + 1 < n_times; ++k) {
            if (n >= NF_CNF_MAX_STEPS || (write && n >= cap_steps)) return NF_E_BADARG;
            const double t0 = times[k], dt = times[k + 1] - t0;
            if (write) {
                step_dt[n] = dt;
                stage_t[n * tb.stages] = t0;
                for (int i = 1; i < tb.stages; ++i) stage_t[n * tb.stages + i] = tb.ct[i] == 1.0 ? t0 + dt : t0 + tb.ct[i] * dt;
            }
            ++n;
        }
        *slope = 1.0;
        *n_steps = n;
        return 0;
    }
    // AdaptiveODESolver.integrate, odeint.py:68-94
    const double t_start = times[0], t_end = times[n_times - 1];
    double dt = (t_end - t_start) / (double)(n_times - 1);
    if (!(std::fabs(dt) > 0.0)) return NF_E_BADARG;
    const double dt_min = std::fabs(dt) * 0.2, dt_max = std::fabs(dt) * 5.0;
    double t0 = t_start, t1 = t_start;
    while (std::fabs(t1 - t_end) > 1.0e-4) {
        if (n >= NF_CNF_MAX_STEPS || (write && n >= cap_steps)) return NF_E_BADARG;
        if (write) {
            step_dt[n] = dt;
            stage_t[n * tb.stages] = t1;                                     // _step_fn, odeint.py:96-102
            for (int i = 1; i < tb.stages; ++i) stage_t[n * tb.stages + i] = t1 + tb.ct[i] * dt;
        }
        const double ad = std::fmin(std::fmax(std::fabs(dt), dt_min), dt_max);   // torch.clamp(torch.abs(dt), dt_min, dt_max)
        dt = ad * (dt > 0.0 ? 1.0 : (dt < 0.0 ? -1.0 : 0.0));                    // * torch.sign(dt)
        if ((t_start - (t1 + dt)) * (t_end - (t1 + dt)) > 0.0) dt = t_end - t1;
        t0 = t1;
        t1 = t1 + dt;
        ++n;
    }
    if (n == 0) return NF_E_BADARG;
    *slope = (t_end - t0) / (t1 - t0);
    *n_steps = n;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------------------------------------------------
struct CnfPtrs {
    const double* p[6];                // W1 (32, D+1), b1, W2 (32, 33), b2, W3 (D, 33), b3
};

template <int DT>
struct CnfW {                          // the field's weights in LDS, the t column apart, padded to DT features with zeros
    double w1t[CNF_H], w1x[CNF_H * DT], b1[CNF_H];
    double w2t[CNF_H], w2x[CNF_H * CNF_H], b2[CNF_H];
    double w3t[DT], w3x[DT * CNF_H], b3[DT];
};

template <int DT>
__device__ __forceinline__ void cnf_stage_weights(CnfW<DT>& w, const CnfPtrs& p, int D) {
    for (int i = threadIdx.x; i < CNF_H; i += blockDim.x) {
        w.w1t[i] = p.p[0][i * (D + 1)];
        w.b1[i] = p.p[1][i];
        w.w2t[i] = p.p[2][i * (CNF_H + 1)];
        w.b2[i] = p.p[3][i];
#pragma unroll
        for (int d = 0; d < DT; ++d) w.w1x[i * DT + d] = d < D ? p.p[0][i * (D + 1) + 1 + d] : 0.0;
    }
    for (int e = threadIdx.x; e < CNF_H * CNF_H; e += blockDim.x) w.w2x[e] = p.p[2][(e >> 5) * (CNF_H + 1) + 1 + (e & 31)];
    for (int e = threadIdx.x; e < DT * CNF_H; e += blockDim.x) {
        const int d = e >> 5, j = e & 31;
        w.w3x[e] = d < D ? p.p[4][d * (CNF_H + 1) + 1 + j] : 0.0;
    }
    for (int d = threadIdx.x; d < DT; d += blockDim.x) {
        w.w3t[d] = d < D ? p.p[4][d * (CNF_H + 1)] : 0.0;
        w.b3[d] = d < D ? p.p[5][d] : 0.0;
    }
    __syncthreads();
}

// F.softplus (beta 1, threshold 20) with its first derivative: x above the threshold, else log1p(e^x) and e^x / (e^x + 1).  The second
// derivative is s (1 - s), which is 0 where s is exactly 1 (above the threshold) and nowhere else (s <= 1 - 2e-9 at x <= 20).
__device__ __forceinline__ void cnf_softplus(double x, double& a, double& s) {
    if (x > 20.0) {
        a = x;
        s = 1.0;
    } else {
        const double e = exp(x);
        a = log1p(e);
        s = e / (e + 1.0);
    }
}

// The 32-wide vectors of a row live in registers (static indices); a product with 32 outputs runs its output index as a runtime loop
// (32 x less code than the full unroll) and hands the outputs back through the lane's own row of an LDS staging buffer.  Lane-private
// traffic: no barrier.  W[i * RS + j * CS]: RS = NIN, CS = 1 for W x; RS = 1, CS = 32 for W^T x.
template <int NIN, int RS, int CS>
__device__ __forceinline__ void cnf_matvec(const double* __restrict__ W, const double (&in)[NIN], double* __restrict__ st, double (&out)[CNF_H]) {
#pragma unroll 4
    for (int i = 0; i < CNF_H; ++i) {                                     // (four independent FMA chains in flight: one wave per SIMD)
        double h = 0.0;
#pragma unroll
        for (int j = 0; j < NIN; ++j) h = fma(W[i * RS + j * CS], in[j], h);
        st[i] = h;
    }
#pragma unroll
    for (int i = 0; i < CNF_H; ++i) out[i] = st[i];
}

// a ConcatLinear with its softplus (cnf.py:48-51, :117): a = softplus(W x + wt t + b), s = softplus'
template <int NIN>
__device__ __forceinline__ void cnf_layer(const double* __restrict__ W, const double* __restrict__ wt, const double* __restrict__ bias, double t,
                                          const double (&in)[NIN], double* __restrict__ sta, double* __restrict__ sts, double (&a)[CNF_H],
                                          double (&s)[CNF_H]) {
#pragma unroll 4
    for (int i = 0; i < CNF_H; ++i) {
        double h = fma(wt[i], t, bias[i]);
#pragma unroll
        for (int j = 0; j < NIN; ++j) h = fma(W[i * NIN + j], in[j], h);
        double av, sv;
        cnf_softplus(h, av, sv);
        sta[i] = av;
        sts[i] = sv;
    }
#pragma unroll
    for (int i = 0; i < CNF_H; ++i) {
        a[i] = sta[i];
        s[i] = sts[i];
    }
}

// Contraction over the 64 rows of the wave: acc[jj] += sum_r L_r[i] * R_r[g * PER + jj] for the (i, g) this lane owns.  L carries the
// stage weight (0 for dead lanes).  The same ownership map writes the slab at the end.
template <int NL, int NR, int PER, int ISHIFT>
__device__ __forceinline__ void cnf_contract(double* __restrict__ lb, double* __restrict__ rb, const double (&L)[NL], double scale,
                                             const double (&R)[NR], double (&acc)[PER]) {
    const int lane = threadIdx.x;
    __syncthreads();                                                     // (the buffers double as the lanes' staging rows)
#pragma unroll
    for (int i = 0; i < NL; ++i) lb[lane * CNF_LS + i] = L[i] * scale;
#pragma unroll
    for (int j = 0; j < NR; ++j) rb[lane * CNF_RS + j] = R[j];
    __syncthreads();
    const int i = lane & ((1 << ISHIFT) - 1), g = lane >> ISHIFT;
    const bool row_ok = i < NL;
    const int ic = row_ok ? i : 0;
#pragma unroll 2
    for (int r = 0; r < CNF_WG; ++r) {
        const double l = row_ok ? lb[r * CNF_LS + ic] : 0.0;
#pragma unroll
        for (int jj = 0; jj < PER; ++jj) {
            const int j = g * PER + jj;
            const double rv = j < NR ? rb[r * CNF_RS + (j < NR ? j : 0)] : 0.0;
            acc[jj] = fma(l, rv, acc[jj]);
        }
    }
    __syncthreads();
}

// the noise vector of (evaluation e, row b, sample s): explicit tensor, in-kernel Philox, or the unit tangent e_s (exact trace)
template <int DT>
__device__ __forceinline__ void cnf_tangent(double (&v)[DT], int trace, const float* __restrict__ noise, unsigned k0, unsigned k1, int64_t e,
                                            int64_t b, int64_t B, int s, int S, int D, bool live) {
    if (trace == NF_CNF_TRACE_EXACT) {
#pragma unroll
        for (int d = 0; d < DT; ++d) v[d] = d == s ? 1.0 : 0.0;
        return;
    }
    if (noise != nullptr) {
        const float* src = noise + ((e * B + (live ? b : 0)) * S + s) * D;
#pragma unroll
        for (int d = 0; d < DT; ++d) v[d] = (live && d < D) ? (double)src[d] : 0.0;
        return;
    }
    float n[8];
#pragma unroll
    for (int h = 0; h < (DT + 3) / 4; ++h) {
        const NfPhilox r = nf_philox((unsigned)b, (unsigned)((uint64_t)b >> 32), (unsigned)e, (unsigned)(2 * s + h), k0, k1);
        nf_box_muller(r.c[0], r.c[1], n[4 * h], n[4 * h + 1]);
        nf_box_muller(r.c[2], r.c[3], n[4 * h + 2], n[4 * h + 3]);
    }
#pragma unroll
    for (int d = 0; d < DT; ++d) v[d] = d < D ? (double)n[d] : 0.0;
}

// the Philox key of a pass: seed[0] the seed, seed[1] the stream offset the host moves on with every pass (device memory: no host sync)
__device__ __forceinline__ void cnf_keys(const int64_t* __restrict__ seed, unsigned& k0, unsigned& k1) {
    const uint64_t sd = (uint64_t)seed[0], off = (uint64_t)seed[1];
    k0 = (unsigned)sd ^ ((unsigned)off * 0x9E3779B9u);
    k1 = (unsigned)(sd >> 32) ^ (unsigned)(off >> 32) ^ 0x5bd1e995u;
}

__device__ __forceinline__ double cnf_load(const void* p, int64_t i, bool f64) {
    return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}
__device__ __forceinline__ void cnf_store(void* p, int64_t i, bool f64, double v) {
    if (f64) ((double*)p)[i] = v;
    else ((float*)p)[i] = (float)v;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// One kernel body for both passes.  ADJ = false: x = (z, ld), dx/dt = (f, trace).  ADJ = true: x = (a_z, z, ld) with a_ld constant,
// dx/dt = (-a^T dF/dz, f, trace) and the parameter VJP contracted into the lane-owned accumulators with the stage's weight.
// ---------------------------------------------------------------------------------------------------------------------------------------
template <int DT, bool ADJ>
__global__ void __launch_bounds__(CNF_WG) k_cnf(const void* __restrict__ in_z, const void* __restrict__ in_ld, void* __restrict__ out_z,
                                                void* __restrict__ out_ld, double* __restrict__ state, double* __restrict__ slab, CnfPtrs prm,
                                                const double* __restrict__ sched, int n_steps, int method, int trace, int S,
                                                const float* __restrict__ noise, const int64_t* __restrict__ seed, int f64, int64_t B, int D) {
    constexpr int NS = ADJ ? 2 * DT + 1 : DT + 1;      // state length per row
    constexpr int ZO = ADJ ? DT : 0;                   // offset of z in the state
    constexpr int LO = ZO + DT;                        // offset of ld
    constexpr int NR1 = DT + 2, PER1 = (NR1 + 1) / 2;  // layer 1 right vector [z, 1, t]; two column groups of 32 lanes
    constexpr int NR2 = CNF_H + 2, PER2 = NR2 / 2;     // layer 2 right vector [a1, 1, t]
    constexpr int PER3 = 5;                            // layer 3: 8 row lanes x 8 column groups of 5 (34 columns used)
    __shared__ CnfW<DT> w;
    __shared__ double lbuf[CNF_WG * CNF_LS];
    __shared__ double rbuf[CNF_WG * CNF_RS];
    cnf_stage_weights<DT>(w, prm, D);

    const int lane = threadIdx.x;
    double* const sta = lbuf + lane * CNF_LS;          // the lane's staging rows
    double* const stb = rbuf + lane * CNF_RS;
    const int64_t b = (int64_t)blockIdx.x * CNF_WG + lane;
    const bool live = b < B;
    const int64_t bl = live ? b : 0;
    const bool is64 = f64 != 0;
    const CnfTableau& tb = c_tab[method];
    const int nst = tb.stages;
    const bool lerp = method >= NF_CNF_BOSHA3;
    const double slope = sched[0];
    const double* __restrict__ step_dt = sched + 1;
    const double* __restrict__ stage_t = sched + 1 + n_steps;
    const int ntan = trace == NF_CNF_TRACE_EXACT ? D : S;
    const double tr_div = trace == NF_CNF_TRACE_EXACT ? 1.0 : (double)S;
    unsigned k0 = 0, k1 = 0;
    if (noise == nullptr && trace != NF_CNF_TRACE_EXACT) cnf_keys(seed, k0, k1);

    double x[NS], xp[NS], ks[CNF_STAGES][NS];
    double a_ld = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) x[c] = 0.0;
    if (live) {
        if constexpr (ADJ) {
#pragma unroll
            for (int d = 0; d < DT; ++d)
                if (d < D) {
                    x[d] = cnf_load(in_z, bl * D + d, is64);             // the incoming gradient of z
                    x[ZO + d] = state[bl * (D + 1) + d];
                }
            x[LO] = state[bl * (D + 1) + D];
            a_ld = cnf_load(in_ld, bl, is64);
        } else {
#pragma unroll
            for (int d = 0; d < DT; ++d)
                if (d < D) x[d] = cnf_load(in_z, bl * D + d, is64);
            x[LO] = cnf_load(in_ld, bl, is64);
        }
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) xp[c] = x[c];

    double acc1[PER1], acc2[PER2], acc3[PER3];
#pragma unroll
    for (int j = 0; j < PER1; ++j) acc1[j] = 0.0;
#pragma unroll
    for (int j = 0; j < PER2; ++j) acc2[j] = 0.0;
#pragma unroll
    for (int j = 0; j < PER3; ++j) acc3[j] = 0.0;

    for (int step = 0; step < n_steps; ++step) {
        const double dt = step_dt[step];
#pragma unroll 1
        for (int st = 0; st < nst; ++st) {
            // the argument of the stage: x + sum_j k_j a_ij (odeint.py:100-101), in the reference's order
            double xs[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                double kx = 0.0;
                for (int j = 0; j < st; ++j) kx += ks[j][c] * tb.a[st][j];
                xs[c] = st == 0 ? x[c] : x[c] + kx;
            }
            const double t = stage_t[step * nst + st];
            const int64_t e = (int64_t)step * nst + st;
            // the weight this evaluation's parameter VJP has in g_theta: final-row weight x dt (x slope in the last step of a lerped method)
            const double wgt = ADJ ? tb.b[st] / tb.div * dt * ((lerp && step == n_steps - 1) ? slope : 1.0) : 0.0;
            const double lw = live ? wgt : 0.0;

            // ---- value pass (cnf.py:113-117)
            double zz[DT], a1[CNF_H], s1[CNF_H], a2[CNF_H], s2[CNF_H], f[DT];
#pragma unroll
            for (int d = 0; d < DT; ++d) zz[d] = xs[ZO + d];
            cnf_layer<DT>(w.w1x, w.w1t, w.b1, t, zz, sta, stb, a1, s1);
            cnf_layer<CNF_H>(w.w2x, w.w2t, w.b2, t, a1, sta, stb, a2, s2);
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                double h = fma(w.w3t[d], t, w.b3[d]);
#pragma unroll
                for (int j = 0; j < CNF_H; ++j) h = fma(w.w3x[d * CNF_H + j], a2[j], h);
                f[d] = h;
            }

            // ---- tangents: the trace, and in the adjoint the VJP through each tangent
            const double kap = -a_ld / tr_div;                            // grad_outputs = -adj (odeint.py:239)
            double bs1[ADJ ? CNF_H : 1], bs2[ADJ ? CNF_H : 1];
            if constexpr (ADJ) {
#pragma unroll
                for (int i = 0; i < CNF_H; ++i) bs1[i] = bs2[i] = 0.0;
            }
            double trs = 0.0;
#pragma unroll 1
            for (int s = 0; s < ntan; ++s) {
                double v[DT], d1[CNF_H], d2[CNF_H], da[CNF_H];
                cnf_tangent<DT>(v, trace, noise, k0, k1, e, b, B, s, S, D, live);
                cnf_matvec<DT, DT, 1>(w.w1x, v, sta, d1);
#pragma unroll
                for (int i = 0; i < CNF_H; ++i) da[i] = s1[i] * d1[i];
                if constexpr (ADJ) {
                    if (wgt != 0.0) {                                     // (the pair of dL/dW2x, while da1 is at hand)
#pragma unroll
                        for (int i = 0; i < CNF_H; ++i) stb[i] = da[i];
                    }
                }
                cnf_matvec<CNF_H, CNF_H, 1>(w.w2x, da, sta, d2);
#pragma unroll
                for (int i = 0; i < CNF_H; ++i) da[i] = s2[i] * d2[i];
                double q = 0.0;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    double h = 0.0;
#pragma unroll
                    for (int j = 0; j < CNF_H; ++j) h = fma(w.w3x[d * CNF_H + j], da[j], h);
                    q = fma(v[d], h, q);
                }
                trs += q;
                if constexpr (ADJ) {
                    // trace = (1 / S) sum_s v_s . (W3x (s2 * (W2x (s1 * (W1x v_s)))))
                    double bdf[DT], bd2[CNF_H], bd1[CNF_H], r2[NR2], r1[NR1];
#pragma unroll
                    for (int i = 0; i < CNF_H; ++i) r2[i] = stb[i];           // da1 again (stb is untouched by the products above)
                    r2[CNF_H] = r2[CNF_H + 1] = 0.0;
#pragma unroll
                    for (int d = 0; d < DT; ++d) bdf[d] = kap * v[d];
#pragma unroll
                    for (int j = 0; j < CNF_H; ++j) {
                        double h = 0.0;
#pragma unroll
                        for (int d = 0; d < DT; ++d) h = fma(w.w3x[d * CNF_H + j], bdf[d], h);
                        bs2[j] = fma(h, d2[j], bs2[j]);
                        bd2[j] = h * s2[j];
                    }
                    cnf_matvec<CNF_H, 1, CNF_H>(w.w2x, bd2, sta, bd1);
#pragma unroll
                    for (int j = 0; j < CNF_H; ++j) {
                        bs1[j] = fma(bd1[j], d1[j], bs1[j]);
                        bd1[j] = bd1[j] * s1[j];
                    }
                    if (wgt != 0.0) {                                     // (uniform: stages outside dx need no parameter VJP)
                        cnf_contract<CNF_H, NR2, PER2, 5>(lbuf, rbuf, bd2, lw, r2, acc2);
#pragma unroll
                        for (int j = 0; j < CNF_H; ++j) r2[j] = da[j];
                        cnf_contract<DT, NR2, PER3, 3>(lbuf, rbuf, bdf, lw, r2, acc3);
#pragma unroll
                        for (int d = 0; d < DT; ++d) r1[d] = v[d];
                        r1[DT] = r1[DT + 1] = 0.0;
                        cnf_contract<CNF_H, NR1, PER1, 5>(lbuf, rbuf, bd1, lw, r1, acc1);
                    }
                }
            }
            const double tr = trs / tr_div;

            // ---- derivative of the state
            double dF[NS];
#pragma unroll
            for (int d = 0; d < DT; ++d) dF[ZO + d] = f[d];
            dF[LO] = tr;
            if constexpr (ADJ) {
                double cf[DT], bh2[CNF_H], bh1[CNF_H], r2[NR2], r1[NR1];
#pragma unroll
                for (int d = 0; d < DT; ++d) cf[d] = -xs[d];
#pragma unroll
                for (int j = 0; j < CNF_H; ++j) {
                    double h = 0.0;
#pragma unroll
                    for (int d = 0; d < DT; ++d) h = fma(w.w3x[d * CNF_H + j], cf[d], h);
                    bh2[j] = fma(h, s2[j], bs2[j] * (s2[j] * (1.0 - s2[j])));
                }
                cnf_matvec<CNF_H, 1, CNF_H>(w.w2x, bh2, sta, bh1);
#pragma unroll
                for (int j = 0; j < CNF_H; ++j) bh1[j] = fma(bh1[j], s1[j], bs1[j] * (s1[j] * (1.0 - s1[j])));
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    double h = 0.0;
#pragma unroll
                    for (int i = 0; i < CNF_H; ++i) h = fma(w.w1x[i * DT + d], bh1[i], h);
                    dF[d] = h;
                }
                if (wgt != 0.0) {
#pragma unroll
                    for (int j = 0; j < CNF_H; ++j) r2[j] = a2[j];
                    r2[CNF_H] = 1.0;
                    r2[CNF_H + 1] = t;
                    cnf_contract<DT, NR2, PER3, 3>(lbuf, rbuf, cf, lw, r2, acc3);
#pragma unroll
                    for (int j = 0; j < CNF_H; ++j) r2[j] = a1[j];
                    cnf_contract<CNF_H, NR2, PER2, 5>(lbuf, rbuf, bh2, lw, r2, acc2);
#pragma unroll
                    for (int d = 0; d < DT; ++d) r1[d] = zz[d];
                    r1[DT] = 1.0;
                    r1[DT + 1] = t;
                    cnf_contract<CNF_H, NR1, PER1, 5>(lbuf, rbuf, bh1, lw, r1, acc1);
                }
            }
#pragma unroll
            for (int c = 0; c < NS; ++c) ks[st][c] = dt * dF[c];
        }
        // dx (odeint.py:36, :51, :104) and the step
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            double dx = 0.0;
            for (int j = 0; j < nst; ++j) dx += ks[j][c] * tb.b[j];
            dx = dx / tb.div;
            xp[c] = x[c];
            x[c] = x[c] + dx;
        }
    }
    if (lerp) {                                                          // odeint.py:91-92
#pragma unroll
        for (int c = 0; c < NS; ++c) x[c] = xp[c] + (x[c] - xp[c]) * slope;
    }

    if (live) {
        if constexpr (ADJ) {
#pragma unroll
            for (int d = 0; d < DT; ++d)
                if (d < D) cnf_store(out_z, bl * D + d, is64, x[d]);
            cnf_store(out_ld, bl, is64, a_ld);
        } else {
#pragma unroll
            for (int d = 0; d < DT; ++d)
                if (d < D) {
                    cnf_store(out_z, bl * D + d, is64, x[d]);
                    if (state != nullptr) state[bl * (D + 1) + d] = x[d];
                }
            cnf_store(out_ld, bl, is64, x[LO]);
            if (state != nullptr) state[bl * (D + 1) + D] = x[LO];
        }
    }
    if constexpr (ADJ) {
        // the workgroup's slab, flat in parameter order: W1 (32, D+1), b1, W2 (32, 33), b2, W3 (D, 33), b3
        const int o_b1 = CNF_H * (D + 1), o_w2 = o_b1 + CNF_H, o_b2 = o_w2 + CNF_H * (CNF_H + 1), o_w3 = o_b2 + CNF_H;
        const int o_b3 = o_w3 + D * (CNF_H + 1), P = o_b3 + D;
        double* __restrict__ dst = slab + (int64_t)blockIdx.x * P;
        {
            const int i = lane & 31, g = lane >> 5;
#pragma unroll
            for (int jj = 0; jj < PER1; ++jj) {
                const int j = g * PER1 + jj;
                if (j < D) dst[i * (D + 1) + 1 + j] = acc1[jj];
                else if (j == DT) dst[o_b1 + i] = acc1[jj];
                else if (j == DT + 1) dst[i * (D + 1)] = acc1[jj];
            }
#pragma unroll
            for (int jj = 0; jj < PER2; ++jj) {
                const int j = g * PER2 + jj;
                if (j < CNF_H) dst[o_w2 + i * (CNF_H + 1) + 1 + j] = acc2[jj];
                else if (j == CNF_H) dst[o_b2 + i] = acc2[jj];
                else dst[o_w2 + i * (CNF_H + 1)] = acc2[jj];
            }
        }
        {
            const int d = lane & 7, g = lane >> 3;
            if (d < D) {
#pragma unroll
                for (int jj = 0; jj < PER3; ++jj) {
                    const int j = g * PER3 + jj;
                    if (j < CNF_H) dst[o_w3 + d * (CNF_H + 1) + 1 + j] = acc3[jj];
                    else if (j == CNF_H) dst[o_b3 + d] = acc3[jj];
                    else if (j == CNF_H + 1) dst[o_w3 + d * (CNF_H + 1)] = acc3[jj];
                }
            }
        }
    }
}

// fold: one wave per gradient element; lane l sums slabs l, l + 64, ... in order, then a fixed xor tree
__global__ void __launch_bounds__(NF_BLOCK) k_cnf_fold(const double* __restrict__ slab, int64_t n_slabs, double* __restrict__ grads, int P) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (NF_BLOCK / NF_WAVE) + (threadIdx.x >> 6);
    if (e >= P) return;
    double s = 0.0;
    for (int64_t k = lane; k < n_slabs; k += NF_WAVE) s += slab[k * P + e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, NF_WAVE);
    if (lane == 0) grads[e] = s;
}

// the in-kernel noise of a pass, written out (what cnf_tangent hands the integration for the same seed words): out[E][B][S][D]
__global__ void __launch_bounds__(NF_BLOCK) k_cnf_noise(float* __restrict__ out, const int64_t* __restrict__ seed, int64_t E, int64_t B, int S,
                                                        int D) {
    unsigned k0, k1;
    cnf_keys(seed, k0, k1);
    const int64_t total = E * B * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int s = (int)(i % S);
        const int64_t b = (i / S) % B, e = i / S / B;
        double v[NF_CNF_MAX_DIM];
        cnf_tangent<NF_CNF_MAX_DIM>(v, NF_CNF_TRACE_HUTCHINSON, nullptr, k0, k1, e, b, B, s, S, D, true);
#pragma unroll
        for (int d = 0; d < NF_CNF_MAX_DIM; ++d)
            if (d < D) out[i * D + d] = (float)v[d];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------------------------------------------------------------------
extern "C" int nf_cnf_noise(float* out, const int64_t* seed, int64_t E, int64_t B, int n_samples, int D, nf_stream_t stream) {
    if (D < 1 || D > NF_CNF_MAX_DIM || n_samples < 1 || n_samples > NF_CNF_MAX_SAMPLES || E < 0 || B < 0 || seed == nullptr) return NF_E_BADARG;
    if (E > 0 && B > 0 && (out == nullptr || E > ((int64_t)1 << 40) / B / n_samples)) return NF_E_BADARG;
    if (E == 0 || B == 0) return 0;
    hipLaunchKernelGGL(k_cnf_noise, dim3(nf_grid_for(E * B * n_samples)), dim3(NF_BLOCK), 0, (hipStream_t)stream, out, seed, E, B, n_samples, D);
    NF_CHECK_LAUNCH();
    return 0;
}

static int cnf_param_count(int D) { return CNF_H * (D + 1) + CNF_H + CNF_H * (CNF_H + 1) + CNF_H + D * (CNF_H + 1) + D; }

static bool cnf_common_ok(CnfPtrs& t, const int64_t* params, const double* sched, int n_steps, int method, int trace, int n_samples,
                          const float* noise, const int64_t* seed, int64_t B, int D) {
    if (D < 1 || D > NF_CNF_MAX_DIM || B < 0 || (B + CNF_WG - 1) / CNF_WG > 0x7fffffff) return false;
    if (!cnf_method_ok(method) || n_steps < 1 || n_steps > NF_CNF_MAX_STEPS || sched == nullptr || params == nullptr) return false;
    if (trace != NF_CNF_TRACE_HUTCHINSON && trace != NF_CNF_TRACE_EXACT) return false;
    if (trace == NF_CNF_TRACE_HUTCHINSON && (n_samples < 1 || n_samples > NF_CNF_MAX_SAMPLES || (noise == nullptr && seed == nullptr)))
        return false;
    for (int i = 0; i < 6; ++i) {
        t.p[i] = (const double*)(intptr_t)params[i];
        if (t.p[i] == nullptr) return false;
    }
    return true;
}

#define CNF_DISPATCH(D, CALL)       \
    do {                            \
        if ((D) <= 2) CALL(2);      \
        else if ((D) <= 4) CALL(4); \
        else CALL(8);               \
    } while (0)

extern "C" int nf_cnf_integrate(const void* z, const void* ld, void* z_out, void* ld_out, double* state, const int64_t* params,
                                const double* sched, int n_steps, int method, int trace, int n_samples, const float* noise,
                                const int64_t* seed, int is_f64, int64_t B, int D, nf_stream_t stream) {
    CnfPtrs t;
    if (!cnf_common_ok(t, params, sched, n_steps, method, trace, n_samples, noise, seed, B, D)) return NF_E_BADARG;
    if (B > 0 && (z == nullptr || ld == nullptr || z_out == nullptr || ld_out == nullptr)) return NF_E_BADARG;
    if (B == 0) return 0;
    const unsigned g = (unsigned)((B + CNF_WG - 1) / CNF_WG);
#define CALL(DT)                                                                                                                  \
    hipLaunchKernelGGL((k_cnf<DT, false>), dim3(g), dim3(CNF_WG), 0, (hipStream_t)stream, z, ld, z_out, ld_out, state, (double*)nullptr, \
                       t, sched, n_steps, method, trace, n_samples, noise, seed, is_f64, B, D)
    CNF_DISPATCH(D, CALL);
#undef CALL
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_cnf_slab_doubles(int64_t B, int D, int64_t* n_doubles) {
    if (D < 1 || D > NF_CNF_MAX_DIM || B < 0 || n_doubles == nullptr) return NF_E_BADARG;
    *n_doubles = ((B + CNF_WG - 1) / CNF_WG) * (int64_t)cnf_param_count(D);
    return 0;
}

extern "C" int nf_cnf_fold(const double* slab, int64_t n_slabs, double* grads, int D, nf_stream_t stream) {
    if (D < 1 || D > NF_CNF_MAX_DIM || n_slabs < 0 || grads == nullptr || (n_slabs > 0 && slab == nullptr)) return NF_E_BADARG;
    const int P = cnf_param_count(D);
    const unsigned fb = (unsigned)((P + NF_BLOCK / NF_WAVE - 1) / (NF_BLOCK / NF_WAVE));
    hipLaunchKernelGGL(k_cnf_fold, dim3(fb), dim3(NF_BLOCK), 0, (hipStream_t)stream, slab, n_slabs, grads, P);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_cnf_adjoint(const double* state, const void* g_zo, const void* g_ldo, void* g_z, void* g_ld, double* slab, double* grads,
                              const int64_t* params, const double* sched, int n_steps, int method, int trace, int n_samples,
                              const float* noise, const int64_t* seed, int is_f64, int64_t B, int D, nf_stream_t stream) {
    CnfPtrs t;
    if (!cnf_common_ok(t, params, sched, n_steps, method, trace, n_samples, noise, seed, B, D) || grads == nullptr) return NF_E_BADARG;
    if (B > 0 && (state == nullptr || g_zo == nullptr || g_ldo == nullptr || g_z == nullptr || g_ld == nullptr || slab == nullptr))
        return NF_E_BADARG;
    const int64_t g = (B + CNF_WG - 1) / CNF_WG;
    if (B > 0) {
#define CALL(DT)                                                                                                         \
    hipLaunchKernelGGL((k_cnf<DT, true>), dim3((unsigned)g), dim3(CNF_WG), 0, (hipStream_t)stream, g_zo, g_ldo, g_z, g_ld, \
                       (double*)state, slab, t, sched, n_steps, method, trace, n_samples, noise, seed, is_f64, B, D)
        CNF_DISPATCH(D, CALL);
#undef CALL
        NF_CHECK_LAUNCH();
    }
    return nf_cnf_fold(slab, g, grads, D, stream);
}
