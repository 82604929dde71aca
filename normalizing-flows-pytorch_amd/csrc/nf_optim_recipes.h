// One element of every fused optimizer step -- Adam, RMSprop, Adamax, AdamW -- stated once, for the one kernel body of csrc/optim.hip
// (k_optim_step) to run plain, guarded and guarded with the average.  Each follows torch.optim as torch 2.10 writes it (optim/adam.py,
// rmsprop.py, adamax.py, adam.py with decoupled_weight_decay), the step constants formed once per thread from the device-resident step
// count and rate.  A recipe is a struct with
//   STATES, USES_STEP      how many state buffers it streams (2: m and s; 1: s alone, m is never touched) and whether it reads step[0]
//   Consts, consts(...)    what a thread forms once before its loop
//   one(p, g, m, s, ...)   the update of one element in registers
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include "nf_common.h"

// The hyper-parameters as the kernel takes them; a recipe reads the fields it names and no other.  omb1 / omb2 are 1 - beta1 / 1 - beta2
// AS TORCH FORMS THEM: in double from the number the caller wrote, rounded to float once.  The betas cross the C ABI as floats, and
// 1 - 0.999f is 1.3e-5 (relative) away from float(1 - 0.999) -- six times the optimizer bar on exp_avg_sq wherever (1 - beta2) g^2
// dominates it.  The 7-digit decimal that names the float (0.999 for 0.999000013f) is the caller's number whenever it reads back as the
// same float; a beta with more digits than a float holds is used as it arrived.  Adamax and AdamW use them; Adam and RMSprop, the two
// the reference trains with, keep the (1.f - beta) and (1.f - alpha) they have always formed in float on the device.
struct NfOptimHyper { float b1, b2, omb1, omb2, alpha, eps, wd; };

static inline float nf_one_minus(float beta) {
    char buf[32];
    snprintf(buf, sizeof buf, "%.7g", (double)beta);
    const double d = strtod(buf, nullptr);
    return (float)(1.0 - ((float)d == beta ? d : (double)beta));
}

static inline NfOptimHyper nf_adam_hyper(float beta1, float beta2, float eps, float weight_decay) {      // the Adam family
    NfOptimHyper h = {};
    h.b1 = beta1; h.b2 = beta2; h.eps = eps; h.wd = weight_decay;
    h.omb1 = nf_one_minus(beta1);
    h.omb2 = nf_one_minus(beta2);
    return h;
}

static inline NfOptimHyper nf_rmsprop_hyper(float alpha, float eps, float weight_decay) {
    NfOptimHyper h = {};
    h.alpha = alpha; h.eps = eps; h.wd = weight_decay;
    return h;
}

// ---- Adam:    g += wd p ; m = b1 m + (1 - b1) g ; v = b2 v + (1 - b2) g^2 ; p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
struct NfAdam {
    static constexpr int STATES = 2;
    static constexpr bool USES_STEP = true;
    struct Consts { NfOptimHyper h; float bc2_sqrt, step_size; };

    static __device__ __forceinline__ Consts consts(const int* step, const float* lr, const NfOptimHyper& h) {
        const float t = (float)step[0];
        Consts c;
        c.h = h;
        c.bc2_sqrt = sqrtf(1.f - powf(h.b2, t));
        c.step_size = lr[0] / (1.f - powf(h.b1, t));
        return c;
    }

    static __device__ __forceinline__ void one(float& p, float g, float& m, float& v, const Consts& c, float grad_scale) {
        float gi = g * grad_scale;
        if (c.h.wd != 0.f) gi = fmaf(c.h.wd, p, gi);
        m = fmaf(c.h.b1, m, (1.f - c.h.b1) * gi);
        v = fmaf(c.h.b2, v, (1.f - c.h.b2) * gi * gi);
        p = p - c.step_size * (m / (sqrtf(v) / c.bc2_sqrt + c.h.eps));
    }
};

// ---- RMSprop (momentum 0, not centred):  g += wd p ; v = alpha v + (1 - alpha) g^2 ; p -= lr g / (sqrt(v) + eps) ------------------
struct NfRmsprop {
    static constexpr int STATES = 1;
    static constexpr bool USES_STEP = false;
    struct Consts { NfOptimHyper h; float lr; };

    static __device__ __forceinline__ Consts consts(const int*, const float* lr, const NfOptimHyper& h) {
        Consts c;
        c.h = h;
        c.lr = lr[0];
        return c;
    }

    static __device__ __forceinline__ void one(float& p, float g, float&, float& v, const Consts& c, float grad_scale) {
        float gi = g * grad_scale;
        if (c.h.wd != 0.f) gi = fmaf(c.h.wd, p, gi);
        v = fmaf(c.h.alpha, v, (1.f - c.h.alpha) * gi * gi);
        p = p - c.lr * (gi / (sqrtf(v) + c.h.eps));
    }
};

// ---- Adamax:  g += wd p ; m = m + (1 - b1)(g - m) ; u = max(b2 u, |g| + eps) ; p -= (lr / (1 - b1^t)) m / u ----------------
struct NfAdamax {
    static constexpr int STATES = 2;
    static constexpr bool USES_STEP = true;
    struct Consts { NfOptimHyper h; float clr; };

    static __device__ __forceinline__ Consts consts(const int* step, const float* lr, const NfOptimHyper& h) {
        Consts c;
        c.h = h;
        c.clr = lr[0] / (1.f - powf(h.b1, (float)step[0]));
        return c;
    }

    static __device__ __forceinline__ void one(float& p, float g, float& m, float& u, const Consts& c, float grad_scale) {
        float gi = g * grad_scale;
        if (c.h.wd != 0.f) gi = fmaf(c.h.wd, p, gi);
        m = fmaf(c.h.omb1, gi - m, m);                        // Tensor.lerp_(g, 1 - b1)
        const float a = c.h.b2 * u, b = fabsf(gi) + c.h.eps;  // b >= eps > 0: a zero gradient on a zero exp_inf divides by eps, not by 0
        u = (a != a || a >= b) ? a : b;                       // torch.maximum: a NaN on either side stays
        p = p - c.clr * (m / u);
    }
};

// ---- AdamW:   p *= 1 - lr wd ; then Adam's moments and update without the L2 term, on torch's 1 - beta (omb1, omb2) -----------------
struct NfAdamW {
    static constexpr int STATES = 2;
    static constexpr bool USES_STEP = true;
    struct Consts { NfOptimHyper h; float shrink, bc2_sqrt, step_size; };

    static __device__ __forceinline__ Consts consts(const int* step, const float* lr, const NfOptimHyper& h) {
        const float t = (float)step[0];
        Consts c;
        c.h = h;
        c.shrink = 1.f - lr[0] * h.wd;
        c.bc2_sqrt = sqrtf(1.f - powf(h.b2, t));
        c.step_size = lr[0] / (1.f - powf(h.b1, t));
        return c;
    }

    static __device__ __forceinline__ void one(float& p, float g, float& m, float& v, const Consts& c, float grad_scale) {
        const float gi = g * grad_scale;
        const float pi = p * c.shrink;
        m = fmaf(c.h.b1, m, c.h.omb1 * gi);
        v = fmaf(c.h.b2, v, c.h.omb2 * gi * gi);
        p = pi - c.step_size * (m / (sqrtf(v) / c.bc2_sqrt + c.h.eps));
    }
};
