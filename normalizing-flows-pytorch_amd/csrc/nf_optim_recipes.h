// One element of the Adamax and AdamW steps, stated once for the plain kernels (csrc/optim.hip) and the guarded ones
// (csrc/optim_guard.hip).  Both follow torch.optim as torch 2.10 writes it (optim/adamax.py, optim/adam.py with
// decoupled_weight_decay), the step constants formed once per thread from the device-resident step count and rate.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include "nf_common.h"

// The hyper-parameters as the kernels take them.  omb1 / omb2 are 1 - beta1 / 1 - beta2 AS TORCH FORMS THEM: in double from the
// number the caller wrote, rounded to float once.  The betas cross the C ABI as floats, and 1 - 0.999f is 1.3e-5 (relative) away
// from float(1 - 0.999) -- six times the optimizer bar on exp_avg_sq wherever (1 - beta2) g^2 dominates it.  The 7-digit decimal
// that names the float (0.999 for 0.999000013f) is the caller's number whenever it reads back as the same float; a beta with
// more digits than a float holds is used as it arrived.
struct NfRecipeHyper { float b1, b2, omb1, omb2, eps, wd; };

static inline float nf_one_minus(float beta) {
    char buf[32];
    snprintf(buf, sizeof buf, "%.7g", (double)beta);
    const double d = strtod(buf, nullptr);
    return (float)(1.0 - ((float)d == beta ? d : (double)beta));
}

static inline NfRecipeHyper nf_recipe_hyper(float beta1, float beta2, float eps, float weight_decay) {
    NfRecipeHyper h;
    h.b1 = beta1; h.b2 = beta2; h.eps = eps; h.wd = weight_decay;
    h.omb1 = nf_one_minus(beta1);
    h.omb2 = nf_one_minus(beta2);
    return h;
}

// ---- Adamax:  g += wd p ; m = m + (1 - b1)(g - m) ; u = max(b2 u, |g| + eps) ; p -= (lr / (1 - b1^t)) m / u ----------------
// ---- AdamW:   p *= 1 - lr wd ; then Adam's moments and update without the L2 term (k_adam_step's arithmetic) ----------------
// The two as template arguments of ONE kernel body per file (k_recipe_step, k_recipe_step_guarded): same buffers (parameter, gradient,
// first moment, second buffer), same 28 B per element, only the element's arithmetic differs.
struct NfAdamax {
    struct Consts { NfRecipeHyper h; float clr; };

    static __device__ __forceinline__ Consts consts(const int* step, const float* lr, const NfRecipeHyper& h) {
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

struct NfAdamW {
    struct Consts { NfRecipeHyper h; float shrink, bc2_sqrt, step_size; };

    static __device__ __forceinline__ Consts consts(const int* step, const float* lr, const NfRecipeHyper& h) {
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
