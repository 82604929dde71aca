// The MADE masks of a MAF step drawn on the device (MADE._create_masks, flows/maf.py:66-85), so that a captured training step and the
// one-launch inverse need nothing from the host's np.random: the reference redraws the hidden degrees on every call (maf.py:50), and
// for D >= 3 the draw varies from call to call.
//   nf_made_draw_masks   n_draws independent mask sets per launch, ONE WAVE per draw; lane k (and its twin k + 32) holds unit k of
//                        the hidden layer at hand.  Three hidden layers of 32 units (what the step kernels of made_chain.hip take):
//                            m_0 = arange(D);   m_l[k] ~ uniform{lo_l .. D - 2},  lo_l = min(min_k m_{l-1}[k], D - 2)    (maf.py:72-74)
//                        lo_l is a wave minimum over the lanes that hold layer l - 1 (the reference's data-dependent bound).  D = 1 gives
//                        every degree -1 and D = 2 every degree 0 by the same formula (a range of one value), as np.random.randint does.
//                        The four fp32 masks land where the step kernels read them (O x I, row-major, per layer):
//                            layer 0 (32, D):  m_0[i] <= m_1[k]      layers 1, 2 (32, 32):  m_l[i] <= m_{l+1}[k]           (maf.py:75)
//                            layer 3 (D, 32):  r >= m_3[k] + 1                                                            (maf.py:81-84)
// Random numbers: Philox4x32-10 (nf_philox.h), key = seed[0], counter = (seed[1] + draw as 64 bits, layer << 8 | unit, a tag): a pure
// function of the seed words, the draw index, the layer and the unit -- the same words give the same masks on any grid.  A 32-bit word
// w goes to the range of R = D - 1 - lo_l <= 3 values by multiply-shift, lo_l + floor(w R / 2^32): exact for R = 1 and R = 2; for
// R = 3, 2^32 = 3 x 1431655765 + 1, so one of the three values is hit by one word more than the others (a relative bias of 7e-10).
// The stream offset seed[1] moves on by n_draws per launch in a one-thread launch BEHIND the draw (stream order): every workgroup of
// the draw reads the word before anybody writes it.  No spin loop, no grid exchange, no atomics; plain vector stores only.
#include "nf_common.h"
#include "nf_philox.h"

#define NF_MK_H 32                                        // hidden units per layer
#define NF_MK_TAG 0x4D414445u                             // counter word 3: keeps these draws apart from other users of the same seed
static_assert(NF_MADE_MASK_OFF_1 == 4 * NF_MK_H && NF_MADE_MASK_OFF_2 == NF_MADE_MASK_OFF_1 + NF_MK_H * NF_MK_H &&
              NF_MADE_MASK_OFF_3 == NF_MADE_MASK_OFF_2 + NF_MK_H * NF_MK_H && NF_MADE_MASK_STRIDE == NF_MADE_MASK_OFF_3 + 4 * NF_MK_H,
              "mask layout in include/nfhip.h (sized for D = 4)");

__device__ __forceinline__ int nf_mk_wave_min32(int v) {  // both halves of the wave hold the same 32 values
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s));
    return v;
}

__global__ void __launch_bounds__(NF_BLOCK) k_made_draw_masks(float* __restrict__ masks, int* __restrict__ degrees,
                                                              const int64_t* __restrict__ seed, int n_draws, int D) {
    const int lane = threadIdx.x & (NF_WAVE - 1), k = lane & (NF_MK_H - 1), half = lane >> 5;
    const int waves = NF_BLOCK / NF_WAVE;
    const uint64_t s = (uint64_t)seed[0], off = (uint64_t)seed[1];
    for (int d = blockIdx.x * waves + (threadIdx.x >> 6); d < n_draws; d += gridDim.x * waves) {       // wave-uniform
        const uint64_t ctr = off + (uint64_t)d;
        float* M = masks + (size_t)d * NF_MADE_MASK_STRIDE;
        int m[4];
        m[0] = k < D ? k : D - 1;                         // lanes beyond D repeat the largest input degree: the minimum stays 0
#pragma unroll
        for (int l = 1; l <= 3; ++l) {
            const int lo = min(nf_mk_wave_min32(m[l - 1]), D - 2);
            const unsigned R = (unsigned)(D - 1 - lo);    // >= 1
            const NfPhilox r = nf_philox((unsigned)ctr, (unsigned)(ctr >> 32), ((unsigned)l << 8) | (unsigned)k, NF_MK_TAG, (unsigned)s,
                                         (unsigned)(s >> 32));
            m[l] = lo + (int)__umulhi(r.c[0], R);
            if (degrees != nullptr && half == 0) degrees[((size_t)d * 3 + (l - 1)) * NF_MK_H + k] = m[l];
        }
        // layer 0 (32, D): element e = o * D + i
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = lane + NF_WAVE * j, o = e / D, i = e - o * D;
            const int mo = __shfl(m[1], o & (NF_MK_H - 1));
            if (e < NF_MK_H * D) M[NF_MADE_MASK_OFF_0 + e] = i <= mo ? 1.f : 0.f;
        }
        // layers 1, 2 (32, 32): rows o = half + 2 j, column i = k (this lane's own unit of the layer below)
#pragma unroll
        for (int l = 1; l <= 2; ++l)
#pragma unroll 4
            for (int j = 0; j < NF_MK_H / 2; ++j) {
                const int o = half + 2 * j;
                const int mo = __shfl(m[l + 1], o);
                M[(l == 1 ? NF_MADE_MASK_OFF_1 : NF_MADE_MASK_OFF_2) + o * NF_MK_H + k] = m[l] <= mo ? 1.f : 0.f;
            }
        // layer 3 (D, 32): rows r = half + 2 j
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = half + 2 * j;
            if (r < D) M[NF_MADE_MASK_OFF_3 + r * NF_MK_H + k] = r >= m[3] + 1 ? 1.f : 0.f;
        }
    }
}

__global__ void k_made_advance(int64_t* seed, int n) { seed[1] += (int64_t)n; }

extern "C" int nf_made_draw_masks(float* masks, int* degrees, int64_t* seed, int n_draws, int D, int advance, nf_stream_t stream) {
    if (masks == nullptr || seed == nullptr || n_draws < 0 || D < 1 || D > 4) return NF_E_BADARG;
    if (n_draws == 0) return 0;
    hipLaunchKernelGGL(k_made_draw_masks, dim3(nf_grid_for(n_draws, NF_BLOCK / NF_WAVE)), dim3(NF_BLOCK), 0, (hipStream_t)stream, masks,
                       degrees, (const int64_t*)seed, n_draws, D);
    NF_CHECK_LAUNCH();
    if (advance) {
        hipLaunchKernelGGL(k_made_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, seed, n_draws);
        NF_CHECK_LAUNCH();
    }
    return 0;
}
