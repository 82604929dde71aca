// Device-resident data sets: the reference's loader (flows/dataset.py:53-127) keeps its set on the host, shuffles an index array once per
// pass (:104-106) and builds every batch there -- idx = indices[iter : iter + B] (:116), uint8 / 255 (:120), HWC -> CHW (:121-122),
// MNIST's 2-pixel pad (:71) -- before main.py:79 copies it to the device.  Here the set is uploaded once and a batch is GATHERED where it
// is consumed, by a kernel that reads its step from device memory (as k_sample_data does), so a captured hipGraph walks through the
// batches and the epochs on its own once nf_sample_advance follows it.
//
// The pass's order is not an index array but a counter-based bijection of [0, N) evaluated per sample:
//   perm(seed, epoch, pos): a balanced Feistel network over 2h bits, h = max(1, ceil(bits(N - 1) / 2)), NF_DS_ROUNDS = 8 rounds
//     (L, R) -> (R, L ^ F(R, round)),  F = word 0 of Philox4x32-10(counter = (R, round, epoch lo, epoch hi), key = (seed lo,
//     seed hi ^ NF_DS_KEY)) masked to h bits;  the result is walked (perm applied again) while it is >= N.
//   The domain 2^(2h) is < 4 N, so a walk goes on with probability <= 3/4 per application: after NF_DS_WALK = 155 further applications
//   (3/4)^155 < 2^-64 and the kernel gives up with the position itself (in range, so no read can leave the set).  Integer arithmetic
//   only: data.dataset_perm restates it in numpy bit for bit.
// Schedule (dataset.py:111-117): a pass serves batches while N > iter + B, i.e. E = (N - 1) / stride steps of stride = W * B positions;
// step s -> epoch = s / E, k = s % E; a rank takes positions k * stride + offset + j, j < B, offset = rank * B.
// Sweep schedule (what main.py:121-127 scores, over a whole set): a pass is E = S = ceil(N / stride) steps and counts every sample once;
// a position >= N is served sample N - 1 (clamped: no read leaves the set) and is invalid -- nf_logp_accumulate (logp.hip) leaves it out.
//
// Dequantised images (the DQ arm of k_dataset_gather_u8): byte v at byte offset b of HWC sample idx becomes
//   q = v * 2^15 + (w >> 17)  (23 bits),  x = ((float)q + 0.5f) * 2^-23   -- nf_u01's construction: q + 0.5 needs 24 bits, nothing rounds --
//   w = word b & 3 of Philox4x32-10(counter = (b >> 2, idx, step lo, step hi), key = (seed lo, seed hi ^ NF_DQ_KEY)),
// so x lies in (0, 1), floor(256 x) == v, the noise is a pure function of (seed, step, sample, byte) and a graph replay draws it afresh;
// data.dequant_words / DeviceDataset.host_batch restate it in numpy bit for bit.
#include "nf_common.h"
#include "nf_philox.h"

#define NF_DS_ROUNDS 8
#define NF_DS_WALK 155
#define NF_DS_KEY 0x510e527fu
#define NF_DQ_KEY 0x9b05688cu   // sets the dequantisation noise's Philox stream apart from the permutation's
#define NF_DS_STAGE_MAX 32768   // bytes of one staged slice (LDS): the host picks the rows per slice under it

struct NfDsSched {
    int64_t N, B, stride, offset, E;
    unsigned seed_lo, seed_hi;
    int shuffle, half_bits, sweep;
};

__device__ __forceinline__ unsigned nf_ds_feistel(unsigned x, int h, unsigned e_lo, unsigned e_hi, unsigned k0, unsigned k1) {
    const unsigned mask = (1u << h) - 1u;
    unsigned L = x >> h, R = x & mask;
#pragma unroll 1
    for (unsigned r = 0; r < NF_DS_ROUNDS; ++r) {
        const unsigned f = nf_philox(R, r, e_lo, e_hi, k0, k1).c[0] & mask;
        const unsigned t = L ^ f;
        L = R;
        R = t;
    }
    return (L << h) | R;
}
// index of sample j of this rank's batch at the step in device memory
__device__ __forceinline__ int64_t nf_ds_index(const NfDsSched& s, const int64_t* __restrict__ step_ptr, int64_t j) {
    const unsigned long long step = step_ptr != nullptr ? (unsigned long long)step_ptr[0] : 0ull;
    const unsigned long long epoch = step / (unsigned long long)s.E, k = step - epoch * (unsigned long long)s.E;
    const int64_t pos = (int64_t)k * s.stride + s.offset + j;                        // < E * stride <= N - 1 (loader schedule)
    if (s.sweep && pos >= s.N) return s.N - 1;                                        // the sweep's tail: clamped, counted by nobody
    if (!s.shuffle) return pos;
    const unsigned e_lo = (unsigned)epoch, e_hi = (unsigned)(epoch >> 32), k1 = s.seed_hi ^ NF_DS_KEY;
    unsigned x = nf_ds_feistel((unsigned)pos, s.half_bits, e_lo, e_hi, s.seed_lo, k1);
#pragma unroll 1
    for (int w = 0; w < NF_DS_WALK && (int64_t)x >= s.N; ++w) x = nf_ds_feistel(x, s.half_bits, e_lo, e_hi, s.seed_lo, k1);
    return (int64_t)x < s.N ? (int64_t)x : pos;
}

// ---- images: data uint8 (N, H, W, C) -> out float32 (B, C, H + 2 pad, W + 2 pad) ---------------------------------------------------
// grid = B * n_slices (4, 2 or 1 slices by B): workgroup (j, sl) owns output rows [sl * rows, (sl + 1) * rows) of every channel of
// sample j.  Thread 0 computes the sample's index and shares it through LDS; the slice's input rows (contiguous bytes of the HWC sample) are staged in LDS -- with
// 16-byte loads over the enclosing aligned range where the sample size is a multiple of 16, byte loads otherwise -- and the CHW turn
// happens on the LDS read: consecutive lanes read bytes C apart (C = 3: 32 lanes span 24 dwords, no two on one bank) and write
// consecutive floats of one output row.  The pad ring is written with zeros by the same loop; every output element has one writer.
// DQ = 1: between the two phases the slice's noise is drawn ONCE per aligned quad of bytes -- one Philox call serves four bytes -- into
// 16-bit LDS slots behind the stage (at the 16-byte boundary after rows * row_bytes + 32); the write loop then reads byte and noise.
template <int DQ>
__global__ void __launch_bounds__(NF_BLOCK) k_dataset_gather_u8(const uint8_t* __restrict__ data, float* __restrict__ out, int H, int W,
                                                                int C, int pad, NfDsSched s, const int64_t* __restrict__ step_ptr,
                                                                int64_t* __restrict__ idx_out, int rows, int n_slices, int vec) {
    extern __shared__ __align__(16) uint8_t stage[];
    __shared__ int64_t s_idx;
    const int64_t j = blockIdx.x / n_slices;
    const int sl = blockIdx.x - (int)j * n_slices;
    if (threadIdx.x == 0) {
        const int64_t idx = nf_ds_index(s, step_ptr, j);
        s_idx = idx;
        if (sl == 0 && idx_out != nullptr) idx_out[j] = idx;
    }
    __syncthreads();
    const int Ho = H + 2 * pad, Wo = W + 2 * pad, row_bytes = W * C;
    const int yo0 = sl * rows, yo1 = min(yo0 + rows, Ho);
    const int yi0 = min(max(yo0 - pad, 0), H), yi1 = min(max(yo1 - pad, 0), H);       // input rows under this slice (may be none)
    const int b0 = yi0 * row_bytes, b1 = yi1 * row_bytes;
    const uint8_t* __restrict__ src = data + (size_t)s_idx * ((size_t)H * row_bytes);
    int shift = 0;                                                                    // stage[shift + b - b0] = byte b of the sample
    if (b1 > b0) {
        if (vec) {
            const int a0 = b0 & ~15, a1 = (b1 + 15) & ~15;                            // a1 <= H * row_bytes: a multiple of 16
            shift = b0 - a0;
            const uint4* __restrict__ src4 = reinterpret_cast<const uint4*>(src + a0);
            uint4* stage4 = reinterpret_cast<uint4*>(stage);
            for (int t = threadIdx.x; t < (a1 - a0) >> 4; t += NF_BLOCK) stage4[t] = src4[t];
        } else {
            for (int t = threadIdx.x; t < b1 - b0; t += NF_BLOCK) stage[t] = src[b0 + t];
        }
    }
    const int q0 = b0 >> 2;                                                           // first quad of bytes under this slice
    const uint16_t* noise = nullptr;
    if (DQ) {
        uint16_t* nz = reinterpret_cast<uint16_t*>(stage + ((rows * row_bytes + 32 + 15) & ~15));
        noise = nz;
        const unsigned long long step = step_ptr != nullptr ? (unsigned long long)step_ptr[0] : 0ull;
        const unsigned idx_w = (unsigned)s_idx, k1 = s.seed_hi ^ NF_DQ_KEY;
        const int n_quads = b1 > b0 ? ((b1 + 3) >> 2) - q0 : 0;                       // <= (rows * row_bytes + 6) / 4; none under a pad-only slice
        for (int t = threadIdx.x; t < n_quads; t += NF_BLOCK) {
            const NfPhilox p = nf_philox((unsigned)(q0 + t), idx_w, (unsigned)step, (unsigned)(step >> 32), s.seed_lo, k1);
            uint2 pk;
            pk.x = (p.c[0] >> 17) | ((p.c[1] >> 17) << 16);
            pk.y = (p.c[2] >> 17) | ((p.c[3] >> 17) << 16);
            reinterpret_cast<uint2*>(nz)[t] = pk;
        }
    }
    __syncthreads();
    const int n_rows = yo1 - yo0, per_c = n_rows * Wo;
    float* __restrict__ dst = out + (size_t)j * ((size_t)C * Ho * Wo);
    for (int e = threadIdx.x; e < C * per_c; e += NF_BLOCK) {
        const int c = e / per_c, r = e - c * per_c;
        const int yl = r / Wo, xo = r - yl * Wo;
        const int yi = yo0 + yl - pad, xi = xo - pad;
        float v = 0.f;
        if (yi >= 0 && yi < H && xi >= 0 && xi < W) {
            const int rel = (yi - yi0) * row_bytes + xi * C + c;                      // byte b0 + rel of the sample
            if (DQ) {
                const unsigned q = ((unsigned)stage[shift + rel] << 15) | (unsigned)noise[b0 + rel - 4 * q0];
                v = ((float)q + 0.5f) * (1.f / 8388608.f);
            } else {
                v = (float)stage[shift + rel] / 255.0f;
            }
        }
        dst[((size_t)c * Ho + yo0 + yl) * Wo + xo] = v;
    }
}

// ---- rows: data float32 (N, D) -> out (B, D) ------------------------------------------------------------------------------------------
// D <= 4: one row per thread (its own index, D loads, D stores)
__global__ void __launch_bounds__(NF_BLOCK) k_dataset_gather_row(const float* __restrict__ data, float* __restrict__ out, int D, NfDsSched s,
                                                                 const int64_t* __restrict__ step_ptr, int64_t* __restrict__ idx_out) {
    const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < s.B; j += gstride) {
        const int64_t idx = nf_ds_index(s, step_ptr, j);
        if (idx_out != nullptr) idx_out[j] = idx;
        for (int d = 0; d < D; ++d) out[j * D + d] = data[idx * D + d];
    }
}
// larger D: one wave per row, lane 0 computes the index, the lanes stride over the row
__global__ void __launch_bounds__(NF_BLOCK) k_dataset_gather_wide(const float* __restrict__ data, float* __restrict__ out, int64_t D,
                                                                  NfDsSched s, const int64_t* __restrict__ step_ptr,
                                                                  int64_t* __restrict__ idx_out) {
    const int lane = threadIdx.x & (NF_WAVE - 1), waves = NF_BLOCK / NF_WAVE;
    for (int64_t j = (int64_t)blockIdx.x * waves + (threadIdx.x >> 6); j < s.B; j += (int64_t)gridDim.x * waves) {
        long long idx = 0;
        if (lane == 0) {
            idx = nf_ds_index(s, step_ptr, j);
            if (idx_out != nullptr) idx_out[j] = idx;
        }
        idx = __shfl(idx, 0, NF_WAVE);
        for (int64_t d = lane; d < D; d += NF_WAVE) out[j * D + d] = data[idx * D + d];
    }
}

static bool nf_ds_sched(NfDsSched& s, int64_t N, int64_t B, int64_t stride, int64_t offset, int64_t E, int64_t seed, int shuffle,
                        int sweep) {
    if (N <= 0 || N >= ((int64_t)1 << 31) || B <= 0 || E < 1 || offset < 0 || stride <= 0 || offset + B > stride) return false;
    if (sweep != 0 && sweep != 1) return false;
    if (sweep) {                                          // a pass of ceil(N / stride) steps: positions < N + stride, the tail clamped
        if (stride >= ((int64_t)1 << 31) || E > (N + stride - 1) / stride) return false;
    } else if (E > (N - 1) / stride) {
        return false;                                     // every position of a pass lies in the set: E * stride <= N - 1
    }
    s.sweep = sweep;
    s.N = N; s.B = B; s.stride = stride; s.offset = offset; s.E = E;
    s.seed_lo = (unsigned)seed;
    s.seed_hi = (unsigned)((unsigned long long)seed >> 32);
    s.shuffle = shuffle ? 1 : 0;
    int bits = 0;
    while (((int64_t)1 << bits) < N) ++bits;              // bits(N - 1)
    s.half_bits = bits < 2 ? 1 : (bits + 1) / 2;
    return true;
}

static int nf_ds_gather_u8(const uint8_t* data, float* out, int64_t N, int H, int W, int C, int pad, int64_t B, int64_t stride,
                           int64_t offset, int64_t E, int64_t seed, int shuffle, int dequant, int sweep, const int64_t* step,
                           int64_t* idx_out, nf_stream_t stream) {
    NfDsSched s;
    if (data == nullptr || out == nullptr || H < 1 || W < 1 || C < 1 || pad < 0 || (dequant != 0 && dequant != 1)) return NF_E_BADARG;
    if (!nf_ds_sched(s, N, B, stride, offset, E, seed, shuffle, sweep)) return NF_E_BADARG;
    const int64_t row_bytes = (int64_t)W * C, Ho = (int64_t)H + 2 * pad, Wo = (int64_t)W + 2 * pad;
    // the dequantising arm keeps two noise bytes per staged byte behind the stage: a third of the rows fit
    const int64_t per_row = dequant ? 3 * row_bytes : row_bytes, room = NF_DS_STAGE_MAX - (dequant ? 64 : 32);
    if (per_row > room || (int64_t)C * Ho * Wo >= ((int64_t)1 << 31) || (int64_t)H * row_bytes >= ((int64_t)1 << 31))
        return NF_E_BADARG;                               // one input row must fit the stage; per-sample offsets are int32
    // four slices per sample below 512 samples (B = 64 -> 256 workgroups), two below 1024, one above -- every workgroup pays the serial
    // latency of its sample's index, and a large batch fills the device without slicing --, more where the rows would not fit the stage
    const int64_t want = B < 512 ? 4 : (B < 1024 ? 2 : 1);
    int64_t rows = (Ho + want - 1) / want;
    const int64_t fit = room / per_row;
    if (rows > fit) rows = fit;
    const int64_t n_slices = (Ho + rows - 1) / rows;
    if (B * n_slices >= ((int64_t)1 << 31)) return NF_E_BADARG;
    const int vec = ((H * row_bytes) % 16 == 0 && ((uintptr_t)data & 15) == 0) ? 1 : 0;
    const size_t stage_bytes = (size_t)(rows * row_bytes + 32);
    if (dequant) {
        // noise slots: 16 bits per byte of the quads that enclose the slice's bytes (<= rows * row_bytes + 6 bytes), 8-byte stores
        const size_t lds = ((stage_bytes + 15) & ~(size_t)15) + 2 * (size_t)(rows * row_bytes + 8);
        hipLaunchKernelGGL(k_dataset_gather_u8<1>, dim3((unsigned)(B * n_slices)), dim3(NF_BLOCK), lds, (hipStream_t)stream, data, out, H, W,
                           C, pad, s, step, idx_out, (int)rows, (int)n_slices, vec);
    } else {
        hipLaunchKernelGGL(k_dataset_gather_u8<0>, dim3((unsigned)(B * n_slices)), dim3(NF_BLOCK), stage_bytes, (hipStream_t)stream, data, out,
                           H, W, C, pad, s, step, idx_out, (int)rows, (int)n_slices, vec);
    }
    NF_CHECK_LAUNCH();
    return 0;
}

static int nf_ds_gather_f32(const float* data, float* out, int64_t N, int64_t D, int64_t B, int64_t stride, int64_t offset, int64_t E,
                            int64_t seed, int shuffle, int sweep, const int64_t* step, int64_t* idx_out, nf_stream_t stream) {
    NfDsSched s;
    if (data == nullptr || out == nullptr || D < 1) return NF_E_BADARG;
    if (!nf_ds_sched(s, N, B, stride, offset, E, seed, shuffle, sweep)) return NF_E_BADARG;
    if (D <= 4)
        hipLaunchKernelGGL(k_dataset_gather_row, dim3(nf_grid_for(B)), dim3(NF_BLOCK), 0, (hipStream_t)stream, data, out, (int)D, s, step,
                           idx_out);
    else
        hipLaunchKernelGGL(k_dataset_gather_wide, dim3(nf_grid_for(B, NF_BLOCK / NF_WAVE)), dim3(NF_BLOCK), 0, (hipStream_t)stream, data, out,
                           D, s, step, idx_out);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_dataset_gather_u8(const uint8_t* data, float* out, int64_t N, int H, int W, int C, int pad, int64_t B, int64_t stride,
                                    int64_t offset, int64_t E, int64_t seed, int shuffle, const int64_t* step, int64_t* idx_out,
                                    nf_stream_t stream) {
    return nf_ds_gather_u8(data, out, N, H, W, C, pad, B, stride, offset, E, seed, shuffle, 0, 0, step, idx_out, stream);
}
extern "C" int nf_dataset_gather_u8_x(const uint8_t* data, float* out, int64_t N, int H, int W, int C, int pad, int64_t B, int64_t stride,
                                      int64_t offset, int64_t E, int64_t seed, int shuffle, int dequant, int sweep, const int64_t* step,
                                      int64_t* idx_out, nf_stream_t stream) {
    return nf_ds_gather_u8(data, out, N, H, W, C, pad, B, stride, offset, E, seed, shuffle, dequant, sweep, step, idx_out, stream);
}

extern "C" int nf_dataset_gather_f32(const float* data, float* out, int64_t N, int64_t D, int64_t B, int64_t stride, int64_t offset,
                                     int64_t E, int64_t seed, int shuffle, const int64_t* step, int64_t* idx_out, nf_stream_t stream) {
    return nf_ds_gather_f32(data, out, N, D, B, stride, offset, E, seed, shuffle, 0, step, idx_out, stream);
}
extern "C" int nf_dataset_gather_f32_x(const float* data, float* out, int64_t N, int64_t D, int64_t B, int64_t stride, int64_t offset,
                                       int64_t E, int64_t seed, int shuffle, int sweep, const int64_t* step, int64_t* idx_out,
                                       nf_stream_t stream) {
    return nf_ds_gather_f32(data, out, N, D, B, stride, offset, E, seed, shuffle, sweep, step, idx_out, stream);
}
