// The batch contraction of the CNF adjoint (csrc/cnf.hip, cnf_contract at the 32 x 32 weight of the middle layer): G[i][j] += sum over the
// 64 rows of a wave of L_r[i] * R_r[j], from LDS.  Two forms, same data, same LDS layout, one wave per workgroup:
//   valu   lane (i = lane & 31, h = lane >> 5) owns G[i][16 h .. 16 h + 15]: 64 x (1 + 16) ds_read_b64, 64 x 16 v_fma_f64
//   mfma   v_mfma_f64_16x16x4_f64: 2 x 2 tiles x 16 k-steps = 64 MFMAs, 16 x 4 ds_read_b64; A[i][k] = lane (i = l & 15, k = l >> 4),
//          B[k][j] = lane (k = l >> 4, j = l & 15), D: col = l & 15, row = (l >> 4) + 4 reg
// Prints the time per contraction (write + barrier + contract + barrier, as the kernel does it) and the largest difference of the results.
//   hipcc --offload-arch=gfx950 -O3 -o tools/probes/_bin/cnf_contract_probe tools/probes/cnf_contract_probe.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

#define LS 33
#define RS 35
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <bool MFMA>
__global__ void __launch_bounds__(64) k_contract(double* __restrict__ out, int n) {
    __shared__ double lb[64 * LS], rb[64 * RS];
    const int lane = threadIdx.x;
    double L[32], R[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        L[i] = 1.0e-3 * ((lane * 37 + i * 11 + blockIdx.x) % 101) - 0.05;
        R[i] = 1.0e-3 * ((lane * 13 + i * 29) % 103) - 0.05;
    }
    double acc[16];
    f64x4 t[4];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) t[a] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < n; ++it) {
        const double sc = 1.0 + 1.0e-3 * it;
#pragma unroll
        for (int i = 0; i < 32; ++i) lb[lane * LS + i] = L[i] * sc;
#pragma unroll
        for (int j = 0; j < 32; ++j) rb[lane * RS + j] = R[j];
        __syncthreads();
        if (MFMA) {
            const int m = lane & 15, k = lane >> 4;
#pragma unroll 4
            for (int ks = 0; ks < 16; ++ks) {
                const double a0 = lb[(4 * ks + k) * LS + m], a1 = lb[(4 * ks + k) * LS + 16 + m];
                const double b0 = rb[(4 * ks + k) * RS + m], b1 = rb[(4 * ks + k) * RS + 16 + m];
                t[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, t[0], 0, 0, 0);
                t[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, t[1], 0, 0, 0);
                t[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, t[2], 0, 0, 0);
                t[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, t[3], 0, 0, 0);
            }
        } else {
            const int i = lane & 31, h = lane >> 5;
#pragma unroll 2
            for (int r = 0; r < 64; ++r) {
                const double l = lb[r * LS + i];
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[j] = fma(l, rb[r * RS + 16 * h + j], acc[j]);
            }
        }
        __syncthreads();
    }
    double* g = out + (size_t)blockIdx.x * 1024;
    if (MFMA) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) g[((a >> 1) * 16 + (lane >> 4) + 4 * r) * 32 + (a & 1) * 16 + (lane & 15)] = t[a][r];
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) g[(lane & 31) * 32 + 16 * (lane >> 5) + j] = acc[j];
    }
}

template <bool MFMA>
static double run(int blocks, int n, double* out) {
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    hipLaunchKernelGGL(k_contract<MFMA>, dim3(blocks), dim3(64), 0, 0, out, n);
    hipDeviceSynchronize();
    hipEventRecord(a, 0);
    hipLaunchKernelGGL(k_contract<MFMA>, dim3(blocks), dim3(64), 0, 0, out, n);
    hipEventRecord(b, 0);
    hipDeviceSynchronize();
    float ms = 0.f;
    hipEventElapsedTime(&ms, a, b);
    return ms * 1e6 / n;                                 // ns per contraction of a wave
}

int main() {
    const int max_blocks = 4096, n = 2000;
    double *o0, *o1;
    hipMalloc(&o0, (size_t)max_blocks * 1024 * sizeof(double));
    hipMalloc(&o1, (size_t)max_blocks * 1024 * sizeof(double));
    for (int blocks : {16, 256, 1024, 4096}) {
        const double tv = run<false>(blocks, n, o0), tm = run<true>(blocks, n, o1);
        std::vector<double> h0((size_t)blocks * 1024), h1((size_t)blocks * 1024);
        hipMemcpy(h0.data(), o0, h0.size() * sizeof(double), hipMemcpyDeviceToHost);
        hipMemcpy(h1.data(), o1, h1.size() * sizeof(double), hipMemcpyDeviceToHost);
        double err = 0.0, mx = 0.0;
        for (size_t i = 0; i < h0.size(); ++i) {
            err = std::fmax(err, std::fabs(h0[i] - h1[i]));
            mx = std::fmax(mx, std::fabs(h0[i]));
        }
        printf("waves %5d: valu %8.1f ns  mfma %8.1f ns per 32x32x64 contraction (x%.2f)   max |valu - mfma| %.3e of %.3e\n", blocks, tv, tm,
               tv / tm, err, mx);
    }
    return 0;
}
