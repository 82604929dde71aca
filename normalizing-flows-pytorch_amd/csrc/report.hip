// What Model.report computes on its way to matplotlib (main.py:135-284, common/utils.py:12-83), on the device: the density-map grid, the
// finite range of a colour vector, value -> colour through matplotlib's 256-entry tables, scatter panels and torchvision's image grid, all
// as uint8 RGB.  None of it is matrix work: the roofs are HBM and launch latency.
//   k_report_grid       one thread per grid point                                                       main.py:199-206
//   k_minmax_*          three launches: sentinels, block min / max -> two integer atomics per workgroup on an order-preserving image
//                       of the double, decode.  min and max do not depend on the order they are taken in: same bits every run
//   k_report_colorize   p = v or (float)exp((double)v); index from the STORED float32 p, in double         common/utils.py:19, :59
//   k_report_clear / k_report_splat / k_report_resolve
//                       a scatter panel: one thread per point, atomicMax of (depth_q << 32 | index + 1) over the pixels of its disc; the
//                       largest key of a pixel owns it, whatever the scheduling                           common/utils.py:12-43
//   k_report_image_grid one thread per OUTPUT pixel                                                      main.py:258-278, common/utils.py:76-78
// Every number that decides a pixel or a table index is a double computed WITHOUT multiply-add contraction (the pragma below covers the
// whole file; the build passes -ffp-contract=on), so that numpy's separately rounded operations give the same bits (report.py: *_host).
// No spin loops, no float atomics, no grid exchange.
#include "nf_common.h"

#pragma clang fp contract(off)

#include "nf_cmaps.h"                                   // host copy: NF_CMAP_TABLES (nf_report_cmap)
#undef NF_CMAP_DECL
#define NF_CMAP_DECL __constant__ uint8_t d_cmap_tables  // device copy, the same initialiser
#include "nf_cmaps.h"

#define NF_REPORT_MAX_MAP 16384
#define NF_REPORT_MAX_CANVAS 4096
#define NF_REPORT_MAX_RADIUS 8

// ---- grid ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NF_BLOCK) k_report_grid(float* __restrict__ y, int map_size) {
    const int64_t total = (int64_t)map_size * map_size, gstride = (int64_t)gridDim.x * blockDim.x;
    const double ms = (double)map_size;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gstride) {
        const int64_t i = e / map_size, j = e - i * map_size;
        const double ix = ((double)j + 0.5) / ms * 2.0 - 1.0;          // main.py:200
        const double iy = ((double)i + 0.5) / ms * -2.0 + 1.0;         // main.py:201
        y[2 * e] = (float)ix;
        y[2 * e + 1] = (float)iy;
    }
}

extern "C" int nf_report_grid(float* y, int map_size, nf_stream_t stream) {
    if (y == nullptr || map_size < 1 || map_size > NF_REPORT_MAX_MAP) return NF_E_BADARG;
    hipLaunchKernelGGL(k_report_grid, dim3(nf_grid_for((int64_t)map_size * map_size)), dim3(NF_BLOCK), 0, (hipStream_t)stream, y, map_size);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---- finite range ----------------------------------------------------------------------------------------------------------------------
// order-preserving image of a double in the unsigned integers: a < b  <=>  ord(a) < ord(b) for all finite a, b (and -0 < +0).  No finite
// value maps to 0 or to 2^64 - 1: those two are the "nothing seen yet" sentinels.
__device__ __forceinline__ unsigned long long nf_ord(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double nf_unord(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

__global__ void k_minmax_init(unsigned long long* __restrict__ r) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        r[0] = ~0ull;
        r[1] = 0ull;
    }
}

__global__ void __launch_bounds__(NF_BLOCK) k_minmax_reduce(const float* __restrict__ v, int64_t n, unsigned long long* __restrict__ r) {
    __shared__ float s_lo[NF_BLOCK / NF_WAVE], s_hi[NF_BLOCK / NF_WAVE];
    float lo = INFINITY, hi = -INFINITY;                    // lo > hi: no finite value seen
    const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gstride) {
        const float x = v[e];
        if (fabsf(x) <= 3.402823466e+38f) {                 // finite (false for NaN)
            lo = fminf(lo, x);
            hi = fmaxf(hi, x);
        }
    }
#pragma unroll
    for (int off = NF_WAVE / 2; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, NF_WAVE));
        hi = fmaxf(hi, __shfl_xor(hi, off, NF_WAVE));
    }
    const int lane = threadIdx.x & (NF_WAVE - 1), wid = threadIdx.x >> 6;
    if (lane == 0) {
        s_lo[wid] = lo;
        s_hi[wid] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NF_BLOCK / NF_WAVE; ++w) {
            lo = fminf(lo, s_lo[w]);
            hi = fmaxf(hi, s_hi[w]);
        }
        if (lo <= hi) {
            atomicMin(&r[0], nf_ord((double)lo));
            atomicMax(&r[1], nf_ord((double)hi));
        }
    }
}

__global__ void k_minmax_decode(unsigned long long* __restrict__ r) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long a = r[0], b = r[1];
        double* out = reinterpret_cast<double*>(r);
        if (a == ~0ull) {                                   // no finite value
            out[0] = 0.0;
            out[1] = 1.0;
        } else {
            out[0] = nf_unord(a);
            out[1] = nf_unord(b);
        }
    }
}

extern "C" int nf_report_minmax(const float* v, int64_t n, double* range2, nf_stream_t stream) {
    if (v == nullptr || range2 == nullptr || n < 1) return NF_E_BADARG;
    unsigned long long* r = reinterpret_cast<unsigned long long*>(range2);
    hipLaunchKernelGGL(k_minmax_init, dim3(1), dim3(NF_WAVE), 0, (hipStream_t)stream, r);
    NF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_minmax_reduce, dim3(nf_grid_for(n, 4 * NF_BLOCK)), dim3(NF_BLOCK), 0, (hipStream_t)stream, v, n, r);
    NF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_minmax_decode, dim3(1), dim3(NF_WAVE), 0, (hipStream_t)stream, r);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---- value -> colour -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NF_BLOCK) k_report_colorize(const float* v, int64_t n, int is_log, const double* __restrict__ range_dev,
                                                              double vmin, double vmax, int cmap, float* p_out, uint8_t* __restrict__ rgb) {
    const double lo = range_dev != nullptr ? range_dev[0] : vmin, hi = range_dev != nullptr ? range_dev[1] : vmax;
    const uint8_t* __restrict__ tab = d_cmap_tables[cmap];
    const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gstride) {
        float p = v[e];
        if (is_log) p = (float)exp((double)p);
        if (p_out != nullptr) p_out[e] = p;
        if (rgb == nullptr) continue;
        uint8_t c0 = 0, c1 = 0, c2 = 0;                     // NaN: matplotlib's "bad" colour as bytes
        if (p == p) {
            int idx = 0;
            if (hi != lo) {
                const double x = ((double)p - lo) / (hi - lo);
                if (!(x >= 0.0)) idx = 0;
                else if (x >= 1.0) idx = 255;
                else idx = (int)floor(x * 256.0);
            }
            c0 = tab[3 * idx];
            c1 = tab[3 * idx + 1];
            c2 = tab[3 * idx + 2];
        }
        rgb[3 * e] = c0;
        rgb[3 * e + 1] = c1;
        rgb[3 * e + 2] = c2;
    }
}

extern "C" int nf_report_colorize(const float* v, int64_t n, int is_log, const double* range_dev, double vmin, double vmax, int cmap,
                                  float* p_out, uint8_t* rgb, nf_stream_t stream) {
    if (v == nullptr || n < 1 || (p_out == nullptr && rgb == nullptr)) return NF_E_BADARG;
    if (cmap < 0 || cmap >= NF_CMAP_COUNT || (is_log != 0 && is_log != 1)) return NF_E_BADARG;
    if (range_dev == nullptr && !(fabs(vmin) <= 1.7976931348623157e308 && fabs(vmax) <= 1.7976931348623157e308)) return NF_E_BADARG;
    hipLaunchKernelGGL(k_report_colorize, dim3(nf_grid_for(n)), dim3(NF_BLOCK), 0, (hipStream_t)stream, v, n, is_log, range_dev, vmin, vmax,
                       cmap, p_out, rgb);
    NF_CHECK_LAUNCH();
    return 0;
}

extern "C" int nf_report_cmap(int cmap, uint8_t* out768) {
    if (out768 == nullptr || cmap < 0 || cmap >= NF_CMAP_COUNT) return NF_E_BADARG;
    for (int k = 0; k < 768; ++k) out768[k] = NF_CMAP_TABLES[cmap][k];
    return 0;
}

// ---- scatter panel ---------------------------------------------------------------------------------------------------------------------
struct NfView9 {
    double m[9];
};

__global__ void __launch_bounds__(NF_BLOCK) k_report_clear(unsigned long long* __restrict__ keys, int64_t n) {
    const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gstride) keys[e] = 0ull;
}

__device__ __forceinline__ bool nf_finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

__global__ void __launch_bounds__(NF_BLOCK) k_report_splat(const float* __restrict__ pts, int64_t n, int D, NfView9 view, int S, int radius,
                                                           unsigned long long* __restrict__ keys) {
    const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    const double Sd = (double)S, rd = (double)radius;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gstride) {
        const double x = (double)pts[i * D], y = (double)pts[i * D + 1];
        double u = x, w = y, depth = 0.0;
        if (D == 3) {
            const double z = (double)pts[i * D + 2];
            u = (view.m[0] * x + view.m[1] * y) + view.m[2] * z;
            w = (view.m[3] * x + view.m[4] * y) + view.m[5] * z;
            depth = (view.m[6] * x + view.m[7] * y) + view.m[8] * z;
        }
        if (!(nf_finite_d(u) && nf_finite_d(w) && nf_finite_d(depth))) continue;       // a NaN / inf coordinate ends here too
        const double cxd = floor((u + 1.0) * 0.5 * Sd), cyd = floor((1.0 - w) * 0.5 * Sd);
        if (cxd + rd < 0.0 || cxd - rd >= Sd || cyd + rd < 0.0 || cyd - rd >= Sd) continue;   // the disc lies wholly outside
        const int cx = (int)cxd, cy = (int)cyd;             // within [-radius, S + radius): fits
        double t = (depth + 2.0) / 4.0;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const unsigned long long key = ((unsigned long long)floor(t * 1048575.0) << 32) | (unsigned long long)(i + 1);
        for (int dy = -radius; dy <= radius; ++dy) {
            const int py = cy + dy;
            if (py < 0 || py >= S) continue;
            for (int dx = -radius; dx <= radius; ++dx) {
                const int px = cx + dx;
                if (px < 0 || px >= S || dx * dx + dy * dy > radius * radius) continue;
                atomicMax(&keys[(int64_t)py * S + px], key);
            }
        }
    }
}

__global__ void __launch_bounds__(NF_BLOCK) k_report_resolve(const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ rgb_pt,
                                                             int64_t n_pix, uint8_t* __restrict__ out) {
    const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_pix; e += gstride) {
        const unsigned long long key = keys[e];
        uint8_t c0 = 255, c1 = 255, c2 = 255;               // nobody painted here: the white background
        if (key != 0ull) {
            const int64_t idx = (int64_t)(key & 0xffffffffull) - 1;
            c0 = rgb_pt[3 * idx];
            c1 = rgb_pt[3 * idx + 1];
            c2 = rgb_pt[3 * idx + 2];
        }
        out[3 * e] = c0;
        out[3 * e + 1] = c1;
        out[3 * e + 2] = c2;
    }
}

extern "C" int nf_report_scatter(const float* pts, const uint8_t* rgb_pt, int64_t n, int D, const double* view9, int S, int radius,
                                 unsigned long long* keys, uint8_t* rgb_out, nf_stream_t stream) {
    if (keys == nullptr || rgb_out == nullptr || n < 0 || n >= ((int64_t)1 << 31)) return NF_E_BADARG;
    if (n > 0 && (pts == nullptr || rgb_pt == nullptr)) return NF_E_BADARG;
    if ((D != 2 && D != 3) || (D == 3 && view9 == nullptr)) return NF_E_BADARG;
    if (S < 1 || S > NF_REPORT_MAX_CANVAS || radius < 0 || radius > NF_REPORT_MAX_RADIUS) return NF_E_BADARG;
    NfView9 view;
    for (int k = 0; k < 9; ++k) view.m[k] = (D == 3) ? view9[k] : (k % 4 == 0 ? 1.0 : 0.0);
    const int64_t n_pix = (int64_t)S * S;
    hipLaunchKernelGGL(k_report_clear, dim3(nf_grid_for(n_pix)), dim3(NF_BLOCK), 0, (hipStream_t)stream, keys, n_pix);
    NF_CHECK_LAUNCH();
    if (n > 0) {
        hipLaunchKernelGGL(k_report_splat, dim3(nf_grid_for(n)), dim3(NF_BLOCK), 0, (hipStream_t)stream, pts, n, D, view, S, radius, keys);
        NF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_report_resolve, dim3(nf_grid_for(n_pix)), dim3(NF_BLOCK), 0, (hipStream_t)stream, keys, rgb_pt, n_pix, rgb_out);
    NF_CHECK_LAUNCH();
    return 0;
}

// ---- image grid ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t nf_to_byte(float x) {    // (uint8)(clamp(x, 0, 1) * 255.0f), NaN -> 0
    const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;
    return (uint8_t)(c * 255.0f);
}

__global__ void __launch_bounds__(NF_BLOCK) k_report_image_grid(const float* __restrict__ x, int64_t n, int C, int H, int W, int xmaps,
                                                                int padding, float pad_value, int Hout, int Wout,
                                                                uint8_t* __restrict__ out) {
    const int64_t total = (int64_t)Hout * Wout, gstride = (int64_t)gridDim.x * blockDim.x;
    const int ch = H + padding, cw = W + padding;
    const uint8_t pad = nf_to_byte(pad_value);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gstride) {
        const int oy = (int)(e / Wout), ox = (int)(e - (int64_t)oy * Wout);
        const int gy = oy - padding, gx = ox - padding;
        uint8_t c0 = pad, c1 = pad, c2 = pad;
        if (gy >= 0 && gx >= 0) {
            const int ry = gy / ch, iy = gy - ry * ch, rx = gx / cw, ix = gx - rx * cw;
            const int64_t k = (int64_t)ry * xmaps + rx;
            if (iy < H && ix < W && rx < xmaps && k < n) {
                const float* __restrict__ img = x + k * C * H * W + (int64_t)iy * W + ix;
                c0 = nf_to_byte(img[0]);
                if (C == 3) {
                    c1 = nf_to_byte(img[(int64_t)H * W]);
                    c2 = nf_to_byte(img[(int64_t)2 * H * W]);
                } else {
                    c1 = c2 = c0;
                }
            }
        }
        out[3 * e] = c0;
        out[3 * e + 1] = c1;
        out[3 * e + 2] = c2;
    }
}

extern "C" int nf_report_image_grid(const float* x, int64_t n, int C, int H, int W, int nrow, int padding, float pad_value, uint8_t* out,
                                    nf_stream_t stream) {
    if (x == nullptr || out == nullptr || n < 1 || (C != 1 && C != 3) || H < 1 || W < 1 || nrow < 1 || padding < 0) return NF_E_BADARG;
    const int64_t xmaps = n < nrow ? n : nrow, ymaps = (n + xmaps - 1) / xmaps;
    const int64_t Hout = ((int64_t)H + padding) * ymaps + padding, Wout = ((int64_t)W + padding) * xmaps + padding;
    if (Hout >= ((int64_t)1 << 31) || Wout >= ((int64_t)1 << 31) || Hout * Wout >= ((int64_t)1 << 40)) return NF_E_BADARG;
    hipLaunchKernelGGL(k_report_image_grid, dim3(nf_grid_for(Hout * Wout)), dim3(NF_BLOCK), 0, (hipStream_t)stream, x, n, C, H, W, (int)xmaps,
                       padding, pad_value, (int)Hout, (int)Wout, out);
    NF_CHECK_LAUNCH();
    return 0;
}
