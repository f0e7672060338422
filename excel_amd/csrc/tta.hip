// Test-time augmentation of the training-free LAMs (include/excel_hip.h, "flip and multi-scale LAM fuse"): the fuse that sits between
// the patch-text CAM and the random walk when infer_lam runs several scales and / or the mirrored image (utils/camutils.py:8-63).
//
//   lam_tta_accumulate_kernel   every scale's maps [B or 2B, g_s^2, F] -> bilinear to the g_out grid -> max with the mirrored half
//                               -> sum over scales, in registers -> out [B, g_out^2, F] (un-normalised)
//   lam_tta_normalize_kernel    per (b, f) plane of out: lam -= min ; lam /= max + 1e-5, in place; a plane with a non-finite value
//                               becomes NaN as a whole
//
// Both walk memory with the class as the fastest index, the layout of the model's maps and of what the random walk reads: a wave's
// loads and stores cover consecutive classes of one token, then the next token.  The sources are small (B * g^2 * F floats per scale,
// L2-resident); the op is launch- and gather-bound.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define TTA_MAX_SCALES 8
#define TTA_MAX_GRID 48
#define TTA_COLS 16          // classes per workgroup of the normalise pass
#define TTA_THREADS 1024

struct TtaScales {
    const float* maps[TTA_MAX_SCALES];   // [B or 2B, g*g, F]: image b, then (flip) its mirrored copy at b + B
    int g[TTA_MAX_SCALES];
    int ns;
};

__device__ __forceinline__ bool tta_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// one thread per output value, (b, token, class) with the class fastest.  The sample is lam_scale_accumulate_kernel's (attr.hip:
// bilinear_tap + bilinear_blend), and contraction is off so that nothing fuses across the steps around it: the GPU tests pin the
// fuse to the chain of lam_scale_accumulate + plane_minmax_normalize bit for bit.  fmaxf drops a NaN (and -inf) of one half, so a
// non-finite sample of either half is carried on as a NaN: the sum stays non-finite and the normalise pass sees it.
__global__ __launch_bounds__(256) void lam_tta_accumulate_kernel(TtaScales sc, int B, int F, int G, int flip, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int P = G * G;
    if (i >= (long long)B * P * F) return;
    const int f = (int)(i % F), p = (int)((i / F) % P), b = (int)(i / ((long long)F * P));
    const int y = p / G, x = p % G;
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < TTA_MAX_SCALES; ++s) {
        if (s < sc.ns) {
            const int g = sc.g[s];
            const long long img = (long long)g * g * F;
            auto sample = [&](const float* __restrict__ m, int xx) {   // m = the (image, class) plane's first element; token stride F
                const BilinearTap t = bilinear_tap(xx, y, g, g, G, G, 0);
                auto at = [&](int yy, int xc) { return m[(yy * g + xc) * F]; };
                return bilinear_blend(t, at(t.y0, t.x0), at(t.y0, t.x1), at(t.y1, t.x0), at(t.y1, t.x1));
            };
            float v = sample(sc.maps[s] + b * img + f, x);
            if (flip) {
                const float c = sample(sc.maps[s] + (b + B) * img + f, G - 1 - x);   // lam[B + b].flip(-1)
                v = (tta_nonfinite(v) || tta_nonfinite(c)) ? NAN : fmaxf(v, c);
            }
            acc = s == 0 ? v : acc + v;
        }
    }
    out[i] = acc;
}

// grid (B, cdiv(F, TTA_COLS)), 1024 threads: the workgroup owns fw <= 16 consecutive classes of image b; thread (r, c) = (tid / fw,
// tid % fw) walks the tokens r, r + rows, ... of class f0 + c (rows = the largest power of two with rows * fw <= 1024), so a wave
// reads runs of consecutive classes and a thread holds a dozen values of a 28 x 28 plane, not the whole column: the pass is a chain
// of memory round trips per thread, and 32 images are only 32 x cdiv(F, 16) workgroups.  Every thread re-reads only what it read
// before.  min / max do not depend on the order they are taken in: the bits are plane_minmax_normalize_kernel's.
__global__ __launch_bounds__(TTA_THREADS) void lam_tta_normalize_kernel(float* __restrict__ out, int P, int F) {
    __shared__ float smn[TTA_THREADS], smx[TTA_THREADS];
    __shared__ int sbad[TTA_THREADS];
    const int f0 = blockIdx.y * TTA_COLS, b = blockIdx.x, tid = threadIdx.x;
    const int fw = min(TTA_COLS, F - f0);
    const int rows = 1 << (31 - __clz(TTA_THREADS / fw));
    const int r = tid / fw, c = tid % fw;
    float* pl = out + (long long)b * P * F + f0 + c;
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    if (r < rows) {
#pragma unroll 4
        for (int p = r; p < P; p += rows) {
            const float v = pl[(long long)p * F];
            mn = fminf(mn, v); mx = fmaxf(mx, v);
            bad |= tta_nonfinite(v);
        }
    }
    smn[tid] = mn; smx[tid] = mx; sbad[tid] = bad;
    __syncthreads();
    for (int h = rows >> 1; h > 0; h >>= 1) {          // rows r and r + h of the same class: tid + h * fw < rows * fw <= 1024
        if (r < h) {
            const int o = tid + h * fw;
            smn[tid] = fminf(smn[tid], smn[o]); smx[tid] = fmaxf(smx[tid], smx[o]); sbad[tid] |= sbad[o];
        }
        __syncthreads();
    }
    if (r >= rows) return;
    mn = smn[c]; mx = smx[c]; bad = sbad[c];
    const float den = (mx - mn) + 1e-5f;
#pragma unroll 4
    for (int p = r; p < P; p += rows) pl[(long long)p * F] = bad ? NAN : (pl[(long long)p * F] - mn) / den;
}

extern "C" int excel_lam_tta_fuse(const float* const* maps, const int32_t* g, int ns, int flip, int B, int F, int g_out, float* out,
                                  void* stream) {
    EXCEL_CHECK_ARG(maps && g && out, "lam_tta_fuse: null argument");
    EXCEL_CHECK_ARG(ns >= 1 && ns <= TTA_MAX_SCALES, "lam_tta_fuse: ns = %d outside [1, %d]", ns, TTA_MAX_SCALES);
    EXCEL_CHECK_ARG(g_out >= 1 && g_out <= TTA_MAX_GRID, "lam_tta_fuse: g_out = %d outside [1, %d]", g_out, TTA_MAX_GRID);
    EXCEL_CHECK_ARG(B >= 1 && F >= 1, "lam_tta_fuse: need B >= 1 and F >= 1 (B = %d, F = %d)", B, F);
    // every offset inside one image's planes is an int: g^2 * F of the largest grid
    EXCEL_CHECK_ARG((long long)TTA_MAX_GRID * TTA_MAX_GRID * F <= 2147483647ll, "lam_tta_fuse: F = %d: 48^2 * F must stay below 2^31", F);
    TtaScales sc;
    memset(&sc, 0, sizeof(sc));
    sc.ns = ns;
    for (int s = 0; s < ns; ++s) {
        EXCEL_CHECK_ARG(maps[s], "lam_tta_fuse: scale %d: null maps", s);
        EXCEL_CHECK_ARG(g[s] >= 1 && g[s] <= TTA_MAX_GRID, "lam_tta_fuse: scale %d: g = %d outside [1, %d]", s, g[s], TTA_MAX_GRID);
        sc.maps[s] = maps[s];
        sc.g[s] = g[s];
    }
    const int P = g_out * g_out;
    const long long total = (long long)B * P * F;
    EXCEL_CHECK_ARG(cdivl(total, 256) <= 2147483647ll, "lam_tta_fuse: B * g_out^2 * F = %lld is too large for one launch", total);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lam_tta_accumulate_kernel, dim3((unsigned)cdivl(total, 256)), dim3(256), 0, st, sc, B, F, g_out, flip ? 1 : 0, out);
    EXCEL_CHECK_LAUNCH("lam_tta_accumulate");
    hipLaunchKernelGGL(lam_tta_normalize_kernel, dim3(B, cdiv(F, TTA_COLS)), dim3(TTA_THREADS), 0, st, out, P, F);
    EXCEL_CHECK_LAUNCH("lam_tta_normalize");
    return EXCEL_OK;
}
