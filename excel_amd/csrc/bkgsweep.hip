// Background-scale sweep (include/excel_hip.h, "background-scale sweep").
//
// The pseudo labels are the arg-max over [b0 ; cam_1 .. cam_k] of PAR's output (argmax_key, par.hip).  PAR is linear per channel, so the
// labels a background scaled by `a` would have given need no second PAR pass: pixel (x,y) is background at scale a iff a * b0 >= F, with
// F the best foreground score.  One kernel reads the step's PAR output once and
//
//   bkg_sweep_kernel : totals[j,0,g] += pixels with ground truth g                      (the margins of the confusion matrix the labels of
//                      totals[j,1,p] += pixels with key_j == p                           scale j would have given: row sums, column sums,
//                      totals[j,2,g] += pixels with g == key_j                           diagonal - image_scores_kernel's rows, per scale)
//                      over the pixels with g < nc and key_j < nc of the images with skip[b] == 0, for all K scales at once, and
//                      labels[pixel] = key_{label_sel}                                   (optional: the label map of ONE scale)
//
// Tiles and lanes are argmax_label_ragged_kernel's (64 x 16 tiles, one lane per column, four rows per lane: a plane read is 64
// consecutive floats per wave); a workgroup takes four tiles at a time and strides over the tile list, so that few workgroups flush.
//
// Counters.  Counting every scale on its own costs up to 2K + 1 LDS atomics per pixel.  Instead a pixel is counted under the scales at
// which it CHANGES sides.  With f(j) = 1 where the pixel is foreground at scale j, f(K) = 0, any f is a sum of prefix steps:
//     f(j) = sum over m > j of a_m,   1 - f(j) = sum over m <= j of a_m,   a_0 = 1 - f(0),  a_m = f(m-1) - f(m)  (m = 1..K),
// so the pixel adds a_m (+1 or -1, in wrapping u32) to bin [m] and the flush turns the bins into per-scale counts by one running sum.
// For increasing scales and b0 >= 0 - what PAR of a non-negative plane always gives - the pixel is foreground on a prefix j < m only,
// and exactly one a_m is non-zero: one atomic.  Per pixel that is
//     G[g] += 1                      ground-truth area, the same at every scale
//     P[m][key_fg] += a_m            predicted area: column c >= 1 sums m > j; background = the ROW sums of P, summed over m <= j
//     I[m][g] += a_m                 intersection, only when g == key_fg (summed m > j) or g == 0 (column 0, summed m <= j)
// - at most 3 LDS atomics whatever K, and 1 + 2 * (sign changes + 1) for a pixel whose mask is no such prefix (b0 < 0, unsorted
// scales): the same bins, no second form.  The sums are exact: every true count is below 2^32, so wrapping cancels.  A pixel whose
// foreground key is >= nc counts only where it is background and cannot use G; it adds to the totals directly (a caller whose class
// keys exceed num_classes: rare by construction).  LDS: (1 + 2 (K+1)) nc + K + 1 words, allocated at launch for the call's K and nc
// (1.6 KB at K = 8, nc = 21; 35.1 KB at K = 16, nc = 256; none for a call that only writes labels).  No workspace, no
// scratch; scales travel by value in the kernel arguments.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define BKG_MAXK 16
#define BKG_MAXNC 256
// A counting launch ends in one 64-bit global atomic per workgroup and non-zero (scale, row, class): they queue up per address, and that
// queue, not the LDS atomics, is what the kernel waits for (EXPERIMENTS.md, "Background-scale sweep": 2048 workgroups of 256 threads
// 97 us, 1024 of them 83 us, 256 of 1024 threads 58 us; folding the lanes of a wave that share a bin into one LDS atomic gained
// nothing).  So a workgroup is 16 waves that take four tiles at a time, and a counting launch has at most one per CU of the MI355X.
#define BKG_THREADS 1024
#define BKG_SUBS (BKG_THREADS / 256)             // tiles a workgroup works on at a time (256 threads each: argmax_label_ragged_kernel's)
#define BKG_MAX_GROUPS 256                       // workgroups of a launch that counts (and flushes)
static inline size_t bkg_lds_bytes(int K, int nc) { return sizeof(unsigned int) * ((size_t)(1 + 2 * (K + 1)) * nc + K + 1); }

struct BkgScales { float s[BKG_MAXK]; };

__global__ __launch_bounds__(BKG_THREADS) void bkg_sweep_kernel(const float* __restrict__ planes, const int* __restrict__ nchan,
                                                        const int* __restrict__ cls_idx, const unsigned char* __restrict__ gt, TileGeo geo,
                                                        int total_tiles, int Smax, int Cmax, BkgScales sc, int K,
                                                        const int* __restrict__ skip, int nc, unsigned long long* __restrict__ totals,
                                                        int label_sel, unsigned char* __restrict__ lab8) {
    extern __shared__ unsigned int lds[];                    // bkg_lds_bytes(K, nc), or nothing when totals == nullptr
    const int rows = K + 1;
    unsigned int* G = lds;                                   // [nc]
    unsigned int* P = G + nc;                                // [K+1][nc]
    unsigned int* I = P + rows * nc;                         // [K+1][nc]
    unsigned int* Z = I + rows * nc;                         // [K+1] row sums of P (flush)
    const int words = (1 + 2 * rows) * nc + rows;
    if (totals) {
        for (int i = threadIdx.x; i < words; i += BKG_THREADS) lds[i] = 0;
        __syncthreads();
    }
    const unsigned int full = (1u << K) - 1u;
    const int lane256 = threadIdx.x & 255;                   // the thread's place in its tile: argmax_label_ragged_kernel's
    for (int tile = blockIdx.x * BKG_SUBS + (threadIdx.x >> 8); tile < total_tiles; tile += gridDim.x * BKG_SUBS) {
        const Tile t = tile_of_ragged(geo, tile);
        const int x = t.x0 + (lane256 & 63);
        if (x >= t.W) continue;                              // (no barrier inside the loop)
        const int nch = nchan ? min(nchan[t.b], Cmax) : Cmax;
        const int* cls_row = cls_idx ? cls_idx + (long long)t.b * Smax : nullptr;
        const float* cb = planes + (long long)Cmax * t.base;
        const bool count = totals && !(skip && skip[t.b] != 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = t.y0 + (lane256 >> 6) + 4 * r;
            if (y >= t.H) continue;
            const float* p = cb + (long long)y * t.Wp + x;
            const float b0 = p[0];
            unsigned int bg = full;                          // bit j: background at scale j
            int key_fg = 0;
            if (nch > 1) {
                float F = p[t.HW];
                int ci = 1;
                for (int c = 2; c < nch; ++c) {
                    const float v = p[(long long)c * t.HW];
                    if (v > F) { F = v; ci = c; }            // the first maximum wins, like argmax_key (par.hip)
                }
                key_fg = cls_row ? cls_row[ci - 1] + 1 : ci;
                bg = 0;
#pragma unroll
                for (int j = 0; j < BKG_MAXK; ++j)
                    if (j < K && __fmul_rn(sc.s[j], b0) >= F) bg |= 1u << j;
                if (key_fg == 0) bg = full;                  // a foreground slot that maps to key 0: background either way
            }
            const long long pix = t.lab + (long long)y * t.W + x;
            if (lab8) lab8[pix] = (unsigned char)(((bg >> label_sel) & 1u) ? 0 : key_fg);
            if (!count) continue;
            const int g = gt[pix];
            if (g >= nc) continue;
            const unsigned int fg = ~bg & full;
            if (key_fg >= nc) {                              // counts only where it is background: straight to the totals
                for (unsigned int m = bg; m; m &= m - 1) {
                    const int j = __ffs(m) - 1;
                    unsigned long long* tj = totals + (long long)j * 3 * nc;
                    atomicAdd(&tj[g], 1ull);
                    atomicAdd(&tj[nc], 1ull);
                    if (g == 0) atomicAdd(&tj[2 * nc], 1ull);
                }
                continue;
            }
            const unsigned int up = ((fg << 1) | 1u) & ~fg;  // bits m (0..K) with a_m = +1
            const unsigned int dn = fg & ~((fg << 1) | 1u);  // bits m (1..K-1) with a_m = -1
            const bool hit = (g == 0 || g == key_fg);
            atomicAdd(&G[g], 1u);
            for (unsigned int m = up; m; m &= m - 1) {
                const int mm = __ffs(m) - 1;
                atomicAdd(&P[mm * nc + (mm ? key_fg : 0)], 1u);
                if (hit) atomicAdd(&I[mm * nc + g], 1u);
            }
            for (unsigned int m = dn; m; m &= m - 1) {
                const int mm = __ffs(m) - 1;
                atomicAdd(&P[mm * nc + key_fg], 0xffffffffu);
                if (hit) atomicAdd(&I[mm * nc + g], 0xffffffffu);
            }
        }
    }
    if (!totals) return;
    __syncthreads();
    // ---- flush: row sums of P (the pixels that turn background at m), then one running sum per class
    for (int m = threadIdx.x >> 6; m < rows; m += BKG_THREADS / 64) {
        unsigned int s = 0;
        for (int c = threadIdx.x & 63; c < nc; c += 64) s += P[m * nc + c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0) Z[m] = s;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= nc) return;
    const unsigned int area = G[c];
    if (c == 0) {                                            // background: the bins at or below the scale
        unsigned int pred = 0, inter = 0;
        for (int j = 0; j < K; ++j) {
            pred += Z[j];
            inter += I[j * nc];
            unsigned long long* tj = totals + (long long)j * 3 * nc;
            if (area) atomicAdd(&tj[0], (unsigned long long)area);
            if (pred) atomicAdd(&tj[nc], (unsigned long long)pred);
            if (inter) atomicAdd(&tj[2 * nc], (unsigned long long)inter);
        }
    } else {                                                 // a foreground class: the bins above the scale
        unsigned int pred = 0, inter = 0;
        for (int j = K - 1; j >= 0; --j) {
            pred += P[(j + 1) * nc + c];
            inter += I[(j + 1) * nc + c];
            unsigned long long* tj = totals + (long long)j * 3 * nc;
            if (area) atomicAdd(&tj[c], (unsigned long long)area);
            if (pred) atomicAdd(&tj[nc + c], (unsigned long long)pred);
            if (inter) atomicAdd(&tj[2 * nc + c], (unsigned long long)inter);
        }
    }
}

extern "C" int excel_bkg_sweep_ragged(const float* planes, const int32_t* nchan, const int32_t* cls_idx, const uint8_t* gt,
                                      const int32_t* table, const excel_ragged_info* info, int Smax, int Cmax, const float* scales, int K,
                                      const int32_t* skip, int num_classes, int64_t* totals, int label_sel, uint8_t* labels_u8,
                                      void* stream) {
    EXCEL_CHECK_ARG(planes && table && info, "bkg_sweep_ragged: null argument (planes, table and info are required)");
    EXCEL_CHECK_ARG(totals || labels_u8, "bkg_sweep_ragged: nothing to do (neither totals nor labels_u8)");
    EXCEL_CHECK_ARG(!totals || gt, "bkg_sweep_ragged: totals needs the ground truth (gt is null)");
    EXCEL_CHECK_ARG(K >= 1 && K <= BKG_MAXK, "bkg_sweep_ragged: need 1 <= K <= %d (K = %d)", BKG_MAXK, K);
    EXCEL_CHECK_ARG(scales, "bkg_sweep_ragged: null scales");
    BkgScales sc;
    for (int j = 0; j < BKG_MAXK; ++j) sc.s[j] = 0.f;
    for (int j = 0; j < K; ++j) {
        EXCEL_CHECK_ARG(scales[j] >= 0.f && scales[j] <= 3.402823466e38f, "bkg_sweep_ragged: scale %d is %g: scales must be finite and >= 0", j,
                        (double)scales[j]);
        sc.s[j] = scales[j];
    }
    EXCEL_CHECK_ARG(!labels_u8 || (label_sel >= 0 && label_sel < K), "bkg_sweep_ragged: label_sel = %d is outside [0, %d)", label_sel, K);
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= BKG_MAXNC, "bkg_sweep_ragged: need 1 <= num_classes <= %d (got %d)", BKG_MAXNC,
                    num_classes);
    EXCEL_CHECK_ARG(((uintptr_t)totals & 7) == 0, "bkg_sweep_ragged: totals must be 8-byte aligned");
    EXCEL_CHECK_ARG(((uintptr_t)planes & 15) == 0, "bkg_sweep_ragged: planes must be 16-byte aligned");
    EXCEL_CHECK_ARG((((uintptr_t)nchan | (uintptr_t)cls_idx | (uintptr_t)skip | (uintptr_t)table) & 3) == 0,
                    "bkg_sweep_ragged: nchan, cls_idx, skip and table must be 4-byte aligned");
    EXCEL_CHECK_ARG(Cmax >= 1 && (!cls_idx || Smax >= Cmax - 1), "bkg_sweep_ragged: need Cmax >= 1 and, with cls_idx, Smax >= Cmax - 1 (Cmax = %d, Smax = %d)",
                    Cmax, Smax);
    EXCEL_CHECK_ARG(info->B >= 1 && info->total_tiles >= 1, "bkg_sweep_ragged: the plan holds no tile");
    TileGeo geo;
    geo.tab = table; geo.B = info->B; geo.H = geo.W = 0;
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    const int want = cdiv(info->total_tiles, BKG_SUBS);
    const int groups = (totals && want > BKG_MAX_GROUPS) ? BKG_MAX_GROUPS : want;
    const size_t lds = totals ? bkg_lds_bytes(K, num_classes) : 0;         // 35 972 B at most: under the 64 KB of a plain launch
    hipLaunchKernelGGL(bkg_sweep_kernel, dim3((unsigned)groups), dim3(BKG_THREADS), lds, st, planes, nchan, cls_idx, gt, geo, info->total_tiles, Smax, Cmax,
                       sc, K, skip, num_classes, (unsigned long long*)totals, labels_u8 ? label_sel : 0, labels_u8);
    EXCEL_CHECK_LAUNCH("bkg_sweep_ragged");
    return EXCEL_OK;
}
