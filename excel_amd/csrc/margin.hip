// Arg-max margin (include/excel_hip.h, "arg-max margin").
//
// The pseudo labels are the arg-max over [a * b0 ; cam_1 .. cam_k] of PAR's output (bkgsweep.hip at scale a).  The step knows by how
// much the winning plane won - winner minus runner-up - and this kernel keeps it: one pass over the planes the step already has gives
//
//   margin_kernel : margin_out[pixel] = margin                                            (optional)
//                   labels[pixel]     = margin >= label_thre ? key : 255                  (optional: the label set cut at ONE value)
//                   kept[j]          += pixels with margin >= t_j,  kept[K] += all pixels (optional; images with skip[b] == 0)
//                   totals[j,0,g]    += kept pixels with ground truth g                   (optional: the margins of the confusion matrix
//                   totals[j,1,key]  += kept pixels with label key                         of "labels with 255 where margin < t_j", for all
//                   totals[j,2,g]    += kept pixels with g == key                          K thresholds at once; g < nc and key < nc)
//
// Tiles, lanes and the workgroup's walk over the tile list are bkg_sweep_kernel's (64 x 16 tiles, one lane per column, four rows per
// lane, 1024 threads on four tiles at a time, at most 256 workgroups in a launch that counts).
//
// Counters.  The thresholds increase, so the kept sets are nested and a pixel is described by m = the number of thresholds it passes:
// it is counted ONCE, in bin m (1..K; a pixel with m == 0 is kept nowhere and only counts in kept[K]), and the flush turns the bins into
// per-threshold counts with one suffix sum (threshold j holds the bins m > j).  Per pixel that is one LDS atomic on the kept counter and
//     G[m][g] += 1,   P[m][key] += 1,   I[m][g] += 1 when g == key
// - at most 3 more whatever K.  The bins are u32 and cannot wrap (a launch has fewer than 2^31 pixels); the flush adds them to the
// 64-bit totals with one global atomic per workgroup and non-zero (threshold, row, class).  A pixel whose key is >= nc is in no row of
// the totals (bkgsweep.hip counts such a pixel where it is background; here it has one key, so there is nothing to add).
// LDS: (K + 1) + 3 (K+1) nc words for the call's K and nc (2.3 KB at K = 8, nc = 21; 52.3 KB at K = 16, nc = 256; K + 1 words for a
// call that only wants kept; none for a call that only writes labels or margins).  No workspace, no scratch; the thresholds travel by
// value in the kernel arguments.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define MRG_MAXK 16
#define MRG_MAXNC 256
#define MRG_THREADS 1024
#define MRG_SUBS (MRG_THREADS / 256)             // tiles a workgroup works on at a time (256 threads each)
#define MRG_MAX_GROUPS 256                       // workgroups of a launch that counts (and flushes): bkgsweep.hip's measurement
static inline size_t margin_lds_bytes(int K, int nc, bool totals, bool kept) {
    return sizeof(unsigned int) * ((totals || kept ? (size_t)(K + 1) : 0) + (totals ? (size_t)3 * (K + 1) * nc : 0));
}

struct MarginThr { float t[MRG_MAXK]; };         // the slots >= K hold NaN: no margin passes them

__global__ __launch_bounds__(MRG_THREADS) void margin_kernel(const float* __restrict__ planes, const int* __restrict__ nchan,
                                                             const int* __restrict__ cls_idx, const unsigned char* __restrict__ gt, TileGeo geo,
                                                             int total_tiles, int Smax, int Cmax, float a, MarginThr th, int K,
                                                             const int* __restrict__ skip, int nc, unsigned long long* __restrict__ totals,
                                                             unsigned long long* __restrict__ kept, float label_thre,
                                                             unsigned char* __restrict__ lab8, float* __restrict__ margin_out) {
    extern __shared__ unsigned int lds[];                    // margin_lds_bytes(K, nc, totals, kept)
    const int rows = K + 1;
    unsigned int* Kc = lds;                                  // [K+1] pixels per bin
    unsigned int* G = Kc + rows;                             // [K+1][nc]
    unsigned int* P = G + rows * nc;                         // [K+1][nc]
    unsigned int* I = P + rows * nc;                         // [K+1][nc]
    const bool counting = totals || kept;
    if (counting) {
        const int words = rows + (totals ? 3 * rows * nc : 0);
        for (int i = threadIdx.x; i < words; i += MRG_THREADS) lds[i] = 0;
        __syncthreads();
    }
    const int lane256 = threadIdx.x & 255;                   // the thread's place in its tile: argmax_label_ragged_kernel's
    for (int tile = blockIdx.x * MRG_SUBS + (threadIdx.x >> 8); tile < total_tiles; tile += gridDim.x * MRG_SUBS) {
        const Tile t = tile_of_ragged(geo, tile);
        const int x = t.x0 + (lane256 & 63);
        if (x >= t.W) continue;                              // (no barrier inside the loop)
        const int nch = nchan ? min(nchan[t.b], Cmax) : Cmax;
        const int* cls_row = cls_idx ? cls_idx + (long long)t.b * Smax : nullptr;
        const float* cb = planes + (long long)Cmax * t.base;
        const bool count = counting && !(skip && skip[t.b] != 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = t.y0 + (lane256 >> 6) + 4 * r;
            if (y >= t.H) continue;
            const float* p = cb + (long long)y * t.Wp + x;
            int key = 0;
            float margin = __builtin_inff();                 // nch == 1: the background has no rival
            if (nch > 1) {
                const float v0 = __fmul_rn(a, p[0]);
                float F = p[t.HW];                           // the best foreground plane, the first that attains it ...
                float S = -__builtin_inff();                 // ... and the best of the others (read only when nch > 2)
                int ci = 1;
                bool bad = (v0 != v0) || (F != F);
                for (int c = 2; c < nch; ++c) {
                    const float v = p[(long long)c * t.HW];
                    bad |= (v != v);
                    if (v > F) { S = F; F = v; ci = c; }     // the first maximum wins, like argmax_key (par.hip)
                    else if (v > S) S = v;
                }
                const int key_fg = cls_row ? cls_row[ci - 1] + 1 : ci;
                if (v0 >= F || key_fg == 0) {                // background (a foreground slot that maps to key 0: background either way)
                    margin = __fsub_rn(v0, F);
                } else {
                    key = key_fg;
                    const float R = (nch > 2 && S > v0) ? S : v0;
                    margin = __fsub_rn(F, R);
                }
                if (bad) margin = __builtin_nanf("");        // a NaN plane: the pixel is kept nowhere
            }
            const long long pix = t.lab + (long long)y * t.W + x;
            if (margin_out) margin_out[pix] = margin;
            if (lab8) lab8[pix] = (unsigned char)(margin >= label_thre ? key : 255);
            if (!count) continue;
            int m = 0;
#pragma unroll
            for (int j = 0; j < MRG_MAXK; ++j) m += (margin >= th.t[j]) ? 1 : 0;
            atomicAdd(&Kc[m], 1u);                           // (K + 1 addresses; folding the lanes of a wave that share m: measured, not adopted)
            if (!totals || m == 0) continue;
            const int g = gt[pix];
            if (g >= nc || (unsigned)key >= (unsigned)nc) continue;   // (a key below 0 - a class slot below -1 - is in no row either)
            atomicAdd(&G[m * nc + g], 1u);
            atomicAdd(&P[m * nc + key], 1u);
            if (g == key) atomicAdd(&I[m * nc + g], 1u);
        }
    }
    if (!counting) return;
    __syncthreads();
    // ---- flush: threshold j holds the bins m > j - one suffix sum per counter
    if (kept && threadIdx.x == 0) {
        unsigned int s = 0;
        for (int j = K; j >= 1; --j) {
            s += Kc[j];
            if (s) atomicAdd(&kept[j - 1], (unsigned long long)s);
        }
        s += Kc[0];
        if (s) atomicAdd(&kept[K], (unsigned long long)s);
    }
    if (!totals) return;
    for (int i = threadIdx.x; i < 3 * nc; i += MRG_THREADS) {   // i = row * nc + class: G, P and I are laid out one after the other
        const unsigned int* bins = G + (i / nc) * rows * nc + (i % nc);
        unsigned int s = 0;
        for (int j = K - 1; j >= 0; --j) {
            s += bins[(j + 1) * nc];
            if (s) atomicAdd(&totals[(long long)j * 3 * nc + i], (unsigned long long)s);
        }
    }
}

extern "C" int excel_margin_sweep_ragged(const float* planes, const int32_t* nchan, const int32_t* cls_idx, const uint8_t* gt,
                                         const int32_t* table, const excel_ragged_info* info, int Smax, int Cmax, float bkg_scale,
                                         const float* thresholds, int K, const int32_t* skip, int num_classes, int64_t* totals, int64_t* kept,
                                         float label_thre, uint8_t* labels_u8, float* margin_out, void* stream) {
    EXCEL_CHECK_ARG(planes && table && info, "margin_sweep_ragged: null argument (planes, table and info are required)");
    EXCEL_CHECK_ARG(totals || kept || labels_u8 || margin_out, "margin_sweep_ragged: nothing to do (no totals, kept, labels_u8 or margin_out)");
    EXCEL_CHECK_ARG(!totals || gt, "margin_sweep_ragged: totals needs the ground truth (gt is null)");
    EXCEL_CHECK_ARG(K >= 0 && K <= MRG_MAXK, "margin_sweep_ragged: need 0 <= K <= %d (K = %d)", MRG_MAXK, K);
    EXCEL_CHECK_ARG(K >= 1 || !(totals || kept), "margin_sweep_ragged: totals and kept need at least one threshold (K = 0)");
    EXCEL_CHECK_ARG(K == 0 || thresholds, "margin_sweep_ragged: null thresholds");
    MarginThr th;
    for (int j = 0; j < MRG_MAXK; ++j) th.t[j] = __builtin_nanf("");
    for (int j = 0; j < K; ++j) {
        EXCEL_CHECK_ARG(thresholds[j] >= 0.f && thresholds[j] <= 3.402823466e38f,
                        "margin_sweep_ragged: threshold %d is %g: thresholds must be finite and >= 0", j, (double)thresholds[j]);
        EXCEL_CHECK_ARG(j == 0 || thresholds[j] > thresholds[j - 1], "margin_sweep_ragged: threshold %d is %g after %g: thresholds must be strictly increasing",
                        j, (double)thresholds[j], (double)thresholds[j - 1]);
        th.t[j] = thresholds[j];
    }
    EXCEL_CHECK_ARG(!labels_u8 || label_thre == label_thre, "margin_sweep_ragged: label_thre is NaN");
    EXCEL_CHECK_ARG(bkg_scale >= 0.f && bkg_scale <= 3.402823466e38f, "margin_sweep_ragged: bkg_scale is %g: it must be finite and >= 0", (double)bkg_scale);
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= MRG_MAXNC, "margin_sweep_ragged: need 1 <= num_classes <= %d (got %d)", MRG_MAXNC,
                    num_classes);
    EXCEL_CHECK_ARG(((uintptr_t)planes & 15) == 0, "margin_sweep_ragged: planes must be 16-byte aligned");
    EXCEL_CHECK_ARG((((uintptr_t)totals | (uintptr_t)kept) & 7) == 0, "margin_sweep_ragged: totals and kept must be 8-byte aligned");
    EXCEL_CHECK_ARG((((uintptr_t)margin_out | (uintptr_t)nchan | (uintptr_t)cls_idx | (uintptr_t)skip | (uintptr_t)table) & 3) == 0,
                    "margin_sweep_ragged: margin_out, nchan, cls_idx, skip and table must be 4-byte aligned");
    EXCEL_CHECK_ARG(Cmax >= 1 && (!cls_idx || Smax >= Cmax - 1), "margin_sweep_ragged: need Cmax >= 1 and, with cls_idx, Smax >= Cmax - 1 (Cmax = %d, Smax = %d)",
                    Cmax, Smax);
    EXCEL_CHECK_ARG(info->B >= 1 && info->total_tiles >= 1, "margin_sweep_ragged: the plan holds no tile");
    TileGeo geo;
    geo.tab = table; geo.B = info->B; geo.H = geo.W = 0;
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    const bool counting = totals || kept;
    const int want = cdiv(info->total_tiles, MRG_SUBS);
    const int groups = (counting && want > MRG_MAX_GROUPS) ? MRG_MAX_GROUPS : want;
    const size_t lds = margin_lds_bytes(K, num_classes, totals != nullptr, kept != nullptr);   // 52 292 B at most: under the 64 KB of a plain launch
    hipLaunchKernelGGL(margin_kernel, dim3((unsigned)groups), dim3(MRG_THREADS), lds, st, planes, nchan, cls_idx, gt, geo, info->total_tiles, Smax, Cmax,
                       bkg_scale, th, K, skip, num_classes, (unsigned long long*)totals, (unsigned long long*)kept, label_thre, labels_u8, margin_out);
    EXCEL_CHECK_LAUNCH("margin_sweep_ragged");
    return EXCEL_OK;
}
