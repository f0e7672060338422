// What the kernels over uint8 label maps share (confusion.hip, boundary.hip, components.hip, guard.hip): the streaming sweep over a pair
// of maps, the two kinds of LDS bins a pixel pair is counted into, and the host checks of their entries.
#pragma once
#include "../../include/excel_hip.h"
#include "common.h"

// ---------------------------------------------------------------- the sweep
// One contiguous range [0, n) of two label maps, cut over the gridDim.x workgroups of 256 lanes that share it (chunk = blockIdx.x):
// count(g, p) is called exactly once per pixel of the range.  gt / pred are slices of larger tensors and need not be 16-byte aligned:
// when both share their misalignment, chunk 0's first lanes take the (up to 15) pixels in front of the first 16-byte boundary and
// everything behind goes 16 pixels per lane and round - one 16-byte load per map where base + 16 <= n, pixel by pixel in the last,
// partial group; otherwise the whole range goes pixel by pixel.  Nothing outside [0, n) of either map is read.  gt, pred and n are
// wave-uniform, and so is everything derived from them here (scalar loads / SALU only).
template <class Count>
__device__ __forceinline__ void label_pair_sweep(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred, long long n,
                                                 Count count) {
    const int mg = (int)((16 - ((uintptr_t)gt & 15)) & 15), mp = (int)((16 - ((uintptr_t)pred & 15)) & 15);
    const int head = (mg == mp) ? mg : -1;                   // -1: no common alignment
    if (head > 0 && blockIdx.x == 0 && threadIdx.x < head && threadIdx.x < n) count((int)gt[threadIdx.x], (int)pred[threadIdx.x]);
    if (head >= 0) {
        gt += head; pred += head; n -= head;
        if (n < 0) n = 0;
    }
    const long long stride = (long long)gridDim.x * 256 * 16;
    for (long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * 16; base < n; base += stride) {
        if (head >= 0 && base + 16 <= n) {
            const uint4 g4 = *reinterpret_cast<const uint4*>(gt + base);
            const uint4 p4 = *reinterpret_cast<const uint4*>(pred + base);
            const unsigned int gw[4] = {g4.x, g4.y, g4.z, g4.w}, pw[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) count((int)((gw[k >> 2] >> (8 * (k & 3))) & 255), (int)((pw[k >> 2] >> (8 * (k & 3))) & 255));
        } else {
            const long long end = (base + 16 < n) ? base + 16 : n;
            for (long long j = base; j < end; ++j) count((int)gt[j], (int)pred[j]);
        }
    }
}

// The range of a workgroup of a launch over (chunk, image = blockIdx.y): tab == nullptr: uniform images of per_image pixels; else image
// b = [loff_b, loff_{b+1}) of the ragged plan.  The image index is a grid dimension so that the start, the misalignment and the skip
// flag are wave-uniform and a skipped image's workgroups leave before they touch LDS.  -> false: nothing to do (the image is skipped,
// or it has fewer chunks than the grid); else gt / pred point at the image and n is its pixel count.
__device__ __forceinline__ bool label_image_range(const int* __restrict__ tab, long long per_image, const int* __restrict__ skip,
                                                  const unsigned char* __restrict__& gt, const unsigned char* __restrict__& pred, long long& n) {
    const int b = blockIdx.y;
    if (skip && skip[b] != 0) return false;
    long long start;
    if (tab) {
        start = tab[EXCEL_RAG_REC * b + 4];
        n = (long long)tab[EXCEL_RAG_REC * (b + 1) + 4] - start;
    } else {
        start = (long long)b * per_image;
        n = per_image;
    }
    if (blockIdx.x > 0 && (long long)blockIdx.x * 256 * 16 >= n) return false;
    gt += start; pred += start;
    return true;
}

// ---------------------------------------------------------------- the bins
// A pixel pair counts when g < nc and p < nc.  Both kinds of bins are u32 counters private to the workgroup, in LDS, flushed once - the
// non-zero ones only.  A workgroup's share of a range cannot wrap them: its stride loop covers n / gridDim.x pixels, and 2^32 of them
// would need n > 2^43; the tile kernels count 1024 pixels.  So every count is integer-exact.
#define LABEL_MAXNC 256                          // raw values are bytes
#define LABEL_MAXBINS 8192                       // 32 KB of LDS: the whole [nc, nc] matrix up to nc = 90

__device__ __forceinline__ void label_bins_clear(unsigned int* lh, int bins) {
    for (int i = threadIdx.x; i < bins; i += 256) lh[i] = 0;
}

// The confusion matrix, lh[(g - r0) * nc + p] of LABEL_MAXBINS counters.  BAND (nc * nc > LABEL_MAXBINS): the matrix does not fit one
// workgroup's LDS, so `band` (a grid dimension) selects LABEL_MAXBINS / nc ground-truth rows; a workgroup reads the same pixels as its
// twins of the other bands and counts those whose gt lies in its own, so every pixel is counted by exactly one band.
// (The bins are functions of plain values, not members of an object that holds lh and nc: counted through such an object, the narrow
// kernel's byte-select operands come out as separate instructions - EXPERIMENTS.md, "One label-pair sweep".)
struct RowBand { int r0, rows; };
template <bool BAND>
__device__ __forceinline__ RowBand matrix_band(int nc, int band) {
    const int band_rows = BAND ? LABEL_MAXBINS / nc : nc;
    const int r0 = BAND ? band * band_rows : 0;
    return RowBand{r0, BAND ? min(band_rows, nc - r0) : nc};
}
template <bool BAND>
__device__ __forceinline__ void matrix_count(unsigned int* lh, int nc, RowBand b, int g, int p) {
    if (BAND) {
        const unsigned int gr = (unsigned int)(g - b.r0);
        if (gr < (unsigned int)b.rows && p < nc) atomicAdd(&lh[gr * nc + p], 1u);
    } else {
        if (g < nc && p < nc) atomicAdd(&lh[g * nc + p], 1u);
    }
}
template <bool BAND>
__device__ __forceinline__ void matrix_flush(const unsigned int* lh, int nc, RowBand b, unsigned long long* hist) {   // hist: the whole [nc, nc]
    for (int i = threadIdx.x; i < b.rows * nc; i += 256)
        if (lh[i]) atomicAdd(&hist[(BAND ? b.r0 * nc : 0) + i], (unsigned long long)lh[i]);
}

// The three margins of the matrix, 3 * nc counters: lh[g] row sums, lh[nc + p] column sums, lh[2 nc + g] the diagonal - 3 KB at most,
// whatever nc: no bands.  in_g / in_p restrict a pixel to the part of either map a caller scores (boundary.hip: the contour bands); the
// diagonal counts where both hold.
__device__ __forceinline__ void margin_count(unsigned int* lh, int nc, int g, int p, bool in_g = true, bool in_p = true) {
    if (g < nc && p < nc) {
        if (in_g) atomicAdd(&lh[g], 1u);
        if (in_p) atomicAdd(&lh[nc + p], 1u);
        if (g == p && in_g && in_p) atomicAdd(&lh[2 * nc + g], 1u);
    }
}
__device__ __forceinline__ void margin_flush(const unsigned int* lh, int nc, int* out) {   // out: the image's [3, nc] rows
    for (int i = threadIdx.x; i < 3 * nc; i += 256)
        if (lh[i]) atomicAdd(&out[i], (int)lh[i]);
}

// ---------------------------------------------------------------- host side of the entries
// `who` names the entry in every refusal.

static inline int clear_on_stream(const char* who, const char* what, void* p, size_t bytes, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    if (e != hipSuccess) {
        excel_set_error("%s: clearing the %s failed: %s", who, what, hipGetErrorString(e));
        return EXCEL_ERR_LAUNCH;
    }
    return EXCEL_OK;
}

// The images of a launch over (chunk, image): B uniform images of per_image pixels, or a plan's table plus info.  -> max_pix, the
// pixels of the largest image (ragged: H_b * Wp_b >= H_b * W_b - an upper bound is enough for the grid).
static inline int label_images(const char* who, int B, long long per_image, const int32_t* table, const excel_ragged_info* info,
                               long long* max_pix) {
    EXCEL_CHECK_ARG(B >= 1 && B <= 65535, "%s: need 1 <= B <= 65535 (B = %d)", who, B);
    if (table) {
        EXCEL_CHECK_ARG(info && info->B == B, "%s: the plan holds %d images, B = %d", who, info ? info->B : -1, B);
        *max_pix = info->max_plane_pix;
    } else {
        EXCEL_CHECK_ARG(per_image >= 1 && per_image < (1LL << 31), "%s: per_image must be in [1, 2^31) (got %lld)", who, per_image);
        *max_pix = per_image;
    }
    return EXCEL_OK;
}
// Chunks per image (gridDim.x of the sweep): one per 4096 pixels of the largest image, and at most 2048 / B - a bound on the workgroups
// that flush their bins.
static inline unsigned label_pair_chunks(long long max_pix, int B) {
    const long long want = cdivl(max_pix, 256 * 16);
    const long long cap = 2048 / B > 1 ? 2048 / B : 1;
    return (unsigned)(want < cap ? (want > 0 ? want : 1) : cap);
}

// Tight label maps on the 64 x 16 tiles of the ragged plan, uniform [B,H,W] or ragged: refusals first, then the grid of one workgroup
// per tile.  total (optional): the pixels of the whole batch, for entries that index them with 32 bits.
static inline int label_tile_geometry(const char* who, int B, int H, int W, const int32_t* table, const excel_ragged_info* info, TileGeo* geo,
                                      dim3* grid, long long* total) {
    EXCEL_CHECK_ARG(B >= 1 && B <= 65535, "%s: need 1 <= B <= 65535 (B = %d)", who, B);
    geo->tab = table; geo->B = B; geo->H = H; geo->W = W;
    if (table) {
        EXCEL_CHECK_ARG(info && info->B == B, "%s: the plan holds %d images, B = %d", who, info ? info->B : -1, B);
        EXCEL_CHECK_ARG(info->total_tiles >= 1, "%s: the plan holds no tile", who);
        if (total) {
            EXCEL_CHECK_ARG(info->total_label_pix >= 1 && info->total_label_pix < (1LL << 31),
                            "%s: the plan holds %lld pixels, outside [1, 2^31)", who, (long long)info->total_label_pix);
            *total = info->total_label_pix;
        }
        *grid = dim3((unsigned)info->total_tiles);
    } else {
        EXCEL_CHECK_ARG(H >= 1 && W >= 1, "%s: need H >= 1 and W >= 1 (got %d x %d)", who, H, W);
        EXCEL_CHECK_ARG((long long)H * W < (1LL << 31) && cdiv(H, 16) <= 65535, "%s: %d x %d is too large an image", who, H, W);
        if (total) *total = (long long)B * H * W;
        *grid = dim3((unsigned)cdiv(W, 64), (unsigned)cdiv(H, 16), (unsigned)B);
    }
    return EXCEL_OK;
}
