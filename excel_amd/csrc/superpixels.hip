// Superpixel snapping of label maps (include/excel_hip.h, "superpixel snap"): an integer SLIC on a fixed grid (the gSLIC form) and the
// majority vote of a label map inside every superpixel.  Integers only: the result is canonical, it does not depend on tiling,
// scheduling or the order of any atomic (the only atomics add integers).
//
// THE WINDOW.  Grid step S, cells of S x S pixels, centre k = cy * gx + cx lives in cell (cx, cy).  A pixel of cell (px, py) only ever
// considers the centres of the cells (px - 1 .. px + 1, py - 1 .. py + 1), so the pixels of centre k all lie in the 3 x 3 cells around
// its own cell, the 3S x 3S WINDOW of k (cut at the image's border).  Everything per centre is therefore a gather over that window:
//
//   slic_init_kernel     a lane per centre: the initial position and the colour of the pixel there;
//   slic_assign_kernel   a lane per pixel (four rows of a 64 x 16 tile): the centres of the cells under the tile, plus one cell around,
//                        staged in LDS (at most 35 x 11 of them, at S = 2), then the up to nine candidates in ascending k, a strictly
//                        smaller D wins: the smallest D, the smallest k on a tie.  Reads centres, writes sp;
//   slic_update_kernel   a wave per centre: it scans the window of sp, sums x, y, r, g, b and the count of its own pixels (positions
//                        relative to the window's corner, so the sums are small), reduces by shuffles and writes the rounded means.
//                        Reads sp, writes centres;
//   snap_vote_kernel     a wave per centre: a 256-bin histogram in LDS of the voting labels of its pixels, the largest count and the
//                        smallest class that attains it, and where the superpixel is snapped a second scan that rewrites the voting
//                        pixels that differ (out was made a copy of labels on the stream before).
//
// A workgroup of four waves owns the centres whose cell's corner (cx S, cy S) lies in its 64 x 16 tile - every cell's corner is inside
// the image, so every centre has exactly one owner - and the image comes with the tile: no search over cent_off.  Where a tile owns
// fewer than four centres (S > 16: few centres, large windows) its four waves share each of them instead of three idling (SP_COOP).  A centre's owner alone
// writes that centre; a pixel of sp is written by the lane that owns it; a pixel of out is rewritten by the wave of its one centre.  So
// centres is the only intermediate, there is no workspace, no global atomic but the three counters, and no ping-pong: launches on one
// stream alternate  assign (centres -> sp)  and  update (sp -> centres).
//
// D < 2^31.  D = S^2 (dr^2 + dg^2 + db^2) + m^2 (dx^2 + dy^2), S <= 64, m <= 64.  Colours: 3 * 255^2 = 195075.  Positions: a centre
// stays inside its window (it is a rounded mean of pixels of the window, or its initial pixel), the window of a candidate reaches two
// cells beyond the pixel's own cell, so |dx|, |dy| < 3S and dx^2 + dy^2 < 18 S^2.  D <= 4096 * 195075 + 4096 * 18 * 4096 =
// 799 027 200 + 301 989 888 = 1 101 017 088 < 2^31.  The sums of a window: at most 9 S^2 = 36864 pixels, relative positions below 192,
// colours up to 255: below 9.5e6; a histogram count, times 1000 for the share, below 3.7e7.
//
// No workgroup waits for another one.  Every loop is bounded by the window (9 S^2 pixels), the centres of a tile (at most 256) or the
// iteration count.  A superpixel is not made connected here.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"
#include "label_maps.h"

#define SP_MIN_STEP 2
#define SP_MAX_STEP 64
#define SP_MAX_COMPACTNESS 64
#define SP_MAX_ITERS 16
#define SP_LDS_CX 35                             // cells under 64 columns at S = 2, loosely: ceil(63 / S) + 1, plus one on either side
#define SP_LDS_CY 11                             // likewise under 16 rows

// The grid of one image and what the caller said about it.  ok == false: cent_off does not hold gx * gy centres for this image inside
// [0, cent_total) - the image is refused (sp = -1, nothing else of it is read or written), never clamped.
struct SpGrid {
    int gx, gy;
    long long c0;                                // the image's first centre
    bool ok;
};
__device__ __forceinline__ SpGrid sp_grid(const Tile& t, const int* __restrict__ cent_off, int cent_total, int S) {
    SpGrid g;
    g.gx = (t.W + S - 1) / S;
    g.gy = (t.H + S - 1) / S;
    const long long c0 = cent_off[t.b], c1 = cent_off[t.b + 1];
    g.c0 = c0;
    g.ok = c0 >= 0 && c1 <= (long long)cent_total && c1 - c0 == (long long)g.gx * g.gy;
    return g;
}

// The centres a tile owns: the cells whose corner lies in it, cx in [xa, xa + nx), cy in [ya, ya + ny); nx * ny <= 256, or <= 0.
struct SpOwned { int xa, ya, nx, ny; };
__device__ __forceinline__ SpOwned sp_owned(const Tile& t, const SpGrid& g, int S) {
    SpOwned o;
    o.xa = (t.x0 + S - 1) / S;
    o.ya = (t.y0 + S - 1) / S;
    o.nx = min(g.gx - 1, (t.x0 + 63) / S) - o.xa + 1;
    o.ny = min(g.gy - 1, (t.y0 + 15) / S) - o.ya + 1;
    return o;
}

// The window of centre (cx, cy), cut at the border, and a lane's walk over it in raster order.
// A walk takes `stride` lanes: the 64 of one wave where a tile owns four centres or more (a centre per wave), all 256 of the workgroup
// where it owns fewer (S > 16: the windows are large and the centres few; the waves then share every centre - SP_COOP).
struct SpWindow { int x0, y0, w, h; };
#define SP_COOP(n) ((n) < 4)
__device__ __forceinline__ SpWindow sp_window(const Tile& t, int cx, int cy, int S) {
    SpWindow w;
    w.x0 = max(0, (cx - 1) * S);
    w.y0 = max(0, (cy - 1) * S);
    w.w = min(t.W, (cx + 2) * S) - w.x0;
    w.h = min(t.H, (cy + 2) * S) - w.y0;
    return w;
}
template <class Visit>
__device__ __forceinline__ void sp_window_walk(const SpWindow& w, int first, int stride, Visit visit) {   // visit(dx, dy): offsets inside the window
    const int n = w.w * w.h, sx = stride % w.w, sy = stride / w.w;
    int dx = first % w.w, dy = first / w.w;
    for (int j = first; j < n; j += stride) {
        visit(dx, dy);
        dx += sx; dy += sy;
        if (dx >= w.w) { dx -= w.w; ++dy; }
    }
}

// ---------------------------------------------------------------- 1. SLIC
template <bool RAGGED>
__global__ __launch_bounds__(256) void slic_init_kernel(const unsigned char* __restrict__ hwc, TileGeo geo, const int* __restrict__ cent_off,
                                                        int cent_total, int S, int* __restrict__ centres) {
    const Tile t = tile_of<RAGGED>(geo);
    const SpGrid g = sp_grid(t, cent_off, cent_total, S);
    if (!g.ok) return;
    const SpOwned o = sp_owned(t, g, S);
    const int i = threadIdx.x;
    if (o.nx <= 0 || o.ny <= 0 || i >= o.nx * o.ny) return;
    const int cy = o.ya + i / o.nx, cx = o.xa + i % o.nx;
    const int x = min(t.W - 1, cx * S + S / 2), y = min(t.H - 1, cy * S + S / 2);
    const unsigned char* __restrict__ p = hwc + 3 * (t.lab + (long long)y * t.W + x);
    int* __restrict__ c = centres + 5 * (g.c0 + (long long)cy * g.gx + cx);
    c[0] = x; c[1] = y; c[2] = p[0]; c[3] = p[1]; c[4] = p[2];
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void slic_assign_kernel(const unsigned char* __restrict__ hwc, TileGeo geo, const int* __restrict__ cent_off,
                                                          int cent_total, int S, int m2, const int* __restrict__ centres, int* __restrict__ sp) {
    __shared__ int lc[SP_LDS_CX * SP_LDS_CY * 5];
    const Tile t = tile_of<RAGGED>(geo);
    const int H = t.H, W = t.W;
    const SpGrid g = sp_grid(t, cent_off, cent_total, S);
    // the cells under the tile and one around
    const int xa = max(t.x0 / S - 1, 0), xb = min((min(t.x0 + 64, W) - 1) / S + 1, g.gx - 1);
    const int ya = max(t.y0 / S - 1, 0), yb = min((min(t.y0 + 16, H) - 1) / S + 1, g.gy - 1);
    const int nx = xb - xa + 1, ny = yb - ya + 1;
    if (g.ok) {
        for (int i = threadIdx.x; i < nx * ny * 5; i += 256) {
            const int c = i / 5, f = i - 5 * c, cy = ya + c / nx, cx = xa + c % nx;
            lc[i] = centres[5 * (g.c0 + (long long)cy * g.gx + cx) + f];
        }
    }
    __syncthreads();
    const int x = t.x0 + (threadIdx.x & 63);
    if (x >= W) return;
    const int px = x / S, S2 = S * S;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = t.y0 + (threadIdx.x >> 6) + 4 * r;
        if (y >= H) break;
        const long long pix = t.lab + (long long)y * W + x;
        if (!g.ok) {
            sp[pix] = -1;
            continue;
        }
        const unsigned char* __restrict__ p = hwc + 3 * pix;
        const int cr = p[0], cg = p[1], cb = p[2];
        const int py = y / S;
        int best = 0x7fffffff, bk = -1;
        for (int cy = max(py - 1, 0); cy <= min(py + 1, g.gy - 1); ++cy) {
            for (int cx = max(px - 1, 0); cx <= min(px + 1, g.gx - 1); ++cx) {     // ascending k: a tie keeps the smaller one
                const int* c = lc + 5 * ((cy - ya) * nx + (cx - xa));
                const int dx = x - c[0], dy = y - c[1], dr = cr - c[2], dg = cg - c[3], db = cb - c[4];
                const int D = S2 * (dr * dr + dg * dg + db * db) + m2 * (dx * dx + dy * dy);
                if (D < best) { best = D; bk = cy * g.gx + cx; }
            }
        }
        sp[pix] = bk;
    }
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void slic_update_kernel(const unsigned char* __restrict__ hwc, TileGeo geo, const int* __restrict__ cent_off,
                                                          int cent_total, int S, const int* __restrict__ sp, int* __restrict__ centres) {
    const Tile t = tile_of<RAGGED>(geo);
    const SpGrid g = sp_grid(t, cent_off, cent_total, S);
    if (!g.ok) return;
    const SpOwned o = sp_owned(t, g, S);
    if (o.nx <= 0 || o.ny <= 0) return;
    __shared__ int part[4][6];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = o.nx * o.ny;
    const bool coop = SP_COOP(n);                            // the same in every wave of the workgroup
    for (int i = coop ? 0 : wave; i < n; i += coop ? 1 : 4) {
        const int cy = o.ya + i / o.nx, cx = o.xa + i % o.nx, k = cy * g.gx + cx;
        const SpWindow w = sp_window(t, cx, cy, S);
        const int* __restrict__ wsp = sp + t.lab + (long long)w.y0 * t.W + w.x0;
        const unsigned char* __restrict__ wim = hwc + 3 * (t.lab + (long long)w.y0 * t.W + w.x0);
        int cnt = 0, sx = 0, sy = 0, sr = 0, sg = 0, sb = 0;
        sp_window_walk(w, coop ? (int)threadIdx.x : lane, coop ? 256 : 64, [&](int dx, int dy) {
            const long long q = (long long)dy * t.W + dx;
            if (wsp[q] == k) {
                const unsigned char* __restrict__ p = wim + 3 * q;
                ++cnt; sx += dx; sy += dy; sr += p[0]; sg += p[1]; sb += p[2];
            }
        });
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            cnt += __shfl_xor(cnt, s, 64);
            sx += __shfl_xor(sx, s, 64); sy += __shfl_xor(sy, s, 64);
            sr += __shfl_xor(sr, s, 64); sg += __shfl_xor(sg, s, 64); sb += __shfl_xor(sb, s, 64);
        }
        if (coop) {                                          // the four waves' sums through LDS, then thread 0 alone goes on
            if (lane == 0) {
                part[wave][0] = cnt; part[wave][1] = sx; part[wave][2] = sy; part[wave][3] = sr; part[wave][4] = sg; part[wave][5] = sb;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                cnt = part[0][0] + part[1][0] + part[2][0] + part[3][0]; sx = part[0][1] + part[1][1] + part[2][1] + part[3][1];
                sy = part[0][2] + part[1][2] + part[2][2] + part[3][2]; sr = part[0][3] + part[1][3] + part[2][3] + part[3][3];
                sg = part[0][4] + part[1][4] + part[2][4] + part[3][4]; sb = part[0][5] + part[1][5] + part[2][5] + part[3][5];
            }
            __syncthreads();                                 // part has been read: the next centre may overwrite it
        }
        if ((coop ? threadIdx.x : lane) == 0 && cnt > 0) {   // a centre without a pixel keeps its values
            int* __restrict__ c = centres + 5 * (g.c0 + k);
            // (2 (sum + cnt x0) + cnt) / (2 cnt) = x0 + (2 sum + cnt) / (2 cnt): everything is >= 0
            c[0] = w.x0 + (2 * sx + cnt) / (2 * cnt);
            c[1] = w.y0 + (2 * sy + cnt) / (2 * cnt);
            c[2] = (2 * sr + cnt) / (2 * cnt);
            c[3] = (2 * sg + cnt) / (2 * cnt);
            c[4] = (2 * sb + cnt) / (2 * cnt);
        }
    }
}

// ---------------------------------------------------------------- 2. the vote
// The four waves of a workgroup take the tile's centres four at a time, every wave through the same number of turns (a wave without a
// centre in the last turn idles through it), so the barriers between clearing, counting and reading a histogram are workgroup barriers.
// A tile with fewer than four centres gives each of them all four waves and one histogram (SP_COOP).
template <bool RAGGED>
__global__ __launch_bounds__(256) void snap_vote_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ sp, TileGeo geo,
                                                        const int* __restrict__ cent_off, int cent_total, int S, int nc, int share_pm,
                                                        unsigned char* __restrict__ out, int* __restrict__ counts) {
    __shared__ unsigned int hist[4][256];
    __shared__ int sums[3];
    const Tile t = tile_of<RAGGED>(geo);
    const SpGrid g = sp_grid(t, cent_off, cent_total, S);
    if (!g.ok) return;                                       // wave-uniform and the same in every wave: nobody is left at a barrier
    const SpOwned o = sp_owned(t, g, S);
    if (o.nx <= 0 || o.ny <= 0) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = o.nx * o.ny;
    if (threadIdx.x < 3) sums[threadIdx.x] = 0;
    int n_vote = 0, n_snap = 0, n_changed = 0;
    const bool coop = SP_COOP(n);                            // the same in every wave: all four then share one centre and hist[0]
    unsigned int* __restrict__ h = hist[coop ? 0 : wave];
    const int first = coop ? (int)threadIdx.x : lane, stride = coop ? 256 : 64;
    for (int i0 = 0; i0 < n; i0 += coop ? 1 : 4) {
        const int i = coop ? i0 : i0 + wave;
        const bool active = i < n;
        const int cy = o.ya + (active ? i / o.nx : 0), cx = o.xa + (active ? i % o.nx : 0), k = cy * g.gx + cx;
        const SpWindow w = sp_window(t, cx, cy, S);
        const long long corner = t.lab + (long long)w.y0 * t.W + w.x0;
#pragma unroll
        for (int j = 0; j < 4; ++j) h[lane + 64 * j] = 0;
        __syncthreads();
        if (active) {
            sp_window_walk(w, first, stride, [&](int dx, int dy) {
                const long long q = corner + (long long)dy * t.W + dx;
                if (sp[q] == k) {
                    const int v = labels[q];
                    if (v < nc) atomicAdd(&h[v], 1u);
                }
            });
        }
        __syncthreads();
        // the largest count, the smallest class among equals: the largest (count << 8 | 255 - class)
        unsigned int key = 0;
        int tot = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = lane + 64 * j;
            const unsigned int c = h[v];
            tot += (int)c;
            if (c) key = max(key, (c << 8) | (unsigned int)(255 - v));
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            key = max(key, (unsigned int)__shfl_xor((int)key, s, 64));
            tot += __shfl_xor(tot, s, 64);
        }
        const int top = (int)(key >> 8), win = 255 - (int)(key & 255);
        const bool snapped = active && tot > 0 && 1000 * top >= share_pm * tot;
        const bool counts_it = !coop || wave == 0;           // every wave of a shared centre knows the outcome, one reports it
        if (active && tot > 0 && counts_it) ++n_vote;
        if (snapped) {
            if (counts_it) ++n_snap;
            if (top < tot) {                                 // else every voting pixel already holds win
                sp_window_walk(w, first, stride, [&](int dx, int dy) {
                    const long long q = corner + (long long)dy * t.W + dx;
                    if (sp[q] == k) {
                        const int v = labels[q];
                        if (v < nc && v != win) {
                            out[q] = (unsigned char)win;
                            ++n_changed;
                        }
                    }
                });
            }
        }
        __syncthreads();                                     // the histogram has been read: the next turn may clear it
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) n_changed += __shfl_xor(n_changed, s, 64);
    if (lane == 0) {                                         // n_vote and n_snap are wave-uniform
        if (n_vote) atomicAdd(&sums[0], n_vote);
        if (n_snap) atomicAdd(&sums[1], n_snap);
        if (n_changed) atomicAdd(&sums[2], n_changed);
    }
    __syncthreads();
    if (threadIdx.x < 3 && sums[threadIdx.x]) atomicAdd(&counts[3 * t.b + threadIdx.x], sums[threadIdx.x]);
}

// ---------------------------------------------------------------- host entries
static inline bool sp_overlap(const void* a, size_t na, const void* b, size_t nb) {
    return !((uintptr_t)a + na <= (uintptr_t)b || (uintptr_t)b + nb <= (uintptr_t)a);
}

static int sp_common_checks(const char* who, const void* cent_off, long long cent_total, int step) {
    EXCEL_CHECK_ARG(cent_off, "%s: null cent_off", who);
    EXCEL_CHECK_ARG(((uintptr_t)cent_off & 3) == 0, "%s: cent_off must be 4-byte aligned", who);
    EXCEL_CHECK_ARG(step >= SP_MIN_STEP && step <= SP_MAX_STEP, "%s: need %d <= step <= %d (got %d)", who, SP_MIN_STEP, SP_MAX_STEP, step);
    EXCEL_CHECK_ARG(cent_total >= 1 && cent_total < (1LL << 31), "%s: %lld centres in all, outside [1, 2^31)", who, cent_total);
    return EXCEL_OK;
}

extern "C" int excel_slic_superpixels(const uint8_t* hwc, int B, int H, int W, const int32_t* table, const excel_ragged_info* info,
                                      const int32_t* cent_off, long long cent_total, int step, int compactness, int iters, int32_t* sp,
                                      int32_t* centres, void* stream) {
    EXCEL_CHECK_ARG(hwc && sp && centres, "slic_superpixels: null argument (hwc, sp and centres are required)");
    TRY(sp_common_checks("slic_superpixels", cent_off, cent_total, step));
    EXCEL_CHECK_ARG(compactness >= 1 && compactness <= SP_MAX_COMPACTNESS, "slic_superpixels: need 1 <= compactness <= %d (got %d)",
                    SP_MAX_COMPACTNESS, compactness);
    EXCEL_CHECK_ARG(iters >= 0 && iters <= SP_MAX_ITERS, "slic_superpixels: need 0 <= iters <= %d (got %d)", SP_MAX_ITERS, iters);
    EXCEL_CHECK_ARG(((uintptr_t)sp & 3) == 0 && ((uintptr_t)centres & 3) == 0 && ((uintptr_t)table & 3) == 0,
                    "slic_superpixels: sp, centres and table must be 4-byte aligned");
    TileGeo geo;
    dim3 grid;
    long long total;
    TRY(label_tile_geometry("slic_superpixels", B, H, W, table, info, &geo, &grid, &total));
    EXCEL_CHECK_ARG(total >= 1 && total < (1LL << 31), "slic_superpixels: %lld pixels in all, outside [1, 2^31)", total);
    EXCEL_CHECK_ARG(cent_total <= total, "slic_superpixels: %lld centres for %lld pixels", cent_total, total);
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    const int m2 = compactness * compactness;
#define SP_LAUNCH(R)                                                                                                                     \
    do {                                                                                                                                 \
        hipLaunchKernelGGL(slic_init_kernel<R>, grid, dim3(256), 0, st, hwc, geo, cent_off, (int)cent_total, step, centres);             \
        for (int it = 0; it <= iters; ++it) {                                                                                            \
            hipLaunchKernelGGL(slic_assign_kernel<R>, grid, dim3(256), 0, st, hwc, geo, cent_off, (int)cent_total, step, m2, centres, sp); \
            if (it < iters)                                                                                                              \
                hipLaunchKernelGGL(slic_update_kernel<R>, grid, dim3(256), 0, st, hwc, geo, cent_off, (int)cent_total, step, sp, centres); \
        }                                                                                                                                \
    } while (0)
    if (table) SP_LAUNCH(true); else SP_LAUNCH(false);
#undef SP_LAUNCH
    EXCEL_CHECK_LAUNCH("slic_superpixels");
    return EXCEL_OK;
}

extern "C" int excel_snap_labels_to_superpixels(const uint8_t* labels, const int32_t* sp, int B, int H, int W, const int32_t* table,
                                                const excel_ragged_info* info, const int32_t* cent_off, long long cent_total, int step,
                                                int num_classes, int min_share_pm, uint8_t* out, int32_t* counts, void* stream) {
    EXCEL_CHECK_ARG(labels && sp && out && counts, "snap_labels_to_superpixels: null argument (labels, sp, out and counts are required)");
    TRY(sp_common_checks("snap_labels_to_superpixels", cent_off, cent_total, step));
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= 255, "snap_labels_to_superpixels: need 1 <= num_classes <= 255 (got %d): 255 never votes",
                    num_classes);
    EXCEL_CHECK_ARG(min_share_pm >= 0 && min_share_pm <= 1000, "snap_labels_to_superpixels: need 0 <= min_share_pm <= 1000 (got %d)", min_share_pm);
    EXCEL_CHECK_ARG(((uintptr_t)sp & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)table & 3) == 0,
                    "snap_labels_to_superpixels: sp, counts and table must be 4-byte aligned");
    TileGeo geo;
    dim3 grid;
    long long total;
    TRY(label_tile_geometry("snap_labels_to_superpixels", B, H, W, table, info, &geo, &grid, &total));
    EXCEL_CHECK_ARG(total >= 1 && total < (1LL << 31), "snap_labels_to_superpixels: %lld pixels in all, outside [1, 2^31)", total);
    EXCEL_CHECK_ARG(cent_total <= total, "snap_labels_to_superpixels: %lld centres for %lld pixels", cent_total, total);
    EXCEL_CHECK_ARG(!sp_overlap(out, (size_t)total, labels, (size_t)total),
                    "snap_labels_to_superpixels: out overlaps labels (the snap does not run in place)");
    EXCEL_CHECK_ARG(!sp_overlap(out, (size_t)total, sp, 4 * (size_t)total), "snap_labels_to_superpixels: out overlaps sp");
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    TRY(clear_on_stream("snap_labels_to_superpixels", "counts", counts, sizeof(int32_t) * (size_t)B * 3, st));
    const hipError_t e = hipMemcpyAsync(out, labels, (size_t)total, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
        excel_set_error("snap_labels_to_superpixels: copying labels to out failed: %s", hipGetErrorString(e));
        return EXCEL_ERR_LAUNCH;
    }
    if (table)
        hipLaunchKernelGGL(snap_vote_kernel<true>, grid, dim3(256), 0, st, labels, sp, geo, cent_off, (int)cent_total, step, num_classes,
                           min_share_pm, out, counts);
    else
        hipLaunchKernelGGL(snap_vote_kernel<false>, grid, dim3(256), 0, st, labels, sp, geo, cent_off, (int)cent_total, step, num_classes,
                           min_share_pm, out, counts);
    EXCEL_CHECK_LAUNCH("snap_labels_to_superpixels");
    return EXCEL_OK;
}
