// Nearest-label fill of label maps (include/excel_hip.h, "nearest-label fill"): every hole (a 255 pixel, where the mask allows it) takes
// the value of the nearest seed (a pixel with a class value) of its own image, by exact squared Euclidean distance; ties go to the
// first seed in raster order.  Integers only: the result is canonical.
//
// The distance separates: for a hole (y, x) and a seed (y', x'),  d2 = (x - x')^2 + (y - y')^2,  so among the seeds of ONE column x' only
// the one nearest in y can win - for every other seed of that column d2 is larger at the same x', or equal with a larger y' (the column
// pass breaks its tie towards the smaller y', which is also the raster order).  Two launches:
//
//   fill_col_kernel   one wave per 64 x 16 tile, one thread per column of it (neighbouring threads read neighbouring bytes): a walk down
//                     its 16 rows leaves the row of the last seed at or above every pixel, the walk back up compares it with the first
//                     seed at or below and keeps the nearer one, the upper one on a tie; the last seed above the tile and the first
//                     one below it the thread finds itself.  cand = dist2[y, x] = that row y', or -1;
//   fill_row_kernel   one workgroup per image row at a time: it stages the row's candidates into LDS, and every hole then looks outward
//                     over dx = 0, 1, 2, ... on both sides for the smallest key (d2, y', x'), d2 = dx^2 + (y - cand)^2.  It stops once
//                     dx^2 exceeds the best d2 so far (no farther column can be nearer) or max_dist2, or both sides have left the
//                     row.  It writes out, the final dist2 and the counts.
//
// dist2 IS THE ONLY INTERMEDIATE, and that is safe: the column pass writes every element of it and ends before the row pass starts (two
// launches on one stream); a workgroup of the row pass reads dist2 only in the row it is working on, and no other workgroup ever touches
// that row.  Inside the row, element x is read once, by the thread that owns x, on its way into LDS; that thread alone writes the final
// value of x, after its own read - at once where x is no hole, behind the barrier that follows the staging where it is one.  The
// searches read LDS, not dist2.  So no value is overwritten before its only reader has read it, and there is no workspace.
//
// No workgroup waits for another one; every loop is bounded by the height (column pass) or the width (row pass) of the image.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"
#include "label_maps.h"

#define FILL_MAX_SIDE 8192                       // d2 <= 2 * 8191^2 < 2^28; a row of 16-bit candidates is 16 KB of LDS
#define FILL_ROW_THREADS 256
#define FILL_COL_UNROLL 8                        // rows per direction and turn of the column pass's look outside its tile

// an image beyond FILL_MAX_SIDE in a ragged batch (the host cannot see the device table): refused by the kernels, never clamped
__device__ __forceinline__ bool fill_refused(int H, int W) { return H > FILL_MAX_SIDE || W > FILL_MAX_SIDE; }

// ---------------------------------------------------------------- 1. the nearest seed of every column
// One wave per 64 x 16 tile, one thread per column of the tile (neighbouring threads read neighbouring bytes).  A thread holds its 16
// rows in registers and needs two things from outside the tile: the last seed of its column above the tile and the first one below.
// It looks for them itself, 8 rows per direction and turn, and stops at the first hit - in a label map with a few holes that is the
// first turn; in a column without a seed it is the whole column, the bound of the loop.  So no tile depends on another one: no walk
// down the whole image (a chain of H dependent steps per column, and as many idle lanes as the image has tile rows), no LDS, no barrier.
// Then the walk down the 16 rows (the last seed at or above) and back up (the first seed at or below) runs in registers.
template <bool RAGGED>
__global__ __launch_bounds__(64) void fill_col_kernel(const unsigned char* __restrict__ labels, TileGeo geo, int nc, int* __restrict__ cand) {
    const Tile t = tile_of<RAGGED>(geo);
    const int H = t.H, W = t.W;
    const int x = t.x0 + threadIdx.x;
    if (x >= W || fill_refused(H, W)) return;
    const unsigned char* __restrict__ lab = labels + t.lab + x;
    int* __restrict__ c = cand + t.lab + x;
    const int y0 = t.y0, y1 = min(t.y0 + 16, H);
    int v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = y0 + k < y1 ? (int)lab[(long long)(y0 + k) * W] : 255;
    int last = -1, next = -1;                                // the last seed above the tile, the first one below
    for (int ua = y0 - 1, da = y1; (last < 0 && ua >= 0) || (next < 0 && da < H); ua -= FILL_COL_UNROLL, da += FILL_COL_UNROLL) {
        int u[FILL_COL_UNROLL], w[FILL_COL_UNROLL];
#pragma unroll
        for (int k = 0; k < FILL_COL_UNROLL; ++k) {
            u[k] = (last < 0 && ua - k >= 0) ? (int)lab[(long long)(ua - k) * W] : 255;
            w[k] = (next < 0 && da + k < H) ? (int)lab[(long long)(da + k) * W] : 255;
        }
#pragma unroll
        for (int k = FILL_COL_UNROLL - 1; k >= 0; --k) {     // k = 0 is the row next to the tile: it is assigned last and wins
            if (u[k] < nc) last = ua - k;                    // (a row that was not read holds 255 here, and nc <= 255)
            if (w[k] < nc) next = da + k;
        }
    }
    int up[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {                           // down: the last seed at or above y
        if (v[k] < nc) last = y0 + k;
        up[k] = last;
    }
#pragma unroll
    for (int k = 15; k >= 0; --k) {                          // up: the first seed at or below y
        const int y = y0 + k;
        if (v[k] < nc) next = y;
        // up[k] <= y <= next where they exist; the upper seed keeps a tie (the smaller y')
        const int pick = next < 0 ? up[k] : (up[k] < 0 ? next : (y - up[k] <= next - y ? up[k] : next));
        if (y < y1) c[(long long)y * W] = pick;
    }
}

// ---------------------------------------------------------------- 2. the nearest seed of every hole
// One workgroup per 64 x 16 tile again, but a workgroup works on whole ROWS: the tiles of one tile row share its 16 rows among them -
// tile column tx takes the rows tx, tx + ntx, ... of the 16 (two rows each at a width of 500; a tile column beyond the 16th has none) -
// so every workgroup of the launch has work and a row has exactly one workgroup.  Per row, a thread owns the pixels x = lane,
// lane + 256, ... (at most 32 of them at the largest width).  First sweep: it moves its candidates from dist2 to LDS, and writes out /
// dist2 of every pixel that is no hole at once - dist2[x] has exactly one reader, this thread, and the read has just happened; its holes
// it notes in a 32-bit mask.  Behind the barrier it runs the search for those.
template <bool RAGGED>
__global__ __launch_bounds__(FILL_ROW_THREADS) void fill_row_kernel(const unsigned char* __restrict__ labels, const unsigned char* __restrict__ mask,
                                                                    TileGeo geo, int nc, int max_dist2, unsigned char* __restrict__ out,
                                                                    int* dist2, int* __restrict__ counts) {
    __shared__ short cand[FILL_MAX_SIDE];                    // -1 .. 8191
    __shared__ int sums[3];
    const Tile t = tile_of<RAGGED>(geo);
    const int H = t.H, W = t.W;
    const int ntx = (W + 63) >> 6, tx = t.x0 >> 6;
    if (tx >= 16) return;
    const bool refused = fill_refused(H, W);                 // the map is copied, the image's first tile marks its counts row
    if (refused && t.x0 == 0 && t.y0 == 0 && threadIdx.x < 3) counts[3 * t.b + threadIdx.x] = -1;
    const unsigned char* __restrict__ img = labels + t.lab;
    if (threadIdx.x < 3) sums[threadIdx.x] = 0;
    int n_hole = 0, n_fill = 0, d_max = 0;
    for (int y = t.y0 + tx; y < min(t.y0 + 16, H); y += ntx) {
        const long long off = t.lab + (long long)y * W;
        const unsigned char* __restrict__ lab = labels + off;
        const unsigned char* __restrict__ msk = mask ? mask + off : nullptr;
        unsigned char* __restrict__ o = out + off;
        int* d = dist2 + off;
        __syncthreads();                                     // the searches of the previous row are over: cand may be overwritten
        unsigned holes = 0;
        int has = 0, it = 0;
        for (int x = threadIdx.x; x < W; x += FILL_ROW_THREADS, ++it) {
            const int c = refused ? -1 : d[x];
            const int v = lab[x];
            const int m = msk ? (int)msk[x] : 0;
            if (!refused) cand[x] = (short)c;
            has |= c >= 0;
            if (v == 255 && m != 255 && !refused) {
                holes |= 1u << it;                           // W <= 8192: it < 32
            } else {
                o[x] = (unsigned char)v;
                d[x] = v < nc ? 0 : -1;
            }
        }
        const int any = __syncthreads_or(has);               // every read of this row of dist2 lies before this barrier
        while (holes) {
            const int x = threadIdx.x + FILL_ROW_THREADS * (__ffs(holes) - 1);
            holes &= holes - 1;
            ++n_hole;
            unsigned long long best = ~0ull;                 // (d2 << 26) | (y' << 13) | x'
            int bd = max_dist2;                              // nothing beyond it is taken; shrinks to the best d2
            if (any) {
                for (int dx = 0;; ++dx) {
                    const int xl = x - dx, xr = x + dx, dx2 = dx * dx;
                    if ((xl < 0 && xr >= W) || dx2 > bd) break;
                    if (xl >= 0) {
                        const int c = cand[xl];
                        const int dy = y - c, d2 = dx2 + dy * dy;
                        if (c >= 0 && d2 <= bd) {
                            const unsigned long long key = ((unsigned long long)d2 << 26) | ((unsigned long long)c << 13) | (unsigned)xl;
                            if (key < best) { best = key; bd = d2; }
                        }
                    }
                    if (dx && xr < W) {
                        const int c = cand[xr];
                        const int dy = y - c, d2 = dx2 + dy * dy;
                        if (c >= 0 && d2 <= bd) {
                            const unsigned long long key = ((unsigned long long)d2 << 26) | ((unsigned long long)c << 13) | (unsigned)xr;
                            if (key < best) { best = key; bd = d2; }
                        }
                    }
                }
            }
            int value = 255, dd = -1;
            if (best != ~0ull) {
                const int qy = (int)(best >> 13) & (FILL_MAX_SIDE - 1), qx = (int)best & (FILL_MAX_SIDE - 1);
                value = img[qy * W + qx];
                dd = bd;
                ++n_fill;
                d_max = max(d_max, bd);
            }
            o[x] = (unsigned char)value;
            d[x] = dd;
        }
    }
    // one LDS atomic per wave and field, one global atomic per workgroup and field; a workgroup without a hole issues none
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        n_hole += __shfl_xor(n_hole, s, 64);
        n_fill += __shfl_xor(n_fill, s, 64);
        d_max = max(d_max, __shfl_xor(d_max, s, 64));
    }
    __syncthreads();                                         // (a workgroup without a row has not passed a barrier since sums was cleared)
    if ((threadIdx.x & 63) == 0) {
        if (n_hole) atomicAdd(&sums[0], n_hole);
        if (n_fill) atomicAdd(&sums[1], n_fill);
        if (d_max) atomicMax(&sums[2], d_max);
    }
    __syncthreads();
    if (threadIdx.x < 2 && sums[threadIdx.x]) atomicAdd(&counts[3 * t.b + threadIdx.x], sums[threadIdx.x]);
    if (threadIdx.x == 2 && sums[2]) atomicMax(&counts[3 * t.b + 2], sums[2]);
}

// ---------------------------------------------------------------- host entry
static inline bool fill_overlap(const void* a, const void* b, size_t n) {
    return b && !((uintptr_t)a + n <= (uintptr_t)b || (uintptr_t)b + n <= (uintptr_t)a);
}

extern "C" int excel_fill_nearest_label(const uint8_t* labels, const uint8_t* mask, int B, int H, int W, const int32_t* table,
                                        const excel_ragged_info* info, int num_classes, int max_dist2, uint8_t* out, int32_t* dist2,
                                        int32_t* counts, void* stream) {
    EXCEL_CHECK_ARG(labels && out && dist2 && counts, "fill_nearest_label: null argument (labels, out, dist2 and counts are required)");
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= 255, "fill_nearest_label: need 1 <= num_classes <= 255 (got %d): 255 is the hole",
                    num_classes);
    EXCEL_CHECK_ARG(max_dist2 >= 1, "fill_nearest_label: need max_dist2 >= 1 (got %d)", max_dist2);
    EXCEL_CHECK_ARG(((uintptr_t)dist2 & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)table & 3) == 0,
                    "fill_nearest_label: dist2, counts and table must be 4-byte aligned");
    TileGeo geo;
    dim3 grid;
    long long total;
    TRY(label_tile_geometry("fill_nearest_label", B, H, W, table, info, &geo, &grid, &total));
    EXCEL_CHECK_ARG(total >= 1 && total < (1LL << 31), "fill_nearest_label: %lld pixels in all, outside [1, 2^31)", total);
    EXCEL_CHECK_ARG(table || (H <= FILL_MAX_SIDE && W <= FILL_MAX_SIDE), "fill_nearest_label: %d x %d is beyond %d pixels a side", H, W,
                    FILL_MAX_SIDE);
    EXCEL_CHECK_ARG(!fill_overlap(out, labels, (size_t)total), "fill_nearest_label: out overlaps labels (the fill does not run in place)");
    EXCEL_CHECK_ARG(!fill_overlap(out, mask, (size_t)total), "fill_nearest_label: out overlaps mask");
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    TRY(clear_on_stream("fill_nearest_label", "counts", counts, sizeof(int32_t) * (size_t)B * 3, st));
    if (table) {
        hipLaunchKernelGGL(fill_col_kernel<true>, grid, dim3(64), 0, st, labels, geo, num_classes, dist2);
        hipLaunchKernelGGL(fill_row_kernel<true>, grid, dim3(FILL_ROW_THREADS), 0, st, labels, mask, geo, num_classes, max_dist2, out, dist2, counts);
    } else {
        hipLaunchKernelGGL(fill_col_kernel<false>, grid, dim3(64), 0, st, labels, geo, num_classes, dist2);
        hipLaunchKernelGGL(fill_row_kernel<false>, grid, dim3(FILL_ROW_THREADS), 0, st, labels, mask, geo, num_classes, max_dist2, out, dist2, counts);
    }
    EXCEL_CHECK_LAUNCH("fill_nearest_label");
    return EXCEL_OK;
}
