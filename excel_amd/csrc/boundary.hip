// Boundary scores (include/excel_hip.h, "boundary scores"): the counts Boundary IoU (Cheng et al., CVPR 2021) is computed from.
//
// image_scores_kernel (confusion.hip) counts every valid pixel; the kernel here counts only those in the BAND of their map - the pixels
// whose (2d+1) x (2d+1) window leaves the image or holds another raw value:
//
//   boundary_scores_kernel : counts[b,0,g] = valid pixels with ground truth g in the band of the ground truth
//                            counts[b,1,p] = valid pixels predicted p in the band of the prediction
//                            counts[b,2,g] = valid pixels with g == p in both bands
//                            valid = g < nc and p < nc; zero for an image with skip[b] != 0, -1 for an image whose radius is refused
//
// One workgroup per 64 x 16 tile (the tile map of the ragged plan, or grid (cdiv(W,64), cdiv(H,16), B)), d = the image's radius.  The
// two maps take turns in the same LDS:
//   stage   the tile plus a halo of d pixels, (16+2d) x (64+2d) bytes.  Tight ragged maps start anywhere and d is often odd, so every
//           staged row starts at the 4-byte boundary at or before its first pixel (s = 0..3 bytes earlier, per row): all loads in the
//           row's interior are aligned dwords, only a dword that straddles the image's edge is assembled from byte loads.  Positions
//           outside the image are never read - rows outside are not staged at all, columns outside are written as 0 and never
//           looked at.  The row pass puts the s bytes back with v_alignbyte;
//   rows    a window is uniform iff each of its row segments is uniform and its centre column is.  A lane walks 16 + 2d pixels of one
//           staged row with a run length (reset by a change of value and by a column outside the image); the segment [x-d, x+d] is
//           uniform iff the run that ends at x + d is at least 2d + 1 long.  It writes v(r,x) = the value, or 256 for "not uniform";
//   columns the same walk down v for a quarter of a tile column: the window of (y,x) is uniform iff the run of equal v < 256 that ends
//           at row y + d is at least 2d + 1 long.  The band flag and the centre value go to two 1 KB arrays per map.
// Cost per pixel is independent of d up to the halo; LDS is sized by max_radius (10 KB at 13, 55 KB at 72).  The count goes
// into image_scores_kernel's bins (margin_count, label_maps.h).  No workspace, no scratch.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"
#include "label_maps.h"

#define BND_TH 16
#define BND_TW 64
#define BND_MAXR 72                              // the largest halo whose LDS (55 KB + 7 KB static) stays under the 64 KB of a plain launch
#define BND_VP (BND_TW + 2)                      // pitch of v in u16: 33 dwords, so the lanes of the row pass (one row each) spread over the banks
#define BND_BAD 256

// pitch of the staged map in bytes for radius d: 64 + 2d plus the 3 bytes a row may start early, rounded up to a dword, then to an odd
// number of dwords (same reason)
__host__ __device__ __forceinline__ int bnd_pitch(int d) {
    int p = (BND_TW + 2 * d + 3 + 3) & ~3;
    if (((p >> 2) & 1) == 0) p += 4;
    return p;
}
__host__ __device__ __forceinline__ int bnd_map_bytes(int d) { return (BND_TH + 2 * d) * bnd_pitch(d); }
static inline size_t bnd_lds_bytes(int d) { return (size_t)bnd_map_bytes(d) + (size_t)(BND_TH + 2 * d) * BND_VP * 2; }

template <bool RAGGED>
__global__ __launch_bounds__(256) void boundary_scores_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                              TileGeo geo, const int* __restrict__ radius, int max_radius,
                                                              const int* __restrict__ skip, int nc, int* __restrict__ counts) {
    extern __shared__ unsigned int bnd_dyn[];                 // the staged map [RH][P] bytes, then v [RH][BND_VP] u16
    __shared__ unsigned int lh[3 * LABEL_MAXNC];
    __shared__ unsigned char edge[2][BND_TH * BND_TW], centre[2][BND_TH * BND_TW];
    const Tile t = tile_of<RAGGED>(geo);
    const int b = t.b;
    if (skip && skip[b] != 0) return;                        // the rows stay as the host entry cleared them
    const int bins = 3 * nc;
    const int d = radius ? radius[b] : max_radius;
    if (d < 1 || d > max_radius) {                           // refused: the image's first tile marks its rows, nobody counts
        if (t.x0 == 0 && t.y0 == 0)
            for (int i = threadIdx.x; i < bins; i += 256) counts[(long long)b * bins + i] = -1;
        return;
    }
    const int H = t.H, W = t.W;
    const int RH = BND_TH + 2 * d, P = bnd_pitch(d), P4 = P >> 2;
    const int ys = t.y0 - d, xs = t.x0 - d;                  // image position of the staged region's corner
    unsigned char* M = reinterpret_cast<unsigned char*>(bnd_dyn);
    unsigned short* V = reinterpret_cast<unsigned short*>(M + bnd_map_bytes(max_radius));
    label_bins_clear(lh, bins);

    for (int m = 0; m < 2; ++m) {
        const unsigned char* __restrict__ src = (m ? pred : gt) + t.lab;
        // bytes by which the staged row of image row y starts before column xs: its first byte is 4-byte aligned in memory
        auto early = [&](int y) { return (int)(((uintptr_t)src + (unsigned long long)((long long)y * W + xs)) & 3); };
        // ---- stage: 8 rows per turn, 32 lanes along a row, one aligned dword per lane
        for (int r = threadIdx.x >> 5; r < RH; r += 8) {
            const int y = ys + r;
            if (y < 0 || y >= H) continue;                   // never read: the row pass knows the row is outside
            const unsigned char* row = src + (long long)y * W;
            const int xa = xs - early(y);                    // image column of the staged row's byte 0
            for (int c4 = threadIdx.x & 31; c4 < P4; c4 += 32) {
                const int x = xa + 4 * c4;
                unsigned int w;
                if (x >= 0 && x + 3 < W) {
                    w = *reinterpret_cast<const unsigned int*>(row + x);
                } else {
                    w = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (x + k >= 0 && x + k < W) w |= (unsigned int)row[x + k] << (8 * k);
                }
                reinterpret_cast<unsigned int*>(M)[r * P4 + c4] = w;
            }
        }
        __syncthreads();
        // ---- rows: work item = (staged row, 16 output columns); it walks the 16 + 2d staged columns those need
        for (int u = threadIdx.x; u < RH * (BND_TW / 16); u += 256) {
            const int r = u >> 2, seg = u & 3;
            unsigned short* vrow = V + r * BND_VP + seg * 16;
            const int y = ys + r;
            if (y < 0 || y >= H) {
#pragma unroll
                for (int k = 0; k < 16; ++k) vrow[k] = BND_BAD;
                continue;
            }
            const unsigned int* mrow = reinterpret_cast<const unsigned int*>(M) + r * P4 + seg * 4;
            const int x_first = xs + seg * 16;               // image column of the walk's first pixel
            int run = 0, prev = -1;
            const int n = 16 + 2 * d;
            const unsigned int s = (unsigned int)early(y);
            unsigned int lo = mrow[0];
            for (int c = 0; c < n; c += 4) {
                const unsigned int hi = mrow[(c >> 2) + 1];   // < P4: the pitch holds 64 + 2d + 3 bytes
                const unsigned int w = __builtin_amdgcn_alignbyte(hi, lo, s);
                lo = hi;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cc = c + k, x = x_first + cc;
                    const int val = (w >> (8 * k)) & 255;
                    run = (x >= 0 && x < W) ? ((val == prev && run > 0) ? run + 1 : 1) : 0;
                    prev = val;
                    if (cc >= 2 * d && cc < n) vrow[cc - 2 * d] = run >= 2 * d + 1 ? (unsigned short)val : (unsigned short)BND_BAD;
                }
            }
        }
        __syncthreads();
        // ---- columns: work item = (tile column, 4 tile rows); it walks the 4 + 2d staged rows those need
        {
            const int x = threadIdx.x & 63, q = threadIdx.x >> 6;
            const unsigned short* vcol = V + (q * 4) * BND_VP + x;
            int run = 0, prev = -1;
            const int n = 4 + 2 * d;
            for (int r = 0; r < n; ++r) {
                const int v = vcol[r * BND_VP];
                run = v < BND_BAD ? ((v == prev && run > 0) ? run + 1 : 1) : 0;
                prev = v;
                if (r >= 2 * d) edge[m][(q * 4 + r - 2 * d) * BND_TW + x] = run >= 2 * d + 1 ? 0 : 1;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t.y0 + q * 4 + k < H) centre[m][(q * 4 + k) * BND_TW + x] = M[(q * 4 + k + d) * P + x + d + early(t.y0 + q * 4 + k)];
        }
        __syncthreads();                                     // the next map overwrites M and V
    }
    // ---- count: band pixels only
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k;
        const int ty = i >> 6, tx = i & 63;
        if (t.y0 + ty < H && t.x0 + tx < W) {                 // centre[] of a pixel outside the image was never staged
            margin_count(lh, nc, centre[0][i], centre[1][i], edge[0][i] != 0, edge[1][i] != 0);
        }
    }
    __syncthreads();
    margin_flush(lh, nc, counts + (long long)b * bins);
}

extern "C" int excel_boundary_max_radius(void) { return BND_MAXR; }

extern "C" int excel_boundary_scores(const uint8_t* gt, const uint8_t* pred, int B, int H, int W, const int32_t* table,
                                     const excel_ragged_info* info, const int32_t* radius, int max_radius, const int32_t* skip,
                                     int num_classes, int32_t* counts, void* stream) {
    EXCEL_CHECK_ARG(gt && pred && counts, "boundary_scores: null argument (gt, pred and counts are required)");
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= LABEL_MAXNC, "boundary_scores: need 1 <= num_classes <= %d (got %d)", LABEL_MAXNC,
                    num_classes);
    EXCEL_CHECK_ARG(max_radius >= 1 && max_radius <= BND_MAXR, "boundary_scores: need 1 <= max_radius <= %d (got %d)", BND_MAXR, max_radius);
    EXCEL_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)skip & 3) == 0 && ((uintptr_t)radius & 3) == 0,
                    "boundary_scores: counts, skip and radius must be 4-byte aligned");
    TileGeo geo;
    dim3 grid;
    TRY(label_tile_geometry("boundary_scores", B, H, W, table, info, &geo, &grid, nullptr));
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    TRY(clear_on_stream("boundary_scores", "counts", counts, sizeof(int32_t) * (size_t)B * 3 * (size_t)num_classes, st));
    const size_t lds = bnd_lds_bytes(max_radius);            // 55 040 B at 72: with the 7 KB of static arrays under the 64 KB of a plain launch
    if (table)
        hipLaunchKernelGGL(boundary_scores_kernel<true>, grid, dim3(256), lds, st, gt, pred, geo, radius, max_radius, skip, num_classes, counts);
    else
        hipLaunchKernelGGL(boundary_scores_kernel<false>, grid, dim3(256), lds, st, gt, pred, geo, radius, max_radius, skip, num_classes, counts);
    EXCEL_CHECK_LAUNCH("boundary_scores");
    return EXCEL_OK;
}
