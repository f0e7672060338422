// Connected components of label maps (include/excel_hip.h, "connected components") and the small-region filter built on them.
//
// Two pixels of one image are connected when they are 4- or 8-neighbours and hold the same raw value.  comp[i] = the image-local index
// y * W + x of the first pixel, in raster order, of i's component; area[i] = the pixel count of that component.  Block-based union-find
// (Komura 2015; Playne & Hawick 2018) over the 64 x 16 tiles every ragged kernel of the library uses, as SEPARATE launches - no
// workgroup ever waits for another one:
//
//   cc_tile_kernel      one workgroup per tile: the tile's pieces, labelled in LDS.  Row runs come from one ballot per row, so only
//                       the first pixel of a contact between two runs issues a union.  comp[i] = the image-local index of the
//                       smallest pixel of i's piece;
//   cc_merge_kernel     the seams: every tile joins its top row to the row above and its left column to the column on its left; with
//                       8-connectivity the diagonal pairs as well, those through the tile corners included (the top seam reaches one
//                       column into both neighbouring tiles);
//   cc_flatten_kernel   comp[i] = find(i), and the areas: runs of equal parents are counted by ballot inside a wave, summed per piece
//                       in LDS, and added to area[root] with one atomic per piece and tile (areas were cleared on the stream);
//   cc_broadcast_kernel area[i] = area[comp[i]]: root slots are only read, all other slots only written.
//
// THE INVARIANT that bounds every loop here: every value ever stored in comp[] (and in the LDS labels of cc_tile_kernel) satisfies
// parent <= child - a pixel starts as its own parent, and the only later writes are atomicMin with a value below the slot's index (the
// larger root goes under the smaller one; path compression stores an ancestor).  find() therefore walks strictly downhill and ends
// after at most `index` steps whatever the other workgroups do meanwhile; it also stops at any value that is not below the slot it
// was read from, so even a map this library never wrote cannot make it loop or leave the image.  unite() lowers max(a, b) with every
// turn.  Nothing spins on another workgroup's progress.
//
// A link that atomicMin replaces is not lost: the atomic returns the parent it replaced, and unite() goes on joining THAT parent to
// the new one.  So a read that is stale (another XCD's L2) only costs another turn - the decision is always the atomic's.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"
#include "label_maps.h"

#define CC_TH 16
#define CC_TW 64
#define CC_SP (CC_TW + 2)                        // pitch of the staged values: one marker column on either side
#define CC_OUT 0x100                             // "no pixel": differs from every raw value

// ---------------------------------------------------------------- union-find in LDS (one tile)
__device__ __forceinline__ int lds_find(int* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((unsigned)p >= (unsigned)x) return x;            // a root (p == x); the invariant admits nothing else here
        x = p;
    }
}
__device__ __forceinline__ void lds_unite(int* L, int a, int b) {
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }        // a > b: the larger root goes under the smaller
        const int old = atomicMin(&L[a], b);
        if (old == a) return;                                // a was still a root: linked
        a = old;                                             // a had a parent already (whichever of old, b stays stored): join it to b
    }
}

// ---------------------------------------------------------------- union-find in global memory (one image: c = comp + loff_b)
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int* c, int x) {
    for (;;) {
        const int p = g_load(c + x);
        if ((unsigned)p >= (unsigned)x) return x;            // root, or a value the invariant excludes: stop, never climb or leave
        x = p;
    }
}
// find, then hang every pixel on the way below `x` itself directly under the root (x keeps pointing at its piece's root)
__device__ __forceinline__ int g_find_compress(int* c, int x) {
    const int r = g_find(c, x);
    int y = g_load(c + x);
    while ((unsigned)y < (unsigned)x && y > r) {
        const int p = g_load(c + y);
        atomicMin(c + y, r);                                 // r < y: parent <= child holds
        if ((unsigned)p >= (unsigned)y) break;
        x = y;
        y = p;
    }
    return r;
}
__device__ __forceinline__ void g_unite(int* c, int a, int b) {
    a = g_find_compress(c, a);
    b = g_find_compress(c, b);
    for (;;) {
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(c + a, b);
        if (old == a) return;
        a = g_find(c, old);
        b = g_find(c, b);
    }
}

// ---------------------------------------------------------------- 1. the pieces of every tile
template <bool RAGGED>
__global__ __launch_bounds__(256) void cc_tile_kernel(const unsigned char* __restrict__ labels, TileGeo geo, int conn8, int* __restrict__ comp) {
    __shared__ unsigned short sv[(CC_TH + 1) * CC_SP];       // row 0 and columns 0, 65 stay CC_OUT
    __shared__ int L[CC_TH * CC_TW];
    const Tile t = tile_of<RAGGED>(geo);
    const int H = t.H, W = t.W;
    const unsigned char* __restrict__ src = labels + t.lab;
    for (int i = threadIdx.x; i < (CC_TH + 1) * CC_SP; i += 256) sv[i] = CC_OUT;
    __syncthreads();
    {   // stage: 4 threads per 16-pixel segment of a row; one 16-byte load where the segment is whole and aligned, bytes otherwise
        const int g = threadIdx.x >> 2, sub = threadIdx.x & 3;
        const int r = g >> 2, seg = g & 3;
        const int y = t.y0 + r, xs = t.x0 + seg * 16;
        if (y < H && xs < W) {
            const unsigned char* p = src + (long long)y * W + xs;
            unsigned short* d = sv + (r + 1) * CC_SP + 1 + seg * 16;
            if (xs + 16 <= W && ((uintptr_t)p & 15) == 0) {
                if (sub == 0) {
                    const uint4 q = *reinterpret_cast<const uint4*>(p);
                    const unsigned int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int k = 0; k < 16; ++k) d[k] = (unsigned short)((w[k >> 2] >> (8 * (k & 3))) & 255u);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (xs + sub * 4 + k < W) d[sub * 4 + k] = p[sub * 4 + k];
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- row runs: a pixel starts as the first pixel of its run (one ballot per row)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = 4 * k + wave;
        const unsigned short* s = sv + (r + 1) * CC_SP + 1 + lane;
        const bool same_left = s[0] == s[-1] && s[0] != CC_OUT;
        const unsigned long long heads = __ballot(!same_left);                   // bit 0 is always set: column -1 is CC_OUT
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
        L[r * CC_TW + lane] = r * CC_TW + start;
    }
    __syncthreads();
    // ---- contacts with the row above: the first pixel of every contact between two runs unites them
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = 4 * k + wave;
        if (r == 0) continue;
        const unsigned short* s = sv + (r + 1) * CC_SP + 1 + lane;
        const unsigned short* u = s - CC_SP;
        const int v = s[0];
        if (v == CC_OUT) continue;
        const int i = r * CC_TW + lane;
        if (v == u[0]) {
            if (!(s[-1] == v && u[-1] == v)) lds_unite(L, i, i - CC_TW);         // else the pixel on the left made this contact
        } else if (conn8) {
            if (v == u[-1] && s[-1] != v) lds_unite(L, i, i - CC_TW - 1);
            if (v == u[1] && s[1] != v) lds_unite(L, i, i - CC_TW + 1);
        }
    }
    __syncthreads();
    // ---- flatten; the order of the local indices is the raster order of the image, so the local minimum is the piece's first pixel
    int* __restrict__ out = comp + t.lab;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = 4 * k + wave;
        const int y = t.y0 + r, x = t.x0 + lane;
        if (y < H && x < W) {
            const int root = lds_find(L, r * CC_TW + lane);
            out[(long long)y * W + x] = (t.y0 + (root >> 6)) * W + t.x0 + (root & 63);
        }
    }
}

// ---------------------------------------------------------------- 2. the seams
template <bool RAGGED>
__global__ __launch_bounds__(128) void cc_merge_kernel(const unsigned char* __restrict__ labels, TileGeo geo, int conn8, int* __restrict__ comp) {
    const Tile t = tile_of<RAGGED>(geo);
    const int H = t.H, W = t.W;
    const unsigned char* __restrict__ m = labels + t.lab;
    int* c = comp + t.lab;
    const int lane = threadIdx.x & 63;
    auto val = [&](int y, int x) -> int { return (y >= 0 && y < H && x >= 0 && x < W) ? (int)m[(long long)y * W + x] : CC_OUT; };
    if (threadIdx.x < 64) {                                  // top seam: row y0 against row y0 - 1
        const int y = t.y0, x = t.x0 + lane;
        if (y == 0 || x >= W) return;
        const int v = val(y, x), up = val(y - 1, x), vl = val(y, x - 1), ul = val(y - 1, x - 1);
        const int i = y * W + x;
        if (v == up) {
            if (!(vl == v && ul == v)) g_unite(c, i, i - W);                     // else the pixel on the left (this tile's or the next's) does
        } else if (conn8) {
            if (v == ul && vl != v) g_unite(c, i, i - W - 1);                    // x - 1 may lie in the tile on the left: the corner pair
            if (v == val(y - 1, x + 1) && val(y, x + 1) != v) g_unite(c, i, i - W + 1);   // x + 1 may lie in the tile on the right
        }
    } else {                                                 // left seam: column x0 against column x0 - 1
        const int y = t.y0 + lane, x = t.x0;
        if (lane >= CC_TH || x == 0 || y >= H) return;
        const int v = val(y, x), l = val(y, x - 1), va = val(y - 1, x), la = val(y - 1, x - 1);
        const int i = y * W + x;
        if (v == l) {
            // else the pixel above does.  Only inside the tile: there the two columns hang together through the tile's own pieces,
            // while the first row's contact with the row above is a top-seam union that may itself lean on this one
            if (!(lane > 0 && va == v && la == v)) g_unite(c, i, i - 1);
        } else if (conn8) {
            if (v == la && va != v) g_unite(c, i, i - W - 1);
            if (v == val(y + 1, x - 1) && val(y + 1, x) != v) g_unite(c, i, i + W - 1);
        }
    }
}

// ---------------------------------------------------------------- 3. flatten and count
template <bool RAGGED>
__global__ __launch_bounds__(256) void cc_flatten_kernel(TileGeo geo, int* __restrict__ comp, int* __restrict__ area) {
    __shared__ int cnt[CC_TH * CC_TW], rootv[CC_TH * CC_TW];
    const Tile t = tile_of<RAGGED>(geo);
    const int H = t.H, W = t.W;
    int* c = comp + t.lab;
    int* a = area + t.lab;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < CC_TH * CC_TW; i += 256) cnt[i] = 0;
    __syncthreads();
    int rootk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = 4 * k + wave;
        const int y = t.y0 + r, x = t.x0 + lane;
        const bool in = y < H && x < W;
        const int i = y * W + x;
        // the parent: the root of the pixel's piece (inside this tile), or wherever the merge hung a pixel that was such a root
        const int p = in ? g_load(c + i) : -1;
        const int pl = __shfl_up(p, 1, 64);
        const bool head = lane == 0 || p != pl;
        const unsigned long long heads = __ballot(head);
        const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));     // the head of this lane's run
        const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = after ? __ffsll((long long)after) : 64 - lane;                 // of a head: the length of its run
        int root = -1;
        if (head && in) {
            root = g_find(c, p);
            const int py = p / W, px = p - py * W;
            const int ly = py - t.y0, lx = px - t.x0;
            if (ly >= 0 && ly < CC_TH && lx >= 0 && lx < CC_TW) {                      // equal parents have equal roots: count per parent
                atomicAdd(&cnt[ly * CC_TW + lx], len);
                rootv[ly * CC_TW + lx] = root;
            } else {
                atomicAdd(a + root, len);
            }
        }
        rootk[k] = __shfl(root, first, 64);
    }
    // the stores come after every find of the workgroup: a find that meets a flattened pixel would be right as well (parent <= child
    // still holds, roots never change), this only keeps the loads of the walk apart from the stores
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = 4 * k + wave;
        const int y = t.y0 + r, x = t.x0 + lane;
        if (y < H && x < W) __hip_atomic_store(c + (y * W + x), rootk[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = threadIdx.x + 256 * k;
        const int n = cnt[s];
        if (n) atomicAdd(a + rootv[s], n);
    }
}

// ---------------------------------------------------------------- 4. every pixel gets its component's area
template <bool RAGGED>
__global__ __launch_bounds__(256) void cc_broadcast_kernel(TileGeo geo, const int* __restrict__ comp, int* area) {
    const Tile t = tile_of<RAGGED>(geo);
    const int H = t.H, W = t.W;
    const int* __restrict__ c = comp + t.lab;
    int* a = area + t.lab;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = t.y0 + 4 * k + wave, x = t.x0 + lane;
        if (y < H && x < W) {
            const int i = y * W + x, r = c[i];
            if (r != i) a[i] = a[r];                         // a[r]: a root slot, written by nobody in this launch
        }
    }
}

// ---------------------------------------------------------------- the small-region filter
// One thread per 4 pixels of a row (16 threads per tile row).  comp / area travel as 16-byte loads and the maps as dwords where the
// addresses allow; a quad that crosses the image's edge or is misaligned goes pixel by pixel.
template <bool RAGGED>
__global__ __launch_bounds__(256) void cc_filter_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ comp,
                                                        const int* __restrict__ area, TileGeo geo, const int* __restrict__ min_area,
                                                        int min_area_all, int nc, unsigned char* __restrict__ out, int* __restrict__ counts) {
    __shared__ int sums[3];
    const Tile t = tile_of<RAGGED>(geo);
    const int H = t.H, W = t.W;
    const int thr = min_area ? min_area[t.b] : min_area_all;
    const bool refused = thr < 1;                            // the map is copied, the image's first tile marks its row
    if (refused && t.x0 == 0 && t.y0 == 0 && threadIdx.x < 3) counts[3 * t.b + threadIdx.x] = -1;
    if (threadIdx.x < 3) sums[threadIdx.x] = 0;
    __syncthreads();
    const int y = t.y0 + (threadIdx.x >> 4), x = t.x0 + 4 * (threadIdx.x & 15);
    int n_comp = 0, n_gone = 0, n_pix = 0;
    if (y < H && x < W) {
        const int i = y * W + x;
        const long long gi = t.lab + i;
        int v[4], cc[4], ar[4];
        const int n = min(4, W - x);
        if (n == 4 && (((uintptr_t)(comp + gi) | (uintptr_t)(area + gi)) & 15) == 0) {
            const int4 q = *reinterpret_cast<const int4*>(comp + gi), s = *reinterpret_cast<const int4*>(area + gi);
            cc[0] = q.x; cc[1] = q.y; cc[2] = q.z; cc[3] = q.w;
            ar[0] = s.x; ar[1] = s.y; ar[2] = s.z; ar[3] = s.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { cc[k] = k < n ? comp[gi + k] : -1; ar[k] = k < n ? area[gi + k] : 0; }
        }
        const bool vec_in = n == 4 && (((uintptr_t)labels + (unsigned long long)gi) & 3) == 0;
        if (vec_in) {
            const unsigned int w = *reinterpret_cast<const unsigned int*>(labels + gi);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (w >> (8 * k)) & 255;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < n ? (int)labels[gi + k] : 255;
        }
        unsigned int packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool cls = k < n && v[k] < nc && !refused;
            const bool gone = cls && ar[k] < thr;
            n_comp += cls && cc[k] == i + k;
            n_gone += gone && cc[k] == i + k;
            n_pix += gone;
            if (gone) v[k] = 255;
            packed |= (unsigned int)v[k] << (8 * k);
        }
        if (n == 4 && (((uintptr_t)out + (unsigned long long)gi) & 3) == 0) {
            *reinterpret_cast<unsigned int*>(out + gi) = packed;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) out[gi + k] = (unsigned char)v[k];
        }
    }
    // one LDS add per wave and counter, one global add per workgroup and counter
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_comp += __shfl_xor(n_comp, o, 64);
        n_gone += __shfl_xor(n_gone, o, 64);
        n_pix += __shfl_xor(n_pix, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_comp) atomicAdd(&sums[0], n_comp);
        if (n_gone) atomicAdd(&sums[1], n_gone);
        if (n_pix) atomicAdd(&sums[2], n_pix);
    }
    __syncthreads();
    if (threadIdx.x < 3 && sums[threadIdx.x]) atomicAdd(&counts[3 * t.b + threadIdx.x], sums[threadIdx.x]);
}

// ---------------------------------------------------------------- host entries
extern "C" int excel_label_components(const uint8_t* labels, int B, int H, int W, const int32_t* table, const excel_ragged_info* info,
                                      int connectivity, int32_t* comp, int32_t* area, void* stream) {
    EXCEL_CHECK_ARG(labels && comp && area, "label_components: null argument (labels, comp and area are required)");
    EXCEL_CHECK_ARG(connectivity == 4 || connectivity == 8, "label_components: connectivity must be 4 or 8 (got %d)", connectivity);
    EXCEL_CHECK_ARG(((uintptr_t)comp & 3) == 0 && ((uintptr_t)area & 3) == 0 && ((uintptr_t)table & 3) == 0,
                    "label_components: comp, area and table must be 4-byte aligned");
    TileGeo geo;
    dim3 grid;
    long long total;
    TRY(label_tile_geometry("label_components", B, H, W, table, info, &geo, &grid, &total));
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    TRY(clear_on_stream("label_components", "areas", area, sizeof(int32_t) * (size_t)total, st));      // the root slots are added to
    const int conn8 = connectivity == 8;
    if (table) {
        hipLaunchKernelGGL(cc_tile_kernel<true>, grid, dim3(256), 0, st, labels, geo, conn8, comp);
        hipLaunchKernelGGL(cc_merge_kernel<true>, grid, dim3(128), 0, st, labels, geo, conn8, comp);
        hipLaunchKernelGGL(cc_flatten_kernel<true>, grid, dim3(256), 0, st, geo, comp, area);
        hipLaunchKernelGGL(cc_broadcast_kernel<true>, grid, dim3(256), 0, st, geo, comp, area);
    } else {
        hipLaunchKernelGGL(cc_tile_kernel<false>, grid, dim3(256), 0, st, labels, geo, conn8, comp);
        hipLaunchKernelGGL(cc_merge_kernel<false>, grid, dim3(128), 0, st, labels, geo, conn8, comp);
        hipLaunchKernelGGL(cc_flatten_kernel<false>, grid, dim3(256), 0, st, geo, comp, area);
        hipLaunchKernelGGL(cc_broadcast_kernel<false>, grid, dim3(256), 0, st, geo, comp, area);
    }
    EXCEL_CHECK_LAUNCH("label_components");
    return EXCEL_OK;
}

extern "C" int excel_filter_small_regions(const uint8_t* labels, const int32_t* comp, const int32_t* area, int B, int H, int W,
                                          const int32_t* table, const excel_ragged_info* info, const int32_t* min_area, int min_area_all,
                                          int num_classes, uint8_t* out, int32_t* counts, void* stream) {
    EXCEL_CHECK_ARG(labels && comp && area && out && counts,
                    "filter_small_regions: null argument (labels, comp, area, out and counts are required)");
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= 256, "filter_small_regions: need 1 <= num_classes <= 256 (got %d)", num_classes);
    EXCEL_CHECK_ARG(((uintptr_t)comp & 3) == 0 && ((uintptr_t)area & 3) == 0 && ((uintptr_t)counts & 3) == 0 &&
                        ((uintptr_t)min_area & 3) == 0 && ((uintptr_t)table & 3) == 0,
                    "filter_small_regions: comp, area, counts, min_area and table must be 4-byte aligned");
    TileGeo geo;
    dim3 grid;
    long long total;
    TRY(label_tile_geometry("filter_small_regions", B, H, W, table, info, &geo, &grid, &total));
    EXCEL_CHECK_ARG((uintptr_t)out + (size_t)total <= (uintptr_t)labels || (uintptr_t)labels + (size_t)total <= (uintptr_t)out,
                    "filter_small_regions: out overlaps labels (the filter does not run in place)");
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    TRY(clear_on_stream("filter_small_regions", "counts", counts, sizeof(int32_t) * (size_t)B * 3, st));
    if (table)
        hipLaunchKernelGGL(cc_filter_kernel<true>, grid, dim3(256), 0, st, labels, comp, area, geo, min_area, min_area_all, num_classes, out, counts);
    else
        hipLaunchKernelGGL(cc_filter_kernel<false>, grid, dim3(256), 0, st, labels, comp, area, geo, min_area, min_area_all, num_classes, out, counts);
    EXCEL_CHECK_LAUNCH("filter_small_regions");
    return EXCEL_OK;
}
