// Fully-connected CRF post-processing (utils/dcrf.py:42-68 class DenseCRF, :7-40 crf_inference*; driven by tools/infer_lam.py:179-237):
// mean-field inference with a Gaussian (x,y) and a bilateral (x,y,r,g,b) Potts term, message passing = high-dimensional Gaussian
// filtering on the permutohedral lattice (Adams, Baek & Davis 2010), as Kraehenbuehl & Koltun's densecrf - the library behind the
// reference's pydensecrf dependency - does it.  Everything on the device, for ONE image (excel_dcrf_inference) or for a GROUP of images
// of a ragged batch in the same chain of launches (excel_dcrf_inference_ragged: the group is one array of sum H_b W_b pixels with
// image-local (x, y); the image index rides in the spare short 7 of every lattice key, so one hash table per lattice kind serves the
// group, no blur neighbour crosses an image, and every image gets the bits it gets alone):
//   crf_lattice_kernel<D>   per pixel: feature -> elevate -> nearest 0-coloured lattice point -> rank -> barycentric weights + the D+1 vertex keys
//   crf_hash_insert         open-addressing hash of vertex keys (atomicCAS claims a slot for the first vertex with a key; later ones compare)
//   crf_offsets / crf_neighbors   vertex -> lattice point index; per lattice point and axis the two blur neighbours (key -+ 1, axis j: +- D)
//   crf_csr_*   per lattice point the list of its vertices (built in tables that are dead once the neighbours are found)
//   splat (a segmented sum over those lists in 64-bit fixed point: the sum is order independent, so results are bit-reproducible although lattice indices are
//   handed out by an atomic counter) -> D+1 blur passes -> slice, symmetric normalisation 1/sqrt(K 1)
//   mean field: Q = softmax(-U); 10 x { Q = softmax(-U + w_g K_g Q + w_b K_b Q) }
// excel_dcrf_lam_ragged is the group form for LAMs (tools/infer_lam.py:179-237 inline): every image b of the group has its OWN class count
// nchan[b] (its k_b + 1 planes) and reads the pipeline's pitched step cams in place.  The value rows of pixels and lattice points keep ONE
// stride per group, Cg = max nchan; a work item (point, k) with k >= the class count of the point's image returns, so rows of an image
// with fewer classes are partly unused (memory, idle lanes) but never read or written past its count.  A lattice point's image is
// short 7 of its key; the CSR build reuses the key table, so the per-point class counts are written to workspace of their own before
// it (crf_point_classes_kernel).  The per-class arithmetic and the order of the softmax sum are those of the uniform path, so every image
// gets, bit for bit, the Q and labels excel_dcrf_inference gives it alone with C = nchan[b] on its tight planes.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define CRF_KS 8                 // shorts per stored key (D <= 6: short 7 carries the image index of a group)
#define CRF_IMG_SLOT 7
#define CRF_MAX_IMAGES 32767
#define CRF_FIX 1099511627776.0  // 2^40 fixed-point scale of the splat accumulators

struct CrfKey { unsigned long long a, b; };   // 8 shorts

__device__ __forceinline__ unsigned crf_hash(const CrfKey& k) {
    unsigned long long h = k.a * 0x9E3779B97F4A7C15ull ^ (k.b + 0x7F4A7C15ull) * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return (unsigned)h;
}
__device__ __forceinline__ void crf_setk(CrfKey& k, int i, int v) {
    const unsigned long long m = (unsigned long long)(unsigned short)(short)v << (16 * (i & 3));
    if (i < 4) k.a |= m; else k.b |= m;
}
__device__ __forceinline__ int crf_getk(const CrfKey& k, int i) {
    return (short)(unsigned short)(((i < 4) ? k.a : k.b) >> (16 * (i & 3)));
}

// feature layout of DenseCRF2D (densecrf.cpp addPairwiseGaussian / addPairwiseBilateral): (x/sxy, y/sxy[, r/srgb, g/srgb, b/srgb])
// tab == nullptr: one image of H x W.  Otherwise pixel n of a group of B images (ragged table `tab`): image b = ragged_image_of_pixel,
// (x, y) local to it, the key tagged with b.  rgb is packed like the pixels (image b at 3 * loff_b), so it is indexed by n either way.
template <int D>
__global__ __launch_bounds__(256) void crf_lattice_kernel(const unsigned char* __restrict__ rgb, const int* __restrict__ tab, int B, long long N, int H,
                                                          int W, float sxy, float srgb, CrfKey* __restrict__ keys, float* __restrict__ bary) {
    // Contraction is off in this kernel: the roundings of the construction decide the simplex and the weights, and they are the ones
    // written here, as permutohedral.cpp and oracle/dcrf.py make them.  Plain operators, not __fmul_rn / __fsub_rn: those are inlined
    // as plain operations that carry their header's contraction flag into this body, and hipcc -O3 made fma(-j, cf, sm) of
    // elevated[j] = __fsub_rn(sm, __fmul_rn(j, cf)), which moved barycentric weights by up to 2e-5 at bi_rgb_std 1 and a message by
    // 2e-6 where two pixels couple through one blur neighbour (tests/test_gpu_dcrf_filter.py, `distinct`).
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    int img = 0, loc = (int)n;
    if (tab) {
        img = ragged_image_of_pixel(tab, B, n);
        const int* rec = tab + EXCEL_RAG_REC * img;
        W = rec[1];
        loc = (int)(n - rec[4]);
    }
    const int x = loc % W, y = loc / W;
    float f[D];
    f[0] = (float)x / sxy;
    f[1] = (float)y / sxy;
    if (D == 5) {
#pragma unroll
        for (int c = 0; c < 3; ++c) f[2 + c] = (float)rgb[(long long)n * 3 + c] / srgb;
    }
    const float inv_std = sqrtf(2.0f / 3.0f) * (float)(D + 1);      // expected std of the filter (Adams et al. p.6)
    float elevated[D + 1];
    float sm = 0.f;
#pragma unroll
    for (int j = D; j > 0; --j) {
        const float scale = (float)(1.0 / sqrt((double)((j + 1) * j))) * inv_std;
        const float cf = f[j - 1] * scale;
        elevated[j] = sm - (float)j * cf;
        sm = sm + cf;
    }
    elevated[0] = sm;
    const float down = 1.0f / (float)(D + 1), up = (float)(D + 1);
    int rem0[D + 1], rank[D + 1], sum = 0;
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        const float v = down * elevated[i];
        const float u = ceilf(v) * up, dn = floorf(v) * up;
        rem0[i] = (u - elevated[i] < elevated[i] - dn) ? (int)u : (int)dn;
        sum += rem0[i] / (D + 1);
        rank[i] = 0;
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i + 1; j <= D; ++j) {
            if (elevated[i] - (float)rem0[i] < elevated[j] - (float)rem0[j]) ++rank[i]; else ++rank[j];
        }
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        rank[i] += sum;
        if (rank[i] < 0) { rank[i] += D + 1; rem0[i] += D + 1; }
        else if (rank[i] > D) { rank[i] -= D + 1; rem0[i] -= D + 1; }
    }
    float bc[D + 2];
#pragma unroll
    for (int i = 0; i <= D + 1; ++i) bc[i] = 0.f;
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        const float v = (elevated[i] - (float)rem0[i]) * down;
#pragma unroll
        for (int q = 0; q <= D + 1; ++q) {       // static indexing (a dynamically indexed register array goes to scratch)
            if (q == D - rank[i]) bc[q] += v;
            if (q == D - rank[i] + 1) bc[q] -= v;
        }
    }
    bc[0] += 1.0f + bc[D + 1];
#pragma unroll
    for (int r = 0; r <= D; ++r) {
        CrfKey k{0ull, 0ull};
#pragma unroll
        for (int i = 0; i < D; ++i) {
            // canonical[r][rank] = r for rank <= D - r, else r - (D+1)
            const int can = (rank[i] <= D - r) ? r : r - (D + 1);
            crf_setk(k, i, rem0[i] + can);
        }
        crf_setk(k, CRF_IMG_SLOT, img);
        keys[(long long)n * (D + 1) + r] = k;
        bary[(long long)n * (D + 1) + r] = bc[r];
    }
}

__global__ __launch_bounds__(256) void crf_hash_insert_kernel(const CrfKey* __restrict__ keys, long long npv, int* __restrict__ table, unsigned mask,
                                                              int* __restrict__ rep, int* __restrict__ latidx, int* __restrict__ counter,
                                                              CrfKey* __restrict__ lkeys) {
    const long long pv = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pv >= npv) return;
    const CrfKey k = keys[pv];
    unsigned h = crf_hash(k) & mask;
    while (true) {
        const int e = atomicCAS(&table[h], -1, (int)pv);
        if (e == -1) {
            const int li = atomicAdd(counter, 1);
            latidx[pv] = li;
            lkeys[li] = k;
            rep[pv] = (int)pv;
            return;
        }
        const CrfKey ke = keys[e];
        if (ke.a == k.a && ke.b == k.b) { rep[pv] = e; return; }
        h = (h + 1) & mask;
    }
}

__global__ __launch_bounds__(256) void crf_offsets_kernel(const int* __restrict__ rep, const int* __restrict__ latidx, long long npv, int* __restrict__ offset) {
    const long long pv = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pv < npv) offset[pv] = latidx[rep[pv]];
}

__device__ __forceinline__ int crf_find(const CrfKey& k, const CrfKey* keys, const int* table, unsigned mask, const int* latidx) {
    unsigned h = crf_hash(k) & mask;
    while (true) {
        const int e = table[h];
        if (e == -1) return -1;
        const CrfKey ke = keys[e];
        if (ke.a == k.a && ke.b == k.b) return latidx[e];
        h = (h + 1) & mask;
    }
}

template <int D>
__global__ __launch_bounds__(256) void crf_neighbors_kernel(const CrfKey* __restrict__ lkeys, const int* __restrict__ counter, const CrfKey* __restrict__ keys,
                                                            const int* __restrict__ table, unsigned mask, const int* __restrict__ latidx,
                                                            int2* __restrict__ nbr, long long Mcap) {
    const int M = *counter;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t % Mcap), j = (int)(t / Mcap);
    if (j > D || i >= M) return;
    const CrfKey k = lkeys[i];
    CrfKey n1{0ull, 0ull}, n2{0ull, 0ull};
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const int v = crf_getk(k, c);
        crf_setk(n1, c, (c == j) ? v + D : v - 1);
        crf_setk(n2, c, (c == j) ? v - D : v + 1);
    }
    const int img = crf_getk(k, CRF_IMG_SLOT);                  // neighbours stay inside the image
    crf_setk(n1, CRF_IMG_SLOT, img);
    crf_setk(n2, CRF_IMG_SLOT, img);
    nbr[(long long)j * Mcap + i] = make_int2(crf_find(n1, keys, table, mask, latidx), crf_find(n2, keys, table, mask, latidx));
}

// ---- message passing of one mean-field step: BOTH kernels (Gaussian: lattice g, bilateral: lattice b) ride in the same launches
//   splat (1 launch) -> blur passes (max(D_g, D_b) + 1 launches; pass 0 reads the fixed-point accumulators, pass 1 re-zeroes them for
//   the next step) -> slice + mean-field update (1 launch): 8 launches per step instead of 18 (a memset, splat, fixed->float, D+1 blurs
//   and a slice per kernel, then the update).  Same operations in the same order as the per-kernel form: same bits.
struct CrfSide {                 // one lattice as the message-passing kernels see it
    const int* offset;           // [npv] vertex -> lattice point
    const float* bary;           // [npv]
    const float* norm;           // [N] symmetric normaliser (may be null while it is being built)
    const int2* nbr;             // [D+1][npv] blur neighbours
    const int* counter;          // number of lattice points
    long long* acc;              // [npv*C] fixed-point splat accumulators
    float *lat0, *lat1;          // [npv*C] ping-pong
    long long npv;
    int Dp1;
    float alpha;                 // 1 / (1 + 2^-D)
    const int *seg_start, *seg_cnt, *seg_list;   // per lattice point: its vertices list[start .. start + cnt) (segmented splat)
    const int* ncls;             // LAM groups: class count of every lattice point's image (<= the row stride C); null otherwise
};

// splat: acc[o][k] = sum over the vertices of lattice point o of w * (in[n][k] * norm[n]), in 2^-40 fixed point (integer sums commute:
// bit-reproducible whatever the order of a list).  No atomics: lattice point i adds up the vertices of its list (built once per lattice,
// crf_csr_*), which gives the bits the earlier 64-bit atomicAdd splat gave and measured faster (EXPERIMENTS "Batched DenseCRF").  One
// thread per (i, k), k fastest: the threads of a point walk the same list (broadcast loads) and read `in` along k.
// LAM: rows have stride C = the group's largest class count; item (i, k) beyond the class count of point i's image has no work.
template <bool LAM>
__device__ __forceinline__ void crf_splat_side(const float* __restrict__ in, int use_norm, const CrfSide& L, int C) {
    const long long total = (long long)(*L.counter) * C, stride = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int i = (int)(t / C), k = (int)(t - (long long)i * C);
        if (LAM && k >= L.ncls[i]) continue;
        const int* lst = L.seg_list + L.seg_start[i];
        const int cnt = L.seg_cnt[i];
        long long sum = 0;
        for (int e = 0; e < cnt; ++e) {
            const long long pv = lst[e];
            const long long n = pv / L.Dp1;
            float v = in[n * C + k];
            if (use_norm) v = __fmul_rn(v, L.norm[n]);
            const float wv = __fmul_rn(L.bary[pv], v);
            sum += (long long)__double2ll_rn((double)wv * CRF_FIX);
        }
        L.acc[t] = sum;
    }
}
template <bool LAM>
__global__ __launch_bounds__(256) void crf_splat2_kernel(const float* __restrict__ in, int use_norm, CrfSide g, CrfSide b, int C) {
    crf_splat_side<LAM>(in, use_norm, g, C);
    crf_splat_side<LAM>(in, use_norm, b, C);
}
// vertex lists per lattice point: count, hand every point a segment (in any order: the sum does not care), fill
__global__ __launch_bounds__(256) void crf_csr_count_kernel(const int* __restrict__ offset, long long npv, int* __restrict__ cnt) {
    const long long pv = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pv < npv) atomicAdd(&cnt[offset[pv]], 1);
}
__global__ __launch_bounds__(256) void crf_csr_start_kernel(const int* __restrict__ cnt, const int* __restrict__ counter, int* __restrict__ cursor,
                                                            int* __restrict__ start) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < *counter) start[i] = atomicAdd(cursor, cnt[i]);
}
__global__ __launch_bounds__(256) void crf_csr_fill_kernel(const int* __restrict__ offset, long long npv, const int* __restrict__ start,
                                                           int* __restrict__ fill, int* __restrict__ list) {
    const long long pv = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pv >= npv) return;
    const int o = offset[pv];
    list[start[o] + atomicAdd(&fill[o], 1)] = (int)pv;
}
__device__ __forceinline__ float crf_fix(long long a) { return (float)((double)a * (1.0 / CRF_FIX)); }
// blur pass j of one lattice: grid-stride over its M lattice points (M is read on the device: the bilateral lattice of
// tools/infer_lam.py's parameters (sxy 67) has a few thousand points, the launch capacity would be 6 N).  Pass 0 converts the
// accumulators on the fly, pass 1 clears them (nobody reads them after pass 0).
template <bool LAM>
__device__ __forceinline__ void crf_blur_side(const CrfSide& L, int j, int C) {
    if (j >= L.Dp1) return;
    const long long total = (long long)(*L.counter) * C, stride = (long long)gridDim.x * 256;
    float* nw = (j & 1) ? L.lat0 : L.lat1;             // pass 0: acc -> lat1, pass 1: lat1 -> lat0, ...
    const float* old = (j & 1) ? L.lat1 : L.lat0;
    const int2* nbr = L.nbr + (long long)j * L.npv;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int i = (int)(t / C), k = (int)(t - (long long)i * C);
        if (LAM && k >= L.ncls[i]) continue;                   // (the neighbours are points of the same image: same count)
        const int2 nb = nbr[i];
        if (j == 0) {
            const float a = nb.x >= 0 ? crf_fix(L.acc[(long long)nb.x * C + k]) : 0.f, c = nb.y >= 0 ? crf_fix(L.acc[(long long)nb.y * C + k]) : 0.f;
            nw[t] = crf_fix(L.acc[t]) + 0.5f * (a + c);
        } else {
            const float a = nb.x >= 0 ? old[(long long)nb.x * C + k] : 0.f, c = nb.y >= 0 ? old[(long long)nb.y * C + k] : 0.f;
            nw[t] = old[t] + 0.5f * (a + c);
            if (j == 1) L.acc[t] = 0;
        }
    }
}
template <bool LAM>
__global__ __launch_bounds__(256) void crf_blur2_kernel(CrfSide g, CrfSide b, int j, int C) {
    crf_blur_side<LAM>(g, j, C);
    crf_blur_side<LAM>(b, j, C);
}
// LAM groups: the class count of every lattice point = that of its image (short 7 of its key), clamped to the row stride.  Runs before
// crf_csr_build, which reuses lkeys.
__global__ __launch_bounds__(256) void crf_point_classes_kernel(const CrfKey* __restrict__ lkeys, const int* __restrict__ counter,
                                                                const int* __restrict__ nchan, int B, int Cg, int* __restrict__ ncls) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= *counter) return;
    const int img = min(max(crf_getk(lkeys[i], CRF_IMG_SLOT), 0), B - 1);
    ncls[i] = min(max(nchan[img], 1), Cg);
}
// the Dp1 vertices of pixel n (lattice point, barycentric weight x alpha... kept separate: same roundings as the per-kernel form) in
// registers: a pixel's C classes reuse them
template <int DP1>
struct CrfVerts {
    long long off[DP1];
    float w[DP1];
    __device__ __forceinline__ void load(const CrfSide& L, long long n, int C) {
#pragma unroll
        for (int j = 0; j < DP1; ++j) { off[j] = (long long)L.offset[n * DP1 + j] * C; w[j] = L.bary[n * DP1 + j]; }
    }
    __device__ __forceinline__ float slice(const float* __restrict__ lat, int k, float alpha) const {
        float v[DP1];
#pragma unroll
        for (int j = 0; j < DP1; ++j) v[j] = lat[off[j] + k];          // independent gathers, all in flight
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < DP1; ++j) s += __fmul_rn(__fmul_rn(w[j], v[j]), alpha);
        return s;
    }
};
__device__ __forceinline__ const float* crf_final_lat(const CrfSide& L) { return (L.Dp1 & 1) ? L.lat1 : L.lat0; }   // buffer the last pass wrote

// normalisers of both lattices from K 1: norm = 1 / sqrt(K 1 + 1e-20)   (DenseKernel::initLattice, NORMALIZE_SYMMETRIC); C = 1
__global__ __launch_bounds__(256) void crf_make_norm2_kernel(CrfSide g, CrfSide b, long long N, float* __restrict__ norm_g, float* __restrict__ norm_b) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    CrfVerts<3> vg;
    CrfVerts<6> vb;
    vg.load(g, n, 1);
    vb.load(b, n, 1);
    norm_g[n] = 1.0f / sqrtf(vg.slice(crf_final_lat(g), 0, g.alpha) + 1e-20f);
    norm_b[n] = 1.0f / sqrtf(vb.slice(crf_final_lat(b), 0, b.alpha) + 1e-20f);
}
// slice both messages + the mean-field update of one pixel:  Q = softmax(-U + w_g K_g Q + w_b K_b Q).  U [C,N] (plane-major, as
// unary_from_softmax lays it out); Q [N,C].  have_msg = 0: the initial Q = softmax(-U).  With a ragged table U and out_cn are tight
// [C, H_b, W_b] per image (image b at C * loff_b) and pixel n reads / writes the planes of its own image; lab (optional) = the arg-max
// of the q values written, first maximum (excel_argmax_label's rule).
// LAM: U and out_cn are Cmax PITCHED planes per image (image b at Cmax * poff_b, rows of Wp_b floats: the pipeline's step cams), pixel n
// runs over the first nc = nchan[image] planes only (clamped to 1..C; C = the stride of the Q rows), pad columns and planes >= nc are
// neither read nor written, and lab = the key of the arg-max (channel 0 -> 0, c -> cls_idx[b, c-1] + 1: excel_argmax_label_ragged's map).
struct CrfLam {
    const int* nchan;            // device [B]
    const int* cls_idx;          // device [B, smax] or null
    int smax, Cmax;
};
template <bool LAM>
__global__ __launch_bounds__(256) void crf_update_kernel(const float* __restrict__ prob, int is_energy, const int* __restrict__ tab, int B, long long N, int C,
                                                         int have_msg, CrfSide g, float wg, CrfSide b, float wb, float* __restrict__ Q,
                                                         float* __restrict__ out_cn, unsigned char* __restrict__ lab, CrfLam lam) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    long long ps = N, po = n;                                   // plane stride and offset of pixel n in U / out_cn
    int nc = C;
    const int* cls_row = nullptr;
    if (LAM) {
        const int img = ragged_image_of_pixel(tab, B, n);
        const int* rec = tab + EXCEL_RAG_REC * img;
        const int W = rec[1], Wp = (W + 3) & ~3, loc = (int)(n - rec[4]), y = loc / W;
        ps = (long long)rec[0] * Wp;
        po = (long long)lam.Cmax * rec[2] + (long long)y * Wp + (loc - y * W);
        nc = min(max(lam.nchan[img], 1), C);
        if (lam.cls_idx) cls_row = lam.cls_idx + (long long)img * lam.smax;
    } else if (tab) {
        const int* rec = tab + EXCEL_RAG_REC * ragged_image_of_pixel(tab, B, n);
        ps = (long long)rec[0] * rec[1];
        po = (long long)C * rec[4] + (n - rec[4]);
    }
    CrfVerts<3> vg;
    CrfVerts<6> vb;
    float ng = 0.f, nb = 0.f;
    const float *lg = crf_final_lat(g), *lb = crf_final_lat(b);
    if (have_msg) { vg.load(g, n, C); vb.load(b, n, C); ng = g.norm[n]; nb = b.norm[n]; }
    float mx = -INFINITY;
    for (int k = 0; k < nc; ++k) {
        const float pv = prob[(long long)k * ps + po];
        const float u = is_energy ? pv : -logf(fminf(fmaxf(pv, 1e-5f), 1.0f));                  // unary_from_softmax (clip 1e-5)
        float t = -u;
        if (have_msg) {
            const float mg = __fmul_rn(vg.slice(lg, k, g.alpha), ng), mb = __fmul_rn(vb.slice(lb, k, b.alpha), nb);
            t = t + wg * mg + wb * mb;
        }
        Q[n * C + k] = t;
        mx = fmaxf(mx, t);
    }
    float sum = 0.f;
    for (int k = 0; k < nc; ++k) { const float e = expf(Q[n * C + k] - mx); Q[n * C + k] = e; sum += e; }
    float best = 0.f;
    int bi = 0;
    for (int k = 0; k < nc; ++k) {
        const float q = Q[n * C + k] / sum;
        Q[n * C + k] = q;
        if (out_cn) out_cn[(long long)k * ps + po] = q;
        if (k == 0 || q > best) { best = q; bi = k; }
    }
    if (LAM && bi > 0 && cls_row) bi = cls_row[bi - 1] + 1;     // valid_key = [0, cls + 1 ...] (tools/infer_lam.py:225-226)
    if (lab) lab[n] = (unsigned char)bi;
}

struct CrfLattice {
    CrfKey *keys, *lkeys;
    float *bary, *norm;
    int *table, *rep, *latidx, *offset, *counter;
    int2* nbr;
    unsigned mask;
    long long npv;
    int D;
};
static CrfLattice crf_lattice_layout(Workspace& ws, long long N, int D) {
    CrfLattice L;
    const long long npv = N * (D + 1);
    unsigned cap = 1024;                                        // hash slots: the first power of two >= 2 per vertex
    while ((long long)cap < 2 * npv) cap <<= 1;
    L.keys = ws.take<CrfKey>(npv); L.lkeys = ws.take<CrfKey>(npv);
    L.bary = ws.take<float>(npv); L.norm = ws.take<float>(N);
    L.table = ws.take<int>(cap);
    L.rep = ws.take<int>(npv); L.latidx = ws.take<int>(npv); L.offset = ws.take<int>(npv);
    L.counter = ws.take<int>(1);
    L.nbr = ws.take<int2>((size_t)npv * (D + 1));
    L.mask = cap - 1; L.npv = npv; L.D = D;
    return L;
}

// The workspace of all three entries.  Per lattice (Gaussian D = 2, bilateral D = 5): the build tables, then the fixed-point accumulators
// [npv*C] and two float lattices [npv*C] of each side; Q [N,C]; ones [N]; LAM groups: + one class count per lattice point (capacity: one
// per vertex) of both lattices.  N = the pixels of the image, or of the whole group: the group shares one set of tables, so a group of
// one costs what the image costs alone.
struct CrfWs {
    CrfLattice Lg, Lb;
    CrfSide sg, sb;
    float *Q, *ones;
    int *cg, *cb;                // LAM only
    size_t total;
};
static CrfWs crf_ws_layout(long long N, int C, bool lam, void* base) {
    CrfWs w;
    Workspace ws(base);
    w.Lg = crf_lattice_layout(ws, N, 2);
    w.Lb = crf_lattice_layout(ws, N, 5);
    auto side = [&](CrfSide& s, const CrfLattice& L) {
        s.offset = L.offset; s.bary = L.bary; s.norm = L.norm; s.nbr = L.nbr; s.counter = L.counter; s.npv = L.npv; s.Dp1 = L.D + 1;
        s.alpha = 1.0f / (1.0f + powf(2.0f, (float)-L.D));
        s.seg_start = s.seg_cnt = s.seg_list = nullptr;
        s.acc = ws.take<long long>((size_t)L.npv * C);
        s.lat0 = ws.take<float>((size_t)L.npv * C);
        s.lat1 = ws.take<float>((size_t)L.npv * C);
    };
    side(w.sg, w.Lg);
    side(w.sb, w.Lb);
    w.Q = ws.take<float>((size_t)N * C);
    w.ones = ws.take<float>(N);
    w.cg = lam ? ws.take<int>(w.Lg.npv) : nullptr;
    w.cb = lam ? ws.take<int>(w.Lb.npv) : nullptr;
    w.sg.ncls = w.cg; w.sb.ncls = w.cb;
    w.total = ws.total();
    return w;
}
static size_t crf_workspace_bytes(long long N, int C) { return crf_ws_layout(N, C, false, nullptr).total; }
static size_t crf_lam_workspace_bytes(long long N, int Cg) { return crf_ws_layout(N, Cg, true, nullptr).total; }
// vertex indices (6 per pixel on the bilateral lattice) are ints and the hash table holds 2x as many slots, counted in 32 bits
static bool crf_fits(long long N) { return N >= 1 && N * 6 <= (1ll << 30); }

extern "C" size_t excel_dcrf_workspace_bytes(int H, int W, int C) {
    return crf_workspace_bytes((long long)H * W, C);
}

extern "C" int excel_dcrf_ragged_workspace_bytes(long long total_label_pix, int C, size_t* bytes) {
    EXCEL_CHECK_ARG(bytes && C >= 1 && total_label_pix >= 1, "dcrf_ragged_workspace_bytes: bad argument");
    EXCEL_CHECK_ARG(crf_fits(total_label_pix), "dcrf_ragged_workspace_bytes: a group of %lld pixels has more lattice vertices (6 per pixel) than "
                    "the 32-bit vertex indices hold: split it (ops.dcrf_groups)", total_label_pix);
    *bytes = crf_workspace_bytes(total_label_pix, C);
    return EXCEL_OK;
}

template <int D>
static int crf_build(const CrfLattice& L, const unsigned char* rgb, const int* tab, int B, long long N, int H, int W, float sxy, float srgb,
                     hipStream_t st) {
    hipMemsetAsync(L.table, 0xFF, 4ull * (L.mask + 1), st);
    hipMemsetAsync(L.counter, 0, 4, st);
    hipLaunchKernelGGL(crf_lattice_kernel<D>, dim3((unsigned)cdivl(N, 256)), dim3(256), 0, st, rgb, tab, B, N, H, W, sxy, srgb, L.keys, L.bary);
    hipLaunchKernelGGL(crf_hash_insert_kernel, dim3((unsigned)cdivl(L.npv, 256)), dim3(256), 0, st, L.keys, L.npv, L.table, L.mask, L.rep, L.latidx, L.counter, L.lkeys);
    hipLaunchKernelGGL(crf_offsets_kernel, dim3((unsigned)cdivl(L.npv, 256)), dim3(256), 0, st, L.rep, L.latidx, L.npv, L.offset);
    hipLaunchKernelGGL(crf_neighbors_kernel<D>, dim3((unsigned)cdivl(L.npv * (D + 1), 256)), dim3(256), 0, st, L.lkeys, L.counter, L.keys, L.table, L.mask,
                       L.latidx, L.nbr, L.npv);
    EXCEL_CHECK_LAUNCH("dcrf lattice build");
    return EXCEL_OK;
}

// The vertex lists live in tables that are dead once the neighbours are found: cnt / fill in lkeys (4 ints per vertex), start in latidx,
// the list in keys, the segment cursor in table[0].  No workspace of their own.
static int crf_csr_build(const CrfLattice& L, CrfSide& s, hipStream_t st) {
    int *cnt = (int*)L.lkeys, *fill = cnt + L.npv, *start = L.latidx, *list = (int*)L.keys, *cursor = L.table;
    hipMemsetAsync(cnt, 0, 8ull * L.npv, st);
    hipMemsetAsync(cursor, 0, 4, st);
    const unsigned gv = (unsigned)cdivl(L.npv, 256);
    hipLaunchKernelGGL(crf_csr_count_kernel, dim3(gv), dim3(256), 0, st, L.offset, L.npv, cnt);
    hipLaunchKernelGGL(crf_csr_start_kernel, dim3(gv), dim3(256), 0, st, cnt, L.counter, cursor, start);
    hipLaunchKernelGGL(crf_csr_fill_kernel, dim3(gv), dim3(256), 0, st, L.offset, L.npv, start, fill, list);
    EXCEL_CHECK_LAUNCH("dcrf vertex lists");
    s.seg_start = start; s.seg_cnt = cnt; s.seg_list = list;
    return EXCEL_OK;
}

// messages of BOTH kernels for `in` [N,C]: splat, blur passes; the caller slices (crf_make_norm2 / crf_update)
template <bool LAM>
static int crf_pass(const CrfSide& g, const CrfSide& b, const float* in, int use_norm, int C, hipStream_t st) {
    const long long work = (g.npv + b.npv) * C;
    const unsigned gm = (unsigned)(cdivl(work, 256) < 4096 ? cdivl(work, 256) : 4096);      // grid-stride kernels
    hipLaunchKernelGGL(crf_splat2_kernel<LAM>, dim3(gm), dim3(256), 0, st, in, use_norm, g, b, C);
    const int passes = g.Dp1 > b.Dp1 ? g.Dp1 : b.Dp1;
    for (int j = 0; j < passes; ++j) hipLaunchKernelGGL(crf_blur2_kernel<LAM>, dim3(gm), dim3(256), 0, st, g, b, j, C);
    EXCEL_CHECK_LAUNCH("dcrf message passing");
    return EXCEL_OK;
}

struct CrfParams { int iters; float pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std; };

// The one chain of launches behind all entries: N pixels = one image (tab == nullptr, H x W) or a group of B images (tab).  LAM: the
// group's images have their own class counts (lam.nchan), C = the group's largest = the stride of the value rows.
template <bool LAM>
static int crf_run(const unsigned char* rgb_hwc, const float* prob, int prob_is_energy, const int* tab, int B, long long N, int H, int W, int C,
                   const CrfParams& P, float* q_out, unsigned char* labels, void* workspace, hipStream_t st, const CrfLam& lam = CrfLam{}) {
    static_assert(true, "the message-passing kernels are written for the D = 2 (Gaussian) and D = 5 (bilateral) lattices of DenseCRF2D");
    const int iters = P.iters;
    CrfWs w = crf_ws_layout(N, C, LAM, workspace);
    const CrfLattice &Lg = w.Lg, &Lb = w.Lb;
    CrfSide &sg = w.sg, &sb = w.sb;
    float *Q = w.Q, *ones = w.ones;
    TRY(crf_build<2>(Lg, rgb_hwc, tab, B, N, H, W, P.pos_xy_std, 1.f, st));
    TRY(crf_build<5>(Lb, rgb_hwc, tab, B, N, H, W, P.bi_xy_std, P.bi_rgb_std, st));
    if (LAM) {                                                  // before the CSR build takes lkeys over
        hipLaunchKernelGGL(crf_point_classes_kernel, dim3((unsigned)cdivl(Lg.npv, 256)), dim3(256), 0, st, Lg.lkeys, Lg.counter, lam.nchan, B, C, w.cg);
        hipLaunchKernelGGL(crf_point_classes_kernel, dim3((unsigned)cdivl(Lb.npv, 256)), dim3(256), 0, st, Lb.lkeys, Lb.counter, lam.nchan, B, C, w.cb);
        EXCEL_CHECK_LAUNCH("dcrf point classes");
    }
    TRY(crf_csr_build(Lg, sg, st));
    TRY(crf_csr_build(Lb, sb, st));
    // the accumulators are cleared once; every message pass leaves them cleared (blur pass 1)
    hipMemsetAsync(sg.acc, 0, 8ull * Lg.npv * C, st);
    hipMemsetAsync(sb.acc, 0, 8ull * Lb.npv * C, st);
    {
        const float one = 1.0f;
        unsigned pattern;
        memcpy(&pattern, &one, 4);
        hipMemsetD32Async((hipDeviceptr_t)ones, (int)pattern, (size_t)N, st);
    }
    const unsigned gn = (unsigned)cdivl(N, 256);
    // normalisers: norm = 1 / sqrt(K 1 + 1e-20)
    TRY(crf_pass<false>(sg, sb, ones, 0, 1, st));               // (one value per point: every image has it)
    hipLaunchKernelGGL(crf_make_norm2_kernel, dim3(gn), dim3(256), 0, st, sg, sb, N, Lg.norm, Lb.norm);
    hipLaunchKernelGGL(crf_update_kernel<LAM>, dim3(gn), dim3(256), 0, st, prob, prob_is_energy, tab, B, N, C, 0, sg, 0.f, sb, 0.f, Q,
                       iters == 0 ? q_out : nullptr, iters == 0 ? labels : nullptr, lam);
    for (int it = 0; it < iters; ++it) {
        TRY(crf_pass<LAM>(sg, sb, Q, 1, C, st));
        const bool last = it == iters - 1;
        hipLaunchKernelGGL(crf_update_kernel<LAM>, dim3(gn), dim3(256), 0, st, prob, prob_is_energy, tab, B, N, C, 1, sg, P.pos_w, sb, P.bi_w, Q,
                           last ? q_out : nullptr, last ? labels : nullptr, lam);
    }
    EXCEL_CHECK_LAUNCH("dcrf mean field");
    return EXCEL_OK;
}

extern "C" int excel_dcrf_inference(const unsigned char* rgb_hwc, const float* prob, int prob_is_energy, int H, int W, int C, int iters, float pos_w,
                                    float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, float* q_out, void* workspace, void* stream) {
    EXCEL_CHECK_ARG(rgb_hwc && prob && q_out && workspace && H > 0 && W > 0 && C >= 1 && iters >= 0, "dcrf_inference: bad argument");
    EXCEL_CHECK_ALIGN(workspace, 8, "dcrf_inference", "workspace");                 // 64-bit fixed-point accumulators
    EXCEL_CHECK_ARG(pos_xy_std > 0.f && bi_xy_std > 0.f && bi_rgb_std > 0.f, "dcrf_inference: standard deviations must be positive");
    const CrfParams P{iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std};
    return crf_run<false>(rgb_hwc, prob, prob_is_energy, nullptr, 1, (long long)H * W, H, W, C, P, q_out, nullptr, workspace, (hipStream_t)stream);
}

// tools/infer_seg_voc.py:103-174 (crf_proc), tools/infer_seg_coco.py:144-145 and utils/dcrf.py:42-68 for a group of images at once
extern "C" int excel_dcrf_inference_ragged(const uint8_t* hwc, const float* unary, int unary_is_energy, const int32_t* table,
                                           const excel_ragged_info* info, int C, int iters, float pos_w, float pos_xy_std, float bi_w,
                                           float bi_xy_std, float bi_rgb_std, uint8_t* labels_u8, float* q_out, void* workspace, void* stream) {
    EXCEL_CHECK_ARG(hwc && unary && table && info && workspace, "dcrf_inference_ragged: null argument");
    EXCEL_CHECK_ALIGN(workspace, 8, "dcrf_inference_ragged", "workspace");          // 64-bit fixed-point accumulators
    EXCEL_CHECK_ARG(labels_u8 || q_out, "dcrf_inference_ragged: ask for labels, Q or both");
    EXCEL_CHECK_ARG(info->B > 0 && info->B <= CRF_MAX_IMAGES, "dcrf_inference_ragged: %d images, need 1..%d", info->B, CRF_MAX_IMAGES);
    EXCEL_CHECK_ARG(C >= 1 && iters >= 0, "dcrf_inference_ragged: need C >= 1 and iters >= 0");
    EXCEL_CHECK_ARG(!labels_u8 || C <= 256, "dcrf_inference_ragged: uint8 labels need C <= 256 (C = %d)", C);
    EXCEL_CHECK_ARG(pos_xy_std > 0.f && bi_xy_std > 0.f && bi_rgb_std > 0.f, "dcrf_inference_ragged: standard deviations must be positive");
    EXCEL_CHECK_ARG(crf_fits(info->total_label_pix), "dcrf_inference_ragged: a group of %lld pixels has more lattice vertices (6 per pixel) than "
                    "the 32-bit vertex indices hold: split it (ops.dcrf_groups)", (long long)info->total_label_pix);
    const CrfParams P{iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std};
    return crf_run<false>(hwc, unary, unary_is_energy, table, info->B, info->total_label_pix, 0, 0, C, P, q_out, labels_u8, workspace, (hipStream_t)stream);
}

// tools/infer_lam.py:179-237 (crf_proc) for a group of LAMs with their own class counts, on the step's cams where they lie
static int crf_lam_counts(const int32_t* nchan_host, int B, int Cmax, const char* who, int* Cg) {
    int mx = 0;
    for (int b = 0; b < B; ++b) {
        EXCEL_CHECK_ARG(nchan_host[b] >= 1 && (Cmax <= 0 || nchan_host[b] <= Cmax), "%s: image %d has %d classes, need 1..%d", who, b,
                        (int)nchan_host[b], Cmax > 0 ? Cmax : 2147483647);
        if (nchan_host[b] > mx) mx = nchan_host[b];
    }
    *Cg = mx;
    return EXCEL_OK;
}

extern "C" int excel_dcrf_lam_ragged_workspace_bytes(const int32_t* hw, const int32_t* nchan, int B, size_t* bytes) {
    EXCEL_CHECK_ARG(hw && nchan && bytes && B >= 1 && B <= CRF_MAX_IMAGES, "dcrf_lam_ragged_workspace_bytes: bad argument");
    long long N = 0;
    for (int b = 0; b < B; ++b) {
        EXCEL_CHECK_ARG(hw[2 * b] >= 1 && hw[2 * b + 1] >= 1, "dcrf_lam_ragged_workspace_bytes: image %d has size %d x %d", b, (int)hw[2 * b], (int)hw[2 * b + 1]);
        N += (long long)hw[2 * b] * hw[2 * b + 1];
    }
    int Cg = 0;
    TRY(crf_lam_counts(nchan, B, 0, "dcrf_lam_ragged_workspace_bytes", &Cg));
    EXCEL_CHECK_ARG(crf_fits(N), "dcrf_lam_ragged_workspace_bytes: a group of %lld pixels has more lattice vertices (6 per pixel) than "
                    "the 32-bit vertex indices hold: split it (ops.dcrf_lam_groups)", N);
    *bytes = crf_lam_workspace_bytes(N, Cg);
    return EXCEL_OK;
}

extern "C" int excel_dcrf_lam_ragged(const uint8_t* hwc, const float* cams, const int32_t* nchan, const int32_t* nchan_host, const int32_t* cls_idx,
                                     const int32_t* table, const excel_ragged_info* info, int smax, int Cmax, int iters, float pos_w,
                                     float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, uint8_t* labels_u8, float* q_out,
                                     void* workspace, void* stream) {
    EXCEL_CHECK_ARG(hwc && cams && nchan && nchan_host && table && info && workspace, "dcrf_lam_ragged: null argument");
    EXCEL_CHECK_ALIGN(workspace, 8, "dcrf_lam_ragged", "workspace");                // 64-bit fixed-point accumulators
    EXCEL_CHECK_ARG(labels_u8 || q_out, "dcrf_lam_ragged: ask for labels, Q or both");
    EXCEL_CHECK_ARG(info->B > 0 && info->B <= CRF_MAX_IMAGES, "dcrf_lam_ragged: %d images, need 1..%d", info->B, CRF_MAX_IMAGES);
    EXCEL_CHECK_ARG(Cmax >= 1 && iters >= 0, "dcrf_lam_ragged: need Cmax >= 1 and iters >= 0");
    EXCEL_CHECK_ARG(!cls_idx || (smax >= 1 && Cmax <= smax + 1), "dcrf_lam_ragged: cls_idx rows of %d entries cannot map %d channels", smax, Cmax);
    EXCEL_CHECK_ARG(!labels_u8 || Cmax <= 256, "dcrf_lam_ragged: uint8 labels need Cmax <= 256 (Cmax = %d)", Cmax);
    EXCEL_CHECK_ARG(pos_xy_std > 0.f && bi_xy_std > 0.f && bi_rgb_std > 0.f, "dcrf_lam_ragged: standard deviations must be positive");
    EXCEL_CHECK_ARG(crf_fits(info->total_label_pix), "dcrf_lam_ragged: a group of %lld pixels has more lattice vertices (6 per pixel) than "
                    "the 32-bit vertex indices hold: split it (ops.dcrf_lam_groups)", (long long)info->total_label_pix);
    int Cg = 0;
    TRY(crf_lam_counts(nchan_host, info->B, Cmax, "dcrf_lam_ragged", &Cg));
    const CrfParams P{iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std};
    const CrfLam lam{nchan, cls_idx, smax, Cmax};
    return crf_run<true>(hwc, cams, 0, table, info->B, info->total_label_pix, 0, 0, Cg, P, q_out, labels_u8, workspace, (hipStream_t)stream, lam);
}
