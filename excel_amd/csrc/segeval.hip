// Segmentation evaluation over ragged batches (include/excel_hip.h, "segmentation evaluation"): the size-dependent half of
// tools/infer_seg_voc.py / tools/infer_seg_coco.py (_validate :58-91, crf_proc :134-152) for a whole batch of images of different sizes.
//
//   seg_msc_fuse_ragged     every scale's decoder logits -> bilinear to (h_b, w_b) -> flip mean -> mean over scales, in registers:
//                           the operations of a per-image chain of seg_scale_accumulate_kernel (attr.hip), in its order, so the
//                           result is the same bits; optional pitched logits planes and/or tight arg-max labels
//   seg_resize_argmax_ragged pitched planes of one plan -> bilinear to the sizes of a second plan -> arg-max -> tight labels; the
//                           resized nc-class logits never reach memory (bilinear_resize_kernel + argmax_key, same bits)
//   seg_resize_argmax_uniform the same kernel with a tight uniform [B, nc, h, w] source (the decoder's seg logits of one batch)
//   seg_softmax_resize      one image's pitched planes -> (bilinear to (H, W)) -> softmax over classes -> tight [nc,H,W]: the CRF's input
//   seg_softmax_resize_ragged  the same kernel over every image of a batch in one launch (source and target sizes from two plans)
//
// All three are gather-bound: the sources are small (2B * nc * g^2 floats per scale, L2-resident) and each output pixel reads 4 (8 with
// the flip) of them per class and scale.  Tiles are the 64 x 16 pixel tiles of the ragged plan (common.h).
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define SEG_MAX_SCALES 8

struct SegScales {
    const float* segs[SEG_MAX_SCALES];   // [2B, nc, g, g]: image b, then its flipped copy at b + B
    int g[SEG_MAX_SCALES];
    int flip[SEG_MAX_SCALES];
    int ns;
    float last_scale;                    // (float)(1.0 / ns): the mean over scales folded into the last step
};

// One workgroup per 64 x 16 tile; lane (tx, ty) = (tid % 16, tid / 16) owns pixels x0 + 4 tx .. +3 of row y0 + ty, so the pitched
// planes are stored 16 bytes per lane (rows are padded to 4 floats; the pad columns get the value of the clamped sample, which is
// in bounds and never read as a pixel).  The separable bilinear taps of every scale - row taps of the tile's 16 rows, column taps
// of its 64 columns and of their mirror images W-1-x - are computed once per tile into LDS; the class loop then only gathers and
// blends.  The taps and the blend are seg_scale_accumulate_kernel's (linear_tap, bilinear_blend) and the steps around the sample
// are written as there, with contraction off so that nothing fuses across them: the GPU tests pin this kernel to the chain of
// seg_scale_accumulate calls bit for bit.
__global__ __launch_bounds__(256) void seg_msc_fuse_ragged_kernel(SegScales sc, int B, int nc, TileGeo geo, float* __restrict__ planes,
                                                                  unsigned char* __restrict__ labels) {
#pragma clang fp contract(off)
    __shared__ int cx0[SEG_MAX_SCALES][64], cx1[SEG_MAX_SCALES][64], fx0[SEG_MAX_SCALES][64], fx1[SEG_MAX_SCALES][64];
    __shared__ float clx[SEG_MAX_SCALES][64], flx[SEG_MAX_SCALES][64];
    __shared__ int ry0[SEG_MAX_SCALES][16], ry1[SEG_MAX_SCALES][16];
    __shared__ float rly[SEG_MAX_SCALES][16];
    const Tile t = tile_of<true>(geo);
    const int tid = threadIdx.x;
#pragma unroll
    for (int s = 0; s < SEG_MAX_SCALES; ++s) {
        if (s < sc.ns) {
            const int g = sc.g[s];
            if (tid < 64) {
                // the column taps of x and of the mirrored W - 1 - x
                const int x = t.x0 + tid;
                const LinearTap c = linear_tap(x, g, t.W, 0), f = linear_tap(t.W - 1 - x, g, t.W, 0);
                cx0[s][tid] = c.i0; cx1[s][tid] = c.i1; clx[s][tid] = c.l;
                fx0[s][tid] = f.i0; fx1[s][tid] = f.i1; flx[s][tid] = f.l;
            } else if (tid < 80) {
                const int r = tid - 64;
                const LinearTap ry = linear_tap(t.y0 + r, g, t.H, 0);
                ry0[s][r] = ry.i0 * g; ry1[s][r] = ry.i1 * g; rly[s][r] = ry.l;
            }
        }
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    const int y = t.y0 + ty, xb = t.x0 + 4 * tx;
    if (y >= t.H || xb >= t.Wp) return;
    float* prow = planes ? planes + (long long)nc * t.base + (long long)y * t.Wp + xb : nullptr;
    float best[4];
    int bi[4];
    for (int c = 0; c < nc; ++c) {
        float acc[4];
#pragma unroll
        for (int s = 0; s < SEG_MAX_SCALES; ++s) {
            if (s < sc.ns) {
                const int g = sc.g[s];
                const long long pl = (long long)t.b * nc + c;
                const float* m = sc.segs[s] + pl * g * g;
                const float* mf = sc.segs[s] + (pl + (long long)B * nc) * g * g;
                const int y0 = ry0[s][ty], y1 = ry1[s][ty];
                const float ly = rly[s][ty];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int col = 4 * tx + k;
                    // seg_scale_accumulate_kernel: sample(plane, x), then (v + sample(plane + B*nc, W-1-x)) / 2 where flip_mean is set
                    const int a0 = cx0[s][col], a1 = cx1[s][col];
                    float v = bilinear_blend(ly, clx[s][col], m[y0 + a0], m[y0 + a1], m[y1 + a0], m[y1 + a1]);
                    if (sc.flip[s]) {
                        const int b0 = fx0[s][col], b1 = fx1[s][col];
                        v = (v + bilinear_blend(ly, flx[s][col], mf[y0 + b0], mf[y0 + b1], mf[y1 + b0], mf[y1 + b1])) * 0.5f;
                    }
                    v = s == 0 ? v : acc[k] + v;
                    acc[k] = v * (s == sc.ns - 1 ? sc.last_scale : 1.f);
                }
            }
        }
        if (prow) *(f32x4*)(prow + (long long)c * t.HW) = f32x4{acc[0], acc[1], acc[2], acc[3]};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c == 0 || acc[k] > best[k]) { best[k] = acc[k]; bi[k] = c; }     // first maximum, like argmax_key (par.hip)
    }
    if (labels) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (xb + k < t.W) labels[t.lab + (long long)y * t.W + xb + k] = (unsigned char)bi[k];
    }
}

// Tiles of the DESTINATION plan; one lane per column, four rows per lane (argmax_label_ragged_kernel's shape).  The source image b is
// read through `sg`: with a table, record b of the source plan (pitched planes); without one (sg.tab == nullptr), image b of a TIGHT
// uniform [B, nc, sg.H, sg.W] tensor - the decoder's seg logits as they are, whatever g is (TileGeo's uniform convention, Wp = W).
// Per pixel: bilinear_tap once, then bilinear_blend + running arg-max over the classes.
__global__ __launch_bounds__(256) void seg_resize_argmax_ragged_kernel(const float* __restrict__ src, TileGeo sg, int nc,
                                                                       TileGeo dst, unsigned char* __restrict__ labels) {
    const Tile t = tile_of<true>(dst);
    const int x = t.x0 + (threadIdx.x & 63);
    if (x >= t.W) return;
    int h, w, wp;
    long long off;
    if (sg.tab) {
        const int* rec = sg.tab + EXCEL_RAG_REC * t.b;
        h = rec[0]; w = rec[1]; wp = (w + 3) & ~3;
        off = rec[2];
    } else {
        h = sg.H; w = sg.W; wp = w;
        off = (long long)t.b * h * w;
    }
    const long long hw = (long long)h * wp;
    const float* base = src + (long long)nc * off;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = t.y0 + (threadIdx.x >> 6) + 4 * r;
        if (y >= t.H) continue;
        const BilinearTap tp = bilinear_tap(x, y, h, w, t.H, t.W, 0);
        const int o00 = tp.y0 * wp + tp.x0, o01 = tp.y0 * wp + tp.x1, o10 = tp.y1 * wp + tp.x0, o11 = tp.y1 * wp + tp.x1;
        float best = 0.f;
        int bi = 0;
        for (int c = 0; c < nc; ++c) {
            const float* p = base + (long long)c * hw;
            const float v = bilinear_blend(tp, p[o00], p[o01], p[o10], p[o11]);
            if (c == 0 || v > best) { best = v; bi = c; }
        }
        labels[t.lab + (long long)y * t.W + x] = (unsigned char)bi;
    }
}

// One lane per output pixel; three passes over the classes (max, sum of exp, store) re-gather the (L2-resident) source instead of
// holding nc values in registers.  dtab == nullptr: one image, (h, w) -> (H, W).  Otherwise pixel i of the tight pixels of the target
// plan `dtab` (B images): its image's sizes and offsets come from record b of the two plans (source planes at nc * poff_b, target
// [nc, H_b, W_b] at nc * loff_b).
__global__ __launch_bounds__(256) void seg_softmax_resize_kernel(const float* __restrict__ src, const int* __restrict__ stab,
                                                                 const int* __restrict__ dtab, int B, long long total, int h, int w, int nc, int H,
                                                                 int W, float* __restrict__ prob) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (dtab) {
        const int b = ragged_image_of_pixel(dtab, B, i);
        const int *sr = stab + EXCEL_RAG_REC * b, *dr = dtab + EXCEL_RAG_REC * b;
        h = sr[0]; w = sr[1]; H = dr[0]; W = dr[1];
        src += (long long)nc * sr[2];
        prob += (long long)nc * dr[4];
        i -= dr[4];
    }
    const long long HW = (long long)H * W;
    const int x = (int)(i % W), y = (int)(i / W);
    const int wp = (w + 3) & ~3;
    const long long hw = (long long)h * wp;
    const bool same = h == H && w == W;
    const BilinearTap tp = bilinear_tap(x, y, h, w, H, W, 0);
    const int o00 = same ? y * wp + x : tp.y0 * wp + tp.x0, o01 = tp.y0 * wp + tp.x1, o10 = tp.y1 * wp + tp.x0, o11 = tp.y1 * wp + tp.x1;
    auto val = [&](int c) {
        const float* p = src + (long long)c * hw;
        return same ? p[o00] : bilinear_blend(tp, p[o00], p[o01], p[o10], p[o11]);
    };
    float m = -INFINITY;
    for (int c = 0; c < nc; ++c) m = fmaxf(m, val(c));
    float sum = 0.f;
    for (int c = 0; c < nc; ++c) sum += expf(val(c) - m);
    const float inv = 1.f / sum;
    for (int c = 0; c < nc; ++c) prob[(long long)c * HW + i] = expf(val(c) - m) * inv;
}

static const long long kI32 = 2147483647ll;

extern "C" int excel_seg_msc_fuse_ragged(const float* const* segs, const int32_t* g, const int32_t* flip_mean, int ns, int nc, const int32_t* table,
                                         const excel_ragged_info* info, float* planes, uint8_t* labels_u8, void* stream) {
    EXCEL_CHECK_ARG(segs && g && flip_mean && table && info && (planes || labels_u8), "seg_msc_fuse_ragged: null argument");
    EXCEL_CHECK_ARG(ns >= 1 && ns <= SEG_MAX_SCALES, "seg_msc_fuse_ragged: ns = %d outside [1, %d]", ns, SEG_MAX_SCALES);
    EXCEL_CHECK_ARG(nc >= 1 && info->B >= 1, "seg_msc_fuse_ragged: need nc >= 1 and B >= 1");
    EXCEL_CHECK_ARG(!labels_u8 || nc <= 256, "seg_msc_fuse_ragged: uint8 labels need nc <= 256 (nc = %d)", nc);
    EXCEL_CHECK_ARG(!planes || (long long)nc * info->total_pix <= kI32, "seg_msc_fuse_ragged: nc * total_pix must stay below 2^31");
    EXCEL_CHECK_ARG(!planes || ((uintptr_t)planes & 15) == 0, "seg_msc_fuse_ragged: planes must be 16-byte aligned");
    SegScales sc;
    memset(&sc, 0, sizeof(sc));
    sc.ns = ns;
    sc.last_scale = (float)(1.0 / ns);
    for (int s = 0; s < ns; ++s) {
        EXCEL_CHECK_ARG(segs[s] && g[s] >= 1, "seg_msc_fuse_ragged: scale %d: null map or g < 1", s);
        EXCEL_CHECK_ARG(2ll * info->B * nc * g[s] * g[s] <= kI32, "seg_msc_fuse_ragged: scale %d: 2B * nc * g^2 must stay below 2^31", s);
        sc.segs[s] = segs[s];
        sc.g[s] = g[s];
        sc.flip[s] = flip_mean[s] ? 1 : 0;
    }
    if (info->total_tiles == 0) return EXCEL_OK;
    TileGeo geo;
    geo.tab = table; geo.B = info->B; geo.H = geo.W = 0;
    hipLaunchKernelGGL(seg_msc_fuse_ragged_kernel, dim3(info->total_tiles), dim3(256), 0, ST(stream), sc, info->B, nc, geo, planes, labels_u8);
    EXCEL_CHECK_LAUNCH("seg_msc_fuse_ragged");
    return EXCEL_OK;
}

extern "C" int excel_seg_resize_argmax_ragged(const float* planes, const int32_t* src_table, const excel_ragged_info* src_info,
                                              const int32_t* dst_table, const excel_ragged_info* dst_info, int nc, uint8_t* labels_u8,
                                              void* stream) {
    EXCEL_CHECK_ARG(planes && src_table && src_info && dst_table && dst_info && labels_u8, "seg_resize_argmax_ragged: null argument");
    EXCEL_CHECK_ARG(nc >= 1 && nc <= 256, "seg_resize_argmax_ragged: need 1 <= nc <= 256 (nc = %d)", nc);
    EXCEL_CHECK_ARG(src_info->B == dst_info->B && src_info->B >= 1, "seg_resize_argmax_ragged: the two plans hold %d and %d images",
                    src_info->B, dst_info->B);
    EXCEL_CHECK_ARG((long long)nc * src_info->total_pix <= kI32, "seg_resize_argmax_ragged: nc * total_pix must stay below 2^31");
    if (dst_info->total_tiles == 0) return EXCEL_OK;
    TileGeo dst;
    dst.tab = dst_table; dst.B = dst_info->B; dst.H = dst.W = 0;
    TileGeo src;
    src.tab = src_table; src.B = src_info->B; src.H = src.W = 0;
    hipLaunchKernelGGL(seg_resize_argmax_ragged_kernel, dim3(dst_info->total_tiles), dim3(256), 0, ST(stream), planes, src, nc, dst, labels_u8);
    EXCEL_CHECK_LAUNCH("seg_resize_argmax_ragged");
    return EXCEL_OK;
}

extern "C" int excel_seg_resize_argmax_uniform(const float* segs, int B, int h, int w, int nc, const int32_t* dst_table,
                                               const excel_ragged_info* dst_info, uint8_t* labels_u8, void* stream) {
    EXCEL_CHECK_ARG(segs && dst_table && dst_info && labels_u8, "seg_resize_argmax_uniform: null argument");
    EXCEL_CHECK_ARG(nc >= 1 && nc <= 256, "seg_resize_argmax_uniform: need 1 <= nc <= 256 (nc = %d)", nc);
    EXCEL_CHECK_ARG(h >= 1 && w >= 1, "seg_resize_argmax_uniform: source planes of %d x %d", h, w);
    EXCEL_CHECK_ARG(B == dst_info->B && B >= 1, "seg_resize_argmax_uniform: %d source images, the plan holds %d", B, dst_info->B);
    EXCEL_CHECK_ARG((long long)B * nc * h * w <= kI32, "seg_resize_argmax_uniform: B * nc * h * w must stay below 2^31");
    if (dst_info->total_tiles == 0) return EXCEL_OK;
    TileGeo src, dst;
    src.tab = nullptr; src.B = B; src.H = h; src.W = w;
    dst.tab = dst_table; dst.B = dst_info->B; dst.H = dst.W = 0;
    hipLaunchKernelGGL(seg_resize_argmax_ragged_kernel, dim3(dst_info->total_tiles), dim3(256), 0, ST(stream), segs, src, nc, dst, labels_u8);
    EXCEL_CHECK_LAUNCH("seg_resize_argmax_uniform");
    return EXCEL_OK;
}

extern "C" int excel_seg_softmax_resize(const float* planes, int h, int w, int nc, int H, int W, float* prob, void* stream) {
    EXCEL_CHECK_ARG(planes && prob, "seg_softmax_resize: null argument");
    EXCEL_CHECK_ARG(nc >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "seg_softmax_resize: bad shape");
    EXCEL_CHECK_ARG((long long)nc * h * ((w + 3) & ~3) <= kI32 && (long long)nc * H * W <= kI32,
                    "seg_softmax_resize: nc * h * Wp and nc * H * W must stay below 2^31");
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(seg_softmax_resize_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST(stream), planes, (const int*)nullptr,
                       (const int*)nullptr, 1, n, h, w, nc, H, W, prob);
    EXCEL_CHECK_LAUNCH("seg_softmax_resize");
    return EXCEL_OK;
}

extern "C" int excel_seg_softmax_resize_ragged(const float* planes, const int32_t* src_table, const excel_ragged_info* src_info,
                                               const int32_t* dst_table, const excel_ragged_info* dst_info, int nc, float* prob, void* stream) {
    EXCEL_CHECK_ARG(planes && src_table && src_info && dst_table && dst_info && prob, "seg_softmax_resize_ragged: null argument");
    EXCEL_CHECK_ARG(nc >= 1, "seg_softmax_resize_ragged: nc >= 1");
    EXCEL_CHECK_ARG(src_info->B == dst_info->B && src_info->B >= 1, "seg_softmax_resize_ragged: the two plans hold %d and %d images",
                    src_info->B, dst_info->B);
    EXCEL_CHECK_ARG((long long)nc * src_info->total_pix <= kI32, "seg_softmax_resize_ragged: nc * total_pix must stay below 2^31");
    const long long n = dst_info->total_label_pix;
    hipLaunchKernelGGL(seg_softmax_resize_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST(stream), planes, src_table, dst_table,
                       dst_info->B, n, 0, 0, nc, 0, 0, prob);
    EXCEL_CHECK_LAUNCH("seg_softmax_resize_ragged");
    return EXCEL_OK;
}
