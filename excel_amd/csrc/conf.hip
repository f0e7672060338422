// Two-threshold pseudo labels with an ignore band over ragged batches (include/excel_hip.h, "confident labels"): the size-dependent
// ends of utils/affutils.py:101-158 (refine_cams_with_bkg_v2) around the PAR pass, for a whole batch of images of different sizes.
//
//   conf_planes_ragged   the step's cams (smax + 1 pitched planes per image, plane 0 never read) -> bilinear to the half plan ->
//                        softmax over [high_thre, m_1 .. m_k] and over [low_thre, m_1 .. m_k]: 2 (k + 1) planes per image, the two
//                        groups back to back, which is what ONE excel_par_forward_ragged refines (nchan2[b] = 2 (k_b + 1))
//   conf_merge_ragged    PAR's 2 (k + 1) planes on the half plan -> per group bilinear to the label size + first-maximum arg-max + key
//                        lookup (bilinear_resize_kernel + argmax_key, same bits) -> the merge of :154-156 and the img_box of :146-149
//
// Both are streaming kernels over the 64 x 16 pixel tiles of the DESTINATION plan (common.h), one lane per column and four rows per
// lane like seg_resize_argmax_ragged_kernel (segeval.hip).  The sources are a quarter (conf_planes: four times) of the destination and
// every pixel gathers 4 values per plane; nothing is staged.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

// Source = record b of the label-size plan, `Cs` planes per image; destination tile = the half plan, `2 Cs` planes per image.
// Pass 1 resizes every class plane ONCE (bilinear_tap + bilinear_blend: excel_bilinear_resize's operations) and parks the value in its
// own slot of the first group; pass 2 reads it back, takes both exponentials and sums them in channel order 0..k; pass 3 divides.
// A lane re-reads only what it wrote itself.  softmax == 0 stops behind pass 1: group one holds [high_thre, m_1 .. m_k] as resized
// (what the tests compare with excel_bilinear_resize bit for bit).
__global__ __launch_bounds__(256) void conf_planes_ragged_kernel(const float* __restrict__ cams, const int* __restrict__ nchan, TileGeo sg,
                                                                 int Cs, float high_thre, float low_thre, int softmax, TileGeo dst,
                                                                 float* __restrict__ out, int* __restrict__ nchan2) {
#pragma clang fp contract(off)
    const Tile t = tile_of<true>(dst);
    const int nch = min(max(nchan[t.b], 1), Cs);                 // k_b + 1
    if (t.x0 == 0 && t.y0 == 0 && threadIdx.x == 0) nchan2[t.b] = 2 * nch;
    const int x = t.x0 + (threadIdx.x & 63);
    if (x >= t.W) return;
    const int* rec = sg.tab + EXCEL_RAG_REC * t.b;
    const int h = rec[0], w = rec[1], wp = (w + 3) & ~3;
    const long long hw = (long long)h * wp;
    const float* base = cams + (long long)Cs * rec[2];
    float* ob = out + 2ll * Cs * t.base;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = t.y0 + (threadIdx.x >> 6) + 4 * r;
        if (y >= t.H) continue;
        const BilinearTap tp = bilinear_tap(x, y, h, w, t.H, t.W, 0);
        const int o00 = tp.y0 * wp + tp.x0, o01 = tp.y0 * wp + tp.x1, o10 = tp.y1 * wp + tp.x0, o11 = tp.y1 * wp + tp.x1;
        float* o = ob + (long long)y * t.Wp + x;
        float mx = -INFINITY;
        for (int c = 1; c < nch; ++c) {
            const float* p = base + (long long)c * hw;
            const float v = bilinear_blend(tp, p[o00], p[o01], p[o10], p[o11]);
            o[(long long)c * t.HW] = v;
            mx = fmaxf(mx, v);
        }
        if (!softmax) {
            o[0] = high_thre;                                    // a resized constant is the constant
            continue;
        }
        const float mh = fmaxf(high_thre, mx), ml = fmaxf(low_thre, mx);
        const float bh = expf(high_thre - mh), bl = expf(low_thre - ml);
        float sh = bh, sl = bl;
        float* ol = o + (long long)nch * t.HW;                   // the low group starts right behind the k + 1 planes of the high one
        for (int c = 1; c < nch; ++c) {
            const float v = o[(long long)c * t.HW];
            const float eh = expf(v - mh), el = expf(v - ml);
            sh += eh;
            sl += el;
            o[(long long)c * t.HW] = eh;
            ol[(long long)c * t.HW] = el;
        }
        o[0] = bh / sh;
        ol[0] = bl / sl;
        for (int c = 1; c < nch; ++c) {
            o[(long long)c * t.HW] = o[(long long)c * t.HW] / sh;
            ol[(long long)c * t.HW] = ol[(long long)c * t.HW] / sl;
        }
    }
}

// Source = record b of the half plan, 2 Cs planes per image (groups of nch = k_b + 1 planes back to back); destination tile = the
// label-size plan.  Per pixel: bilinear_tap once, then per group bilinear_blend + argmax_key's running first maximum and key lookup.
__global__ __launch_bounds__(256) void conf_merge_ragged_kernel(const float* __restrict__ planes, const int* __restrict__ nchan,
                                                                const int* __restrict__ cls_idx, int Smax, TileGeo sg, int Cs,
                                                                const int* __restrict__ img_box, int ignore_index, TileGeo dst,
                                                                unsigned char* __restrict__ labels) {
    const Tile t = tile_of<true>(dst);
    const int x = t.x0 + (threadIdx.x & 63);
    if (x >= t.W) return;
    const int nch = min(max(nchan[t.b], 1), Cs);
    const int* cls_row = cls_idx ? cls_idx + (long long)t.b * Smax : nullptr;
    const int* rec = sg.tab + EXCEL_RAG_REC * t.b;
    const int h = rec[0], w = rec[1], wp = (w + 3) & ~3;
    const long long hw = (long long)h * wp;
    const float* base = planes + 2ll * Cs * rec[2];
    int by0 = 0, by1 = t.H, bx0 = 0, bx1 = t.W;
    if (img_box) { by0 = img_box[4 * t.b]; by1 = img_box[4 * t.b + 1]; bx0 = img_box[4 * t.b + 2]; bx1 = img_box[4 * t.b + 3]; }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = t.y0 + (threadIdx.x >> 6) + 4 * r;
        if (y >= t.H) continue;
        int lab = ignore_index;                                  // outside the box both passes keep ignore_index (:124-127, :146-149)
        if (y >= by0 && y < by1 && x >= bx0 && x < bx1) {
            const BilinearTap tp = bilinear_tap(x, y, h, w, t.H, t.W, 0);
            const int o00 = tp.y0 * wp + tp.x0, o01 = tp.y0 * wp + tp.x1, o10 = tp.y1 * wp + tp.x0, o11 = tp.y1 * wp + tp.x1;
            int key[2];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const float* p = base + (long long)g * nch * hw;
                float best = bilinear_blend(tp, p[o00], p[o01], p[o10], p[o11]);
                int bi = 0;
                for (int c = 1; c < nch; ++c) {
                    const float* q = p + (long long)c * hw;
                    const float v = bilinear_blend(tp, q[o00], q[o01], q[o10], q[o11]);
                    if (v > best) { best = v; bi = c; }          // first maximum wins, like argmax_key (par.hip)
                }
                key[g] = (bi == 0) ? 0 : (cls_row ? cls_row[bi - 1] + 1 : bi);
            }
            // :154-156: lab = lab_h; lab_h == 0 -> ignore_index; lab_h == 0 and lab_l == 0 -> 0
            lab = key[0] != 0 ? key[0] : (key[1] == 0 ? 0 : ignore_index);
        }
        labels[t.lab + (long long)y * t.W + x] = (unsigned char)lab;
    }
}

static const long long kI32 = 2147483647ll;

static int conf_check_plans(const char* who, const excel_ragged_info* src_info, const excel_ragged_info* half_info, int smax) {
    EXCEL_CHECK_ARG(smax >= 1 && smax <= 127, "%s: need 1 <= smax <= 127 (smax = %d)", who, smax);
    EXCEL_CHECK_ARG(src_info->B == half_info->B && src_info->B >= 1, "%s: the two plans hold %d and %d images", who, src_info->B, half_info->B);
    EXCEL_CHECK_ARG((long long)(smax + 1) * src_info->total_pix <= kI32, "%s: (smax + 1) * total_pix of the label-size plan must stay below 2^31", who);
    EXCEL_CHECK_ARG(2ll * (smax + 1) * half_info->total_pix <= kI32, "%s: 2 (smax + 1) * total_pix of the half plan must stay below 2^31", who);
    return EXCEL_OK;
}

extern "C" int excel_conf_planes_ragged(const float* cams, const int32_t* nchan, const int32_t* src_table, const excel_ragged_info* src_info,
                                        const int32_t* half_table, const excel_ragged_info* half_info, int smax, float high_thre,
                                        float low_thre, int softmax, float* planes, int32_t* nchan2, void* stream) {
    EXCEL_CHECK_ARG(cams && nchan && src_table && src_info && half_table && half_info && planes && nchan2, "conf_planes_ragged: null argument");
    int rc = conf_check_plans("conf_planes_ragged", src_info, half_info, smax);
    if (rc) return rc;
    if (half_info->total_tiles == 0) return EXCEL_OK;
    ProfScope prof__(PROF_UPSAMPLE, ST(stream));
    TileGeo src, dst;
    src.tab = src_table; src.B = src_info->B; src.H = src.W = 0;
    dst.tab = half_table; dst.B = half_info->B; dst.H = dst.W = 0;
    hipLaunchKernelGGL(conf_planes_ragged_kernel, dim3(half_info->total_tiles), dim3(256), 0, ST(stream), cams, nchan, src, smax + 1, high_thre,
                       low_thre, softmax ? 1 : 0, dst, planes, nchan2);
    EXCEL_CHECK_LAUNCH("conf_planes_ragged");
    return EXCEL_OK;
}

extern "C" int excel_conf_merge_ragged(const float* planes, const int32_t* nchan, const int32_t* cls_idx, const int32_t* half_table,
                                       const excel_ragged_info* half_info, const int32_t* dst_table, const excel_ragged_info* dst_info, int smax,
                                       const int32_t* img_box, int ignore_index, uint8_t* labels_u8, void* stream) {
    EXCEL_CHECK_ARG(planes && nchan && half_table && half_info && dst_table && dst_info && labels_u8, "conf_merge_ragged: null argument");
    EXCEL_CHECK_ARG(ignore_index >= 0 && ignore_index <= 255, "conf_merge_ragged: ignore_index %d does not fit the uint8 labels", ignore_index);
    int rc = conf_check_plans("conf_merge_ragged", dst_info, half_info, smax);
    if (rc) return rc;
    if (dst_info->total_tiles == 0) return EXCEL_OK;
    ProfScope prof__(PROF_ARGMAX, ST(stream));
    TileGeo src, dst;
    src.tab = half_table; src.B = half_info->B; src.H = src.W = 0;
    dst.tab = dst_table; dst.B = dst_info->B; dst.H = dst.W = 0;
    hipLaunchKernelGGL(conf_merge_ragged_kernel, dim3(dst_info->total_tiles), dim3(256), 0, ST(stream), planes, nchan, cls_idx, smax, src, smax + 1,
                       img_box, ignore_index, dst, labels_u8);
    EXCEL_CHECK_LAUNCH("conf_merge_ragged");
    return EXCEL_OK;
}
