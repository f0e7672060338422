// Training-progress image panels (include/excel_hip.h, "training-progress panels"): the six grids scripts/train_voc.py:233-246 hands to
// TensorBoard every --log_iters iterations (utils/tbutils.py:28-61, :88-93), for one training batch in ONE launch.
//
//   img1      tbutils.denormalize_img(inputs)                                   (uint8) (((x * std_c) + mean_c) * 255), float32
//   cam1      jet(max_f(bilinear(attr_maps_raw as [B,F,g,g]) * cls_label)) * 255 * 0.5 + img1 * 0.5, truncated, float64
//   pseu_aff, seg_gt, seg_pred   [B,S,S] uint8 label maps through the VOC palette
//   pseu_mid  the same for a [B,g,g] label map
//
// each laid out as torchvision.utils.make_grid(nrow) lays a batch out: cells of (h+2) x (w+2), a 2-pixel frame, zeros between the
// images and in the cells past B; B == 1 is the bare image.  The kernel writes EVERY byte of every panel (the zeros too), so the output
// buffer needs no clearing.  The up-sampled class planes never reach memory: each pixel blends its four taps of every class in registers.
//
// Memory-bound and small (about 7.5 MB out at S = 320, B = 4), camviz.hip's shape: the jet table (6 KB) and the palette in LDS once per
// workgroup, workgroups loop over 64 x 16 tiles of all panels, one lane per grid column so a wave stores 192 consecutive bytes.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"
#include "jet.h"

#define TV_PANELS EXCEL_TRAIN_PANELS

struct TvPanel { int Hg, Wg, h, tile0, ntx; long long off; };     // h: side of one image of the grid (S, or g for pseu_mid)
struct TvArgs {
    TvPanel p[TV_PANELS];          // in tile order; unrequested panels: tile0 = ntiles (no tile selects them)
    const float* img; const float* attr; const float* cls;
    const uint8_t* lab[TV_PANELS]; // label map of the palette panels (null for img1 / cam1)
    const double* jet; const uint8_t* palette; uint8_t* out;
    int B, F, g, S, xmaps, pad, ntiles;
    float mean[3], std[3];
};

// tbutils.denormalize_img for one value: float32, no contraction; the conversion truncates (clamped: the reference's is undefined outside)
__device__ __forceinline__ int tv_denorm(float x, float mean, float std) {
#pragma clang fp contract(off)
    const float v = ((x * std) + mean) * 255.f;
    return (int)fminf(fmaxf(v, 0.f), 255.f);
}

__global__ __launch_bounds__(256) void train_panels_kernel(TvArgs a) {
#pragma clang fp contract(off)
    __shared__ double lut[(CAMVIZ_LUT + 1) * 3];    // [idx][ch] = 0.5 * (jet * 255); entry 256 = bad = 0
    __shared__ uint8_t pal[768];
    for (int i = threadIdx.x; i < 768; i += 256) {
        lut[i] = a.jet[i];
        pal[i] = a.palette[i];
    }
    if (threadIdx.x < 3) lut[CAMVIZ_BAD * 3 + threadIdx.x] = 0.0;
    __syncthreads();
    const long long SS = (long long)a.S * a.S;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        // the panel of this tile: panels are in tile order, constant indices after unrolling (no dynamically indexed argument array)
        int kind = 0;
        TvPanel P = a.p[0];
        const uint8_t* lab = a.lab[0];
#pragma unroll
        for (int k = 1; k < TV_PANELS; ++k)
            if (tile >= a.p[k].tile0) { kind = k; P = a.p[k]; lab = a.lab[k]; }
        const int t = tile - P.tile0;
        const int ty = t / P.ntx;
        const int gx = (t - ty * P.ntx) * 64 + (threadIdx.x & 63);
        if (gx >= P.Wg) continue;
        const int cell = P.h + a.pad;
        const int ux = gx - a.pad;
        const int cc = ux >= 0 ? ux / cell : 0;
        const int ix = ux - cc * cell;
        uint8_t* ob = a.out + P.off;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gy = ty * 16 + (threadIdx.x >> 6) + 4 * r;
            if (gy >= P.Hg) continue;
            const int uy = gy - a.pad;
            const int cr = uy >= 0 ? uy / cell : 0;
            const int iy = uy - cr * cell;
            const int b = cr * a.xmaps + cc;
            int c0 = 0, c1 = 0, c2 = 0;
            if (ux >= 0 && uy >= 0 && ix < P.h && iy < P.h && b < a.B) {
                if (kind >= 2) {
                    const int j = 3 * lab[((long long)b * P.h + iy) * P.h + ix];
                    c0 = pal[j]; c1 = pal[j + 1]; c2 = pal[j + 2];
                } else {
                    const float* ip = a.img + (long long)b * 3 * SS + (long long)iy * a.S + ix;
                    c0 = tv_denorm(ip[0], a.mean[0], a.std[0]);
                    c1 = tv_denorm(ip[SS], a.mean[1], a.std[1]);
                    c2 = tv_denorm(ip[2 * SS], a.mean[2], a.std[2]);
                    if (kind == 1) {
                        // F.interpolate(bilinear, align_corners=False) of plane f at this pixel, times cls_label[b, f]; torch.max over f
                        const BilinearTap tp = bilinear_tap(ix, iy, a.g, a.g, a.S, a.S, 0);
                        const float* ab = a.attr + (long long)b * a.g * a.g * a.F;          // [P, F]: class f of patch p at p * F + f
                        const float* q00 = ab + (long long)(tp.y0 * a.g + tp.x0) * a.F;
                        const float* q01 = ab + (long long)(tp.y0 * a.g + tp.x1) * a.F;
                        const float* q10 = ab + (long long)(tp.y1 * a.g + tp.x0) * a.F;
                        const float* q11 = ab + (long long)(tp.y1 * a.g + tp.x1) * a.F;
                        const float* cl = a.cls + (long long)b * a.F;
                        float m = bilinear_blend(tp, q00[0], q01[0], q10[0], q11[0]) * cl[0];
                        for (int f = 1; f < a.F; ++f) {
                            const float v = bilinear_blend(tp, q00[f], q01[f], q10[f], q11[f]) * cl[f];
                            m = (v > m || isnan(v)) ? v : m;
                        }
                        const int j = 3 * jet_index(m);
                        c0 = (int)(lut[j] + 0.5 * (double)c0);
                        c1 = (int)(lut[j + 1] + 0.5 * (double)c1);
                        c2 = (int)(lut[j + 2] + 0.5 * (double)c2);
                    }
                }
            }
            uint8_t* op = ob + 3 * ((long long)gy * P.Wg + gx);
            op[0] = (uint8_t)c0;
            op[1] = (uint8_t)c1;
            op[2] = (uint8_t)c2;
        }
    }
}

// make_grid's geometry of every requested panel, in panel order; -> total bytes, or -1 when a size leaves the supported range
static long long tv_layout(int B, int nrow, int S, int g, int mask, long long out[3 * TV_PANELS]) {
    const int xmaps = nrow < B ? nrow : B;
    const int ymaps = cdiv(B, xmaps);
    const int pad = B == 1 ? 0 : 2;
    long long off = 0;
    for (int k = 0; k < TV_PANELS; ++k) {
        out[3 * k] = out[3 * k + 1] = out[3 * k + 2] = 0;
        if (!((mask >> k) & 1)) continue;
        const long long h = k == EXCEL_TRAIN_PANEL_PSEU_MID ? g : S;
        const long long Hg = (h + pad) * ymaps + pad, Wg = (h + pad) * xmaps + pad;
        if (Hg >= (1LL << 31) || Wg >= (1LL << 31) || Hg * Wg >= (1LL << 31)) return -1;
        out[3 * k] = Hg; out[3 * k + 1] = Wg; out[3 * k + 2] = off;
        off += 3 * Hg * Wg;
        if (off >= (1LL << 31)) return -1;
    }
    return off;
}

static int tv_check_shape(const char* who, int B, int nrow, int S, int g, int mask) {
    EXCEL_CHECK_ARG(B >= 1 && nrow >= 1 && S >= 1 && g >= 1, "%s: need B, nrow, S, g >= 1 (got %d, %d, %d, %d)", who, B, nrow, S, g);
    EXCEL_CHECK_ARG(mask > 0 && mask < (1 << TV_PANELS), "%s: panel_mask must select some of the %d panels (got %d)", who, TV_PANELS, mask);
    EXCEL_CHECK_ARG(3LL * B * S * S < (1LL << 31), "%s: 3 * B * S * S must stay below 2^31", who);
    return EXCEL_OK;
}

extern "C" int excel_train_panels_plan(int B, int nrow, int S, int g, int panel_mask, int64_t* out) {
    EXCEL_CHECK_ARG(out, "train_panels_plan: null argument");
    const int rc = tv_check_shape("train_panels_plan", B, nrow, S, g, panel_mask);
    if (rc != EXCEL_OK) return rc;
    long long lay[3 * TV_PANELS];
    const long long total = tv_layout(B, nrow, S, g, panel_mask, lay);
    EXCEL_CHECK_ARG(total >= 0, "train_panels_plan: the panels must stay below 2^31 bytes");
    for (int i = 0; i < 3 * TV_PANELS; ++i) out[i] = lay[i];
    out[3 * TV_PANELS] = total;
    return EXCEL_OK;
}

extern "C" int excel_train_panels(const float* img, const float* attr, const float* cls_label, const uint8_t* pseu_aff, const uint8_t* pseu_mid,
                                  const uint8_t* seg_gt, const uint8_t* seg_pred, int B, int F, int P, int g, int S, int nrow, int panel_mask,
                                  const float* mean, const float* std, const double* jet, const uint8_t* palette, uint8_t* out,
                                  size_t out_bytes, void* stream) {
    const int rc = tv_check_shape("train_panels", B, nrow, S, g, panel_mask);
    if (rc != EXCEL_OK) return rc;
    EXCEL_CHECK_ARG(out && palette && jet && mean && std, "train_panels: null argument");
    EXCEL_CHECK_ALIGN(jet, 8, "train_panels", "jet");                       // doubles
    const int m = panel_mask;
    const int want_img = (m >> EXCEL_TRAIN_PANEL_IMG1) & 1, want_cam = (m >> EXCEL_TRAIN_PANEL_CAM1) & 1;
    EXCEL_CHECK_ARG(!(want_img || want_cam) || img, "train_panels: img1 / cam1 requested without the input images");
    EXCEL_CHECK_ARG(!want_cam || (attr && cls_label), "train_panels: cam1 requested without attr_maps_raw / cls_label");
    EXCEL_CHECK_ARG(!want_cam || (F >= 1 && P == g * g), "train_panels: cam1 needs F >= 1 and P == g * g (F %d, P %d, g %d)", F, P, g);
    EXCEL_CHECK_ARG(!want_cam || (long long)B * P * F < (1LL << 31), "train_panels: B * P * F must stay below 2^31");
    const uint8_t* labs[TV_PANELS] = {nullptr, nullptr, pseu_aff, pseu_mid, seg_gt, seg_pred};
    static const char* const names[TV_PANELS] = {"img1", "cam1", "pseu_aff", "pseu_mid", "seg_gt", "seg_pred"};
    for (int k = 2; k < TV_PANELS; ++k)
        EXCEL_CHECK_ARG(!((m >> k) & 1) || labs[k], "train_panels: %s requested without its label map", names[k]);
    long long lay[3 * TV_PANELS];
    const long long total = tv_layout(B, nrow, S, g, m, lay);
    EXCEL_CHECK_ARG(total >= 0, "train_panels: the panels must stay below 2^31 bytes");
    EXCEL_CHECK_ARG((long long)out_bytes >= total, "train_panels: out holds %lld bytes, the panels need %lld", (long long)out_bytes, total);
    TvArgs a = {};
    a.img = img; a.attr = attr; a.cls = cls_label; a.jet = jet; a.palette = palette; a.out = out;
    a.B = B; a.F = F; a.g = g; a.S = S;
    a.xmaps = nrow < B ? nrow : B;
    a.pad = B == 1 ? 0 : 2;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
    long long ntiles = 0;
    for (int k = 0; k < TV_PANELS; ++k) {
        if (!((m >> k) & 1)) continue;
        TvPanel& p = a.p[k];
        p.Hg = (int)lay[3 * k]; p.Wg = (int)lay[3 * k + 1]; p.off = lay[3 * k + 2];
        p.h = k == EXCEL_TRAIN_PANEL_PSEU_MID ? g : S;
        p.ntx = cdiv(p.Wg, 64);
        p.tile0 = (int)ntiles;
        a.lab[k] = labs[k];
        ntiles += (long long)p.ntx * cdiv(p.Hg, 16);
    }
    EXCEL_CHECK_ARG(ntiles < (1LL << 31), "train_panels: too many tiles");
    a.ntiles = (int)ntiles;
    for (int k = 0; k < TV_PANELS; ++k)
        if (!((m >> k) & 1)) { a.p[k].tile0 = a.ntiles; a.p[k].ntx = 1; }
    // a few tiles per workgroup: the table staging is paid once per workgroup, and 2048 workgroups still fill 256 CUs
    const int grid = (int)(ntiles < 2048 ? ntiles : 2048);
    hipLaunchKernelGGL(train_panels_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    EXCEL_CHECK_LAUNCH("train_panels");
    return EXCEL_OK;
}
