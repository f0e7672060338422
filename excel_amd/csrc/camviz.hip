// CAM overlay images (include/excel_hip.h, "CAM overlay images"): tools/infer_lam.py:97-111 for a whole ragged batch in one launch.
//
//   out = uint8(trunc(alpha * jet(cam) * 255 + (1 - alpha) * denormalize_img(normalize_img(image))))
//
// per output byte, with cam = the max over the k foreground planes (max mode) or each foreground plane (per-class mode).  The host
// pre-scales both terms in float64 exactly as the reference computes them (utils/imutils.jet_lut, denormalize_roundtrip_table), so
// the kernel's arithmetic is one float64 add and a truncation - numpy's `a + b` followed by astype(uint8).
//
// Memory-bound and small: per output pixel one float per plane read, 3 image bytes read, 3 bytes written.  The two 1.5 K-entry tables
// (12 KB) are staged in LDS once per workgroup; workgroups loop over the tiles of the ragged plan (common.h) so a workgroup amortises
// the staging over several tiles.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"
#include "jet.h"

// Tile `tile` of the ragged plan, or of one tight H x W image (geo.tab == nullptr: b = 0, Wp = W, no offsets).
__device__ __forceinline__ Tile camviz_tile(const TileGeo& g, int tile) {
    if (g.tab) return tile_of_ragged(g, tile);
    Tile t;
    const int ntx = (g.W + 63) >> 6;
    const int ty = tile / ntx;
    t.b = 0; t.x0 = (tile - ty * ntx) * 64; t.y0 = ty * 16;
    t.H = g.H; t.W = g.W; t.Wp = g.W;
    t.HW = (long long)g.H * g.W;
    t.base = 0; t.lab = 0;
    return t;
}

// One lane per column, four rows per lane (argmax_label_ragged_kernel's shape): cam loads are 64 consecutive floats per wave, image
// bytes 192 consecutive bytes.  Only x < W_b and planes 1..k_b are read: the pipeline's step buffers hold garbage elsewhere.
__global__ __launch_bounds__(256) void cam_overlay_ragged_kernel(const uint8_t* __restrict__ hwc, const float* __restrict__ cams, int Cmax,
                                                                 const int32_t* __restrict__ ncls, int k_single, const int64_t* __restrict__ out_off,
                                                                 TileGeo geo, int ntiles, int per_class, const double* __restrict__ tabs,
                                                                 uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double lut[(CAMVIZ_LUT + 1) * 3];    // [idx][ch] = alpha * jet * 255; entry 256 = bad = 0
    __shared__ double img[3 * 256];                 // [ch][v]   = (1 - alpha) * denormalize_img(normalize_img(v))
    for (int i = threadIdx.x; i < 2 * 768; i += 256) {
        if (i < 768) lut[i] = tabs[i];
        else img[i - 768] = tabs[i];
    }
    if (threadIdx.x < 3) lut[CAMVIZ_BAD * 3 + threadIdx.x] = 0.0;
    __syncthreads();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const Tile t = camviz_tile(geo, tile);
        const int k = ncls ? ncls[t.b] : k_single;
        const int x = t.x0 + (threadIdx.x & 63);
        if (k <= 0 || x >= t.W) continue;
        const float* cb = cams + (long long)Cmax * t.base;
        const long long HWt = (long long)t.H * t.W;        // tight pixels of image b
        uint8_t* ob = out + (out_off ? out_off[t.b] : 3 * t.lab);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = t.y0 + (threadIdx.x >> 6) + 4 * r;
            if (y >= t.H) continue;
            const long long pix = (long long)y * t.W + x;
            const uint8_t* ip = hwc + 3 * (t.lab + pix);
            const double i0 = img[ip[0]], i1 = img[256 + ip[1]], i2 = img[512 + ip[2]];
            const float* cp = cb + (long long)y * t.Wp + x;
            if (!per_class) {
                // torch.max over the foreground rows (dim 0): NaN propagates
                float m = cp[t.HW];
                for (int c = 2; c <= k; ++c) {
                    const float v = cp[(long long)c * t.HW];
                    m = (v > m || isnan(v)) ? v : m;
                }
                const int j = 3 * jet_index(m);
                uint8_t* op = ob + 3 * pix;
                op[0] = (uint8_t)(int)(lut[j] + i0);
                op[1] = (uint8_t)(int)(lut[j + 1] + i1);
                op[2] = (uint8_t)(int)(lut[j + 2] + i2);
            } else {
                for (int c = 0; c < k; ++c) {
                    const int j = 3 * jet_index(cp[(long long)(c + 1) * t.HW]);
                    uint8_t* op = ob + 3 * ((long long)c * HWt + pix);
                    op[0] = (uint8_t)(int)(lut[j] + i0);
                    op[1] = (uint8_t)(int)(lut[j + 1] + i1);
                    op[2] = (uint8_t)(int)(lut[j + 2] + i2);
                }
            }
        }
    }
}

static int camviz_launch(const uint8_t* hwc, const float* cams, int Cmax, const int32_t* ncls, int k_single, const int64_t* out_off,
                         TileGeo geo, long long ntiles, int mode, const double* tables, uint8_t* out, void* stream) {
    if (ntiles == 0) return EXCEL_OK;
    // a few tiles per workgroup: the 12 KB table staging is paid once per workgroup, and 2048 workgroups still fill 256 CUs
    const int grid = (int)(ntiles < 2048 ? ntiles : 2048);
    hipLaunchKernelGGL(cam_overlay_ragged_kernel, dim3(grid), dim3(256), 0, ST(stream), hwc, cams, Cmax, ncls, k_single, out_off, geo,
                       (int)ntiles, mode == EXCEL_CAM_OVERLAY_PER_CLASS ? 1 : 0, tables, out);
    EXCEL_CHECK_LAUNCH("cam_overlay");
    return EXCEL_OK;
}

extern "C" int excel_cam_overlay_ragged(const uint8_t* hwc, const float* cams, int Cmax, const int32_t* ncls, const int64_t* out_off,
                                        const int32_t* table, const excel_ragged_info* info, int mode, const double* tables, uint8_t* out,
                                        void* stream) {
    EXCEL_CHECK_ARG(hwc && cams && ncls && table && info && tables && out, "cam_overlay_ragged: null argument");
    EXCEL_CHECK_ALIGN(tables, 8, "cam_overlay_ragged", "tables");           // doubles
    EXCEL_CHECK_ALIGN(out_off, 8, "cam_overlay_ragged", "out_off");         // int64 offsets
    EXCEL_CHECK_ARG(mode == EXCEL_CAM_OVERLAY_MAX || mode == EXCEL_CAM_OVERLAY_PER_CLASS, "cam_overlay_ragged: unknown mode %d", mode);
    EXCEL_CHECK_ARG(mode == EXCEL_CAM_OVERLAY_MAX || out_off, "cam_overlay_ragged: per-class mode needs out_off");
    EXCEL_CHECK_ARG(Cmax >= 1 && info->B >= 1, "cam_overlay_ragged: need Cmax >= 1 and B >= 1");
    EXCEL_CHECK_ARG((long long)Cmax * info->total_pix < (1LL << 31), "cam_overlay_ragged: Cmax * total_pix must stay below 2^31");
    TileGeo geo;
    geo.tab = table; geo.B = info->B; geo.H = geo.W = 0;
    return camviz_launch(hwc, cams, Cmax, ncls, 0, out_off, geo, info->total_tiles, mode, tables, out, stream);
}

extern "C" int excel_cam_overlay(const uint8_t* hwc, const float* cams, int k, int H, int W, int mode, const double* tables, uint8_t* out,
                                 void* stream) {
    EXCEL_CHECK_ARG(hwc && cams && tables && out, "cam_overlay: null argument");
    EXCEL_CHECK_ALIGN(tables, 8, "cam_overlay", "tables");                  // doubles
    EXCEL_CHECK_ARG(mode == EXCEL_CAM_OVERLAY_MAX || mode == EXCEL_CAM_OVERLAY_PER_CLASS, "cam_overlay: unknown mode %d", mode);
    EXCEL_CHECK_ARG(k >= 0 && H >= 1 && W >= 1, "cam_overlay: bad shape (k %d, %d x %d)", k, H, W);
    EXCEL_CHECK_ARG((long long)(k + 1) * H * W < (1LL << 31) && 3LL * (k > 1 ? k : 1) * H * W < (1LL << 31),
                    "cam_overlay: (k + 1) * H * W and 3 * k * H * W must stay below 2^31");
    if (k == 0) return EXCEL_OK;
    TileGeo geo;
    geo.tab = nullptr; geo.B = 1; geo.H = H; geo.W = W;
    return camviz_launch(hwc, cams, k + 1, nullptr, k, nullptr, geo, cdivl(W, 64) * cdivl(H, 16), mode, tables, out, stream);
}
