// Training augmentation of VOC12ClsDataset(aug=True) (datasets/voc.py:110-117 over datasets/transforms.py) for a ragged batch of
// decoded uint8 images and labels on the device: Pillow BILINEAR / NEAREST rescale, horizontal flip, pad + crop with the
// cat_max_ratio rule, normalisation and the CHW store (include/excel_hip.h, "training augmentation").
//
// The host builds Pillow's coefficient and index tables (excel_train_aug_plan: the same double arithmetic as Pillow's
// precompute_coeffs / ImagingScaleAffine, contraction off), so the device work is integer arithmetic and table lookups:
//   aug_hist_kernel     label histogram of every (image, candidate window) through the NEAREST tables   grid (S/8, 10, B)
//   aug_choose_kernel   first candidate with >= 1 class and max/sum < 0.75, else the 10th; img_box       grid (B)
//   aug_hpass_kernel    Pillow's horizontal pass -> uint8 workspace, only the chosen crop's columns and
//                       the source rows its vertical taps read                                            grid (w'/64, h/4, B)
//   aug_vpass_kernel    Pillow's vertical pass + flip + pad + crop + normalise + CHW store + label crop   grid (S*S/256, B)
// The image-only transform of CocoClsDataset(aug=True) (datasets/coco.py:112-142: random_crop with label=None takes the first draw)
// runs the <false> instances: aug_choose_kernel<false> takes candidate 0 without histograms, aug_vpass_kernel<false> has no label
// load or store; there is no histogram memset or launch.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#include <math.h>
#include <vector>

namespace {

constexpr int NCAND = EXCEL_AUG_CANDIDATES;
constexpr int REC = EXCEL_AUG_REC;
constexpr int PREC = 22;                       // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)
constexpr int IGNORE = 255;

enum { R_H = 0, R_W, R_H2, R_W2, R_LOFF, R_WS, R_XOFF, R_KX, R_YOFF, R_KY, R_NX, R_NY, R_FLIP, R_HPAD, R_WPAD, R_HP, R_WP, R_CH = 18,
       R_CW = 28 };

size_t hist_bytes(int B) { return align_up((size_t)B * NCAND * 256 * sizeof(int), 256); }
size_t choice_bytes(int B) { return align_up((size_t)B * 2 * sizeof(int), 256); }

#pragma clang fp contract(off)
// Pillow's precompute_coeffs (libImaging/Resample.c) with the bilinear filter (support 1) for in -> out, then
// normalize_coeffs_8bpc: per output index {xmin, n, k[0..ksize)} appended to `tab`; returns ksize.
int pillow_bilinear_coeffs(int in, int out, std::vector<int32_t>& tab) {
    const double scale = (double)(float)in / out;          // (double)(in1 - in0) / outSize with float box edges
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        double ww = 0.0;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            const double w = t < 1.0 ? 1.0 - t : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (int x = xmax; x < ksize; ++x) k[x] = 0.0;
        tab.push_back(xmin);
        tab.push_back(xmax);
        for (int x = 0; x < ksize; ++x)
            tab.push_back(k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << PREC)) : (int32_t)(0.5 + k[x] * (1 << PREC)));
    }
    return ksize;
}

// Pillow's NEAREST resize (ImagingScaleAffine): source index of output i = (int)xo, xo = a/2 + i*a as a running double sum.
void pillow_nearest_index(int in, int out, std::vector<int32_t>& tab) {
    const double a = (double)(float)in / out;
    double xo = 0.0 + a * 0.5;
    for (int x = 0; x < out; ++x) {
        int xin = xo < 0.0 ? -1 : (int)xo;
        if (xin < 0) xin = 0;                            // (never taken for out >= 1: kept so no index can leave the image)
        if (xin > in - 1) xin = in - 1;
        tab.push_back(xin);
        xo += a;
    }
}
#pragma clang fp contract(on)

struct Crop {       // the chosen window in the rescaled, flipped image's coordinates, intersected with the image
    int ry0, ry1, rx0, rx1;
};

__device__ __forceinline__ Crop crop_of(const int* rec, const int* choice, int S) {
    const int hs = choice[0], ws = choice[1];
    Crop c;
    c.ry0 = max(hs - rec[R_HPAD], 0);
    c.ry1 = min(hs + S - rec[R_HPAD], rec[R_H2]);
    c.rx0 = max(ws - rec[R_WPAD], 0);
    c.rx1 = min(ws + S - rec[R_WPAD], rec[R_W2]);
    return c;
}

// label histogram of candidate window `cand` of image b (padded coordinates; pixels outside the placed image are the 255 pad and
// are not counted).  The reference takes np.unique of the UNPADDED rescaled label sliced with the padded window's bounds
// (transforms.py:150-151); on an axis with padding the window is [0, S) and covers the whole image, on an axis without padding
// both coordinate systems coincide - the two counts are the same.
__global__ __launch_bounds__(256) void aug_hist_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ tab, int S,
                                                       int* __restrict__ hist) {
    __shared__ int h[256];
    const int b = blockIdx.z, cand = blockIdx.y;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int* rec = tab + REC * b;
    const int w = rec[R_W], h2 = rec[R_H2], w2 = rec[R_W2], flip = rec[R_FLIP], hpad = rec[R_HPAD], wpad = rec[R_WPAD];
    const int hs = rec[R_CH + cand], ws = rec[R_CW + cand];
    const int* nx = tab + rec[R_NX];
    const int* ny = tab + rec[R_NY];
    const unsigned char* lab = labels + rec[R_LOFF];
    const int x0 = max(ws - wpad, 0), x1 = min(ws + S - wpad, w2);            // rescaled columns inside the window
    const int y0 = max(hs - hpad, 0) + blockIdx.x * 8, y1 = min(min(hs + S - hpad, h2), y0 + 8);
    for (int ry = y0; ry < y1; ++ry) {
        const unsigned char* row = lab + (long long)ny[ry] * w;
        for (int rx = x0 + threadIdx.x; rx < x1; rx += 256) {
            const int v = row[nx[flip ? w2 - 1 - rx : rx]];
            if (v != IGNORE) atomicAdd(&h[v], 1);
        }
    }
    __syncthreads();
    const int v = h[threadIdx.x];
    if (v) atomicAdd(&hist[((long long)b * NCAND + cand) * 256 + threadIdx.x], v);
}

// get_random_cropbox (transforms.py:141-159): the first candidate with at least one non-ignore class and max/sum < 0.75, else the
// last; then img_box (:165-169).  max/sum < 0.75 is tested as 4 max < 3 sum: with sum < 2^31 the float64 quotient of the reference
// cannot round across 0.75, so the two agree.  kHist == false: no label, the first draw is returned (:145-146) - candidate 0, `hist`
// is not read.
template <bool kHist>
__global__ __launch_bounds__(256) void aug_choose_kernel(const int* __restrict__ tab, const int* __restrict__ hist, int S,
                                                         int* __restrict__ choice, int* __restrict__ img_box) {
    __shared__ long long ssum[4];
    __shared__ int smax[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const int* rec = tab + REC * b;
    int pick = kHist ? NCAND - 1 : 0;
    for (int c = 0; kHist && c < NCAND; ++c) {
        const int v = t == IGNORE ? 0 : hist[((long long)b * NCAND + c) * 256 + t];
        long long s = v;
        int m = v;
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o);
            m = max(m, __shfl_xor(m, o));
        }
        if ((t & 63) == 0) { ssum[t >> 6] = s; smax[t >> 6] = m; }
        __syncthreads();
        const long long sum = ssum[0] + ssum[1] + ssum[2] + ssum[3];
        const long long mx = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
        __syncthreads();
        if (sum > 0 && 4 * mx < 3 * sum) { pick = c; break; }
    }
    if (t == 0) {
        const int hs = rec[R_CH + pick], ws = rec[R_CW + pick];
        choice[2 * b] = hs;
        choice[2 * b + 1] = ws;
        img_box[4 * b + 0] = max(rec[R_HPAD] - hs, 0);
        img_box[4 * b + 1] = min(hs + S, rec[R_HPAD] + rec[R_H2]);
        img_box[4 * b + 2] = max(rec[R_WPAD] - ws, 0);
        img_box[4 * b + 3] = min(ws + S, rec[R_WPAD] + rec[R_W2]);
    }
}

// ImagingResampleHorizontal_8bpc: out[y][x][c] = clip8((2^21 + sum_j src[y][xmin+j][c] * k_j) >> 22), for the rescaled columns of the
// chosen crop (in unflipped coordinates) and the source rows [first tap row of the crop's first row, last tap row of its last row].
__global__ __launch_bounds__(256) void aug_hpass_kernel(const unsigned char* __restrict__ hwc, const int* __restrict__ tab,
                                                        const int* __restrict__ choice, int S, unsigned char* __restrict__ ws) {
    const int b = blockIdx.z;
    const int* rec = tab + REC * b;
    const int kx = rec[R_KX];
    if (!kx) return;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int w = rec[R_W], h = rec[R_H], w2 = rec[R_W2];
    if (x >= w2 || y >= h) return;
    const Crop c = crop_of(rec, choice + 2 * b, S);
    const int cx0 = rec[R_FLIP] ? w2 - c.rx1 : c.rx0, cx1 = rec[R_FLIP] ? w2 - c.rx0 : c.rx1;
    int sy0 = c.ry0, sy1 = c.ry1;
    const int ky = rec[R_KY];
    if (ky) {
        const int* vy = tab + rec[R_YOFF];
        sy0 = vy[(long long)c.ry0 * (2 + ky)];
        sy1 = vy[(long long)(c.ry1 - 1) * (2 + ky)] + vy[(long long)(c.ry1 - 1) * (2 + ky) + 1];
    }
    if (x < cx0 || x >= cx1 || y < sy0 || y >= sy1) return;
    const int* k = tab + rec[R_XOFF] + (long long)x * (2 + kx);
    const int xmin = k[0], n = k[1];
    const unsigned char* src = hwc + 3ll * rec[R_LOFF] + ((long long)y * w + xmin) * 3;
    int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
        const int kj = k[2 + j];
        a0 += src[3 * j] * kj;
        a1 += src[3 * j + 1] * kj;
        a2 += src[3 * j + 2] * kj;
    }
    unsigned char* o = ws + rec[R_WS] + ((long long)y * w2 + x) * 3;
    o[0] = (unsigned char)min(max(a0 >> PREC, 0), 255);
    o[1] = (unsigned char)min(max(a1 >> PREC, 0), 255);
    o[2] = (unsigned char)min(max(a2 >> PREC, 0), 255);
}

// ImagingResampleVertical_8bpc on the horizontal pass' rows (or the source rows when the width is unchanged), then flip / pad / crop /
// normalize_img / HWC->CHW: one thread per output pixel, coalesced fp32 stores of the three planes; the label crop (NEAREST, 255 pad)
// in the same thread (kLabel == false: no label, `labels` / `out_label` are not touched).
template <bool kLabel>
__global__ __launch_bounds__(256) void aug_vpass_kernel(const unsigned char* __restrict__ hwc, const unsigned char* __restrict__ labels,
                                                        const int* __restrict__ tab, const int* __restrict__ choice, int S,
                                                        const unsigned char* __restrict__ ws, double m0, double m1, double m2,
                                                        double s0, double s1, double s2, float* __restrict__ out,
                                                        unsigned char* __restrict__ out_label) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * S) return;
    const int b = blockIdx.y;
    const int* rec = tab + REC * b;
    const int oy = i / S, ox = i % S;
    const int ry = choice[2 * b] + oy - rec[R_HPAD], rx = choice[2 * b + 1] + ox - rec[R_WPAD];
    const int h2 = rec[R_H2], w2 = rec[R_W2];
    int v0 = 0, v1 = 0, v2 = 0, lv = IGNORE;
    if (ry >= 0 && ry < h2 && rx >= 0 && rx < w2) {
        const int x = rec[R_FLIP] ? w2 - 1 - rx : rx;                   // column of the rescaled, unflipped image
        const int kx = rec[R_KX], ky = rec[R_KY];
        // rows of width w2: the horizontal pass' output, or the source itself when the width is unchanged (w2 == w)
        const unsigned char* mid = kx ? ws + rec[R_WS] : hwc + 3ll * rec[R_LOFF];
        if (ky) {
            const int* k = tab + rec[R_YOFF] + (long long)ry * (2 + ky);
            const int ymin = k[0], n = k[1];
            int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
            for (int j = 0; j < n; ++j) {
                const unsigned char* p = mid + ((long long)(ymin + j) * w2 + x) * 3;
                const int kj = k[2 + j];
                a0 += p[0] * kj;
                a1 += p[1] * kj;
                a2 += p[2] * kj;
            }
            v0 = min(max(a0 >> PREC, 0), 255);
            v1 = min(max(a1 >> PREC, 0), 255);
            v2 = min(max(a2 >> PREC, 0), 255);
        } else {
            const unsigned char* p = mid + ((long long)ry * w2 + x) * 3;
            v0 = p[0]; v1 = p[1]; v2 = p[2];
        }
        if constexpr (kLabel) {
            const int* nx = tab + rec[R_NX];
            const int* ny = tab + rec[R_NY];
            lv = labels[rec[R_LOFF] + (long long)ny[ry] * rec[R_W] + nx[x]];
        }
    }
    const long long plane = (long long)S * S;
    float* o = out + (long long)b * 3 * plane + i;
    // excel_normalize_img_u8's arithmetic (attr.hip normalize_u8_kernel): double (v - mean) / std, rounded to float
    o[0] = (float)(((double)v0 - m0) / s0);
    o[plane] = (float)(((double)v1 - m1) / s1);
    o[2 * plane] = (float)(((double)v2 - m2) / s2);
    if constexpr (kLabel) out_label[(long long)b * plane + i] = (unsigned char)lv;
}

}  // namespace

int excel_aug_plan(const int32_t* hw, const excel_aug_params* prm, int B, int S, excel_train_aug_info* info, int32_t* table) {
    EXCEL_CHECK_ARG(hw && prm && info && B >= 1 && S >= 1, "train_aug_plan: bad argument (B %d, S %d)", B, S);
    std::vector<int32_t> recs((size_t)REC * B, 0), coef;
    long long loff = 0, wsb = 0;
    int max_h = 0, max_w2 = 0;
    for (int b = 0; b < B; ++b) {
        const excel_aug_params& p = prm[b];
        const int h = hw[2 * b], w = hw[2 * b + 1];
        EXCEL_CHECK_ARG(h >= 1 && w >= 1, "train_aug_plan: image %d has size %d x %d", b, h, w);
        EXCEL_CHECK_ARG(p.ratio >= 0.125 && p.ratio <= 8.0, "train_aug_plan: image %d: ratio %g outside [1/8, 8]", b, p.ratio);
        const int w2 = (int)(p.ratio * w), h2 = (int)(p.ratio * h);           // [int(scale * w), int(scale * h)] (transforms.py:40)
        EXCEL_CHECK_ARG(h2 >= 1 && w2 >= 1, "train_aug_plan: image %d rescales to %d x %d", b, h2, w2);
        const int Hp = S > h2 ? S : h2, Wp = S > w2 ? S : w2;
        EXCEL_CHECK_ARG(p.flip == 0 || p.flip == 1, "train_aug_plan: image %d: flip must be 0 or 1", b);
        EXCEL_CHECK_ARG(p.h_pad >= 0 && p.h_pad <= Hp - h2 && p.w_pad >= 0 && p.w_pad <= Wp - w2,
                        "train_aug_plan: image %d: placement (%d, %d) outside [0, %d] x [0, %d]", b, p.h_pad, p.w_pad, Hp - h2, Wp - w2);
        for (int c = 0; c < NCAND; ++c)
            EXCEL_CHECK_ARG(p.cand_h[c] >= 0 && p.cand_h[c] <= Hp - S && p.cand_w[c] >= 0 && p.cand_w[c] <= Wp - S,
                            "train_aug_plan: image %d: candidate %d origin (%d, %d) outside [0, %d] x [0, %d]", b, c, p.cand_h[c],
                            p.cand_w[c], Hp - S, Wp - S);
        int32_t* r = recs.data() + (size_t)REC * b;
        r[R_H] = h; r[R_W] = w; r[R_H2] = h2; r[R_W2] = w2; r[R_LOFF] = (int32_t)loff;
        r[R_FLIP] = p.flip; r[R_HPAD] = p.h_pad; r[R_WPAD] = p.w_pad; r[R_HP] = Hp; r[R_WP] = Wp;
        for (int c = 0; c < NCAND; ++c) { r[R_CH + c] = p.cand_h[c]; r[R_CW + c] = p.cand_w[c]; }
        const long long base = (long long)REC * B;
        r[R_XOFF] = r[R_KX] = r[R_YOFF] = r[R_KY] = 0;
        r[R_WS] = 0;
        if (w2 != w) {            // Pillow skips the pass of an axis that keeps its size
            r[R_XOFF] = (int32_t)(base + coef.size());
            r[R_KX] = pillow_bilinear_coeffs(w, w2, coef);
            r[R_WS] = (int32_t)wsb;
            wsb += align_up((size_t)h * w2 * 3, 256);
        }
        if (h2 != h) {
            r[R_YOFF] = (int32_t)(base + coef.size());
            r[R_KY] = pillow_bilinear_coeffs(h, h2, coef);
        }
        r[R_NX] = (int32_t)(base + coef.size());
        pillow_nearest_index(w, w2, coef);
        r[R_NY] = (int32_t)(base + coef.size());
        pillow_nearest_index(h, h2, coef);
        loff += (long long)h * w;
        if (h > max_h) max_h = h;
        if (w2 > max_w2) max_w2 = w2;
        EXCEL_CHECK_ARG(3 * loff < (1LL << 31) && wsb < (1LL << 31) && base + (long long)coef.size() < (1LL << 31),
                        "train_aug_plan: batch too large for 32-bit offsets");
    }
    EXCEL_CHECK_ARG((long long)S * S * 3 < (1LL << 31) && S <= 8192, "train_aug_plan: crop size %d too large", S);
    info->B = B; info->S = S; info->max_h = max_h; info->max_w2 = max_w2;
    info->table_ints = (long long)REC * B + (long long)coef.size();
    info->total_label_pix = loff;
    info->workspace_bytes = (long long)(hist_bytes(B) + choice_bytes(B) + (size_t)wsb);
    if (table) {
        memcpy(table, recs.data(), recs.size() * sizeof(int32_t));
        if (!coef.empty()) memcpy(table + recs.size(), coef.data(), coef.size() * sizeof(int32_t));
    }
    return EXCEL_OK;
}

int excel_launch_train_augment(const unsigned char* hwc, const unsigned char* labels, const int* table, const excel_train_aug_info& info,
                               const double* mean, const double* stdv, float* img, unsigned char* label, int* img_box, void* workspace,
                               hipStream_t st) {
    ProfScope prof__(PROF_OTHER, st);
    const int B = info.B, S = info.S;
    int* hist = (int*)workspace;
    int* choice = (int*)((char*)workspace + hist_bytes(B));
    unsigned char* mid = (unsigned char*)workspace + hist_bytes(B) + choice_bytes(B);
    if (hipMemsetAsync(hist, 0, (size_t)B * NCAND * 256 * sizeof(int), st) != hipSuccess) {
        excel_set_error("train_augment: hipMemsetAsync failed");
        return EXCEL_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(aug_hist_kernel, dim3(cdiv(S, 8), NCAND, B), dim3(256), 0, st, labels, table, S, hist);
    EXCEL_CHECK_LAUNCH("aug_hist");
    hipLaunchKernelGGL(aug_choose_kernel<true>, dim3(B), dim3(256), 0, st, table, hist, S, choice, img_box);
    EXCEL_CHECK_LAUNCH("aug_choose");
    hipLaunchKernelGGL(aug_hpass_kernel, dim3(cdiv(info.max_w2, 64), cdiv(info.max_h, 4), B), dim3(64, 4), 0, st, hwc, table, choice, S, mid);
    EXCEL_CHECK_LAUNCH("aug_hpass");
    hipLaunchKernelGGL(aug_vpass_kernel<true>, dim3(cdiv(S * S, 256), B), dim3(256), 0, st, hwc, labels, table, choice, S, mid, mean[0],
                       mean[1], mean[2], stdv[0], stdv[1], stdv[2], img, label);
    EXCEL_CHECK_LAUNCH("aug_vpass");
    return EXCEL_OK;
}

// The image-only transform: the same table and workspace layout (the histogram region is left unused), three launches.
int excel_launch_train_augment_image(const unsigned char* hwc, const int* table, const excel_train_aug_info& info, const double* mean,
                                     const double* stdv, float* img, int* img_box, void* workspace, hipStream_t st) {
    ProfScope prof__(PROF_OTHER, st);
    const int B = info.B, S = info.S;
    int* choice = (int*)((char*)workspace + hist_bytes(B));
    unsigned char* mid = (unsigned char*)workspace + hist_bytes(B) + choice_bytes(B);
    hipLaunchKernelGGL(aug_choose_kernel<false>, dim3(B), dim3(64), 0, st, table, nullptr, S, choice, img_box);
    EXCEL_CHECK_LAUNCH("aug_choose_first");
    hipLaunchKernelGGL(aug_hpass_kernel, dim3(cdiv(info.max_w2, 64), cdiv(info.max_h, 4), B), dim3(64, 4), 0, st, hwc, table, choice, S, mid);
    EXCEL_CHECK_LAUNCH("aug_hpass");
    hipLaunchKernelGGL(aug_vpass_kernel<false>, dim3(cdiv(S * S, 256), B), dim3(256), 0, st, hwc, nullptr, table, choice, S, mid, mean[0],
                       mean[1], mean[2], stdv[0], stdv[1], stdv[2], img, nullptr);
    EXCEL_CHECK_LAUNCH("aug_vpass_image");
    return EXCEL_OK;
}
