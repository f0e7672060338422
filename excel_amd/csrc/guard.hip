// Overflow guard of the f16 GEMM modes (include/excel_hip.h, "overflow guard").
//
// split_hi (common.h) is a plain conversion to IEEE half: a value beyond 65 504 becomes +-inf and every product it enters a NaN.  The
// two kernels here make that NaN visible per image without a host round trip:
//
//   nonfinite_count_kernel   : count[b] (+)= number of fp32 values of image b whose exponent field is all ones (+-inf, any NaN)
//   confusion_masked_kernel  : confusion_kernel (par.hip) over the images whose skip[b] == 0
//
// Both are laid out over (image, chunk of that image): the image index is blockIdx.y, so every per-image quantity (the start, the
// misalignment, the skip flag) is wave-uniform and a skipped image's workgroups leave before they touch LDS.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

__device__ __forceinline__ int nonfinite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u; }

// Pure streaming read: x is only 4-byte aligned and per_image is arbitrary, so an image starts anywhere in a 16-byte line.  Chunk 0's
// first lanes take the (up to 3) floats in front of the first 16-byte boundary and the (up to 3) behind the last whole uint4; everything
// between goes through 16-byte loads, four in flight per lane.  A wave whose lanes found nothing issues no atomic and no reduction.
#define NFC_UNROLL 4
__global__ __launch_bounds__(256) void nonfinite_count_kernel(const unsigned* __restrict__ x, long long per_image, int* __restrict__ count) {
    const int b = blockIdx.y;
    const unsigned* p = x + (long long)b * per_image;
    long long head = (long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    if (head > per_image) head = per_image;
    const long long nvec = (per_image - head) >> 2;
    const long long tail0 = head + 4 * nvec;                 // first element behind the vector body
    int c = 0;
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) c += nonfinite_bits(p[threadIdx.x]);
        if (tail0 + threadIdx.x < per_image) c += nonfinite_bits(p[tail0 + threadIdx.x]);
    }
    const uint4* v = reinterpret_cast<const uint4*>(p + head);
    const long long stride = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    for (; i + (NFC_UNROLL - 1) * stride < nvec; i += NFC_UNROLL * stride) {
        uint4 q[NFC_UNROLL];
#pragma unroll
        for (int k = 0; k < NFC_UNROLL; ++k) q[k] = v[i + k * stride];
#pragma unroll
        for (int k = 0; k < NFC_UNROLL; ++k)
            c += nonfinite_bits(q[k].x) + nonfinite_bits(q[k].y) + nonfinite_bits(q[k].z) + nonfinite_bits(q[k].w);
    }
    for (; i < nvec; i += stride) {
        const uint4 q = v[i];
        c += nonfinite_bits(q.x) + nonfinite_bits(q.y) + nonfinite_bits(q.z) + nonfinite_bits(q.w);
    }
    if (__ballot(c != 0) == 0ull) return;                    // the clean case: nothing more happens
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&count[b], c);
}

// confusion_kernel (par.hip) restricted to one image per blockIdx.y: the same LDS-private histogram, the same scalar head / 16-byte
// body / scalar tail, with the head computed per image (gt and pred of an image share their offset, so their misalignments differ by
// what the two base pointers differ).  tab == nullptr: uniform images of per_image pixels; else image b = [loff_b, loff_{b+1}).
// BAND (nc * nc > GUARD_CONF_MAXBINS): blockIdx.z selects a band of GUARD_CONF_MAXBINS / nc ground-truth rows, as in confusion_kernel<true>.
#define GUARD_CONF_MAXBINS 8192
#define GUARD_CONF_MAXNC 256
// (a macro: as a function the narrow kernel's byte-select operands come out as separate instructions)
#define GUARD_CONF_COUNT(g, p)                                                              \
    do {                                                                              \
        if (BAND) {                                                                   \
            const unsigned int gr_ = (unsigned int)((g) - r0);                        \
            if (gr_ < (unsigned int)rows && (p) < nc) atomicAdd(&lh[gr_ * nc + (p)], 1u); \
        } else {                                                                      \
            if ((g) < nc && (p) < nc) atomicAdd(&lh[(g) * nc + (p)], 1u);             \
        }                                                                             \
    } while (0)
template <bool BAND>
__global__ __launch_bounds__(256) void confusion_masked_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                               const int* __restrict__ tab, long long per_image,
                                                               const int* __restrict__ skip, int nc, unsigned long long* __restrict__ hist) {
    __shared__ unsigned int lh[GUARD_CONF_MAXBINS];
    const int b = blockIdx.y;
    if (skip[b] != 0) return;
    long long start, n;
    if (tab) {
        start = tab[EXCEL_RAG_REC * b + 4];
        n = (long long)tab[EXCEL_RAG_REC * (b + 1) + 4] - start;
    } else {
        start = (long long)b * per_image;
        n = per_image;
    }
    if (blockIdx.x > 0 && (long long)blockIdx.x * 256 * 16 >= n) return;     // more chunks than this image has
    gt += start; pred += start;
    const int band_rows = BAND ? GUARD_CONF_MAXBINS / nc : nc;
    const int r0 = BAND ? (int)blockIdx.z * band_rows : 0, rows = BAND ? min(band_rows, nc - r0) : nc;
    const int bins = rows * nc;
    for (int i = threadIdx.x; i < bins; i += 256) lh[i] = 0;
    __syncthreads();
    const int mg = (int)((16 - ((uintptr_t)gt & 15)) & 15), mp = (int)((16 - ((uintptr_t)pred & 15)) & 15);
    const int head = (mg == mp) ? mg : -1;
    if (head > 0 && blockIdx.x == 0 && threadIdx.x < head && threadIdx.x < n) {
        const int g = gt[threadIdx.x], p = pred[threadIdx.x];
        GUARD_CONF_COUNT(g, p);
    }
    if (head >= 0) {
        gt += head; pred += head; n -= head;
        if (n < 0) n = 0;
    }
    const long long stride = (long long)gridDim.x * 256 * 16;
    for (long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * 16; base < n; base += stride) {
        if (head >= 0 && base + 16 <= n) {
            const uint4 g4 = *reinterpret_cast<const uint4*>(gt + base);
            const uint4 p4 = *reinterpret_cast<const uint4*>(pred + base);
            const unsigned int gw[4] = {g4.x, g4.y, g4.z, g4.w}, pw[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int g = (gw[k >> 2] >> (8 * (k & 3))) & 255, p = (pw[k >> 2] >> (8 * (k & 3))) & 255;
                GUARD_CONF_COUNT(g, p);
            }
        } else {
            const long long end = (base + 16 < n) ? base + 16 : n;
            for (long long j = base; j < end; ++j) {
                const int g = gt[j], p = pred[j];
                GUARD_CONF_COUNT(g, p);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256)
        if (lh[i]) atomicAdd(&hist[(BAND ? r0 * nc : 0) + i], (unsigned long long)lh[i]);
}

extern "C" int excel_nonfinite_count(const float* x, int B, long long per_image, int32_t* count, int init, void* stream) {
    EXCEL_CHECK_ARG(x && count, "nonfinite_count: null argument");
    EXCEL_CHECK_ARG(B >= 1 && B <= 65535, "nonfinite_count: need 1 <= B <= 65535 (B = %d)", B);
    EXCEL_CHECK_ARG(per_image >= 1 && per_image < (1LL << 31), "nonfinite_count: per_image must be in [1, 2^31) (got %lld)", per_image);
    EXCEL_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)count & 3) == 0, "nonfinite_count: x and count must be 4-byte aligned");
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    if (init) {
        const hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)B, st);
        if (e != hipSuccess) {
            excel_set_error("nonfinite_count: clearing the counters failed: %s", hipGetErrorString(e));
            return EXCEL_ERR_LAUNCH;
        }
    }
    // one chunk = 256 lanes x NFC_UNROLL uint4 x 4 rounds; at most ~4096 workgroups per launch
    const long long want = cdivl(per_image, 256LL * 4 * NFC_UNROLL * 4);
    const long long cap = 4096 / B > 1 ? 4096 / B : 1;
    const unsigned chunks = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(nonfinite_count_kernel, dim3(chunks, B), dim3(256), 0, st, reinterpret_cast<const unsigned*>(x), per_image, count);
    EXCEL_CHECK_LAUNCH("nonfinite_count");
    return EXCEL_OK;
}

extern "C" int excel_confusion_accumulate_masked(const uint8_t* gt, const uint8_t* pred, int B, long long per_image, const int32_t* table,
                                                 const excel_ragged_info* info, const int32_t* skip, int num_classes, int64_t* hist,
                                                 void* stream) {
    EXCEL_CHECK_ARG(gt && pred && skip && hist, "confusion_accumulate_masked: null argument");
    EXCEL_CHECK_ARG(B >= 1 && B <= 65535, "confusion_accumulate_masked: need 1 <= B <= 65535 (B = %d)", B);
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= GUARD_CONF_MAXNC, "confusion_accumulate_masked: need 1 <= num_classes <= %d (got %d)",
                    GUARD_CONF_MAXNC, num_classes);
    long long max_pix;
    if (table) {
        EXCEL_CHECK_ARG(info && info->B == B, "confusion_accumulate_masked: the plan holds %d images, B = %d", info ? info->B : -1, B);
        max_pix = info->max_plane_pix;                       // H_b * Wp_b >= H_b * W_b: an upper bound is enough for the grid
    } else {
        EXCEL_CHECK_ARG(per_image >= 1 && per_image < (1LL << 31), "confusion_accumulate_masked: per_image must be in [1, 2^31) (got %lld)",
                        per_image);
        max_pix = per_image;
    }
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    const long long want = cdivl(max_pix, 256 * 16);
    const long long cap = 2048 / B > 1 ? 2048 / B : 1;        // confusion_kernel's bound on the workgroups that flush a histogram
    const unsigned chunks = (unsigned)(want < cap ? (want > 0 ? want : 1) : cap);
    if (num_classes * num_classes <= GUARD_CONF_MAXBINS)
        hipLaunchKernelGGL(confusion_masked_kernel<false>, dim3(chunks, B), dim3(256), 0, st, gt, pred, table, per_image, skip, num_classes,
                           (unsigned long long*)hist);
    else
        hipLaunchKernelGGL(confusion_masked_kernel<true>, dim3(chunks, B, (unsigned)cdivl(num_classes, GUARD_CONF_MAXBINS / num_classes)), dim3(256),
                           0, st, gt, pred, table, per_image, skip, num_classes, (unsigned long long*)hist);
    EXCEL_CHECK_LAUNCH("confusion_accumulate_masked");
    return EXCEL_OK;
}
