// Per-image scores (include/excel_hip.h, "per-image scores").
//
// The confusion kernels (par.hip, guard.hip) add every image of a step into one [nc,nc] matrix; what an image contributed is gone after
// the launch.  The kernel here keeps it, in the form every per-image score is computed from - the three margins of the image's own matrix:
//
//   image_scores_kernel : counts[b,0,g] = pixels of image b with ground truth g          (row sums)
//                         counts[b,1,p] = pixels predicted p                              (column sums)
//                         counts[b,2,g] = pixels with g == p                              (diagonal)
//                         over the pixels with g < nc and p < nc - confusion_kernel's rule - and zero for an image with skip[b] != 0
//
// It is confusion_masked_kernel (guard.hip) with another set of bins: image = blockIdx.y, so the start, the misalignment and the skip flag
// are wave-uniform; the same scalar head / 16-byte body / scalar tail; 3 * nc u32 counters in LDS (3 KB at most, whatever nc: no bands);
// one flush of the non-zero bins per workgroup.  A pixel costs up to three LDS atomics where the matrix costs one, yet the kernel takes
// what confusion_masked_kernel takes on noise-like labels and a third of it on coherent maps; folding a lane's runs of equal (g, p) into
// one count before touching LDS gained nothing on coherent maps and 1 - 2 us of a 21 ms step on noise (EXPERIMENTS.md, "Per-image
// scores"), so every pixel counts itself.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define IMGSCORE_MAXNC 256

__device__ __forceinline__ void imgscore_count(unsigned int* lh, int nc, int g, int p) {
    if (g < nc && p < nc) {
        atomicAdd(&lh[g], 1u);
        atomicAdd(&lh[nc + p], 1u);
        if (g == p) atomicAdd(&lh[2 * nc + g], 1u);
    }
}

__global__ __launch_bounds__(256) void image_scores_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                           const int* __restrict__ tab, long long per_image, const int* __restrict__ skip,
                                                           int nc, int* __restrict__ counts) {
    __shared__ unsigned int lh[3 * IMGSCORE_MAXNC];
    const int b = blockIdx.y;
    if (skip && skip[b] != 0) return;                        // the rows stay as the host entry cleared them
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
    const int bins = 3 * nc;
    for (int i = threadIdx.x; i < bins; i += 256) lh[i] = 0;
    __syncthreads();
    const int mg = (int)((16 - ((uintptr_t)gt & 15)) & 15), mp = (int)((16 - ((uintptr_t)pred & 15)) & 15);
    const int head = (mg == mp) ? mg : -1;
    if (head > 0 && blockIdx.x == 0 && threadIdx.x < head && threadIdx.x < n)
        imgscore_count(lh, nc, gt[threadIdx.x], pred[threadIdx.x]);
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
            for (int k = 0; k < 16; ++k)
                imgscore_count(lh, nc, (gw[k >> 2] >> (8 * (k & 3))) & 255, (pw[k >> 2] >> (8 * (k & 3))) & 255);
        } else {
            const long long end = (base + 16 < n) ? base + 16 : n;
            for (long long j = base; j < end; ++j) imgscore_count(lh, nc, gt[j], pred[j]);
        }
    }
    __syncthreads();
    int* out = counts + (long long)b * bins;
    for (int i = threadIdx.x; i < bins; i += 256)
        if (lh[i]) atomicAdd(&out[i], (int)lh[i]);
}

extern "C" int excel_image_scores(const uint8_t* gt, const uint8_t* pred, int B, long long per_image, const int32_t* table,
                                  const excel_ragged_info* info, const int32_t* skip, int num_classes, int32_t* counts, void* stream) {
    EXCEL_CHECK_ARG(gt && pred && counts, "image_scores: null argument (gt, pred and counts are required)");
    EXCEL_CHECK_ARG(B >= 1 && B <= 65535, "image_scores: need 1 <= B <= 65535 (B = %d)", B);
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= IMGSCORE_MAXNC, "image_scores: need 1 <= num_classes <= %d (got %d)", IMGSCORE_MAXNC,
                    num_classes);
    EXCEL_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)skip & 3) == 0, "image_scores: counts and skip must be 4-byte aligned");
    long long max_pix;
    if (table) {
        EXCEL_CHECK_ARG(info && info->B == B, "image_scores: the plan holds %d images, B = %d", info ? info->B : -1, B);
        max_pix = info->max_plane_pix;                       // H_b * Wp_b >= H_b * W_b: an upper bound is enough for the grid
    } else {
        EXCEL_CHECK_ARG(per_image >= 1 && per_image < (1LL << 31), "image_scores: per_image must be in [1, 2^31) (got %lld)", per_image);
        max_pix = per_image;
    }
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)B * 3 * (size_t)num_classes, st);
    if (e != hipSuccess) {
        excel_set_error("image_scores: clearing the counts failed: %s", hipGetErrorString(e));
        return EXCEL_ERR_LAUNCH;
    }
    const long long want = cdivl(max_pix, 256 * 16);
    const long long cap = 2048 / B > 1 ? 2048 / B : 1;        // confusion_masked_kernel's bound on the workgroups that flush
    const unsigned chunks = (unsigned)(want < cap ? (want > 0 ? want : 1) : cap);
    hipLaunchKernelGGL(image_scores_kernel, dim3(chunks, B), dim3(256), 0, st, gt, pred, table, per_image, skip, num_classes, counts);
    EXCEL_CHECK_LAUNCH("image_scores");
    return EXCEL_OK;
}
