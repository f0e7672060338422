// Counting label pairs: the confusion matrix (include/excel_hip.h, excel_confusion_accumulate; "overflow guard",
// excel_confusion_accumulate_masked) and the per-image scores ("per-image scores").  utils/evaluate.py:9-20 of the reference.
//
// Every score the library reports comes from one streaming pass over a ground-truth map and a predicted map (label_pair_sweep,
// label_maps.h) into LDS-private bins that a workgroup flushes once.  The grid is (chunk, image, band): the image index is blockIdx.y,
// so every per-image quantity (the start, the misalignment, the skip flag) is wave-uniform and a skipped image's workgroups leave
// before they touch LDS.
//
//   confusion_masked_kernel<BAND> : hist[nc * g + p] += 1 over the pixels with g < nc and p < nc of the images whose skip[b] == 0 (a
//                                   null skip: every image).  The matrix of one step adds every image into one [nc,nc] table;
//                                   nc * nc > LABEL_MAXBINS runs in bands of ground-truth rows (matrix_band, blockIdx.z)
//   image_scores_kernel           : what an image contributed, in the form every per-image score is computed from - the three margins
//                                   of the image's own matrix (margin_count):
//                                     counts[b,0,g] = pixels of image b with ground truth g          (row sums)
//                                     counts[b,1,p] = pixels predicted p                              (column sums)
//                                     counts[b,2,g] = pixels with g == p                              (diagonal)
//                                   over the same pixels, and zero for an image with skip[b] != 0
//
// A pixel costs up to three LDS atomics in the margins where the matrix costs one, yet image_scores_kernel takes what the matrix takes
// on noise-like labels and a third of it on coherent maps; folding a lane's runs of equal (g, p) into one count before touching LDS
// gained nothing on coherent maps and 1 - 2 us of a 21 ms step on noise (EXPERIMENTS.md, "Per-image scores"), so every pixel counts
// itself.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"
#include "label_maps.h"

template <bool BAND>
__global__ __launch_bounds__(256) void confusion_masked_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                               const int* __restrict__ tab, long long per_image,
                                                               const int* __restrict__ skip, int nc, unsigned long long* __restrict__ hist) {
    __shared__ unsigned int lh[LABEL_MAXBINS];
    long long n;
    if (!label_image_range(tab, per_image, skip, gt, pred, n)) return;
    const RowBand band = matrix_band<BAND>(nc, blockIdx.z);
    label_bins_clear(lh, band.rows * nc);
    __syncthreads();
    label_pair_sweep(gt, pred, n, [&](int g, int p) { matrix_count<BAND>(lh, nc, band, g, p); });
    __syncthreads();
    matrix_flush<BAND>(lh, nc, band, hist);
}

__global__ __launch_bounds__(256) void image_scores_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                           const int* __restrict__ tab, long long per_image, const int* __restrict__ skip,
                                                           int nc, int* __restrict__ counts) {
    __shared__ unsigned int lh[3 * LABEL_MAXNC];
    long long n;
    if (!label_image_range(tab, per_image, skip, gt, pred, n)) return;      // a skipped image's rows stay as the host entry cleared them
    label_bins_clear(lh, 3 * nc);
    __syncthreads();
    label_pair_sweep(gt, pred, n, [&](int g, int p) { margin_count(lh, nc, g, p); });
    __syncthreads();
    margin_flush(lh, nc, counts + (long long)blockIdx.y * 3 * nc);
}

// per_image is a long long in the kernel: the one range of excel_confusion_accumulate may hold 2^31 pixels and more
static void launch_confusion(const uint8_t* gt, const uint8_t* pred, int B, long long per_image, const int32_t* table, long long max_pix,
                             const int32_t* skip, int nc, int64_t* hist, hipStream_t st) {
    const unsigned chunks = label_pair_chunks(max_pix, B);
    if (nc * nc <= LABEL_MAXBINS)
        hipLaunchKernelGGL(confusion_masked_kernel<false>, dim3(chunks, B), dim3(256), 0, st, gt, pred, table, per_image, skip, nc,
                           (unsigned long long*)hist);
    else
        hipLaunchKernelGGL(confusion_masked_kernel<true>, dim3(chunks, B, (unsigned)cdiv(nc, LABEL_MAXBINS / nc)), dim3(256), 0, st, gt, pred,
                           table, per_image, skip, nc, (unsigned long long*)hist);
}

extern "C" int excel_confusion_accumulate(const uint8_t* gt, const uint8_t* pred, long long n, int num_classes, int64_t* hist,
                                          void* stream) {
    EXCEL_CHECK_ARG(gt && pred && hist && n >= 0, "confusion_accumulate: null argument");
    EXCEL_CHECK_ALIGN(hist, 8, "confusion_accumulate", "hist");             // 64-bit atomic adds
    if (n == 0) return EXCEL_OK;
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= LABEL_MAXNC, "confusion: need 1 <= num_classes <= %d (got %d)", LABEL_MAXNC, num_classes);
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_CONFUSION, st);
    launch_confusion(gt, pred, 1, n, nullptr, n, nullptr, num_classes, hist, st);
    EXCEL_CHECK_LAUNCH("confusion");
    return EXCEL_OK;
}

extern "C" int excel_confusion_accumulate_masked(const uint8_t* gt, const uint8_t* pred, int B, long long per_image, const int32_t* table,
                                                 const excel_ragged_info* info, const int32_t* skip, int num_classes, int64_t* hist,
                                                 void* stream) {
    EXCEL_CHECK_ARG(gt && pred && skip && hist, "confusion_accumulate_masked: null argument");
    EXCEL_CHECK_ALIGN(hist, 8, "confusion_accumulate_masked", "hist");      // 64-bit atomic adds
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= LABEL_MAXNC, "confusion_accumulate_masked: need 1 <= num_classes <= %d (got %d)",
                    LABEL_MAXNC, num_classes);
    long long max_pix;
    TRY(label_images("confusion_accumulate_masked", B, per_image, table, info, &max_pix));
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    launch_confusion(gt, pred, B, per_image, table, max_pix, skip, num_classes, hist, st);
    EXCEL_CHECK_LAUNCH("confusion_accumulate_masked");
    return EXCEL_OK;
}

extern "C" int excel_image_scores(const uint8_t* gt, const uint8_t* pred, int B, long long per_image, const int32_t* table,
                                  const excel_ragged_info* info, const int32_t* skip, int num_classes, int32_t* counts, void* stream) {
    EXCEL_CHECK_ARG(gt && pred && counts, "image_scores: null argument (gt, pred and counts are required)");
    EXCEL_CHECK_ARG(num_classes >= 1 && num_classes <= LABEL_MAXNC, "image_scores: need 1 <= num_classes <= %d (got %d)", LABEL_MAXNC,
                    num_classes);
    EXCEL_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)skip & 3) == 0, "image_scores: counts and skip must be 4-byte aligned");
    long long max_pix;
    TRY(label_images("image_scores", B, per_image, table, info, &max_pix));
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    TRY(clear_on_stream("image_scores", "counts", counts, sizeof(int32_t) * (size_t)B * 3 * (size_t)num_classes, st));
    hipLaunchKernelGGL(image_scores_kernel, dim3(label_pair_chunks(max_pix, B), B), dim3(256), 0, st, gt, pred, table, per_image, skip,
                       num_classes, counts);
    EXCEL_CHECK_LAUNCH("image_scores");
    return EXCEL_OK;
}
