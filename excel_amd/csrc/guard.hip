// Overflow guard of the f16 GEMM modes (include/excel_hip.h, "overflow guard").
//
// split_hi (common.h) is a plain conversion to IEEE half: a value beyond 65 504 becomes +-inf and every product it enters a NaN.  The
// kernel here makes that NaN visible per image without a host round trip:
//
//   nonfinite_count_kernel   : count[b] (+)= number of fp32 values of image b whose exponent field is all ones (+-inf, any NaN)
//
// Its counters are the skip flags of confusion_masked_kernel and image_scores_kernel (confusion.hip).  The grid is (chunk of an image,
// image): the image index is blockIdx.y, so the image's start and misalignment are wave-uniform.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"
#include "label_maps.h"

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

extern "C" int excel_nonfinite_count(const float* x, int B, long long per_image, int32_t* count, int init, void* stream) {
    EXCEL_CHECK_ARG(x && count, "nonfinite_count: null argument");
    EXCEL_CHECK_ARG(B >= 1 && B <= 65535, "nonfinite_count: need 1 <= B <= 65535 (B = %d)", B);
    EXCEL_CHECK_ARG(per_image >= 1 && per_image < (1LL << 31), "nonfinite_count: per_image must be in [1, 2^31) (got %lld)", per_image);
    EXCEL_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)count & 3) == 0, "nonfinite_count: x and count must be 4-byte aligned");
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    if (init) TRY(clear_on_stream("nonfinite_count", "counters", count, sizeof(int32_t) * (size_t)B, st));
    // one chunk = 256 lanes x NFC_UNROLL uint4 x 4 rounds; at most ~4096 workgroups per launch
    const long long want = cdivl(per_image, 256LL * 4 * NFC_UNROLL * 4);
    const long long cap = 4096 / B > 1 ? 4096 / B : 1;
    const unsigned chunks = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(nonfinite_count_kernel, dim3(chunks, B), dim3(256), 0, st, reinterpret_cast<const unsigned*>(x), per_image, count);
    EXCEL_CHECK_LAUNCH("nonfinite_count");
    return EXCEL_OK;
}
