// Zero-shot image tags from CLIP's own image embedding (include/excel_hip.h, "image tags").
//
// Row 0 of the tower's x_raw is the class token of the ORIGINAL attention path after ln_post / proj (the reference puts it back,
// clip/clip_surgery_model.py:442-446): CLIP's image embedding.  One workgroup per image turns it into the [F] one-hot row
// excel_cls_compact reads, without a host round trip:
//
//   cos[t]   = <x, text_t> / (||x|| ||text_t||)         both norms computed here
//   p[t]     = softmax over ALL T rows of scale * cos   background prompts compete
//   rank[f]  = #{g < F : p[g] > p[f] or (p[g] == p[f] and g < f)}
//   tag[f]   = rank[f] < kmax and (rank[f] == 0 or p[f] >= rel_thre * max_f p[f])
//
// The class-token row lives in LDS; the four waves stride over the text rows with 16-byte loads (the bank is a few hundred kB and stays
// in L2 across the images), one wave reduction per row for the dot product and the row's norm.  Every row is summed by the same lanes in
// the same order whichever wave takes it, so two identical text rows get bit-identical logits and the tie rule decides between them.
// The softmax runs in LDS; one thread per foreground class counts its rank over the F <= 254 scores (broadcast LDS reads).  No global
// workspace, no atomics, no scratch.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#define TAG_MAXC 1024
#define TAG_MAXT 512
#define TAG_MAXF 254
#define TAG_NW 4           // waves of a workgroup

__device__ __forceinline__ float tag_block_sum(float v, float* red, int wave, int lane) {
    v = wave_sum(v);
    __syncthreads();                                         // (red may still be read from the reduction before)
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float tag_block_max(float v, float* red, int wave, int lane) {
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void clip_tags_kernel(const float* __restrict__ x_cls, long long stride, const float* __restrict__ text,
                                                        int C, int T, int F, float scale, float rel_thre, int kmax,
                                                        float* __restrict__ onehot, float* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) float xs[TAG_MAXC];
    __shared__ float p[TAG_MAXT];                            // logits, then probabilities
    __shared__ float red[TAG_NW];
    __shared__ int bad;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int C4 = C >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x_cls + (long long)b * stride);
    float4* xs4 = reinterpret_cast<float4*>(xs);
    if (tid == 0) bad = 0;
    float ss = 0.f;
    for (int i = tid; i < C4; i += 256) {
        const float4 v = x4[i];
        xs4[i] = v;
        ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    const float xn = sqrtf(tag_block_sum(ss, red, wave, lane));   // (its barriers also publish xs and bad)
    for (int t = wave; t < T; t += TAG_NW) {
        const float4* r4 = reinterpret_cast<const float4*>(text + (long long)t * C);
        float dot = 0.f, tt = 0.f;
        for (int i = lane; i < C4; i += 64) {
            const float4 w = r4[i], v = xs4[i];
            dot += (w.x * v.x + w.y * v.y) + (w.z * v.z + w.w * v.w);
            tt += (w.x * w.x + w.y * w.y) + (w.z * w.z + w.w * w.w);
        }
        dot = wave_sum(dot);
        tt = wave_sum(tt);
        if (lane == 0) p[t] = scale * (dot / (xn * sqrtf(tt)));
    }
    __syncthreads();
    // softmax over all T rows; a logit that is not finite (integer test on the bits) condemns the image
    const float l0 = tid < T ? p[tid] : -INFINITY, l1 = tid + 256 < T ? p[tid + 256] : -INFINITY;
    if ((tid < T && (__float_as_uint(l0) & 0x7f800000u) == 0x7f800000u) || (tid + 256 < T && (__float_as_uint(l1) & 0x7f800000u) == 0x7f800000u))
        bad = 1;
    const float m = tag_block_max(fmaxf(l0, l1), red, wave, lane);       // (publishes bad)
    if (bad) {
        if (tid < F) {
            onehot[(long long)b * F + tid] = tid == 0 ? 1.f : 0.f;
            if (scores) scores[(long long)b * F + tid] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    const float e0 = tid < T ? expf(l0 - m) : 0.f, e1 = tid + 256 < T ? expf(l1 - m) : 0.f;
    const float sum = tag_block_sum(e0 + e1, red, wave, lane);
    if (tid < T) p[tid] = e0 / sum;
    if (tid + 256 < T) p[tid + 256] = e1 / sum;
    __syncthreads();
    if (tid >= F) return;
    const float s = p[tid];
    float pmax = s;
    int rank = 0;
    for (int g = 0; g < F; ++g) {
        const float q = p[g];
        pmax = fmaxf(pmax, q);
        rank += (q > s || (q == s && g < tid)) ? 1 : 0;
    }
    onehot[(long long)b * F + tid] = (rank < kmax && (rank == 0 || s >= rel_thre * pmax)) ? 1.f : 0.f;
    if (scores) scores[(long long)b * F + tid] = s;
}

extern "C" int excel_clip_tags(const float* x_cls, long long stride, const float* text, int B, int C, int T, int F, float scale,
                               float rel_thre, int kmax, float* onehot_out, float* scores_out, void* stream) {
    EXCEL_CHECK_ARG(x_cls && text && onehot_out, "clip_tags: null argument");
    EXCEL_CHECK_ARG(B >= 1, "clip_tags: need B >= 1 (B = %d)", B);
    EXCEL_CHECK_ARG(F >= 1 && F <= T && T <= TAG_MAXT && F <= TAG_MAXF, "clip_tags: need 1 <= F <= T <= %d and F <= %d (F = %d, T = %d)",
                    TAG_MAXT, TAG_MAXF, F, T);
    EXCEL_CHECK_ARG(C >= 4 && (C & 3) == 0 && C <= TAG_MAXC, "clip_tags: need C %% 4 == 0 and 4 <= C <= %d (C = %d)", TAG_MAXC, C);
    EXCEL_CHECK_ARG(stride >= C && (stride & 3) == 0, "clip_tags: need stride >= C and stride %% 4 == 0 (stride = %lld, C = %d)", stride, C);
    EXCEL_CHECK_ARG(((uintptr_t)x_cls & 15) == 0 && ((uintptr_t)text & 15) == 0, "clip_tags: x_cls and text must be 16-byte aligned");
    EXCEL_CHECK_ARG(((uintptr_t)onehot_out & 3) == 0 && ((uintptr_t)scores_out & 3) == 0, "clip_tags: the outputs must be 4-byte aligned");
    EXCEL_CHECK_ARG(kmax >= 1 && kmax <= F, "clip_tags: need 1 <= kmax <= F (kmax = %d, F = %d)", kmax, F);
    EXCEL_CHECK_ARG(rel_thre >= 0.f && rel_thre <= 1.f, "clip_tags: need 0 <= rel_thre <= 1 (got %g)", (double)rel_thre);
    EXCEL_CHECK_ARG(scale > 0.f && scale <= 3.0e38f, "clip_tags: need a finite scale > 0 (got %g)", (double)scale);
    hipStream_t st = ST(stream);
    ProfScope prof__(PROF_OTHER, st);
    hipLaunchKernelGGL(clip_tags_kernel, dim3((unsigned)B), dim3(256), 0, st, x_cls, stride, text, C, T, F, scale, rel_thre, kmax, onehot_out,
                       scores_out);
    EXCEL_CHECK_LAUNCH("clip_tags");
    return EXCEL_OK;
}
