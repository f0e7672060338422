// LVC ("learned visual cue") side of the path, SURVEY 8(f) rank 1 -- the pieces around the decoder features:
//   * feature affinity: channel-normalised token similarity, shifted by beta x its mean over the WHOLE batch tensor and
//     scaled by gamma; then either sigmoid (attn_pred, model/model_excel.py:70-76) or "negatives -> -inf, row softmax"
//     (ex_attn, clip/clip_surgery_model.py:128-137); the grouped form takes each mean over one group of images instead;
//   * seg_attn layer selection of refine_cams_with_aff (utils/affutils.py:182-195).
// All reductions are fixed-order (no atomics): results are run-to-run identical.
#include "common.h"
#include "excel_internal.h"

// ---------------------------------------------------------------------------------------------- feature affinity
// f [B,C,P]: inv[b,p] = 1 / max(||f[b,:,p]||, 1e-12)        (F.normalize(dim=1))
__global__ __launch_bounds__(256) void lvc_col_invnorm_kernel(const float* __restrict__ f, float* __restrict__ inv, int C, int P) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float* src = f + (long long)b * C * P + p;
    float ss = 0.f;
    for (int c = 0; c < C; ++c) { const float v = src[(long long)c * P]; ss = fmaf(v, v, ss); }
    inv[(long long)b * P + p] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
}

// fn[b,p,c] = f[b,c,p] * inv[b,p]   (row-major [P,Cp] per image, zero-padded to Cp % 4 == 0: the GEMM's K operand)
__global__ __launch_bounds__(256) void lvc_transpose_scale_kernel(const float* __restrict__ f, const float* __restrict__ inv,
                                                                  float* __restrict__ fn, int C, int Cp, int P) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, p = p0 + tx;
        tile[j][tx] = (c < C && p < P) ? f[((long long)b * C + c) * P + p] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int p = p0 + j, c = c0 + tx;
        if (p < P && c < Cp) fn[((long long)b * P + p) * Cp + c] = tile[tx][j] * inv[(long long)b * P + p];
    }
}

// fixed-order two-stage sum in double: partial[i] = sum of chunk i
__global__ __launch_bounds__(256) void lvc_partial_sum_kernel(const float* __restrict__ x, long long n, double* __restrict__ partial) {
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per, hi = min(lo + per, n);
    double s = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) s += (double)x[i];
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void lvc_final_mean_kernel(const double* __restrict__ partial, int n_partial, long long n, float* __restrict__ mean) {
    if (threadIdx.x || blockIdx.x) return;
    double s = 0.0;
    for (int i = 0; i < n_partial; ++i) s += partial[i];
    mean[0] = (float)(s / (double)n);
}

// one wave per row: z = (sim - mean*beta)*gamma ; mode 0: sigmoid(z) ; mode 1: z < 0 -> -inf, softmax over the row
// (shared by the whole-batch and the grouped entry: the same instructions, so a group's rows equal a standalone call's bit for bit)
__device__ __forceinline__ void lvc_finish_row(float* __restrict__ r, float shift, int P, float gamma, int mode, int lane) {
    if (mode == 0) {
        for (int i = lane; i < P; i += 64) {
            const float z = (r[i] - shift) * gamma;
            r[i] = 1.f / (1.f + expf(-z));
        }
        return;
    }
    float m = -INFINITY;
    for (int i = lane; i < P; i += 64) {
        const float z = (r[i] - shift) * gamma;
        if (!(z < 0.f)) m = fmaxf(m, z);
    }
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < P; i += 64) {
        const float z = (r[i] - shift) * gamma;
        if (!(z < 0.f)) s += expf(z - m);
    }
    s = wave_sum(s);
    // a row whose every entry is masked is softmax over all -inf: NaN in every position, like torch.softmax (a row with one entry
    // left has s >= 1, and its masked entries are exp(-inf) / s = 0)
    const float masked = s > 0.f ? 0.f : NAN;
    for (int i = lane; i < P; i += 64) {
        const float z = (r[i] - shift) * gamma;
        r[i] = (z < 0.f) ? masked : expf(z - m) / s;
    }
}

__global__ __launch_bounds__(256) void lvc_finish_kernel(float* __restrict__ sim, const float* __restrict__ mean, long long rows, int P,
                                                         float beta, float gamma, int mode) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    lvc_finish_row(sim + row * P, mean[0] * beta, P, gamma, mode, lane);
}

// inverse norms [B,P], normalised features [B,P,Cp], 1024 double partials per group, one mean per group (the whole-batch form is one group)
struct AffWs { float *inv, *fn, *mean; double* partial; int Cp; size_t total; };
static AffWs aff_ws_layout(int B, int C, int P, int ngroups, void* base) {
    AffWs w;
    w.Cp = (C + 3) / 4 * 4;
    Workspace ws(base);
    w.inv = ws.take<float>((size_t)B * P);
    w.fn = ws.take<float>((size_t)B * P * w.Cp);
    w.partial = ws.take<double>((size_t)ngroups * 1024);
    w.mean = ws.take<float>(ngroups);
    w.total = ws.total();
    return w;
}
// fn [B,P,Cp] = the channel-normalised features; sim[b] = fn[b] . fn[b]^T (exact fp32 MFMA GEMM, NT form, one image per batch entry)
static int lvc_normalized_sim(const float* feats, int B, int C, int P, const AffWs& w, float* out, const char* who, hipStream_t st) {
    hipLaunchKernelGGL(lvc_col_invnorm_kernel, dim3(cdiv(P, 256), B), dim3(256), 0, st, feats, w.inv, C, P);
    hipLaunchKernelGGL(lvc_transpose_scale_kernel, dim3(cdiv(P, 32), cdiv(w.Cp, 32), B), dim3(256), 0, st, feats, w.inv, w.fn, C, w.Cp, P);
    EXCEL_CHECK_LAUNCH(who);
    GemmArgs g = gemm_args(w.fn, w.fn, out, nullptr, nullptr, P, P, w.Cp, w.Cp, w.Cp, P, 0, GEMM_ACT_NONE);
    g.sA = g.sB = (long long)P * w.Cp; g.sC = (long long)P * P;
    return excel_launch_gemm(g, true, B, st);
}

size_t excel_feature_affinity_ws_bytes(int B, int C, int P) { return aff_ws_layout(B, C, P, 1, nullptr).total; }

int excel_launch_feature_affinity(const float* feats, int B, int C, int P, float beta, float gamma, int mode, float* out, void* ws,
                                  hipStream_t st) {
    ProfScope prof__(PROF_OTHER, st);
    EXCEL_CHECK_ARG(feats && out && ws && B > 0 && C > 0 && P > 0 && (mode == 0 || mode == 1), "feature_affinity: bad argument");
    const AffWs w = aff_ws_layout(B, C, P, 1, ws);
    float* mean = w.mean;
    double* partial = w.partial;
    TRY(lvc_normalized_sim(feats, B, C, P, w, out, "feature_affinity/normalize", st));
    const long long n = (long long)B * P * P;
    const int nparts = (int)min((long long)1024, cdivl(n, 4096));
    hipLaunchKernelGGL(lvc_partial_sum_kernel, dim3(nparts), dim3(256), 0, st, out, n, partial);
    hipLaunchKernelGGL(lvc_final_mean_kernel, dim3(1), dim3(64), 0, st, partial, nparts, n, mean);
    hipLaunchKernelGGL(lvc_finish_kernel, dim3((unsigned)cdivl((long long)B * P, 4)), dim3(256), 0, st, out, mean, (long long)B * P, P,
                       beta, gamma, mode);
    EXCEL_CHECK_LAUNCH("feature_affinity");
    return EXCEL_OK;
}

// ---------------------------------------------------------------------------------------------- grouped feature affinity
// Same affinity, but the mean of each GROUP of `group` images is taken over that group alone (include/excel_hip.h).  Member m of
// group j is image first(j) + m * ms with first(j) = (j / ms) * group * ms + j % ms: ms = 1 -> consecutive images, ms = B / group ->
// image j of every slice of B / group images (the (x, flip x) pairs of a [2B] stack).
__device__ __forceinline__ long long lvc_group_first(int j, int group, int ms) {
    return (long long)(j / ms) * group * ms + (j % ms);
}

// partial[j, i] = sum of chunk i of group j's concatenated sims (member order): the chunking and the order of the additions of
// lvc_partial_sum_kernel over a [group,P,P] tensor, reading the members where they lie.  grid (nparts, ngroups)
__global__ __launch_bounds__(256) void lvc_group_partial_sum_kernel(const float* __restrict__ x, long long PP, int group, int ms,
                                                                    double* __restrict__ partial) {
    const int j = blockIdx.y;
    const long long n = PP * group;
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per, hi = min(lo + per, n);
    const float* src = x + lvc_group_first(j, group, ms) * PP;
    const long long mstride = (long long)ms * PP;
    double s = 0.0;
    long long i = lo + threadIdx.x;
    long long m = i / PP, off = i - m * PP;
    for (; i < hi; i += 256) {
        s += (double)src[m * mstride + off];
        off += 256;
        while (off >= PP) { off -= PP; ++m; }
    }
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(long long)j * gridDim.x + blockIdx.x] = red[0];
}

// mean[j] = (sum of group j's partials in order) / n          grid (ngroups)
__global__ void lvc_group_final_mean_kernel(const double* __restrict__ partial, int n_partial, long long n, float* __restrict__ mean) {
    if (threadIdx.x) return;
    const int j = blockIdx.x;
    double s = 0.0;
    for (int i = 0; i < n_partial; ++i) s += partial[(long long)j * n_partial + i];
    mean[j] = (float)(s / (double)n);
}

// row r of image b = r / P uses the mean of b's group
__global__ __launch_bounds__(256) void lvc_group_finish_kernel(float* __restrict__ sim, const float* __restrict__ mean, long long rows, int P,
                                                               int group, int ms, float beta, float gamma, int mode) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int b = (int)(row / P), slab = group * ms, r = b % slab;
    const int j = (b / slab) * ms + r % ms;
    lvc_finish_row(sim + row * P, mean[j] * beta, P, gamma, mode, lane);
}

static int lvc_group_nparts(long long n) { return (int)min((long long)1024, cdivl(n, 4096)); }

size_t excel_feature_affinity_grouped_ws_bytes(int B, int C, int P, int group) {
    return aff_ws_layout(B, C, P, group > 0 ? B / group : 0, nullptr).total;
}

int excel_launch_feature_affinity_grouped(const float* feats, int B, int C, int P, int group, int member_stride, float beta, float gamma,
                                          int mode, float* out, void* ws, hipStream_t st) {
    ProfScope prof__(PROF_OTHER, st);
    EXCEL_CHECK_ARG(feats && out && ws && B > 0 && C > 0 && P > 0 && (mode == 0 || mode == 1), "feature_affinity_grouped: bad argument");
    EXCEL_CHECK_ARG(group >= 1 && member_stride >= 1 && B % ((long long)group * member_stride) == 0,
                    "feature_affinity_grouped: B=%d is not a multiple of group (%d) x member_stride (%d)", B, group, member_stride);
    const int ngroups = B / group;
    const AffWs w = aff_ws_layout(B, C, P, ngroups, ws);
    float* mean = w.mean;
    double* partial = w.partial;
    TRY(lvc_normalized_sim(feats, B, C, P, w, out, "feature_affinity_grouped/normalize", st));
    const long long PP = (long long)P * P, n = PP * group;      // a standalone call on one group: n = group * P * P
    const int nparts = lvc_group_nparts(n);
    hipLaunchKernelGGL(lvc_group_partial_sum_kernel, dim3(nparts, ngroups), dim3(256), 0, st, out, PP, group, member_stride, partial);
    hipLaunchKernelGGL(lvc_group_final_mean_kernel, dim3(ngroups), dim3(64), 0, st, partial, nparts, n, mean);
    hipLaunchKernelGGL(lvc_group_finish_kernel, dim3((unsigned)cdivl((long long)B * P, 4)), dim3(256), 0, st, out, mean, (long long)B * P, P,
                       group, member_stride, beta, gamma, mode);
    EXCEL_CHECK_LAUNCH("feature_affinity_grouped");
    return EXCEL_OK;
}

// ---------------------------------------------------------------------------------------------- seg_attn layer selection
// attn [Lw,B,N,N] (stacked per-layer maps, the last n_layers of which are used), seg [B,P,P], P = N-1.
// diff[b,l] = sum_{m,n} (seg[b,m,n] - attn[l,b,1+m,1+n]) ; one block per (chunk, l, b), fixed order, double
__global__ __launch_bounds__(256) void lvc_layer_diff_kernel(const float* __restrict__ attn, const float* __restrict__ seg, int B, int N,
                                                             int first_layer, double* __restrict__ partial) {
    const int l = blockIdx.y, b = blockIdx.z, P = N - 1;
    const long long n = (long long)P * P;
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per, hi = min(lo + per, n);
    const float* a = attn + (((long long)(first_layer + l) * B + b) * N) * N;
    const float* s = seg + (long long)b * n;
    double acc = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const int m = (int)(i / P), k = (int)(i - (long long)m * P);
        acc += (double)(s[i] - a[(long long)(m + 1) * N + (k + 1)]);
    }
    __shared__ double red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[((long long)b * gridDim.y + l) * gridDim.x + blockIdx.x] = red[0];
}

// per image: layer mask (diff <= mean diff), 1 / (count + 1e-5)
__global__ void lvc_layer_mask_kernel(const double* __restrict__ partial, int nchunk, int L, float* __restrict__ mask /*[B,L+1]*/) {
    const int b = blockIdx.x;
    if (threadIdx.x) return;
    float diff[16];
    float mean = 0.f;
    for (int l = 0; l < L; ++l) {
        double s = 0.0;
        for (int c = 0; c < nchunk; ++c) s += partial[((long long)b * L + l) * nchunk + c];
        diff[l] = (float)s;
        mean += diff[l];
    }
    mean /= (float)L;                                           // :185
    float cnt = 0.f;
    for (int l = 0; l < L; ++l) {
        const float mk = diff[l] <= mean ? 1.f : 0.f;           // :187-188
        mask[b * (L + 1) + l] = mk;
        cnt += mk;
    }
    mask[b * (L + 1) + L] = 1.f / (cnt + 1e-5f);                // :193
}

__global__ __launch_bounds__(256) void lvc_select_mean_kernel(const float* __restrict__ attn, const float* __restrict__ seg,
                                                              const float* __restrict__ mask, int B, int N, int first_layer, int L,
                                                              float* __restrict__ out) {
    const int P = N - 1;
    const long long n = (long long)P * P;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= n) return;
    const int m = (int)(i / P), k = (int)(i - (long long)m * P);
    float acc = 0.f;
    for (int l = 0; l < L; ++l)
        acc += mask[b * (L + 1) + l] * attn[(((long long)(first_layer + l) * B + b) * N + (m + 1)) * N + (k + 1)];
    out[(long long)b * n + i] = acc * mask[b * (L + 1) + L] * seg[(long long)b * n + i];      // :193, :195
}

struct SelectWs { double* partial; float* mask; size_t total; };
static SelectWs select_ws_layout(int B, int n_layers, void* base) {
    SelectWs w;
    Workspace ws(base);
    w.partial = ws.take<double>((size_t)B * n_layers * 64);        // 64 chunks per (image, layer)
    w.mask = ws.take<float>((size_t)B * (n_layers + 1));
    w.total = ws.total();
    return w;
}
size_t excel_attn_select_ws_bytes(int B, int n_layers) { return select_ws_layout(B, n_layers, nullptr).total; }

int excel_launch_attn_select_mean(const float* attn, int Lw, int B, int N, int first_layer, int n_layers, const float* seg_attn,
                                  float* out, void* ws, hipStream_t st) {
    ProfScope prof__(PROF_OTHER, st);
    EXCEL_CHECK_ARG(attn && seg_attn && out && ws && first_layer >= 0 && n_layers >= 1 && n_layers <= 16 && first_layer + n_layers <= Lw,
                    "attn_select_mean: bad layer range");
    const SelectWs w = select_ws_layout(B, n_layers, ws);
    double* partial = w.partial;
    float* mask = w.mask;
    hipLaunchKernelGGL(lvc_layer_diff_kernel, dim3(64, n_layers, B), dim3(256), 0, st, attn, seg_attn, B, N, first_layer, partial);
    hipLaunchKernelGGL(lvc_layer_mask_kernel, dim3(B), dim3(64), 0, st, partial, 64, n_layers, mask);
    const long long n = (long long)(N - 1) * (N - 1);
    hipLaunchKernelGGL(lvc_select_mean_kernel, dim3((unsigned)cdivl(n, 256), B), dim3(256), 0, st, attn, seg_attn, mask, B, N, first_layer,
                       n_layers, out);
    EXCEL_CHECK_LAUNCH("attn_select_mean");
    return EXCEL_OK;
}
