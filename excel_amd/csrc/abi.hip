// extern "C" entry points of libexcel_hip (declared in include/excel_hip.h): error text, build id, profiling hooks and the wrappers
// around the launchers.  The ViT (excel_vit_*) is in vit.hip; launchers that depend on the split type are reached through split_api().
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#include <stdarg.h>
#include <vector>

static thread_local char g_err[512] = "";

void excel_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* excel_last_error(void) { return g_err; }
extern "C" int excel_abi_version(void) { return 6; }
#ifndef EXCEL_BUILD_ID
#define EXCEL_BUILD_ID "unstamped"
#endif
extern "C" const char* excel_build_id(void) { return EXCEL_BUILD_ID; }

// ------------------------------------------------------------------------------------ profiling hooks
bool g_excel_prof_on = false;
thread_local int g_excel_prof_gemm_cat = -1;    // per host thread: concurrent forwards on different threads do not race on it
unsigned long long g_excel_prof_mask = ~0ull;
int g_excel_prof_every = 1;
unsigned g_excel_prof_seen[PROF_NCAT];
namespace {
struct ProfRec { int cat; hipEvent_t a, b; };
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
double g_prof_work[PROF_NCAT];
const char* PROF_NAMES[PROF_NCAT] = {"gemm_nt", "gemm_nn", "gemm_bf16x3", "attn_rowpass", "attn_accum", "layernorm", "embed", "token_norm",
                                     "cam_epilogue", "sinkhorn", "bbox_mask", "matvec", "cam_upsample", "par_affinity",
                                     "par_iterate", "argmax", "confusion", "other", "cam_proj", "cam_fused"};
hipEvent_t prof_event() {
    if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
}  // namespace
void excel_prof_begin(int cat, hipStream_t st, double work) {
    ProfRec r{cat, prof_event(), prof_event()};
    (void)hipEventRecord(r.a, st);
    g_prof_recs.push_back(r);
    g_prof_work[cat] += work;
}
void excel_prof_end(int cat, hipStream_t st) {
    for (size_t i = g_prof_recs.size(); i-- > 0;)
        if (g_prof_recs[i].cat == cat) { (void)hipEventRecord(g_prof_recs[i].b, st); return; }
}
extern "C" int excel_prof_enable(int on) {
    g_excel_prof_on = on != 0;
    return EXCEL_OK;
}
extern "C" int excel_prof_set_mask(unsigned long long mask) {
    g_excel_prof_mask = mask;
    return EXCEL_OK;
}
extern "C" int excel_prof_set_sampling(int every) {
    g_excel_prof_every = every > 0 ? every : 1;
    for (int c = 0; c < PROF_NCAT; ++c) g_excel_prof_seen[c] = 0;
    return EXCEL_OK;
}
extern "C" int excel_prof_num_categories(void) { return PROF_NCAT; }
extern "C" const char* excel_prof_category_name(int cat) { return (cat >= 0 && cat < PROF_NCAT) ? PROF_NAMES[cat] : ""; }
// Synchronises on the recorded events, sums elapsed ms / launches / algorithmic work per category, resets the log.
extern "C" int excel_prof_collect(double* ms, long long* launches, double* work) {
    for (int c = 0; c < PROF_NCAT; ++c) { ms[c] = 0.0; launches[c] = 0; work[c] = g_prof_work[c]; g_prof_work[c] = 0.0; }
    for (auto& r : g_prof_recs) {
        float t = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            ms[r.cat] += t;
            launches[r.cat] += 1;
        }
        g_prof_pool.push_back(r.a);
        g_prof_pool.push_back(r.b);
    }
    g_prof_recs.clear();
    return EXCEL_OK;
}

// ------------------------------------------------------------------------------------ small helper kernels
__global__ void attn_layer_mean_kernel(const float* __restrict__ attn, int B, int N, int first, int nl, float* __restrict__ out) {
    const long long P = N - 1;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * P * P) return;
    const int c = (int)(i % P), r = (int)((i / P) % P);
    const long long b = i / (P * P);
    float s = 0.f;
    for (int l = 0; l < nl; ++l) s += attn[(((long long)(first + l) * B + b) * N + (r + 1)) * N + (c + 1)];
    out[i] = s / (float)nl;
}

// ------------------------------------------------------------------------------------ building blocks
extern "C" int excel_gemm_f32(const float* A, const float* Bm, float* C, const float* bias, const float* residual, int M, int N,
                              int K, int lda, int ldb, int ldc, int ldr, int b_kmajor, int act, int batch, long long sA,
                              long long sB, long long sC, long long sR, void* stream) {
    GemmArgs g = gemm_args(A, Bm, C, bias, residual, M, N, K, lda, ldb, ldc, ldr, act);
    EXCEL_CHECK_ALIGN(A, 16, "excel_gemm_f32", "A");              // gemm_f32_kernel loads both operands as f32x4 (gemm.hip load_tile)
    EXCEL_CHECK_ALIGN(Bm, 16, "excel_gemm_f32", "Bm");
    EXCEL_CHECK_ARG((K % 4) == 0 || !b_kmajor, "excel_gemm_f32: K must be a multiple of 4 in NT mode (K=%d)", K);
    if (!b_kmajor) {
        EXCEL_CHECK_ARG((K % 4) == 0, "excel_gemm_f32: K must be a multiple of 4 (pad A with zeros) (K=%d)", K);
    }
    g.sA = sA; g.sB = sB; g.sC = sC; g.sR = sR;
    return excel_launch_gemm(g, b_kmajor != 0, batch, ST(stream));
}

// the split-plane building blocks: `mode` (the ViT's gemm_mode numbering) picks the 16-bit type of the planes
static int split_planes(int mode, const char* name, const float* in, void* out, long long rows, int K, void* stream) {
    EXCEL_CHECK_ARG(in && out && rows > 0 && K > 0, "%s: bad argument", name);
    return split_api(mode).split_bf16(in, out, rows, K, ST(stream));
}
extern "C" int excel_split_bf16(const float* in, void* out, long long rows, int K, void* stream) {
    return split_planes(1, "split_bf16", in, out, rows, K, stream);
}
extern "C" int excel_split_f16(const float* in, void* out, long long rows, int K, void* stream) {
    return split_planes(2, "split_f16", in, out, rows, K, stream);
}

extern "C" int excel_pack_f16(const float* in, void* out, long long rows, int K, unsigned long long* inexact_dev, void* stream) {
    EXCEL_CHECK_ARG(in && out && inexact_dev && rows > 0 && K > 0, "pack_f16: bad argument");
    return split_api(2).pack_hi(in, out, rows, K, inexact_dev, ST(stream));
}

static int gemm_split(int mode, const char* name, const void* A_split, const void* W_split, const void* W_half, int w_lo_zero, float* C,
                      const float* bias, const float* residual, int M, int N, int K, int act, int split_out, void* stream) {
    EXCEL_CHECK_ARG(A_split && W_split && C, "%s: null argument", name);
    // (the launcher refuses A_split, W_split, C, bias and residual below 16 bytes; a W_half below 16 bytes is left unused)
    GemmBfArgs g = gemm_bf_args(A_split, (const unsigned short*)W_split, C, C, bias, residual, M, N, K, N, N, act,
                                split_out ? GEMM_OUT_SPLIT_BF16 : GEMM_OUT_PLAIN);
    if (w_lo_zero) { g.w_lo_zero = 1; g.Bh = (const unsigned short*)W_half; g.ldbh = K; }
    return split_api(mode).gemm_bf16x3(g, ST(stream));
}
extern "C" int excel_gemm_bf16x3(const void* A_split, const void* W_split, float* C, const float* bias, const float* residual,
                                 int M, int N, int K, int act, int split_out, void* stream) {
    return gemm_split(1, "gemm_bf16x3", A_split, W_split, nullptr, 0, C, bias, residual, M, N, K, act, split_out, stream);
}
extern "C" int excel_gemm_f16x3(const void* A_split, const void* W_split, float* C, const float* bias, const float* residual,
                                int M, int N, int K, int act, int split_out, void* stream) {
    return gemm_split(2, "gemm_f16x3", A_split, W_split, nullptr, 0, C, bias, residual, M, N, K, act, split_out, stream);
}
extern "C" int excel_gemm_f16x2(const void* A_split, const void* W_split, const void* W_half, float* C, const float* bias,
                                const float* residual, int M, int N, int K, int act, int split_out, void* stream) {
    return gemm_split(3, "gemm_f16x2", A_split, W_split, W_half, 1, C, bias, residual, M, N, K, act, split_out, stream);
}

extern "C" int excel_gemm_plan(int M, int N, int K, int batch, int out_mode, int has_residual, int gemm_mode, int has_half, int n_cu, int32_t* plan) {
    EXCEL_CHECK_ARG(plan && M > 0 && N > 0 && K > 0 && batch >= 1 && out_mode >= GEMM_OUT_PLAIN && out_mode <= GEMM_OUT_SPLIT_BF16 &&
                    gemm_mode >= 1 && gemm_mode <= 3 && n_cu >= 1, "gemm_plan: bad argument");
    // the arguments excel_gemm_bf16x3 / _f16x3 / _f16x2 (gemm_bf_args) and the ViT's linear layers build: dense rows, head dim 64
    const GemmShape s = {M, N, K, 2 * K, 2 * K, N, N, out_mode == GEMM_OUT_QKV_HEADMAJOR ? 64 : 0, out_mode, has_residual != 0, batch,
                         gemm_mode >= 2, gemm_mode == 3, gemm_half_ok(has_half != 0, N, K, K)};
    const GemmPlan p = gemm_plan(s, n_cu);
    const int v[EXCEL_GEMM_PLAN_INTS] = {p.kernel, p.tile, p.nt_m, p.x2, p.tall, p.shrt, p.second, p.grid_x, p.grid_y, p.block};
    for (int i = 0; i < EXCEL_GEMM_PLAN_INTS; ++i) plan[i] = v[i];
    return EXCEL_OK;
}

extern "C" int excel_attn_plan(int B, int H, int N, int gemm_mode, int surgery, int want_w, int32_t* plan) {
    EXCEL_CHECK_ARG(plan && B >= 1 && H >= 1 && N >= 1 && N <= (1 << 20) && (long long)B * H <= 65535 && gemm_mode >= 0 && gemm_mode <= 3 &&
                    (surgery == 0 || surgery == 1) && (want_w == 0 || want_w == 1), "attn_plan: bad argument");
    const AttnPlan p = attn_plan(B, H, N, gemm_mode, surgery, want_w);
    const int v[EXCEL_ATTN_PLAN_INTS] = {p.path, p.ntiles, p.ntw, p.nw, p.nw_full, p.rp_ntypes, p.rp_grid[0], p.rp_grid[1], p.rp_grid[2],
                                         p.grid[0], p.grid[1], p.grid[2], p.block, p.split_c};
    for (int i = 0; i < EXCEL_ATTN_PLAN_INTS; ++i) plan[i] = v[i];
    return EXCEL_OK;
}

extern "C" int excel_patch_text_cam_plan(int B, int N, int C, int T, int gemm_mode, int32_t* plan) {
    EXCEL_CHECK_ARG(plan && B >= 1 && B <= 65535 && N >= 1 && N <= (1 << 20) && T >= 1 && T <= PTC_WIDE_T && C >= 32 && C <= 1024 && (C % 32) == 0 &&
                    gemm_mode >= 0 && gemm_mode <= 3, "patch_text_cam_plan: bad argument");
    const CamPlan p = cam_plan(B, N, C, T, gemm_mode);
    const int v[EXCEL_CAM_PLAN_INTS] = {p.kernel, p.split, p.ct, p.tlds, p.G, p.prep_grid[0], p.prep_grid[1], p.prep_grid[2], p.sim_grid[0],
                                        p.sim_grid[1], p.block, p.finish_grid[0], p.finish_grid[1], p.finish_pitch};
    for (int i = 0; i < EXCEL_CAM_PLAN_INTS; ++i) plan[i] = v[i];
    return EXCEL_OK;
}

extern "C" int excel_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int D, float eps, void* stream) {
    EXCEL_CHECK_ARG(x && w && b && y, "excel_layernorm: null argument");
    return excel_launch_layernorm_f32(x, w, b, y, rows, D, eps, ST(stream));
}

extern "C" size_t excel_train_losses_workspace_bytes(int B, int nc, int H, int W) { return excel_train_losses_ws_bytes(B, nc, H, W); }

extern "C" int excel_train_losses(const float* seg, const float* attn_pred, const unsigned char* pseudo, const unsigned char* aff_labels, int B, int nc,
                                  int g_h, int g_w, int H, int W, int radius, int ignore_index, float w_seg, float w_diver, float* losses,
                                  float* d_seg, float* d_attn_pred, void* workspace, void* stream) {
    return excel_launch_train_losses(seg, attn_pred, pseudo, aff_labels, B, nc, g_h, g_w, H, W, radius, ignore_index, w_seg, w_diver, losses, d_seg,
                                     d_attn_pred, workspace, ST(stream));
}

extern "C" int excel_lam_to_label(const float* cam, const float* cls_label, const int32_t* img_box, int B, int F, int H, int W, float bkg_thre,
                                 float high_thre, float low_thre, int ignore_mid, int ignore_index, float* valid_cam, unsigned char* label,
                                 void* stream) {
    EXCEL_CHECK_ARG(cam && cls_label && label && B > 0 && F > 0 && H > 0 && W > 0, "lam_to_label: bad argument");
    return excel_launch_lam_to_label(cam, cls_label, img_box, B, F, H, W, bkg_thre, high_thre, low_thre, ignore_mid, ignore_index, valid_cam, label,
                                     ST(stream));
}

extern "C" int excel_normalize_img_u8(const unsigned char* hwc, int B, int H, int W, const double* mean3, const double* std3, float* out, void* stream) {
    EXCEL_CHECK_ARG(hwc && out && mean3 && std3 && B > 0 && H > 0 && W > 0, "normalize_img_u8: bad argument");
    return excel_launch_normalize_u8(hwc, out, B, (long long)H * W, mean3, std3, ST(stream));
}

extern "C" int excel_denormalize_img(const float* img, int B, int H, int W, const float* mean3, const float* std3, unsigned char* out_u8,
                                    float* out_f32, void* stream) {
    EXCEL_CHECK_ARG(img && mean3 && std3 && (out_u8 || out_f32) && B > 0 && H > 0 && W > 0, "denormalize_img: bad argument");
    return excel_launch_denormalize(img, out_u8, out_f32, B, (long long)H * W, mean3, std3, ST(stream));
}

extern "C" int excel_seg_scale_accumulate(const float* segs, float* acc, int B, int nc, int h, int w, int H, int W, int flip_mean,
                                         int init, float scale, void* stream) {
    EXCEL_CHECK_ARG(segs && acc && B > 0 && nc > 0 && h > 0 && w > 0 && H > 0 && W > 0, "seg_scale_accumulate: bad argument");
    return excel_launch_seg_scale_accumulate(segs, acc, B, nc, h, w, H, W, flip_mean, init, scale, ST(stream));
}

extern "C" size_t excel_feature_affinity_workspace_bytes(int B, int C, int P) { return excel_feature_affinity_ws_bytes(B, C, P); }

extern "C" int excel_feature_affinity(const float* feats, int B, int C, int P, float beta, float gamma, int mode, float* out,
                                      void* workspace, void* stream) {
    EXCEL_CHECK_ALIGN(workspace, 16, "feature_affinity", "workspace");      // fn, both operands of the similarity GEMM, and the double partials
    return excel_launch_feature_affinity(feats, B, C, P, beta, gamma, mode, out, workspace, ST(stream));
}

extern "C" size_t excel_feature_affinity_grouped_workspace_bytes(int B, int C, int P, int group) {
    return excel_feature_affinity_grouped_ws_bytes(B, C, P, group);
}

extern "C" int excel_feature_affinity_grouped(const float* feats, int B, int C, int P, int group, int member_stride, float beta, float gamma,
                                              int mode, float* out, void* workspace, void* stream) {
    EXCEL_CHECK_ALIGN(workspace, 16, "feature_affinity_grouped", "workspace");
    return excel_launch_feature_affinity_grouped(feats, B, C, P, group, member_stride, beta, gamma, mode, out, workspace, ST(stream));
}

extern "C" size_t excel_attn_select_workspace_bytes(int B, int n_layers) { return excel_attn_select_ws_bytes(B, n_layers); }

extern "C" int excel_attn_select_mean(const float* attn, int Lw, int B, int N, int first_layer, int n_layers, const float* seg_attn,
                                      float* w_out, void* workspace, void* stream) {
    EXCEL_CHECK_ALIGN(workspace, 8, "attn_select_mean", "workspace");       // double partials
    return excel_launch_attn_select_mean(attn, Lw, B, N, first_layer, n_layers, seg_attn, w_out, workspace, ST(stream));
}

// ------------------------------------------------------------------------------------ CAM
struct CamWs { float* S; int ldT; size_t total; };         // S [B*N, ldT]: the token-text similarities, rows padded to 4 floats
static CamWs cam_ws_layout(int B, int N, int T, void* base) {
    CamWs w;
    Workspace ws(base);
    w.ldT = (T + 3) / 4 * 4;
    w.S = ws.take<float>((size_t)B * N * w.ldT);
    w.total = ws.total();
    return w;
}
extern "C" size_t excel_cam_workspace_bytes(int B, int N, int T) { return cam_ws_layout(B, N, T, nullptr).total; }

extern "C" int excel_clip_feature_surgery(const float* image_features, const float* text, int B, int N, int C, int T, int F,
                                          float temperature, float* out_full, float* out_slice, void* workspace, void* stream) {
    EXCEL_CHECK_ARG(image_features && text && workspace && (out_full || out_slice), "clip_feature_surgery: null argument");
    EXCEL_CHECK_ARG((C % 4) == 0, "clip_feature_surgery: C must be a multiple of 4");
    EXCEL_CHECK_ALIGN(image_features, 16, "clip_feature_surgery", "image_features");      // A and B of the similarity GEMM (f32x4 loads)
    EXCEL_CHECK_ALIGN(text, 16, "clip_feature_surgery", "text");
    EXCEL_CHECK_ALIGN(workspace, 16, "clip_feature_surgery", "workspace");
    const CamWs w = cam_ws_layout(B, N, T, workspace);
    // S[b*N+n, t] = f . text[t]  -- one NT GEMM over all B*N token rows (text shared)
    GemmArgs ga = gemm_args(image_features, text, w.S, nullptr, nullptr, B * N, T, C, C, C, w.ldT, 0, GEMM_ACT_NONE);
    TRY(excel_launch_gemm(ga, true, 1, ST(stream)));
    return split_api(0).cam_epilogue(w.S, out_full, out_slice, B, N, T, w.ldT, F, temperature, ST(stream));     // fp32 in, fp32 out
}

// Fused path (cam.hip): token-axis norm + similarity on the matrix core + surgery epilogue, straight from the un-normalised token
// features excel_vit_forward returns as x_raw (+ their token-axis sums of squares x_colsq when the forward produced them).
struct PtcWs { float *sim, *part, *colsq; unsigned short* ts; size_t total; };
static PtcWs ptc_ws_layout(int B, int N, int C, int T, char* base) {
    PtcWs w;
    Workspace ws(base);
    const auto ws_floats = split_api(0).patch_text_cam_ws_floats;      // host arithmetic on the shape: the same for every split type
    w.sim = ws.take<float>(ws_floats(B, N, C, T, 0));
    w.ts = ws.take<unsigned short>((size_t)T * C * 2);        // the split text bank: hi and lo planes
    w.part = ws.take<float>(ws_floats(B, N, C, T, 1));
    w.colsq = ws.take<float>(ws_floats(B, N, C, T, 2));
    w.total = ws.total();
    return w;
}
extern "C" size_t excel_patch_text_cam_workspace_bytes(int B, int N, int C, int T) { return ptc_ws_layout(B, N, C, T, nullptr).total; }

extern "C" int excel_patch_text_cam(const float* x_raw, const float* text, int B, int N, int C, int T, int F, float temperature, int mode,
                                    float* out_full, float* out_slice, float* image_features, void* workspace, void* stream) {
    EXCEL_CHECK_ARG(x_raw && text && workspace && (out_full || out_slice), "patch_text_cam: null argument");
    EXCEL_CHECK_ARG(mode == 0 || mode == 1 || mode == 2, "patch_text_cam: mode must be 0 (exact fp32), 1 (bf16x3) or 2 (f16x3)");
    EXCEL_CHECK_ARG(B > 0 && N > 0 && C > 0 && T > 0, "patch_text_cam: bad shape");
    EXCEL_CHECK_ALIGN(x_raw, 16, "patch_text_cam", "x_raw");                // f32x4 loads, 16-byte LDS DMA of the split text bank (cam.hip)
    EXCEL_CHECK_ALIGN(text, 16, "patch_text_cam", "text");
    EXCEL_CHECK_ALIGN(image_features, 16, "patch_text_cam", "image_features");
    EXCEL_CHECK_ALIGN(workspace, 16, "patch_text_cam", "workspace");
    const int ldT = (T + 3) / 4 * 4;
    const PtcWs w = ptc_ws_layout(B, N, C, T, (char*)workspace);
    return split_api(mode).patch_text_cam(x_raw, text, mode ? w.ts : nullptr, w.sim, w.part, w.colsq, out_full, out_slice, image_features, B, N, C,
                                          T, F, ldT, temperature, mode ? 1 : 0, ST(stream));
}

// ------------------------------------------------------------------------------------ affinity
extern "C" int excel_attn_layer_mean(const float* attn, int Lw, int B, int N, int first_layer, int n_layers, float* w_aff, void* stream) {
    EXCEL_CHECK_ARG(attn && w_aff && first_layer >= 0 && n_layers >= 1 && first_layer + n_layers <= Lw, "attn_layer_mean: bad layer range");
    const long long n = (long long)B * (N - 1) * (N - 1);
    hipLaunchKernelGGL(attn_layer_mean_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, ST(stream), attn, B, N, first_layer, n_layers, w_aff);
    EXCEL_CHECK_LAUNCH("attn_layer_mean");
    return EXCEL_OK;
}

// random walk: the transition matrix T and its symmetrised form [B,P,P], the column sums [B,P]; the refinement adds the masked score
// maps v and the intermediate u = Tsym v [B,Smax,P] (Smax = 0: none)
struct WalkWs { float *T, *Tsym, *cs, *v, *u; size_t total; };
static WalkWs walk_ws_layout(int B, int P, int Smax, void* base) {
    WalkWs w;
    Workspace ws(base);
    w.T = ws.take<float>((size_t)B * P * P);
    w.Tsym = ws.take<float>((size_t)B * P * P);
    w.cs = ws.take<float>((size_t)B * P);
    w.v = ws.take<float>((size_t)B * Smax * P);
    w.u = ws.take<float>((size_t)B * Smax * P);
    w.total = ws.total();
    return w;
}
extern "C" size_t excel_trans_mat_workspace_bytes(int B, int P) { return walk_ws_layout(B, P, 0, nullptr).total; }

extern "C" int excel_compute_trans_mat(const float* w_aff, int B, int P, float* trans_out, void* workspace, void* stream) {
    EXCEL_CHECK_ARG(w_aff && trans_out && workspace, "compute_trans_mat: null argument");
    EXCEL_CHECK_ARG((P % 4) == 0, "compute_trans_mat: P must be a multiple of 4 (P=%d)", P);
    EXCEL_CHECK_ALIGN(workspace, 16, "compute_trans_mat", "workspace");     // Tsym is both operands of the squaring GEMM
    const WalkWs w = walk_ws_layout(B, P, 0, workspace);
    TRY(excel_launch_trans_mat_sym(w_aff, w.T, w.Tsym, w.cs, B, P, ST(stream)));
    // Tsym . Tsym ; Tsym symmetric => B operand [N,K] = Tsym itself (NT form)
    GemmArgs ga = gemm_args(w.Tsym, w.Tsym, trans_out, nullptr, nullptr, P, P, P, P, P, P, 0, GEMM_ACT_NONE);
    ga.sA = ga.sB = ga.sC = (long long)P * P;
    return excel_launch_gemm(ga, true, B, ST(stream));
}

extern "C" int excel_cls_compact(const float* onehot, int B, int F, int Smax, int32_t* cls_idx, int32_t* ncls, int32_t* nchan,
                                 void* stream) {
    EXCEL_CHECK_ARG(onehot && cls_idx && ncls && Smax >= 1, "cls_compact: bad argument");
    return excel_launch_cls_compact(onehot, B, F, Smax, cls_idx, ncls, nchan, ST(stream));
}

extern "C" int excel_scoremap_box_mask(const float* attr, const int32_t* cls_idx, const int32_t* ncls, int B, int g, int F, int Smax,
                                       double caa_thre, float* v_out, uint8_t* mask_out, void* stream) {
    EXCEL_CHECK_ARG(attr && cls_idx && ncls && v_out, "scoremap_box_mask: null argument");
    return excel_launch_bbox_mask(attr, cls_idx, ncls, B, g, F, Smax, caa_thre, v_out, mask_out, ST(stream));
}

extern "C" size_t excel_refine_workspace_bytes(int B, int P, int Smax) { return walk_ws_layout(B, P, Smax, nullptr).total; }

extern "C" int excel_refine_cams_with_aff(const float* attr, const float* w_aff, const int32_t* cls_idx, const int32_t* ncls, int B,
                                          int g, int F, int Smax, double caa_thre, float* refined, void* workspace, void* stream) {
    EXCEL_CHECK_ARG(attr && w_aff && cls_idx && ncls && refined && workspace, "refine_cams_with_aff: null argument");
    const int P = g * g;
    const WalkWs w = walk_ws_layout(B, P, Smax, workspace);
    hipStream_t st = ST(stream);
    TRY(excel_launch_trans_mat_sym(w_aff, w.T, w.Tsym, w.cs, B, P, st));
    TRY(excel_launch_bbox_mask(attr, cls_idx, ncls, B, g, F, Smax, caa_thre, w.v, nullptr, st));
    TRY(excel_launch_matvec(w.Tsym, w.v, ncls, w.u, B, P, Smax, st));        // u = Tsym (mask.g)
    TRY(excel_launch_matvec(w.Tsym, w.u, ncls, refined, B, P, Smax, st));    // refined = Tsym u = (Tsym.Tsym)(mask.g)
    return EXCEL_OK;
}

extern "C" int excel_cam_upsample_bkg(const float* refined, const int32_t* ncls, int B, int g, int Smax, int H, int W, float* cams,
                                      void* workspace, int flags, void* stream) {
    EXCEL_CHECK_ARG(refined && ncls && cams && workspace, "cam_upsample_bkg: null argument");
    return excel_launch_cam_upsample_bkg(refined, ncls, (float*)workspace, cams, B, g, Smax, H, W, (flags & EXCEL_CAMS_ZERO_UNUSED) ? 1 : 0, ST(stream));
}

// ------------------------------------------------------------------------------------ ragged batches (images of different sizes)
extern "C" int excel_ragged_plan(const int32_t* hw, int B, excel_ragged_info* info, int32_t* table) {
    EXCEL_CHECK_ARG(hw && info && B >= 1, "ragged_plan: bad argument");
    long long pix = 0, lab = 0, tiles = 0, max_plane = 0;
    for (int b = 0; b < B; ++b) {
        const long long H = hw[2 * b], W = hw[2 * b + 1];
        EXCEL_CHECK_ARG(H >= 1 && W >= 1, "ragged_plan: image %d has size %lld x %lld", b, H, W);
        const long long Wp = (W + 3) / 4 * 4, plane = H * Wp, nt = ((W + 63) / 64) * ((H + 15) / 16);
        if (table) {
            int32_t* rec = table + EXCEL_RAG_REC * b;
            rec[0] = (int32_t)H; rec[1] = (int32_t)W; rec[2] = (int32_t)pix; rec[3] = (int32_t)tiles; rec[4] = (int32_t)lab; rec[5] = rec[6] = rec[7] = 0;
            for (long long t = 0; t < nt; ++t) table[EXCEL_RAG_REC * (B + 1) + tiles + t] = b;
        }
        pix += plane; lab += H * W; tiles += nt;
        if (plane > max_plane) max_plane = plane;
        EXCEL_CHECK_ARG(pix < (1LL << 31) && 3 * lab < (1LL << 31) && tiles < (1LL << 31), "ragged_plan: batch too large for 32-bit offsets");
    }
    if (table) {
        int32_t* rec = table + EXCEL_RAG_REC * B;
        rec[0] = rec[1] = 0; rec[2] = (int32_t)pix; rec[3] = (int32_t)tiles; rec[4] = (int32_t)lab; rec[5] = rec[6] = rec[7] = 0;
    }
    info->B = B; info->total_tiles = (int32_t)tiles; info->total_pix = pix; info->total_label_pix = lab; info->max_plane_pix = max_plane;
    info->table_ints = EXCEL_RAG_REC * (long long)(B + 1) + tiles;
    return EXCEL_OK;
}

static TileGeo ragged_geo(const int32_t* table, int B) {
    TileGeo g;
    g.tab = table; g.B = B; g.H = g.W = 0;
    return g;
}
static TileGeo uniform_geo(int B, int H, int W) {
    TileGeo g;
    g.tab = nullptr; g.B = B; g.H = H; g.W = W;
    return g;
}

extern "C" int excel_normalize_resize_u8_ragged(const uint8_t* hwc, const int32_t* table, int B, int S, const double* mean3, const double* std3,
                                                float* out, void* stream) {
    EXCEL_CHECK_ARG(hwc && table && out && mean3 && std3 && B > 0 && S > 0, "normalize_resize_u8_ragged: bad argument");
    return excel_launch_normalize_resize_u8_ragged(hwc, out, ragged_geo(table, B), S, mean3, std3, ST(stream));
}

extern "C" int excel_normalize_resize_u8_ragged_mirror(const uint8_t* hwc, const int32_t* table, int B, int S, const double* mean3,
                                                       const double* std3, float* out, void* stream) {
    EXCEL_CHECK_ARG(hwc && table && out && mean3 && std3 && B > 0 && S > 0, "normalize_resize_u8_ragged_mirror: bad argument");
    return excel_launch_normalize_resize_u8_ragged_mirror(hwc, out, ragged_geo(table, B), S, mean3, std3, ST(stream));
}

extern "C" int excel_cam_upsample_bkg_ragged(const float* refined, const int32_t* ncls, const int32_t* table, const excel_ragged_info* info, int g,
                                             int Smax, float* cams, void* workspace, int flags, void* stream) {
    EXCEL_CHECK_ARG(refined && ncls && table && info && cams && workspace, "cam_upsample_bkg_ragged: null argument");
    EXCEL_CHECK_ARG((((uintptr_t)cams) & 15) == 0, "cam_upsample_bkg_ragged: cams must be 16-byte aligned");
    return excel_launch_cam_upsample_bkg_ragged(refined, ncls, (float*)workspace, cams, g, Smax, ragged_geo(table, info->B), info->total_tiles,
                                                (flags & EXCEL_CAMS_ZERO_UNUSED) ? 1 : 0, ST(stream));
}

// ------------------------------------------------------------------------------------ training augmentation (datasets/voc.py:110-117)
// aug.hip
int excel_aug_plan(const int32_t* hw, const excel_aug_params* prm, int B, int S, excel_train_aug_info* info, int32_t* table);
int excel_launch_train_augment(const unsigned char* hwc, const unsigned char* labels, const int* table, const excel_train_aug_info& info,
                               const double* mean, const double* stdv, float* img, unsigned char* label, int* img_box, void* workspace,
                               hipStream_t st);
int excel_launch_train_augment_image(const unsigned char* hwc, const int* table, const excel_train_aug_info& info, const double* mean,
                                     const double* stdv, float* img, int* img_box, void* workspace, hipStream_t st);
extern "C" int excel_train_aug_plan(const int32_t* hw, const excel_aug_params* params, int B, int S, excel_train_aug_info* info, int32_t* table) {
    return excel_aug_plan(hw, params, B, S, info, table);
}

extern "C" size_t excel_train_augment_workspace_bytes(const excel_train_aug_info* info) {
    return info ? (size_t)info->workspace_bytes : 0;
}

extern "C" int excel_train_augment(const uint8_t* hwc, const uint8_t* labels, const int32_t* table, const excel_train_aug_info* info,
                                   const double* mean3, const double* std3, float* img, uint8_t* label, int32_t* img_box, void* workspace,
                                   void* stream) {
    EXCEL_CHECK_ARG(hwc && labels && table && info && mean3 && std3 && img && label && img_box && workspace, "train_augment: null argument");
    EXCEL_CHECK_ARG(info->B >= 1 && info->S >= 1 && info->max_h >= 1 && info->max_w2 >= 1 && info->workspace_bytes > 0,
                    "train_augment: info was not filled by excel_train_aug_plan");
    return excel_launch_train_augment(hwc, labels, table, *info, mean3, std3, img, label, img_box, workspace, ST(stream));
}

extern "C" int excel_train_augment_image(const uint8_t* hwc, const int32_t* table, const excel_train_aug_info* info, const double* mean3,
                                         const double* std3, float* img, int32_t* img_box, void* workspace, void* stream) {
    EXCEL_CHECK_ARG(hwc && table && info && mean3 && std3 && img && img_box && workspace, "train_augment_image: null argument");
    EXCEL_CHECK_ARG(info->B >= 1 && info->S >= 1 && info->max_h >= 1 && info->max_w2 >= 1 && info->workspace_bytes > 0,
                    "train_augment_image: info was not filled by excel_train_aug_plan");
    return excel_launch_train_augment_image(hwc, table, *info, mean3, std3, img, img_box, workspace, ST(stream));
}

// ------------------------------------------------------------------------------------ PAR / labels / metric
// affinities [aff_planes planes: 8 per dilation streamed, or the 5 statistics the step recomputes them from] + ping-pong [Cmax planes] +
// resized guide [3 planes]; `pix` = the pixels of one plane over the whole batch (ragged: in the pitched layout)
struct ParWs { float *aff, *pp, *guide; size_t total; };
static ParWs par_ws_layout(size_t pix, int aff_planes, int Cmax, void* base) {
    ParWs w;
    Workspace ws(base);
    w.aff = ws.take<float>(aff_planes * pix);
    w.pp = ws.take<float>(Cmax * pix);
    w.guide = ws.take<float>(3 * pix);
    w.total = ws.total();
    return w;
}
static ParWs par_ws_uniform(int B, int Cmax, int H, int W, int ndil, void* base) { return par_ws_layout((size_t)B * H * W, 8 * ndil, Cmax, base); }
static ParWs par_ws_ragged(long long total_pix, int Cmax, void* base) { return par_ws_layout((size_t)total_pix, 5, Cmax, base); }
extern "C" size_t excel_par_workspace_bytes(int B, int Cmax, int H, int W, int ndil) { return par_ws_uniform(B, Cmax, H, W, ndil, nullptr).total; }

// ping-pong so that the LAST step writes `out`: out, pp alternate backwards from the end
template <class Step>
static int par_jacobi(const float* masks, float* out, float* pp, int n_iter, Step step) {
    const float* cur = masks;
    for (int it = 0; it < n_iter; ++it) {
        float* dst = (((n_iter - 1 - it) & 1) == 0) ? out : pp;
        TRY(step(cur, dst));
        cur = dst;
    }
    return EXCEL_OK;
}

extern "C" int excel_par_forward(const float* imgs, int h, int w, const float* masks, const int32_t* nchan, int B, int Cmax, int H,
                                 int W, const int32_t* dilations, int ndil, int n_iter, float w1, float w2, float* out,
                                 void* workspace, int flags, void* stream) {
    EXCEL_CHECK_ARG(imgs && masks && out && workspace && dilations, "par_forward: null argument");
    EXCEL_CHECK_ARG(n_iter >= 0 && ndil >= 1 && ndil <= 8, "par_forward: bad n_iter/ndil");
    EXCEL_CHECK_ARG(B > 0 && Cmax > 0 && H > 0 && W > 0 && h > 0 && w > 0, "par_forward: bad shape");
    // fp32 planes are carved from the workspace; 4 bytes is all the streamed kernels need (16-byte aligned buffers: see aligned16 below)
    EXCEL_CHECK_ALIGN(workspace, 4, "par_forward", "workspace");
    const size_t hw = (size_t)H * W;
    const ParWs ws = par_ws_uniform(B, Cmax, H, W, ndil, workspace);
    float *aff = ws.aff, *pp = ws.pp, *guide = ws.guide;
    hipStream_t st = ST(stream);
    // the resize, the form of the affinities (streamed planes or statistics the step recomputes them from) and both kernels: par_plan.hip
    const float* gimg = (h != H || w != W) ? guide : imgs;
    const bool aligned16 = ((((uintptr_t)gimg | (uintptr_t)aff | (uintptr_t)masks | (uintptr_t)out | (uintptr_t)pp) & 15) == 0);
    const ParShape shape = {B, Cmax, h, w, H, W, (long long)hw, 0, dilations, ndil, n_iter, (flags & EXCEL_PAR_STREAM_AFFINITIES) ? 1 : 0, 0, aligned16};
    const ParPlan plan = par_plan(shape);
    if (plan.resize) TRY(excel_launch_bilinear_ac(imgs, guide, B * 3, h, w, H, W, st));   // F.interpolate(..., align_corners=True) (PAR.py:67)
    const TileGeo geo = uniform_geo(B, H, W);
    TRY(excel_launch_par_affinity(gimg, aff, geo, dilations, ndil, w1, w2, plan, st));
    if (plan.step == PAR_STEP_NONE) {
        hipMemcpyAsync(out, masks, sizeof(float) * (size_t)B * Cmax * hw, hipMemcpyDeviceToDevice, st);
        return EXCEL_OK;
    }
    if (plan.step == PAR_STEP_RECOMPUTE)
        return par_jacobi(masks, out, pp, n_iter, [&](const float* cur, float* dst) {
            return excel_launch_par_iterate_guide(gimg, aff, cur, dst, nchan, Cmax, geo, dilations, ndil, w1, w2, plan, st);
        });
    return par_jacobi(masks, out, pp, n_iter, [&](const float* cur, float* dst) {
        return excel_launch_par_iterate(aff, cur, dst, nchan, Cmax, H, W, dilations, ndil, w1, w2, plan, st);
    });
}

extern "C" size_t excel_par_ragged_workspace_bytes(long long total_pix, int Cmax) { return par_ws_ragged(total_pix, Cmax, nullptr).total; }

extern "C" int excel_par_forward_ragged(const float* imgs, int h, int w, const float* masks, const int32_t* nchan, const int32_t* table,
                                        const excel_ragged_info* info, int Cmax, const int32_t* dilations, int ndil, int n_iter, float w1,
                                        float w2, float* out, void* workspace, void* stream) {
    EXCEL_CHECK_ARG(imgs && masks && out && workspace && dilations && table && info, "par_forward_ragged: null argument");
    EXCEL_CHECK_ARG(Cmax > 0 && h > 0 && w > 0 && info->B > 0, "par_forward_ragged: bad n_iter / shape");
    // the tile kernels stage masks, the statistics and the guide in 16-byte pieces (par.hip).  These name the pointer; the plan's own
    // alignment refusal (PAR_REFUSE_ALIGN, reason 3) can then no longer be met here and is kept for excel_par_plan's callers
    EXCEL_CHECK_ALIGN(masks, 16, "par_forward_ragged", "masks");
    EXCEL_CHECK_ALIGN(out, 16, "par_forward_ragged", "out");
    EXCEL_CHECK_ALIGN(workspace, 16, "par_forward_ragged", "workspace");
    const ParWs ws = par_ws_ragged(info->total_pix, Cmax, workspace);
    float *stats = ws.aff, *pp = ws.pp, *guide = ws.guide;
    hipStream_t st = ST(stream);
    const TileGeo geo = ragged_geo(table, info->B);
    const bool aligned16 = ((((uintptr_t)guide | (uintptr_t)stats | (uintptr_t)masks | (uintptr_t)out | (uintptr_t)pp) & 15) == 0);
    const ParShape shape = {info->B, Cmax, h, w, 0, 0, info->max_plane_pix, info->total_tiles, dilations, ndil, n_iter, 0, 1, aligned16};
    const ParPlan plan = par_plan(shape);
    EXCEL_CHECK_ARG(plan.refused != PAR_REFUSE_NITER, "par_forward_ragged: bad n_iter / shape");
    EXCEL_CHECK_ARG(!plan.refused,
                    "par_forward_ragged: needs dilations [1,2,4,8,12,24] and max(Cmax,5) * H * Wp * 4 < 2^31 per image "
                    "(Wp = W rounded up to 4)");
    TRY(excel_launch_bilinear_ac_ragged(imgs, guide, h, w, geo, info->total_tiles, st));
    TRY(excel_launch_par_affinity(guide, stats, geo, dilations, ndil, w1, w2, plan, st));
    return par_jacobi(masks, out, pp, n_iter, [&](const float* cur, float* dst) {
        return excel_launch_par_iterate_guide(guide, stats, cur, dst, nchan, Cmax, geo, dilations, ndil, w1, w2, plan, st);
    });
}

// (a batch of B images of H x W each stands for the ragged batch: its largest plane and its tile list are what the launch depends on)
extern "C" int excel_par_plan(int B, int Cmax, int h, int w, int H, int W, const int32_t* dilations, int ndil, int n_iter, int flags, int ragged,
                              int aligned16, int32_t* plan) {
    EXCEL_CHECK_ARG(plan && dilations && B >= 1 && Cmax >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && ndil >= 1 && ndil <= 8 && n_iter >= 0 &&
                    (flags & ~EXCEL_PAR_STREAM_AFFINITIES) == 0 && (ragged == 0 || ragged == 1) && (aligned16 == 0 || aligned16 == 1),
                    "par_plan: bad argument");
    for (int i = 0; i < ndil; ++i) EXCEL_CHECK_ARG(dilations[i] >= 1, "par_plan: dilations must be >= 1 (got %d)", dilations[i]);
    const long long Wp = ragged ? (W + 3LL) / 4 * 4 : W, tiles = (long long)B * ((W + 63) / 64) * ((H + 15) / 16);
    EXCEL_CHECK_ARG(B <= 65535 && tiles < (1LL << 31), "par_plan: batch too large for one launch");
    const ParShape shape = {B, Cmax, h, w, H, W, (long long)H * Wp, ragged ? (int)tiles : 0, dilations, ndil, n_iter, flags ? 1 : 0, ragged, aligned16};
    const ParPlan p = par_plan(shape);
    const int v[EXCEL_PAR_PLAN_INTS] = {p.resize, p.stats, p.nd, p.step, p.stats_grid[0], p.stats_grid[1], p.stats_grid[2], p.stats_block,
                                        p.step_grid[0], p.step_grid[1], p.step_grid[2], p.step_block, p.tiles_interior, p.tiles_border, p.refused};
    for (int i = 0; i < EXCEL_PAR_PLAN_INTS; ++i) plan[i] = v[i];
    return EXCEL_OK;
}

extern "C" int excel_argmax_label_ragged(const float* cams, const int32_t* nchan, const int32_t* cls_idx, const int32_t* table,
                                         const excel_ragged_info* info, int Smax, int Cmax, uint8_t* labels_u8, void* stream) {
    EXCEL_CHECK_ARG(cams && table && info && labels_u8, "argmax_label_ragged: null argument");
    return excel_launch_argmax_label_ragged(cams, nchan, cls_idx, Smax, Cmax, ragged_geo(table, info->B), info->total_tiles, labels_u8, ST(stream));
}

extern "C" int excel_argmax_label(const float* cams, const int32_t* nchan, const int32_t* cls_idx, int B, int Smax, int Cmax,
                                  long long HW, uint8_t* labels_u8, int64_t* labels_i64, void* stream) {
    EXCEL_CHECK_ARG(cams && (labels_u8 || labels_i64), "argmax_label: null argument");
    EXCEL_CHECK_ALIGN(labels_i64, 8, "argmax_label", "labels_i64");
    return excel_launch_argmax_label(cams, nchan, cls_idx, B, Smax, Cmax, HW, labels_u8, (long long*)labels_i64, ST(stream));
}

// ------------------------------------------------------------------------------------ one-time / auxiliary
extern "C" int excel_attr_aggregate(const float* text, const float* bank, int F, int T, int C, int K, double topK, float* out,
                                    void* stream) {
    EXCEL_CHECK_ARG(text && bank && out, "attr_aggregate: null argument");
    const int drop = (int)((1.0 - topK) * (double)K);       // topk = int((1-topK) * K)  (load_attr.py:100)
    return excel_launch_attr_aggregate(text, bank, F, T, C, K, drop, out, ST(stream));
}

extern "C" int excel_bilinear_resize(const float* in, float* out, long long planes, int h, int w, int H, int W, int align_corners,
                                     void* stream) {
    EXCEL_CHECK_ARG(in && out && planes > 0 && h > 0 && w > 0 && H > 0 && W > 0, "bilinear_resize: bad argument");
    return excel_launch_bilinear_resize(in, out, planes, h, w, H, W, align_corners, ST(stream));
}

extern "C" int excel_flip_max_normalize(const float* attr, float* out, int B, int g, int F, void* stream) {
    EXCEL_CHECK_ARG(attr && out, "flip_max_normalize: null argument");
    return excel_launch_flip_max_normalize(attr, out, B, g, F, ST(stream));
}

extern "C" int excel_lam_scale_accumulate(const float* maps, float* acc, int B, int g, int F, int H, int W, int init, void* stream) {
    EXCEL_CHECK_ARG(maps && acc && B > 0 && g > 0, "lam_scale_accumulate: bad argument");
    return excel_launch_lam_scale_accumulate(maps, acc, B, g, F, H, W, init, ST(stream));
}

extern "C" int excel_plane_minmax_normalize(float* lam, long long planes, long long HW, void* stream) {
    EXCEL_CHECK_ARG(lam && planes > 0 && HW > 0, "plane_minmax_normalize: bad argument");
    return excel_launch_plane_minmax_normalize(lam, planes, HW, ST(stream));
}
