// Internal (C++) launch interfaces shared between the .hip translation units.  The launchers built once are declared at global scope;
// those built per 16-bit split type live in namespaces excel_bf16 / excel_f16 and are called through the SplitApi table below.
#pragma once
#include <hip/hip_runtime.h>

enum { GEMM_ACT_NONE = 0, GEMM_ACT_QUICKGELU = 1, GEMM_ACT_RELU = 2 };
enum { GEMM_OUT_PLAIN = 0, GEMM_OUT_QKV_HEADMAJOR = 1, GEMM_OUT_SPLIT_BF16 = 2 };

struct GemmArgs {
    const float* A;
    const float* B;
    float* C;
    const float* bias;   // [N] or null
    const float* res;    // [M,ldr] or null (may alias C: x += ...)
    int M, N, K;         // K = true reduction length (rows of B guarded by it in NN mode)
    int Kld;             // K rounded up to a multiple of 4 that A (and B in NT mode) can be read to;
                         // the operands must hold zeros (or finite*0-safe data with the other side zero) there
    int lda, ldb, ldc, ldr;
    long long sA, sB, sC, sR, sBias;   // batch strides in elements, applied to z / zdiv
    int zdiv;                          // blockIdx.z = z1*zdiv + z2 (zdiv >= 1)
    long long sA2, sB2, sC2;           // strides applied to z % zdiv
    int act;
    int out_mode;
    int tokN, heads, hd;  // GEMM_OUT_QKV_HEADMAJOR: C is [B,3,heads,tokN,hd]
    float alpha;
};
// one unbatched plain-output GEMM (Kld = K rounded up to 4, alpha = 1); callers set strides / out_mode / alpha on the result
inline GemmArgs gemm_args(const float* A, const float* B, float* C, const float* bias, const float* res, int M, int N, int K, int lda, int ldb,
                          int ldc, int ldr, int act) {
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.res = res;
    g.M = M; g.N = N; g.K = K; g.Kld = (K + 3) / 4 * 4;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldr = ldr;
    g.act = act; g.out_mode = GEMM_OUT_PLAIN; g.alpha = 1.f; g.zdiv = 1;
    return g;
}

// bf16x3 GEMM (gemm_bf16x3.hip): A, B are "split" tensors [rows][2][K] bf16 (hi plane, lo plane)
struct GemmBfArgs {
    const unsigned short* A;   // [M][2][K]  (lda = elements per row >= 2K)
    const unsigned short* B;   // [N][2][K]
    float* C;                  // fp32 output (plain / head-major)
    unsigned short* Cs;        // split output [M][2][N] (GEMM_OUT_SPLIT_BF16)
    const float* bias;
    const float* res;
    int M, N, K;
    int lda, ldb, ldc, ldr;
    int act, out_mode;
    int tokN, heads, hd;
    unsigned short* qkv_split;   // GEMM_OUT_QKV_HEADMAJOR: also write q|k|v head-major in split format [B,3,H,N][2][hd] (may be null)
    int dbg;                     // dev only: bit0 = skip MFMA/LDS-read work, bit1 = skip the staging loads after the first tile
    int batch;                   // >= 1: blockIdx.y; operands advance by sA / sB bf16 elements, C by sC floats, Cs by sCs bf16 elements
    long long sA, sB, sC, sCs;
    int mix_tall, mix_short;     // set by the launcher (mixed-height 320x256 / 256x256 row tiles, gemm_bf16x3.hip); 0 = uniform tiles
    int mix_first;               // short tiles dispatched FIRST in every XCD's chunk (the rest follow the tall ones): staggers the epilogues
    // "f16x2" (IEEE-half split type only): the caller guarantees that B's lo plane is all zero (fp16-valued weights) - the a.hi x b.lo
    // products are skipped (bit-identical results, 2 MFMAs per product).  Bh (optional): the same weights as a plain half matrix
    // [N][ldbh >= K], the four-wave kernel's compact operand (gemm_w4x2.hip)
    int w_lo_zero;
    const unsigned short* Bh;
    int ldbh;
};

// Kernel selection of the split-plane GEMM (gemm_plan.hip): a problem as integers and flags -> the instance and grid it runs on
struct GemmShape {
    int M, N, K, lda, ldb, ldc, ldr, hd, out_mode, has_residual, batch;
    int f16;         // IEEE-half split planes (namespace excel_f16): the two-product kernels exist
    int w_lo_zero;   // GemmBfArgs::w_lo_zero
    int half_ok;     // the compact half weights are usable (gemm_half_ok)
};
enum { GEMM_8WAVE = 0, GEMM_8WAVE_MIXED = 1, GEMM_W4 = 2, GEMM_W4_MIX = 3 };
struct GemmPlan {
    int kernel;                // GEMM_8WAVE: uniform tiles of gemm_bf16x3.hip; GEMM_8WAVE_MIXED: its 320- / 256-row mixed-height tiles;
                               // GEMM_W4: one four-wave instance (gemm_w4.hip, gemm_w4x2.hip); GEMM_W4_MIX: a launch of two of them
    int tile;                  // 8-wave tile: 0 128x128, 1 256x128, 2 256x256, 3 320x256
    int nt_m;                  // GEMM_W4: 10 / 8 / 5 = 320- / 256- / 160-row tiles
    int x2;                    // two-product kernel: 1 weights in the split layout, 2 as the plain half matrix GemmBfArgs::Bh
    int tall, shrt, second;    // mixed / two-instance launches: row tiles of 320 rows, then of the short height (GEMM_W4_MIX: instance 8 / 5)
    int grid_x, grid_y, block;
};
constexpr int GEMM_W4_BN = 256;          // columns of a four-wave tile (w4::BN, gemm_w4_body.inc)
GemmPlan gemm_plan(const GemmShape& s, int n_cu);
// Kernel selection of the ViT attention (attn_plan.hip): which kernels one layer's attention runs on, with their grids.  Host arithmetic
// on integers, shared by the launchers (attn.hip, attn_f32.hip, attn_strip.hip), the ViT forward and the host query of the C ABI (excel_attn_plan).
enum { ATTN_STRIP = 0, ATTN_TWOPASS_SPLIT = 1, ATTN_TWOPASS_F32 = 2 };
constexpr int ATTN_STRIP_MAX_TILES = 40;   // the strip-resident kernel keeps 32 query rows x ALL keys in registers: 8 waves x 5 key tiles of 32
struct AttnPlan {
    int path;                  // ATTN_STRIP: flash row pass + attn_strip_kernel<ntw>; ATTN_TWOPASS_SPLIT: row pass + attn_accum_bf_kernel (split
                               // modes beyond the strip envelope); ATTN_TWOPASS_F32: row pass + attn_accum_kernel (exact fp32)
    int ntiles;                // key tiles of 32: cdiv(N, 32) (also the number of 32-row query strips)
    int ntw, nw, nw_full;      // strip: tiles per wave (the instance), waves, waves that own ntw tiles (the others own ntw - 1)
    int rp_ntypes;             // row pass: 1 = q.k alone, 4 = q.k, q.q, k.k, v.v (a surgery layer on a two-pass path)
    int rp_grid[3];            // row pass grid (256 threads)
    int grid[3], block;        // second kernel (strip / accumulate); all 0 when the layer needs none (no surgery, no weights wanted)
    int split_c;               // strip with both sweeps: strips per XCD chunk (StripArgs::split_c), else 0
};
AttnPlan attn_plan(int B, int H, int N, int gemm_mode, int surgery, int want_w);
// Kernel selection of the fused patch-text CAM (cam_plan.hip): which instance of the similarity kernel runs for (mode, T, C), with the
// grids of its three launches.  Host arithmetic on integers, shared by the launcher (cam.hip: it launches exactly what the plan names)
// and the host query of the C ABI (excel_patch_text_cam_plan).
enum { CAM_NARROW = 0, CAM_WIDE = 1 };
constexpr int PTC_MAXCT = 4;          // class tiles of 32 held in accumulators at once: T <= 128 in one pass, wider vocabularies in chunks
constexpr int PTC_WIDE_T = 512;       // rows of the wide path (patch_text_sim_wide_kernel)
constexpr int PTC_NW = 4;             // waves (= token tiles) per workgroup
constexpr int PTC_HB = 64;            // tokens per column-norm block
constexpr int PTC_TLDS_ROWS = 48;     // the split text bank is staged in LDS up to this many rows ...
constexpr int PTC_TLDS_C = 512;       // ... of this many columns (and C % 256 == 0: whole 1-KB LDS-DMA pieces per split row)
struct CamPlan {
    int kernel;                // CAM_NARROW: patch_text_sim_kernel<split, ct, tlds> (T <= 128); CAM_WIDE: patch_text_sim_wide_kernel<split>
    int split;                 // a split-plane mode (bf16x3, f16x3, f16x2): 16-bit MFMAs on hi / lo planes; 0: exact fp32
    int ct;                    // narrow: the instantiated class tiles of 32 (1 / 2 / 4); wide: 0
    int tlds;                  // narrow split instances: the text bank is staged in LDS
    int G;                     // workgroups per image: cdiv(cdiv(N, 32), PTC_NW)
    int prep_grid[3];          // patch_text_prep_kernel, 256 threads
    int sim_grid[2], block;    // the similarity kernel
    int finish_grid[2];        // patch_text_finish_kernel<finish_pitch>, 256 threads
    int finish_pitch;          // row pitch of the per-workgroup min / max table: 128 (narrow) or 512 (wide)
};
CamPlan cam_plan(int B, int N, int C, int T, int gemm_mode);
// the plain half matrix of the weights, [N][ldbh] at a 16-byte aligned address, can feed the compact-weight four-wave instances
inline bool gemm_half_ok(bool aligned, int N, int K, int ldbh) {
    return aligned && ldbh >= K && (ldbh & 7) == 0 && (long long)N * ldbh * 2 < 0x7fffffffLL;
}

// exact-fp32 GEMM (gemm.hip) and the exact-fp32 attention of an ATTN_TWOPASS_F32 plan (attn_f32.hip)
int excel_launch_gemm(const GemmArgs& p, bool b_kmajor, int batch, hipStream_t stream);
int excel_launch_attn_rowpass_f32(const float* qkvh, float* out, float* stats, int B, int H, int N, int hd, float scale,
                                  const AttnPlan& plan, hipStream_t st, int flash_nq);
int excel_launch_attn_accum_f32(const float* qkvh, const float* stats, float* a_sum, float* w_aff, float* attn_out, int B, int H,
                                int N, int NP, int hd, float scale, int surgery, float w_scale, float aff_scale, int aff_init,
                                const AttnPlan& plan, hipStream_t st, const float* ex_attn);

int excel_launch_trans_mat_sym(const float* W, float* T, float* Tsym, float* cs, int B, int P, hipStream_t st);
int excel_launch_cls_compact(const float* onehot, int B, int F, int Smax, int* cls_idx, int* ncls, int* nchan, hipStream_t st);
int excel_launch_bbox_mask(const float* attr, const int* cls_idx, const int* ncls, int B, int g, int F, int Smax, double thre,
                           float* v_out, unsigned char* mask_out, hipStream_t st);
int excel_launch_matvec(const float* T, const float* v, const int* ncls, float* u, int B, int P, int Smax, hipStream_t st);
int excel_launch_cam_upsample_bkg(const float* r, const int* ncls, float* rn, float* cams, int B, int g, int Smax, int H, int W,
                                  int zero_unused, hipStream_t st);
struct TileGeo;
// Kernel selection of the pixel-adaptive refinement (par_plan.hip): the statistics kernel and its output form, the step kernel, the
// grids of both launches and the tile kinds of one image.  Host arithmetic on integers, shared by excel_par_forward,
// excel_par_forward_ragged, the launchers of par.hip (they launch exactly what the plan names) and the host query of the C ABI
// (excel_par_plan).
enum { PAR_STATS_TILE = 0, PAR_STATS_POINT_COMPACT = 1, PAR_STATS_POINT_PLANES = 2 };
enum { PAR_STEP_NONE = 0, PAR_STEP_RECOMPUTE = 1, PAR_STEP_STREAM = 2 };
enum { PAR_REFUSE_NITER = 1, PAR_REFUSE_DILATIONS = 2, PAR_REFUSE_ALIGN = 3, PAR_REFUSE_SIZE = 4 };
constexpr int PAR_HALO = 24;          // the largest dilation of the standard set: halo of a 64 x 16 tile
struct ParShape {
    int B, Cmax;
    int h, w;                  // the guide as given (network input)
    int H, W;                  // masks of a uniform batch; ragged: one image (tile kinds), or 0 for a batch of mixed sizes
    long long max_plane;       // the largest H_b * Wp_b of the launch (uniform: H * W)
    int total_tiles;           // ragged: 64 x 16 tiles of the whole batch
    const int* dil;            // host
    int ndil, n_iter;
    int stream;                // EXCEL_PAR_STREAM_AFFINITIES
    int ragged;
    int aligned16;             // guide, statistics, masks, out and the ping-pong buffer are 16-byte aligned
};
struct ParPlan {
    int resize;                // the guide goes through the align_corners=True resize
    int stats;                 // PAR_STATS_TILE: par_stats_tile_kernel<ragged>; _POINT_COMPACT: par_affinity_kernel<nd, ragged> writing the 5
                               // statistics; _POINT_PLANES: par_affinity_kernel<nd, false> writing 8 * nd planes
    int nd;                    // dilations (the pointwise kernel's instance)
    int step;                  // PAR_STEP_NONE (n_iter == 0: masks are copied); _RECOMPUTE: par_iterate_guide_kernel<ragged>; _STREAM: par_iterate_stream_kernel
    int stats_grid[3], stats_block;
    int step_grid[3], step_block;      // all 0 for PAR_STEP_NONE
    int tiles_interior, tiles_border;  // tile kernels: tiles of ONE H x W image staged in 16-byte pieces / in 4-byte pieces with clamped columns
    int refused;               // ragged only: PAR_REFUSE_* when excel_par_forward_ragged does not take the request (everything else 0), else 0
};
bool par_dil_ok(const int* dil, int ndil);
ParPlan par_plan(const ParShape& s);
int excel_launch_par_affinity(const float* img, float* aff, const TileGeo& geo, const int* dil, int ndil, float w1, float w2, const ParPlan& plan,
                              hipStream_t st);
int excel_launch_par_iterate_guide(const float* guide, const float* stats, const float* in, float* out, const int* nchan, int Cmax,
                                   const TileGeo& geo, const int* dil, int ndil, float w1, float w2, const ParPlan& plan, hipStream_t st);
int excel_launch_par_iterate(const float* aff, const float* in, float* out, const int* nchan, int Cmax, int H, int W, const int* dil, int ndil,
                             float w1, float w2, const ParPlan& plan, hipStream_t st);
int excel_launch_bilinear_ac_ragged(const float* in, float* out, int h, int w, const TileGeo& geo, int total_tiles, hipStream_t st);
int excel_launch_argmax_label_ragged(const float* cams, const int* nchan, const int* cls_idx, int Smax, int Cmax, const TileGeo& geo,
                                     int total_tiles, unsigned char* lab8, hipStream_t st);
int excel_launch_cam_upsample_bkg_ragged(const float* r, const int* ncls, float* rn, float* cams, int g, int Smax, const TileGeo& geo,
                                         int total_tiles, int zero_unused, hipStream_t st);
int excel_launch_normalize_resize_u8_ragged(const unsigned char* hwc, float* out, const TileGeo& geo, int S, const double* mean, const double* stdv,
                                            hipStream_t st);
int excel_launch_normalize_resize_u8_ragged_mirror(const unsigned char* hwc, float* out, const TileGeo& geo, int S, const double* mean,
                                                   const double* stdv, hipStream_t st);
int excel_launch_bilinear_ac(const float* in, float* out, int planes, int h, int w, int H, int W, hipStream_t st);
int excel_launch_argmax_label(const float* cams, const int* nchan, const int* cls_idx, int B, int Smax, int Cmax, long long HW,
                              unsigned char* lab8, long long* lab64, hipStream_t st);
int excel_launch_attr_aggregate(const float* text, const float* bank, int F, int T, int C, int K, int drop, float* out,
                                hipStream_t st);
int excel_launch_bilinear_resize(const float* in, float* out, long long planes, int h, int w, int H, int W, int align_corners,
                                 hipStream_t st);
int excel_launch_flip_max_normalize(const float* attr, float* out, int B, int g, int F, hipStream_t st);
int excel_launch_lam_scale_accumulate(const float* maps, float* acc, int B, int g, int F, int H, int W, int init, hipStream_t st);
int excel_launch_plane_minmax_normalize(float* lam, long long planes, long long HW, hipStream_t st);
int excel_launch_seg_scale_accumulate(const float* segs, float* acc, int B, int nc, int h, int w, int H, int W, int flip_mean, int init,
                                      float scale, hipStream_t st);
int excel_launch_denormalize(const float* img, unsigned char* out8, float* outf, int B, long long HW, const float* mean, const float* stdv,
                             hipStream_t st);
int excel_launch_normalize_u8(const unsigned char* hwc, float* out, int B, long long HW, const double* mean, const double* stdv, hipStream_t st);
int excel_launch_lam_to_label(const float* cam, const float* cls, const int* box, int B, int F, int H, int W, float bkg, float high, float low,
                              int ignore_mid, int ignore, float* valid, unsigned char* lab, hipStream_t st);
// training step (train.hip)
size_t excel_train_losses_ws_bytes(int B, int nc, int H, int W);
int excel_launch_train_losses(const float* seg, const float* attn_pred, const unsigned char* pseudo, const unsigned char* aff_labels, int B, int nc,
                              int g_h, int g_w, int H, int W, int radius, int ignore, float w_seg, float w_diver, float* losses, float* d_seg,
                              float* d_attn_pred, void* ws, hipStream_t st);
// LVC side (lvc.hip)
size_t excel_feature_affinity_ws_bytes(int B, int C, int P);
int excel_launch_feature_affinity(const float* feats, int B, int C, int P, float beta, float gamma, int mode, float* out, void* ws,
                                  hipStream_t st);
size_t excel_feature_affinity_grouped_ws_bytes(int B, int C, int P, int group);
int excel_launch_feature_affinity_grouped(const float* feats, int B, int C, int P, int group, int member_stride, float beta, float gamma,
                                          int mode, float* out, void* ws, hipStream_t st);
size_t excel_attn_select_ws_bytes(int B, int n_layers);
int excel_launch_attn_select_mean(const float* attn, int Lw, int B, int N, int first_layer, int n_layers, const float* seg_attn,
                                  float* out, void* ws, hipStream_t st);

// ---------------------------------------------------------------- the split-type dependent launchers, once per 16-bit type
namespace excel_bf16 {
#include "excel_split_api.inc"
}
namespace excel_f16 {
#include "excel_split_api.inc"
}
#ifdef EXCEL_SPLIT_F16
#define EXCEL_SPLIT_NS excel_f16
#else
#define EXCEL_SPLIT_NS excel_bf16
#endif
// Host code outside those six translation units reaches the launchers through this table alone: no using-directive makes an unqualified
// excel_launch_* name visible, so a call that is not routed through split_api() does not compile.  The list is written once; the
// member types and both instances are generated from it, so a slot cannot hold the other type's function.
#define EXCEL_SPLIT_API(X, ns)                                                                                            \
    X(ns, gemm_bf16x3, excel_launch_gemm_bf16x3) X(ns, split_bf16, excel_launch_split_bf16) X(ns, pack_hi, excel_launch_pack_hi) \
    X(ns, vt_from_planes, excel_launch_vt_from_planes) X(ns, layernorm, excel_launch_layernorm)                           \
    X(ns, assemble_ln_pre, excel_launch_assemble_ln_pre) X(ns, token_axis_normalize, excel_launch_token_axis_normalize)   \
    X(ns, im2col, excel_launch_im2col) X(ns, attn_rowpass, excel_launch_attn_rowpass) X(ns, attn_accum, excel_launch_attn_accum) \
    X(ns, attn_strip, excel_launch_attn_strip) X(ns, cam_epilogue, excel_launch_cam_epilogue)                             \
    X(ns, patch_text_cam, excel_launch_patch_text_cam) X(ns, patch_text_cam_ws_floats, excel_patch_text_cam_ws_floats)
#define EXCEL_SPLIT_MEMBER(ns, member, fn) decltype(&ns::fn) member;
#define EXCEL_SPLIT_ENTRY(ns, member, fn) &ns::fn,
struct SplitApi { EXCEL_SPLIT_API(EXCEL_SPLIT_MEMBER, excel_bf16) };      // (function pointers carry no default arguments: callers state every one)
inline constexpr SplitApi g_split_api[2] = {{EXCEL_SPLIT_API(EXCEL_SPLIT_ENTRY, excel_bf16)}, {EXCEL_SPLIT_API(EXCEL_SPLIT_ENTRY, excel_f16)}};
// gemm_mode 0 (exact fp32: only the fp32-output paths of the bf16 objects run) and 1 (bf16x3): bf16; 2 (f16x3) and 3 (f16x2): IEEE half
inline const SplitApi& split_api(int gemm_mode) { return g_split_api[gemm_mode >= 2 ? 1 : 0]; }
// LayerNorm of fp32 rows into fp32 rows (decoder, training step, excel_layernorm).  norm.hip is built per split type, but this path
// writes no split planes and is the same code in both objects: the bf16 object's is the one that runs.
inline int excel_launch_layernorm_f32(const float* x, const float* w, const float* b, float* y, int rows, int D, float eps, hipStream_t st) {
    return excel_bf16::excel_launch_layernorm(x, nullptr, 1, w, b, y, rows, D, eps, st, 0, 0);
}
// one unbatched split-plane GEMM over dense operand rows (lda = ldb = 2K); callers set batch strides, the head-major fields and the
// two-product fields on the result
inline GemmBfArgs gemm_bf_args(const void* A, const unsigned short* W, float* C, void* Cs, const float* bias, const float* res,
                               int M, int N, int K, int ldc, int ldr, int act, int out_mode) {
    GemmBfArgs g{};
    g.A = (const unsigned short*)A; g.B = W; g.C = C; g.Cs = (unsigned short*)Cs; g.bias = bias; g.res = res;
    g.M = M; g.N = N; g.K = K; g.lda = 2 * K; g.ldb = 2 * K; g.ldc = ldc; g.ldr = ldr; g.act = act; g.out_mode = out_mode;
    return g;
}

// ---------------------------------------------------------------- the bilinear sampler: every F.interpolate(mode='bilinear') site
// One axis of ATen's area_pixel_compute_source_index: output index d of n_out -> the two source indices in [0, n_in) and the weight
// of the second.  Contraction is off, so the operations below are the ones that run, in every kernel this is inlined into:
//   align_corners=False: f = max(fma(n_in / n_out, d + 0.5, -0.5), 0) - the product and the -0.5 in ONE rounding (what hipcc -O3
//     made of `scale * (d + 0.5f) - 0.5f` at every site before they shared this body; __fmul_rn / __fsub_rn do not prevent it, they
//     are inlined as plain operations);
//   align_corners=True: f = scale * d, ROUNDED before the weight is taken from it (ATen: lambda = src - floor(src)).  Fused into
//     one fma, `f - i0` keeps what the rounding of f drops (4e-6 near 47) and PAR's outputs move by 2e-5
//     (tests/test_gpu_par_shapes.py, ragged batch).
struct LinearTap { int i0, i1; float l; };
__device__ __forceinline__ LinearTap linear_tap(int d, int n_in, int n_out, int align_corners) {
#pragma clang fp contract(off)
    const float f = align_corners ? ((n_out > 1) ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f) * (float)d
                                  : fmaxf(fmaf((float)n_in / (float)n_out, (float)d + 0.5f, -0.5f), 0.f);
    LinearTap t;
    t.i0 = min((int)f, n_in - 1);
    t.i1 = min(t.i0 + 1, n_in - 1);
    t.l = f - (float)t.i0;
    return t;
}
struct BilinearTap { int y0, y1, x0, x1; float ly, lx; };
__device__ __forceinline__ BilinearTap bilinear_tap(int x, int y, int h, int w, int H, int W, int align_corners) {
    const LinearTap ty = linear_tap(y, h, H, align_corners), tx = linear_tap(x, w, W, align_corners);
    return BilinearTap{ty.i0, ty.i1, tx.i0, tx.i1, ty.l, tx.l};
}
// the two-stage blend: each (1 - l) product rounded, then one fma per stage
__device__ __forceinline__ float bilinear_blend(float ly, float lx, float p00, float p01, float p10, float p11) {
    const float top = fmaf(lx, p01, __fmul_rn(1.f - lx, p00));
    const float bot = fmaf(lx, p11, __fmul_rn(1.f - lx, p10));
    return fmaf(ly, bot, __fmul_rn(1.f - ly, top));
}
__device__ __forceinline__ float bilinear_blend(const BilinearTap& t, float p00, float p01, float p10, float p11) {
    return bilinear_blend(t.ly, t.lx, p00, p01, p10, p11);
}

// The 12 weights of a transformer block (excel_vit_block_weights and excel_decoder_block_weights name them alike) for the *_create entries:
// every one is read 16 bytes at a time somewhere - the matrices as GEMM operands and by the split / pack kernels, the LayerNorm weights by
// ln_row, the biases by the split-plane GEMM's epilogue (the fp32 GEMM reads them by element: one rule per handle all the same).
template <class BlockWeights>
static inline int check_block_weights_aligned(const char* who, const BlockWeights* blocks, int n) {
    static const char* const name[12] = {"ln1_w", "ln1_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"};
    for (int l = 0; l < n; ++l) {
        const BlockWeights& b = blocks[l];
        const void* p[12] = {b.ln1_w, b.ln1_b, b.in_proj_w, b.in_proj_b, b.out_proj_w, b.out_proj_b, b.ln2_w, b.ln2_b, b.fc1_w, b.fc1_b, b.fc2_w, b.fc2_b};
        for (int i = 0; i < 12; ++i) EXCEL_CHECK_ARG(((uintptr_t)p[i] & 15) == 0, "%s: blocks[%d].%s must be 16-byte aligned", who, l, name[i]);
    }
    return EXCEL_OK;
}
