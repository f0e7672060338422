/* libexcel_hip -- C ABI of the MI355X-native ExCEL training-free CAM + affinity + PAR hot path.
 *
 * The reference (zwyang6/ExCEL) is pure Python on PyTorch: it has no FFI/plugin boundary, its drop-in
 * boundary is the Python call surface (model_excel / clip / affutils / PAR / evaluate).  excel_amd/ keeps
 * that surface and binds THIS library underneath it with ctypes.  Every entry point
 * below cites the reference interface it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless marked (host); tensors are dense row-major fp32 unless noted
 *   - every call takes an explicit hipStream_t (passed as void*), launches asynchronously, never syncs,
 *     never allocates (callers own all buffers; *_workspace_bytes tell how much scratch to bring),
 *     except excel_vit_create / excel_vit_destroy
 *   - return 0 on success, <0 on error (-1 bad argument, -2 launch failure, -3 allocation failure);
 *     excel_last_error() returns a thread-local message
 *   - alignment: a device pointer needs the alignment of its element type (4 bytes for fp32 / int32, 8 for int64 / double, 1 for
 *     uint8) unless the entry's comment asks for more.  Where it does ("16-byte aligned", "8-byte aligned"), a pointer below that is
 *     refused with EXCEL_ERR_ARG, the message names the argument, and nothing has been launched.  excel_amd/ops.py copies a misaligned
 *     INPUT into fresh storage first and refuses a misaligned OUTPUT (tests/_align_cases.py has one row per op)
 *   - B images, S x S input, g = S/patch, P = g*g patches, N = P+1 tokens, D = width, H = heads (D/H must be 64),
 *     C = out_dim, T text rows, F foreground classes, L layers
 */
#ifndef EXCEL_HIP_H
#define EXCEL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* excel_last_error(void);
int excel_abi_version(void);
/* (host) id of the sources this library was compiled from: first 16 hex digits of the sha256 over csrc/*.hip, csrc/*.h and this header
 * (excel_amd/build.py:source_id; "-dev" appended for an EXCEL_DEV build, "unstamped" when compiled outside build.py).  The harness
 * compares it with the sources next to it so that a stale library is never measured. */
const char* excel_build_id(void);

/* ------------------------------------------------------------------ building blocks (exported for tests / reuse) */

/* C = act(A . op(B) + bias) + residual on the f32-input matrix core (exact-fp32 numerics).
 * b_kmajor=1: B is [N,K] (torch nn.Linear weight layout); 0: B is [K,N].  act: 0 none, 1 QuickGELU
 * (clip/clip_surgery_model.py:280-282).  Batched: `batch` problems with element strides sA/sB/sC.
 * Replaces the cuBLAS GEMMs behind nn.Linear / torch.matmul on the path.
 * A and Bm 16-byte aligned with lda, ldb and the batch strides multiples of 4 (both operands are loaded 16 bytes at a time); C, bias and
 * residual are touched by element: 4 bytes. */
int excel_gemm_f32(const float* A, const float* Bm, float* C, const float* bias, const float* residual,
                   int M, int N, int K, int lda, int ldb, int ldc, int ldr, int b_kmajor, int act,
                   int batch, long long sA, long long sB, long long sC, long long sR, void* stream);

/* "bf16x3" building blocks: excel_split_bf16 turns fp32 [rows,K] into the split operand format [rows][2][K] bf16
 * (hi plane, lo plane; same number of bytes); excel_gemm_bf16x3 computes C = act(A.W^T + bias) + residual from two split
 * operands with three bf16 MFMAs per product (fp32 accumulate).  C is fp32 [M,N], or a split tensor when split_out.
 * excel_split_*: `in` 16-byte aligned, `out` 8-byte aligned.  excel_gemm_*: A_split and W_split 16-byte aligned (16-byte DMA into LDS),
 * and so are C, bias and residual (the epilogue moves 16 bytes at a time). */
int excel_split_bf16(const float* in, void* out, long long rows, int K, void* stream);
int excel_gemm_bf16x3(const void* A_split, const void* W_split, float* C, const float* bias, const float* residual,
                      int M, int N, int K, int act, int split_out, void* stream);
/* The same two building blocks with IEEE-half planes ("f16x3": hi = half(x), lo = half(x - hi); 11 + 11 mantissa bits where lo stays
 * a normal half, range 65 504; v_mfma_f32_16x16x32_f16 in the GEMM, same layouts and rate). */
int excel_split_f16(const float* in, void* out, long long rows, int K, void* stream);
int excel_gemm_f16x3(const void* A_split, const void* W_split, float* C, const float* bias, const float* residual,
                     int M, int N, int K, int act, int split_out, void* stream);
/* "f16x2": the f16x3 GEMM for fp16-VALUED weights - two matrix-core instructions per product.  The published CLIP archives store
 * half-precision parameters and the reference loads them into its fp32 model unchanged (clip/build_model.py:72, clip/clip.py:138-154),
 * so the lo plane of every nn.Linear weight is exactly zero and the a.hi x w.lo pass of the three-product scheme multiplies zeros; it
 * is not issued.  The results are bit-identical to excel_gemm_f16x3 on the same operands.
 *   excel_pack_f16: fp32 [rows,K] -> the hi plane as a plain half matrix [rows,K]; adds to *inexact_dev (device, zero it first) the
 *                   number of elements that are NOT representable in IEEE half - the mode's precondition is that count == 0.
 *   excel_gemm_f16x2: W_split as excel_split_f16 wrote it (its lo plane must be all zero: not checked here); W_half (optional, may be
 *                   NULL) = the excel_pack_f16 matrix of the same weights: the large-tile kernel then streams half the weight bytes.
 * excel_pack_f16: `in` 16-byte aligned, `out` and inexact_dev 8-byte aligned.  excel_gemm_f16x2: as excel_gemm_f16x3; a W_half that is
 * not 16-byte aligned is not refused but left unused (the split weights serve: the same bits). */
int excel_pack_f16(const float* in, void* out, long long rows, int K, unsigned long long* inexact_dev, void* stream);
int excel_gemm_f16x2(const void* A_split, const void* W_split, const void* W_half, float* C, const float* bias, const float* residual,
                     int M, int N, int K, int act, int split_out, void* stream);
/* Which kernel instance the split-plane GEMM runs a problem on (a HOST function: no device work).  The problem is described as
 * excel_gemm_bf16x3 / _f16x3 / _f16x2 and the ViT's linear layers pass it: operands [M,K] and [N,K], `batch` problems (the ViT's A_sum.V
 * form), out_mode 0 = fp32 [M,N], 1 = q|k|v head-major with head dim 64 (the ViT's in_proj), 2 = split output; has_residual; gemm_mode
 * as in excel_vit_set_gemm_mode (1 bf16x3, 2 f16x3, 3 f16x2); has_half: the f16x2 call passes W_half; n_cu: the device's compute units.
 * plan[EXCEL_GEMM_PLAN_INTS] = {kernel, tile, nt_m, x2, tall, shrt, second, grid_x, grid_y, block}:
 *   kernel: 0 uniform 8-wave tiles (tile: 0 128x128, 1 256x128, 2 256x256, 3 320x256), 1 mixed-height 8-wave tiles (`tall` row tiles of
 *           320 rows, then `shrt` of 256), 2 one four-wave instance (nt_m: 10 / 8 / 5 = 320- / 256- / 160-row tiles), 3 a launch of two
 *           four-wave instances (`tall` row tiles of 320 rows, then `shrt` of the instance `second` = 8 / 5);
 *   x2: two-product kernel (0 no, 1 on the split weights, 2 on the half weights); grid_x, grid_y, block: the launch.  Unused fields are 0. */
#define EXCEL_GEMM_PLAN_INTS 10
int excel_gemm_plan(int M, int N, int K, int batch, int out_mode, int has_residual, int gemm_mode, int has_half, int n_cu,
                    int32_t* plan /*host*/);
/* Which kernels one ViT layer's attention runs on for B images of N tokens and H heads of dim 64 (a HOST function: no device work).
 * gemm_mode as in excel_vit_set_gemm_mode (0 f32, 1 bf16x3, 2 f16x3, 3 f16x2); surgery: the layer is one of the last n_surgery (q.q /
 * k.k / v.v attention); want_w: the head-mean q.k weights are wanted (w_aff and / or attn_out cover this layer).
 * plan[EXCEL_ATTN_PLAN_INTS] = {path, ntiles, ntw, waves, waves_full, rowpass_ntypes, rowpass_grid x, y, z, grid x, y, z, block, split_c}:
 *   path: 0 flash row pass + strip-resident kernel (split modes, ntiles = cdiv(N, 32) <= 40: instance ntw = cdiv(ntiles, 8) key tiles per
 *         wave on waves = cdiv(ntiles, ntw) waves, of which waves_full own ntw tiles and the others ntw - 1), 1 row pass + split-plane
 *         accumulate kernel (split modes beyond that), 2 row pass + fp32 accumulate kernel (f32);
 *   rowpass_ntypes: 4 on a surgery layer of a two-pass path (q.k, q.q, k.k, v.v statistics), else 1; rowpass_grid: 256 threads each;
 *   grid, block: the second kernel's launch (all 0 when the layer needs none: no surgery, no weights wanted); split_c: strips per XCD
 *   chunk when the strip kernel's two sweeps run as separate workgroups (surgery and want_w), else 0.  Unused fields are 0. */
#define EXCEL_ATTN_PLAN_INTS 14
int excel_attn_plan(int B, int H, int N, int gemm_mode, int surgery, int want_w, int32_t* plan /*host*/);
/* Which kernels excel_patch_text_cam runs B images of N tokens x C columns against T text rows on (a HOST function: no device work; the
 * launcher itself launches what this names).  gemm_mode as in excel_vit_set_gemm_mode (0 f32, 1 bf16x3, 2 f16x3, 3 f16x2: the CAM runs
 * f16x2 as f16x3).  1 <= T <= 512, C a multiple of 32 up to 1024.
 * plan[EXCEL_CAM_PLAN_INTS] = {kernel, split, ct, tlds, groups, prep_grid x, y, z, sim_grid x, y, block, finish_grid x, y, finish_pitch}:
 *   kernel: 0 the narrow similarity kernel (T <= 128: all classes in the accumulators at once), 1 the wide one (class chunks of 128);
 *   split: 1 in the split-plane modes (three 16-bit MFMAs per product), 0 exact fp32;  ct: the narrow instance's class tiles of 32
 *   (1 / 2 / 4; 0 for the wide kernel);  tlds: the narrow split instance stages the text bank in LDS (T <= 48, C <= 512, C % 256 == 0:
 *   ct = 1 / 2; otherwise the split instances are ct = 2 / 4 and the f32 ones 1 / 2 / 4);  groups = cdiv(cdiv(N, 32), 4) workgroups per
 *   image;  prep_grid (cdiv(N, 64), B, cdiv(C, 256) + 1) and finish_grid (cdiv(N, 64), B) of 256 threads, sim_grid (groups, B) of `block`;
 *   finish_pitch: row pitch of the per-workgroup min / max table (128 narrow, 512 wide). */
#define EXCEL_CAM_PLAN_INTS 14
int excel_patch_text_cam_plan(int B, int N, int C, int T, int gemm_mode, int32_t* plan /*host*/);

/* LayerNorm over the last dim, fp32, eps as given (clip/clip_surgery_model.py:271-277).  D % 4 == 0; x, w, b and y 16-byte aligned
 * (a row is read and written 16 bytes at a time). */
int excel_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int D, float eps, void* stream);

/* ------------------------------------------------------------------ ViT "surgery" forward */

typedef struct {
    int width, layers, heads, patch, out_dim;
    int n_surgery;   /* blocks [layers-n_surgery, layers) use q-q/k-k/v-v attention; reload_self_attn(layers=6) -> 5
                        (clip/clip_surgery_model.py:396-405) */
    int pos_grid;    /* side of the stored positional grid (positional_embedding has 1 + pos_grid^2 rows) */
} excel_vit_config;

typedef struct {
    const float *ln1_w, *ln1_b;
    const float *in_proj_w, *in_proj_b;    /* [3D,D], [3D]  rows q|k|v (nn.MultiheadAttention.in_proj_* == Attention.qkv.*) */
    const float *out_proj_w, *out_proj_b;  /* [D,D], [D] */
    const float *ln2_w, *ln2_b;
    const float *fc1_w, *fc1_b;            /* mlp.c_fc   [4D,D], [4D] */
    const float *fc2_w, *fc2_b;            /* mlp.c_proj [D,4D], [D] */
} excel_vit_block_weights;

typedef struct {
    const float* conv1_w;    /* [D,3,patch,patch] */
    const float* class_emb;  /* [D] */
    const float* pos_emb;    /* [1+pos_grid^2, D] */
    const float *ln_pre_w, *ln_pre_b, *ln_post_w, *ln_post_b;
    const float* proj;       /* [D, out_dim] */
    const excel_vit_block_weights* blocks;   /* (host) array of `layers` entries of device pointers */
} excel_vit_weights;

typedef struct excel_vit* excel_vit_t;

/* Binds device weight pointers (NOT copied, must outlive the handle) and prepares derived weights
 * (proj^T; bilinearly resized positional grids are cached per g on first use, clip_surgery_model.py:426-435).
 * Replaces ExCEL_CLIP.visual construction + reload_self_attn (clip/clip_surgery_model.py:396-416).
 * Every weight pointer 16-byte aligned (the message names the first one that is not). */
int excel_vit_create(const excel_vit_config* cfg, const excel_vit_weights* w, excel_vit_t* out);
void excel_vit_destroy(excel_vit_t h);

/* GEMM numerics of the linear layers (and attention products) of this handle:
 *   0 = exact fp32 (v_mfma_f32_32x32x2_f32, 157 TFLOP/s peak);
 *   1 = "bf16x3": operands as bf16 hi+lo planes, 3 bf16 MFMAs per product, 16 mantissa bits per operand at the fp32 exponent range -
 *       the fastest mode; its CAM error is ~12x that of fp32 arithmetic (1e-5 on well-conditioned weights);
 *   2 = "f16x3": the same scheme on IEEE-half planes (22 mantissa bits where lo stays normal): fp32-grade results (within 1.4x of fp32
 *       arithmetic's own error on every network measured), ~2.5 % slower than mode 1 (the part is power-limited), values beyond 65 504
 *       (the largest finite IEEE half) overflow LOUDLY (hi = inf, lo = -inf: every product they enter is a NaN, never a finite wrong
 *       number).  Nothing inside the forward pass looks for that NaN: the overflow guard below (excel_nonfinite_count over the
 *       tensors a step hands on, excel_confusion_accumulate_masked) is what catches it per image, and the caller re-runs the
 *       flagged images in mode 0;
 *   3 = "f16x2": mode 2 with the nn.Linear GEMMs on two MFMAs per product (excel_gemm_f16x2 above) - available when every weight
 *       matrix of the handle is fp16-valued (excel_vit_weights_fp16_exact; true for every published CLIP archive), refused with
 *       EXCEL_ERR_ARG otherwise.  Bit-identical to mode 2 on such weights, and the fastest mode: a third of the GEMMs' matrix-core
 *       work is gone.  The attention products (activation x activation) stay three-product.  Same 65 504 range and the same loud
 *       overflow as mode 2; the same guard catches it.
 * Default 0, or the mode named by the environment variable EXCEL_GEMM_MODE (bf16x3 | f16x3 | f16x2) at create time.  Switching between
 * 1 and 2/3 re-splits the weights (synchronises the device). */
int excel_vit_set_gemm_mode(excel_vit_t h, int mode);
int excel_vit_get_gemm_mode(excel_vit_t h);
/* 1 when every GEMM weight of the handle (in_proj, out_proj, fc1, fc2 of every block, conv1, proj) is exactly representable in IEEE
 * half, 0 when not, < 0 on error.  The first call packs the weights (one pass over them, synchronises); the answer is cached. */
int excel_vit_weights_fp16_exact(excel_vit_t h);

size_t excel_vit_workspace_bytes(excel_vit_t h, int B, int S);

/* VisionTransformer.forward + generate_clip_fts (clip/clip_surgery_model.py:419-448, clip/clip.py:348-358).
 *   img            [B,3,S,S]
 *   image_features [B,N,C]  token-axis L2-normalised (clip.py:353)                         (optional when x_raw is given)
 *   x_raw          [B,N,C]  ln_post(x) @ proj before the normalisation                      (optional, may be NULL)
 *   w_aff          [B,P,P]  mean over the last `aff_layers` layers of attn[:,1:,1:] -- exactly what
 *                           refine_cams_with_aff consumes (utils/affutils.py:180,197); block weights are head-MEAN
 *                           for nn.MultiheadAttention blocks, head-SUM for surgery blocks    (optional)
 *   attn_out       [n_attn_out,B,N,N] per-layer weights of the LAST n_attn_out layers (0..L) (optional)
 *   feats_out      [L,B,N,D] per-block original-path features ("all_feats", clean copies)   (optional)
 * img, workspace, image_features and x_raw 16-byte aligned; w_aff, attn_out and feats_out 4 bytes.
 */
int excel_vit_forward(excel_vit_t h, const float* img, int B, int S, void* workspace, size_t workspace_bytes,
                      float* image_features, float* x_raw, float* w_aff, int aff_layers,
                      float* attn_out, int n_attn_out, float* feats_out, void* stream);

/* Same, with the LVC cue of Attention.forward's `ex_feats` branch (clip/clip_surgery_model.py:127-141):
 *   ex_attn [B,P,P] (= excel_feature_affinity(ex_feats, mode 1)) is added to attn[:, :, 1:, 1:] of EVERY head of every
 *   surgery block before the head sum; NULL = the ex_feats=None branch (identical to excel_vit_forward).
 *   flags: EXCEL_VIT_FEATS_AS_REFERENCE = feats_out holds what the reference's decoder receives: the reference stacks
 *          its per-block list after the forward, and in-place updates (clip_surgery_model.py:317,319,329,442) have by then
 *          rewritten the entries of the last single-path block (= final new-path x incl. the cls swap) and of every
 *          surgery block but the last (= x_ori + the next block's attention residual).  Default: clean block outputs.
 * Alignment as for excel_vit_forward (img, workspace, image_features, x_raw 16-byte aligned); ex_attn 4 bytes. */
#define EXCEL_VIT_FEATS_AS_REFERENCE 1
int excel_vit_forward_ex(excel_vit_t h, const float* img, int B, int S, void* workspace, size_t workspace_bytes,
                         float* image_features, float* x_raw, float* w_aff, int aff_layers,
                         float* attn_out, int n_attn_out, float* feats_out, const float* ex_attn, int flags, void* stream);

/* Token affinity of decoder features, shared by attn_pred (model/model_excel.py:70-76) and the ex_feats branch
 * (clip/clip_surgery_model.py:128-137):  feats [B,C,P] -> F.normalize over C -> sim = f^T f [B,P,P]
 *   -> z = (sim - mean(sim over the WHOLE batch tensor) * beta) * gamma
 *   mode 0: out = sigmoid(z)                                  (attn_pred: beta 1, gamma 3)
 *   mode 1: z < 0 -> -inf, out = softmax(z, dim=-1)           (ex_attn:   beta 1, gamma 3)
 * workspace 16-byte aligned (it holds both operands of the similarity GEMM); feats and out 4 bytes.              */
size_t excel_feature_affinity_workspace_bytes(int B, int C, int P);
int excel_feature_affinity(const float* feats, int B, int C, int P, float beta, float gamma, int mode, float* out,
                           void* workspace, void* stream);

/* excel_feature_affinity with each mean taken over one GROUP of images instead of the whole batch.  The reference computes
 * attn_pred on one image (tools/infer_lam.py:79, batch 1) and ex_attn on the pair (x, flip x) (utils/camutils.py:15-18): a batched
 * step of many images needs those means per image / per pair.
 *   feats [B,C,P]; `group` images per group, B / group groups.  Member m (0 <= m < group) of group j is image
 *       first(j) + m * member_stride,   first(j) = (j / member_stride) * group * member_stride + j % member_stride
 *   requires B % (group * member_stride) == 0.  The two layouts the optimised-LAM step uses:
 *       group 1, member_stride 1                  one image per group (attn_pred);
 *       group 2, member_stride B/2 over a [2B'] stack   the pair (image j, image B' + j) (ex_attn over [x; flip x], B' = B/2).
 *   BIT CONTRACT: every group's rows are bit-identical to excel_feature_affinity called on that group's images alone, stacked in
 *   member order.  The per-group mean reproduces that call's fixed-order double sum: n = group*P*P, nparts = min(1024,
 *   ceil(n / 4096)) chunks of ceil(n / nparts) values in member order, each summed by 256 strided lanes and a tree, the chunk sums
 *   added in order (mode 1 masks z < 0, so one last bit of the mean can change the mask).
 * One launch sequence per call (normalise, one batched similarity GEMM, partial sums over a (chunk, group) grid, per-group mean,
 * finish); workspace: excel_feature_affinity_grouped_workspace_bytes(B, C, P, group), 16-byte aligned; feats and out 4 bytes.    */
size_t excel_feature_affinity_grouped_workspace_bytes(int B, int C, int P, int group);
int excel_feature_affinity_grouped(const float* feats, int B, int C, int P, int group, int member_stride, float beta, float gamma,
                                   int mode, float* out, void* workspace, void* stream);

/* ------------------------------------------------------------------ decoder head
 * SegFormerHead fuse (model/segformer_head.py:47-77: per ViT layer Linear(D,E) -> ReLU -> Linear(E,E) on the patch
 * tokens, channel concat, 1x1 conv L*E -> E) and DecoderTransformer (model/decoder/TransDecoder.py:105-124: dec_layers
 * pre-LN blocks of MHA(heads) + QuickGELU MLP(4E), then the 1x1 linear_pred E -> num_classes), exact fp32.
 * Weight pointers are device pointers in the reference modules' state_dict layout (Linear: [out,in]; 1x1 conv:
 * [out,in,1,1] == [out,in]) and must stay valid for the life of the handle.  Every weight pointer 16-byte aligned
 * (the GEMMs and LayerNorm read them 16 bytes at a time); all_feats and the workspace of excel_decoder_forward 16-byte aligned. */
typedef struct excel_decoder* excel_decoder_t;
typedef struct { int vit_layers, vit_width, embed, dec_layers, heads, num_classes; } excel_decoder_config;
typedef struct { const float *proj_w, *proj_b, *proj2_w, *proj2_b; } excel_fuse_layer_weights;
typedef struct {
    const float *ln1_w, *ln1_b, *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} excel_decoder_block_weights;
typedef struct {
    const excel_fuse_layer_weights* fuse;          /* [vit_layers] */
    const float *fuse_w, *fuse_b;                  /* linear_fuse [E, L*E], [E] */
    const excel_decoder_block_weights* blocks;     /* [dec_layers] */
    const float *pred_w, *pred_b;                  /* linear_pred [num_classes, E], [num_classes] */
} excel_decoder_weights;
int excel_decoder_create(const excel_decoder_config* cfg, const excel_decoder_weights* w, excel_decoder_t* out);
void excel_decoder_destroy(excel_decoder_t h);
size_t excel_decoder_workspace_bytes(excel_decoder_t h, int B, int g);
/* all_feats [L,B,N,D] (excel_vit_forward's feats_out; N = g*g+1, the cls row is skipped as model/model_excel.py:60 does)
 *   -> attn_fts_out [B,E,g,g] (optional; model_excel.py:64-65) and seg_out [B,num_classes,g,g] (optional; :68).           */
int excel_decoder_forward(excel_decoder_t h, const float* all_feats, int B, int g, void* workspace, size_t workspace_bytes,
                          float* attn_fts_out, float* seg_out, void* stream);

/* ------------------------------------------------------------------ CLIP text tower (one-time text bank)
 * encode_text (clip/clip_surgery_model.py:551-564): tokens [B,context_length] int32 -> token + positional embedding ->
 * `layers` causal pre-LN blocks (nn.MultiheadAttention + QuickGELU MLP) -> ln_final -> row of the EOT token (first arg-max of
 * the ids) @ text_projection [width, embed_dim] -> out [B, embed_dim].  Exact fp32.  Weights: device pointers, state_dict layout,
 * every one 16-byte aligned; the workspace of excel_text_encode 16-byte aligned, tokens and out 4 bytes. */
typedef struct excel_text* excel_text_t;
typedef struct { int vocab_size, context_length, width, layers, heads, embed_dim; } excel_text_config;
typedef struct {
    const float *token_embedding, *positional_embedding, *ln_final_w, *ln_final_b, *text_projection;
    const excel_decoder_block_weights* blocks;     /* [layers] */
} excel_text_weights;
int excel_text_create(const excel_text_config* cfg, const excel_text_weights* w, excel_text_t* out);
void excel_text_destroy(excel_text_t h);
size_t excel_text_workspace_bytes(excel_text_t h, int B);
int excel_text_encode(excel_text_t h, const int32_t* tokens, int B, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* encode_text_with_prompt_ensemble's reduction (clip/clip.py:262-266): emb [n,E] -> rows normalised, mean, normalised -> out [E]. */
int excel_prompt_ensemble(const float* emb, int n, int E, float* out, void* stream);

/* ------------------------------------------------------------------ training iteration of the decoder
 * Losses of scripts/train_voc.py:202-215 and their gradients:
 *   seg [B,nc,g_h,g_w] -> bilinear (align_corners=False) to (H,W) -> get_seg_loss (model/losses.py:4-18) against pseudo [B,H,W] u8
 *   attn_pred [B,P,P] -> get_aff_loss (model/losses.py:20-31) against cams_to_affinity_label(pseudo, get_mask_by_radius(g,g,radius))
 *                        (utils/camutils.py:438-476; nearest down-sampling by H/g_h, 255 outside the window / on ignored tokens)
 *   losses[0] = seg_loss, losses[1] = aff ("diver") loss (device floats); d_seg, d_attn_pred = gradients of
 *   w_seg*seg_loss + w_diver*aff_loss.  aff_labels (NULL = pseudo): the map the affinity labels are built from -- the reference
 *   switches it to the arg-max of the up-sampled seg logits after 24 000 iterations (train_voc.py:210).  Fixed-order reductions.
 *   workspace 8-byte aligned (double partial sums). */
size_t excel_train_losses_workspace_bytes(int B, int nc, int H, int W);
int excel_train_losses(const float* seg, const float* attn_pred, const unsigned char* pseudo, const unsigned char* aff_labels, int B, int nc,
                       int g_h, int g_w, int H, int W, int radius, int ignore_index, float w_seg, float w_diver, float* losses,
                       float* d_seg, float* d_attn_pred, void* workspace, void* stream);

/* The decoder head in training mode (SegFormerHead + DecoderTransformer + attn_pred, model/model_excel.py:60-76), exact fp32:
 *   forward_train keeps the activations in `workspace` and returns seg [B,nc,g,g] and attn_pred [B,P,P];
 *   backward (same all_feats / workspace) writes d loss / d parameter for every parameter into `grads`, a table with the layout
 *   of the weights whose pointers are WRITTEN (device memory of each parameter's shape); d_attn_pred may be NULL.
 *   dropout_p / dropout_seed: the head's Dropout2d (segformer_head.py:66,75; the reference trains with p = 0.1) as a counter-based
 *   channel mask, a pure function of (seed, image, channel): pass the same pair to forward_train and backward.  g*g % 4 == 0.
 * excel_adamw_step: torch.optim.AdamW update of one tensor (decoupled weight decay, bias correction with `step` >= 1), the
 * arithmetic under utils/optimizer.py's PolyWarmupAdamW; the learning-rate schedule stays on the host.
 * The workspace of all three entries and forward_train's all_feats 16-byte aligned; everything else, the gradient table included, 4 bytes. */
size_t excel_decoder_train_workspace_bytes(excel_decoder_t h, int B, int g);
int excel_decoder_forward_train(excel_decoder_t h, const float* all_feats, int B, int g, void* workspace, size_t workspace_bytes,
                                float* seg_out, float* attn_pred_out, float dropout_p, unsigned dropout_seed, void* stream);
/* attn_fts [B,E,g,g] of the last excel_decoder_forward_train on `workspace`: the fused features AFTER the head's Dropout2d, what the
 * reference's training loop clones as the LVC cue (scripts/train_voc.py:186-189: fts_diver = attn_fts.clone().detach()). */
int excel_decoder_train_attn_fts(excel_decoder_t h, int B, int g, const void* workspace, size_t workspace_bytes, float* attn_fts_out,
                                 void* stream);
int excel_decoder_backward(excel_decoder_t h, const float* all_feats, int B, int g, void* workspace, size_t workspace_bytes,
                           const float* d_seg, const float* d_attn_pred, const excel_decoder_weights* grads, float dropout_p,
                           unsigned dropout_seed, void* stream);
int excel_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, void* stream);

/* lam_to_label (utils/camutils.py:123-145): cam [B,F,H,W], cls_label [B,F] -> valid_cam = cls*cam (optional) and label u8 [B,H,W] =
 * argmax+1, thresholded (ignore_mid: value <= high -> ignore_index, value <= low -> 0; else value <= bkg -> 0); img_box [B,4] int32
 * (y0,y1,x0,x1; optional): pixels outside the box -> ignore_index. */
int excel_lam_to_label(const float* cam, const float* cls_label, const int32_t* img_box, int B, int F, int H, int W, float bkg_thre,
                       float high_thre, float low_thre, int ignore_mid, int ignore_index, float* valid_cam, unsigned char* label,
                       void* stream);

/* transforms.normalize_img + the HWC->CHW transpose of the dataset (datasets/transforms.py; datasets/voc.py:115-116):
 * hwc [B,H,W,3] uint8 (decoded image) -> out [B,3,H,W] f32 = (u8 - mean[c]) / std[c], double intermediate like numpy.  mean3/std3: HOST doubles. */
int excel_normalize_img_u8(const unsigned char* hwc, int B, int H, int W, const double* mean3, const double* std3, float* out, void* stream);

/* denormalize_img / denormalize_img2 (utils/imutils.py:11-25): img [B,3,H,W] f32 (normalised) -> v = img*std[c] + mean[c]
 * truncated to uint8 (out_u8, optional) and/or that value / 255 as float (out_f32, optional).  mean3/std3: HOST pointers to 3 floats. */
int excel_denormalize_img(const float* img, int B, int H, int W, const float* mean3, const float* std3, unsigned char* out_u8,
                          float* out_f32, void* stream);

/* Multi-scale / flip fuse of the segmentation logits (tools/infer_seg_voc.py:66-82): segs [2B,nc,h,w] of one scale (second
 * half from the x-flipped inputs) -> bilinear (align_corners=False) to (H,W) -> flip_mean ? (seg + flip_x(seg_flipped))/2 : seg
 * (scale 1.0 uses the un-flipped half alone, :69) -> acc [B,nc,H,W] = ((init ? 0 : acc) + .) * scale (mean over scales: pass
 * 1/n_scales with the last scale, 1 otherwise). */
int excel_seg_scale_accumulate(const float* segs, float* acc, int B, int nc, int h, int w, int H, int W, int flip_mean, int init,
                               float scale, void* stream);

/* ------------------------------------------------------------------ patch-text CAM */

/* clip_feature_surgery (clip/clip.py:288-310, redundant_feats=None) on normalised features:
 *   image_features [B,N,C], text [T,C] (unit rows) -> out_full [B,N,T] and/or the caller's slice
 *   out_slice [B,N-1,F] = out_full[:, 1:, :F] (model/model_excel.py:58).  workspace: B*N*ldT floats, ldT = T rounded up to 4.
 * 1 <= F <= T <= 512 (above 128 rows a kernel with eight class columns per lane takes over; up to 128 nothing changes).
 * image_features, text and the workspace 16-byte aligned (the operands and the output of the similarity GEMM); out_full, out_slice 4 bytes. */
size_t excel_cam_workspace_bytes(int B, int N, int T);
int excel_clip_feature_surgery(const float* image_features, const float* text, int B, int N, int C, int T, int F,
                               float temperature, float* out_full, float* out_slice, void* workspace, void* stream);

/* The same attribute maps from the UN-normalised token features (x_raw of excel_vit_forward): token-axis L2 norm (clip/clip.py:353) +
 * similarity GEMM on the matrix core + the surgery epilogue (clip/clip.py:288-310) -- model/model_excel.py:57-58 back to back.  Three
 * launches, each over the whole chip: column sums of squares in image-aligned row blocks (fixed order: an image's maps do not depend
 * on its position in the batch), the similarity tiles (one wave per 32-token tile, >= 7 workgroups per image), and the min-max
 * normalisation over a two-stage (exact) min / max reduction.
 *   mode 1: bf16x3 (fp32 operands as bf16 hi+lo, 3 MFMAs per product), mode 2: f16x3 (IEEE-half planes), mode 0: exact fp32 MFMA.
 *   image_features [B,N,C] (optional): the normalised features generate_clip_fts returns.
 * 1 <= F <= T <= 512, C % 32 == 0, C <= 1024; x_raw, text, image_features and the workspace 16-byte aligned.  Up to 128 text rows all
 * classes of a token tile sit in the accumulators at once; above, the similarity kernel walks the class axis in chunks of 128 rows and
 * takes the redundancy term from f . ((1/T) sum_t w[t] text[t]) (the same sum, associated the other way), so a chunk is complete in
 * itself.  An image's maps do not depend on its place in the batch on either path. */
size_t excel_patch_text_cam_workspace_bytes(int B, int N, int C, int T);
int excel_patch_text_cam(const float* x_raw, const float* text, int B, int N, int C, int T, int F, float temperature, int mode,
                         float* out_full, float* out_slice, float* image_features, void* workspace, void* stream);

/* ------------------------------------------------------------------ DenseCRF post-processing */

/* utils/dcrf.py:42-68 (class DenseCRF; :7-40 crf_inference / crf_inference_label use the same call with other parameters), driven by
 * tools/infer_lam.py:179-237: DenseCRF2D(W, H, C) + setUnaryEnergy + addPairwiseGaussian(sxy = pos_xy_std, compat = pos_w) +
 * addPairwiseBilateral(sxy = bi_xy_std, srgb = bi_rgb_std, rgbim, compat = bi_w) + inference(iters) of pydensecrf (DIAG kernels,
 * symmetric normalisation, Potts compatibilities): mean-field inference with permutohedral-lattice message passing, all on the device.
 *   rgb_hwc [H,W,3] uint8, prob [C,H,W]: probabilities (prob_is_energy = 0: unary = -log(clip(p, 1e-5, 1)), pydensecrf's
 *   unary_from_softmax) or the unary energies themselves (prob_is_energy = 1, e.g. unary_from_labels)  ->  q_out [C,H,W].
 * workspace 8-byte aligned (64-bit fixed-point accumulators); rgb_hwc at any byte. */
size_t excel_dcrf_workspace_bytes(int H, int W, int C);
int excel_dcrf_inference(const unsigned char* rgb_hwc, const float* prob, int prob_is_energy, int H, int W, int C, int iters, float pos_w,
                         float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, float* q_out, void* workspace, void* stream);

/* A group of images of a ragged batch in one chain of launches: excel_dcrf_inference_ragged, below ("segmentation evaluation"). */

/* ------------------------------------------------------------------ affinity random walk */

/* mean over layers of attn[l, 1:, 1:] for one stacked tensor [Lw,B,N,N] -> [B,P,P] (utils/affutils.py:180,197). */
int excel_attn_layer_mean(const float* attn, int Lw, int B, int N, int first_layer, int n_layers, float* w_aff, void* stream);

/* seg_attn branch of refine_cams_with_aff (utils/affutils.py:182-195): of the n_layers per-layer maps
 * attn[first_layer .. first_layer+n_layers) ([Lw,B,N,N] stacked, [1:,1:] used) keep those whose total difference to
 * seg_attn [B,P,P] is <= the mean difference, average them (/ (count + 1e-5)) and gate by seg_attn -> w_out [B,P,P].
 * workspace 8-byte aligned (double partial sums). */
size_t excel_attn_select_workspace_bytes(int B, int n_layers);
int excel_attn_select_mean(const float* attn, int Lw, int B, int N, int first_layer, int n_layers, const float* seg_attn,
                           float* w_out, void* workspace, void* stream);

/* compute_trans_mat (utils/affutils.py:8-24): 3x(col,row) normalise, symmetrise, square (batched fp32 MFMA GEMM).
 * workspace: (2*B*P*P + B*P) floats, 16-byte aligned (the symmetrised matrix is both operands of the squaring GEMM); w_aff and
 * trans_out 4 bytes. */
size_t excel_trans_mat_workspace_bytes(int B, int P);
int excel_compute_trans_mat(const float* w_aff, int B, int P, float* trans_out, void* workspace, void* stream);

/* present-class compaction of one-hot labels [B,F] -> cls_idx [B,Smax] (-1 padded), ncls [B], and optionally
 * nchan [B] = min(ncls,Smax)+1 (channels incl. background)  (cls_lst = torch.where(cls_label)[0], utils/affutils.py:203).
 * More present classes than Smax: ncls[b] is the TRUE count (it may exceed Smax: that is how a caller sees the overflow), cls_idx
 * holds the first Smax present class indices in ascending order, and nchan[b] = Smax + 1.  Every consumer of ncls below clamps it
 * with min(ncls, Smax) and touches rows / channels < Smax (+ 1) only, so such an image is processed as if only its first Smax
 * classes were marked present - same bits, nothing written behind [B,Smax,..] - and the classes beyond are silently dropped.
 * Nothing in the library refuses it: a caller that must not lose classes compares ncls with Smax itself (tools/infer_lam does). */
int excel_cls_compact(const float* onehot, int B, int F, int Smax, int32_t* cls_idx, int32_t* ncls, int32_t* nchan, void* stream);

/* scoremap2bbox + box mask (utils/affutils.py:26-53, :208-214) for every (image, present class):
 *   attr [B,P,F] -> v [B,Smax,P] = mask .* attr[:, :, cls]; mask_out [B,Smax,P] u8 optional. */
int excel_scoremap_box_mask(const float* attr, const int32_t* cls_idx, const int32_t* ncls, int B, int g, int F, int Smax,
                            double caa_thre, float* v_out, uint8_t* mask_out, void* stream);

/* refine_cams_with_aff, batched and fused (utils/affutils.py:177-223, seg_attn=None):
 *   refined[b,s,:] = T2 (mask_s .* attr[:, cls_s]) with T2 = Tsym.Tsym applied as two mat-vecs.
 *   workspace: excel_refine_workspace_bytes.  refined [B,Smax,P]. */
size_t excel_refine_workspace_bytes(int B, int P, int Smax);
int excel_refine_cams_with_aff(const float* attr, const float* w_aff, const int32_t* cls_idx, const int32_t* ncls,
                               int B, int g, int F, int Smax, double caa_thre, float* refined, void* workspace, void* stream);

/* generate_cam_label/scale_cam_image + background channel (utils/affutils.py:55-78, :164-166):
 *   refined [B,Smax,P] -> cams [B,Smax+1,H,W]: channel 0 = 1 - max_c, channels 1..ncls[b] = min-max normalised,
 *   bilinearly (cv2.resize INTER_LINEAR rule) up-sampled maps.  workspace: B*Smax*P floats.
 *   flags: EXCEL_CAMS_ZERO_UNUSED = also write zeros to channels ncls[b]+1..Smax (nothing on the path reads them). */
#define EXCEL_CAMS_ZERO_UNUSED 1
int excel_cam_upsample_bkg(const float* refined, const int32_t* ncls, int B, int g, int Smax, int H, int W, float* cams,
                           void* workspace, int flags, void* stream);

/* ------------------------------------------------------------------ PAR + labels + metric */

/* PAR.forward (utils/PAR.py:64-92): imgs [B,3,h,w], masks [B,Cmax,H,W] -> out [B,Cmax,H,W] after n_iter steps.
 * nchan (optional) [B]: only channels < nchan[b] of image b are refined (ragged class counts).
 * workspace: excel_par_workspace_bytes (aff planes + ping-pong + resized guide).
 * Affinities: by default the 8*ndil weights of a pixel are recomputed inside every Jacobi step from the guide image and 5 per-pixel
 * statistics (20 B/pixel instead of 192 B/pixel of HBM traffic per step) where the tiled kernel applies (dilations [1,2,4,8,12,24] -
 * the only set the reference uses: tools/infer_lam.py:168 - W % 4 == 0, imgs, masks, out and the workspace 16-byte aligned); otherwise, or with
 * flags & EXCEL_PAR_STREAM_AFFINITIES, they are streamed as planes.  Same arithmetic in the same order: the outputs are bit-identical. */
#define EXCEL_PAR_STREAM_AFFINITIES 1
size_t excel_par_workspace_bytes(int B, int Cmax, int H, int W, int ndil);
int excel_par_forward(const float* imgs, int h, int w, const float* masks, const int32_t* nchan, int B, int Cmax, int H, int W,
                      const int32_t* dilations /*host*/, int ndil, int n_iter, float w1, float w2, float* out,
                      void* workspace, int flags, void* stream);

/* Which kernels excel_par_forward (ragged = 0) or excel_par_forward_ragged (ragged = 1) runs a request on (a HOST function: no device
 * work; both entries and their launchers take every decision from the same function).  B images, Cmax mask planes, guide [h, w], masks
 * [H, W]; ragged = 1: a batch of B images of H x W each in the pitched layout.  flags as for excel_par_forward; aligned16: the guide, the
 * workspace, masks and out are all 16-byte aligned (what the entries find out from their pointers).
 * plan[EXCEL_PAR_PLAN_INTS] = {resize, stats, nd, step, stats_grid x, y, z, stats_block, step_grid x, y, z, step_block, tiles_interior,
 *                              tiles_border, refused}:
 *   resize: the guide goes through the align_corners=True resize ((h, w) != (H, W); always for ragged batches);
 *   stats: 0 the tile kernel writing the 5 statistics (recomputing step, W >= 8), 1 the pointwise kernel <nd> writing the 5 statistics
 *          (recomputing step, W == 4), 2 the pointwise kernel <nd> writing 8 * nd affinity planes (streamed step);  nd = ndil;
 *   step: 0 none (n_iter == 0: masks are copied), 1 the recomputing tile kernel (dilations [1,2,4,8,12,24], W % 4 == 0 in the uniform
 *         layout, aligned16, max(Cmax,5) * H * Wp * 4 < 2^31, no EXCEL_PAR_STREAM_AFFINITIES), 2 the streamed-plane kernel;
 *   grids: tile kernels (cdiv(W,64), cdiv(H,16), B) of 512 threads, pointwise and streamed kernels (cdiv(W,64), cdiv(H,4), B) of 256;
 *          ragged: (tiles of the batch, 1 or 4, 1);  step grid and block are 0 for step == 0;
 *   tiles_interior / tiles_border (tile kernels, else 0): the 64 x 16 tiles of ONE image staged in 16-byte pieces (x0 - 24 >= 0 and
 *          x0 + 88 <= W) / in 4-byte pieces with clamped columns;
 *   refused (ragged = 1): 0, or why excel_par_forward_ragged returns EXCEL_ERR_ARG: 1 n_iter < 1, 2 dilations, 3 alignment, 4 the 2^31
 *          limit; every other field is then 0. */
#define EXCEL_PAR_PLAN_INTS 15
int excel_par_plan(int B, int Cmax, int h, int w, int H, int W, const int32_t* dilations /*host*/, int ndil, int n_iter, int flags,
                   int ragged, int aligned16, int32_t* plan /*host*/);

/* refined.argmax(1) -> valid_key lookup (utils/affutils.py:86-87, :168).  cls_idx may be NULL (identity keys).  labels_i64 8-byte aligned. */
int excel_argmax_label(const float* cams, const int32_t* nchan, const int32_t* cls_idx, int B, int Smax, int Cmax,
                       long long HW, uint8_t* labels_u8, int64_t* labels_i64, void* stream);

/* _fast_hist accumulated on device (utils/evaluate.py:9-20): hist[nc*gt+pred] += 1 for gt < nc; hist is int64 [nc*nc].
 * 1 <= num_classes <= 256 (at 256 the label 255 is a class like any other).  Up to 90 classes (nc*nc <= 8192) a workgroup keeps the whole
 * histogram in LDS; above, the same launch runs one set of workgroups per band of 8192 / nc ground-truth rows, each reading all pixels
 * (2 bytes per pixel and band) and counting those of its band.  Integer-exact either way.  gt and pred may start at any byte (a scalar head
 * in front of the 16-byte body); hist 8-byte aligned (64-bit atomic adds). */
int excel_confusion_accumulate(const uint8_t* gt, const uint8_t* pred, long long n, int num_classes, int64_t* hist, void* stream);

/* ------------------------------------------------------------------ ragged batches: B images of DIFFERENT label sizes in one launch
 * The reference evaluates at every image's own label size (tools/infer_lam.py:74,94: the input is resized to S x S, everything after
 * the random walk runs at labels.shape[-2:]) with batch 1; these entry points run the size-dependent half of the path (input resize,
 * CAM up-sampling, PAR, arg-max) for a whole batch at once.  The ViT / CAM / random-walk half is size-uniform (S x S) already.
 *
 * Layout ("pitched planes"): image b has H_b x W_b pixels; rows are padded to Wp_b = W_b rounded up to 4 floats, a plane is
 * H_b * Wp_b floats; image b of a K-plane fp32 tensor starts at element K * poff_b (poff_b = sum_{i<b} H_i * Wp_i) with its planes
 * back to back.  uint8 maps (decoded HWC images, ground truth, labels) are TIGHT: image b at pixel loff_b = sum_{i<b} H_i * W_i, so
 * excel_confusion_accumulate runs over the flat label arrays unchanged.  Work is cut into 64 x 16 pixel tiles, numbered image-major.
 * excel_ragged_plan (a HOST function: no device work) fills `info` and, when `table` != NULL, the int32 table the kernels read:
 *   (B+1) records of 8 ints {H, W, poff, tile_off, loff, 0, 0, 0} (record B = totals), then the image index of every tile;
 * the caller copies `table` (info->table_ints int32) to the device.  Offsets are 32-bit: total padded pixels < 2^31. */
typedef struct {
    int32_t B, total_tiles;
    int64_t total_pix;         /* sum H_b * Wp_b: elements of a one-plane pitched tensor */
    int64_t total_label_pix;   /* sum H_b * W_b:  elements of a tight u8 map */
    int64_t max_plane_pix;     /* max H_b * Wp_b */
    int64_t table_ints;
} excel_ragged_info;
int excel_ragged_plan(const int32_t* hw /*host [B,2] = (H_b, W_b)*/, int B, excel_ragged_info* info /*host*/, int32_t* table /*host or NULL*/);

/* ------------------------------------------------------------------ overflow guard of the f16 modes
 * Modes 2 and 3 of excel_vit_set_gemm_mode turn an activation beyond 65 504 into NaNs.  These two entries let a batched step see that per
 * image and keep such an image out of its scores without a host synchronisation; the caller re-runs the flagged images in mode 0.
 *
 * excel_nonfinite_count: x = B images of per_image fp32 values each, back to back; count[b] receives (init != 0) or is increased by
 * (init == 0) the number of values of image b whose exponent field is all ones (+-inf and every NaN; an integer test on the bits), so the
 * tensors of one step can share one counter.  x need only be 4-byte aligned, per_image is any value in [1, 2^31).  A streaming read: no
 * workspace, and a tensor without such a value issues no atomic. */
int excel_nonfinite_count(const float* x, int B, long long per_image, int32_t* count /*device [B]*/, int init, void* stream);

/* excel_confusion_accumulate restricted to the images with skip[b] == 0 (skip: e.g. the counts above).  table == NULL: B uniform images
 * of per_image pixels each (info unused); otherwise the tight label maps of the ragged plan (image b at loff_b; per_image ignored,
 * info->B == B).  Integer counts: with nothing skipped the result equals excel_confusion_accumulate over the whole array bit for bit,
 * otherwise excel_confusion_accumulate over the concatenation of the kept images.  1 <= num_classes <= 256, banded above 90 likewise.
 * gt and pred at any byte, hist 8-byte aligned as there. */
int excel_confusion_accumulate_masked(const uint8_t* gt, const uint8_t* pred, int B, long long per_image, const int32_t* table,
                                      const excel_ragged_info* info, const int32_t* skip /*device [B]*/, int num_classes, int64_t* hist,
                                      void* stream);

/* ------------------------------------------------------------------ per-image scores
 * The confusion entries above add a whole step into one matrix; this one keeps what every image contributed, as the three margins of the
 * image's own matrix - all that IoU, mIoU and pixel accuracy of one image are computed from (utils/evaluate.py, image_score_rows).
 * Images are addressed exactly as in excel_confusion_accumulate_masked: table == NULL means B uniform images of per_image pixels each
 * (info unused); otherwise the tight u8 maps of the ragged plan (image b at loff_b; per_image ignored, info->B == B).  A pixel of image
 * b with ground truth g and prediction p counts only when g < nc and p < nc (the rule of the confusion kernels: a 255 in either map
 * drops the pixel); for a counted pixel
 *   counts[b,0,g] += 1 (ground-truth area),   counts[b,1,p] += 1 (predicted area),   counts[b,2,g] += 1 when g == p (intersection).
 * Every element of counts is written (cleared on the stream first); the rows of an image with skip[b] != 0 stay zero (skip may be NULL).
 * Summed over the images, rows 0 / 1 / 2 are the row sums, column sums and diagonal of excel_confusion_accumulate's matrix (with skip:
 * of excel_confusion_accumulate_masked's), integer for integer.  1 <= num_classes <= 256, 1 <= B <= 65535, per_image in [1, 2^31): a
 * count fits an int32.  No workspace, no host synchronisation; one kernel, the 3 * nc counters of a workgroup live in LDS. */
int excel_image_scores(const uint8_t* gt, const uint8_t* pred, int B, long long per_image, const int32_t* table,
                       const excel_ragged_info* info, const int32_t* skip /*device [B] or NULL*/, int num_classes,
                       int32_t* counts /*device [B,3,num_classes]*/, void* stream);

/* ------------------------------------------------------------------ boundary scores
 * excel_image_scores restricted to the contour bands: the counts Boundary IoU (Cheng et al., CVPR 2021) is computed from.  For a map m
 * and an integer radius d >= 1, pixel (x,y) lies in the band of m iff some position (x',y') with max(|x'-x|, |y'-y|) <= d is outside
 * the image or holds a value m(x',y') != m(x,y) - raw values: 255 and any value >= nc are simply different.  For the binary mask
 * m == c that is the original implementation's mask_to_boundary: mask - erode(mask), 3x3 kernel, d iterations, a one-pixel zero border.
 * Over the pixels with g < nc and p < nc (the rule of the confusion kernels)
 *   counts[b,0,c] = #{g == c, in the band of gt},  counts[b,1,c] = #{p == c, in the band of pred},
 *   counts[b,2,c] = #{g == p == c, in both bands},
 * so utils/evaluate.image_score_rows turns a row into the image's Boundary IoU per class, unchanged.  Images: table == NULL means B
 * uniform [H,W] maps; otherwise the tight u8 maps of the ragged plan (row pitch W_b, image b at loff_b; H, W ignored, info->B == B).
 * radius: device int32 [B], or NULL: every image uses max_radius.  The radius is the caller's (host) arithmetic - the device does none;
 * max_radius (host) bounds every radius[b] and sizes the halo, 1 <= max_radius <= excel_boundary_max_radius() (72: 2 % of a 3600-pixel
 * diagonal).  Every element of counts is written (cleared on the stream first); the rows of an image with skip[b] != 0 stay zero (skip
 * may be NULL); otherwise an image with radius[b] < 1 or radius[b] > max_radius gets -1 in all 3 * nc entries - refused, never clamped.
 * 1 <= num_classes <= 256, 1 <= B <= 65535.  One launch behind the clearing, no workspace, no host synchronisation; positions outside
 * an image are never read, and the maps may start at any byte address. */
int excel_boundary_scores(const uint8_t* gt, const uint8_t* pred, int B, int H, int W, const int32_t* table, const excel_ragged_info* info,
                          const int32_t* radius /*device [B] or NULL*/, int max_radius, const int32_t* skip /*device [B] or NULL*/,
                          int num_classes, int32_t* counts /*device [B,3,num_classes]*/, void* stream);
int excel_boundary_max_radius(void);

/* ------------------------------------------------------------------ background-scale sweep
 * The pseudo labels are excel_argmax_label_ragged of PAR's output, whose plane 0 is the background 1 - max_c cam_c (utils/affutils.py:
 * 161-174: torch.pow(1 - max, 1.)).  PAR is linear per channel, PAR(a * bkg) = a * PAR(bkg), so the labels of a background scaled by
 * `a` are a second compare on the SAME planes - no second PAR pass.  This entry scores K such scales against the ground truth in one
 * pass over the planes, without a label map per scale, and / or writes the label map of one of them.
 *   planes = PAR's output, Cmax pitched planes per image in the layout of excel_argmax_label_ragged (table, info, nchan, cls_idx, Smax
 *   and Cmax as there; with cls_idx, Smax >= Cmax - 1);  gt = the tight u8 ground truth (image b at loff_b), NULL when totals is NULL.
 * For pixel (x,y) of image b, x < W_b:  nch = nchan ? min(nchan[b], Cmax) : Cmax;  b0 = plane 0;  F = the maximum of planes 1..nch-1;
 * ci = the first plane index that attains F;
 *   key_j = (nch == 1 || scales[j] * b0 >= F) ? 0 : (cls_idx ? cls_idx[b*Smax + ci-1] + 1 : ci)        for j = 0..K-1
 * - one fp32 multiply (round to nearest, nothing fused into it) and one compare.  With scales[j] == 1.0f key_j is the label
 * excel_argmax_label_ragged writes, on finite planes: the background wins a tie, the first foreground maximum wins.  Pad columns
 * (W_b <= x < Wp_b) and planes c >= nch are never read.
 *   totals (device int64 [K,3,num_classes], or NULL): a pixel counts for scale j iff (skip == NULL || skip[b] == 0), g = gt < num_classes
 *   and key_j < num_classes (the rule of the confusion kernels); then
 *     totals[j,0,g] += 1,   totals[j,1,key_j] += 1,   totals[j,2,g] += 1 when g == key_j
 *   - the row sums, column sums and diagonal of the [nc,nc] confusion matrix of the labels at scale j, in the row layout of
 *   excel_image_scores (utils/evaluate.image_score_rows reads them).  totals is ADDED to, like `hist`, across calls: the caller clears it.
 *   labels_u8 (device, tight, info->total_label_pix bytes, or NULL): key_{label_sel} of every pixel, whatever skip says.
 * scales: HOST array of K floats, copied into the kernel arguments (no upload, no host synchronisation); any order - the result does not
 * depend on it or on the sign of b0; increasing scales on b0 >= 0 are the fast case (bkgsweep.hip).
 * EXCEL_ERR_ARG with a message for: null planes, table or info; neither totals nor labels_u8; totals without gt; K outside 1..16; a scale
 * that is not finite or < 0; label_sel outside [0, K) when labels_u8 is given; num_classes outside 1..256; totals not 8-byte or planes
 * not 16-byte aligned.  One launch on `stream`, no workspace, no scratch memory. */
int excel_bkg_sweep_ragged(const float* planes, const int32_t* nchan /*device [B] or NULL*/, const int32_t* cls_idx /*device [B,Smax] or NULL*/,
                           const uint8_t* gt, const int32_t* table, const excel_ragged_info* info, int Smax, int Cmax,
                           const float* scales /*HOST [K]*/, int K, const int32_t* skip /*device [B] or NULL*/, int num_classes,
                           int64_t* totals /*device [K,3,num_classes], ADDED to, or NULL*/, int label_sel,
                           uint8_t* labels_u8 /*device, tight, or NULL*/, void* stream);

/* ------------------------------------------------------------------ arg-max margin
 * By how much the winning plane of the arg-max won: a confidence per pixel that PAR's output already holds.  One pass over the planes
 * scores the labels cut at K margin thresholds (a risk-coverage sweep) and / or writes the label map cut at one value and / or the
 * margins themselves.  planes, nchan, cls_idx, gt, table, info, Smax, Cmax and skip are those of excel_bkg_sweep_ragged, and so are the
 * tiles; pad columns and planes c >= nch are never read.
 * For pixel (x,y) of image b, x < W_b, with nch = nchan ? min(nchan[b], Cmax) : Cmax and a = bkg_scale:
 *   v0 = a * plane 0 (one fp32 multiply, round to nearest);  for nch > 1:  F = the maximum of planes 1..nch-1, ci = the first plane index
 *   that attains it, key_fg = cls_idx ? cls_idx[b*Smax + ci-1] + 1 : ci.
 *   The pixel is background iff nch == 1 or v0 >= F or key_fg == 0: key = 0; otherwise key = key_fg - the labels of
 *   excel_bkg_sweep_ragged at scale a, bit for bit.
 *   Runner-up R:  background: R = F;  foreground: R = max(v0, S), S = the maximum of the foreground planes other than ci (nch == 2 has
 *   none: R = v0).
 *   margin = winner - R (winner = v0 or F): one fp32 subtract, round to nearest, nothing fused into it.  nch == 1: margin = +inf, plane 0
 *   plays no part.  When nch > 1 and v0 or one of the planes 1..nch-1 is NaN the margin is NaN, and inf - inf is NaN: a NaN margin fails
 *   every comparison below.  A negative margin is possible only for the key_fg == 0 case (v0 < F) and stays as it is.
 * thresholds: HOST array of K floats (0 <= K <= 16), finite, >= 0, strictly increasing, copied into the kernel arguments.  The pixel is
 * kept at j iff margin >= thresholds[j]; the kept sets are nested.
 *   totals (device int64 [K,3,num_classes], ADDED to, or NULL; needs gt): over the pixels kept at j with g = gt < num_classes and
 *     key < num_classes of the images with skip == NULL || skip[b] == 0:  totals[j,0,g] += 1, totals[j,1,key] += 1, totals[j,2,g] += 1
 *     when g == key - the row sums, column sums and diagonal of the confusion matrix of "key, with 255 where the pixel is dropped", in
 *     the layout of excel_bkg_sweep_ragged's totals.
 *   kept (device int64 [K+1], ADDED to, or NULL; needs no gt): kept[j] += the pixels kept at j, kept[K] += all pixels, of the images
 *     with skip == NULL || skip[b] == 0, whatever their ground truth.  Coverage at j = kept[j] / kept[K].
 *   labels_u8 (device, tight, info->total_label_pix bytes, or NULL): margin >= label_thre ? key : 255, for every image whatever skip
 *     says.  label_thre is independent of `thresholds` (any value but NaN; -inf keeps every pixel whose margin is not NaN).
 *   margin_out (device float [info->total_label_pix], tight, or NULL): the margin.
 * EXCEL_ERR_ARG with a message, before any launch, for: null planes, table or info; none of the four outputs; totals without gt; K
 * outside 0..16; K == 0 with totals or kept; a threshold that is not finite, is < 0 or does not increase; labels_u8 with a NaN
 * label_thre; bkg_scale not finite or < 0; num_classes outside 1..256; planes not 16-byte aligned; totals or kept not 8-byte aligned;
 * margin_out, nchan, cls_idx, skip or table not 4-byte aligned; a plan without a tile.  labels_u8 and gt may start at any byte.
 * One launch on `stream`, no workspace, no host synchronisation, no scratch memory (csrc/margin.hip). */
int excel_margin_sweep_ragged(const float* planes, const int32_t* nchan /*device [B] or NULL*/, const int32_t* cls_idx /*device [B,Smax] or NULL*/,
                              const uint8_t* gt, const int32_t* table, const excel_ragged_info* info, int Smax, int Cmax, float bkg_scale,
                              const float* thresholds /*HOST [K]*/, int K, const int32_t* skip /*device [B] or NULL*/, int num_classes,
                              int64_t* totals /*device [K,3,num_classes], ADDED to, or NULL*/, int64_t* kept /*device [K+1], ADDED to, or NULL*/,
                              float label_thre, uint8_t* labels_u8 /*device, tight, or NULL*/, float* margin_out /*device, tight, or NULL*/,
                              void* stream);

/* ------------------------------------------------------------------ connected components
 * The regions of label maps, and the filter that turns the small ones into ignore (255).  Images are addressed exactly as in
 * excel_boundary_scores: table == NULL means B uniform [H,W] maps; otherwise the tight u8 maps of the ragged plan (row pitch W_b, image b
 * at loff_b; H, W ignored, info->B == B).  The maps may start at any byte address; comp and area use the same pixel indexing, 4-byte
 * aligned.
 *
 * excel_label_components: two pixels of ONE image are connected when they are 4- or 8-neighbours (connectivity 4 or 8) and hold the same
 * raw value - every raw value forms components, 0 and 255 included, and nothing connects across images (not even the last pixel of
 * image b and the first of image b + 1 in the tight layout).
 *   comp[i] = the image-local linear index y * W_b + x of the first pixel, in raster order, of i's component - canonical: it does not
 *             depend on tiling, scheduling or the order of the atomics;
 *   area[i] = the number of pixels of i's component, at every pixel.
 * Every element of both outputs is written, neither is read before it is written (area is cleared on the stream).  Block union-find in
 * four launches (tile pieces in LDS, seams, flatten + count, broadcast; csrc/components.hip) with no waiting between workgroups: every
 * link ever stored satisfies parent <= child, so every loop is bounded by construction.  No workspace, no host synchronisation, no
 * scratch memory.  EXCEL_ERR_ARG before any launch for: a null labels, comp or area; connectivity other than 4 or 8; B outside
 * [1, 65535]; a uniform H * W or a ragged total outside [1, 2^31); comp or area not 4-byte aligned. */
int excel_label_components(const uint8_t* labels, int B, int H, int W, const int32_t* table, const excel_ragged_info* info,
                           int connectivity, int32_t* comp /*device, one per pixel*/, int32_t* area /*device, one per pixel*/,
                           void* stream);

/* excel_filter_small_regions: with thr = min_area ? min_area[b] : min_area_all, for every pixel of image b
 *   out = 255 if labels < num_classes and area < thr, else out = labels
 * - a region of exactly thr pixels stays; pixels with a value >= num_classes (255 included) pass through and their components are never
 * counted.  counts (device int32 [B,3], cleared on the stream): counts[b,0] = components with a value < num_classes, counts[b,1] = those
 * removed, counts[b,2] = pixels set to 255; a component is counted once, at its root pixel (comp[i] == i).  An image with thr < 1 is
 * refused, never clamped: its counts row is -1 and its map is copied unchanged.  comp / area: excel_label_components' outputs for the
 * same maps and addressing.  out may not overlap labels.  One launch behind the clearing, no workspace, no host synchronisation.
 * EXCEL_ERR_ARG before any launch for: a null labels, comp, area, out or counts; out overlapping labels; num_classes outside 1..256; B or
 * the sizes as above; comp, area, counts or min_area not 4-byte aligned. */
int excel_filter_small_regions(const uint8_t* labels, const int32_t* comp, const int32_t* area, int B, int H, int W, const int32_t* table,
                               const excel_ragged_info* info, const int32_t* min_area /*device [B] or NULL*/, int min_area_all,
                               int num_classes, uint8_t* out, int32_t* counts /*device [B,3]*/, void* stream);

/* ------------------------------------------------------------------ nearest-label fill
 * The other half of the cleaning above: a removed pixel takes the class it sits in.  An exact Euclidean nearest-label transform in
 * integers (squared distances); the result is canonical.  Images are addressed exactly as in excel_label_components: table == NULL means
 * B uniform [H,W] maps; otherwise the tight u8 maps of the ragged plan (row pitch W_b, image b at loff_b; H, W ignored, info->B == B).
 * labels, mask and out may start at any byte address; dist2 uses the same pixel indexing, 4-byte aligned.
 *   seed   a pixel with labels < num_classes (a mask never un-seeds a pixel);
 *   hole   a pixel with labels == 255, and with mask[i] != 255 when mask is given (mask: a second map with the same addressing, e.g. the
 *          map before the cleaning - what was 255 there stays 255); with mask == NULL every 255 pixel is a hole;
 *   other  values in [num_classes, 255) are neither: they pass through and block nothing.
 * For a hole p = (py, px) of image b, among the seeds q = (qy, qx) of the SAME image that minimise d2 = (py-qy)^2 + (px-qx)^2 take the
 * first in raster order (the smallest qy, then the smallest qx).  If d2 <= max_dist2:  out[p] = labels[q], dist2[p] = d2.  Otherwise, or
 * when the image has no seed:  out[p] = 255, dist2[p] = -1.  Every other pixel:  out = labels;  dist2 = 0 at seeds and -1 elsewhere.
 * Nothing reaches across images (not even between the last pixel of image b and the first of image b + 1 in the tight layout).
 *   counts[b] = (holes, holes filled, the largest d2 of a filled hole or 0), device int32 [B,3], cleared on the stream.
 * Every element of out, dist2 and counts is written and none is read before it is written, except what this entry wrote earlier in the
 * same call: dist2 carries the intermediate (per pixel the row of the nearest seed of its column) between the two launches - a column
 * pass, then a row pass whose every workgroup reads only its own row of it (csrc/fill.hip).  No workspace and no size query, no host synchronisation, no
 * scratch memory, everything on `stream`; no workgroup waits for another, every loop is bounded by a side of the image.
 * EXCEL_ERR_ARG before any launch for: a null labels, out, dist2 or counts; out overlapping labels or mask; num_classes outside 1..255;
 * max_dist2 < 1; B outside [1, 65535]; a uniform image higher or wider than 8192 (d2 then fits 28 bits and a row of candidates fits in
 * LDS); a total outside [1, 2^31); dist2 or counts not 4-byte aligned.  The sizes of a ragged batch live in the device table, which the
 * host entry does not read: there an image beyond 8192 a side is refused by the kernels, never clamped - its map is copied, its dist2 is
 * 0 at seeds and -1 elsewhere, and its counts row is -1 (utils/label_fill.py refuses such a plan on the host). */
int excel_fill_nearest_label(const uint8_t* labels, const uint8_t* mask /*or NULL*/, int B, int H, int W, const int32_t* table,
                             const excel_ragged_info* info, int num_classes, int max_dist2, uint8_t* out,
                             int32_t* dist2 /*device, one per pixel*/, int32_t* counts /*device [B,3]*/, void* stream);

/* ------------------------------------------------------------------ superpixel snap
 * The one stage behind the arg-max that looks at the image again: over-segment the image into superpixels and give every superpixel
 * the majority class of the labels inside it.  Integer arithmetic throughout; the result is canonical - it does not depend on tiling,
 * scheduling or the order of any atomic.  Images are addressed exactly as in excel_label_components: table == NULL means B uniform [H,W]
 * maps; otherwise the tight maps of the ragged plan (image b at loff_b; H, W ignored, info->B == B).  hwc holds the decoded uint8
 * [H_b,W_b,3] images back to back, image b at byte 3 * loff_b.  hwc, labels and out may start at any byte address; sp uses the pixel
 * indexing of the label maps, 4-byte aligned.  Nothing reaches across images.
 *
 * excel_slic_superpixels: integer SLIC on a fixed grid (the gSLIC form), step S in [2, 64], compactness m in [1, 64], iters T in [0, 16].
 *   grid    gx = ceil(W_b / S), gy = ceil(H_b / S); centre k = cy * gx + cx starts at x = min(W_b - 1, cx S + S/2),
 *           y = min(H_b - 1, cy S + S/2) with the colour of the pixel there;
 *   assign  pixel (x, y) lies in cell (x / S, y / S) and considers the centres of the up to nine cells within +-1 of it that exist:
 *           D = S^2 ((r-rk)^2 + (g-gk)^2 + (b-bk)^2) + m^2 ((x-xk)^2 + (y-yk)^2), the smallest D wins, the smallest k on a tie.
 *           D < 2^31: colours give at most 3 * 255^2 = 195075; a centre stays within the 3 x 3 cells around its own cell (it is a mean
 *           of pixels from there), so |x-xk|, |y-yk| < 3S and D <= 4096 * 195075 + 4096 * 18 * 4096 = 1 101 017 088;
 *   update  per centre the sums of x, y, r, g, b and the count cnt over its pixels; new value = (2 sum + cnt) / (2 cnt), floor; a centre
 *           without a pixel keeps its values;
 *   sequence  init, T times (assign, update), a final assign.
 * sp[i] = the image-local centre index of pixel i; centres = int32 {x, y, r, g, b} per centre at the final state, the centres of image b
 * from centre cent_off[b] on.  cent_off: device int32 [B + 1], cent_off[b+1] - cent_off[b] = gy_b * gx_b, supplied by the caller with
 * the host total cent_total (the sizes of a ragged batch live on the device, which the host entry does not read).  An image whose row
 * is wrong - cent_off[b] < 0, cent_off[b+1] > cent_total or a difference other than gy * gx - is refused by the kernels, never clamped:
 * its sp is -1 and none of its centres is written.  Superpixels are NOT made connected; excel_label_components can follow.
 *
 * excel_snap_labels_to_superpixels: a pixel votes iff labels < num_classes (1..255).  Per superpixel: tot = its votes, top = the largest
 * class count, win = the smallest class that attains it; it is snapped iff tot > 0 and 1000 top >= min_share_pm tot (min_share_pm in
 * [0, 1000]).  out = win at the voting pixels of a snapped superpixel; everywhere else out = labels: 255, values in [num_classes, 255),
 * superpixels not snapped, pixels with sp < 0.  sp is what excel_slic_superpixels wrote for the same geometry, step and cent_off (or -1):
 * a pixel whose sp names a centre beyond the 3 x 3 cells around its own cell is not seen by that centre and keeps its label.
 * counts[b] = (superpixels with a vote, superpixels snapped, pixels whose value changed), device int32 [B,3], cleared on the stream; an
 * image with a wrong cent_off row keeps its labels and counts nothing.  out may overlap neither labels nor sp.
 *
 * Both: everything on `stream` (2 T + 2 launches; a copy, a clearing and one launch), no host synchronisation, no workspace (centres is
 * the only intermediate: assign reads it and writes sp, update reads sp and writes it - csrc/superpixels.hip), no scratch memory; no
 * workgroup waits for another; every loop is bounded by the 3S x 3S window, the centres under a tile or T.  EXCEL_ERR_ARG with a message
 * before any launch for: a null pointer; step, compactness, iters, num_classes or min_share_pm out of range; sp, centres, counts,
 * cent_off or table not 4-byte aligned; B outside [1, 65535]; a pixel total or cent_total outside [1, 2^31), or more centres than
 * pixels; out overlapping labels or sp. */
int excel_slic_superpixels(const uint8_t* hwc, int B, int H, int W, const int32_t* table, const excel_ragged_info* info,
                           const int32_t* cent_off /*device [B+1]*/, long long cent_total, int step, int compactness, int iters,
                           int32_t* sp /*device, one per pixel*/, int32_t* centres /*device [cent_total,5]*/, void* stream);
int excel_snap_labels_to_superpixels(const uint8_t* labels, const int32_t* sp, int B, int H, int W, const int32_t* table,
                                     const excel_ragged_info* info, const int32_t* cent_off /*device [B+1]*/, long long cent_total, int step,
                                     int num_classes, int min_share_pm, uint8_t* out, int32_t* counts /*device [B,3]*/, void* stream);

/* ------------------------------------------------------------------ image tags: the one-hot rows excel_cls_compact reads, predicted
 * Row 0 of the tower's x_raw is CLIP's own image embedding: the reference puts the class token of the original attention path back
 * before ln_post / proj (clip/clip_surgery_model.py:442-446).  The reference never tags images itself (weakly-supervised segmentation
 * assumes the tags; its tools carry an unused --tag_threshold 0.2); this entry is CLIP's zero-shot classification over the same text
 * rows the CAM uses, so a batched step runs without image-level labels and without a host synchronisation.
 *   x_cls  = the class-token row of image 0; image b's row is at x_cls + b * stride floats (stride = N * C for x_raw [B,N,C], C for a
 *            compact [B,C]);  text [T,C], the F <= T foreground rows first (the others are background prompts);
 *   cos[t] = <x, text_t> / (||x|| ||text_t||), both norms computed here (the rows need not be unit-norm);
 *   p[t]   = softmax over ALL T rows of scale * cos[t] (the background prompts compete; scale = 100 is CLIP's logit scale);
 *   rank[f] = #{g < F : p[g] > p[f] or (p[g] == p[f] and g < f)}   - a tie goes to the lower class index;
 *   tag[f] = rank[f] < kmax and (rank[f] == 0 or p[f] >= rel_thre * max_f p[f]).
 * The threshold is relative to the best foreground score (the absolute mass depends on how many prompts compete) and the top-1 class is
 * always kept: an image with finite logits never has an empty row, and never more than kmax tags.  An image whose logits are not all
 * finite (a NaN / inf in its row, a zero row) gets tag = {class 0} and a row of NaNs in scores_out - never an empty row; every CAM of
 * such an image is non-finite as well (the class token weights all of them), so the overflow guard above flags it.
 *   onehot_out f32 [B,F] (1.0 / 0.0, every element written);  scores_out f32 [B,F] = p[f], or NULL.
 * One 256-thread workgroup per image; no workspace, no atomics.  EXCEL_ERR_ARG unless 1 <= F <= T <= 512, F <= 254, C % 4 == 0,
 * C <= 1024, stride >= C, stride % 4 == 0, x_cls and text 16-byte aligned, 1 <= kmax <= F, 0 <= rel_thre <= 1, scale > 0. */
int excel_clip_tags(const float* x_cls, long long stride, const float* text, int B, int C, int T, int F, float scale, float rel_thre,
                    int kmax, float* onehot_out, float* scores_out, void* stream);

/* datasets/transforms.normalize_img + HWC->CHW + the harness' input resize (tools/infer_lam.py:74: F.interpolate bilinear,
 * align_corners=False, no antialias) for decoded images of different sizes: hwc = the uint8 [H_b,W_b,3] images back to back
 * (image b at byte 3 * loff_b) -> out [B,3,S,S] f32.  Same operations (same bits) as excel_normalize_img_u8 + excel_bilinear_resize. */
int excel_normalize_resize_u8_ragged(const uint8_t* hwc, const int32_t* table, int B, int S, const double* mean3 /*host*/,
                                     const double* std3 /*host*/, float* out, void* stream);

/* excel_normalize_resize_u8_ragged plus its mirror, in one pass: out [2B,3,S,S], images 0..B-1 bit-identical to
 * excel_normalize_resize_u8_ragged, image B + b = image b mirrored along W (the flip-TTA input [x; flip x] of utils/camutils.py:15,
 * which flips after the resize: the mirrored half is a second store of the same values, not a second resize). */
int excel_normalize_resize_u8_ragged_mirror(const uint8_t* hwc, const int32_t* table, int B, int S, const double* mean3 /*host*/,
                                            const double* std3 /*host*/, float* out, void* stream);

/* excel_cam_upsample_bkg for a ragged batch: refined [B,Smax,P] -> cams = (Smax+1) pitched planes per image. workspace: B*Smax*P floats.
 * cams 16-byte aligned (every pitched row then is: the layout's premise). */
int excel_cam_upsample_bkg_ragged(const float* refined, const int32_t* ncls, const int32_t* table, const excel_ragged_info* info, int g,
                                  int Smax, float* cams, void* workspace, int flags, void* stream);

/* PAR.forward for a ragged batch: imgs [B,3,h,w] (the uniform network input; resized per image with align_corners=True like
 * PAR.py:67), masks / out = Cmax pitched planes per image.
 * Narrower contract than excel_par_forward (only the recomputing tile kernel exists for ragged batches; there is no streamed-affinity
 * fallback): returns EXCEL_ERR_ARG (-1) unless
 *   - n_iter >= 1            (excel_par_forward copies masks to out for n_iter == 0; here that is an error),
 *   - dilations == [1,2,4,8,12,24] (what the reference always uses, PAR.py callers),
 *   - masks, out and the workspace are 16-byte aligned and max(Cmax,5) * H_b * Wp_b * 4 < 2^31 for every image (Wp_b = W_b rounded up to 4).
 * The pad columns (W_b <= x < Wp_b) of `out` and its planes c >= nchan[b] are UNDEFINED on return (masks' pad columns are never read
 * as neighbours); consumers clamp to W_b - 1 and nchan[b] (excel_argmax_label_ragged does). */
size_t excel_par_ragged_workspace_bytes(long long total_pix, int Cmax);
int excel_par_forward_ragged(const float* imgs, int h, int w, const float* masks, const int32_t* nchan, const int32_t* table,
                             const excel_ragged_info* info, int Cmax, const int32_t* dilations /*host*/, int ndil, int n_iter, float w1,
                             float w2, float* out, void* workspace, void* stream);

/* excel_argmax_label for a ragged batch: cams = Cmax pitched planes per image -> tight uint8 labels (info->total_label_pix). */
int excel_argmax_label_ragged(const float* cams, const int32_t* nchan, const int32_t* cls_idx, const int32_t* table,
                              const excel_ragged_info* info, int Smax, int Cmax, uint8_t* labels_u8, void* stream);

/* ------------------------------------------------------------------ segmentation evaluation over ragged batches (segeval.hip)
 * The size-dependent half of tools/infer_seg_voc.py / tools/infer_seg_coco.py: the reference runs one image per step and fuses, resizes
 * and arg-maxes at that image's size (_validate :58-91); these run a whole ragged batch in one launch per stage, in the layout above.
 *
 * excel_seg_msc_fuse_ragged replaces :63-82 (coco :62-80): for ns <= 8 scales, segs[s] = the decoder logits [2B, nc, g_s, g_s] (image b,
 * then the flipped image b at B + b), for every image at its plan size (h_b, w_b) and every class
 *   v_s = bilinear (align_corners=False) of scale s at (h_b, w_b); flip_mean[s] ? (v_s + flip_x(v_s of the flipped copy)) / 2 : v_s
 *   acc = v_0; acc = acc + v_s for s >= 1; the last step multiplies by 1/ns   (torch.mean over the stacked scales, :82)
 * with the operations, in the order, of a per-image chain of excel_seg_scale_accumulate calls: the same bits.
 *   planes    (optional) nc pitched planes per image (16-byte aligned; nc * total_pix < 2^31)
 *   labels_u8 (optional) tight arg-max over classes, first maximum (excel_argmax_label's rule; nc <= 256).  These equal the reference's
 *             labels only where the label size IS the plan size (VOC, :84-85 is then the identity); callers check that.
 * segs, g, flip_mean are host arrays of ns entries; the maps they point to are device memory. */
int excel_seg_msc_fuse_ragged(const float* const* segs /*host [ns]*/, const int32_t* g /*host [ns]*/, const int32_t* flip_mean /*host [ns]*/,
                              int ns, int nc, const int32_t* table, const excel_ragged_info* info, float* planes, uint8_t* labels_u8,
                              void* stream);

/* tools/infer_seg_coco.py:86-87 (F.interpolate of the fused logits to labels.shape, then argmax(1)) without the resized logits: planes =
 * nc pitched planes per image at the sizes of (src_table, src_info) -> tight uint8 labels at the sizes of (dst_table, dst_info), both
 * plans over the same B images.  Same bits as excel_bilinear_resize + excel_argmax_label per image. */
int excel_seg_resize_argmax_ragged(const float* planes, const int32_t* src_table, const excel_ragged_info* src_info, const int32_t* dst_table,
                                   const excel_ragged_info* dst_info, int nc, uint8_t* labels_u8, void* stream);

/* excel_seg_resize_argmax_ragged from a TIGHT uniform source: segs = [B, nc, h, w] f32 (the decoder's seg logits of one batch, any h, w;
 * no row padding) -> tight uint8 arg-max labels at the sizes of (dst_table, dst_info), B images.  The in-training validation's seg
 * prediction (engine/validatation_engine.py:27,37: F.interpolate to labels.shape, argmax(1)) for a ragged batch in one launch.  Same
 * kernel, same bits as excel_bilinear_resize + excel_argmax_label per image. */
int excel_seg_resize_argmax_uniform(const float* segs, int B, int h, int w, int nc, const int32_t* dst_table, const excel_ragged_info* dst_info,
                                    uint8_t* labels_u8, void* stream);

/* The DenseCRF's input for ONE image (tools/infer_seg_voc.py:146-147 softmax(logit); tools/infer_seg_coco.py:144-145 F.interpolate to
 * (H, W) then softmax): planes = nc pitched planes (row pitch w rounded up to 4 floats) at (h, w) -> prob tight [nc, H, W], the layout
 * excel_dcrf_inference takes.  (h, w) == (H, W) skips the resize. */
int excel_seg_softmax_resize(const float* planes, int h, int w, int nc, int H, int W, float* prob, void* stream);

/* excel_seg_softmax_resize for every image of a ragged batch in one launch (tools/infer_seg_voc.py:146-147 with dst = src sizes,
 * tools/infer_seg_coco.py:144-145 with the 0.2x fuse sizes as src): planes = nc pitched planes per image at the sizes of
 * (src_table, src_info) -> prob tight [nc, H_b, W_b] per image at the sizes of (dst_table, dst_info), image b at element nc * loff_b:
 * the unary excel_dcrf_inference_ragged takes.  Same kernel, same bits as excel_seg_softmax_resize per image. */
int excel_seg_softmax_resize_ragged(const float* planes, const int32_t* src_table, const excel_ragged_info* src_info, const int32_t* dst_table,
                                    const excel_ragged_info* dst_info, int nc, float* prob, void* stream);

/* ------------------------------------------------------------------ confident labels: two thresholds and an ignore band (conf.hip)
 * utils/affutils.py:101-158 (refine_cams_with_bkg_v2; twin at utils/camutils.py:264-304) makes one PAR pass per background score at
 * half resolution and ignores the pixels only the strict pass calls background.  For a ragged batch the two passes are ONE
 * excel_par_forward_ragged over 2 (k_b + 1) planes per image on the "half plan" (the excel_ragged_plan of (H_b / ds, W_b / ds)); these
 * two entries are what stands in front of and behind it.  smax <= 127; neither takes a workspace.
 *
 * excel_conf_planes_ragged replaces :115-118 and :129-141: cams = smax + 1 pitched planes per image at the sizes of
 * (src_table, src_info) (the excel_cam_upsample_bkg_ragged layout; plane 0 is never read), nchan[b] = k_b + 1.  Every class plane goes
 * to the half plan (bilinear, align_corners=False: the operations and bits of excel_bilinear_resize, each value computed once) and
 * planes = 2 (smax + 1) pitched planes per image on the half plan receives
 *   planes [0, k_b]            softmax_c([high_thre, m_1 .. m_k])
 *   planes [k_b + 1, 2k_b + 1] softmax_c([low_thre,  m_1 .. m_k])
 * (maximum subtracted, sum in channel order 0..k, one division per value; a resized constant is the constant), and
 * nchan2[b] = 2 (k_b + 1) describes the two groups to excel_par_forward_ragged.  Planes >= nchan2[b] and the pad columns stay undefined.
 * softmax == 0 (tests): the first group receives [high_thre, m_1 .. m_k] as resized and nothing else is written. */
int excel_conf_planes_ragged(const float* cams, const int32_t* nchan, const int32_t* src_table, const excel_ragged_info* src_info,
                             const int32_t* half_table, const excel_ragged_info* half_info, int smax, float high_thre, float low_thre,
                             int softmax, float* planes, int32_t* nchan2 /*device [B], out*/, void* stream);

/* excel_conf_merge_ragged replaces _refine_cams2 :94-96 for both groups, :146-152 and :154-156: planes = 2 (smax + 1) pitched planes per
 * image on the half plan (PAR's output: groups of nchan[b] = k_b + 1 planes back to back).  Per group: bilinear to the sizes of
 * (dst_table, dst_info) (align_corners=False), arg-max with the first maximum winning, key lookup (0 -> 0, c -> cls_idx[b, c-1] + 1; no
 * cls_idx: c) - the bits of excel_bilinear_resize + excel_argmax_label.  Then lab = lab_h; lab_h == 0 -> ignore_index; lab_h == 0 and
 * lab_l == 0 -> 0.  img_box (optional, device int32 [B,4] = y0, y1, x0, x1, non-negative): pixels outside [y0, y1) x [x0, x1) get
 * ignore_index.  labels_u8: tight, image b at loff_b of the destination plan. */
int excel_conf_merge_ragged(const float* planes, const int32_t* nchan, const int32_t* cls_idx /*device [B,smax] or NULL*/,
                            const int32_t* half_table, const excel_ragged_info* half_info, const int32_t* dst_table,
                            const excel_ragged_info* dst_info, int smax, const int32_t* img_box /*device [B,4] or NULL*/, int ignore_index,
                            uint8_t* labels_u8, void* stream);

/* excel_dcrf_inference for a GROUP of images of a ragged batch in one chain of launches (lattice build, normalisers, mean-field steps
 * run once for the group, not once per image): what tools/infer_seg_voc.py:103-174 (crf_proc), tools/infer_seg_coco.py:144-145 and
 * utils/dcrf.py:42-68 do per image.  (table, info) = the excel_ragged_plan of the group (see "ragged batches" below).
 *   hwc     the decoded uint8 [H_b,W_b,3] images back to back (image b at byte 3 * loff_b)
 *   unary   tight [C, H_b, W_b] per image, image b at element C * loff_b: probabilities (unary_is_energy = 0) or energies (1); the
 *           layout excel_seg_softmax_resize_ragged writes
 *   labels_u8 (optional) tight arg-max of Q over the classes, image b at loff_b, first maximum (excel_argmax_label's rule; C <= 256)
 *   q_out     (optional) the marginals, tight [C, H_b, W_b] per image at C * loff_b
 * Every image gets the bits excel_dcrf_inference (+ excel_argmax_label) gives it alone, whatever else is in the group: the image index
 * is part of every lattice key, so no lattice point is shared and no blur neighbour crosses an image, and the splat sums in fixed point.
 * Refused: B <= 0 or B > 32767, null pointers, neither output, and a group of more than 2^30 / 6 pixels (vertex indices are 32-bit).
 * The workspace depends on the group's pixel count alone; for one image it is exactly excel_dcrf_workspace_bytes(H, W, C).  Callers
 * with a memory budget split a batch into consecutive groups (excel_amd.ops.dcrf_groups); the results do not depend on the split.
 * workspace 8-byte aligned; hwc, unary, labels_u8 and q_out are slices of the batch's tensors: element alignment (1 / 4 bytes). */
int excel_dcrf_ragged_workspace_bytes(long long total_label_pix, int C, size_t* bytes /*host, out*/);
int excel_dcrf_inference_ragged(const uint8_t* hwc, const float* unary, int unary_is_energy, const int32_t* table,
                                const excel_ragged_info* info, int C, int iters, float pos_w, float pos_xy_std, float bi_w,
                                float bi_xy_std, float bi_rgb_std, uint8_t* labels_u8, float* q_out, void* workspace, void* stream);

/* The DenseCRF stage of tools/infer_lam.py:179-237 (crf_proc) for a GROUP of LAMs of a ragged batch, in one chain of launches and on the
 * step's cams where they lie: a LAM has k_b + 1 planes and k_b differs per image, so every image runs the mean field over its OWN
 * number of classes.  (table, info) = the excel_ragged_plan of the group.
 *   hwc        the decoded uint8 [H_b,W_b,3] images back to back (image b at byte 3 * loff_b)
 *   cams       Cmax PITCHED planes per image (image b at element Cmax * poff_b, rows of Wp_b floats: the excel_cam_upsample_bkg_ragged
 *              layout, i.e. the pipeline's step cams).  Probabilities: the unary is -log(clip(p, 1e-5, 1)) (utils/dcrf.py
 *              unary_from_softmax; :221 passes the LAM as the probability map).  Only planes c < nchan[b] and columns x < W_b are read
 *              (the rest of a step buffer is uninitialised).
 *   nchan      device int32 [B]: image b runs softmax, splat, blur, slice and arg-max over its first nchan[b] planes, 1 <= nchan[b] <= Cmax
 *   nchan_host host int32 [B], the same values: they size the value rows (one stride per group, Cg = max nchan_host) and are validated
 *              (EXCEL_ERR_ARG outside 1..Cmax).  The kernels clamp the device values to 1..Cg, so a device array that disagrees
 *              cannot make them read or write out of bounds.
 *   cls_idx    device int32 [B, smax] or NULL (then Cmax <= smax + 1 is not required)
 *   labels_u8  (optional) tight, image b at loff_b: the first-maximum arg-max of the final Q mapped like excel_argmax_label_ragged maps
 *              it: channel 0 -> 0, channel c -> cls_idx[b, c-1] + 1 (:225-226 keys = pad(keys_gt + 1, (1, 0)); keys[argmax]); with
 *              cls_idx == NULL the raw channel
 *   q_out      (optional) the marginals in the layout of cams; only planes < nchan[b] and columns < W_b are written
 * Every image gets, BIT FOR BIT, the Q and labels excel_dcrf_inference gives it alone with C = nchan[b] on its tight planes, whatever
 * its batch neighbours and their class counts: the image index is part of every lattice key, the splat sums in fixed point, and the
 * per-class arithmetic and the order of the softmax sum are those of the uniform entries (which keep their own code path and bits).
 * Rows of pixels and lattice points have the stride Cg; a work item (point, k) with k >= the count of the point's image returns: an
 * image with fewer classes costs memory and idle lanes, not memory traffic.  Workspace = that of excel_dcrf_ragged_workspace_bytes at
 * C = Cg plus one int32 per lattice vertex (9 per pixel, each array rounded up to 256 bytes): the class count of every lattice point.
 * Refused: null pointers, neither output, B outside 1..32767, non-positive standard deviations, a group of more than 2^30 / 6 pixels.
 * No host synchronisation; everything on `stream`.  workspace 8-byte aligned. */
int excel_dcrf_lam_ragged_workspace_bytes(const int32_t* hw /*host [B,2]*/, const int32_t* nchan /*host [B]*/, int B, size_t* bytes /*host, out*/);
int excel_dcrf_lam_ragged(const uint8_t* hwc, const float* cams, const int32_t* nchan /*device [B]*/, const int32_t* nchan_host /*host [B]*/,
                          const int32_t* cls_idx /*device [B,smax] or NULL*/, const int32_t* table, const excel_ragged_info* info, int smax,
                          int Cmax, int iters, float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std,
                          uint8_t* labels_u8, float* q_out, void* workspace, void* stream);

/* ------------------------------------------------------------------ CAM overlay images (camviz.hip)
 * tools/infer_lam.py:97-111 (--save_cam): the jet-coloured CAM blended over the photo, per image at its own size, for a ragged batch
 * in one launch.  For every pixel and channel ch
 *   out = (uint8) trunc(tables[0][idx][ch] + tables[1][ch][v])        (one float64 add)
 * where v = the decoded image byte (hwc, tight, image b at byte 3 * loff_b), idx = matplotlib jet's index of the cam value x (float32):
 * floor(x * 256), x == 1 -> 255, x < 0 -> 0 (under), x > 1 -> 255 (over), NaN -> the bad colour (RGB 0, contributes 0.0).
 *   tables (device float64 [2][768]): [0] = alpha * jet_lut * 255 as [256][3]; [1] = (1 - alpha) * denormalize_img(normalize_img(v))
 *   as [3][256] - both pre-scaled on the host exactly as the reference computes them (excel_amd/utils/imutils.py).
 *   mode EXCEL_CAM_OVERLAY_MAX:       x = max over the planes 1..k_b (NaN propagates, torch.max); one tight [H_b,W_b,3] overlay per
 *                                     image at byte 3 * loff_b; an image with k_b = 0 is not written.
 *   mode EXCEL_CAM_OVERLAY_PER_CLASS: x = plane 1 + c for c < k_b; overlay c of image b at byte out_off[b] + 3 * c * H_b * W_b.
 * cams = Cmax pitched planes per image (the excel_cam_upsample_bkg_ragged layout; plane 0 = background, never read).  Only x < W_b and
 * planes 1..k_b are read (pad columns and unused planes of the pipeline's step buffers may hold anything).
 * ncls (device int32 [B]) = k_b, which the caller guarantees to be <= Cmax - 1; out_off (device int64 [B]) is needed in per-class mode.
 * excel_cam_overlay is the same for ONE image whose cams are tight [1+k, H, W] (the per-image path's normed maps): out at byte 0.
 * tables (doubles) and out_off (int64) 8-byte aligned; hwc and out at any byte. */
#define EXCEL_CAM_OVERLAY_MAX 0
#define EXCEL_CAM_OVERLAY_PER_CLASS 1
int excel_cam_overlay_ragged(const uint8_t* hwc, const float* cams, int Cmax, const int32_t* ncls, const int64_t* out_off,
                             const int32_t* table, const excel_ragged_info* info, int mode, const double* tables, uint8_t* out, void* stream);
int excel_cam_overlay(const uint8_t* hwc, const float* cams, int k, int H, int W, int mode, const double* tables, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ training-progress panels (trainviz.hip)
 * The image grids scripts/train_voc.py:233-246 (scripts/train_coco.py:229-242) renders every --log_iters iterations, for one training
 * batch in one launch.  Panel k (EXCEL_TRAIN_PANEL_*, the order of the reference's add_image calls) is a tight uint8 [Hg,Wg,3] RGB grid in
 * torchvision.utils.make_grid's default layout (utils/tbutils.py:46, :59, :92): xmaps = min(nrow, B), ymaps = ceil(B / xmaps), a cell is
 * (h+2) x (w+2), the grid (h+2)*ymaps + 2 by (w+2)*xmaps + 2, image k at row (k / xmaps)*(h+2) + 2, column (k % xmaps)*(w+2) + 2, everything
 * else 0 (the cells past B too); B == 1 is the bare image.  Every byte of a requested panel is written.
 *   IMG1      utils/tbutils.py:28-33 (denormalize_img): (uint8) (((x * std_c) + mean_c) * 255) in float32, truncated, clamped to [0, 255]
 *             (the reference's conversion is undefined outside); img f32 [B,3,S,S], mean / std HOST float[3] (0.485.. / 0.229..)
 *   CAM1      utils/tbutils.py:39, :52-58: attr f32 [B,P,F] read as [B,F,g,g] (P == g*g), every class plane sampled bilinearly
 *             (align_corners = False) at the pixel, times cls_label[b,f] (f32 [B,F]), max over f (NaN propagates, torch.max), jet index
 *             as in excel_cam_overlay, out = (uint8) trunc(jet[idx][ch] + 0.5 * img1 byte) in float64; jet (device float64 [256][3]) =
 *             0.5 * (jet_lut * 255), pre-scaled on the host as the reference computes it; 8-byte aligned
 *   PSEU_AFF, SEG_GT, SEG_PRED   utils/tbutils.py:88-93: uint8 [B,S,S] label maps through `palette` (device uint8 [256][3])
 *   PSEU_MID  the same for a uint8 [B,g,g] label map: a grid of g x g cells
 * excel_train_panels_plan (a HOST function: no device work) -> out[3*k .. 3*k+2] = (Hg, Wg, byte offset) of panel k (0, 0, 0 when bit k of
 * panel_mask is clear), out[3 * EXCEL_TRAIN_PANELS] = total bytes; the requested panels follow each other tightly in panel order.
 * excel_train_panels renders them into `out` (out_bytes >= the plan's total).  Inputs of panels that are not requested may be NULL; a
 * requested panel without its input, a size at or above 2^31 (3*B*S*S, B*P*F, the total bytes) and P != g*g are argument errors. */
#define EXCEL_TRAIN_PANELS 6
#define EXCEL_TRAIN_PANEL_IMG1 0
#define EXCEL_TRAIN_PANEL_CAM1 1
#define EXCEL_TRAIN_PANEL_PSEU_AFF 2
#define EXCEL_TRAIN_PANEL_PSEU_MID 3
#define EXCEL_TRAIN_PANEL_SEG_GT 4
#define EXCEL_TRAIN_PANEL_SEG_PRED 5
#define EXCEL_TRAIN_PANELS_PLAN_INTS (3 * EXCEL_TRAIN_PANELS + 1)
int excel_train_panels_plan(int B, int nrow, int S, int g, int panel_mask, int64_t* out /*host*/);
int excel_train_panels(const float* img, const float* attr, const float* cls_label, const uint8_t* pseu_aff, const uint8_t* pseu_mid,
                       const uint8_t* seg_gt, const uint8_t* seg_pred, int B, int F, int P, int g, int S, int nrow, int panel_mask,
                       const float* mean /*host*/, const float* std /*host*/, const double* jet, const uint8_t* palette, uint8_t* out,
                       size_t out_bytes, void* stream);

/* ------------------------------------------------------------------ label PNG files (png.hip)
 * The label image the reference saves per sample (tools/infer_lam.py:95, commented out there; tools/training_free_attr.py:225, live), for a
 * ragged batch: labels = the tight uint8 label maps excel_argmax_label_ragged writes (image b at loff_b) -> one COMPLETE palette PNG file
 * per image in `arena`, so that only file bytes cross to the host and nothing there parses or patches them.
 *   file    signature; IHDR (W_b x H_b, 8 bit, colour type 3, no interlace); PLTE = the 256 RGB entries of `palette` (device, 768 bytes);
 *           one IDAT; IEND - every chunk with its CRC-32.
 *   IDAT    a zlib stream (0x78 0x01): ONE final deflate block with the fixed Huffman table (BTYPE = 01) that holds literals and matches
 *           at distance 1 only (lengths 3..258; a run of L equal bytes = literal, (L-1)/258 matches of 258, then the remainder as one
 *           match, or as literals when it is below 3), scanlines with filter type 0 coded independently and joined at bit granularity,
 *           then the Adler-32 of the unfiltered scanlines.
 *   layout  image b's file starts at the sum of excel_png_labels_bound_bytes(H_i, W_i) over i < b; out_table (device int64 [B][2]) receives
 *           (offset, size) of every file.  The bytes are a pure function of the image's labels and the palette (no dependence on the
 *           batch, the stream or the launch order); arena bytes outside the files are zero.
 * excel_png_labels_bound_bytes = ceil(9 (W + 1) H / 8) + 880, rounded up to 16: every byte as a 9-bit literal is the worst case.
 * hw (HOST int32 [B][2]) = the (H_b, W_b) the plan was built from: the sizes are checked against arena_bytes / workspace_bytes before any
 * launch.  workspace: excel_png_labels_workspace_bytes(B, max H_b) bytes, 8-byte aligned; arena 4-byte aligned (it is cleared and the
 * codes are OR-ed in with 32-bit atomics).  Limits: 9 (W_b + 1) H_b < 2^32 - 10, B <= 65535. */
size_t excel_png_labels_bound_bytes(int H, int W);
size_t excel_png_labels_workspace_bytes(int B, int max_h);
int excel_png_encode_labels_ragged(const uint8_t* labels, const int32_t* table, const excel_ragged_info* info, const int32_t* hw /*host*/,
                                   const uint8_t* palette, uint8_t* arena, size_t arena_bytes, int64_t* out_table, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ CAM overlay JPEG files (jpeg.hip)
 * The overlay images the reference saves per sample (tools/infer_lam.py:104,111: imageio.imsave of a uint8 [H,W,3] array to a .jpg, which
 * is Pillow at quality 75), for a ragged batch: rgb = the flat uint8 buffer excel_cam_overlay_ragged writes (tight [H_i,W_i,3] images,
 * image i at byte off_i; any offsets, odd ones included) -> one COMPLETE baseline JFIF file per image in `arena`, so that only file bytes
 * cross to the host.  The bytes are the ones PIL.Image.fromarray(rgb_i).save(f, format="JPEG", quality=quality) writes (Pillow 12 over
 * libjpeg-turbo 3): every stage is libjpeg's integer arithmetic.
 *   file    SOI; APP0 (JFIF 1.01, no units, 1 x 1); two DQT (the Annex K tables at libjpeg's quality scaling, zig-zag order); SOF0 (8 bit,
 *           Y 2x2 with table 0, Cb / Cr 1x1 with table 1); four DHT (DC0, AC0, DC1, AC1: the Annex K tables); one interleaved SOS; the
 *           entropy-coded segment (no restart markers, 0x00 behind every 0xFF, last byte filled with 1-bits); EOI.  623 bytes in front of
 *           the segment, 2 behind it.
 *   pixels  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb / Cr likewise with offset (128 << 16) + 32767; chroma = the mean of 2 x 2
 *           converted pixels with bias 1, 2, 1, 2 ... along a row; level shift 128; "islow" DCT; division by 8 q rounding half away from
 *           zero.  Padding as libjpeg pads (see jpeg.hip): replicated edges, and luma blocks wholly outside the image repeat the DC value
 *           of the block in front of them.
 *   layout  the files lie back to back from arena[0] in the order of the images; out_table (device int64 [n][2]) receives (offset, size)
 *           of every file.  A file that would end behind arena_bytes gets size -1 and none of its bytes is written (so does every file
 *           behind it: the offsets are the running sum of the sizes); arena bytes outside the files are never touched.  The bytes of a
 *           file are a pure function of its pixels and the quality (no dependence on the batch, the stream or the launch order).
 * excel_jpeg_rgb_arena_bytes = the sum of 625 + 3 H_i W_i: the raw size plus the header, which a quality-75 file of an overlay is expected
 * (not proven) to stay below - hence the -1; tiny images do exceed it (the file of a 1 x 1 image has 631 bytes, its bound 628).  excel_jpeg_rgb_workspace_bytes: coefficients, block start bits and the unstuffed stream at
 * its worst case of 208 bytes per 8 x 8 block.  Both return 0 for sizes out of range.
 * off (HOST int64 [n]) and hw (HOST int32 [n][2] = H_i, W_i) are read before the call returns (they travel as kernel arguments).
 * workspace 16-byte aligned, out_table 8-byte aligned.  Limits: 1 <= n <= 65535, 1 <= H_i, W_i <= 65535, 3 H_i W_i < 2^31, 1 <= quality <= 100. */
size_t excel_jpeg_rgb_arena_bytes(const int32_t* hw /*host*/, int n);
size_t excel_jpeg_rgb_workspace_bytes(const int32_t* hw /*host*/, int n);
int excel_jpeg_encode_rgb_ragged(const uint8_t* rgb, const int64_t* off /*host*/, const int32_t* hw /*host*/, int n, int quality, uint8_t* arena,
                                 size_t arena_bytes, int64_t* out_table, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ training augmentation (aug.hip)
 * VOC12ClsDataset(aug=True)'s transform (datasets/voc.py:110-117 over datasets/transforms.py) for a ragged batch of decoded uint8
 * images and label maps on the device, in the reference's order:
 *   random_scaling (:25-50)  image -> (int(r*w), int(r*h)) with Pillow BILINEAR, label with Pillow NEAREST (both bit-identical)
 *   random_fliplr  (:74-87)
 *   random_crop    (:118-176) pad to max(S,h') x max(S,w') (image 0, label 255), place the image at (H_pad, W_pad), choose the crop
 *                  among the 10 candidate origins by the cat_max_ratio = 0.75 rule, img_box in padded coordinates (the reference's
 *                  img_box[1] = min(H_end, H_pad + h'), img_box[3] likewise)
 *   normalize_img  (:7-14) + HWC->CHW, with excel_normalize_img_u8's arithmetic: (float)(((double)v - mean) / std).
 * The random draws are made by the caller (host) and passed in `params`; the crop choice is made on the device.
 * Inputs: hwc = the uint8 [h_b,w_b,3] images back to back, labels = the uint8 [h_b,w_b] maps back to back (the tight layout of the
 * ragged batches above: image b at byte 3 * loff_b, label b at loff_b).
 * Outputs: img [B,3,S,S] f32, label [B,S,S] u8, img_box [B,4] int32. */
#define EXCEL_AUG_CANDIDATES 10
typedef struct {
    double ratio;                                  /* random_scaling's ratio, in [1/8, 8] */
    int32_t flip;                                  /* 1: random_fliplr flipped (random() > 0.5) */
    int32_t h_pad, w_pad;                          /* placement in the padded image: [0, max(S,h') - h'] x [0, max(S,w') - w'] */
    int32_t cand_h[EXCEL_AUG_CANDIDATES];          /* candidate crop origins, all 10 drawn: [0, max(S,h') - S] */
    int32_t cand_w[EXCEL_AUG_CANDIDATES];          /*                                       [0, max(S,w') - S] */
} excel_aug_params;
typedef struct {
    int32_t B, S, max_h, max_w2;                   /* batch, crop size, largest source height, largest rescaled width */
    int64_t table_ints;                            /* int32 entries of the table */
    int64_t workspace_bytes;                       /* device workspace excel_train_augment needs */
    int64_t total_label_pix;                       /* sum h_b * w_b */
} excel_train_aug_info;
/* HOST function (no device work): checks every size and parameter and builds the int32 table the kernels read - per image a
 * record of EXCEL_AUG_REC ints, then Pillow's BILINEAR coefficient tables (per output index: first source index, tap count,
 * kx (resp. ky) fixed-point weights; double arithmetic, contraction off) and NEAREST index tables of both axes.  Record fields:
 *   0 h, 1 w, 2 h', 3 w', 4 loff, 5 workspace byte offset of the horizontal pass' output, 6 x-coefficient offset, 7 kx (0: no
 *   horizontal pass, w' == w), 8 y-coefficient offset, 9 ky (0: no vertical pass), 10 x-index offset, 11 y-index offset, 12 flip,
 *   13 h_pad, 14 w_pad, 15 max(S,h'), 16 max(S,w'), 18..27 cand_h, 28..37 cand_w.
 * With table == NULL only `info` is filled.  The caller copies the table (info->table_ints int32) to the device. */
#define EXCEL_AUG_REC 40
int excel_train_aug_plan(const int32_t* hw /*host [B,2]*/, const excel_aug_params* params /*host [B]*/, int B, int S,
                         excel_train_aug_info* info /*host*/, int32_t* table /*host or NULL*/);
size_t excel_train_augment_workspace_bytes(const excel_train_aug_info* info);
/* Four launches on `stream`, no host synchronisation: label histograms of the 10 candidate windows through the NEAREST tables,
 * the crop choice, the horizontal BILINEAR pass restricted to the chosen crop's columns and the source rows its vertical taps read,
 * and the vertical pass fused with flip, pad, crop, normalisation, the CHW store and the label crop.  mean3 / std3
 * are host arrays. */
int excel_train_augment(const uint8_t* hwc, const uint8_t* labels, const int32_t* table, const excel_train_aug_info* info,
                        const double* mean3 /*host*/, const double* std3 /*host*/, float* img, uint8_t* label, int32_t* img_box,
                        void* workspace, void* stream);
/* CocoClsDataset(aug=True)'s transform (datasets/coco.py:112-142): the same steps on images that carry no label map.  With label=None
 * get_random_cropbox returns its first draw (datasets/transforms.py:141-146), so the crop is candidate 0 of every record (no
 * cat_max_ratio rule) and there is no label output; img_box as above (padded coordinates).  Same table and info (excel_train_aug_plan)
 * and workspace (excel_train_augment_workspace_bytes) as excel_train_augment.  Three launches on `stream`, no host synchronisation:
 * the crop origin and img_box, the horizontal pass, the vertical pass fused with flip, pad, crop, normalisation and the CHW store.
 * Outputs: img [B,3,S,S] f32, img_box [B,4] int32. */
int excel_train_augment_image(const uint8_t* hwc, const int32_t* table, const excel_train_aug_info* info, const double* mean3 /*host*/,
                              const double* std3 /*host*/, float* img, int32_t* img_box, void* workspace, void* stream);

/* ------------------------------------------------------------------ one-time / auxiliary */

/* attr_aggregate (model/load_attr.py:86-119): text [T,C] (F fg rows first), bank [C,K] -> text_attr [C,T], columns unit-norm.
 * topK as in the reference (0.9): the lowest int((1-topK)*K) logits per fg row are dropped before the softmax. */
int excel_attr_aggregate(const float* text, const float* bank, int F, int T, int C, int K, double topK, float* out, void* stream);

/* F.interpolate(mode='bilinear', align_corners=0|1) on `planes` images of h x w -> H x W
 * (tools/infer_lam.py:74 input resize; utils/camutils.py:41,54 multi-scale CAM resize; utils/PAR.py:67). */
int excel_bilinear_resize(const float* in, float* out, long long planes, int h, int w, int H, int W, int align_corners, void* stream);

/* positional_embedding [1+side^2, D] -> [1+g^2, D] (clip/clip_surgery_model.py:407-414 and :426-435). */
int excel_pos_embed_resize(const float* pos, int side, int g, int D, float* out, void* stream);

/* flip-TTA fuse of cure_attr_map_flip (utils/camutils.py:21-26): attr [2B,P,F] -> out [B,P,F]. */
int excel_flip_max_normalize(const float* attr, float* out, int B, int g, int F, void* stream);

/* multi-scale LAM fuse (utils/camutils.py:41-61, multi_scale_lam2 in its evident intent): for one scale, maps [2B,P,F]
 * (second half from horizontally flipped inputs) are bilinearly resized (align_corners=False) to (H,W), flip-maxed and
 * accumulated into acc [B,F,H,W] (init=1: overwrite).  excel_plane_minmax_normalize then applies
 * lam -= min_hw; lam /= max_hw + 1e-5 per (b,f) plane. */
int excel_lam_scale_accumulate(const float* maps, float* acc, int B, int g, int F, int H, int W, int init, void* stream);
int excel_plane_minmax_normalize(float* lam, long long planes, long long HW, void* stream);

/* flip and multi-scale LAM fuse at the patch grid (test-time augmentation of the training-free regime, utils/camutils.py:8-63): the step
 * between the patch-text CAM and the random walk.  maps[s] (device) = the attribute maps of scale s exactly as the model returns them,
 * token-major [flip ? 2B : B, g[s]^2, F]; with flip, image B + b comes from the mirrored input of image b.  For every image b, class f:
 *   r_s = bilinear resize (align_corners = 0, excel_bilinear_resize's arithmetic) of the g[s] x g[s] plane to g_out x g_out
 *   v_s = flip ? max(r_s[b], mirror_x(r_s[B + b])) : r_s[b]
 *   acc = v_0 + v_1 + ... in the order given ;  lam = acc - min(acc) ;  out = lam / (max(lam) + 1e-5)      (min, max over the plane)
 * out [B, g_out^2, F] is the layout excel_refine_cams_with_aff and excel_scoremap_box_mask read.
 * Bits: for finite inputs and flip = 1 the result equals excel_lam_scale_accumulate per scale (init at s = 0) followed by
 * excel_plane_minmax_normalize and a permute to [B,P,F]; with ns = 1 and g[0] == g_out that is also excel_flip_max_normalize.
 * Non-finite values: if a value that a bilinear tap reads for plane (b, f) (every value of the plane while g[s] <= 2 g_out; a zero
 * weight still reads) is NaN or +-inf, out[b, :, f] is NaN as a whole and no other plane changes - the overflow guard's
 * excel_nonfinite_count over `out` then flags the image (max alone would drop a NaN of one half).
 * Limits: 1 <= ns <= 8, 1 <= g[s], g_out <= 48, B, F >= 1.  Two launches on `stream`, no workspace (out holds the sums in between),
 * no host synchronisation; maps and g are host arrays read before the call returns. */
int excel_lam_tta_fuse(const float* const* maps /*host [ns]*/, const int32_t* g /*host [ns]*/, int ns, int flip, int B, int F, int g_out,
                       float* out /*[B, g_out*g_out, F]*/, void* stream);

/* ------------------------------------------------------------------ live per-kernel timing (bench.py) */

/* When enabled, every kernel launch is bracketed by hipEvents on its launch stream, grouped by category.
 * excel_prof_collect synchronises, fills ms[c] (summed elapsed), launches[c], work[c] (algorithmic FLOPs for the GEMM
 * categories, 0 otherwise) for c < excel_prof_num_categories(), and clears the log. */
int excel_prof_enable(int on);
int excel_prof_set_mask(unsigned long long category_mask);   /* bit c: bracket category c (default all) */
int excel_prof_set_sampling(int every);                      /* bracket every n-th launch of a category (default 1) */
int excel_prof_num_categories(void);
const char* excel_prof_category_name(int cat);
int excel_prof_collect(double* ms /*host*/, long long* launches /*host*/, double* work /*host*/);

#ifdef __cplusplus
}
#endif
#endif
