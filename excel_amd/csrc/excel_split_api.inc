// Launch interfaces of the translation units that depend on the 16-bit type of the split operand planes (gemm_bf16x3.hip, gemm_w4.hip,
// norm.hip, attn.hip, attn_strip.hip, cam.hip).  Included twice by excel_internal.h: inside namespace excel_bf16 and inside
// namespace excel_f16 - the six files are compiled once per type (build.py), everything in them lives in the matching namespace.
// Code outside the six files calls these through the SplitApi table (excel_internal.h), which lists the ones it may call.
int excel_launch_gemm_bf16x3(const GemmBfArgs& p, hipStream_t stream);
// the four-wave kernels (gemm_w4.hip; gemm_w4x2.hip, IEEE-half split type only: two MFMAs per product for fp16-valued weights) launching a
// GEMM_W4 / GEMM_W4_MIX plan of gemm_plan(); excel_launch_gemm_bf16x3 routes to them
int excel_launch_gemm_w4(const GemmBfArgs& p, const GemmPlan& plan, hipStream_t stream);
int excel_launch_gemm_w4x2(const GemmBfArgs& p, const GemmPlan& plan, hipStream_t stream);
// fp32 [R,K] -> plain 16-bit hi plane [R,K] (the two-product GEMM's compact weight operand) + the number of elements whose lo plane is
// not zero, added to *inexact (device counter; 0 <=> every value is representable in the 16-bit type)
int excel_launch_pack_hi(const float* in, void* out, long long R, int K, unsigned long long* inexact, hipStream_t st);
int excel_launch_split_bf16(const float* in, void* out, long long R, int K, hipStream_t st);
int excel_launch_vt_from_planes(const unsigned short* qkvs, unsigned short* vt, int B, int H, int N, int KP, hipStream_t st);
int excel_launch_layernorm(const float* x, const float* cls_src, int tokN, const float* w, const float* b, float* y,
                           int rows, int D, float eps, hipStream_t st, int split_out = 0, long long in_stride = 0);
int excel_launch_assemble_ln_pre(const float* patch, const float* cls_emb, const float* pos, const float* w, const float* b,
                                 float* x, int B, int tokN, int D, float eps, hipStream_t st);
int excel_launch_token_axis_normalize(const float* f, float* ss, float* out, int B, int tokN, int C, hipStream_t st);
int excel_launch_im2col(const float* img, float* col, int B, int S, int ps, hipStream_t st, int split_out = 0);
// the split-plane row pass and accumulate pass (attn.hip): qkvs = the q|k|v planes, `out` and `a_sum` are written as split tensors
int excel_launch_attn_rowpass(const unsigned short* qkvs, float* out, float* stats, int B, int H, int N, int hd, float scale,
                              const AttnPlan& plan, hipStream_t st, int flash_nq);
int excel_launch_attn_accum(const unsigned short* qkvs, const float* stats, float* a_sum, float* w_aff, float* attn_out, int B, int H,
                            int N, int NP, int hd, float scale, int surgery, float w_scale, float aff_scale, int aff_init,
                            const AttnPlan& plan, hipStream_t st, const float* ex_attn);
// `plan`: attn_plan() of this layer (excel_internal.h) - the path (strip-resident kernel up to 8 waves x 5 key tiles of 32, else the two-
// pass kernels), the row pass's score types and every grid come from it; a launcher refuses a plan that names another path (the exact-
// fp32 path has launchers of its own: excel_internal.h)
int excel_launch_attn_strip(const unsigned short* qkvs, unsigned short* a_sum, float* w_aff, float* attn_out, int B, int H, int N,
                            int KP, int hd, float scale, int surgery, float w_scale, float aff_scale, int aff_init, const float* ex_attn,
                            const AttnPlan& plan, hipStream_t st, const float* wstats);
// wstats (no default: every caller states it): the {row max in LOG2 units, 1 / row sum} of q.k that excel_launch_attn_rowpass - the split-
// plane ("bf") row pass of THIS layer, run on the SAME qkvs planes, launched earlier on the same stream - left in the type-0 slots of its
// statistics buffer ([B,H,4,N] float2).  The W sweep exponentiates against them without a running maximum: statistics of another layer,
// of the exact-fp32 row pass (natural-log units) or a strip launched in front of its row pass give silently wrong w_aff / attn_out.  May be
// null only when neither w_aff nor attn_out is requested (the launcher checks that much).
int excel_launch_cam_epilogue(float* S, float* out_full, float* out_slice, int B, int N, int T, int ldS, int F, float temp,
                              hipStream_t st);
size_t excel_patch_text_cam_ws_floats(int B, int N, int C, int T, int which);
int excel_launch_patch_text_cam(const float* x_raw, const float* text, unsigned short* text_split_out, float* sim_ws, float* part_ws,
                                float* colsq_ws, float* out_full, float* out_slice, float* feats, int B, int N, int C, int T, int F, int ldT,
                                float temp, int bf, hipStream_t st);
