// "w4" bf16x3 GEMM: the big tiles of gemm_bf16x3.hip on FOUR waves, one per SIMD, with a hand-placed instruction stream.
//
//   C[M,N] (fp32 or split) = act(A_split[M,K] . W_split[N,K]^T + bias) + residual          (same operands, layouts and epilogue semantics)
//
// Why a second kernel (rounds 3 and 4 measured this, EXPERIMENTS.md): the 8-wave kernel's k-loop takes 1.49x its own MFMA stream.  Its
// waves own 160 x 64 outputs - 28 fragment reads per 120 MFMAs - and all eight of them stop at a __syncthreads() every 32 k, read
// their B fragments and only then restart the matrix pipe.  Here a wave owns 16 NT_M x 128 outputs (NT_M = 10: 160 x 128):
//   * 36 ds_read_b128 per 240 MFMAs (0.15 instead of 0.23 LDS fragment bytes per MFMA: under the socket power cap every LDS byte
//     is clock), 320 accumulator registers = 256 AGPRs (row tiles 0-7) + 64 VGPRs (the two tail row tiles) of the 512-register budget
//     of a one-wave-per-SIMD kernel;
//   * the compiler only allocates registers: every instruction of the k-loop is an `asm volatile` statement (MFMA with an explicit
//     accumulator register class, ds_read_b128 with immediate offsets, counted s_waitcnt) or an LDS-DMA builtin between them, in
//     program order - hipcc would otherwise shuttle accumulator tiles between the two register files (340 v_accvgpr moves per
//     k-step, round 3) and drain the DMA queue in front of every LDS read it can see;
//   * ONE barrier per 32-k step, placed in front of the last two row tiles, and nothing waits behind it: by then every A fragment of
//     the step has been read (two tiles ahead, into a 4-deep register ring), so the barrier both publishes the next stage (each wave
//     waited for its own DMA pieces) and frees the current one.  The last two row tiles run column-pair-major, so the B fragments of a
//     column pair are dead after 12 MFMAs and are re-loaded from the NEXT stage right there; the next step's first two A tiles are
//     fetched at the head of this tail.  The matrix pipe never waits for an LDS round trip behind a barrier: by in-kernel stamps a step
//     of 240 MFMAs takes 4 300 cycles for 3 840 of matrix-pipe work (the bare one-wave MFMA stream: 4 080);
//   * MFMAs on one accumulator are 8 apart (pass-major over the 8 column tiles of a row tile; 4 apart in the tail): a single wave
//     has no partner to fill a dependent-accumulator wait (the first attempt, round 3: +44 % on the bare MFMA stream);
//   * the LDS-DMA pieces of the next stage (NT_M + 8 per wave) go out one at a time between MFMAs of the early row tiles, through a
//     buffer descriptor: loop-invariant 32-bit lane offsets + one scalar k offset (64-bit lane pointers spilled in round 3);
//   * the epilogue stores straight from the registers: the MFMA gets the weight fragment as srcA (the tile comes out transposed: a lane
//     holds columns of ONE row) and the weight rows are read in a permuted order with a swizzle of their own, so a lane owns 8
//     consecutive columns per tile pair (no LDS transpose, no barrier; see the epilogue).
// Instances: NT_M = 10 (320 x 256 tiles: the B = 32 layer shapes), 8 (256 x 256), 5 (160 x 256: N = 768 launches of the B = 16 shapes);
// the GEMM plan (gemm_plan.hip) picks instance vs 8-wave tile by modelled time.
// Stage layout: row = [hi 32 | lo 32] bf16 = 128 B = 8 chunks of 16 B; A rows (chunk c at slot c ^ ((row >> 1) & 7)), then the 256 B
// rows (slot c ^ swz_b(row)); two stages.
#include <stdlib.h>
#include <type_traits>
#include "common.h"
#include "excel_internal.h"


namespace EXCEL_SPLIT_NS {

#include "gemm_w4_body.inc"

static_assert(w4::BN == GEMM_W4_BN, "the GEMM plan's grid arithmetic (gemm_plan.hip) assumes this tile width");

// one plain __global__ function per instance (a kernel TEMPLATE launched from inside a function template lost its host-side stub)
#define W4_KERNEL(NT, DBG) __global__ __launch_bounds__(256, 1) void gemm_w4_kernel_##NT##_##DBG(GemmBfArgs p) { W4_UNIFORM_BODY(NT, DBG, 0); }
W4_KERNEL(10, 0) W4_KERNEL(8, 0) W4_KERNEL(5, 0)
__global__ __launch_bounds__(256, 1) void gemm_w4_kernel_mix(GemmBfArgs p) { W4_MIX_BODY(0); }
#ifdef EXCEL_DEV
W4_KERNEL(10, 1) W4_KERNEL(10, 2) W4_KERNEL(10, 4) W4_KERNEL(10, 8) W4_KERNEL(8, 8) W4_KERNEL(5, 8) W4_KERNEL(10, 9) W4_KERNEL(10, 10)
W4_KERNEL(10, 15) W4_KERNEL(10, 24) W4_KERNEL(10, 32) W4_KERNEL(10, 136) W4_KERNEL(10, 143) W4_KERNEL(10, 128)
#endif
#define W4_LAUNCH(NT, DBG) hipLaunchKernelGGL(gemm_w4_kernel_##NT##_##DBG, grid, dim3(256), 0, stream, p)

static void launch_w4(const GemmBfArgs& p_in, int nt_m, dim3 grid, hipStream_t stream) {
    GemmBfArgs p = p_in;
#ifdef EXCEL_DEV
    static const int stagger = getenv("EXCEL_W4_STAGGER") ? atoi(getenv("EXCEL_W4_STAGGER")) : 0;
    p.dbg = (stagger > 0 && (int)grid.x > 320) ? stagger : 0;      // multi-round launches only
    static const int dbg = getenv("EXCEL_W4_DBG") ? atoi(getenv("EXCEL_W4_DBG")) : 0;
    if (nt_m == 10) {
        switch (dbg) {
            case 1: W4_LAUNCH(10, 1); return;
            case 2: W4_LAUNCH(10, 2); return;
            case 4: W4_LAUNCH(10, 4); return;
            case 8: W4_LAUNCH(10, 8); return;
            case 9: W4_LAUNCH(10, 9); return;
            case 10: W4_LAUNCH(10, 10); return;
            case 15: W4_LAUNCH(10, 15); return;
            case 24: W4_LAUNCH(10, 24); return;
            case 32: W4_LAUNCH(10, 32); return;
            case 128: W4_LAUNCH(10, 128); return;
            case 136: W4_LAUNCH(10, 136); return;
            case 143: W4_LAUNCH(10, 143); return;
            default: break;
        }
    }
    if (dbg == 8 && nt_m == 8) { W4_LAUNCH(8, 8); return; }
    if (dbg == 8 && nt_m == 5) { W4_LAUNCH(5, 8); return; }
#endif
    if (nt_m == 10) W4_LAUNCH(10, 0);
    else if (nt_m == 8) W4_LAUNCH(8, 0);
    else W4_LAUNCH(5, 0);
}

// a GEMM_W4 plan (instance plan.nt_m) or a GEMM_W4_MIX one (two instances), three MFMAs per product
int excel_launch_gemm_w4(const GemmBfArgs& p_in, const GemmPlan& plan, hipStream_t stream) {
    if (plan.kernel == GEMM_W4_MIX) {
        GemmBfArgs p = p_in;
        p.mix_tall = plan.tall; p.mix_short = plan.shrt; p.mix_first = plan.second;     // (the kernel reads mix_first as the second instance)
        hipLaunchKernelGGL(gemm_w4_kernel_mix, dim3(plan.grid_x), dim3(256), 0, stream, p);
    } else {
        launch_w4(p_in, plan.nt_m, dim3(plan.grid_x), stream);
    }
    EXCEL_CHECK_LAUNCH("gemm_w4");
    return EXCEL_OK;
}

}  // namespace EXCEL_SPLIT_NS

