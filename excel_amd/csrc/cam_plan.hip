// Kernel selection of the fused patch-text CAM (cam.hip): which instance of the similarity kernel runs for (mode, T, C), and the grids
// of the three launches (prep, similarity, finish).  Pure host arithmetic on integers - no pointers, no device calls, no state - so one
// function serves the launcher and the host query of the C ABI (excel_patch_text_cam_plan), and can be tested without a GPU.
#include "common.h"
#include "excel_internal.h"

CamPlan cam_plan(int B, int N, int C, int T, int gemm_mode) {
    CamPlan pl = {};
    pl.split = gemm_mode != 0;
    pl.G = cdiv(cdiv(N, 32), PTC_NW);                             // one 32-token tile per wave
    // column sums of squares over blocks of PTC_HB tokens x 256 columns; the last z slice splits the text bank (split modes)
    pl.prep_grid[0] = cdiv(N, PTC_HB); pl.prep_grid[1] = B; pl.prep_grid[2] = cdiv(C, 256) + 1;
    pl.sim_grid[0] = pl.G; pl.sim_grid[1] = B;
    pl.block = PTC_NW * 64;
    pl.finish_grid[0] = cdiv(N, 64); pl.finish_grid[1] = B;
    if (T > PTC_MAXCT * 32) {                                     // the class axis goes through the accumulators in chunks
        pl.kernel = CAM_WIDE;
        pl.finish_pitch = PTC_WIDE_T;
        return pl;
    }
    pl.kernel = CAM_NARROW;
    pl.finish_pitch = PTC_MAXCT * 32;
    const int ct = cdiv(T, 32);
    if (pl.split) {
        // the LDS text bank: whole 1-KB LDS-DMA pieces per split row (C % 256 == 0) of at most PTC_TLDS_ROWS x PTC_TLDS_C; its two
        // instances hold 1 / 2 class tiles, the ones that read the text from global memory 2 / 4
        pl.tlds = T <= PTC_TLDS_ROWS && C <= PTC_TLDS_C && (C % 256) == 0;
        pl.ct = pl.tlds ? (ct <= 1 ? 1 : 2) : (ct <= 2 ? 2 : 4);
    } else {
        pl.ct = ct <= 1 ? 1 : (ct == 2 ? 2 : 4);
    }
    return pl;
}
