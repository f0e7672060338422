// Kernel selection of the pixel-adaptive refinement (par.hip): whether the guide is resized, which kernel writes the affinity statistics
// and in which form, which kernel runs the Jacobi steps, the grids of both launches, and how many of an image's 64 x 16 tiles take the
// 16-byte interior staging.  Pure host arithmetic on integers - no pointers into device memory, no device calls, no state - so one
// function serves excel_par_forward, excel_par_forward_ragged, the launchers of par.hip (they launch exactly what the plan names) and
// the host query of the C ABI (excel_par_plan), and can be tested without a GPU.
#include "common.h"
#include "excel_internal.h"

// The recomputing step is built for the dilation set every caller of the reference uses, [1,2,4,8,12,24] (tools/infer_lam.py:168,
// scripts/train_voc.py:112, scripts/train_coco.py:110): 6 x 8 float2 weights stay in registers (96 of 128 VGPRs), halo 24, tap
// offsets as compile-time immediates.  Any other set goes through the streamed kernel.
bool par_dil_ok(const int* dil, int ndil) {
    static const int want[6] = {1, 2, 4, 8, 12, 24};
    if (ndil != 6) return false;
    for (int i = 0; i < 6; ++i)
        if (dil[i] != want[i]) return false;
    return true;
}

ParPlan par_plan(const ParShape& s) {
    ParPlan pl = {};
    const bool dil = par_dil_ok(s.dil, s.ndil);
    // the recomputing tile kernels: 16-byte aligned planes of a pitch that is a multiple of 4 floats (any such pitch works, down to 4:
    // border tiles clamp their source columns per lane - tests/test_gpu_ops.py::test_ragged_tiny_images,
    // test_par_uniform_narrow_images), and 32-bit LDS-DMA offsets inside one image (one buffer descriptor per image and tensor)
    const long long planes = s.Cmax > 5 ? s.Cmax : 5;
    const bool fits = planes * s.max_plane * 4 < (1LL << 31);
    if (s.ragged) {
        // (every pitch of the ragged layout is a multiple of 4 floats by construction - excel_ragged_plan)
        pl.refused = s.n_iter < 1 ? PAR_REFUSE_NITER : !dil ? PAR_REFUSE_DILATIONS : !s.aligned16 ? PAR_REFUSE_ALIGN : !fits ? PAR_REFUSE_SIZE : 0;
        if (pl.refused) return pl;
    }
    // the guide of a ragged batch always goes through the align_corners=True resize (PAR.py:67): it is the identity where
    // (H_b, W_b) == (h, w), and it brings the uniform [B,3,h,w] network input into the pitched per-image layout
    pl.resize = s.ragged || s.h != s.H || s.w != s.W;
    // Affinities: either streamed as 8*ndil planes per image (EXCEL_PAR_STREAM_AFFINITIES, or a shape / dilation set the tiled kernel
    // does not take), or recomputed in every step from the guide image and 5 per-pixel statistics: bit-identical weights from a
    // tenth of the bytes (par.hip).
    const bool recompute = s.ragged || (!s.stream && s.n_iter > 0 && (s.W % 4) == 0 && s.aligned16 && dil && fits);
    // compact statistics of the standard dilation set, 16-byte aligned pitched planes: the tile kernel
    const bool tiled = recompute && (s.ragged || (s.W >= 8 && 5LL * s.H * s.W * 4 < (1LL << 31)));
    pl.stats = tiled ? PAR_STATS_TILE : (recompute ? PAR_STATS_POINT_COMPACT : PAR_STATS_POINT_PLANES);
    pl.nd = s.ndil;
    pl.step = s.n_iter == 0 ? PAR_STEP_NONE : (recompute ? PAR_STEP_RECOMPUTE : PAR_STEP_STREAM);
    const int ntx = cdiv(s.W, 64);
    // 64 x 16 tiles of 512 threads (grid.x = the tile list of a ragged batch); the pointwise kernels: 64 x 4 pixels of 256 threads
    auto grid = [&](int* g, bool tile) {
        if (s.ragged) { g[0] = s.total_tiles; g[1] = tile ? 1 : 4; g[2] = 1; }
        else { g[0] = ntx; g[1] = cdiv(s.H, tile ? 16 : 4); g[2] = s.B; }
    };
    grid(pl.stats_grid, tiled);
    pl.stats_block = tiled ? 512 : 256;
    if (pl.step != PAR_STEP_NONE) {
        grid(pl.step_grid, recompute);
        pl.step_block = recompute ? 512 : 256;
    }
    if (tiled || pl.step == PAR_STEP_RECOMPUTE) {
        // a tile whose 24-pixel halo lies inside the row on both sides is staged in 16-byte pieces, every other one in 4-byte pieces
        // with per-lane clamped columns (par_iterate_guide_kernel, par_stats_tile_kernel: `interior`)
        int nint = 0;
        for (int tx = 0; tx < ntx; ++tx) nint += (tx * 64 - PAR_HALO >= 0 && tx * 64 + 64 + PAR_HALO <= s.W) ? 1 : 0;
        pl.tiles_interior = nint * cdiv(s.H, 16);
        pl.tiles_border = (ntx - nint) * cdiv(s.H, 16);
    }
    return pl;
}
