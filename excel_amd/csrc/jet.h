// matplotlib's jet lookup as the image kernels share it (camviz.hip: CAM overlays, trainviz.hip: training-progress panels).
#pragma once
#include <hip/hip_runtime.h>

#define CAMVIZ_LUT 256
#define CAMVIZ_BAD CAMVIZ_LUT          // LDS entry 256 of the jet table: the "bad" colour (NaN), RGB 0

// matplotlib Colormap.__call__ for N = 256 and a float32 value: floor(x * 256) (exact), x == 1 -> 255, under (x < 0) -> 0,
// over (x > 1) -> 255, NaN -> the bad entry.
__device__ __forceinline__ int jet_index(float x) {
    if (isnan(x)) return CAMVIZ_BAD;
    if (x < 0.f) return 0;
    if (x >= 1.f) return CAMVIZ_LUT - 1;
    return (int)(x * 256.f);
}
