// rvcp_tonemap.h -- the tone map + UNORM8 store of the numeric contract, shared
// by the path kernels and tonemap_kernel (rvcp_kernels.hip) and by remodulate_tonemap_kernel
// (rvcp_albedo.hip), so the stores cannot drift apart.
#pragma once

namespace rvcp {

// Tone map + UNORM8 (:498-500) by the threshold table of DESIGN.md §3.3.
__device__ __forceinline__ uint32_t gamma_u8(float c, const float *__restrict__ T) {
    const float x = (c > 0.0f) ? ((c < 1.0f) ? c : 1.0f) : 0.0f;
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = 128; step >= 1; step >>= 1)
        if (x >= T[lo + step]) lo += step;
    return lo;
}

__device__ __forceinline__ uint32_t pack_rgb8(float r, float g, float b, const float *__restrict__ T) {
    return gamma_u8(r, T) | (gamma_u8(g, T) << 8) | (gamma_u8(b, T) << 16) | 0xFF000000u;
}

}  // namespace rvcp
