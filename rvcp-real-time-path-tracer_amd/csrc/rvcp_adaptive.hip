// rvcp_adaptive.hip -- the plan step of adaptive sampling behind rvcp_spp_plan_async (DESIGN.md
// §4.18): from a frame's filtered colour, the variance left in it and its history lengths (what
// rvcp_svgf_filter_async and rvcp_svgf_accumulate_async hand out) to the next frame's per-pixel
// sample counts, the map rvcp_render_spp_map_async traces through.  The reference has no
// counterpart: its shader gives every pixel the same SPP (ray_tracer_games101_branch.comp:8).
//
// Two kernels, one lane per pixel each:
//   priority_kernel   the pixel's priority q in 0..2^20: its relative variance per accumulated
//     frame, v / (l^2 + epsilon) / n, cut off at weight_cap and scaled to an integer; 0 for a pixel
//     that asks for nothing (not filterable, a non-finite input, v not > 0, n = 0: §4.15's rule).
//     The block's sum of q goes to sums[0] with one 64-bit integer atomic.
//   share_kernel      s = spp_min + min(E q / S, spp_max - spp_min) in unsigned 64-bit integers,
//     S = sums[0] and E the budget above spp_min for every pixel (from the host); with S = 0 every
//     pixel gets min(spp_min + E / n_pixels, spp_max).  The block's sum of s goes to sums[1].
// Both sums are integer sums, so neither depends on the order of addition, and sum(s) <= spp_min
// n_pixels + E holds for any input (each quotient is rounded down); what the spp_max clamp cuts
// off is not handed to other pixels.
//
// Numeric contract: float32, every operation rounded once in the order written (no fma, IEEE
// division: the flags of the Makefile), so tests/adaptive_ref.py, the numpy restatement,
// reproduces every word of the map.
#include <hip/hip_runtime.h>

#include "rvcp_post.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWaveLanes = 64;

// the block's sum of one 32-bit value per lane (each at most 2^20: no carry out of 32 bits),
// added to *dst with one atomic; every lane of the block arrives
__device__ __forceinline__ void block_add(uint32_t v, unsigned long long *dst)
{
    __shared__ uint32_t block_sum;
    if (threadIdx.x == 0) block_sum = 0;
    __syncthreads();
    for (int o = kWaveLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & (kWaveLanes - 1u)) == 0 && v) atomicAdd(&block_sum, v);
    __syncthreads();
    if (threadIdx.x == 0 && block_sum) atomicAdd(dst, (unsigned long long)block_sum);
}

__global__ __launch_bounds__(kBlock) void priority_kernel(
    const float *__restrict__ var, const float *__restrict__ lin, const uint32_t *__restrict__ len,
    const uint32_t *__restrict__ gw, uint32_t n_pixels, float weight_cap, float epsilon,
    uint32_t *__restrict__ q_out, unsigned long long *__restrict__ sums)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t q = 0;
    if (i < n_pixels) {
        const size_t p = i;
        const float v = var[p];
        const rvcp::v3 c = rvcp::load3(lin, p);
        const uint32_t n = len ? len[p] : 1u;
        // gw: the texels as words (face at word 3, material at word 7 of 8)
        const bool asks = rvcp::filterable_w(gw[8 * p + 3], gw[8 * p + 7]) && rvcp::finite1(v) &&
                          rvcp::finite3(c.x, c.y, c.z) && v > 0.0f && n != 0u;
        if (asks) {
            const float l = rvcp::lum(c);
            const float r = v / (l * l + epsilon);
            const float w = r / (float)n;
            const float t = (w < weight_cap ? w : weight_cap) / weight_cap;
            q = (uint32_t)(t * 1048576.0f);
        }
        q_out[p] = q;
    }
    block_add(q, &sums[0]);
}

__global__ __launch_bounds__(kBlock) void share_kernel(
    const uint32_t *__restrict__ q_in, uint32_t n_pixels, uint32_t spp_min, uint32_t spp_max,
    unsigned long long extra, unsigned long long *sums, uint32_t *__restrict__ map_out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long S = sums[0];       // (priority_kernel's, complete: stream order)
    uint32_t s = 0;
    if (i < n_pixels) {
        const unsigned long long room = spp_max - spp_min;
        if (S > 0ull) {
            const unsigned long long share = (extra * (unsigned long long)q_in[i]) / S;
            s = spp_min + (uint32_t)(share < room ? share : room);
        } else {
            const unsigned long long even = (unsigned long long)spp_min + extra / n_pixels;
            s = (uint32_t)(even < spp_max ? even : spp_max);
        }
        map_out[i] = s;
    }
    block_add(s, &sums[1]);
}

}  // namespace

extern "C" int rvcp_launch_spp_plan(const float *var, const float *lin, const uint32_t *len,
                                    const void *gbuffer, uint32_t n_pixels, float weight_cap,
                                    float epsilon, uint32_t spp_min, uint32_t spp_max,
                                    unsigned long long extra, uint32_t *q_plane,
                                    unsigned long long *sums, uint32_t *map_out, void *stream)
{
    const dim3 grid((n_pixels + kBlock - 1) / kBlock), block(kBlock);
    hipLaunchKernelGGL(priority_kernel, grid, block, 0, (hipStream_t)stream, var, lin, len,
                       (const uint32_t *)gbuffer, n_pixels, weight_cap, epsilon, q_plane, sums);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(share_kernel, grid, block, 0, (hipStream_t)stream, q_plane, n_pixels,
                       spp_min, spp_max, extra, sums, map_out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// a uniform map (the chain's first frame): n_pixels words of `value`
namespace {
__global__ __launch_bounds__(kBlock) void fill_map_kernel(uint32_t *__restrict__ map,
                                                          uint32_t n_pixels, uint32_t value)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n_pixels) map[i] = value;
}
}  // namespace

extern "C" int rvcp_launch_fill_map(uint32_t *map, uint32_t n_pixels, uint32_t value, void *stream)
{
    hipLaunchKernelGGL(fill_map_kernel, dim3((n_pixels + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       (hipStream_t)stream, map, n_pixels, value);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
