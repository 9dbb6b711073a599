// rvcp_albedo.hip -- albedo demodulation behind rvcp_demodulate_async and rvcp_remodulate_async
// (Schied et al.: "Spatiotemporal Variance-Guided Filtering", HPG 2017, section 4; DESIGN.md
// §4.12).  The reference has no counterpart (it stores the raw frame,
// ray_tracer_games101_branch.comp:497-500).
//
// Two kernels, one lane per pixel each:
//   demodulate_kernel            colour / albedo of the primary hit's material: the irradiance
//     the filters of §4.9-4.11 then average instead of the colour.  Exactly in place is legal (a
//     lane reads its own pixel only, before it writes it).
//   remodulate_tonemap_kernel    irradiance x the same albedo, stored as linear colour and / or
//     as RGBA8 through the tone map of rvcp_tonemap.h (tonemap_kernel's); it replaces the chains'
//     final tone-map launch.
// A pixel takes part when its primary ray hit a non-emissive surface whose material id lies
// inside the table; every other pixel passes through, as it passes through the filters.  The
// table holds 16 B per material: the three albedo floats as uploaded (not albedo / pi).
//
// Numeric contract: float32, one IEEE division resp. one product per channel
// (-ffp-contract=off, -fhip-fp32-correctly-rounded-divide-sqrt), so tests/albedo_ref.py, the
// numpy float32 restatement, reproduces every output bit.
#include <hip/hip_runtime.h>

#include "rvcp_post.h"
#include "rvcp_tonemap.h"

namespace {

constexpr uint32_t kBlock = 256;

// a_k > 0 and a_k < +inf: false for 0, negatives, NaN and inf
__device__ __forceinline__ bool usable(float a) { return a > 0.0f && a < __builtin_inff(); }

// The albedo of pixel i's material, or false when the pixel passes through.  gw: the texels as
// words (face at word 3, material at word 7 of 8); an id outside the table is never looked up.
__device__ __forceinline__ bool pixel_albedo(const uint32_t *__restrict__ gw, size_t i,
                                             const float4 *__restrict__ albedo,
                                             uint32_t n_materials, float4 &a) {
    const uint32_t face = gw[8 * i + 3], material = gw[8 * i + 7];
    const uint32_t m = material & ~RVCP_GBUFFER_EMISSIVE;
    if (!rvcp::filterable_w(face, material) || m >= n_materials) return false;
    a = albedo[m];
    return true;
}

// (in and out may be the same buffer: no __restrict__ on them)
__global__ __launch_bounds__(kBlock) void demodulate_kernel(
    const float *in, const uint32_t *__restrict__ gw, const float4 *__restrict__ albedo,
    uint32_t n_materials, float *out, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t p = i;
    float r = in[3 * p], g = in[3 * p + 1], b = in[3 * p + 2];
    float4 a;
    if (pixel_albedo(gw, p, albedo, n_materials, a)) {
        r = usable(a.x) ? r / a.x : 0.0f;
        g = usable(a.y) ? g / a.y : 0.0f;
        b = usable(a.z) ? b / a.z : 0.0f;
    }
    out[3 * p] = r;
    out[3 * p + 1] = g;
    out[3 * p + 2] = b;
}

// out_lin and / or out_rgba (either may be null; the threshold table is staged only for RGBA8)
__global__ __launch_bounds__(kBlock) void remodulate_tonemap_kernel(
    const float *__restrict__ in, const uint32_t *__restrict__ gw,
    const float4 *__restrict__ albedo, uint32_t n_materials, const float *__restrict__ gamma_t,
    float *__restrict__ out_lin, uint32_t *__restrict__ out_rgba, uint32_t n)
{
    __shared__ float T[257];
    if (out_rgba) {                              // uniform over the grid: every lane arrives
        T[threadIdx.x] = gamma_t[threadIdx.x];
        if (threadIdx.x == 0) T[256] = gamma_t[256];
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t p = i;
    float r = in[3 * p], g = in[3 * p + 1], b = in[3 * p + 2];
    float4 a;
    if (pixel_albedo(gw, p, albedo, n_materials, a)) {
        r = usable(a.x) ? r * a.x : 0.0f;
        g = usable(a.y) ? g * a.y : 0.0f;
        b = usable(a.z) ? b * a.z : 0.0f;
    }
    if (out_lin) {
        out_lin[3 * p] = r;
        out_lin[3 * p + 1] = g;
        out_lin[3 * p + 2] = b;
    }
    if (out_rgba) out_rgba[p] = rvcp::pack_rgb8(r, g, b, T);
}

}  // namespace

extern "C" int rvcp_launch_demodulate(const float *in, const void *gbuffer, const void *albedo,
                                      uint32_t n_materials, float *out, uint32_t n, void *stream)
{
    hipLaunchKernelGGL(demodulate_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       (hipStream_t)stream, in, (const uint32_t *)gbuffer, (const float4 *)albedo,
                       n_materials, out, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rvcp_launch_remodulate(const float *in, const void *gbuffer, const void *albedo,
                                      uint32_t n_materials, const float *gamma_t, float *out_lin,
                                      uint32_t *out_rgba, uint32_t n, void *stream)
{
    hipLaunchKernelGGL(remodulate_tonemap_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       (hipStream_t)stream, in, (const uint32_t *)gbuffer, (const float4 *)albedo,
                       n_materials, gamma_t, out_lin, out_rgba, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
