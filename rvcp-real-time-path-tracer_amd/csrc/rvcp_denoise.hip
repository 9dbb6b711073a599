// rvcp_denoise.hip -- the edge-avoiding a-trous wavelet filter behind rvcp_denoise_async
// (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global
// Illumination Filtering", HPG 2010), guided by the G-buffer of rvcp_render_gbuffer_async.  The
// reference has no counterpart (it stores the raw frame, ray_tracer_games101_branch.comp:497-500).
//
// One launch per pass, one lane per pixel.  Pass i visits the 25 taps q = p + 2^i (dx, dy),
// dx, dy in -2..2, row-major.  Two kernels, chosen by the step (DESIGN.md §4.9 has the times):
//   steps 1 and 2: atrous_lds_kernel -- the workgroup's 32 x 8 pixels and their halo of 2 x step
//     are staged once in LDS (colour, position, normal and the live flag as separate
//     arrays, so a wave's reads of one array hit consecutive banks), each texel read from memory
//     as two 16-byte loads; the taps then come from LDS.  1024^2: 0.040 / 0.039 ms per pass.
//   steps >= 4: atrous_kernel -- every tap read straight from memory (L2-served); the halo would
//     be 2.6 x the tile (step 4) and more.  0.057 - 0.062 ms per pass at every step (0.085 -
//     0.090 while a tap's colour was loaded only after its texel had passed the test; the live
//     test of §4.15 needs the colour first, so a tap's five loads now issue together).
// Both run the same arithmetic on the same values in the same order.
//
// Numeric contract: every weight is built from single, correctly rounded f32
// +, -, x, / in the order written below -- no fma (-ffp-contract=off), no exp, no pow, IEEE
// division (-fhip-fp32-correctly-rounded-divide-sqrt) -- so tests/denoise_ref.py, the numpy
// float32 restatement, reproduces every output bit.
#include <hip/hip_runtime.h>

#include "rvcp_post.h"

using namespace rvcp;

namespace {

// live for a pass: position, normal and the colour in the pass's input
__device__ __forceinline__ bool live(float4 g0, float4 g1, v3 c) {
    return live_g(g0, g1) && finite3(c.x, c.y, c.z);
}

// the wave-uniform parameters of a pass
struct PassArgs {
    uint32_t normal_power_log2, use_color;
    float color_s2, sigma_plane;       // sigma_i^2 of this pass; the plane-distance width
};

// running sums of a pixel: sum w, sum w c
struct Sums { float w, r, g, b; };

// One tap q of pixel p: w = ((h w_n) w_z) w_c added to the sums, in this order.
//   w_n, w_z: rvcp_post.h's weight_n, weight_z
//   w_c = 1 / (1 + |c_p - c_q|^2 / sigma_i^2)          (1 when the colour weight is off)
__device__ __forceinline__ void tap(Sums &s, float h, const PassArgs &A, v3 pn, v3 pp, v3 pc,
                                    v3 qn, v3 qp, v3 qc) {
    const float wn = weight_n(pn, qn, A.normal_power_log2);
    const float wz = weight_z(pn, pp, qp, A.sigma_plane);
    float wc = 1.0f;
    if (A.use_color) {
        const v3 e = v3{pc.x - qc.x, pc.y - qc.y, pc.z - qc.z};
        wc = 1.0f / (1.0f + dot3(e, e) / A.color_s2);
    }
    const float w = ((h * wn) * wz) * wc;
    s.w = s.w + w;
    s.r = s.r + w * qc.x;
    s.g = s.g + w * qc.y;
    s.b = s.b + w * qc.z;
}

// Steps >= 4: every tap straight from memory.  A wave covers 64 consecutive pixels of a row.
__global__ __launch_bounds__(kTileX * kTileY) void atrous_kernel(
    const float *__restrict__ in, const float4 *__restrict__ guide, float *__restrict__ out,
    uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t step, PassArgs A)
{
    const auto [bx, by, x, y] = tile_pixel(tiles_x);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const v3 pc = load3(in, p);
    const float4 p0 = guide[2 * p], p1 = guide[2 * p + 1];
    v3 o = pc;                                   // a pixel that is not live passes through
    if (live(p0, p1, pc)) {
        const v3 pp = v3{p0.x, p0.y, p0.z}, pn = v3{p1.x, p1.y, p1.z};
        Sums s = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                // unsigned: a tap left of / above the frame wraps to >= 2^31 > width, height
                const uint32_t qx = x + (uint32_t)dx * step, qy = y + (uint32_t)dy * step;
                if (qx >= width || qy >= height) continue;
                const size_t q = (size_t)qy * width + qx;
                const float4 q0 = guide[2 * q], q1 = guide[2 * q + 1];
                const v3 qc = load3(in, q);
                if (!live(q0, q1, qc)) continue;
                tap(s, b3(dy) * b3(dx), A, pn, pp, pc, v3{q1.x, q1.y, q1.z}, v3{q0.x, q0.y, q0.z},
                    qc);
            }
        }
        // The centre tap has w = (9/64) w_n with w_n = |n_p|^2 squared normal_power_log2 times
        // (w_z = w_c = 1): 9/64 for a unit normal, but 0 for a zero normal or one so short that
        // the squaring underflows.  Weights that do not sum to more than 0 (a NaN sum, from
        // finite values whose products overflow, included) leave the colour as it came.
        if (s.w > 0.0f) o = v3{s.r / s.w, s.g / s.w, s.b / s.w};
    }
    store3(out, p, o);
}

// Steps 1 and 2: the tile and its halo in LDS.  (32 + 4 STEP) x (8 + 4 STEP) texels, 40 B each:
// 17.3 KB (STEP 1) and 25.6 KB (STEP 2) per workgroup.  A halo texel outside the frame only gets
// its flag cleared; of an unflagged texel nothing but the flag is read, except by its own pixel
// (inside the frame, so loaded), which passes its colour through.
template <uint32_t STEP>
__global__ __launch_bounds__(kLX * kLY) void atrous_lds_kernel(
    const float *__restrict__ in, const float4 *__restrict__ guide, float *__restrict__ out,
    uint32_t width, uint32_t height, uint32_t tiles_x, PassArgs A)
{
    constexpr uint32_t HW = kLX + 4 * STEP, HH = kLY + 4 * STEP, HN = HW * HH;
    __shared__ float s_px[HN], s_py[HN], s_pz[HN], s_nx[HN], s_ny[HN], s_nz[HN];
    __shared__ float s_r[HN], s_g[HN], s_b[HN];
    __shared__ uint32_t s_ok[HN];
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const uint32_t x0 = bx * kLX, y0 = by * kLY;
    for (uint32_t i = threadIdx.x; i < HN; i += kLX * kLY) {
        const uint32_t hy = i / HW, hx = i - hy * HW;
        // unsigned: left of / above the frame wraps to >= 2^31 > width, height
        const uint32_t gx = x0 + hx - 2 * STEP, gy = y0 + hy - 2 * STEP;
        uint32_t ok = 0;
        if (gx < width && gy < height) {
            const size_t q = (size_t)gy * width + gx;
            const float4 q0 = guide[2 * q], q1 = guide[2 * q + 1];
            s_px[i] = q0.x; s_py[i] = q0.y; s_pz[i] = q0.z;
            s_nx[i] = q1.x; s_ny[i] = q1.y; s_nz[i] = q1.z;
            const v3 qc = load3(in, q);
            s_r[i] = qc.x; s_g[i] = qc.y; s_b[i] = qc.z;
            ok = live(q0, q1, qc) ? 1u : 0u;     // the live flag, once per staged texel
        }
        s_ok[i] = ok;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & (kLX - 1u), ly = threadIdx.x / kLX;
    const uint32_t x = x0 + lx, y = y0 + ly;
    if (x >= width || y >= height) return;
    const uint32_t c = (ly + 2 * STEP) * HW + lx + 2 * STEP;      // the pixel's own LDS slot
    const v3 pc = v3{s_r[c], s_g[c], s_b[c]};
    v3 o = pc;
    if (s_ok[c]) {
        const v3 pp = v3{s_px[c], s_py[c], s_pz[c]}, pn = v3{s_nx[c], s_ny[c], s_nz[c]};
        Sums s = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                // within the halo by construction: |dy|, |dx| <= 2 slots of STEP around c
                const uint32_t q = (uint32_t)((int)c + dy * (int)(STEP * HW) + dx * (int)STEP);
                if (!s_ok[q]) continue;
                tap(s, b3(dy) * b3(dx), A, pn, pp, pc, v3{s_nx[q], s_ny[q], s_nz[q]},
                    v3{s_px[q], s_py[q], s_pz[q]}, v3{s_r[q], s_g[q], s_b[q]});
            }
        }
        if (s.w > 0.0f) o = v3{s.r / s.w, s.g / s.w, s.b / s.w};      // as atrous_kernel
    }
    const size_t p = (size_t)y * width + x;
    store3(out, p, o);
}

}  // namespace

extern "C" int rvcp_launch_denoise_pass(const float *in, const void *gbuffer, float *out,
                                        uint32_t width, uint32_t height, uint32_t step,
                                        uint32_t normal_power_log2, uint32_t use_color,
                                        float color_s2, float sigma_plane, void *stream)
{
    const PassArgs A = {normal_power_log2, use_color, color_s2, sigma_plane};
    const float4 *guide = (const float4 *)gbuffer;
    hipStream_t s = (hipStream_t)stream;
    if (step <= 2) {
        const uint32_t tx = (width + kLX - 1) / kLX, ty = (height + kLY - 1) / kLY;
        hipLaunchKernelGGL(step == 1 ? atrous_lds_kernel<1> : atrous_lds_kernel<2>, dim3(tx * ty),
                           dim3(kLX * kLY), 0, s, in, guide, out, width, height, tx, A);
    } else {
        const uint32_t tx = (width + kTileX - 1) / kTileX, ty = (height + kTileY - 1) / kTileY;
        hipLaunchKernelGGL(atrous_kernel, dim3(tx * ty), dim3(kTileX * kTileY), 0, s, in, guide,
                           out, width, height, tx, step, A);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
