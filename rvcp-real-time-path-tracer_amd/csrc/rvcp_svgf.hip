// rvcp_svgf.hip -- spatiotemporal variance-guided filtering behind rvcp_svgf_filter_async
// (Schied et al.: "Spatiotemporal Variance-Guided Filtering", HPG 2017).
// The reference has no counterpart (it stores the raw frame,
// ray_tracer_games101_branch.comp:497-500).  The accumulation with moments (§4.11 A,
// svgf_temporal_kernel) shares its body with temporal_kernel and lives in rvcp_temporal.hip.
//
// Two kinds of kernel, one lane per pixel each:
//   svgf_variance_kernel   moments -> variance.  A pixel whose history is at least spatial_below
//     frames long takes m2 - m1^2; a younger one the same statistic over its 7 x 7 neighbourhood
//     under the geometric weights, scaled by spatial_below / len.  The workgroup's 32 x 8 pixels
//     and their halo of 3 (38 x 14 texels, nine SoA arrays, 19.2 KB) are staged in LDS only when
//     some pixel of the workgroup is that young (a workgroup-wide vote before any lane returns):
//     after a few static frames no workgroup stages anything.
//   svgf_atrous_lds_kernel<STEP> / svgf_atrous_kernel   one variance-guided a-trous pass: the 25
//     taps of rvcp_denoise.hip with the colour weight replaced by a luminance weight whose width is
//     the pixel's own variance, prefiltered over 3 x 3, and the variance filtered with the squared
//     weights.  Steps 1 and 2 stage the tile and its halo of 2 x step in LDS (eleven SoA arrays:
//     19.0 KB and 28.2 KB), steps >= 4 read every tap from memory, as §4.9 measured for the plain
//     filter.  Both call one tap(); the luminance of a tap is recomputed from its colour.
//
// Numeric contract: float32 throughout, every operation rounded once in the
// order written below -- no fma (-ffp-contract=off), no exp, pow or sqrt, IEEE division
// (-fhip-fp32-correctly-rounded-divide-sqrt) -- so tests/svgf_ref.py, the numpy float32
// restatement, reproduces every output bit.
#include <hip/hip_runtime.h>

#include "rvcp_post.h"

using namespace rvcp;

namespace {

// ---------------------------------------------------------------------------------------------
// B. variance
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLX * kLY) void svgf_variance_kernel(
    const float2 *__restrict__ mom, const uint32_t *__restrict__ len,
    const float4 *__restrict__ guide, float *__restrict__ out_v, uint32_t width, uint32_t height,
    uint32_t tiles_x, uint32_t spatial_below, uint32_t npl2, float sigma_plane)
{
    constexpr uint32_t R = 3, HW = kLX + 2 * R, HH = kLY + 2 * R, HN = HW * HH;
    __shared__ float s_px[HN], s_py[HN], s_pz[HN], s_nx[HN], s_ny[HN], s_nz[HN];
    __shared__ float s_m1[HN], s_m2[HN];
    __shared__ uint32_t s_ok[HN];
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const uint32_t x0 = bx * kLX, y0 = by * kLY;
    const uint32_t lx = threadIdx.x & (kLX - 1u), ly = threadIdx.x / kLX;
    const uint32_t x = x0 + lx, y = y0 + ly;
    const bool inside = x < width && y < height;
    const size_t p = (size_t)y * width + x;
    bool filt = false;
    uint32_t n = 0;
    float2 m = make_float2(0.0f, 0.0f);
    v3 pp = v3{0.0f, 0.0f, 0.0f}, pn = pp;
    if (inside) {
        const float4 p0 = guide[2 * p], p1 = guide[2 * p + 1];
        // live for this launch: finite moments too, and a history of at least one frame (the
        // accumulation leaves length 0 and zero moments on a pixel that was not live for it)
        if (live_g(p0, p1)) {
            m = mom[p];
            n = len[p];
            filt = finite1(m.x) && finite1(m.y) && n >= 1u;
        }
        if (filt) {
            pp = v3{p0.x, p0.y, p0.z};
            pn = v3{p1.x, p1.y, p1.z};
        }
    }
    const bool young = filt && n < spatial_below;
    // every lane of the workgroup votes (none has returned): stage only when someone needs it
    if (__syncthreads_or(young ? 1 : 0)) {
        for (uint32_t i = threadIdx.x; i < HN; i += kLX * kLY) {
            const uint32_t hy = i / HW, hx = i - hy * HW;
            // unsigned: left of / above the frame wraps to >= 2^31 > width, height
            const uint32_t gx = x0 + hx - R, gy = y0 + hy - R;
            uint32_t ok = 0;
            if (gx < width && gy < height) {
                const size_t q = (size_t)gy * width + gx;
                const float4 q0 = guide[2 * q], q1 = guide[2 * q + 1];
                const float2 qm = mom[q];
                if (live_g(q0, q1) && finite1(qm.x) && finite1(qm.y) && len[q] >= 1u) {   // live
                    s_px[i] = q0.x; s_py[i] = q0.y; s_pz[i] = q0.z;
                    s_nx[i] = q1.x; s_ny[i] = q1.y; s_nz[i] = q1.z;
                    s_m1[i] = qm.x; s_m2[i] = qm.y;
                    ok = 1u;
                }
            }
            s_ok[i] = ok;
        }
        __syncthreads();
    }
    if (!inside) return;
    float v = 0.0f;                              // a pixel that is not live has no variance
    if (filt) {
        if (!young) {
            v = m.y - m.x * m.x;
            if (!(v > 0.0f)) v = 0.0f;
        } else {
            const uint32_t c = (ly + R) * HW + lx + R;       // the pixel's own LDS slot
            float ws = 0.0f, a1 = 0.0f, a2 = 0.0f;
            for (int dy = -(int)R; dy <= (int)R; ++dy) {
#pragma unroll
                for (int dx = -(int)R; dx <= (int)R; ++dx) {
                    // within the halo by construction: |dy|, |dx| <= R slots around c
                    const uint32_t q = (uint32_t)((int)c + dy * (int)HW + dx);
                    if (!s_ok[q]) continue;
                    const float wn = weight_n(pn, v3{s_nx[q], s_ny[q], s_nz[q]}, npl2);
                    const float wz = weight_z(pn, pp, v3{s_px[q], s_py[q], s_pz[q]}, sigma_plane);
                    const float w = wn * wz;
                    ws = ws + w;
                    a1 = a1 + w * s_m1[q];
                    a2 = a2 + w * s_m2[q];
                }
            }
            // the centre tap has w ~ 1 for a unit normal (w_n = |n|^2 squared, w_z = 1); weights
            // that do not sum to more than 0 (a zero normal) give no estimate
            if (ws > 0.0f) {
                const float e1 = a1 / ws, e2 = a2 / ws;
                v = e2 - e1 * e1;
                if (!(v > 0.0f)) v = 0.0f;
                v = v * ((float)spatial_below / (float)n);
            }
        }
    }
    out_v[p] = v;
}

// ---------------------------------------------------------------------------------------------
// C. variance-guided a-trous
// ---------------------------------------------------------------------------------------------

// the wave-uniform parameters of a pass
struct GuideArgs {
    uint32_t normal_power_log2, use_lum;
    float sigma_l2, epsilon, sigma_plane;        // sigma_luminance^2 (host, float32)
};

// running sums of a pixel: sum w, sum w c, sum w^2 v
struct Sums { float w, r, g, b, v; };

// One tap q of pixel p: w = ((h w_n) w_z) w_l added to the sums, in this order.
//   w_l = 1 / (1 + (l(c_p) - l(c_q))^2 / den)          (1 when the luminance weight is off)
__device__ __forceinline__ void tap(Sums &s, float h, const GuideArgs &A, float den, float lp,
                                    v3 pn, v3 pp, v3 qn, v3 qp, v3 qc, float qv) {
    const float wn = weight_n(pn, qn, A.normal_power_log2);
    const float wz = weight_z(pn, pp, qp, A.sigma_plane);
    float w = (h * wn) * wz;
    if (A.use_lum) {
        const float dl = lp - lum(qc);
        w = w * (1.0f / (1.0f + (dl * dl) / den));
    }
    s.w = s.w + w;
    s.r = s.r + w * qc.x;
    s.g = s.g + w * qc.y;
    s.b = s.b + w * qc.z;
    s.v = s.v + (w * w) * qv;
}

// The end of a pass.  The centre tap has w = (9/64) w_n with w_n = |n_p|^2 squared
// normal_power_log2 times (w_z = w_l = 1): 9/64 for a unit normal, 0 for a zero normal.  Weights
// that do not sum to more than 0 leave colour and variance as a MISS pixel's (o, ov preset); a sum
// whose square underflows leaves the variance 0.
__device__ __forceinline__ void finish(const Sums &s, v3 &o, float &ov) {
    if (!(s.w > 0.0f)) return;
    o = v3{s.r / s.w, s.g / s.w, s.b / s.w};
    const float w2 = s.w * s.w;
    if (w2 > 0.0f) ov = s.v / w2;
}

// live for a pass: position, normal, colour and variance
__device__ __forceinline__ bool live(float4 g0, float4 g1, v3 c, float v) {
    return live_g(g0, g1) && finite3(c.x, c.y, c.z) && finite1(v);
}

// the 3 x 3 prefilter of the variance: 1/4 centre, 1/8 edges, 1/16 corners
__device__ __forceinline__ constexpr float g3(int dy, int dx) {
    return (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
}

// Any step: every tap straight from memory.
__global__ __launch_bounds__(kTileX * kTileY) void svgf_atrous_kernel(
    const float *__restrict__ in_c, const float *__restrict__ in_v,
    const float4 *__restrict__ guide, float *__restrict__ out_c, float *__restrict__ out_v,
    uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t step, GuideArgs A)
{
    const auto [bx, by, x, y] = tile_pixel(tiles_x);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const v3 pc = load3(in_c, p);
    const float4 p0 = guide[2 * p], p1 = guide[2 * p + 1];
    v3 o = pc;                                   // a pixel that is not live passes through
    float ov = 0.0f;
    if (live(p0, p1, pc, in_v[p])) {
        const v3 pp = v3{p0.x, p0.y, p0.z}, pn = v3{p1.x, p1.y, p1.z};
        float den = 1.0f, lp = 0.0f;
        if (A.use_lum) {
            float gs = 0.0f, vs = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    // unsigned: a tap left of / above the frame wraps to 2^32 - 1 >= width, height
                    const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;
                    if (qx >= width || qy >= height) continue;
                    const size_t q = (size_t)qy * width + qx;
                    const float qv = in_v[q];
                    if (!live(guide[2 * q], guide[2 * q + 1],
                              load3(in_c, q), qv)) continue;
                    gs = gs + g3(dy, dx);
                    vs = vs + g3(dy, dx) * qv;
                }
            }
            den = A.sigma_l2 * (vs / gs) + A.epsilon;            // gs >= 1/4: the centre is live
            lp = lum(pc);
        }
        Sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                // unsigned: a tap left of / above the frame wraps to >= 2^31 > width, height
                const uint32_t qx = x + (uint32_t)dx * step, qy = y + (uint32_t)dy * step;
                if (qx >= width || qy >= height) continue;
                const size_t q = (size_t)qy * width + qx;
                const float4 q0 = guide[2 * q], q1 = guide[2 * q + 1];
                const v3 qc = load3(in_c, q);
                const float qv = in_v[q];
                if (!live(q0, q1, qc, qv)) continue;
                tap(s, b3(dy) * b3(dx), A, den, lp, pn, pp, v3{q1.x, q1.y, q1.z},
                    v3{q0.x, q0.y, q0.z}, qc, qv);
            }
        }
        finish(s, o, ov);
    }
    store3(out_c, p, o);
    out_v[p] = ov;
}

// Steps 1 and 2: the tile and its halo in LDS.  (32 + 4 STEP) x (8 + 4 STEP) texels, 44 B each:
// 19.0 KB (STEP 1) and 28.2 KB (STEP 2) per workgroup.  A halo texel outside the frame only gets
// its flag cleared; of an unflagged texel nothing but the flag is read, except by its own pixel
// (inside the frame, so loaded), which passes its colour through.  The 3 x 3 prefilter reads the
// same tile (its reach of 1 is inside the halo of 2 STEP).
template <uint32_t STEP>
__global__ __launch_bounds__(kLX * kLY) void svgf_atrous_lds_kernel(
    const float *__restrict__ in_c, const float *__restrict__ in_v,
    const float4 *__restrict__ guide, float *__restrict__ out_c, float *__restrict__ out_v,
    uint32_t width, uint32_t height, uint32_t tiles_x, GuideArgs A)
{
    constexpr uint32_t HW = kLX + 4 * STEP, HH = kLY + 4 * STEP, HN = HW * HH;
    __shared__ float s_px[HN], s_py[HN], s_pz[HN], s_nx[HN], s_ny[HN], s_nz[HN];
    __shared__ float s_r[HN], s_g[HN], s_b[HN], s_v[HN];
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
            const v3 qc = load3(in_c, q);
            const float qv = in_v[q];
            s_r[i] = qc.x; s_g[i] = qc.y; s_b[i] = qc.z;
            s_v[i] = qv;
            ok = live(q0, q1, qc, qv) ? 1u : 0u;     // the live flag, once per staged texel
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
    float ov = 0.0f;
    if (s_ok[c]) {
        const v3 pp = v3{s_px[c], s_py[c], s_pz[c]}, pn = v3{s_nx[c], s_ny[c], s_nz[c]};
        float den = 1.0f, lp = 0.0f;
        if (A.use_lum) {
            float gs = 0.0f, vs = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    // within the halo: 2 STEP >= 2 slots around c
                    const uint32_t q = (uint32_t)((int)c + dy * (int)HW + dx);
                    if (!s_ok[q]) continue;
                    gs = gs + g3(dy, dx);
                    vs = vs + g3(dy, dx) * s_v[q];
                }
            }
            den = A.sigma_l2 * (vs / gs) + A.epsilon;            // gs >= 1/4: the centre is live
            lp = lum(pc);
        }
        Sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                // within the halo by construction: |dy|, |dx| <= 2 slots of STEP around c
                const uint32_t q = (uint32_t)((int)c + dy * (int)(STEP * HW) + dx * (int)STEP);
                if (!s_ok[q]) continue;
                tap(s, b3(dy) * b3(dx), A, den, lp, pn, pp, v3{s_nx[q], s_ny[q], s_nz[q]},
                    v3{s_px[q], s_py[q], s_pz[q]}, v3{s_r[q], s_g[q], s_b[q]}, s_v[q]);
            }
        }
        finish(s, o, ov);
    }
    const size_t p = (size_t)y * width + x;
    store3(out_c, p, o);
    out_v[p] = ov;
}

}  // namespace

extern "C" int rvcp_launch_svgf_variance(const float *moments, const uint32_t *len,
                                         const void *gbuffer, float *out_v, uint32_t width,
                                         uint32_t height, uint32_t spatial_below,
                                         uint32_t normal_power_log2, float sigma_plane, void *stream)
{
    const uint32_t tx = (width + kLX - 1) / kLX, ty = (height + kLY - 1) / kLY;
    hipLaunchKernelGGL(svgf_variance_kernel, dim3(tx * ty), dim3(kLX * kLY), 0, (hipStream_t)stream,
                       (const float2 *)moments, len, (const float4 *)gbuffer, out_v, width, height,
                       tx, spatial_below, normal_power_log2, sigma_plane);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// force_direct: steps 1 and 2 through the direct kernel too (tools/svgf_time.py's comparison)
extern "C" int rvcp_launch_svgf_pass(const float *in_c, const float *in_v, const void *gbuffer,
                                     float *out_c, float *out_v, uint32_t width, uint32_t height,
                                     uint32_t step, uint32_t normal_power_log2, uint32_t use_lum,
                                     float sigma_l2, float epsilon, float sigma_plane,
                                     uint32_t force_direct, void *stream)
{
    const GuideArgs A = {normal_power_log2, use_lum, sigma_l2, epsilon, sigma_plane};
    const float4 *guide = (const float4 *)gbuffer;
    hipStream_t s = (hipStream_t)stream;
    if (step <= 2 && !force_direct) {
        const uint32_t tx = (width + kLX - 1) / kLX, ty = (height + kLY - 1) / kLY;
        hipLaunchKernelGGL(step == 1 ? svgf_atrous_lds_kernel<1> : svgf_atrous_lds_kernel<2>,
                           dim3(tx * ty), dim3(kLX * kLY), 0, s, in_c, in_v, guide, out_c, out_v,
                           width, height, tx, A);
    } else {
        const uint32_t tx = (width + kTileX - 1) / kTileX, ty = (height + kTileY - 1) / kTileY;
        hipLaunchKernelGGL(svgf_atrous_kernel, dim3(tx * ty), dim3(kTileX * kTileY), 0, s, in_c,
                           in_v, guide, out_c, out_v, width, height, tx, step, A);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
