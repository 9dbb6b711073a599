// rvcp_temporal.hip -- temporal reprojection and accumulation behind rvcp_temporal_accumulate_async
//  and rvcp_svgf_accumulate_async (§4.11 A).  The reference has no counterpart:
// every frame of it starts from nothing (ray_tracer_games101_branch.comp:497-500 stores the raw
// Monte-Carlo frame).
//
// One launch per frame, one lane per pixel p.  The pixel's primary hit (its G-buffer texel) is
// projected into the previous frame's camera; the four history texels around that point are
// accepted or rejected one by one (inside the frame, live, same material, normal and
// tangent-plane agreement, a history of at least one frame), the accepted ones are averaged with
// their bilinear weights, and the current colour is blended in with alpha = 1 / n, n being the
// shortest accepted history plus one, capped at max_history and alpha kept >= alpha_min.  A
// camera that did not move takes the single tap q = p with weight 1 through the same tests.
//
// Two kernels, one body: temporal_kernel carries colour and length, svgf_temporal_kernel also
// the first two moments of the luminance (8 B more per tap and per pixel) with a blend factor of
// their own.  The taps, the acceptance rules and the colour and length bits are the same by
// construction.
//
// Memory: per pixel 44 B of the current frame (12 B colour as three dwords, 32 B texel as two
// 16-byte loads) and at most four history taps of 48 B, 16 B written.  With a coherent camera
// motion neighbouring lanes read neighbouring taps, so nothing is staged in LDS; a wave covers 64
// consecutive pixels of a row (64 x 4 tile, as atrous_kernel).
//
// Numeric contract: float32 throughout, every operation rounded once in
// the order written below -- no fma (-ffp-contract=off), IEEE division
// (-fhip-fp32-correctly-rounded-divide-sqrt) -- so tests/temporal_ref.py and tests/svgf_ref.py,
// the numpy float32 restatements, reproduce every output bit.
#include <hip/hip_runtime.h>

#include "rvcp_post.h"

namespace rvcp {

namespace {

// running sums over the accepted taps: sum w, sum w c, sum w m, the shortest history
struct HistSums { float w, r, g, b, m1, m2; uint32_t nmin; };

// One history tap q = (qx, qy) of weight w for the pixel with normal pn, position pp and
// material word pm.  A tap that is not live (position, normal, colour, with MOMENTS the moments:
// DESIGN.md §4.15) is rejected as a MISS texel is; the length of a rejected tap is not read.
// Every test only rejects, so their order decides no bit.
template <bool MOMENTS>
__device__ __forceinline__ void hist_tap(HistSums &s, float w, int qx, int qy, uint32_t width,
                                         uint32_t height, v3 pn, v3 pp, uint32_t pm,
                                         const rvcp_temporal_params_t &P,
                                         const float *__restrict__ prev_c,
                                         const float4 *__restrict__ prev_g,
                                         const uint32_t *__restrict__ prev_len,
                                         const float2 *__restrict__ prev_m)
{
    // unsigned: -1 wraps to 2^32 - 1 >= width, height
    if ((uint32_t)qx >= width || (uint32_t)qy >= height) return;
    const size_t q = (size_t)(uint32_t)qy * width + (uint32_t)qx;
    const float4 q0 = prev_g[2 * q], q1 = prev_g[2 * q + 1];
    if (!live_g(q0, q1) || __float_as_uint(q1.w) != pm) return;
    if (!(dot3(pn, v3{q1.x, q1.y, q1.z}) >= P.normal_min)) return;
    const float d = dot3(pn, v3{q0.x - pp.x, q0.y - pp.y, q0.z - pp.z});
    if (!(fabsf(d) <= P.sigma_plane)) return;
    const v3 qc = load3(prev_c, q);
    const float2 m = MOMENTS ? prev_m[q] : make_float2(0.0f, 0.0f);
    if (!finite3(qc.x, qc.y, qc.z) || !finite1(m.x) || !finite1(m.y)) return;
    const uint32_t n = prev_len[q];
    if (n < 1u) return;
    s.w = s.w + w;
    s.r = s.r + w * qc.x;
    s.g = s.g + w * qc.y;
    s.b = s.b + w * qc.z;
    s.m1 = s.m1 + w * m.x;
    s.m2 = s.m2 + w * m.y;
    s.nmin = n < s.nmin ? n : s.nmin;
}

// The step of one pixel.  mode: 0 no history, 1 identity (the camera did not move), 2
// reprojection through `view`.  prev_m, out_m and alpha_moments_min are read with MOMENTS only.
template <bool MOMENTS>
__device__ __forceinline__ void accumulate(
    const float *__restrict__ cur_c, const float4 *__restrict__ cur_g,
    const float *__restrict__ prev_c, const float4 *__restrict__ prev_g,
    const uint32_t *__restrict__ prev_len, const float2 *__restrict__ prev_m,
    float *__restrict__ out_c, uint32_t *__restrict__ out_len, float2 *__restrict__ out_m,
    uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t mode,
    const rvcp_temporal_view_t &view, const rvcp_temporal_params_t &P, float alpha_moments_min)
{
    const auto [bx, by, x, y] = tile_pixel(tiles_x);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const v3 c = load3(cur_c, p);
    const float4 p0 = cur_g[2 * p], p1 = cur_g[2 * p + 1];
    v3 o = c;                                    // no usable history: the current colour
    float2 om = make_float2(0.0f, 0.0f);         // a pixel that is not live keeps no moments
    uint32_t len = 0;                            // ... and no history
    if (live_g(p0, p1) && finite3(c.x, c.y, c.z)) {
        len = 1;
        const float l1 = lum(c);
        const float2 mu = make_float2(l1, l1 * l1);
        om = mu;
        const v3 pp = v3{p0.x, p0.y, p0.z}, pn = v3{p1.x, p1.y, p1.z};
        const uint32_t pm = __float_as_uint(p1.w);
        HistSums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0xFFFFFFFFu};
        const auto tap = [&](float w, int qx, int qy) {
            hist_tap<MOMENTS>(s, w, qx, qy, width, height, pn, pp, pm, P, prev_c, prev_g, prev_len,
                              prev_m);
        };
        if (mode == 1u) {
            tap(1.0f, (int)x, (int)y);
        } else if (mode == 2u) {
            const float fw = (float)width, fh = (float)height;
            float fx, fy;
            const bool ok = project(view, pp, fw, fh, fx, fy);
            bilinear_taps(ok, fx, fy, fw, fh, tap);
        }
        if (s.w > 0.0f) {
            const v3 h = v3{s.r / s.w, s.g / s.w, s.b / s.w};
            const float2 hm = make_float2(s.m1 / s.w, s.m2 / s.w);
            // min(nmin + 1, max_history) without the overflow of nmin + 1
            const uint32_t n = s.nmin >= P.max_history ? P.max_history : s.nmin + 1u;
            const float inv = 1.0f / (float)n;
            const float alpha = inv < P.alpha_min ? P.alpha_min : inv;
            const float am = inv < alpha_moments_min ? alpha_moments_min : inv;
            o = v3{h.x + alpha * (c.x - h.x), h.y + alpha * (c.y - h.y), h.z + alpha * (c.z - h.z)};
            om = make_float2(hm.x + am * (mu.x - hm.x), hm.y + am * (mu.y - hm.y));
            len = n;
        }
    }
    store3(out_c, p, o);
    out_len[p] = len;
    if (MOMENTS) out_m[p] = om;
}

}  // namespace

__global__ __launch_bounds__(kTileX * kTileY) void temporal_kernel(
    const float *__restrict__ cur_c, const float4 *__restrict__ cur_g,
    const float *__restrict__ prev_c, const float4 *__restrict__ prev_g,
    const uint32_t *__restrict__ prev_len, float *__restrict__ out_c,
    uint32_t *__restrict__ out_len, uint32_t width, uint32_t height, uint32_t tiles_x,
    uint32_t mode, rvcp_temporal_view_t view, rvcp_temporal_params_t P)
{
    accumulate<false>(cur_c, cur_g, prev_c, prev_g, prev_len, nullptr, out_c, out_len, nullptr,
                      width, height, tiles_x, mode, view, P, 0.0f);
}

__global__ __launch_bounds__(kTileX * kTileY) void svgf_temporal_kernel(
    const float *__restrict__ cur_c, const float4 *__restrict__ cur_g,
    const float *__restrict__ prev_c, const float4 *__restrict__ prev_g,
    const uint32_t *__restrict__ prev_len, const float2 *__restrict__ prev_m,
    float *__restrict__ out_c, uint32_t *__restrict__ out_len, float2 *__restrict__ out_m,
    uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t mode, rvcp_temporal_view_t view,
    rvcp_temporal_params_t P, float alpha_moments_min)
{
    accumulate<true>(cur_c, cur_g, prev_c, prev_g, prev_len, prev_m, out_c, out_len, out_m, width,
                     height, tiles_x, mode, view, P, alpha_moments_min);
}

}  // namespace rvcp

extern "C" int rvcp_launch_temporal(const float *cur_c, const void *cur_g, const float *prev_c,
                                    const void *prev_g, const uint32_t *prev_len, float *out_c,
                                    uint32_t *out_len, uint32_t width, uint32_t height,
                                    uint32_t mode, const rvcp_temporal_view_t *view,
                                    const rvcp_temporal_params_t *params, void *stream)
{
    const uint32_t tx = (width + rvcp::kTileX - 1) / rvcp::kTileX;
    const uint32_t ty = (height + rvcp::kTileY - 1) / rvcp::kTileY;
    rvcp_temporal_view_t V = {};
    if (view) V = *view;
    hipLaunchKernelGGL(rvcp::temporal_kernel, dim3(tx * ty), dim3(rvcp::kTileX * rvcp::kTileY), 0,
                       (hipStream_t)stream, cur_c, (const float4 *)cur_g, prev_c,
                       (const float4 *)prev_g, prev_len, out_c, out_len, width, height, tx, mode,
                       V, *params);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rvcp_launch_svgf_temporal(const float *cur_c, const void *cur_g, const float *prev_c,
                                         const void *prev_g, const uint32_t *prev_len,
                                         const float *prev_m, float *out_c, uint32_t *out_len,
                                         float *out_m, uint32_t width, uint32_t height,
                                         uint32_t mode, const rvcp_temporal_view_t *view,
                                         const rvcp_temporal_params_t *params,
                                         float alpha_moments_min, void *stream)
{
    const uint32_t tx = (width + rvcp::kTileX - 1) / rvcp::kTileX;
    const uint32_t ty = (height + rvcp::kTileY - 1) / rvcp::kTileY;
    rvcp_temporal_view_t V = {};
    if (view) V = *view;
    hipLaunchKernelGGL(rvcp::svgf_temporal_kernel, dim3(tx * ty), dim3(rvcp::kTileX * rvcp::kTileY),
                       0, (hipStream_t)stream, cur_c, (const float4 *)cur_g, prev_c,
                       (const float4 *)prev_g, prev_len, (const float2 *)prev_m, out_c, out_len,
                       (float2 *)out_m, width, height, tx, mode, V, *params, alpha_moments_min);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
