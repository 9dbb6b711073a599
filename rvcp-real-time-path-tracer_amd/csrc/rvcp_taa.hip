// rvcp_taa.hip -- the temporal anti-aliasing resolve behind rvcp_taa_resolve_async
// (DESIGN.md §4.13).  The reference has no counterpart: sample_ray
// (ray_tracer_games101_branch.comp:217-235) sends every primary ray through the pixel centre.
//
// One launch per frame, one lane per pixel p.  The frame was rendered through a camera rotated
// by a sub-pixel jitter (rvcp_taa_jitter_push); the resolve keeps a history of the DISPLAYED
// colour (clamped to [0, 1]) on the unjittered pixel grid.  The pixel's history lies where the
// difference of its primary hit's projections into the previous and the current unjittered camera
// puts it (a miss pixel: where the rotation alone moves its direction); the four history texels
// around that point are averaged with their bilinear weights (a tap needs a history of at least
// one frame, nothing else: the clamp below is what protects an edge), the average is clamped
// into the colour box of the 3 x 3 current pixels around p (not on the frame's border, whose box
// is degenerate) and the current colour is blended in with alpha = max(1 / n, alpha_min).
//
// Memory: per pixel 28 B of the current frame (12 B colour as three dwords, the texel's first
// 16 B as one load), the 8 neighbouring colours (three rows of a coalesced row segment, served
// by the caches: a wave covers 64 consecutive pixels of a row, 64 x 4 tile as temporal_kernel)
// and at most four history taps of 16 B; 16 B written, 20 B with the fused RGBA8 store.
//
// Numeric contract: float32 throughout, every operation rounded once in the
// order written below -- no fma (-ffp-contract=off), IEEE division
// (-fhip-fp32-correctly-rounded-divide-sqrt) -- so tests/taa_ref.py, the numpy float32
// restatement, reproduces every output bit.
#include <hip/hip_runtime.h>

#include "rvcp_post.h"
#include "rvcp_tonemap.h"

namespace rvcp {

namespace {

// running sums over the accepted taps: sum w, sum w c, the shortest history
struct Sums { float w, r, g, b; uint32_t nmin; };

// One history tap q = (qx, qy) of weight w.  The colour of a rejected tap is not read.
__device__ __forceinline__ void tap(Sums &s, float w, int qx, int qy, uint32_t width,
                                    uint32_t height, const float *__restrict__ prev_c,
                                    const uint32_t *__restrict__ prev_len)
{
    // unsigned: -1 wraps to 2^32 - 1 >= width, height
    if ((uint32_t)qx >= width || (uint32_t)qy >= height) return;
    const size_t q = (size_t)(uint32_t)qy * width + (uint32_t)qx;
    const uint32_t n = prev_len[q];
    if (n < 1u) return;
    s.w = s.w + w;
    s.r = s.r + w * prev_c[3 * q];
    s.g = s.g + w * prev_c[3 * q + 1];
    s.b = s.b + w * prev_c[3 * q + 2];
    s.nmin = n < s.nmin ? n : s.nmin;
}

}  // namespace

// mode: 0 no history, 1 identity (the camera is at rest), 2 reprojection from `cur` into `prev`
__global__ __launch_bounds__(kTileX * kTileY) void taa_resolve_kernel(
    const float *__restrict__ cur_c, const float4 *__restrict__ cur_g,
    const float *__restrict__ prev_c, const uint32_t *__restrict__ prev_len,
    float *__restrict__ out_c, uint32_t *__restrict__ out_len, uint32_t *__restrict__ out_rgba,
    const float *__restrict__ gamma_t, uint32_t width, uint32_t height, uint32_t tiles_x,
    uint32_t mode, rvcp_temporal_view_t cur, rvcp_temporal_view_t prev, rvcp_taa_params_t P)
{
    const auto [bx, by, x, y] = tile_pixel(tiles_x);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const v3 c = load_sat(cur_c, p);
    v3 o = c;                                    // no usable history: the displayed current colour
    uint32_t len = 1;
    Sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0xFFFFFFFFu};
    const auto hist = [&](float w, int qx, int qy) {
        tap(s, w, qx, qy, width, height, prev_c, prev_len);
    };
    if (mode == 1u) {
        hist(1.0f, (int)x, (int)y);
    } else if (mode == 2u) {
        const float fw = (float)width, fh = (float)height;
        float fx, fy;
        // cur_g[2 * p]: position and face, the texel's first 16 bytes
        const bool ok = history_point(cur_g[2 * p], (float)x, (float)y, cur, prev, fw, fh, fx, fy);
        bilinear_taps(ok, fx, fy, fw, fh, hist);
    }
    if (s.w > 0.0f) {
        v3 h = v3{s.r / s.w, s.g / s.w, s.b / s.w};
        // min(nmin + 1, max_history) without the overflow of nmin + 1
        const uint32_t n = s.nmin >= P.max_history ? P.max_history : s.nmin + 1u;
        // x, y >= 1 and x + 1 < width, y + 1 < height: all nine pixels are inside the frame
        if (P.clamp == 1u && x > 0u && x + 1u < width && y > 0u && y + 1u < height) {
            v3 lo = c, hi = c;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    const v3 q = load_sat(cur_c, (size_t)(y + dy) * width + (x + dx));
                    lo = v3{fminf(lo.x, q.x), fminf(lo.y, q.y), fminf(lo.z, q.z)};
                    hi = v3{fmaxf(hi.x, q.x), fmaxf(hi.y, q.y), fmaxf(hi.z, q.z)};
                }
            }
            h = v3{clamp_to(h.x, lo.x, hi.x), clamp_to(h.y, lo.y, hi.y), clamp_to(h.z, lo.z, hi.z)};
        }
        float alpha = 1.0f / (float)n;
        if (alpha < P.alpha_min) alpha = P.alpha_min;
        o = v3{h.x + alpha * (c.x - h.x), h.y + alpha * (c.y - h.y), h.z + alpha * (c.z - h.z)};
        len = n;
    }
    store3(out_c, p, o);
    out_len[p] = len;
    if (out_rgba) out_rgba[p] = pack_rgb8(o.x, o.y, o.z, gamma_t);
}

}  // namespace rvcp

extern "C" int rvcp_launch_taa_resolve(const float *cur_c, const void *cur_g, const float *prev_c,
                                       const uint32_t *prev_len, float *out_c, uint32_t *out_len,
                                       uint32_t *out_rgba, const float *gamma_t, uint32_t width,
                                       uint32_t height, uint32_t mode,
                                       const rvcp_temporal_view_t *cur_view,
                                       const rvcp_temporal_view_t *prev_view,
                                       const rvcp_taa_params_t *params, void *stream)
{
    const uint32_t tx = (width + rvcp::kTileX - 1) / rvcp::kTileX;
    const uint32_t ty = (height + rvcp::kTileY - 1) / rvcp::kTileY;
    rvcp_temporal_view_t C = {}, V = {};
    if (cur_view) C = *cur_view;
    if (prev_view) V = *prev_view;
    hipLaunchKernelGGL(rvcp::taa_resolve_kernel, dim3(tx * ty), dim3(rvcp::kTileX * rvcp::kTileY),
                       0, (hipStream_t)stream, cur_c, (const float4 *)cur_g, prev_c, prev_len, out_c,
                       out_len, out_rgba, gamma_t, width, height, tx, mode, C, V, *params);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
