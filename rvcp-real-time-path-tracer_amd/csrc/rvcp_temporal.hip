// rvcp_temporal.hip -- temporal reprojection and accumulation behind rvcp_temporal_accumulate_async
// (DESIGN.md §4.10).  The reference has no counterpart: every frame of it starts from nothing
// (ray_tracer_games101_branch.comp:497-500 stores the raw Monte-Carlo frame).
//
// One launch per frame, one lane per pixel p.  The pixel's primary hit (its G-buffer texel) is
// projected into the previous frame's camera; the four history texels around that point are
// accepted or rejected one by one (inside the frame, filterable, same material, normal and
// tangent-plane agreement, a history of at least one frame), the accepted ones are averaged with
// their bilinear weights, and the current colour is blended in with alpha = 1 / n, n being the
// shortest accepted history plus one, capped at max_history and alpha kept >= alpha_min.  A
// camera that did not move takes the single tap q = p with weight 1 through the same tests.
//
// Memory: per pixel 44 B of the current frame (12 B colour as three dwords, 32 B texel as two
// 16-byte loads) and at most four history taps of 48 B, 16 B written.  With a coherent camera
// motion neighbouring lanes read neighbouring taps, so nothing is staged in LDS; a wave covers 64
// consecutive pixels of a row (64 x 4 tile, as atrous_kernel).
//
// Numeric contract: float32 throughout, every operation rounded once in the
// order written below -- no fma (-ffp-contract=off), IEEE division
// (-fhip-fp32-correctly-rounded-divide-sqrt) -- so tests/temporal_ref.py, the numpy float32
// restatement, reproduces every output bit.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/rvcp.h"

namespace rvcp {

namespace {

// a pixel takes part when its primary ray hit a non-emissive surface (as rvcp_denoise.hip)
__device__ __forceinline__ bool filterable(float4 g0, float4 g1) {
    return __float_as_uint(g0.w) != RVCP_GBUFFER_MISS &&
           !(__float_as_uint(g1.w) & RVCP_GBUFFER_EMISSIVE);
}

struct v3 { float x, y, z; };

// neither an infinity nor a NaN: the exponent field is not all ones
__device__ __forceinline__ bool finite1(float a) {
    return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u;
}
__device__ __forceinline__ bool finite3(float a, float b, float c) {
    return finite1(a) && finite1(b) && finite1(c);
}

// (a.x b.x + a.y b.y) + a.z b.z, each operation rounded
__device__ __forceinline__ float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// running sums over the accepted taps: sum w, sum w c, the shortest history
struct Sums { float w, r, g, b; uint32_t nmin; };

// One history tap q = (qx, qy) of weight w for the pixel with normal pn, position pp and
// material word pm.  A tap whose position, normal or colour is not finite is rejected as a MISS
// texel is; the length of a rejected tap is not read.
__device__ __forceinline__ void tap(Sums &s, float w, int qx, int qy, uint32_t width,
                                    uint32_t height, v3 pn, v3 pp, uint32_t pm, float normal_min,
                                    float sigma_plane, const float *__restrict__ prev_c,
                                    const float4 *__restrict__ prev_g,
                                    const uint32_t *__restrict__ prev_len)
{
    // unsigned: -1 wraps to 2^32 - 1 >= width, height
    if ((uint32_t)qx >= width || (uint32_t)qy >= height) return;
    const size_t q = (size_t)(uint32_t)qy * width + (uint32_t)qx;
    const float4 q0 = prev_g[2 * q], q1 = prev_g[2 * q + 1];
    if (!filterable(q0, q1) || __float_as_uint(q1.w) != pm) return;
    if (!finite3(q0.x, q0.y, q0.z) || !finite3(q1.x, q1.y, q1.z)) return;
    if (!(dot3(pn, v3{q1.x, q1.y, q1.z}) >= normal_min)) return;
    const float d = dot3(pn, v3{q0.x - pp.x, q0.y - pp.y, q0.z - pp.z});
    if (!(fabsf(d) <= sigma_plane)) return;
    const v3 qc = v3{prev_c[3 * q], prev_c[3 * q + 1], prev_c[3 * q + 2]};
    if (!finite3(qc.x, qc.y, qc.z)) return;
    const uint32_t n = prev_len[q];
    if (n < 1u) return;
    s.w = s.w + w;
    s.r = s.r + w * qc.x;
    s.g = s.g + w * qc.y;
    s.b = s.b + w * qc.z;
    s.nmin = n < s.nmin ? n : s.nmin;
}

constexpr uint32_t kTileX = 64, kTileY = 4;

}  // namespace

// mode: 0 no history, 1 identity (the camera did not move), 2 reprojection through `view`
__global__ __launch_bounds__(kTileX * kTileY) void temporal_kernel(
    const float *__restrict__ cur_c, const float4 *__restrict__ cur_g,
    const float *__restrict__ prev_c, const float4 *__restrict__ prev_g,
    const uint32_t *__restrict__ prev_len, float *__restrict__ out_c,
    uint32_t *__restrict__ out_len, uint32_t width, uint32_t height, uint32_t tiles_x,
    uint32_t mode, rvcp_temporal_view_t view, rvcp_temporal_params_t P)
{
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const uint32_t x = bx * kTileX + (threadIdx.x & (kTileX - 1u));
    const uint32_t y = by * kTileY + (threadIdx.x / kTileX);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const v3 c = v3{cur_c[3 * p], cur_c[3 * p + 1], cur_c[3 * p + 2]};
    const float4 p0 = cur_g[2 * p], p1 = cur_g[2 * p + 1];
    v3 o = c;                                    // no usable history: the current colour
    uint32_t len = 0;                            // a pixel that is not live keeps no history
    // live: filterable, with a finite position, normal and colour
    if (filterable(p0, p1) && finite3(p0.x, p0.y, p0.z) && finite3(p1.x, p1.y, p1.z) &&
        finite3(c.x, c.y, c.z)) {
        len = 1;
        const v3 pp = v3{p0.x, p0.y, p0.z}, pn = v3{p1.x, p1.y, p1.z};
        const uint32_t pm = __float_as_uint(p1.w);
        Sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0xFFFFFFFFu};
        if (mode == 1u) {
            tap(s, 1.0f, (int)x, (int)y, width, height, pn, pp, pm, P.normal_min, P.sigma_plane,
                prev_c, prev_g, prev_len);
        } else if (mode == 2u) {
            const v3 e = v3{pp.x - view.position[0], pp.y - view.position[1], pp.z - view.position[2]};
            const float z = dot3(e, v3{view.forward[0], view.forward[1], view.forward[2]});
            const float a = dot3(e, v3{view.right[0], view.right[1], view.right[2]});
            const float b = dot3(e, v3{view.down[0], view.down[1], view.down[2]});
            const float fw = (float)width, fh = (float)height;
            const float fx = ((a / z) * view.k + 0.5f * fw) - 0.5f;
            const float fy = ((b / z) * view.k + 0.5f * fh) - 0.5f;
            // (a NaN fails every comparison) -- the floats become integers only inside the range
            if (z > 0.0f && fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
                const float xf = floorf(fx), yf = floorf(fy);
                const float tx = fx - xf, ty = fy - yf;
                const int x0 = (int)xf, y0 = (int)yf;
                const float ux = 1.0f - tx, uy = 1.0f - ty;
                tap(s, ux * uy, x0, y0, width, height, pn, pp, pm, P.normal_min, P.sigma_plane,
                    prev_c, prev_g, prev_len);
                tap(s, tx * uy, x0 + 1, y0, width, height, pn, pp, pm, P.normal_min,
                    P.sigma_plane, prev_c, prev_g, prev_len);
                tap(s, ux * ty, x0, y0 + 1, width, height, pn, pp, pm, P.normal_min,
                    P.sigma_plane, prev_c, prev_g, prev_len);
                tap(s, tx * ty, x0 + 1, y0 + 1, width, height, pn, pp, pm, P.normal_min,
                    P.sigma_plane, prev_c, prev_g, prev_len);
            }
        }
        if (s.w > 0.0f) {
            const v3 h = v3{s.r / s.w, s.g / s.w, s.b / s.w};
            // min(nmin + 1, max_history) without the overflow of nmin + 1
            const uint32_t n = s.nmin >= P.max_history ? P.max_history : s.nmin + 1u;
            float alpha = 1.0f / (float)n;
            if (alpha < P.alpha_min) alpha = P.alpha_min;
            o = v3{h.x + alpha * (c.x - h.x), h.y + alpha * (c.y - h.y), h.z + alpha * (c.z - h.z)};
            len = n;
        }
    }
    out_c[3 * p] = o.x;
    out_c[3 * p + 1] = o.y;
    out_c[3 * p + 2] = o.z;
    out_len[p] = len;
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
