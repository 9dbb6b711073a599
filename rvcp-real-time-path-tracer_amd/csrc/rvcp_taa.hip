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

#include <stdint.h>

#include "../../include/rvcp.h"
#include "rvcp_tonemap.h"

namespace rvcp {

namespace {

struct v3 { float x, y, z; };

// (a.x b.x + a.y b.y) + a.z b.z, each operation rounded
__device__ __forceinline__ float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ v3 vec(const float a[3]) { return v3{a[0], a[1], a[2]}; }

// gamma_u8's own clamp: the displayed value of a linear channel (a NaN displays as 0)
__device__ __forceinline__ float sat(float c) { return (c > 0.0f) ? ((c < 1.0f) ? c : 1.0f) : 0.0f; }

// min(max(h, lo), hi) written as selections, so that a NaN history takes lo and no rule about
// signed zeros is needed: max(h, lo) = h >= lo ? h : lo, min(m, hi) = m <= hi ? m : hi
__device__ __forceinline__ float clamp_to(float h, float lo, float hi) {
    const float m = (h >= lo) ? h : lo;
    return (m <= hi) ? m : hi;
}

__device__ __forceinline__ v3 load_sat(const float *__restrict__ c, size_t p) {
    return v3{sat(c[3 * p]), sat(c[3 * p + 1]), sat(c[3 * p + 2])};
}

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

// the pixel coordinates of world point x under view V (§4.10's e, z, a, b, fx, fy)
__device__ __forceinline__ bool project(const rvcp_temporal_view_t &V, v3 x, float fw, float fh,
                                        float &fx, float &fy)
{
    const v3 e = v3{x.x - V.position[0], x.y - V.position[1], x.z - V.position[2]};
    const float z = dot3(e, vec(V.forward));
    const float a = dot3(e, vec(V.right));
    const float b = dot3(e, vec(V.down));
    fx = ((a / z) * V.k + 0.5f * fw) - 0.5f;
    fy = ((b / z) * V.k + 0.5f * fh) - 0.5f;
    return z > 0.0f;
}

constexpr uint32_t kTileX = 64, kTileY = 4;

}  // namespace

// mode: 0 no history, 1 identity (the camera is at rest), 2 reprojection from `cur` into `prev`
__global__ __launch_bounds__(kTileX * kTileY) void taa_resolve_kernel(
    const float *__restrict__ cur_c, const float4 *__restrict__ cur_g,
    const float *__restrict__ prev_c, const uint32_t *__restrict__ prev_len,
    float *__restrict__ out_c, uint32_t *__restrict__ out_len, uint32_t *__restrict__ out_rgba,
    const float *__restrict__ gamma_t, uint32_t width, uint32_t height, uint32_t tiles_x,
    uint32_t mode, rvcp_temporal_view_t cur, rvcp_temporal_view_t prev, rvcp_taa_params_t P)
{
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const uint32_t x = bx * kTileX + (threadIdx.x & (kTileX - 1u));
    const uint32_t y = by * kTileY + (threadIdx.x / kTileX);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const v3 c = load_sat(cur_c, p);
    v3 o = c;                                    // no usable history: the displayed current colour
    uint32_t len = 1;
    Sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0xFFFFFFFFu};
    if (mode == 1u) {
        tap(s, 1.0f, (int)x, (int)y, width, height, prev_c, prev_len);
    } else if (mode == 2u) {
        const float fw = (float)width, fh = (float)height;
        const float4 g0 = cur_g[2 * p];          // position and face: the texel's first 16 bytes
        float fx, fy;
        bool ok;
        if (__float_as_uint(g0.w) != RVCP_GBUFFER_MISS) {
            const v3 pos = v3{g0.x, g0.y, g0.z};
            float ux, uy, vx, vy;
            const bool oku = project(cur, pos, fw, fh, ux, uy);
            const bool okv = project(prev, pos, fw, fh, vx, vy);
            ok = oku && okv;
            fx = (float)x + (vx - ux);
            fy = (float)y + (vy - uy);
        } else {
            // the background is at infinity: the pixel's direction through the current camera,
            // projected by the previous one (only the rotation moves it)
            const float ff = dot3(vec(cur.forward), vec(cur.forward));
            const v3 fwd = v3{cur.forward[0] / ff, cur.forward[1] / ff, cur.forward[2] / ff};
            const float sx = (((float)x + 0.5f) - 0.5f * fw) / cur.k;
            const float sy = (((float)y + 0.5f) - 0.5f * fh) / cur.k;
            const v3 d = v3{(fwd.x + sx * cur.right[0]) + sy * cur.down[0],
                            (fwd.y + sx * cur.right[1]) + sy * cur.down[1],
                            (fwd.z + sx * cur.right[2]) + sy * cur.down[2]};
            const float z = dot3(d, vec(prev.forward));
            const float a = dot3(d, vec(prev.right));
            const float b = dot3(d, vec(prev.down));
            ok = z > 0.0f;
            fx = ((a / z) * prev.k + 0.5f * fw) - 0.5f;
            fy = ((b / z) * prev.k + 0.5f * fh) - 0.5f;
        }
        // (a NaN fails every comparison) -- the floats become integers only inside the range
        if (ok && fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
            const float xf = floorf(fx), yf = floorf(fy);
            const float tx = fx - xf, ty = fy - yf;
            const int x0 = (int)xf, y0 = (int)yf;
            const float ux = 1.0f - tx, uy = 1.0f - ty;
            tap(s, ux * uy, x0, y0, width, height, prev_c, prev_len);
            tap(s, tx * uy, x0 + 1, y0, width, height, prev_c, prev_len);
            tap(s, ux * ty, x0, y0 + 1, width, height, prev_c, prev_len);
            tap(s, tx * ty, x0 + 1, y0 + 1, width, height, prev_c, prev_len);
        }
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
    out_c[3 * p] = o.x;
    out_c[3 * p + 1] = o.y;
    out_c[3 * p + 2] = o.z;
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
