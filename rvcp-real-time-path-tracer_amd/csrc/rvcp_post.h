// rvcp_post.h -- the device code the post-process kernels share: the
// a-trous filter (rvcp_denoise.hip), the accumulation steps (rvcp_temporal.hip), SVGF
// (rvcp_svgf.hip), the TAA resolve (rvcp_taa.hip) and the temporal upsampling (rvcp_taau.hip);
// albedo demodulation (rvcp_albedo.hip) takes its filterable test from here and nothing else.
// Every rule of their numeric contracts that more than one of them applies is written here once,
// so the kernels cannot drift apart; a new post-process stage starts from this header.
//
// Numeric contract (§4.9-§4.14): float32 throughout, every operation rounded once in the order
// written below -- no fma (-ffp-contract=off), IEEE division
// (-fhip-fp32-correctly-rounded-divide-sqrt) -- so the numpy float32 restatements under tests/
// reproduce every output bit.  The path kernels do not use this header (hipRTC never sees it).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/rvcp.h"

namespace rvcp {

struct v3 { float x, y, z; };

// (a.x b.x + a.y b.y) + a.z b.z, each operation rounded (§4.9)
__device__ __forceinline__ float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ v3 vec(const float a[3]) { return v3{a[0], a[1], a[2]}; }

// l(c) = (0.2126 r + 0.7152 g) + 0.0722 b, each operation rounded (§4.11)
__device__ __forceinline__ float lum(v3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// the colour of pixel p: three dwords
__device__ __forceinline__ v3 load3(const float *c, size_t p) {
    return v3{c[3 * p], c[3 * p + 1], c[3 * p + 2]};
}
__device__ __forceinline__ void store3(float *c, size_t p, v3 o) {
    c[3 * p] = o.x;
    c[3 * p + 1] = o.y;
    c[3 * p + 2] = o.z;
}

// ---------------------------------------------------------------------------------------------
// Which texels take part (§4.9, §4.15)
// ---------------------------------------------------------------------------------------------

// a pixel takes part in a filter when its primary ray hit a non-emissive surface (§4.9); on the
// texel's face and material words, and on its two halves
__device__ __forceinline__ bool filterable_w(uint32_t face, uint32_t material) {
    return face != RVCP_GBUFFER_MISS && !(material & RVCP_GBUFFER_EMISSIVE);
}
__device__ __forceinline__ bool filterable(float4 g0, float4 g1) {
    return filterable_w(__float_as_uint(g0.w), __float_as_uint(g1.w));
}

// neither an infinity nor a NaN: the exponent field is not all ones (§4.15)
__device__ __forceinline__ bool finite1(float a) {
    return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u;
}
__device__ __forceinline__ bool finite3(float a, float b, float c) {
    return finite1(a) && finite1(b) && finite1(c);
}

// A texel is live for a launch when it is filterable and every float the launch reads from it is
// finite (§4.15): position and normal here; a kernel adds the colour, the moments or the variance
// where it reads them.  Any other texel is treated as a MISS texel: as a tap it adds nothing, as
// the centre it passes through.
__device__ __forceinline__ bool live_g(float4 g0, float4 g1) {
    return filterable(g0, g1) && finite3(g0.x, g0.y, g0.z) && finite3(g1.x, g1.y, g1.z);
}

// ---------------------------------------------------------------------------------------------
// The geometric weights of an a-trous tap (§4.9)
// ---------------------------------------------------------------------------------------------

// w_n = max(0, n_p . n_q), squared npl2 times
__device__ __forceinline__ float weight_n(v3 pn, v3 qn, uint32_t npl2) {
    const float dn = dot3(pn, qn);
    float wn = dn > 0.0f ? dn : 0.0f;
    for (uint32_t i = 0; i < npl2; ++i) wn = wn * wn;
    return wn;
}

// w_z = 1 / (1 + d^2), d = n_p . (pos_q - pos_p) / sigma_plane
__device__ __forceinline__ float weight_z(v3 pn, v3 pp, v3 qp, float sigma_plane) {
    const float d = dot3(pn, v3{qp.x - pp.x, qp.y - pp.y, qp.z - pp.z}) / sigma_plane;
    return 1.0f / (1.0f + d * d);
}

// the B3 spline (1/16, 1/4, 3/8, 1/4, 1/16): every product of two entries is exact in f32
__device__ __forceinline__ constexpr float b3(int i) {
    return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f;
}

// ---------------------------------------------------------------------------------------------
// Displayed colours (§4.13)
// ---------------------------------------------------------------------------------------------

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

// ---------------------------------------------------------------------------------------------
// Tiles
// ---------------------------------------------------------------------------------------------

// Kernels that read every tap from memory: workgroup blockIdx.x is tile (bx, by) of a grid
// tiles_x wide, 64 x 4 pixels, so that a wave covers 64 consecutive pixels of a row (§4.9).
constexpr uint32_t kTileX = 64, kTileY = 4;
struct TilePixel { uint32_t bx, by, x, y; };
__device__ __forceinline__ TilePixel tile_pixel(uint32_t tiles_x) {
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    return TilePixel{bx, by, bx * kTileX + (threadIdx.x & (kTileX - 1u)),
                     by * kTileY + (threadIdx.x / kTileX)};
}

// kernels that stage a tile and its halo in LDS: 32 x 8 pixels (§4.9, §4.11)
constexpr uint32_t kLX = 32, kLY = 8;

// ---------------------------------------------------------------------------------------------
// Where a pixel's history lies (§4.10, §4.13)
// ---------------------------------------------------------------------------------------------

// the pixel coordinates of world point x under view V in an fw x fh frame (§4.10's e, z, a, b,
// fx, fy); false behind the camera
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

// §4.13's miss-pixel mapping: where the centre direction of pixel (x, y) of V's gw x gh grid
// falls in P's fw x fh grid (the background is at infinity: only the rotation between the two
// moves it)
__device__ __forceinline__ bool direction_to(const rvcp_temporal_view_t &V, float x, float y,
                                             float gw, float gh, const rvcp_temporal_view_t &P,
                                             float fw, float fh, float &fx, float &fy)
{
    const float ff = dot3(vec(V.forward), vec(V.forward));
    const v3 fwd = v3{V.forward[0] / ff, V.forward[1] / ff, V.forward[2] / ff};
    const float sx = ((x + 0.5f) - 0.5f * gw) / V.k;
    const float sy = ((y + 0.5f) - 0.5f * gh) / V.k;
    const v3 d = v3{(fwd.x + sx * V.right[0]) + sy * V.down[0],
                    (fwd.y + sx * V.right[1]) + sy * V.down[1],
                    (fwd.z + sx * V.right[2]) + sy * V.down[2]};
    const float z = dot3(d, vec(P.forward));
    const float a = dot3(d, vec(P.right));
    const float b = dot3(d, vec(P.down));
    fx = ((a / z) * P.k + 0.5f * fw) - 0.5f;
    fy = ((b / z) * P.k + 0.5f * fh) - 0.5f;
    return z > 0.0f;
}

// The history point of pixel (x, y) of the unjittered fw x fh grid, whose texel begins with g0
// (position and face), when the camera went from `prev` to `cur` (§4.13): a hit pixel moves by
// the difference of its primary hit's two projections, a miss pixel by direction_to.
__device__ __forceinline__ bool history_point(float4 g0, float x, float y,
                                              const rvcp_temporal_view_t &cur,
                                              const rvcp_temporal_view_t &prev, float fw, float fh,
                                              float &fx, float &fy)
{
    if (__float_as_uint(g0.w) == RVCP_GBUFFER_MISS)
        return direction_to(cur, x, y, fw, fh, prev, fw, fh, fx, fy);
    const v3 pos = v3{g0.x, g0.y, g0.z};
    float ux, uy, vx, vy;
    const bool oku = project(cur, pos, fw, fh, ux, uy);
    const bool okv = project(prev, pos, fw, fh, vx, vy);
    fx = x + (vx - ux);
    fy = y + (vy - uy);
    return oku && okv;
}

// The bilinear footprint of history point (fx, fy) in an fw x fh frame (§4.10): nothing unless
// `ok` and -1 <= fx < fw, -1 <= fy < fh (a NaN fails every comparison; the floats become
// integers only inside the range); else tap(w, qx, qy) for the four texels around the point, in
// this order.  The tap itself rejects a texel outside the frame.
template <typename Tap>
__device__ __forceinline__ void bilinear_taps(bool ok, float fx, float fy, float fw, float fh,
                                              Tap tap)
{
    if (!(ok && fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh)) return;
    const float xf = floorf(fx), yf = floorf(fy);
    const float tx = fx - xf, ty = fy - yf;
    const int x0 = (int)xf, y0 = (int)yf;
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    tap(ux * uy, x0, y0);
    tap(tx * uy, x0 + 1, y0);
    tap(ux * ty, x0, y0 + 1);
    tap(tx * ty, x0 + 1, y0 + 1);
}

}  // namespace rvcp
