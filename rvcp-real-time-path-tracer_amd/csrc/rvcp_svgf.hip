// rvcp_svgf.hip -- spatiotemporal variance-guided filtering behind rvcp_svgf_accumulate_async and
// rvcp_svgf_filter_async (Schied et al.: "Spatiotemporal Variance-Guided Filtering", HPG 2017;
// DESIGN.md §4.11).  The reference has no counterpart (it stores the raw frame,
// ray_tracer_games101_branch.comp:497-500).
//
// Three kinds of kernel, one lane per pixel each:
//   svgf_temporal_kernel   the accumulation step of rvcp_temporal.hip (§4.10; the same taps, the
//     same acceptance rules, the same colour and length bits) which also carries the first two
//     moments of the luminance through the taps: 8 B more per tap and per pixel.
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

#include <stdint.h>

#include "../../include/rvcp.h"

namespace {

// a pixel takes part when its primary ray hit a non-emissive surface (as rvcp_denoise.hip)
__device__ __forceinline__ bool filterable_w(uint32_t face, uint32_t material) {
    return face != RVCP_GBUFFER_MISS && !(material & RVCP_GBUFFER_EMISSIVE);
}
__device__ __forceinline__ bool filterable(float4 g0, float4 g1) {
    return filterable_w(__float_as_uint(g0.w), __float_as_uint(g1.w));
}

struct v3 { float x, y, z; };

// neither an infinity nor a NaN: the exponent field is not all ones
__device__ __forceinline__ bool finite1(float a) {
    return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u;
}
__device__ __forceinline__ bool finite3(float a, float b, float c) {
    return finite1(a) && finite1(b) && finite1(c);
}

// A texel is live for a launch when it is filterable and every float the launch reads from it is
// finite: position and normal here, plus the colour, the moments or the variance
// where a kernel reads them.  Any other texel is treated as a MISS texel.
__device__ __forceinline__ bool live_g(float4 g0, float4 g1) {
    return filterable(g0, g1) && finite3(g0.x, g0.y, g0.z) && finite3(g1.x, g1.y, g1.z);
}

// (a.x b.x + a.y b.y) + a.z b.z, each operation rounded
__device__ __forceinline__ float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// l(c) = (0.2126 r + 0.7152 g) + 0.0722 b, each operation rounded
__device__ __forceinline__ float lum(v3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// w_n = max(0, n_p . n_q), squared npl2 times (§4.9)
__device__ __forceinline__ float weight_n(v3 pn, v3 qn, uint32_t npl2) {
    const float dn = dot3(pn, qn);
    float wn = dn > 0.0f ? dn : 0.0f;
    for (uint32_t i = 0; i < npl2; ++i) wn = wn * wn;
    return wn;
}

// w_z = 1 / (1 + d^2), d = n_p . (pos_q - pos_p) / sigma_plane (§4.9)
__device__ __forceinline__ float weight_z(v3 pn, v3 pp, v3 qp, float sigma_plane) {
    const float d = dot3(pn, v3{qp.x - pp.x, qp.y - pp.y, qp.z - pp.z}) / sigma_plane;
    return 1.0f / (1.0f + d * d);
}

// ---------------------------------------------------------------------------------------------
// A. accumulation with moments
// ---------------------------------------------------------------------------------------------

// running sums over the accepted taps: sum w, sum w c, sum w m, the shortest history
struct HistSums { float w, r, g, b, m1, m2; uint32_t nmin; };

// One history tap q = (qx, qy) of weight w (rvcp_temporal.hip's tap, plus the moments).  A tap
// that is not live (position, normal, colour, moments) is rejected; the length of a rejected tap
// is not read.
__device__ __forceinline__ void hist_tap(HistSums &s, float w, int qx, int qy, uint32_t width,
                                         uint32_t height, v3 pn, v3 pp, uint32_t pm,
                                         float normal_min, float sigma_plane,
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
    if (!(dot3(pn, v3{q1.x, q1.y, q1.z}) >= normal_min)) return;
    const float d = dot3(pn, v3{q0.x - pp.x, q0.y - pp.y, q0.z - pp.z});
    if (!(fabsf(d) <= sigma_plane)) return;
    const v3 qc = v3{prev_c[3 * q], prev_c[3 * q + 1], prev_c[3 * q + 2]};
    const float2 m = prev_m[q];
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

constexpr uint32_t kTileX = 64, kTileY = 4;      // direct kernels: a wave covers 64 pixels of a row

// mode: 0 no history, 1 identity (the camera did not move), 2 reprojection through `view`
__global__ __launch_bounds__(kTileX * kTileY) void svgf_temporal_kernel(
    const float *__restrict__ cur_c, const float4 *__restrict__ cur_g,
    const float *__restrict__ prev_c, const float4 *__restrict__ prev_g,
    const uint32_t *__restrict__ prev_len, const float2 *__restrict__ prev_m,
    float *__restrict__ out_c, uint32_t *__restrict__ out_len, float2 *__restrict__ out_m,
    uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t mode, rvcp_temporal_view_t view,
    rvcp_temporal_params_t P, float alpha_moments_min)
{
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const uint32_t x = bx * kTileX + (threadIdx.x & (kTileX - 1u));
    const uint32_t y = by * kTileY + (threadIdx.x / kTileX);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const v3 c = v3{cur_c[3 * p], cur_c[3 * p + 1], cur_c[3 * p + 2]};
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
        if (mode == 1u) {
            hist_tap(s, 1.0f, (int)x, (int)y, width, height, pn, pp, pm, P.normal_min,
                     P.sigma_plane, prev_c, prev_g, prev_len, prev_m);
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
                hist_tap(s, ux * uy, x0, y0, width, height, pn, pp, pm, P.normal_min,
                         P.sigma_plane, prev_c, prev_g, prev_len, prev_m);
                hist_tap(s, tx * uy, x0 + 1, y0, width, height, pn, pp, pm, P.normal_min,
                         P.sigma_plane, prev_c, prev_g, prev_len, prev_m);
                hist_tap(s, ux * ty, x0, y0 + 1, width, height, pn, pp, pm, P.normal_min,
                         P.sigma_plane, prev_c, prev_g, prev_len, prev_m);
                hist_tap(s, tx * ty, x0 + 1, y0 + 1, width, height, pn, pp, pm, P.normal_min,
                         P.sigma_plane, prev_c, prev_g, prev_len, prev_m);
            }
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
    out_c[3 * p] = o.x;
    out_c[3 * p + 1] = o.y;
    out_c[3 * p + 2] = o.z;
    out_len[p] = len;
    out_m[p] = om;
}

// ---------------------------------------------------------------------------------------------
// B. variance
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kLX = 32, kLY = 8;            // LDS kernels: a 32 x 8 tile

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

// the B3 spline (1/16, 1/4, 3/8, 1/4, 1/16): every product of two entries is exact in f32
__device__ __forceinline__ constexpr float b3(int i) {
    return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f;
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
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const uint32_t x = bx * kTileX + (threadIdx.x & (kTileX - 1u));
    const uint32_t y = by * kTileY + (threadIdx.x / kTileX);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const v3 pc = v3{in_c[3 * p], in_c[3 * p + 1], in_c[3 * p + 2]};
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
                              v3{in_c[3 * q], in_c[3 * q + 1], in_c[3 * q + 2]}, qv)) continue;
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
                const v3 qc = v3{in_c[3 * q], in_c[3 * q + 1], in_c[3 * q + 2]};
                const float qv = in_v[q];
                if (!live(q0, q1, qc, qv)) continue;
                tap(s, b3(dy) * b3(dx), A, den, lp, pn, pp, v3{q1.x, q1.y, q1.z},
                    v3{q0.x, q0.y, q0.z}, qc, qv);
            }
        }
        finish(s, o, ov);
    }
    out_c[3 * p] = o.x;
    out_c[3 * p + 1] = o.y;
    out_c[3 * p + 2] = o.z;
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
            const v3 qc = v3{in_c[3 * q], in_c[3 * q + 1], in_c[3 * q + 2]};
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
    out_c[3 * p] = o.x;
    out_c[3 * p + 1] = o.y;
    out_c[3 * p + 2] = o.z;
    out_v[p] = ov;
}

}  // namespace

extern "C" int rvcp_launch_svgf_temporal(const float *cur_c, const void *cur_g, const float *prev_c,
                                         const void *prev_g, const uint32_t *prev_len,
                                         const float *prev_m, float *out_c, uint32_t *out_len,
                                         float *out_m, uint32_t width, uint32_t height,
                                         uint32_t mode, const rvcp_temporal_view_t *view,
                                         const rvcp_temporal_params_t *params,
                                         float alpha_moments_min, void *stream)
{
    const uint32_t tx = (width + kTileX - 1) / kTileX, ty = (height + kTileY - 1) / kTileY;
    rvcp_temporal_view_t V = {};
    if (view) V = *view;
    hipLaunchKernelGGL(svgf_temporal_kernel, dim3(tx * ty), dim3(kTileX * kTileY), 0,
                       (hipStream_t)stream, cur_c, (const float4 *)cur_g, prev_c,
                       (const float4 *)prev_g, prev_len, (const float2 *)prev_m, out_c, out_len,
                       (float2 *)out_m, width, height, tx, mode, V, *params, alpha_moments_min);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

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
