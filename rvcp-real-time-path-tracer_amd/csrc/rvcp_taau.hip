// rvcp_taau.hip -- the temporal upsampling step behind rvcp_taa_upsample_async
// (DESIGN.md §4.14).  The reference has no counterpart: it traces every displayed pixel.
//
// One launch per frame, one lane per OUTPUT pixel p of a W x H frame.  The frame was traced at
// w x h = W / s x H / s through a camera rotated by a sub-pixel jitter (rvcp_taa_jitter_push);
// the step keeps a history of the displayed colour and of a float sample weight on the W x H
// grid of the unjittered camera.  Each low-res pixel is one sample that lies where its centre
// direction through the jittered camera falls in the unjittered W x H frame.  The lane visits the
// 3 x 3 low-res pixels around the one over p and sums their colours twice: under a tent of one
// output pixel (`narrow`: what this frame really knows about p) and under a tent of s output
// pixels (`wide`: the bilinear reconstruction, used where there is no history).  The history is
// fetched as the resolve of §4.13 fetches it (identity at rest, else four bilinear taps where the
// two unjittered projections of the W x H G-buffer's primary hit put it), clamped into the colour
// box of the nine taps (not where the low-res pixel lies on the traced frame's border) and
// averaged with the narrow sum by weight: out = (h Wh + Sn) / (Wh + Wn).
//
// Memory: per output pixel the texel's first 16 B when the camera moved and at most four history
// taps of 16 B; 16 B written, 20 B with the fused RGBA8 store; the traced frame adds 12 B per
// TRACED pixel.  A workgroup covers 64 x 4 output pixels (a wave 64 consecutive pixels of a row,
// as §4.13), which lie over at most 32 x 2 traced pixels: it stages the sample positions and the
// clamped colours of those and of the ring around them (at most 34 x 4) in LDS once, one lane
// each, and every lane reads its nine taps from there.  Nine sample positions are six IEEE
// divisions each: the direct form, which recomputes them per lane and reads the colours through
// the caches, is kept behind `force_direct` for tools/taau_time.py's comparison (§4.14 has both
// times); both forms do the same operations on the same values, so their outputs are the same
// bits.
//
// Numeric contract: float32 throughout, every operation rounded once in the
// order written below -- no fma (-ffp-contract=off), IEEE division
// (-fhip-fp32-correctly-rounded-divide-sqrt) -- so tests/taau_ref.py, the numpy float32
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

// §4.13's two selections: a NaN history takes lo
__device__ __forceinline__ float clamp_to(float h, float lo, float hi) {
    const float m = (h >= lo) ? h : lo;
    return (m <= hi) ? m : hi;
}

// 1 - |t| where that is positive, else 0 (a NaN gives 0)
__device__ __forceinline__ float tent(float t) {
    const float u = 1.0f - fabsf(t);
    return (u > 0.0f) ? u : 0.0f;
}

__device__ __forceinline__ v3 load_sat(const float *__restrict__ c, size_t p) {
    return v3{sat(c[3 * p]), sat(c[3 * p + 1]), sat(c[3 * p + 2])};
}

// running sums over the accepted history taps: sum w, sum w c, sum w weight
struct Sums { float w, r, g, b, wt; };

// One history tap q = (qx, qy) of weight w.  The colour of a rejected tap is not read.
__device__ __forceinline__ void tap(Sums &s, float w, int qx, int qy, uint32_t width,
                                    uint32_t height, const float *__restrict__ prev_c,
                                    const float *__restrict__ prev_w)
{
    // unsigned: -1 wraps to 2^32 - 1 >= width, height
    if ((uint32_t)qx >= width || (uint32_t)qy >= height) return;
    const size_t q = (size_t)(uint32_t)qy * width + (uint32_t)qx;
    const float n = prev_w[q];
    if (!(n > 0.0f)) return;                     // (a NaN weight is no history)
    s.w = s.w + w;
    s.r = s.r + w * prev_c[3 * q];
    s.g = s.g + w * prev_c[3 * q + 1];
    s.b = s.b + w * prev_c[3 * q + 2];
    s.wt = s.wt + w * n;
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

// §4.13's miss-pixel mapping: where the centre direction of pixel (x, y) of V's gw x gh grid
// falls in P's fw x fh grid (only the rotation between the two moves it)
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

constexpr uint32_t kTileX = 64, kTileY = 4;
// the staged traced pixels of a tile: kTileX / 2 + 2 columns by kTileY / 2 + 2 rows at scale 2,
// fewer at scales 3 and 4 (the row stride stays)
constexpr uint32_t kStageW = kTileX / 2 + 2, kStageH = kTileY / 2 + 2, kStageN = kStageW * kStageH;
static_assert(kStageN <= kTileX * kTileY, "one lane stages one traced pixel");

// the two tents' sums and the colour box over the taps
struct TapSums { float Wn, Ww; v3 Sn, Sw, lo, hi; };

// One traced pixel of colour c whose sample lies at (sgx, sgy), seen from output pixel (fpx, fpy)
__device__ __forceinline__ void add_tap(TapSums &t, float sgx, float sgy, v3 c, float fpx, float fpy,
                                        float fs)
{
    const float ddx = sgx - fpx, ddy = sgy - fpy;
    const float wn = tent(ddx) * tent(ddy);
    t.Wn = t.Wn + wn;
    t.Sn = v3{t.Sn.x + wn * c.x, t.Sn.y + wn * c.y, t.Sn.z + wn * c.z};
    const float ww = tent(ddx / fs) * tent(ddy / fs);
    t.Ww = t.Ww + ww;
    t.Sw = v3{t.Sw.x + ww * c.x, t.Sw.y + ww * c.y, t.Sw.z + ww * c.z};
    t.lo = v3{fminf(t.lo.x, c.x), fminf(t.lo.y, c.y), fminf(t.lo.z, c.z)};
    t.hi = v3{fmaxf(t.hi.x, c.x), fmaxf(t.hi.y, c.y), fmaxf(t.hi.z, c.z)};
}

}  // namespace

// mode: 0 no history, 1 identity (the camera is at rest), 2 reprojection from `cur` into `prev`.
// width x height is the OUTPUT frame, lw x lh = width / scale x height / scale the traced one.
template <bool LDS>
__global__ __launch_bounds__(kTileX * kTileY) void taa_upsample_kernel(
    const float *__restrict__ cur_c, const float4 *__restrict__ g_hi,
    const float *__restrict__ prev_c, const float *__restrict__ prev_w,
    float *__restrict__ out_c, float *__restrict__ out_w, uint32_t *__restrict__ out_rgba,
    const float *__restrict__ gamma_t, uint32_t width, uint32_t height, uint32_t scale,
    uint32_t tiles_x, uint32_t mode, rvcp_temporal_view_t jit, rvcp_temporal_view_t cur,
    rvcp_temporal_view_t prev, rvcp_taau_params_t P)
{
    const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const uint32_t x = bx * kTileX + (threadIdx.x & (kTileX - 1u));
    const uint32_t y = by * kTileY + (threadIdx.x / kTileX);
    const uint32_t lw = width / scale, lh = height / scale;
    const float fw = (float)width, fh = (float)height, flw = (float)lw, flh = (float)lh;
    // the traced pixel left of and above the tile's first one: staged entry (0, 0); -1 on the
    // frame's first tiles (unsigned: it wraps, and entry + origin wraps back)
    const uint32_t ox = bx * kTileX / scale - 1u, oy = by * kTileY / scale - 1u;
    __shared__ float s_x[LDS ? kStageN : 1], s_y[LDS ? kStageN : 1];
    __shared__ float s_r[LDS ? kStageN : 1], s_g[LDS ? kStageN : 1], s_b[LDS ? kStageN : 1];
    __shared__ uint32_t s_ok[LDS ? kStageN : 1];
    if (LDS) {
        if (threadIdx.x < kStageN) {
            const uint32_t qx = ox + threadIdx.x % kStageW, qy = oy + threadIdx.x / kStageW;
            float sgx = 0.0f, sgy = 0.0f;
            v3 c = v3{0.0f, 0.0f, 0.0f};
            bool ok = false;
            if (qx < lw && qy < lh) {                       // inside the traced frame
                ok = direction_to(jit, (float)qx, (float)qy, flw, flh, cur, fw, fh, sgx, sgy);
                c = load_sat(cur_c, (size_t)qy * lw + qx);
            }
            s_x[threadIdx.x] = sgx;
            s_y[threadIdx.x] = sgy;
            s_r[threadIdx.x] = c.x;
            s_g[threadIdx.x] = c.y;
            s_b[threadIdx.x] = c.z;
            s_ok[threadIdx.x] = ok ? 1u : 0u;
        }
        __syncthreads();
    }
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * width + x;
    const uint32_t lx = x / scale, ly = y / scale;          // the low-res pixel over p
    const float fs = (float)scale, fpx = (float)x, fpy = (float)y;
    // (lx - ox, ly - oy) >= (1, 1) is this pixel's staged entry
    const uint32_t e0 = (ly - oy) * kStageW + (lx - ox);
    const v3 c0 = LDS ? v3{s_r[e0], s_g[e0], s_b[e0]} : load_sat(cur_c, (size_t)ly * lw + lx);
    TapSums t = {0.0f, 0.0f, v3{0.0f, 0.0f, 0.0f}, v3{0.0f, 0.0f, 0.0f}, c0, c0};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (LDS) {
                const uint32_t e = e0 + (uint32_t)(dy * (int)kStageW + dx);
                if (!s_ok[e]) continue;     // outside the traced frame, or behind the camera
                add_tap(t, s_x[e], s_y[e], v3{s_r[e], s_g[e], s_b[e]}, fpx, fpy, fs);
            } else {
                const uint32_t qx = lx + (uint32_t)dx, qy = ly + (uint32_t)dy;
                if (qx >= lw || qy >= lh) continue;         // (unsigned: -1 wraps)
                float sgx, sgy;
                if (!direction_to(jit, (float)qx, (float)qy, flw, flh, cur, fw, fh, sgx, sgy)) continue;
                add_tap(t, sgx, sgy, load_sat(cur_c, (size_t)qy * lw + qx), fpx, fpy, fs);
            }
        }
    }
    const float Wn = t.Wn, Ww = t.Ww;
    const v3 Sn = t.Sn, Sw = t.Sw, lo = t.lo, hi = t.hi;
    Sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (mode == 1u) {
        tap(s, 1.0f, (int)x, (int)y, width, height, prev_c, prev_w);
    } else if (mode == 2u) {
        const float4 g0 = g_hi[2 * p];           // position and face: the texel's first 16 bytes
        float fx, fy;
        bool ok;
        if (__float_as_uint(g0.w) != RVCP_GBUFFER_MISS) {
            const v3 pos = v3{g0.x, g0.y, g0.z};
            float ux, uy, vx, vy;
            const bool oku = project(cur, pos, fw, fh, ux, uy);
            const bool okv = project(prev, pos, fw, fh, vx, vy);
            ok = oku && okv;
            fx = fpx + (vx - ux);
            fy = fpy + (vy - uy);
        } else {
            ok = direction_to(cur, fpx, fpy, fw, fh, prev, fw, fh, fx, fy);
        }
        // (a NaN fails every comparison) -- the floats become integers only inside the range
        if (ok && fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
            const float xf = floorf(fx), yf = floorf(fy);
            const float tx = fx - xf, ty = fy - yf;
            const int x0 = (int)xf, y0 = (int)yf;
            const float ux = 1.0f - tx, uy = 1.0f - ty;
            tap(s, ux * uy, x0, y0, width, height, prev_c, prev_w);
            tap(s, tx * uy, x0 + 1, y0, width, height, prev_c, prev_w);
            tap(s, ux * ty, x0, y0 + 1, width, height, prev_c, prev_w);
            tap(s, tx * ty, x0 + 1, y0 + 1, width, height, prev_c, prev_w);
        }
    }
    v3 o;
    float wt;
    if (s.w > 0.0f) {
        v3 h = v3{s.r / s.w, s.g / s.w, s.b / s.w};
        const float Wh = s.wt / s.w;
        // lx, ly >= 1 and lx + 1 < lw, ly + 1 < lh: all nine low-res pixels are inside the frame
        if (P.clamp == 1u && lx > 0u && lx + 1u < lw && ly > 0u && ly + 1u < lh)
            h = v3{clamp_to(h.x, lo.x, hi.x), clamp_to(h.y, lo.y, hi.y), clamp_to(h.z, lo.z, hi.z)};
        const float Wt = Wh + Wn;
        o = v3{(h.x * Wh + Sn.x) / Wt, (h.y * Wh + Sn.y) / Wt, (h.z * Wh + Sn.z) / Wt};
        wt = (Wt < P.max_weight) ? Wt : P.max_weight;
    } else {
        // no usable history: the wide tent's reconstruction of the current frame
        o = (Ww > 0.0f) ? v3{Sw.x / Ww, Sw.y / Ww, Sw.z / Ww} : c0;
        wt = P.init_weight;
    }
    out_c[3 * p] = o.x;
    out_c[3 * p + 1] = o.y;
    out_c[3 * p + 2] = o.z;
    out_w[p] = wt;
    if (out_rgba) out_rgba[p] = pack_rgb8(o.x, o.y, o.z, gamma_t);
}

}  // namespace rvcp

extern "C" int rvcp_launch_taa_upsample(const float *cur_c, const void *g_hi, const float *prev_c,
                                        const float *prev_w, float *out_c, float *out_w,
                                        uint32_t *out_rgba, const float *gamma_t, uint32_t width,
                                        uint32_t height, uint32_t scale, uint32_t mode,
                                        const rvcp_temporal_view_t *jit_view,
                                        const rvcp_temporal_view_t *cur_view,
                                        const rvcp_temporal_view_t *prev_view,
                                        const rvcp_taau_params_t *params, uint32_t force_direct,
                                        void *stream)
{
    const uint32_t tx = (width + rvcp::kTileX - 1) / rvcp::kTileX;
    const uint32_t ty = (height + rvcp::kTileY - 1) / rvcp::kTileY;
    rvcp_temporal_view_t V = {};
    if (prev_view) V = *prev_view;
    hipLaunchKernelGGL(force_direct ? rvcp::taa_upsample_kernel<false> : rvcp::taa_upsample_kernel<true>,
                       dim3(tx * ty), dim3(rvcp::kTileX * rvcp::kTileY),
                       0, (hipStream_t)stream, cur_c, (const float4 *)g_hi, prev_c, prev_w, out_c,
                       out_w, out_rgba, gamma_t, width, height, scale, tx, mode,
                       *jit_view, *cur_view, V, *params);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
