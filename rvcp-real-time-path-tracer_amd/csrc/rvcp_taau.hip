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

#include "rvcp_post.h"
#include "rvcp_tonemap.h"

namespace rvcp {

namespace {

// 1 - |t| where that is positive, else 0 (a NaN gives 0)
__device__ __forceinline__ float tent(float t) {
    const float u = 1.0f - fabsf(t);
    return (u > 0.0f) ? u : 0.0f;
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
    const auto [bx, by, x, y] = tile_pixel(tiles_x);
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
    const auto hist = [&](float w, int qx, int qy) {
        tap(s, w, qx, qy, width, height, prev_c, prev_w);
    };
    if (mode == 1u) {
        hist(1.0f, (int)x, (int)y);
    } else if (mode == 2u) {
        float fx, fy;
        // g_hi[2 * p]: position and face, the texel's first 16 bytes
        const bool ok = history_point(g_hi[2 * p], fpx, fpy, cur, prev, fw, fh, fx, fy);
        bilinear_taps(ok, fx, fy, fw, fh, hist);
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
    store3(out_c, p, o);
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
