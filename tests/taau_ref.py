"""taau_ref -- numpy float32 restatement of the temporal upsampling step behind
rvcp_taa_upsample_async and of the state the two stateful chains keep for it, a generator of
synthetic inputs and the measurement of the upsampling gates (TEST
INFRASTRUCTURE ONLY: never imported by the package).

It shares no code with csrc/rvcp_taau.hip, only the contract: float32 throughout, every operation
rounded once, in the order DESIGN.md §4.14 writes them; the nine low-res taps visited dy outer, dx
inner, a tap outside the traced frame or behind the camera adding nothing; the history taps in
the order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).  numpy evaluates each array
operation in float32 with one rounding and never fuses, so the kernel's output is reproduced bit
for bit.  taa_ref's clamp `sat`, its `history_coords` and temporal_ref's views are reused by
import.
"""
from __future__ import annotations

import numpy as np

import taa_ref as A
import temporal_ref as T
from denoise_ref import GBUFFER_DTYPE, MISS

F = np.float32
PARAMS_DTYPE = np.dtype([("max_weight", "<f4"), ("init_weight", "<f4"), ("clamp", "<u4"),
                         ("_pad", "<u4")])


def params(max_weight=8.0, init_weight=0.1, clamp=1):
    p = np.zeros((), dtype=PARAMS_DTYPE)
    p["max_weight"], p["init_weight"], p["clamp"] = max_weight, init_weight, clamp
    return p


# ------------------------------------------------------------------------ the step
def sample_positions(jit_view, cur_view, w, h, W, H):
    """Where the centre direction of every pixel of the traced w x h frame (camera jit_view) falls
    in the W x H frame of cur_view: (fx, fy, ok) float32 / bool [h, w]; ok is false where z <= 0
    or NaN.  §4.13's miss-pixel mapping on two grids."""
    ys, xs = np.mgrid[0:h, 0:w]
    xf, yf = xs.astype(F), ys.astype(F)
    V, P = jit_view, cur_view
    with np.errstate(all="ignore"):
        vf = V["forward"].astype(F)
        ff = (vf[0] * vf[0] + vf[1] * vf[1]) + vf[2] * vf[2]
        fwd = vf / ff
        k = F(V["k"])
        sx = ((xf + F(0.5)) - F(0.5) * F(w)) / k
        sy = ((yf + F(0.5)) - F(0.5) * F(h)) / k
        r, dn = V["right"].astype(F), V["down"].astype(F)
        d = [(fwd[i] + sx * r[i]) + sy * dn[i] for i in range(3)]
        pf, pr, pd = (P[n].astype(F) for n in ("forward", "right", "down"))
        z = (d[0] * pf[0] + d[1] * pf[1]) + d[2] * pf[2]
        a = (d[0] * pr[0] + d[1] * pr[1]) + d[2] * pr[2]
        b = (d[0] * pd[0] + d[1] * pd[1]) + d[2] * pd[2]
        pk = F(P["k"])
        fx = ((a / z) * pk + F(0.5) * F(W)) - F(0.5)
        fy = ((b / z) * pk + F(0.5) * F(H)) - F(0.5)
        ok = z > 0
    assert fx.dtype == F and fy.dtype == F
    return fx, fy, ok


def _tent(t):
    u = F(1) - np.abs(t)
    return np.where(u > 0, u, F(0)).astype(F)


def upsample(c, scale, jit_view, cur_view, prev_view, g_hi, prev_res, prev_wt, p, want_info=False):
    """One step: c [h, w, 3] float32 is the frame traced through jit_view; the output is
    [h * scale, w * scale].  cur_view / prev_view: VIEW_DTYPE records of the unjittered cameras at
    the output size (prev_view None or byte-equal to cur_view: the identity mapping); g_hi: the
    output-size G-buffer, read only when the camera moved; prev_res [H, W, 3] and prev_wt [H, W]
    float32 (both None: no history); p: a PARAMS_DTYPE record.  Returns (out, weight) [, a dict:
    `ncontrib` narrow contributions per pixel, `Wn`, `ntaps` accepted history taps, `has`,
    `clamped`, `changed` where the clamp changed h, `lo`, `hi`, `h`, `Wh`, `cur`]."""
    c = np.ascontiguousarray(c, dtype=F)
    s = int(scale)
    h, w = c.shape[:2]
    H, W = h * s, w * s
    cs = A.sat(c)
    sgx, sgy, sok = sample_positions(jit_view, cur_view, w, h, W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    lx, ly = xs // s, ys // s
    fpx, fpy, fs = xs.astype(F), ys.astype(F), F(s)
    c0 = cs[ly, lx]
    lo, hi = c0.copy(), c0.copy()
    Wn, Ww = np.zeros((H, W), dtype=F), np.zeros((H, W), dtype=F)
    Sn, Sw = np.zeros((H, W, 3), dtype=F), np.zeros((H, W, 3), dtype=F)
    ncontrib = np.zeros((H, W), dtype=np.int64)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                qx, qy = lx + dx, ly + dy
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                Q = (np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1))
                use = inside & sok[Q]
                cq = cs[Q]
                ddx, ddy = sgx[Q] - fpx, sgy[Q] - fpy
                wn = _tent(ddx) * _tent(ddy)
                ww = _tent(ddx / fs) * _tent(ddy / fs)
                assert wn.dtype == F and ww.dtype == F
                Wn = np.where(use, Wn + wn, Wn)
                Sn = np.where(use[..., None], Sn + wn[..., None] * cq, Sn)
                Ww = np.where(use, Ww + ww, Ww)
                Sw = np.where(use[..., None], Sw + ww[..., None] * cq, Sw)
                lo = np.where(use[..., None], np.minimum(lo, cq), lo)
                hi = np.where(use[..., None], np.maximum(hi, cq), hi)
                ncontrib += use & (wn > 0)
        cur = np.where((Ww > 0)[..., None], Sw / Ww[..., None], c0).astype(F)
    # ---- the history
    wsum, wacc = np.zeros((H, W), dtype=F), np.zeros((H, W), dtype=F)
    acc = np.zeros((H, W, 3), dtype=F)
    ntaps = np.zeros((H, W), dtype=np.int64)
    taps = []
    if prev_res is not None:
        prev_res = np.ascontiguousarray(prev_res, dtype=F)
        prev_wt = np.ascontiguousarray(prev_wt, dtype=F)
        identity = prev_view is None or \
            np.asarray(cur_view).tobytes() == np.asarray(prev_view).tobytes()
        if identity:
            taps = [(xs, ys, np.ones((H, W), dtype=F), np.ones((H, W), dtype=bool))]
        else:
            fx, fy, ok = A.history_coords(g_hi, cur_view, prev_view)
            with np.errstate(all="ignore"):
                ok = ok & (fx >= F(-1)) & (fx < F(W)) & (fy >= F(-1)) & (fy < F(H))
                x0f, y0f = np.floor(fx), np.floor(fy)
                tx, ty = fx - x0f, fy - y0f
                ux, uy = F(1) - tx, F(1) - ty
                x0 = np.where(ok, x0f, F(0)).astype(np.int64)      # float -> int inside the range
                y0 = np.where(ok, y0f, F(0)).astype(np.int64)
                taps = [(x0, y0, ux * uy, ok), (x0 + 1, y0, tx * uy, ok),
                        (x0, y0 + 1, ux * ty, ok), (x0 + 1, y0 + 1, tx * ty, ok)]
    with np.errstate(all="ignore"):
        for qx, qy, tw, ok in taps:
            assert tw.dtype == F
            inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            Q = (np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1))
            n = prev_wt[Q]
            a = inside & (n > 0)                                   # (a NaN weight is not > 0)
            wsum = np.where(a, wsum + tw, wsum)
            acc = np.where(a[..., None], acc + tw[..., None] * prev_res[Q], acc)
            wacc = np.where(a, wacc + tw * n, wacc)
            ntaps += a
        has = wsum > 0
        hh = (acc / wsum[..., None]).astype(F)
        Wh = (wacc / wsum).astype(F)
        interior = (lx > 0) & (lx + 1 < w) & (ly > 0) & (ly + 1 < h)
        clamped = interior & (int(p["clamp"]) == 1)
        m = np.where(hh >= lo, hh, lo)                             # a NaN history takes lo
        hc = np.where(m <= hi, m, hi)
        h2 = np.where(clamped[..., None], hc, hh).astype(F)
        Wt = Wh + Wn
        blend = (h2 * Wh[..., None] + Sn) / Wt[..., None]
        assert blend.dtype == F and Wt.dtype == F
        mw = F(p["max_weight"])
        wt_h = np.where(Wt < mw, Wt, mw).astype(F)
    out = np.ascontiguousarray(np.where(has[..., None], blend, cur), dtype=F)
    weight = np.ascontiguousarray(np.where(has, wt_h, F(p["init_weight"])), dtype=F)
    if not want_info:
        return out, weight
    changed = has & clamped & np.any(h2.view(np.uint32) != hh.view(np.uint32), axis=-1)
    return out, weight, dict(ncontrib=ncontrib, Wn=Wn, ntaps=ntaps, has=has, clamped=clamped,
                             interior=interior, changed=changed, lo=lo, hi=hi, h=h2, Wh=Wh, cur=cur)


class Chain:
    """The upsampling state of one stateful chain (rvcp_render_temporal / rvcp_render_svgf with
    the scale above 1), restated: feed it every frame's final linear colour at the traced size,
    the view it was traced through, the caller's unjittered push and -- on the frames whose camera
    moved -- the output-size G-buffer through that push (a callable is only called then)."""

    def __init__(self, scale):
        self.scale = int(scale)
        self.reset()

    def reset(self):
        self.res = self.wt = self.push = self.view = None
        self.counter = 0

    def moved(self, push):
        return self.res is not None and \
            np.asarray(push)["camera"].tobytes() != np.asarray(self.push)["camera"].tobytes()

    def step(self, c, jit_view, push, g_hi=None, p=None):
        H = c.shape[0] * self.scale
        view = T.view_of_push(np.asarray(push).reshape(()), H)
        moved = self.moved(push)
        if moved and callable(g_hi):
            g_hi = g_hi()
        out, wt = upsample(c, self.scale, jit_view, view, self.view if moved else None,
                           g_hi if moved else None, self.res, self.wt, params() if p is None else p)
        self.res, self.wt, self.push, self.view = out, wt, np.array(push), view
        self.counter += 1
        return out, wt


# ------------------------------------------------------------------------ synthetic inputs
MIX_MIN_PIXELS = A.MIX_MIN_PIXELS
NARROW_MIN_SIDE = 8         # traced rows and columns below which the narrow tent's shares are not asserted
ZOOM = 1.1                  # the synthetic traced camera's focal length over cur_view's / scale


def derived_view(view, scale, jitter=(0.0, 0.0), zoom=1.0, flip=False):
    """A VIEW_DTYPE record for the traced frame made from the output camera `view`: k / scale x
    zoom, the forward turned by `jitter` traced pixels towards right / down (float64, rounded
    once); flip: the camera looks backwards (every sample lies behind the output camera)."""
    v = np.zeros((), dtype=T.VIEW_DTYPE)
    r, d, f = (view[n].astype(np.float64) for n in ("right", "down", "forward"))
    k = float(view["k"]) / scale * zoom
    fl = 1.0 / np.linalg.norm(f)                    # forward is f / |f|^2
    n = f * fl + r * (jitter[0] / k) + d * (jitter[1] / k)
    n = n / np.linalg.norm(n)
    if flip:
        n = -n
    r2 = np.cross(n, -d)
    r2 = r2 / np.linalg.norm(r2)
    d2 = np.cross(n, r2)
    v["position"], v["k"], v["right"] = view["position"], k, r2
    v["down"], v["forward"] = d2 / np.linalg.norm(d2), n / fl
    return v


def synthetic_case(W, H, scale, seed, p=None, jitter=(0.31, -0.17), zoom=ZOOM):
    """Inputs of one step at output W x H: (c, jit_view, cur_view, prev_view, g_hi, prev_res,
    prev_wt).  The two output cameras, the output-size G-buffer (hit and miss pixels, targets
    behind either camera, histories carried off the frame, wiped tap footprints) and the texels
    without a history are taa_ref.synthetic_case's; a texel without a history gets the weight 0
    or NaN, the others weights from 0.05 to 2 max_weight.  The traced frame is cut into blocks of
    6 x 6 low-res pixels, half of them flat (one colour plus a little noise: a narrow box), half
    noisy over [-0.5, 1.6], about 1 % NaN (and one channel of each kind
    set by hand, for the small frames); the history is the displayed traced colour of the
    low-res pixel over each output pixel plus noise of deviation 0.15, clipped to [0, 1].  The
    traced camera is the current output camera turned by `jitter` traced pixels, its focal length
    `zoom` times that of a frame scale times smaller: with zoom > 1 the samples lie closer than
    `scale` output pixels, so that some output pixels see two of them under the narrow tent and
    those towards the frame's border none.

    On frames of at least MIX_MIN_PIXELS output pixels and two traced rows and columns the
    generator asserts its own mix with `p` (default: the library's defaults); the two shares of
    the narrow tent only where the traced frame has at least NARROW_MIN_SIDE rows and columns (a
    thinner one is nearly all border, and the zoom carries the samples of a long one out of their
    3 x 3 neighbourhoods): >= 10 % of the output pixels with Wn == 0; at scale 2, >= 10 % with two or more narrow contributions (the
    narrow tent is two output pixels wide, so on a camera's regular grid of samples `scale`
    / zoom >= 2 apart no pixel can see two of them along either axis: at scales 3 and 4 the share
    is 0 by geometry for every zoom that keeps the samples near their own traced pixels, and the
    generator asserts only that it is below 10 %); >= 20 % with four accepted history taps, >= 10 %
    with one to three, >= 10 % with none; where at least 64 clamped pixels have a history, the
    clamp changes h on 20-80 % of them; colours below 0, inside [0, 1], above 1 and NaN; history
    weights 0, below and above max_weight, and NaN; targets behind either camera."""
    rng = np.random.default_rng(seed + 7919 * scale)
    p = params() if p is None else p
    s = int(scale)
    assert W % s == 0 and H % s == 0
    w, h = W // s, H // s
    _, g_hi, _, prev_len, cur_view, prev_view = A.synthetic_case(W, H, seed)
    jit_view = derived_view(cur_view, s, jitter, zoom)
    # ---- colours of the traced frame
    ys, xs = np.mgrid[0:h, 0:w]
    b = 6
    nby, nbx = (h + b - 1) // b, (w + b - 1) // b
    flat = ((ys // b + xs // b) % 2 == 0)[..., None]
    base = rng.uniform(-0.3, 1.5, (nby, nbx, 3))[ys // b, xs // b]
    c = np.where(flat, base + rng.uniform(-0.05, 0.05, (h, w, 3)), rng.uniform(-0.5, 1.6, (h, w, 3)))
    c = np.where(rng.random((h, w, 3)) < 0.01, np.nan, c).astype(F)
    # (a small frame gets one channel of each kind by hand)
    c[0, 0], c[-1, -1, 0] = (-0.25, 0.5, 1.3), np.nan
    Ys, Xs = np.mgrid[0:H, 0:W]
    prev_res = np.clip(A.sat(c)[Ys // s, Xs // s] + rng.normal(0.0, 0.15, (H, W, 3)), 0.0, 1.0).astype(F)
    # ---- history weights
    mw = float(p["max_weight"])
    prev_wt = rng.uniform(0.05, 2.0 * mw, (H, W)).astype(F)
    none = prev_len == 0
    prev_wt = np.where(none, np.where(rng.random((H, W)) < 0.5, np.nan, 0.0), prev_wt).astype(F)
    # ---- the mix
    if W * H >= MIX_MIN_PIXELS and min(w, h) >= 2:
        _, _, info = upsample(c, s, jit_view, cur_view, prev_view, g_hi, prev_res, prev_wt, p, True)
        if min(w, h) >= NARROW_MIN_SIDE:
            assert np.mean(info["Wn"] == 0) >= 0.1, np.mean(info["Wn"] == 0)
            two = np.mean(info["ncontrib"] >= 2)
            assert two >= 0.1 if s == 2 else two < 0.1, two
        share = np.bincount(info["ntaps"].ravel(), minlength=5) / info["ntaps"].size
        assert share[4] >= 0.2 and share[1:4].sum() >= 0.1 and share[0] >= 0.1, share
        ch = info["clamped"] & info["has"]
        if int(p["clamp"]) == 1 and np.count_nonzero(ch) >= 64:
            frac = np.count_nonzero(info["changed"]) / np.count_nonzero(ch)
            assert 0.2 <= frac <= 0.8, frac
        with np.errstate(invalid="ignore"):
            assert (c < 0).any() and ((c >= 0) & (c <= 1)).any() and (c > 1).any()
            assert np.isnan(c).any() and (w * h < MIX_MIN_PIXELS or np.isnan(c).mean() < 0.05)
            assert (prev_wt == 0).any() and np.isnan(prev_wt).any()
            assert ((prev_wt > 0) & (prev_wt < mw)).any() and (prev_wt > mw).any()
        hit = g_hi["face"] != MISS
        assert (A._project(prev_view, g_hi["position"], W, H)[2][hit] < 0).any()
        assert (A._project(cur_view, g_hi["position"], W, H)[2][hit] < 0).any()
    return c, jit_view, cur_view, prev_view, g_hi, prev_res, prev_wt


# ------------------------------------------------------------------------ the upsampling gates
GATE_FRAMES = 16
GATE_SCALE = 2


def wide_tent(c, scale, base_push):
    """Comparator A: one centred traced frame put through the step with no history -- the wide
    tent, which is the bilinear upscaling."""
    h = c.shape[0]
    push = np.asarray(base_push).reshape(())
    return upsample(c, scale, T.view_of_push(push, h), T.view_of_push(push, h * scale), None, None,
                    None, None, params())[0]


def rmse(a, truth, mask=None):
    d = np.asarray(a, dtype=np.float64) - truth
    if mask is not None:
        d = d[mask]
    return float(np.sqrt(np.mean(d * d)))


def flat_gate(w, h, base, materials, gbuffer_of, scale=GATE_SCALE):
    """The flat-shade gate's measurement: gbuffer_of(push, w, h) is the G-buffer of the scene
    through `push` at w x h.  GATE_FRAMES jittered traced frames of taa_ref.flat_shade, upsampled
    at the defaults with the camera at rest, against box4 of the clamped shade at 4 W x 4 H.
    Comparator A is wide_tent of one centred traced frame, comparator B one centred W x H frame.
    Returns the edge / all-pixel RMSEs of the three and ratio_edge, ratio_all = resolved / A."""
    W, H = w * scale, h * scale
    base = np.asarray(base).reshape(())
    hi = gbuffer_of(base, 4 * W, 4 * H)
    truth = A.box4(A.sat(A.flat_shade(hi, materials)))
    edge = A.edge_pixels(hi["face"])
    comp_a = wide_tent(A.flat_shade(gbuffer_of(base, w, h), materials), scale, base)
    comp_b = A.sat(A.flat_shade(gbuffer_of(base, W, H), materials))
    chain = Chain(scale)
    for i in range(GATE_FRAMES):
        jp = A.jittered_push(base, h, i)
        out, _ = chain.step(A.flat_shade(gbuffer_of(jp, w, h), materials), T.view_of_push(jp, h), base)
    r = dict(n_edge=int(edge.sum()), n=int(edge.size))
    for name, img in (("a", comp_a), ("b", comp_b), ("resolved", out)):
        r["edge_" + name], r["all_" + name] = rmse(img, truth, edge), rmse(img, truth)
    r["ratio_edge"] = r["edge_resolved"] / r["edge_a"]
    r["ratio_all"] = r["all_resolved"] / r["all_a"]
    return r


# The flat-shade gate: the Cornell box from the default camera traced at
# 20 x 14, output 40 x 28, 16 frames at rest on denoise_ref.cpu_gbuffer -- measured with this
# restatement by
#   python -m pytest tests/test_taau_cpu.py -m slow -k flat_shade_gate -s
# edge (289 of 1120 pixels): rmse A 0.1287, B (one centred 40 x 28 frame) 0.1295, resolved 0.0650;
# all pixels: A 0.0772, B 0.0658, resolved 0.0353
RATIO_MEASURED = dict(ratio_edge=0.505, ratio_all=0.458)
# The path-traced gate: rvcp_render_svgf at output 128 x 128, scale 2 (traced at 64 x 64), SPP 4,
# 16 frames (time seeds 5.0 + i) against box4 of the clamped plain render at 512 x 512, SPP 128;
# the comparator is rvcp_render_svgf at 64 x 64 with both switches off, upscaled by wide_tent --
# (all-pixel rmse comparator, all-pixel rmse on, edge rmse comparator, edge rmse on) as measured on
# the MI355X by
#   python -m pytest tests/test_gpu_taau.py -k path_traced_gate -s
PATH_MEASURED = (0.0351, 0.0275, 0.0680, 0.0376)    # ratios 0.783 (all), 0.554 (1723 edge pixels)
# (rvcp_render_svgf at 128 x 128 with TAA on and scale 1, four times the rays: 0.0181, 0.0275)
