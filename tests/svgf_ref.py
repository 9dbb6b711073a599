"""svgf_ref -- numpy float32 restatement of SVGF as DESIGN.md §4.11 defines it: the accumulation
with luminance moments (A), the per-pixel variance estimate (B), the variance-guided a-trous
passes (C) and the stateful chain of rvcp_render_svgf with and without feedback (TEST
INFRASTRUCTURE ONLY: never imported by the package).

It shares no code with csrc/rvcp_svgf.hip, only the contract: float32 throughout, every
operation rounded once in the order §4.11 writes them, taps in the written order, skipped taps
add nothing, and a texel that is not live for a launch (§4.15) is a MISS texel.  numpy evaluates each array operation in float32 with one rounding and never fuses,
so the kernels' outputs are reproduced bit for bit.
"""
from __future__ import annotations

import numpy as np

from denoise_ref import GBUFFER_DTYPE, KERNEL, filterable, live  # noqa: F401
import temporal_ref as T

F = np.float32
PARAMS_DTYPE = np.dtype([("iterations", "<u4"), ("normal_power_log2", "<u4"),
                         ("sigma_luminance", "<f4"), ("sigma_plane", "<f4"),
                         ("epsilon", "<f4"), ("alpha_moments_min", "<f4"),
                         ("spatial_below", "<u4"), ("_pad", "<u4")])
FEEDBACK = 1
DEFAULTS = dict(iterations=3, normal_power_log2=7, sigma_luminance=1.0, sigma_plane=0.1,
                epsilon=1.0e-4, alpha_moments_min=0.05, spatial_below=4)
# luminance weights and the 3 x 3 variance prefilter (all products by a power of two are exact)
LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)
GAUSS3 = ((F(1 / 16), F(1 / 8), F(1 / 16)), (F(1 / 8), F(1 / 4), F(1 / 8)),
          (F(1 / 16), F(1 / 8), F(1 / 16)))


def params(**kw):
    p = np.zeros((), dtype=PARAMS_DTYPE)
    for k, v in dict(DEFAULTS, **kw).items():
        p[k] = v
    return p


def _dot3(a, b):
    """(a0 b0 + a1 b1) + a2 b2, every operation rounded to float32."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def lum(c):
    """l(c) = (0.2126 r + 0.7152 g) + 0.0722 b, every operation rounded to float32."""
    return (LR * c[..., 0] + LG * c[..., 1]) + LB * c[..., 2]


def _shift(H, W, oy, ox):
    """The slices (P, Q) of the pixels p whose tap q = p + (ox, oy) lies inside the frame."""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _geometry_weight(nrm, pos, P, Q, npl2, sp):
    """(w_n, w_z) of §4.9 for the taps Q of the pixels P."""
    dn = _dot3(nrm[P], nrm[Q])
    wn = np.where(dn > 0, dn, F(0)).astype(F)
    for _ in range(int(npl2)):
        wn = wn * wn
    d = _dot3(nrm[P], pos[Q] - pos[P]) / sp
    wz = F(1) / (F(1) + d * d)
    return wn, wz


# ------------------------------------------------------------------------ A. accumulation
def accumulate(c, g, prev_c, prev_g, prev_len, prev_m, view, tp, sp):
    """One step with moments: the current colour c [H, W, 3] and texels g [H, W]; the history
    prev_c, prev_g, prev_len [H, W] uint32 and prev_m [H, W, 2] (all None: no history); view: the
    previous camera's VIEW_DTYPE record or None for the identity mapping; tp / sp: temporal and
    SVGF parameter records.  Returns (colour, length, moments)."""
    c = np.ascontiguousarray(c, dtype=F)
    H, W = c.shape[:2]
    filt = live(g, c)                  # §4.15: any other texel is a MISS texel, here and below
    pos, nrm, mat = g["position"], g["normal"], g["material"]
    with np.errstate(all="ignore"):
        l1 = lum(c)
        mu = np.stack([l1, l1 * l1], axis=-1)
    assert mu.dtype == F
    wsum = np.zeros((H, W), dtype=F)
    sc = np.zeros((H, W, 3), dtype=F)
    sm = np.zeros((H, W, 2), dtype=F)
    nmin = np.full((H, W), 1 << 40, dtype=np.int64)
    taps = []
    if prev_c is not None:
        prev_c = np.ascontiguousarray(prev_c, dtype=F)
        prev_m = np.ascontiguousarray(prev_m, dtype=F)
        ys, xs = np.mgrid[0:H, 0:W]
        if view is None:
            taps = [(xs, ys, np.ones((H, W), dtype=F), np.ones((H, W), dtype=bool))]
        else:
            fx, fy, _, ok = T.project(view, pos, W, H)
            with np.errstate(all="ignore"):
                xf, yf = np.floor(fx), np.floor(fy)
                tx, ty = fx - xf, fy - yf
                ux, uy = F(1) - tx, F(1) - ty
                x0 = np.where(ok, xf, F(0)).astype(np.int64)
                y0 = np.where(ok, yf, F(0)).astype(np.int64)
            taps = [(x0, y0, ux * uy, ok), (x0 + 1, y0, tx * uy, ok),
                    (x0, y0 + 1, ux * ty, ok), (x0 + 1, y0 + 1, tx * ty, ok)]
    s_plane, n_min = F(tp["sigma_plane"]), F(tp["normal_min"])
    with np.errstate(all="ignore"):
        for qx, qy, w, ok in taps:
            inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            Q = (np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1))
            gq = prev_g[Q]
            a = inside & filt & live(gq, prev_c[Q], prev_m[Q]) & (gq["material"] == mat)
            a &= _dot3(nrm, gq["normal"]) >= n_min
            a &= np.abs(_dot3(nrm, gq["position"] - pos)) <= s_plane
            lq = prev_len[Q].astype(np.int64)
            a &= lq >= 1
            wsum = np.where(a, wsum + w, wsum)
            sc = np.where(a[..., None], sc + w[..., None] * prev_c[Q], sc)
            sm = np.where(a[..., None], sm + w[..., None] * prev_m[Q], sm)
            nmin = np.where(a, np.minimum(nmin, lq), nmin)
        has = filt & (wsum > 0)
        n = np.minimum(nmin + 1, int(tp["max_history"]))
        inv = F(1) / n.astype(F)
        alpha = np.where(inv < F(tp["alpha_min"]), F(tp["alpha_min"]), inv).astype(F)
        am = np.where(inv < F(sp["alpha_moments_min"]), F(sp["alpha_moments_min"]), inv).astype(F)
        hc = sc / wsum[..., None]
        hm = sm / wsum[..., None]
        bc = hc + alpha[..., None] * (c - hc)
        bm = hm + am[..., None] * (mu - hm)
        assert bc.dtype == F and bm.dtype == F
    out = np.ascontiguousarray(np.where(has[..., None], bc, c), dtype=F)
    mom = np.where(has[..., None], bm, mu)
    mom = np.ascontiguousarray(np.where(filt[..., None], mom, F(0)), dtype=F)
    length = np.where(filt, np.where(has, n, 1), 0).astype(np.uint32)
    return out, length, mom


# ------------------------------------------------------------------------ B. variance
def variance_live(m, length, g):
    """The live texels of the variance launch (§4.15): filterable, a finite position, normal and
    moments, and a history of at least one frame -- the accumulation leaves length 0 and zero
    moments on a texel that was not live for it."""
    ok = live(g, m)
    return ok if length is None else ok & (np.asarray(length) >= 1)


def spatial_variance(m, g, sp, length=None):
    """The unboosted 7 x 7 estimate of every live pixel over its live taps (0 elsewhere);
    length None: every history counts as at least one frame long."""
    m = np.ascontiguousarray(m, dtype=F)
    H, W = m.shape[:2]
    filt, pos, nrm = variance_live(m, length, g), g["position"], g["normal"]
    ws = np.zeros((H, W), dtype=F)
    a1 = np.zeros((H, W), dtype=F)
    a2 = np.zeros((H, W), dtype=F)
    with np.errstate(all="ignore"):
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                PQ = _shift(H, W, dy, dx)
                if PQ is None:
                    continue
                P, Q = PQ
                valid = filt[P] & filt[Q]
                wn, wz = _geometry_weight(nrm, pos, P, Q, sp["normal_power_log2"], F(sp["sigma_plane"]))
                w = wn * wz
                ws[P] = np.where(valid, ws[P] + w, ws[P])
                a1[P] = np.where(valid, a1[P] + w * m[Q][..., 0], a1[P])
                a2[P] = np.where(valid, a2[P] + w * m[Q][..., 1], a2[P])
        e1, e2 = a1 / ws, a2 / ws
        v = e2 - e1 * e1
        v = np.where(v > 0, v, F(0))
    # weights that sum to nothing (a zero normal): no estimate
    return np.where(filt & (ws > 0), v, F(0)).astype(F)


def variance(m, length, g, sp):
    """v [H, W]: the temporal estimate where the history is at least spatial_below long, the
    boosted 7 x 7 estimate below that, 0 on a pixel that is not live."""
    m = np.ascontiguousarray(m, dtype=F)
    filt = variance_live(m, length, g)
    below = int(sp["spatial_below"])
    with np.errstate(all="ignore"):
        vt = m[..., 1] - m[..., 0] * m[..., 0]
        vt = np.where(vt > 0, vt, F(0)).astype(F)
        short = filt & (length < below)
        v = vt
        if short.any():
            boost = F(below) / length.astype(F)
            vs = spatial_variance(m, g, sp, length) * boost
            assert vs.dtype == F
            v = np.where(short, vs, vt)
    return np.where(filt, v, F(0)).astype(F)


# ------------------------------------------------------------------------ C. guided a-trous
def prefilter(v, g, c=None):
    """vbar: the 3 x 3 Gaussian of v at distance 1 over the live taps inside the frame (live for
    a pass over colour c: §4.15), 0 where no tap is live."""
    v = np.ascontiguousarray(v, dtype=F)
    H, W = v.shape
    filt = live(g, v) if c is None else live(g, c, v)
    gs = np.zeros((H, W), dtype=F)
    vs = np.zeros((H, W), dtype=F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            PQ = _shift(H, W, dy, dx)
            if PQ is None:
                continue
            P, Q = PQ
            valid = filt[P] & filt[Q]
            k = GAUSS3[dy + 1][dx + 1]
            gs[P] = np.where(valid, gs[P] + k, gs[P])
            with np.errstate(all="ignore"):
                vs[P] = np.where(valid, vs[P] + k * v[Q], vs[P])
    with np.errstate(all="ignore"):
        return np.where(gs > 0, vs / gs, F(0)).astype(F)


def guided_pass(c, v, g, i, sp):
    """Pass i (step 2^i) over colour c [H, W, 3] and variance v [H, W]; returns (c', v')."""
    c = np.ascontiguousarray(c, dtype=F)
    v = np.ascontiguousarray(v, dtype=F)
    H, W = v.shape
    step = 1 << i
    pos, nrm, filt = g["position"], g["normal"], live(g, c, v)
    sl = F(sp["sigma_luminance"])
    use_l = not np.isinf(sl)
    sw = np.zeros((H, W), dtype=F)
    acc = np.zeros((H, W, 3), dtype=F)
    sv = np.zeros((H, W), dtype=F)
    with np.errstate(all="ignore"):
        if use_l:
            den = F(sl * sl) * prefilter(v, g, c) + F(sp["epsilon"])
            lc = lum(c)
            assert den.dtype == F and lc.dtype == F
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                PQ = _shift(H, W, dy * step, dx * step)
                if PQ is None:
                    continue
                P, Q = PQ
                valid = filt[P] & filt[Q]
                wn, wz = _geometry_weight(nrm, pos, P, Q, sp["normal_power_log2"], F(sp["sigma_plane"]))
                h = F(KERNEL[dy + 2] * KERNEL[dx + 2])
                w = (h * wn) * wz
                if use_l:
                    dl = lc[P] - lc[Q]
                    w = w * (F(1) / (F(1) + (dl * dl) / den[P]))
                assert w.dtype == F
                sw[P] = np.where(valid, sw[P] + w, sw[P])
                acc[P] = np.where(valid[..., None], acc[P] + w[..., None] * c[Q], acc[P])
                sv[P] = np.where(valid, sv[P] + (w * w) * v[Q], sv[P])
        # a texel that is not live, or whose weights sum to nothing (a zero normal), passes its
        # colour through with variance 0; so does the variance where sw^2 underflows
        ok = filt & (sw > 0)
        sw2 = sw * sw
        co = np.where(ok[..., None], acc / sw[..., None], c)
        vo = np.where(ok & (sw2 > 0), sv / sw2, F(0))
    return np.ascontiguousarray(co, dtype=F), np.ascontiguousarray(vo, dtype=F)


def filter_frame(c, m, length, g, sp):
    """B and C: (colour, variance after the last pass, colour after pass 0, variance of B)."""
    v0 = variance(m, length, g, sp)
    v, first = v0, None
    for i in range(int(sp["iterations"])):
        c, v = guided_pass(c, v, g, i, sp)
        if i == 0:
            first = c
    return c, v, first, v0


# ------------------------------------------------------------------------ the stateful chain
class Chain:
    """The state rvcp_render_svgf keeps: colour, moments, length, G-buffer and the previous view
    (None: the camera bytes of the next frame equal the previous one's)."""

    def __init__(self, tp, sp, feedback=False):
        self.tp, self.sp, self.feedback = tp, sp, feedback
        self.hist = None

    def reset(self):
        self.hist = None

    def frame(self, c, g, view):
        """One frame; `view`: the previous frame's camera, or None when it did not move.
        Returns (displayed colour, its variance, history length)."""
        if self.hist is None:
            a, n, m = accumulate(c, g, None, None, None, None, None, self.tp, self.sp)
        else:
            pc, pg, pl, pm = self.hist
            a, n, m = accumulate(c, g, pc, pg, pl, pm, view, self.tp, self.sp)
        out, var, first, _ = filter_frame(a, m, n, g, self.sp)
        self.hist = (first if self.feedback else a, g, n, m)
        return out, var, n


def synthetic_moments(c_prev, seed):
    """Random history moments in the range of the history colours' luminance: m1 near l(c), m2 >=
    m1^2 on most pixels and below it on some (the clamp), exact zeros included."""
    rng = np.random.default_rng(seed)
    l1 = lum(np.ascontiguousarray(c_prev, dtype=F))
    m1 = (l1 * rng.uniform(0.5, 1.5, l1.shape).astype(F)).astype(F)
    m2 = (m1 * m1 * rng.uniform(0.9, 3.0, l1.shape).astype(F)).astype(F)
    zero = rng.random(l1.shape) < 0.1
    m1[zero], m2[zero] = 0, 0
    return np.ascontiguousarray(np.stack([m1, m2], axis=-1), dtype=F)


# The quality gate: static camera, Cornell box 64^2, SPP = 4, 8 frames (time
# seeds 5.0 ... 12.0), the defaults without feedback: RATIO_MEASURED = rmse(SVGF output of frame
# 8) / rmse(first raw frame) against the oracle at SPP = 2048 over the filterable pixels.  The
# gate is that value plus a quarter of the distance to 1 (denoise_ref.QUALITY_GATE's rule).
RATIO_MEASURED = 0.172      # rmse 0.1374 -> 0.0237 (temporal only 0.0583, + a-trous defaults 0.0319)
QUALITY_GATE = RATIO_MEASURED + (1.0 - RATIO_MEASURED) / 4.0
QUALITY_SEEDS = T.QUALITY_SEEDS
