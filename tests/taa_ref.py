"""taa_ref -- numpy float32 restatement of the temporal anti-aliasing resolve behind
rvcp_taa_resolve_async, a float64 restatement of the jitter (rvcp_taa_jitter,
rvcp_taa_jitter_push), a generator of synthetic frame pairs and the flat shading of the
anti-aliasing gates (TEST INFRASTRUCTURE ONLY: never imported by the package).

It shares no code with csrc/rvcp_taa.hip, only the contract: float32 throughout, every operation
rounded once, in the order DESIGN.md §4.13 writes them, the taps visited in the order (x0, y0),
(x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), and a rejected tap adds nothing.  numpy evaluates
each array operation in float32 with one rounding and never fuses, so the kernel's output is
reproduced bit for bit, thresholds and floor included.
"""
from __future__ import annotations

import numpy as np

import temporal_ref as T
from denoise_ref import GBUFFER_DTYPE, MISS

F = np.float32
PARAMS_DTYPE = np.dtype([("alpha_min", "<f4"), ("max_history", "<u4"), ("clamp", "<u4"),
                         ("_pad", "<u4")])
JITTER_PERIOD = 16


def params(alpha_min=0.1, max_history=32, clamp=1):
    p = np.zeros((), dtype=PARAMS_DTYPE)
    p["alpha_min"], p["max_history"], p["clamp"] = alpha_min, max_history, clamp
    return p


# ------------------------------------------------------------------------ the jitter (float64)
def halton(i: int, b: int) -> float:
    f, r = 1.0, 0.0
    while i > 0:
        f /= b
        r += f * (i % b)
        i //= b
    return r


def jitter(frame_index: int):
    """(jx, jy) of frame `frame_index` in float64: Halton(2, 3), centred, period 16."""
    i = frame_index % JITTER_PERIOD + 1
    return halton(i, 2) - 0.5, halton(i, 3) - 0.5


def jitter_forward_f64(push, H, j):
    """The forward of `push`'s camera rotated by the jitter j = (jx, jy) pixels, float64."""
    cam = np.asarray(push["camera"]).reshape(())
    f = cam["forward"].astype(np.float64)[:3]
    _, k, r, d, _ = T.view_f64(cam["position"], cam["forward"], cam["up"], cam["vertical_fov"], H)
    fl = np.linalg.norm(f)
    n = f / fl + r * (float(j[0]) / k) + d * (float(j[1]) / k)
    return n / np.linalg.norm(n) * fl


# ------------------------------------------------------------------------ the step
def sat(c):
    """gamma_u8's own clamp: c > 0 ? (c < 1 ? c : 1) : 0 (a NaN gives 0)."""
    c = np.asarray(c, dtype=F)
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, np.where(c < 1, c, F(1)), F(0)).astype(F)


def _dot3v(a, v):
    """(a0 v0 + a1 v1) + a2 v2 of an array of vectors with one vector, float32."""
    v = np.asarray(v, dtype=F)
    return (a[..., 0] * v[0] + a[..., 1] * v[1]) + a[..., 2] * v[2]


def _project(view, pos, W, H):
    """§4.10's e, z, a, b, fx, fy of positions pos under `view`, without the range test."""
    e = pos - view["position"].astype(F)
    z = _dot3v(e, view["forward"])
    a = _dot3v(e, view["right"])
    b = _dot3v(e, view["down"])
    k = F(view["k"])
    fx = ((a / z) * k + F(0.5) * F(W)) - F(0.5)
    fy = ((b / z) * k + F(0.5) * F(H)) - F(0.5)
    return fx, fy, z


def history_coords(g, cur_view, prev_view):
    """Where the history of every pixel lies in the previous frame: (fx, fy, ok) float32 /
    bool [H, W]; ok is false where a projection has z <= 0 or is NaN."""
    H, W = g.shape
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(F), ys.astype(F)
    V, P = cur_view, prev_view
    with np.errstate(all="ignore"):
        # hit pixels: the difference of the two projections of the primary hit
        ux, uy, uz = _project(V, g["position"], W, H)
        vx, vy, vz = _project(P, g["position"], W, H)
        hx, hy, hok = xf + (vx - ux), yf + (vy - uy), (uz > 0) & (vz > 0)
        # miss pixels: the pixel's direction through V, projected by P
        vf = V["forward"].astype(F)
        ff = (vf[0] * vf[0] + vf[1] * vf[1]) + vf[2] * vf[2]
        fwd = vf / ff
        k = F(V["k"])
        sx = ((xf + F(0.5)) - F(0.5) * F(W)) / k
        sy = ((yf + F(0.5)) - F(0.5) * F(H)) / k
        r, dn = V["right"].astype(F), V["down"].astype(F)
        d = np.stack([(fwd[i] + sx * r[i]) + sy * dn[i] for i in range(3)], axis=-1)
        assert d.dtype == F
        z = _dot3v(d, P["forward"])
        a = _dot3v(d, P["right"])
        b = _dot3v(d, P["down"])
        pk = F(P["k"])
        mx = ((a / z) * pk + F(0.5) * F(W)) - F(0.5)
        my = ((b / z) * pk + F(0.5) * F(H)) - F(0.5)
        mok = z > 0
    miss = g["face"] == MISS
    fx, fy = np.where(miss, mx, hx), np.where(miss, my, hy)
    assert fx.dtype == F and fy.dtype == F
    return fx, fy, np.where(miss, mok, hok)


def box3(s):
    """Per channel min and max of s over the 3 x 3 pixels around every interior pixel; (lo, hi,
    interior) -- lo and hi are s itself elsewhere."""
    H, W = s.shape[:2]
    lo, hi = s.copy(), s.copy()
    interior = np.zeros((H, W), dtype=bool)
    if H >= 3 and W >= 3:
        interior[1:-1, 1:-1] = True
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                q = s[dy:H - 2 + dy, dx:W - 2 + dx]
                lo[1:-1, 1:-1] = np.minimum(lo[1:-1, 1:-1], q)
                hi[1:-1, 1:-1] = np.maximum(hi[1:-1, 1:-1], q)
    return lo, hi, interior


def resolve(c, g, prev_res, prev_len, cur_view, prev_view, p, want_info=False):
    """One resolve: current linear colour c [H, W, 3] float32 and texels g [H, W]; history
    prev_res [H, W, 3], prev_len [H, W] uint32 (both None: no history); cur_view / prev_view:
    VIEW_DTYPE records of the two unjittered cameras, both None (or byte-equal) for the identity
    mapping; p: a PARAMS_DTYPE record.  Returns (out, len) [, a dict: accepted taps per pixel,
    `has`, `interior`, and `changed` where the clamp changed h]."""
    c = np.ascontiguousarray(c, dtype=F)
    H, W = c.shape[:2]
    cur = sat(c)
    wsum = np.zeros((H, W), dtype=F)
    acc = np.zeros((H, W, 3), dtype=F)
    nmin = np.full((H, W), 1 << 40, dtype=np.int64)
    ntaps = np.zeros((H, W), dtype=np.int64)
    taps = []
    if prev_res is not None:
        prev_res = np.ascontiguousarray(prev_res, dtype=F)
        ys, xs = np.mgrid[0:H, 0:W]
        identity = cur_view is None or \
            np.asarray(cur_view).tobytes() == np.asarray(prev_view).tobytes()
        if identity:
            taps = [(xs, ys, np.ones((H, W), dtype=F), np.ones((H, W), dtype=bool))]
        else:
            fx, fy, ok = history_coords(g, cur_view, prev_view)
            with np.errstate(all="ignore"):
                ok = ok & (fx >= F(-1)) & (fx < F(W)) & (fy >= F(-1)) & (fy < F(H))
                x0f, y0f = np.floor(fx), np.floor(fy)
                tx, ty = fx - x0f, fy - y0f
                ux, uy = F(1) - tx, F(1) - ty
                # float -> int only inside the range
                x0 = np.where(ok, x0f, F(0)).astype(np.int64)
                y0 = np.where(ok, y0f, F(0)).astype(np.int64)
                taps = [(x0, y0, ux * uy, ok), (x0 + 1, y0, tx * uy, ok),
                        (x0, y0 + 1, ux * ty, ok), (x0 + 1, y0 + 1, tx * ty, ok)]
    with np.errstate(all="ignore"):
        for qx, qy, w, ok in taps:
            assert w.dtype == F
            inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            Q = (np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1))
            lq = prev_len[Q].astype(np.int64)
            a = inside & (lq >= 1)
            wsum = np.where(a, wsum + w, wsum)
            acc = np.where(a[..., None], acc + w[..., None] * prev_res[Q], acc)
            nmin = np.where(a, np.minimum(nmin, lq), nmin)
            ntaps += a
        has = wsum > 0
        h = acc / wsum[..., None]
        n = np.minimum(nmin + 1, int(p["max_history"]))
        lo, hi, interior = box3(cur)
        clamped = interior & (int(p["clamp"]) == 1)
        # min(max(h, lo), hi) as selections: a NaN history takes lo
        m = np.where(h >= lo, h, lo)
        hc = np.where(m <= hi, m, hi)
        h2 = np.where(clamped[..., None], hc, h).astype(F)
        alpha = F(1) / n.astype(F)
        alpha = np.where(alpha < F(p["alpha_min"]), F(p["alpha_min"]), alpha).astype(F)
        blend = h2 + alpha[..., None] * (cur - h2)
        assert blend.dtype == F
    out = np.ascontiguousarray(np.where(has[..., None], blend, cur), dtype=F)
    length = np.where(has, n, 1).astype(np.uint32)
    if not want_info:
        return out, length
    changed = has & clamped & np.any(h2.view(np.uint32) != h.astype(F).view(np.uint32), axis=-1)
    return out, length, dict(ntaps=ntaps, has=has, interior=interior, changed=changed, lo=lo, hi=hi,
                             h=h2, alpha=alpha)


class Chain:
    """The TAA state of one stateful chain (rvcp_render_temporal / rvcp_render_svgf with the
    switch on), restated: feed it every frame's final linear colour and G-buffer (both rendered
    through jitter_push of the frame counter) and the caller's unjittered push."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.res = self.len = self.push = self.view = None
        self.counter = 0

    def step(self, c, g, push, p=None):
        H = c.shape[0]
        view = T.view_of_push(np.asarray(push).reshape(()), H)
        at_rest = self.res is not None and \
            np.asarray(push)["camera"].tobytes() == np.asarray(self.push)["camera"].tobytes()
        out, ln = resolve(c, g, self.res, self.len, None if at_rest else view,
                          None if at_rest else self.view, params() if p is None else p)
        self.res, self.len, self.push, self.view = out, ln, np.array(push), view
        self.counter += 1
        return out, ln


# ------------------------------------------------------------------------ synthetic inputs
MIX_MIN_PIXELS = T.MIX_MIN_PIXELS


def synthetic_case(W, H, seed, p=None):
    """A pair of frames for one resolve: (c, g, prev_res, prev_len, cur_view, prev_view), on
    temporal_ref.synthetic_case's geometry: the previous camera is that generator's, the current
    one has moved (sideways, up and forward) and turned a little, and the frame is cut into blocks
    of b x b pixels (b = 4, or 2 on frames below 256 pixels), each seen at a depth of its own
    along the current camera's rays through slightly off-centre points of its pixels.  By its
    number (block index + seed) mod 10 a block is: 0 miss pixels whose history is wiped (the
    history length of every texel their four taps touch is set to 0), 1-2 miss pixels, 3 hit
    pixels whose history is wiped, 4 hit pixels behind the previous camera (even columns,
    mirrored through it) or behind the current one (odd columns), 5-9 ordinary hit pixels;
    towards the frame's edges the motion carries some histories off the frame.  Wiped
    footprints, and the 4 % of single texels of length 0, leave their neighbours one to three
    taps.  Current colours: half of the blocks flat (one
    colour plus a little noise, a narrow 3 x 3 box), half noisy over [-0.5, 1.6], about 1 % NaN;
    the history is the displayed current colour plus noise of deviation 0.1, clipped to [0, 1];
    history lengths run from 1 to beyond max_history and beyond
    65535.

    On frames of at least MIX_MIN_PIXELS pixels and two rows and columns the generator asserts
    its own mix with `p` (default: the library's defaults): of all pixels >= 20 % with four
    accepted taps, >= 10 % with one to three, >= 10 % with none, >= 5 % miss pixels with a
    history and >= 2 % miss pixels without; and on frames with at least MIX_MIN_PIXELS interior
    pixels, of the interior pixels with a history the clamp changes h on >= 20 % and leaves it on
    >= 20 %."""
    rng = np.random.default_rng(seed)
    p = params() if p is None else p
    cam_pos = np.array([3.0, -2.0, 1.5])
    fwd = np.array([0.3, -0.2, 1.1])                  # deliberately not unit length
    up = np.array([0.1, 1.0, 0.05])
    prev_view = T.make_view(cam_pos, fwd, up, 47.0, H)
    _, k, right, down, _ = T.view_f64(cam_pos, fwd, up, 47.0, H)
    fhat = fwd / np.linalg.norm(fwd)
    cpos = cam_pos + 1.5 * right - 1.0 * down + 3.0 * fhat
    cfwd = fwd + np.linalg.norm(fwd) * (0.04 * right - 0.03 * down)
    cur_view = T.make_view(cpos, cfwd, up, 47.0, H)
    _, ck, cright, cdown, _ = T.view_f64(cpos, cfwd, up, 47.0, H)
    chat = cfwd / np.linalg.norm(cfwd)

    b = 4 if W * H >= 256 else 2
    ys, xs = np.mgrid[0:H, 0:W]
    nbx = (W + b - 1) // b
    kind = ((ys // b) * nbx + xs // b + seed) % 10
    depth = rng.uniform(10.0, 60.0, ((H + b - 1) // b, nbx))[ys // b, xs // b]
    depth = depth + rng.uniform(-0.5, 0.5, (H, W))
    sx, sy = (xs + 0.8 - 0.5 * W) / ck, (ys + 0.3 - 0.5 * H) / ck      # (0.3, -0.2) off-centre
    x = cpos + depth[..., None] * (chat + sx[..., None] * cright + sy[..., None] * cdown)
    x = np.where(((kind == 4) & (xs % 2 == 0))[..., None], 2.0 * cam_pos - x, x)
    x = np.where(((kind == 4) & (xs % 2 == 1))[..., None], 2.0 * cpos - x, x)
    g = np.zeros((H, W), dtype=GBUFFER_DTYPE)
    g["position"] = x
    g["normal"] = -chat
    g["face"] = rng.integers(0, 1000, (H, W))
    g["material"] = rng.integers(0, 4, (H, W))
    g["face"][kind <= 2] = MISS
    # ---- colours
    flat = ((ys // b + xs // b) % 2 == 0)[..., None]
    base = rng.uniform(-0.3, 1.5, ((H + b - 1) // b, nbx, 3))[ys // b, xs // b]
    c = np.where(flat, base + rng.uniform(-0.05, 0.05, (H, W, 3)), rng.uniform(-0.5, 1.6, (H, W, 3)))
    c = np.where(rng.random((H, W, 3)) < 0.01, np.nan, c).astype(F)
    prev_res = np.clip(sat(c) + rng.normal(0.0, 0.1, (H, W, 3)), 0.0, 1.0).astype(F)
    # ---- history lengths
    prev_len = rng.integers(1, 6, (H, W)).astype(np.uint32)
    r = rng.random((H, W))
    mh = int(p["max_history"])
    prev_len = np.where(r < 0.3, rng.integers(max(1, mh - 3), mh + 4, (H, W)), prev_len)
    prev_len = np.where(r < 0.1, rng.integers(65000, 70000, (H, W)), prev_len).astype(np.uint32)
    prev_len[rng.random((H, W)) < 0.04] = 0
    fx, fy, ok = history_coords(g, cur_view, prev_view)
    with np.errstate(all="ignore"):
        ok = ok & (fx >= F(-1)) & (fx < F(W)) & (fy >= F(-1)) & (fy < F(H))
        x0 = np.where(ok, np.floor(fx), 0).astype(np.int64)
        y0 = np.where(ok, np.floor(fy), 0).astype(np.int64)
    wipe = ok & ((kind == 0) | (kind == 3))
    for dy in (0, 1):
        for dx in (0, 1):
            qy, qx = y0[wipe] + dy, x0[wipe] + dx
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            prev_len[qy[inside], qx[inside]] = 0
    # ---- the mix
    if W * H >= MIX_MIN_PIXELS and min(W, H) >= 2:
        _, _, info = resolve(c, g, prev_res, prev_len, cur_view, prev_view, p, True)
        nt, has, miss = info["ntaps"], info["has"], g["face"] == MISS
        share = np.bincount(nt.ravel(), minlength=5) / nt.size
        assert share[4] >= 0.2 and share[1:4].sum() >= 0.1 and share[0] >= 0.1, share
        assert np.mean(miss & has) >= 0.05 and np.mean(miss & ~has) >= 0.02, \
            (np.mean(miss & has), np.mean(miss & ~has))
        if (W - 2) * (H - 2) >= MIX_MIN_PIXELS and int(p["clamp"]) == 1:
            ih = info["interior"] & has
            ch = np.count_nonzero(info["changed"]) / max(1, np.count_nonzero(ih))
            assert 0.2 <= ch <= 0.8, ch
        with np.errstate(invalid="ignore"):
            assert (c < 0).any() and ((c >= 0) & (c <= 1)).any() and (c > 1).any()
        assert np.isnan(c).any() and 0 < np.isnan(c).mean() < 0.05
        assert (prev_len == 0).any() and (prev_len > mh).any() and (prev_len > 65535).any()
        assert (_project(prev_view, g["position"], W, H)[2] < 0).any()
    return c, g, prev_res, prev_len, cur_view, prev_view


# ------------------------------------------------------------------------ the anti-aliasing gates
LIGHT = np.array([0.3, 0.8, -0.5]) / np.linalg.norm([0.3, 0.8, -0.5])


def flat_shade(g, materials):
    """A deterministic shade of a G-buffer: albedo[m] (0.25 + 0.75 |n . L|), emissive -> 1,
    miss -> 0; float32 [H, W, 3]."""
    from denoise_ref import EMISSIVE
    alb = np.asarray(materials["albedo"], dtype=np.float64)[:, :3]
    m = (g["material"] & ~np.uint32(EMISSIVE)).astype(np.int64)
    ndl = np.abs(g["normal"].astype(np.float64) @ LIGHT)
    c = alb[np.clip(m, 0, len(alb) - 1)] * (0.25 + 0.75 * ndl)[..., None]
    c = np.where(((g["material"] & np.uint32(EMISSIVE)) != 0)[..., None], 1.0, c)
    c = np.where((g["face"] == MISS)[..., None], 0.0, c)
    return c.astype(F)


def box4(c):
    """The 4 x 4 box average of a [4H, 4W, ...] array, float64."""
    c = np.asarray(c, dtype=np.float64)
    H, W = c.shape[0] // 4, c.shape[1] // 4
    return c.reshape(H, 4, W, 4, *c.shape[2:]).mean(axis=(1, 3))


def edge_pixels(face_hi):
    """Pixels whose 16 sub-sample face ids [4H, 4W] differ."""
    H, W = face_hi.shape[0] // 4, face_hi.shape[1] // 4
    f = face_hi.reshape(H, 4, W, 4).transpose(0, 2, 1, 3).reshape(H, W, 16)
    return np.any(f != f[..., :1], axis=-1)


def gate(ratio_measured):
    """The project's rule: the measured ratio plus a quarter of the distance to 1."""
    return ratio_measured + (1.0 - ratio_measured) / 4.0


GATE_FRAMES = 16


def jittered_push(base, H, frame_index):
    """`base` (a PUSH_DTYPE record) with its forward rotated by jitter(frame_index): the float64
    restatement rounded once; a zero jitter returns a plain copy."""
    jp = np.array(base).reshape(())
    j = tuple(float(F(v)) for v in jitter(frame_index))
    if j != (0.0, 0.0):
        jp["camera"]["forward"][...] = jitter_forward_f64(jp, H, j).astype(F)
    return jp


def aa_gate(W, H, base, materials, gbuffer_of):
    """The anti-aliasing gate's measurement: gbuffer_of(push, w, h) is the G-buffer of the scene
    through `push` at w x h.  GATE_FRAMES jittered frames of flat_shade, resolved at the defaults
    with the camera at rest, against box4 of the clamped shade at 4 W x 4 H.  Returns the RMSEs
    of one centred frame and of the resolved one over the edge and the other pixels, and
    ratio = edge_resolved / edge_single."""
    hi = gbuffer_of(base, 4 * W, 4 * H)
    truth = box4(sat(flat_shade(hi, materials)))
    edge = edge_pixels(hi["face"])
    single = sat(flat_shade(gbuffer_of(base, W, H), materials))
    chain = Chain()
    for i in range(GATE_FRAMES):
        g = gbuffer_of(jittered_push(base, H, i), W, H)
        out, _ = chain.step(flat_shade(g, materials), g, base)

    def rm(a, m):
        d = a[m].astype(np.float64) - truth[m]
        return float(np.sqrt(np.mean(d * d)))

    r = dict(n_edge=int(edge.sum()), n=int(edge.size), edge_single=rm(single, edge),
             edge_resolved=rm(out, edge), nonedge_single=rm(single, ~edge),
             nonedge_resolved=rm(out, ~edge))
    r["ratio"] = r["edge_resolved"] / r["edge_single"]
    return r


def cpu_gbuffer_of(push, w, h):
    """gbuffer_of for aa_gate: denoise_ref.cpu_gbuffer of the default Cornell box through the
    forward of `push`."""
    import denoise_ref as D
    import rvcp_amd
    sc = rvcp_amd.Scene.default()
    sc.camera.forward = np.asarray(push["camera"]["forward"], dtype=F).reshape(-1)[:3].copy()
    return D.cpu_gbuffer(sc, w, h)
# The anti-aliasing gate: the Cornell box from the default camera, flat_shade of
# the G-buffer through rvcp_taa_jitter_push of frames 0..15, resolved at the defaults, against
# box4 of the clamped shade at 4 W x 4 H from the unjittered camera.  RATIO_MEASURED[(W, H)] =
# rmse(resolved) / rmse(one centred frame) over edge_pixels, measured with this restatement
# (37 x 23 on cpu_gbuffer, 64 x 64 on the library's G-buffers).
RATIO_MEASURED = {(37, 23): 0.338,      # edge rmse 0.1018 -> 0.0344 (227 of 851 pixels)
                  (64, 64): 0.326}     # edge rmse 0.0789 -> 0.0257 (785 of 4096 pixels)
# The path-traced gate: rvcp_render_svgf at 64 x 64, SPP 4, 16 frames (time seeds
# temporal_ref.QUALITY_SEEDS's rule, 5.0 + i), against box4 of the clamped plain render at
# 256 x 256, SPP 128 -- (edge rmse off, edge rmse on, all-pixel rmse off, all-pixel rmse on) as
# measured on the MI355X.
PATH_MEASURED = (0.0699, 0.0353, 0.0357, 0.0270)    # 785 edge pixels: ratio 0.505
