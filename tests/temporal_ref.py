"""temporal_ref -- numpy float32 restatement of the temporal reprojection and accumulation step
behind rvcp_temporal_accumulate_async, an independent float64 camera
projection, and a generator of synthetic frame pairs (TEST INFRASTRUCTURE ONLY: never imported
by the package).

It shares no code with csrc/rvcp_temporal.hip, only the contract: float32 throughout, every
operation rounded once, in the order DESIGN.md §4.10 writes them, the taps visited in the order
(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), a rejected tap adds nothing, and a texel
that is not live (§4.15: not filterable, or a non-finite position, normal or colour) is a MISS
texel, as the current pixel and as a history tap.  numpy
evaluates each array operation in float32 with one rounding and never fuses, so the kernel's
output is reproduced bit for bit, thresholds and floor included.
"""
from __future__ import annotations

import numpy as np

from denoise_ref import EMISSIVE, GBUFFER_DTYPE, MISS, filterable, live

F = np.float32
PARAMS_DTYPE = np.dtype([("alpha_min", "<f4"), ("max_history", "<u4"),
                         ("sigma_plane", "<f4"), ("normal_min", "<f4")])
VIEW_DTYPE = np.dtype([("position", "<f4", (3,)), ("k", "<f4"), ("right", "<f4", (3,)),
                       ("_pad0", "<f4"), ("down", "<f4", (3,)), ("_pad1", "<f4"),
                       ("forward", "<f4", (3,)), ("_pad2", "<f4")])
PI = 3.1415926              # the shader's constant


def params(alpha_min=0.05, max_history=32, sigma_plane=0.1, normal_min=0.9):
    p = np.zeros((), dtype=PARAMS_DTYPE)
    p["alpha_min"], p["max_history"] = alpha_min, max_history
    p["sigma_plane"], p["normal_min"] = sigma_plane, normal_min
    return p


def _dot3(a, b):
    """(a0 b0 + a1 b1) + a2 b2, every operation rounded to float32."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ------------------------------------------------------------------------ the camera
def view_f64(position, forward, up, vfov_deg, H):
    """The projection of a camera in float64: (position, k, right, down, forward / |forward|^2),
    the inverse of the shader's sample_ray (its u along forward x up, its v along forward x u,
    the image plane H pixels high at slope 2 tan(vfov / 2))."""
    pos, f, u = (np.asarray(v, dtype=np.float64)[:3] for v in (position, forward, up))
    r = np.cross(f, u)
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    d = d / np.linalg.norm(d)
    k = H / (2.0 * np.tan(float(vfov_deg) / 2.0 * PI / 180.0))
    return pos, k, r, d, f / np.dot(f, f)


def make_view(position, forward, up, vfov_deg, H):
    """view_f64 rounded once to a VIEW_DTYPE record."""
    pos, k, r, d, f = view_f64(position, forward, up, vfov_deg, H)
    v = np.zeros((), dtype=VIEW_DTYPE)
    v["position"], v["k"], v["right"], v["down"], v["forward"] = pos, k, r, d, f
    return v


def view_of_push(push, H):
    cam = push["camera"]
    return make_view(cam["position"], cam["forward"], cam["up"], cam["vertical_fov"], H)


def project(view, pos, W, H):
    """Float32 pixel coordinates (fx, fy), the depth z and the range test of positions pos
    [..., 3] under `view`, in the kernel's operation order."""
    e = pos - view["position"].astype(F)
    with np.errstate(all="ignore"):
        z = _dot3(e, view["forward"].astype(F))
        a = _dot3(e, view["right"].astype(F))
        b = _dot3(e, view["down"].astype(F))
        k = F(view["k"])
        fx = ((a / z) * k + F(0.5) * F(W)) - F(0.5)
        fy = ((b / z) * k + F(0.5) * F(H)) - F(0.5)
        ok = (z > 0) & (fx >= F(-1)) & (fx < F(W)) & (fy >= F(-1)) & (fy < F(H))
    assert fx.dtype == F and fy.dtype == F
    return fx, fy, z, ok


# ------------------------------------------------------------------------ the step
def accumulate(c, g, prev_c, prev_g, prev_len, view, p, want_taps=False):
    """One step: current colour c [H, W, 3] float32 and texels g [H, W]; history prev_c, prev_g,
    prev_len [H, W] uint32 (all None: no history); view: a VIEW_DTYPE record of the previous
    camera, or None for the identity mapping; p: a PARAMS_DTYPE record.  Returns (out, len)
    [, the number of accepted taps per pixel]."""
    c = np.ascontiguousarray(c, dtype=F)
    H, W = c.shape[:2]
    filt = live(g, c)                  # §4.15: any other texel is a MISS texel, here and below
    pos, nrm, mat = g["position"], g["normal"], g["material"]
    wsum = np.zeros((H, W), dtype=F)
    acc = np.zeros((H, W, 3), dtype=F)
    nmin = np.full((H, W), 1 << 40, dtype=np.int64)
    ntaps = np.zeros((H, W), dtype=np.int64)
    taps = []
    if prev_c is not None:
        prev_c = np.ascontiguousarray(prev_c, dtype=F)
        ys, xs = np.mgrid[0:H, 0:W]
        if view is None:
            taps = [(xs, ys, np.ones((H, W), dtype=F), np.ones((H, W), dtype=bool))]
        else:
            fx, fy, _, ok = project(view, pos, W, H)
            with np.errstate(all="ignore"):
                x0f, y0f = np.floor(fx), np.floor(fy)
                tx, ty = fx - x0f, fy - y0f
                ux, uy = F(1) - tx, F(1) - ty
                # float -> int only inside the range
                x0 = np.where(ok, x0f, F(0)).astype(np.int64)
                y0 = np.where(ok, y0f, F(0)).astype(np.int64)
                taps = [(x0, y0, ux * uy, ok), (x0 + 1, y0, tx * uy, ok),
                        (x0, y0 + 1, ux * ty, ok), (x0 + 1, y0 + 1, tx * ty, ok)]
    sp, nm = F(p["sigma_plane"]), F(p["normal_min"])
    with np.errstate(all="ignore"):
        for qx, qy, w, ok in taps:
            assert w.dtype == F
            inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            Q = (np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1))
            gq = prev_g[Q]
            a = inside & filt & live(gq, prev_c[Q]) & (gq["material"] == mat)
            a &= _dot3(nrm, gq["normal"]) >= nm
            a &= np.abs(_dot3(nrm, gq["position"] - pos)) <= sp
            lq = prev_len[Q].astype(np.int64)
            a &= lq >= 1
            wsum = np.where(a, wsum + w, wsum)
            acc = np.where(a[..., None], acc + w[..., None] * prev_c[Q], acc)
            nmin = np.where(a, np.minimum(nmin, lq), nmin)
            ntaps += a
        has = filt & (wsum > 0)
        h = acc / wsum[..., None]
        n = np.minimum(nmin + 1, int(p["max_history"]))
        alpha = F(1) / n.astype(F)
        alpha = np.where(alpha < F(p["alpha_min"]), F(p["alpha_min"]), alpha).astype(F)
        blend = h + alpha[..., None] * (c - h)
        assert blend.dtype == F
    out = np.ascontiguousarray(np.where(has[..., None], blend, c), dtype=F)
    length = np.where(filt, np.where(has, n, 1), 0).astype(np.uint32)
    return (out, length, ntaps) if want_taps else (out, length)


# ------------------------------------------------------------------------ synthetic inputs
BLOCK = 8                   # the previous frame's surface is one plane per BLOCK x BLOCK pixels
MIX_MIN_PIXELS = 64         # frames below this (or one pixel thin) cannot hold the mix asserted


def synthetic_case(W, H, seed, identity=False, p=None):
    """A pair of frames for one step: (c, g, prev_c, prev_g, prev_len, view).

    The previous frame sees one plane per BLOCK x BLOCK pixels (its own normal, depth and
    material), each texel the float64 intersection of its pixel's ray with its block's plane.
    Some texels are then spoilt, one rule each: MISS, EMISSIVE, another material, a normal
    below normal_min, a position off the plane, prev_len == 0.  Every current pixel chooses a
    continuous target in the previous frame, from -2 to W + 1 and H + 1 (so some land
    off-frame; most are drawn inside it, or a frame a few pixels high would have next to no
    pixel with its four taps inside), and lies where the target's ray meets the plane of the
    block the target falls in: the projection inverted in float64.  Some pixels sit behind the
    previous camera or exactly at it (z <= 0), some carry a material no history texel has, about
    10 % are not filterable; history lengths run from 1 to beyond max_history and beyond 65535.
    identity = True: every target is the pixel's own centre, for the identity mapping.

    The generator asserts its own mix over the filterable pixels, with `p` (default: the
    library's defaults): >= 20 % with four accepted taps, >= 10 % with one to three, >= 10 %
    with none (identity: >= 50 % accepted, >= 10 % rejected), on frames of at least
    MIX_MIN_PIXELS pixels and two rows and columns."""
    rng = np.random.default_rng(seed)
    p = params() if p is None else p
    cam_pos = np.array([3.0, -2.0, 1.5])
    fwd = np.array([0.3, -0.2, 1.1])                  # deliberately not unit length
    up = np.array([0.1, 1.0, 0.05])
    view = make_view(cam_pos, fwd, up, 47.0, H)
    _, k, right, down, _ = view_f64(cam_pos, fwd, up, 47.0, H)
    fhat = fwd / np.linalg.norm(fwd)

    def ray(u, v):                                    # through continuous pixel (u, v); z = 1
        sx, sy = (u + 0.5 - 0.5 * W) / k, (v + 0.5 - 0.5 * H) / k
        return fwd + sx[..., None] * right + sy[..., None] * down

    # the planes, one per block
    bw, bh = (W + BLOCK - 1) // BLOCK + 1, (H + BLOCK - 1) // BLOCK + 1
    tilt = rng.uniform(-0.3, 0.3, (bh, bw, 2))
    pn = -fhat + tilt[..., :1] * right + tilt[..., 1:] * down
    pn /= np.linalg.norm(pn, axis=-1, keepdims=True)
    p0 = cam_pos + rng.uniform(10.0, 60.0, (bh, bw, 1)) * fwd
    pmat = rng.integers(0, 4, (bh, bw)).astype(np.uint32)

    def hit(u, v, by, bx):
        d = ray(u, v)
        n, o = pn[by, bx], p0[by, bx]
        z = np.sum(n * (o - cam_pos), axis=-1) / np.sum(n * d, axis=-1)
        return cam_pos + z[..., None] * d

    ys, xs = np.mgrid[0:H, 0:W]
    # ---- previous frame
    prev_g = np.zeros((H, W), dtype=GBUFFER_DTYPE)
    by, bx = ys // BLOCK, xs // BLOCK
    prev_g["position"] = hit(xs.astype(np.float64), ys.astype(np.float64), by, bx)
    prev_g["normal"] = pn[by, bx]
    prev_g["material"] = pmat[by, bx]
    prev_g["face"] = rng.integers(0, 1000, (H, W))
    prev_len = rng.integers(1, 6, (H, W)).astype(np.uint32)
    r = rng.random((H, W))
    mh = int(p["max_history"])
    prev_len = np.where(r < 0.3, rng.integers(max(1, mh - 3), mh + 4, (H, W)), prev_len)
    prev_len = np.where(r < 0.1, rng.integers(65000, 70000, (H, W)), prev_len).astype(np.uint32)
    spoil = rng.random((H, W))
    rule = lambda i: (spoil >= 0.015 * i) & (spoil < 0.015 * (i + 1))      # noqa: E731
    prev_g["face"][rule(0)] = MISS
    prev_g["material"][rule(1)] |= np.uint32(EMISSIVE)
    prev_g["material"][rule(2)] += 4
    n60 = 0.5 * pn[by, bx] + np.sqrt(0.75) * np.cross(pn[by, bx], right)   # 60 degrees off
    prev_g["normal"][rule(3)] = (n60 / np.linalg.norm(n60, axis=-1, keepdims=True))[rule(3)]
    off = prev_g["position"] + (rng.uniform(0.5, 2.0, (H, W, 1)) * pn[by, bx]).astype(F)
    prev_g["position"][rule(4)] = off[rule(4)]
    prev_len[rule(5)] = 0
    prev_c = (rng.random((H, W, 3)) ** 4 * 100.0).astype(F)
    # ---- current frame
    if identity:
        tu, tv = xs.astype(np.float64), ys.astype(np.float64)
    else:
        wide = rng.random((H, W)) < 0.25
        tu = np.where(wide, rng.uniform(-2.0, W + 1.0, (H, W)), rng.uniform(0.0, W - 1.0, (H, W)))
        tv = np.where(wide, rng.uniform(-2.0, H + 1.0, (H, W)), rng.uniform(0.0, H - 1.0, (H, W)))
    kind = rng.random((H, W))
    far = (kind >= 0.08) & (kind < 0.12) & (not identity)     # wholly off the frame
    tu = np.where(far, np.where(rng.random((H, W)) < 0.5, rng.uniform(-2.0, -1.01, (H, W)),
                                rng.uniform(W + 0.01, W + 1.0, (H, W))), tu)
    cby = np.clip(np.floor(tv + 0.5).astype(np.int64), 0, H - 1) // BLOCK
    cbx = np.clip(np.floor(tu + 0.5).astype(np.int64), 0, W - 1) // BLOCK
    g = np.zeros((H, W), dtype=GBUFFER_DTYPE)
    x = hit(tu, tv, cby, cbx)
    behind = kind < 0.03                                       # z < 0: mirrored through the camera
    x = np.where(behind[..., None], 2.0 * cam_pos - x, x)
    x = np.where(((kind >= 0.03) & (kind < 0.04))[..., None], cam_pos, x)      # z == 0
    g["position"] = x
    g["normal"] = pn[cby, cbx]
    g["material"] = pmat[cby, cbx]
    g["material"][(kind >= 0.04) & (kind < 0.08)] = 9          # no history texel has it
    g["face"] = rng.integers(0, 1000, (H, W))
    nf = rng.random((H, W))
    g["face"][nf < 0.05] = MISS
    g["material"][(nf >= 0.05) & (nf < 0.10)] |= np.uint32(EMISSIVE)
    c = (rng.random((H, W, 3)) ** 4 * 100.0).astype(F)
    # ---- the mix
    if W * H >= MIX_MIN_PIXELS and min(W, H) >= 2:
        _, _, nt = accumulate(c, g, prev_c, prev_g, prev_len, None if identity else view, p, True)
        nt = nt[filterable(g)]
        if identity:
            assert np.mean(nt == 1) >= 0.5 and np.mean(nt == 0) >= 0.1, np.bincount(nt) / nt.size
        else:
            assert np.mean(nt == 4) >= 0.2, np.bincount(nt, minlength=5) / nt.size
            assert np.mean((nt >= 1) & (nt <= 3)) >= 0.1, np.bincount(nt, minlength=5) / nt.size
            assert np.mean(nt == 0) >= 0.1, np.bincount(nt, minlength=5) / nt.size
    return c, g, prev_c, prev_g, prev_len, view


# The quality gate: a static camera on the Cornell box at 64^2, SPP = 4, 8
# frames (time seeds 5.0 ... 12.0) accumulated at the defaults reach RATIO_MEASURED =
# rmse(accumulated) / rmse(first raw frame) against the oracle at SPP = 2048 (filterable pixels).
# The gate is that value plus a quarter of the distance to 1 (denoise_ref.QUALITY_GATE's rule).
RATIO_MEASURED = 0.424      # rmse 0.1374 -> 0.0583
QUALITY_GATE = RATIO_MEASURED + (1.0 - RATIO_MEASURED) / 4.0
QUALITY_SEEDS = tuple(5.0 + i for i in range(8))
