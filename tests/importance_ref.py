"""importance_ref -- the cosine-weighted bounce of RVCP_SAMPLING_COSINE,
restated in pure Python on tests/pyref.py's primitives (TEST INFRASTRUCTURE ONLY).

`trace` is pyref.trace with the continuation half of the surface event replaced and nothing
else: the scans, the light sample, the Russian-roulette test, the attenuation stop, the miss
and light terms and the count and order of rand() calls (one for the roulette, then the
unit-ball rejection loop) are the shader's.  With p the accepted unit-ball sample and n the
shading normal:

    q   = normalize(p)                   v * (1 / sqrt(dot(v, v)))
    h   = n + q
    wi  = n if dot(h, h) < 1e-12 else normalize(h)
    att = att * (f * k)                  f = albedo / PI per channel, k = PI / rr, one division

h is a point of the unit sphere that touches the surface at the hit, so its direction from the
hit has density cos / pi and the path weight f cos / (pdf rr) is albedo / rr for every
direction: no cosine factor, no pdf, and no max(0.1, pdf) clamp, which would bias the grazing
directions whose cos / pi is below 0.1.

It shares no code with the library; the GPU tests compare the kernels with fixtures it wrote
(tests/golden/make_importance_fixture.py) bit for bit."""
from __future__ import annotations

import numpy as np

import pyref
from pyref import F, PI, Rng, add, cross, div, dot, face_area, length, mul, neg, normalize, \
    scale, scene_hit, sub, unit_sphere, v

HH_MIN = F(1e-12)       # below it n and normalize(p) cancel: the direction is the normal


def bounce(n, p):
    """The continuation direction for shading normal n and accepted unit-ball sample p."""
    with np.errstate(all="ignore"):
        q = normalize(p)
        h = add(n, q)
        return n if dot(h, h) < HH_MIN else normalize(h)


def trace(sc, P, g, o, d, tmin, tmax, counter):
    color = v(0, 0, 0)
    att = v(1, 1, 1)
    k = F(PI / P["rr"])                  # the frame constant beside brdf_den / brdf_rcp
    for depth in range(P["max_bounces"]):
        if att[0] < P["att_stop"] and att[1] < P["att_stop"] and att[2] < P["att_stop"]:
            break
        t, p, n, mid, _ = scene_hit(sc, o, d, tmin, tmax, counter)
        if t > tmax:
            color = add(color, v(0.1, 0.1, 0.1))
            break
        alb, ty = sc.mat[mid]
        if ty == 3:
            if depth == 0:
                color = add(color, mul(att, alb))
            break
        nl = len(sc.lum)
        if nl:
            S = F(0.0)
            for i in range(nl):
                S = F(S + face_area(sc, sc.lum_id(i)))
            pl = F(g() * S)
            pdf = F(F(1.0) / S)
            acc = F(0.0)
            chosen = None
            for i in range(nl):
                fid = sc.lum_id(i)
                acc = F(acc + face_area(sc, fid))
                if pl <= acc:
                    chosen = fid
                    break
            if chosen is not None:
                (j0, j1, j2), lmid = sc.faces[chosen]
                x = F(np.sqrt(g()))
                y = g()
                X = add(add(scale(sc.pos[j0], F(F(1.0) - x)), scale(sc.pos[j1], F(x * F(F(1.0) - y)))),
                        scale(sc.pos[j2], F(x * y)))
                Xn = normalize(sc.nrm[j0])
                dist = length(sub(X, p))
                ws = div(sub(X, p), dist)
                _, bp, _, _, _ = scene_hit(sc, add(p, scale(ws, P["eps"])), ws, P["t_min"], P["t_max"],
                                        counter)
                db = length(sub(bp, p))
                if abs(F(dist - db)) < P["eps"]:
                    fb = div(alb, PI) if dot(n, ws) > 0 else v(0, 0, 0)
                    c = mul(mul(att, sc.mat[lmid][0]), fb)
                    c = scale(c, dot(n, ws))
                    c = scale(c, dot(Xn, neg(ws)))
                    c = div(c, F(F(dist * dist) * pdf))
                    color = add(color, c)
        if g() > P["rr"]:
            break
        # ---- the continuation: the only lines that differ from pyref.trace ----
        wi = bounce(n, unit_sphere(g))
        with np.errstate(all="ignore"):
            att = mul(att, scale(div(alb, PI), k))
        o, d, tmin, tmax = add(p, scale(wi, P["eps"])), wi, P["t_min"], P["t_max"]
    return color


def render_pixel(sc, P, push, W, H, x, y):
    """pyref.render_pixel's games101 half with `trace` above: linear RGB of pixel (x, y) and
    the traversal count."""
    cam = push["camera"]
    cpos = tuple(F(c) for c in cam["position"][:3])
    up = tuple(F(c) for c in cam["up"][:3])
    fwd = tuple(F(c) for c in cam["forward"])
    tn, tf, fov = F(cam["t_near"]), F(cam["t_far"]), F(cam["vertical_fov"])
    u_ = F(F(F(x) + F(0.5)) / F(W))
    v_ = F(F(F(y) + F(0.5)) / F(H))
    g = Rng(F(push["time"]), u_, v_)
    rad = F(F(F(fov / F(2.0)) * PI) / F(180.0))
    h = F(F(F(2.0) * tn) * F(pyref._libm.tanf(float(rad))))
    w = F(F(h * F(W)) / F(H))
    uu = scale(normalize(cross(fwd, up)), w)
    vv = scale(normalize(cross(fwd, uu)), h)
    pos = add(cpos, scale(fwd, tn))
    uvp = add(add(pos, scale(uu, F(u_ - F(0.5)))), scale(vv, F(v_ - F(0.5))))
    tc = F(length(sub(uvp, cpos)) / length(sub(pos, cpos)))
    d = normalize(sub(uvp, cpos))
    counter = [0]
    color = v(0, 0, 0)
    for _ in range(P["spp"]):
        L = trace(sc, P, g, cpos, d, F(tn * tc), F(tf * tc), counter)
        color = add(color, div(L, F(P["spp"])))
    return color, counter[0]


# The cases of tests/golden/importance_frames.npz: name -> (scene, W, H); all in cosine mode at
# time FIXTURE_TIME.  The fuzz scenes (tests/fuzz_scenes.py) come with their own configs: seed 2
# is a room at scale 1 seen from inside (max_bounces 3, the std140 light pick), seed 3 one at
# scale 2^22 moved out by 2^38, seen from outside (max_bounces 15, the light pick by face id).
FIXTURE_TIME = 41.0
CASES = {
    "cornell_16x16_spp3": ("cornell", 16, 16),
    "rotated_12x12_spp2": ("rotated", 12, 12),
    "fuzz2_12x10": ("fuzz2", 12, 10),
    "fuzz3_12x10": ("fuzz3", 12, 10),
}


def case_scene(case):
    """(package Scene, config kwargs, W, H) of a fixture case."""
    import rvcp_amd
    kind, W, H = CASES[case]
    if kind == "cornell":
        return rvcp_amd.Scene.default(), dict(spp=3), W, H
    if kind == "rotated":
        return rvcp_amd.scene.rotated_scene(rvcp_amd.Scene.default()), dict(spp=2), W, H
    from fuzz_scenes import fuzz_scene
    sc, kw, _ = fuzz_scene(int(kind[4:]))
    return sc, kw, W, H


def render(scene, cfg, push, W, H, pixels=None):
    """(linear [H, W, 3] float32, traversals [H, W] uint32) of a package Scene under
    abi.make_config record `cfg`; `pixels`: only these (x, y), the rest left 0."""
    ps = pyref.Scene(scene.aligned_materials(), scene.mesh.aligned_vertices(),
                     scene.mesh.aligned_faces(), scene.luminous_face_ids(),
                     quirk=bool(cfg["lum_id_std140_quirk"]))
    P = pyref.params(cfg)
    lin = np.zeros((H, W, 3), np.float32)
    trav = np.zeros((H, W), np.uint32)
    for (x, y) in (pixels if pixels is not None else [(x, y) for y in range(H) for x in range(W)]):
        c, n = render_pixel(ps, P, push, W, H, x, y)
        lin[y, x] = np.array(c, np.float32)
        trav[y, x] = n
    return lin, trav
