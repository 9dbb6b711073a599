"""materials_ref -- the opt-in material scattering of RVCP_MATERIALS_SCATTER,
restated in pure Python on tests/pyref.py's primitives (TEST INFRASTRUCTURE ONLY; no number in it
comes from the code under test).

`trace` is pyref.trace (ray_trace_games101, :406-482) with these changes and no other:

1. At a hit whose material is Metal (1) or Dielectric (2) no light sample is drawn and no shadow
   ray traced.  The roulette comes first (`if (rand() > RR_PROBABILITY) break;`, :462), then the
   new direction nd and colour na are material_scatter's (ray_tracer.comp:491-602, in the
   arithmetic of pyref.trace_legacy), attenuation *= na / RR_PROBABILITY (a vec3 division, then a
   component-wise product), and the next ray is Ray(p + nd * EPS, nd, RAY_T_MIN, RAY_T_MAX).
2. The emission rule (:426) is `depth == 0 || the previous vertex was specular`.
3. Shadow rays are unchanged: a metal or glass face blocks them.
4. The metal redraw is bounded: after METAL_RETRIES rejected draws nd = normalize(r), the
   unfuzzed flipped reflection.

On a scene without a Metal or Dielectric face it is pyref.trace bit for bit
(tests/test_materials_cpu.py).  The GPU tests compare the kernel with it, and with the frames it
wrote into tests/golden/materials_frames.npz (tests/golden/make_materials_fixture.py)."""
from __future__ import annotations

import numpy as np

import paths_ref
import pyref
from pyref import F, PI, Rng, add, cross, div, dot, face_area, length, mul, neg, normalize, \
    reflect, refract, scale, scene_hit, sub, unit_sphere, v

METAL_RETRIES = 16
EVENTS = ("metal_hits", "metal_redraws", "dielectric_hits", "refractions", "fresnel_reflections",
          "total_internal_reflections", "lights_behind_specular", "misses_behind_specular",
          "lambertian_hits")


def new_events():
    return dict.fromkeys(EVENTS, 0)


def metal_direction(r, n, fuzz, draw, ev=None):
    """metal_scatter's direction (ray_tracer.comp:528-530) for the flipped reflection r: the
    first of at most METAL_RETRIES normalize(r + fuzz * normalize(draw())) that does not point
    below the surface, else normalize(r).  draw() returns a unit-ball sample."""
    with np.errstate(all="ignore"):
        for _ in range(METAL_RETRIES):
            nd = normalize(add(r, scale(normalize(draw()), fuzz)))
            if not dot(nd, n) < 0:
                return nd
            if ev is not None:
                ev["metal_redraws"] += 1
        return normalize(r)


def scatter(sc, P, g, d, n, mid, outward, ev):
    """(nd, na) of material_scatter for a Metal or Dielectric hit."""
    alb, ty = sc.mat[mid]
    if ty == 1:
        r = reflect(d, n)
        if dot(r, n) < 0:
            r = neg(r)
        return metal_direction(r, n, sc.fuzz[mid], lambda: unit_sphere(g), ev), alb
    with np.errstate(all="ignore"):
        ratio = F(F(1.0) / sc.ior[mid]) if outward else sc.ior[mid]
        ct = dot(neg(d), n)
        st = F(np.sqrt(F(F(1.0) - F(ct * ct))))
        refr = bool(F(ratio * st) <= 1.0)
        if refr:
            r0 = F(F(F(1.0) - ratio) / F(F(1.0) + ratio))
            r0 = F(r0 * r0)
            x = F(F(1.0) - ct)
            fr = F(r0 + F(F(F(1.0) - r0) * F(F(F(x * x) * F(x * x)) * x)))
            refr = bool(g() >= fr)
            ev["refractions" if refr else "fresnel_reflections"] += 1
        else:
            ev["total_internal_reflections"] += 1
        nd = refract(d, n, ratio) if refr else reflect(d, n)
    return nd, v(1, 1, 1)


def trace(sc, P, g, o, d, tmin, tmax, counter, ev=None):
    ev = new_events() if ev is None else ev
    color = v(0, 0, 0)
    att = v(1, 1, 1)
    specular = False                    # the previous vertex was a Metal or Dielectric one
    for depth in range(P["max_bounces"]):
        if att[0] < P["att_stop"] and att[1] < P["att_stop"] and att[2] < P["att_stop"]:
            break
        t, p, n, mid, outward = scene_hit(sc, o, d, tmin, tmax, counter)
        if t > tmax:
            color = add(color, v(0.1, 0.1, 0.1))
            if specular:
                ev["misses_behind_specular"] += 1
            break
        alb, ty = sc.mat[mid]
        if ty == 3:
            if depth == 0 or specular:                                      # rule 2
                color = add(color, mul(att, alb))
                if specular:
                    ev["lights_behind_specular"] += 1
            break
        if ty == 1 or ty == 2:                                              # rule 1
            ev["metal_hits" if ty == 1 else "dielectric_hits"] += 1        # (before the roulette)
            if g() > P["rr"]:
                break
            nd, na = scatter(sc, P, g, d, n, mid, outward, ev)
            with np.errstate(all="ignore"):
                att = mul(att, div(na, P["rr"]))
                o, d, tmin, tmax = add(p, scale(nd, P["eps"])), nd, P["t_min"], P["t_max"]
            specular = True
            continue
        specular = False
        ev["lambertian_hits"] += 1
        # ---- from here on pyref.trace's Lambertian surface event, line for line ----
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
        while True:
            q = (F(F(F(2.0) * g()) - F(1.0)), F(F(F(2.0) * g()) - F(1.0)),
                 F(F(F(2.0) * g()) - F(1.0)))
            if not dot(q, q) >= 1.0:
                break
        h = q if dot(q, n) > 0 else neg(q)
        wi = normalize(h)
        fb = div(alb, PI) if dot(n, wi) > 0 else v(0, 0, 0)
        pdf_b = F(F(0.5) / PI) if dot(wi, n) > 0 else F(0.0)
        a = div(scale(fb, dot(n, wi)), F(max(F(0.1), pdf_b) * P["rr"]))
        att = mul(att, a)
        o, d, tmin, tmax = add(p, scale(wi, P["eps"])), wi, P["t_min"], P["t_max"]
    return color


def radiance(sc, P, ray, seed, spp, ev=None):
    """paths_ref.radiance with `trace` above: ((r, g, b) float32, traversals) of one ray."""
    if paths_ref.rejected(ray, seed):
        return v(0, 0, 0), 0
    g = Rng.__new__(Rng)
    g.seed = F(seed)
    g.index = F(0.0)
    o = tuple(F(x) for x in ray["o"])
    d = tuple(F(x) for x in ray["d"])
    counter = [0]
    color = v(0, 0, 0)
    with np.errstate(all="ignore"):
        for _ in range(spp):
            L = trace(sc, P, g, o, d, F(ray["t_min"]), F(ray["t_max"]), counter, ev)
            color = add(color, div(L, F(spp)))
    return color, counter[0]


def trace_paths(scene, cfg, rays, seeds, spp, ev=None):
    """(linear [n, 3] float32, traversals [n] uint64) of the rays (paths_ref.RAY_DTYPE records)."""
    sc, P = paths_ref.scene_of(scene, cfg)
    rays = np.ascontiguousarray(rays).view(paths_ref.RAY_DTYPE).reshape(-1)
    seeds = np.ascontiguousarray(seeds, dtype=F).reshape(-1)
    assert len(rays) == len(seeds)
    lin = np.zeros((len(rays), 3), F)
    trav = np.zeros(len(rays), np.uint64)
    for i, (r, s) in enumerate(zip(rays, seeds)):
        c, t = radiance(sc, P, r, s, spp, ev)
        lin[i] = c
        trav[i] = t
    return lin, trav


def render_pixel(sc, P, push, W, H, x, y, ev=None, trace_fn=None):
    """pyref.render_pixel's games101 half with `trace` above (trace_fn: another integrator with
    pyref.trace's signature): linear RGB of pixel (x, y) and the traversal count."""
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
    with np.errstate(all="ignore"):
        for _ in range(P["spp"]):
            if trace_fn is not None:
                L = trace_fn(sc, P, g, cpos, d, F(tn * tc), F(tf * tc), counter)
            else:
                L = trace(sc, P, g, cpos, d, F(tn * tc), F(tf * tc), counter, ev)
            color = add(color, div(L, F(P["spp"])))
    return color, counter[0]


def render(scene, cfg, push, W, H, ev=None, trace_fn=None):
    """(linear [H, W, 3] float32, traversals [H, W] uint32) of a package Scene under
    abi.make_config record `cfg`."""
    sc, P = paths_ref.scene_of(scene, cfg)
    lin = np.zeros((H, W, 3), np.float32)
    trav = np.zeros((H, W), np.uint32)
    for y in range(H):
        for x in range(W):
            c, n = render_pixel(sc, P, push, W, H, x, y, ev, trace_fn)
            lin[y, x] = np.array(c, np.float32)
            trav[y, x] = n
    return lin, trav


# ---- the cases of tests/golden/materials_frames.npz -------------------------------------------
FIXTURE_TIME = 7.0
# name -> (scene kind, scene kwargs, config kwargs, W, H)
CASES = {
    "default": ("specular", {}, dict(spp=2), 24, 16),
    "fuzz03": ("specular", dict(fuzz=0.3), dict(spp=2), 24, 16),
    "noquirk": ("specular", {}, dict(spp=2, lum_id_std140_quirk=0), 24, 16),
    "short": ("specular", {}, dict(spp=2, max_bounces=3, rr_probability=1.0), 24, 16),
    "metal_box": ("metal_box", {}, dict(spp=1), 16, 12),
}


def metal_box_scene():
    """The Cornell box whose five walls (faces 2-11) are all fuzz = 1 metal: long specular
    chains and many redraws."""
    import rvcp_amd
    S = rvcp_amd.scene
    Face, Material, Mesh, Scene, vec3 = S.Face, S.Material, S.Mesh, S.Scene, S.vec3
    base = rvcp_amd.Scene.default()
    mats = list(base.materials) + [Material.new_metal(vec3(0.8, 0.8, 0.8), 1.0)]
    faces = [Face(f.vertices, len(mats) - 1 if 2 <= i <= 11 else f.material_id)
             for i, f in enumerate(base.mesh.faces)]
    return Scene(base.camera, mats, [], Mesh(list(base.mesh.vertices), faces))


def case_scene(case):
    """(package Scene, config kwargs, W, H) of a fixture case."""
    import rvcp_amd
    kind, skw, ckw, W, H = CASES[case]
    sc = rvcp_amd.scene.specular_cornell_scene(**skw) if kind == "specular" else metal_box_scene()
    return sc, dict(ckw), W, H


def case_frame(case, ev=None):
    """(linear, traversals) of a fixture case, by the restatement."""
    from rvcp_amd import abi
    sc, kw, W, H = case_scene(case)
    return render(sc, abi.make_config(**kw), sc.push_constant(FIXTURE_TIME), W, H, ev)


# ---- the mirror test: 1024 rays straight down onto the mirror floor ------------------------------
MIRROR_N = 1024


def mirror_rays():
    """(rays, seeds): MIRROR_N rays from (10, 100, -20) straight down, seeds from default_rng(3)."""
    rays = np.zeros(MIRROR_N, paths_ref.RAY_DTYPE)
    rays["o"] = (10.0, 100.0, -20.0)
    rays["d"] = (0.0, -1.0, 0.0)
    rays["t_min"], rays["t_max"] = 0.01, 10000.0
    seeds = np.random.default_rng(3).random(MIRROR_N, dtype=np.float32)
    return rays, seeds


def mirror_result():
    """(linear, traversals) of the mirror rays at SPP 1 on specular_cornell_scene()."""
    import rvcp_amd
    from rvcp_amd import abi
    rays, seeds = mirror_rays()
    return trace_paths(rvcp_amd.scene.specular_cornell_scene(), abi.make_config(spp=1), rays,
                       seeds, 1)
