"""The path queries' reference (rvcp_trace_paths_async): the radiance along each
ray and the traversals it stands for, by pyref.trace (TEST INFRASTRUCTURE ONLY; no number in it
comes from the code under test).

Ray i with seed s and `spp` samples is main's loop (ray_tracer_games101_branch.comp:493-496) for a
pixel whose sample_ray is the ray as given and whose srand result is s: an Rng whose seed is set
directly and whose index is 0 runs on through the samples, and color += ray_trace(ray) / spp --
the accumulation of pyref.render_pixel's games101 half.  The header's two own rules are restated
here: a ray with a non-finite word, or a seed outside [0, 1) (a NaN seed is outside), gives zeros
and no traversal."""
import numpy as np

import pyref

F = np.float32
RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("d", "<f4", (3,)), ("t_min", "<f4"), ("t_max", "<f4")])


def scene_of(scene, cfg):
    """(pyref.Scene, pyref.params) of a package Scene under an abi.make_config record."""
    sc = pyref.Scene(scene.aligned_materials(), scene.mesh.aligned_vertices(),
                     scene.mesh.aligned_faces(), scene.luminous_face_ids(),
                     quirk=bool(cfg["lum_id_std140_quirk"]))
    return sc, pyref.params(cfg)


def rejected(ray, seed):
    words = np.frombuffer(np.asarray(ray).tobytes(), "<f4")
    seed = F(seed)
    return not np.isfinite(words).all() or not (F(0.0) <= seed < F(1.0))


def radiance(sc, P, ray, seed, spp):
    """((r, g, b) float32, traversals) of one ray."""
    if rejected(ray, seed):
        return pyref.v(0, 0, 0), 0
    g = pyref.Rng.__new__(pyref.Rng)
    g.seed = F(seed)
    g.index = F(0.0)
    o = tuple(F(x) for x in ray["o"])
    d = tuple(F(x) for x in ray["d"])
    counter = [0]
    color = pyref.v(0, 0, 0)
    with np.errstate(all="ignore"):
        for _ in range(spp):
            L = pyref.trace(sc, P, g, o, d, F(ray["t_min"]), F(ray["t_max"]), counter)
            color = pyref.add(color, pyref.div(L, F(spp)))
    return color, counter[0]


def trace_paths(scene, cfg, rays, seeds, spp):
    """(linear [n, 3] float32, traversals [n] uint64) of the rays (RAY_DTYPE records)."""
    sc, P = scene_of(scene, cfg)
    rays = np.ascontiguousarray(rays).view(RAY_DTYPE).reshape(-1)
    seeds = np.ascontiguousarray(seeds, dtype=F).reshape(-1)
    assert len(rays) == len(seeds)
    lin = np.zeros((len(rays), 3), F)
    trav = np.zeros(len(rays), np.uint64)
    for i, (r, s) in enumerate(zip(rays, seeds)):
        c, t = radiance(sc, P, r, s, spp)
        lin[i] = c
        trav[i] = t
    return lin, trav


def frame_seeds(time, W, H):
    """The seeds main() gives the pixels of a W x H frame, row-major: srand(time, u, v)."""
    out = np.zeros(W * H, F)
    for y in range(H):
        v_ = F(F(F(y) + F(0.5)) / F(H))
        for x in range(W):
            u_ = F(F(F(x) + F(0.5)) / F(W))
            out[y * W + x] = pyref.Rng(F(time), u_, v_).seed
    return out
