"""The ray queries' reference (rvcp_trace_rays_async): the nearest hit of each
ray as get_intersection_with_scene keeps it, by walking the faces in order through the oracle's
own is_intersect_with_face under the keep rule (oracle.intersect_array, rays[:, 7] the running
bt).  Test infrastructure; no number in it comes from the code under test.

Two rules are the header's and not the shader's, restated here from include/rvcp.h: a miss is
reported as face -1 with t = b1 = b2 = 0, and a ray with a non-finite word is a miss."""
import numpy as np

import oracle

RAY_DTYPE = np.dtype([("o", "<f4", 3), ("d", "<f4", 3), ("t_min", "<f4"), ("t_max", "<f4")])
RAY_HIT_DTYPE = np.dtype([("face", "<i4"), ("t", "<f4"), ("b1", "<f4"), ("b2", "<f4")])


def triangles(scene_arrays):
    """[F, 9] float32 vertex positions of a scene_arrays dict (conftest.scene_arrays), or a
    [F, 3, 3] position array as tests/bvh_adversarial.py's Mesh.pos."""
    if isinstance(scene_arrays, dict):
        v = scene_arrays["vertices"]["position"][:, :3]
        return np.ascontiguousarray(v[scene_arrays["faces"]["vertices"]], np.float32).reshape(-1, 9)
    return np.ascontiguousarray(scene_arrays, np.float32).reshape(-1, 9)


def nearest(scene_arrays, rays):
    """RAY_HIT_DTYPE [R]: the scan's nearest hit of every ray (the later face at equal t)."""
    tris = triangles(scene_arrays)
    rays = np.ascontiguousarray(rays).view(RAY_DTYPE).reshape(-1)
    r8 = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()
    out = np.zeros(len(rays), RAY_HIT_DTYPE)
    out["face"] = -1
    live = np.flatnonzero(np.isfinite(r8).all(axis=1))
    if len(live) == 0:
        return out
    cur = r8[live]
    res = out[live]
    for i, tri in enumerate(tris):
        hit, o = oracle.intersect_array(cur, np.broadcast_to(tri, (len(cur), 9)))
        cur[hit, 7] = o[hit, 0]
        res["face"][hit] = i
        res["t"][hit], res["b1"][hit], res["b2"][hit] = o[hit, 0], o[hit, 1], o[hit, 2]
    out[live] = res
    return out


def any_hit(scene_arrays, rays):
    """uint32 [R]: 1 where something lies in [t_min, t_max]."""
    return (nearest(scene_arrays, rays)["face"] >= 0).astype(np.uint32)
