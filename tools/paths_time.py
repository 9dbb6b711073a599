#!/usr/bin/env python3
"""Device time of the path queries on one GPU.

Workloads, each after WARMUP untimed rounds, REPEATS (default 12, at least 10) timed rounds with
the arms alternating inside each round; min / median / max of the device times (HIP events:
rvcp_paths_wait for a query, rvcp_stats_t.kernel_ms for a render) and Msamples/s at the median:

  cornell_spp4, cornell_spp30   the SIZE^2 (default 1024) frame's own rays and seeds
      (rvcp_primary_rays_async, rvcp_primary_seeds_async) through rvcp_trace_paths_async, against
      rvcp_render_async with the linear output on a kernel_variant = 1, specialize = OFF context
      (the like-for-like: the same machine form and the same scan) and on the default context
      (the price of not being scene-specialised).  The query's result is compared with the
      variant-1 render's linear frame, bit for bit (`equals_render`).
  tree_spp4, tree_spp30         the same on Cornell + 2000 random triangles with accel = BVH,
      against that context's own render.
  incoherent_spp4               2^20 rays, origins uniform in the scene's box, directions uniform
      on the sphere, seeds uniform in [0, 1): the query alone.

--static-ab: the query's arm twice, with the queue and with one static ray per lane (a grid of as
many lanes as rays), alternating.  It needs the debug build of the library, which reads the arm
per call (RVCP_LIB=.../csrc/build/librvcp_debug.so).

Prints one JSON line and, with --out, writes it to a file (profiles/paths_time.json and
profiles/paths_time_static_ab.json are this tool's output).

    timeout -k 10 600 python tools/paths_time.py [--size 1024] [--repeats 12] [--warmup 3] [--out F]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rvcp_amd                 # noqa: E402
from rvcp_amd import abi        # noqa: E402

N_INCOHERENT = 1 << 20
TREE_TRIS = 2000
SEED = 0x50415448


def spread(x):
    return dict(median=statistics.median(x), min=min(x), max=max(x))


def incoherent(torch, sc, n, seed):
    """([n, 8] rays, [n] seeds) float32 on the device."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    p = torch.from_numpy(sc.mesh.aligned_vertices()["position"][:, :3].copy()).cuda()
    lo, hi = p.min(0).values, p.max(0).values
    o = lo + (hi - lo) * torch.rand((n, 3), generator=g, device="cuda")
    d = torch.randn((n, 3), generator=g, device="cuda")
    d = d / d.norm(dim=1, keepdim=True)
    t = torch.tensor([1e-2, 1e4], device="cuda").expand(n, 2)
    rays = torch.cat([o, d, t], dim=1).to(torch.float32).contiguous()
    seeds = torch.rand(n, generator=g, device="cuda", dtype=torch.float32).clamp_(0.0, 0.99999994)
    return rays, seeds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--static-ab", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    if a.static_ab and not abi.LIB_PATH.endswith("librvcp_debug.so"):
        ap.error("--static-ab needs RVCP_LIB=<csrc/build/librvcp_debug.so>")
    import torch
    n = a.size
    cornell = rvcp_amd.Scene.default()
    tree = rvcp_amd.scene.with_random_triangles(cornell, TREE_TRIS)
    res = dict(size=n, n_incoherent=N_INCOHERENT, repeats=a.repeats, warmup=a.warmup, seed=SEED,
               device=torch.cuda.get_device_name(0), version=abi.load().rvcp_version().decode(),
               static_ab=bool(a.static_ab))
    q_arms = ("query_queue", "query_static") if a.static_ab else ("query",)

    def run_query(rt, arm, d_r, d_s, count, spp, d_o):
        if a.static_ab:
            os.environ["RVCP_DEBUG_PATHS_STATIC"] = "1" if arm == "query_static" else "0"
        rt.trace_paths_async(d_r.data_ptr(), d_s.data_ptr(), count, spp, d_o.data_ptr())
        return rt.paths_wait()

    def frame_workload(sc, spp, renders):
        """renders: {arm: RayTracer keywords}; the query runs on the first arm's context."""
        push = sc.push_constant(0.0)
        px = n * n
        rts = {arm: rvcp_amd.RayTracer(spp=spp, **kw) for arm, kw in renders.items()}
        try:
            for rt in rts.values():
                rt.upload_scene(sc)
            first = next(iter(rts.values()))
            d_r = torch.zeros((px, 8), dtype=torch.float32, device="cuda")
            d_s = torch.zeros(px, dtype=torch.float32, device="cuda")
            first.primary_rays_async(push, n, n, d_r.data_ptr())
            first.primary_seeds_async(push, n, n, d_s.data_ptr())
            d_o = torch.zeros((px, 3), dtype=torch.float32, device="cuda")
            d_rgba = torch.zeros(px, dtype=torch.int32, device="cuda")
            d_lin = torch.zeros((px, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ms = {arm: [] for arm in q_arms + tuple(rts)}
            trav = {}
            equal = None
            for r in range(a.warmup + a.repeats):
                for arm in q_arms:
                    t, trav[arm] = run_query(first, arm, d_r, d_s, px, spp, d_o)
                    if r >= a.warmup:
                        ms[arm].append(t)
                for arm, rt in rts.items():
                    rt.render_async(push, n, n, d_rgba.data_ptr(), d_lin.data_ptr())
                    st = rt.wait()
                    trav[arm] = int(st["traversals"])
                    if r >= a.warmup:
                        ms[arm].append(float(st["kernel_ms"]))
                    if equal is None:       # against the first render arm's linear frame
                        equal = bool(torch.equal(d_o.view(torch.int32), d_lin.view(torch.int32)))
            out = dict(faces=len(sc.mesh.aligned_faces()), spp=spp, rays=px, equals_render=equal)
            for arm, v in ms.items():
                out[arm + "_ms"] = spread(v)
                out[arm + "_msamples_s"] = px * spp / statistics.median(v) / 1e3
                out[arm + "_traversals"] = trav[arm]
            q = out[q_arms[0] + "_ms"]["median"]
            for arm in rts:
                out[f"query_vs_{arm}"] = q / out[arm + "_ms"]["median"]
            if a.static_ab:
                out["queue_vs_static"] = q / out["query_static_ms"]["median"]
            return out
        finally:
            for rt in rts.values():
                rt.close()

    cornell_arms = {"render_v1": dict(kernel_variant=1, specialize=abi.SPECIALIZE_OFF),
                    "render_default": dict()}
    for spp in (4, 30):
        res[f"cornell_spp{spp}"] = frame_workload(cornell, spp, cornell_arms)
        res[f"tree_spp{spp}"] = frame_workload(tree, spp, {"render_tree": dict(accel=abi.ACCEL_BVH)})
    with rvcp_amd.RayTracer(spp=4) as rt:
        rt.upload_scene(cornell)
        d_r, d_s = incoherent(torch, cornell, N_INCOHERENT, SEED)
        d_o = torch.zeros((N_INCOHERENT, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ms = {arm: [] for arm in q_arms}
        trav = {}
        for r in range(a.warmup + a.repeats):
            for arm in q_arms:
                t, trav[arm] = run_query(rt, arm, d_r, d_s, N_INCOHERENT, 4, d_o)
                if r >= a.warmup:
                    ms[arm].append(t)
        out = dict(faces=len(cornell.mesh.aligned_faces()), spp=4, rays=N_INCOHERENT)
        for arm, v in ms.items():
            out[arm + "_ms"] = spread(v)
            out[arm + "_msamples_s"] = N_INCOHERENT * 4 / statistics.median(v) / 1e3
            out[arm + "_traversals"] = trav[arm]
        if a.static_ab:
            out["queue_vs_static"] = out["query_queue_ms"]["median"] / out["query_static_ms"]["median"]
        res["incoherent_spp4"] = out
    line = json.dumps(res, allow_nan=False)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
