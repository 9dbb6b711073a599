#!/usr/bin/env python3
"""Device time of the material scattering mode on one GPU (rvcp_set_materials).

For SPP 4 and 30 at SIZE^2 (default 1024), each after WARMUP untimed rounds, REPEATS (default 12,
at least 10) timed rounds with the arms alternating inside each round; min / median / max of the
device times (HIP events: rvcp_paths_wait for a query, rvcp_stats_t.kernel_ms for a render):

  a  query_off        the Cornell box frame's own rays and seeds through rvcp_trace_paths_async
                      with the mode off (path_query_kernel)
  b  query_on         the same rays with the mode on: what the material branch costs on a scene
                      that never takes it (path_scatter_kernel; the results are compared, bit for
                      bit: `on_equals_off`)
  c  query_specular   scene.specular_cornell_scene()'s frame with the mode on
  d  render_on        rvcp_render_async of the Cornell box with the mode on, against
     render_default   the default context's render of it (the scene-specialised schedule)
  e  tree_render_on   the same two on specular_cornell_scene() + 2000 random triangles,
     tree_render_off  accel = BVH (mode off: every face Lambertian, the BVH path kernel)

Prints one JSON line and, with --out, writes it to a file (profiles/materials_time.json is this
tool's output).

    timeout -k 10 600 python tools/materials_time.py [--size 1024] [--repeats 12] [--out F]
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

TREE_TRIS = 2000


def spread(x):
    return dict(median=statistics.median(x), min=min(x), max=max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    import torch
    n = a.size
    px = n * n
    cornell = rvcp_amd.Scene.default()
    specular = rvcp_amd.scene.specular_cornell_scene()
    tree = rvcp_amd.scene.with_random_triangles(specular, TREE_TRIS)
    res = dict(size=n, repeats=a.repeats, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), version=abi.load().rvcp_version().decode())

    def context(sc, spp, mode, **kw):
        rt = rvcp_amd.RayTracer(spp=spp, **kw)
        rt.materials = mode
        rt.upload_scene(sc)
        return rt

    def frame_inputs(rt, sc):
        push = sc.push_constant(0.0)
        d_r = torch.zeros((px, 8), dtype=torch.float32, device="cuda")
        d_s = torch.zeros(px, dtype=torch.float32, device="cuda")
        rt.primary_rays_async(push, n, n, d_r.data_ptr())
        rt.primary_seeds_async(push, n, n, d_s.data_ptr())
        torch.cuda.synchronize()
        return d_r, d_s

    for spp in (4, 30):
        on, off = abi.MATERIALS_SCATTER, abi.MATERIALS_LAMBERTIAN
        rts = dict(query_off=context(cornell, spp, off), query_on=context(cornell, spp, on),
                   query_specular=context(specular, spp, on),
                   render_on=context(cornell, spp, on), render_default=context(cornell, spp, off),
                   tree_render_on=context(tree, spp, on, accel=abi.ACCEL_BVH),
                   tree_render_off=context(tree, spp, off, accel=abi.ACCEL_BVH))
        scenes = dict(query_off=cornell, query_on=cornell, query_specular=specular,
                      render_on=cornell, render_default=cornell, tree_render_on=tree,
                      tree_render_off=tree)
        try:
            inputs = {arm: frame_inputs(rts[arm], scenes[arm])
                      for arm in ("query_off", "query_specular")}
            inputs["query_on"] = inputs["query_off"]
            d_o = {arm: torch.zeros((px, 3), dtype=torch.float32, device="cuda") for arm in inputs}
            d_rgba = torch.zeros(px, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ms = {arm: [] for arm in rts}
            trav, variant = {}, {}
            for r in range(a.warmup + a.repeats):
                for arm, rt in rts.items():
                    if arm in inputs:
                        d_r, d_s = inputs[arm]
                        rt.trace_paths_async(d_r.data_ptr(), d_s.data_ptr(), px, spp,
                                             d_o[arm].data_ptr())
                        t, trav[arm] = rt.paths_wait()
                    else:
                        rt.render_async(scenes[arm].push_constant(0.0), n, n, d_rgba.data_ptr())
                        st = rt.wait()
                        t, trav[arm] = float(st["kernel_ms"]), int(st["traversals"])
                        variant[arm] = int(st["kernel_variant"])
                    if r >= a.warmup:
                        ms[arm].append(t)
            out = dict(spp=spp, rays=px, kernel_variant=variant,
                       on_equals_off=bool(torch.equal(d_o["query_on"].view(torch.int32),
                                                      d_o["query_off"].view(torch.int32))))
            for arm, v in ms.items():
                out[arm + "_ms"] = spread(v)
                out[arm + "_traversals"] = trav[arm]
            med = lambda arm: out[arm + "_ms"]["median"]        # noqa: E731
            out["b_over_a"] = med("query_on") / med("query_off")
            out["c_over_a"] = med("query_specular") / med("query_off")
            out["d_render_on_over_default"] = med("render_on") / med("render_default")
            out["e_tree_on_over_off"] = med("tree_render_on") / med("tree_render_off")
            res[f"spp{spp}"] = out
        finally:
            for rt in rts.values():
                rt.close()
    line = json.dumps(res, allow_nan=False)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
