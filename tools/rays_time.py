#!/usr/bin/env python3
"""Throughput of the ray queries on one GPU.

Three scenes -- the Cornell box (accel = NONE: the generic scan), c6 (Cornell + 310 triangles,
accel = BVH: the hybrid) and the C5 mesh (Cornell + 100 000 triangles, accel = BVH) -- each with
two ray sets made on the device from a seed: the SIZE^2 (default 1024) primary rays
(rvcp_primary_rays_async) and 2^20 incoherent rays, origins uniform in the scene's box,
directions uniform on the sphere, t in [1e-2, 1e4].  Per scene, set and mode (NEAREST, ANY), after
WARMUP untimed rounds: the median, minimum and maximum of REPEATS (default 25, at least 20) device
times (rvcp_rays_wait, HIP events) and Mrays/s at the median.  The yardstick is the G-buffer
kernel on the same scene in the same rounds (HIP events around rvcp_render_gbuffer_async): it runs
the same tests on the same primary rays, and `nearest_primary_vs_gbuffer` is the ratio of medians.

--stack-ab: the A/B of the tree's traversal stack, private array against LDS columns, on the C5
mesh, alternating in one run.  It needs the debug build of the library, which reads the arm per
call (RVCP_LIB=.../csrc/build/librvcp_debug.so).

Prints one JSON line and, with --out, writes it to a file (profiles/rays_time.json and
profiles/rays_time_stack_ab.json are this tool's output).

    timeout -k 10 600 python tools/rays_time.py [--size 1024] [--repeats 25] [--warmup 5] [--out F]
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
C5_TRIS, C6_TRIS = 100000, 310
SEED = 0x52415953


def spread(x):
    return dict(median=statistics.median(x), min=min(x), max=max(x))


def incoherent_rays(torch, sc, n, seed):
    """[n, 8] float32 on the device: o uniform in the scene's box, d uniform on the sphere."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    p = torch.from_numpy(sc.mesh.aligned_vertices()["position"][:, :3].copy()).cuda()
    lo, hi = p.min(0).values, p.max(0).values
    o = lo + (hi - lo) * torch.rand((n, 3), generator=g, device="cuda")
    d = torch.randn((n, 3), generator=g, device="cuda")
    d = d / d.norm(dim=1, keepdim=True)
    t = torch.tensor([1e-2, 1e4], device="cuda").expand(n, 2)
    return torch.cat([o, d, t], dim=1).to(torch.float32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stack-ab", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    if a.stack_ab and not abi.LIB_PATH.endswith("librvcp_debug.so"):
        ap.error("--stack-ab needs RVCP_LIB=<csrc/build/librvcp_debug.so>")
    import torch
    n = a.size
    cornell = rvcp_amd.Scene.default()
    scenes = {"cornell_scan": (cornell, abi.ACCEL_NONE),
              "c6_hybrid": (rvcp_amd.scene.with_random_triangles(cornell, C6_TRIS), abi.ACCEL_BVH),
              "c5_bvh": (rvcp_amd.scene.with_random_triangles(cornell, C5_TRIS), abi.ACCEL_BVH)}
    if a.stack_ab:
        scenes = {"c5_bvh": scenes["c5_bvh"]}
    res = dict(size=n, n_incoherent=N_INCOHERENT, repeats=a.repeats, warmup=a.warmup, seed=SEED,
               device=torch.cuda.get_device_name(0), version=abi.load().rvcp_version().decode(),
               stack_ab=bool(a.stack_ab))
    side = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, (sc, accel) in scenes.items():
        push = sc.push_constant(0.0)
        with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
            rt.upload_scene(sc)
            d_prim = torch.zeros((n * n, 8), dtype=torch.float32, device="cuda")
            rt.primary_rays_async(push, n, n, d_prim.data_ptr(), stream=side.cuda_stream)
            sets = {"primary": d_prim, "incoherent": incoherent_rays(torch, sc, N_INCOHERENT, SEED)}
            d_g = torch.zeros(n * n * 32, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(max(n * n, N_INCOHERENT) * 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            arms = [(s, m, lds) for s in sets for m in ("nearest", "any")
                    for lds in (("private", "lds") if a.stack_ab else (None,))]
            ms = {arm: [] for arm in arms}
            gb = []
            for r in range(a.warmup + a.repeats):
                with torch.cuda.stream(side):
                    e0.record()
                    rt.render_gbuffer_async(push, n, n, d_g.data_ptr(), stream=side.cuda_stream)
                    e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    gb.append(e0.elapsed_time(e1))
                for arm in arms:
                    s, m, lds = arm
                    if lds is not None:
                        os.environ["RVCP_DEBUG_RAYS_LDS"] = "1" if lds == "lds" else "0"
                    rt.trace_rays_async(sets[s].data_ptr(), len(sets[s]), d_out.data_ptr(),
                                        abi.RAYS_ANY if m == "any" else abi.RAYS_NEAREST,
                                        stream=side.cuda_stream)
                    t = rt.rays_wait()
                    if r >= a.warmup:
                        ms[arm].append(t)
            out = dict(faces=len(sc.mesh.aligned_faces()), gbuffer_ms=spread(gb))
            for (s, m, lds), v in ms.items():
                key = f"{m}_{s}" + (f"_{lds}" if lds else "")
                out[key + "_ms"] = spread(v)
                out[key + "_mrays_s"] = len(sets[s]) / statistics.median(v) / 1e3
            if a.stack_ab:
                for s in sets:
                    for m in ("nearest", "any"):
                        out[f"{m}_{s}_lds_vs_private"] = (out[f"{m}_{s}_lds_ms"]["median"] /
                                                          out[f"{m}_{s}_private_ms"]["median"])
            else:
                out["nearest_primary_vs_gbuffer"] = out["nearest_primary_ms"]["median"] / out["gbuffer_ms"]["median"]
                out["any_primary_vs_gbuffer"] = out["any_primary_ms"]["median"] / out["gbuffer_ms"]["median"]
            res[name] = out
    line = json.dumps(res, allow_nan=False)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
