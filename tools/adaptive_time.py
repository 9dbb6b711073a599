#!/usr/bin/env python3
"""Cost and quality of adaptive sampling on one GPU.

The Cornell box at SIZE^2 (default 1024), the automatic schedule (the scene-specialised schedule
3).  Every comparison alternates its arms in this one process; after WARMUP untimed rounds, per arm
the median, minimum and maximum of REPEATS (default 25, at least 20) device times of a frame
(rvcp_stats_t.kernel_ms, HIP events).

 1. The price of the per-pixel count itself: a uniform map of s through the map kernels against
    rvcp_render_async at cfg.spp = s, for s = 4 and 30.
 2. The price of unequal chains: the map the chain plans at its defaults after 8 frames of
    rvcp_render_svgf, against the uniform map of 4; time per sample and wave_iterations per sample.
 3. The plan step's two kernels (rvcp_spp_plan_wait's plan_ms).
 4. Quality at equal budget, at 64^2: mean_spp = 4, eight frames at rest through
    rvcp_render_svgf, RMSE of clipped colours over the filterable pixels against the 2048-sample
    oracle render, eight seeds; adaptive against the uniform cfg.spp = 4, the samples both traced,
    and the fraction of pixels whose count changes by more than 1 between frames 4..8.

Prints one JSON line and, with --out, writes it to a file (profiles/adaptive_time_1024sq.json is
this tool's output).

    timeout -k 10 600 python tools/adaptive_time.py [--size 1024] [--repeats 25] [--warmup 5] [--out F]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import denoise_ref as R         # noqa: E402
import rvcp_amd                 # noqa: E402
from rvcp_amd import abi        # noqa: E402

Q_SIZE, Q_FRAMES = 64, 8
Q_SEEDS = tuple(5.0 + 10.0 * k for k in range(8))


def spread(x):
    return dict(median=statistics.median(x), min=min(x), max=max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    import torch
    n = a.size
    sc = rvcp_amd.Scene.default()
    res = dict(size=n, repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               version=abi.load().rvcp_version().decode())
    d_rgba = torch.zeros((n, n), dtype=torch.int32, device="cuda")

    def map_ms(rt, d_map, hint, t):
        rt.render_spp_map_async(sc.push_constant(t), n, n, d_map.data_ptr(), hint, d_rgba.data_ptr())
        return rt.wait()

    def default_ms(rt, t):
        rt.render_async(sc.push_constant(t), n, n, d_rgba.data_ptr())
        return rt.wait()

    # ---- 1. the per-pixel count itself
    for s in (4, 30):
        d_map = torch.full((n, n), s, dtype=torch.int32, device="cuda")
        with rvcp_amd.RayTracer(spp=s) as rt:
            rt.upload_scene(sc)
            ms = {"default": [], "map": []}
            for r in range(a.warmup + a.repeats):
                for arm in ("default", "map"):
                    st = default_ms(rt, float(r)) if arm == "default" else map_ms(rt, d_map, s, float(r))
                    if r >= a.warmup:
                        ms[arm].append(float(st["kernel_ms"]))
                    res[f"spp{s}_{arm}_kernel_variant"] = int(st["kernel_variant"])
            res[f"spp{s}_default_ms"], res[f"spp{s}_map_ms"] = spread(ms["default"]), spread(ms["map"])
            res[f"spp{s}_map_vs_default"] = res[f"spp{s}_map_ms"]["median"] / res[f"spp{s}_default_ms"]["median"]

    # ---- 2. unequal chains, 3. the plan step
    prm = abi.make_adaptive_params()
    with rvcp_amd.RayTracer(spp=4) as rt:
        rt.upload_scene(sc)
        rt.adaptive = prm
        for i in range(8):
            rt.render_svgf(n, n, 5.0 + i)
        planned = rt.adaptive_last_map()
        rt.adaptive = None
        d_plan = torch.from_numpy(planned.astype(np.int32)).cuda()
        d_uni = torch.full((n, n), 4, dtype=torch.int32, device="cuda")
        arms = {"planned": d_plan, "uniform4": d_uni}
        ms = {k: [] for k in arms}
        for r in range(a.warmup + a.repeats):
            for arm, d_map in arms.items():
                st = map_ms(rt, d_map, 4, 100.0 + r)
                if r >= a.warmup:
                    ms[arm].append(float(st["kernel_ms"]))
                res[f"{arm}_samples"] = int(st["samples"])
                res[f"{arm}_wave_iterations"] = int(st["wave_iterations"])
                res[f"{arm}_traversals"] = int(st["traversals"])
        for arm in arms:
            res[f"{arm}_ms"] = spread(ms[arm])
            res[f"{arm}_ns_per_sample"] = 1e6 * res[f"{arm}_ms"]["median"] / res[f"{arm}_samples"]
            res[f"{arm}_wave_iterations_per_sample"] = res[f"{arm}_wave_iterations"] / res[f"{arm}_samples"]
        res["planned_vs_uniform_ns_per_sample"] = res["planned_ns_per_sample"] / res["uniform4_ns_per_sample"]
        hist = np.bincount(planned.ravel(), minlength=int(prm["spp_max"]) + 1)
        res["planned_count_histogram"] = hist.tolist()
        # the plan step on the chain's own kind of inputs: variance, colour, lengths, G-buffer
        d_var = torch.rand((n, n), dtype=torch.float32, device="cuda") * 0.01
        d_lin = torch.rand((n, n, 3), dtype=torch.float32, device="cuda")
        d_len = torch.full((n, n), 8, dtype=torch.int32, device="cuda")
        d_g = torch.zeros((n * n * 32,), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((n, n), dtype=torch.int32, device="cuda")
        rt.render_gbuffer_async(sc.push_constant(5.0), n, n, d_g.data_ptr())
        torch.cuda.synchronize()
        plan = []
        for r in range(a.warmup + a.repeats):
            rt.spp_plan_async(d_var.data_ptr(), d_lin.data_ptr(), d_len.data_ptr(), d_g.data_ptr(), n, n,
                              d_out.data_ptr(), prm)
            t, total = rt.spp_plan_wait()
            if r >= a.warmup:
                plan.append(t)
        res["plan_ms"] = spread(plan)
        res["plan_samples"] = total

    # ---- 4. quality at equal budget
    q = Q_SIZE
    mask, ref = R.filterable(R.cornell_gbuffer(q, q)), R.cornell_reference(q, q)
    out = {}
    for name in ("uniform", "adaptive"):
        errs, samples, unstable = [], [], []
        with rvcp_amd.RayTracer(spp=4) as rt:
            rt.upload_scene(sc)
            if name == "adaptive":
                rt.adaptive = prm
            for s0 in Q_SEEDS:
                rt.svgf_reset()
                maps, total = [], 0
                for i in range(Q_FRAMES):
                    lin = rt.render_svgf(q, q, s0 + i, want_linear=True)[1]
                    total += int(rt.last_stats["samples"])
                    if name == "adaptive":
                        maps.append(rt.adaptive_last_map().astype(np.int64))
                errs.append(R.rmse(lin, ref, mask))
                samples.append(total)
                unstable += [float((np.abs(x - y) > 1).mean()) for x, y in zip(maps[3:-1], maps[4:])]
        out[name] = (errs, samples, unstable)
    res["quality_uniform_rmse"] = out["uniform"][0]
    res["quality_adaptive_rmse"] = out["adaptive"][0]
    res["quality_uniform_samples"] = out["uniform"][1]
    res["quality_adaptive_samples"] = out["adaptive"][1]
    assert all(x <= y for x, y in zip(out["adaptive"][1], out["uniform"][1]))
    res["quality_ratio_mean"] = float(np.mean(out["adaptive"][0]) / np.mean(out["uniform"][0]))
    res["quality_ratio_per_seed"] = [x / y for x, y in zip(out["adaptive"][0], out["uniform"][0])]
    res["quality_unstable_fraction"] = spread(out["adaptive"][2])
    line = json.dumps(res, allow_nan=False)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
