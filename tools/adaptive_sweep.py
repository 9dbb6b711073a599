#!/usr/bin/env python3
"""Sweep of the adaptive-sampling parameters on one GPU: which
rvcp_adaptive_params_t should rvcp_adaptive_params_default return?

Input: a static Cornell box at SIZE^2 (default 64), a budget of mean_spp = 4 samples per pixel,
8 frames through rvcp_render_svgf (everything else at its defaults) per seed, eight seeds (frame i
of seed k at time 5 + 10 k + i).  Error: RMSE over the filterable pixels of the colour clamped to
[0, 1] of the 8th frame against an oracle render at SPP = REF_SPP (default 2048, time seed 77.0),
as README's SVGF row; per row its mean over the seeds as a ratio to the same chain at the uniform
cfg.spp = 4, the share of the budget the row really traced, and the loop's stability: the fraction
of pixels whose count changes by more than 1 between consecutive frames 4..8.  Grid: weight_cap
1/16 .. 16, epsilon 1e-4 / 1e-2, spp_max / mean_spp 2 / 4 / 8.  Prints the table, best first, and
one JSON line with the best row; --out writes that line to a file.

    timeout -k 10 600 python tools/adaptive_sweep.py [--size 64] [--ref-spp 2048] [--out F]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import denoise_ref as R       # noqa: E402
import rvcp_amd               # noqa: E402
from rvcp_amd import abi      # noqa: E402

MEAN_SPP = 4
FRAMES = 8
SEEDS = tuple(5.0 + 10.0 * k for k in range(8))
WEIGHT_CAP = (0.0625, 0.25, 1.0, 4.0, 16.0)
EPSILON = (1e-4, 1e-2)
MAX_OVER_MEAN = (2, 4, 8)


def run(sc, n, prm, ref, mask):
    """(mean RMSE, samples traced / budget, mean unstable fraction) of one row; prm None: uniform."""
    errs, spent, unstable = [], [], []
    with rvcp_amd.RayTracer(spp=MEAN_SPP) as rt:
        rt.upload_scene(sc)
        if prm is not None:
            rt.adaptive = prm
        for s0 in SEEDS:
            rt.svgf_reset()
            maps, samples = [], 0
            for i in range(FRAMES):
                lin = rt.render_svgf(n, n, s0 + i, want_linear=True)[1]
                samples += int(rt.last_stats["samples"])
                if prm is not None:
                    maps.append(rt.adaptive_last_map().astype(np.int64))
            errs.append(R.rmse(lin, ref, mask))
            spent.append(samples / float(FRAMES * MEAN_SPP * n * n))
            unstable += [float((np.abs(a - b) > 1).mean()) for a, b in zip(maps[3:-1], maps[4:])]
    return float(np.mean(errs)), float(np.mean(spent)), float(np.mean(unstable)) if unstable else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.size
    sc = rvcp_amd.Scene.default()
    mask = R.filterable(R.cornell_gbuffer(n, n))
    ref = R.cornell_reference(n, n, spp=a.ref_spp)
    uniform, _, _ = run(sc, n, None, ref, mask)
    print(f"uniform cfg.spp = {MEAN_SPP}: mean RMSE over {len(SEEDS)} seeds {uniform:.5f}", flush=True)
    rows = []
    for cap, eps, k in itertools.product(WEIGHT_CAP, EPSILON, MAX_OVER_MEAN):
        prm = abi.make_adaptive_params(spp_min=1, spp_max=k * MEAN_SPP, mean_spp=float(MEAN_SPP),
                                       weight_cap=cap, epsilon=eps)
        e, spent, unstable = run(sc, n, prm, ref, mask)
        rows.append((e, cap, eps, k, spent, unstable))
    rows.sort()
    print("| weight_cap | epsilon | spp_max / mean_spp | RMSE | ratio to uniform | budget traced | unstable |")
    print("|---|---|---|---|---|---|---|")
    for e, cap, eps, k, spent, unstable in rows:
        print(f"| {cap:g} | {eps:g} | {k} | {e:.5f} | {e / uniform:.3f} | {spent:.3f} | {unstable:.3f} |")
    e, cap, eps, k, spent, unstable = rows[0]
    line = json.dumps(dict(size=n, ref_spp=a.ref_spp, mean_spp=MEAN_SPP, frames=FRAMES,
                           seeds=list(SEEDS), uniform_rmse=uniform,
                           best=dict(weight_cap=cap, epsilon=eps, spp_max_over_mean=k),
                           best_rmse=e, best_ratio=e / uniform, best_budget_traced=spent,
                           best_unstable=unstable, rows=len(rows)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
