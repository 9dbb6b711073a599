#!/usr/bin/env python3
"""Sweep of the a-trous denoiser's parameters on the CPU: which
rvcp_denoise_params_t should rvcp_denoise_params_default return?

Input: oracle renders of the Cornell box at SIZE^2 (default 128), SPP in {1, 4, 10}; the filter is
tests/denoise_ref.py (the numpy float32 restatement of csrc/rvcp_denoise.hip) under the CPU
G-buffer of the same module.  Error: RMSE over the filterable pixels of the colour clamped to
[0, 1] against an oracle render at SPP = REF_SPP (default 2048, another time seed).  Prints one
table row per parameter set (the RMSE ratio denoised / noisy per SPP and its mean), best mean
first (ties: see main), and one JSON line with the best row.  No GPU.

    python tools/denoise_sweep.py [--size 128] [--ref-spp 2048] [--top 12]
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
import oracle as O            # noqa: E402
import rvcp_amd               # noqa: E402

SPPS = (1, 4, 10)
ITERATIONS = (1, 2, 3, 4, 5)
NORMAL_POWER_LOG2 = (0, 3, 5, 7)
SIGMA_COLOR = (0.1, 0.3, 1.0, 3.0, float("inf"))
SIGMA_PLANE = (0.1, 1.0, 10.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--top", type=int, default=12)
    a = ap.parse_args()
    n = a.size
    sc = rvcp_amd.Scene.default()
    arrays = dict(materials=sc.aligned_materials(), vertices=sc.mesh.aligned_vertices(),
                  faces=sc.mesh.aligned_faces(), lum_face_ids=sc.luminous_face_ids())
    g = R.cpu_gbuffer(sc, n, n)
    mask = R.filterable(g)
    ref, _, _ = O.render(arrays, sc.push_constant(77.0), rvcp_amd.abi.make_config(spp=a.ref_spp), n, n)
    noisy = {spp: O.render(arrays, sc.push_constant(5.0), rvcp_amd.abi.make_config(spp=spp), n, n)[0]
             for spp in SPPS}
    base = {spp: R.rmse(noisy[spp], ref, mask) for spp in SPPS}
    print("noisy RMSE: " + "  ".join(f"SPP={s}: {base[s]:.4f}" for s in SPPS), flush=True)
    rows = []
    for it, npow, sc_, sp in itertools.product(ITERATIONS, NORMAL_POWER_LOG2, SIGMA_COLOR, SIGMA_PLANE):
        ratios = [R.rmse(R.denoise(noisy[spp], g, it, npow, sc_, sp), ref, mask) / base[spp]
                  for spp in SPPS]
        rows.append((float(np.mean(ratios)), it, npow, sc_, sp, ratios))
    # best mean first, compared to three decimals (two time seeds differ by more); rows that tie
    # -- on the Cornell box's flat, axis-aligned walls the two geometric weights cannot tell
    # parameter sets apart -- go to the stricter geometric edge-stopping (higher normal power,
    # then smaller sigma_plane), which is what keeps curved or close surfaces apart
    rows.sort(key=lambda r: (round(r[0], 3), -r[2], r[4]))
    print("| iterations | normal_power_log2 | sigma_color | sigma_plane | "
          + " | ".join(f"SPP={s}" for s in SPPS) + " | mean |")
    print("|---|---|---|---|" + "---|" * (len(SPPS) + 1))
    for mean, it, npow, sc_, sp, ratios in rows[:a.top] + rows[-3:]:
        print(f"| {it} | {npow} | {sc_} | {sp} | " + " | ".join(f"{r:.3f}" for r in ratios)
              + f" | {mean:.3f} |")
    mean, it, npow, sc_, sp, ratios = rows[0]
    print(json.dumps(dict(size=n, ref_spp=a.ref_spp, spps=SPPS, noisy_rmse=[base[s] for s in SPPS],
                          best=dict(iterations=it, normal_power_log2=npow, sigma_color=sc_,
                                    sigma_plane=sp),
                          ratios=ratios, mean_ratio=mean, rows=len(rows))))


if __name__ == "__main__":
    main()
