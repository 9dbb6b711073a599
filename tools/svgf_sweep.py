#!/usr/bin/env python3
"""Sweep of the SVGF parameters on the CPU: which rvcp_svgf_params_t should
rvcp_svgf_params_default return, and is feedback worth its bias?

Input: a static Cornell box at SIZE^2 (default 64), SPP = 4, 8 oracle frames at the time seeds
5.0 ... 12.0 (the set of §4.10).  The chain is tests/svgf_ref.py (the numpy float32 restatement of
csrc/rvcp_svgf.hip) under the CPU G-buffer of tests/denoise_ref.py, the temporal parameters at
their defaults.  Error: RMSE over the filterable pixels of the colour clamped to [0, 1] of the
8th frame's output against an oracle render at SPP = REF_SPP (default 2048, time seed 77.0), as a
ratio to the first raw frame's.  Grid: iterations 3-5, sigma_luminance 1/2/4/8, spatial_below 1/4,
feedback off/on.  Two yardsticks from the same frames: the temporal-only accumulation (§4.10) and
that accumulation filtered by the a-trous filter at its defaults (§4.9).  Prints the table, best
first, and one JSON line with the best row.  No GPU.

    python tools/svgf_sweep.py [--size 64] [--ref-spp 2048]
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import denoise_ref as R       # noqa: E402
import svgf_ref as S          # noqa: E402
import temporal_ref as T      # noqa: E402
import oracle as O            # noqa: E402
import rvcp_amd               # noqa: E402
from rvcp_amd import abi      # noqa: E402

SPP = 4
ITERATIONS = (3, 4, 5)
SIGMA_LUMINANCE = (1.0, 2.0, 4.0, 8.0)
SPATIAL_BELOW = (1, 4)
FEEDBACK = (False, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=2048)
    a = ap.parse_args()
    n = a.size
    sc = rvcp_amd.Scene.default()
    arrays = dict(materials=sc.aligned_materials(), vertices=sc.mesh.aligned_vertices(),
                  faces=sc.mesh.aligned_faces(), lum_face_ids=sc.luminous_face_ids())
    g = R.cpu_gbuffer(sc, n, n)
    mask = R.filterable(g)
    ref, _, _ = O.render(arrays, sc.push_constant(77.0), abi.make_config(spp=a.ref_spp), n, n)
    frames = [O.render(arrays, sc.push_constant(t), abi.make_config(spp=SPP), n, n)[0]
              for t in S.QUALITY_SEEDS]
    first = R.rmse(frames[0], ref, mask)
    tp = T.params()
    acc = length = None
    for c in frames:
        acc, length = T.accumulate(c, g, acc, None if acc is None else g, length, None, tp)
    dp = abi.make_denoise_params()
    y_temporal = R.rmse(acc, ref, mask)
    y_filtered = R.rmse(R.denoise_params(acc, g, dp), ref, mask)
    print(f"first raw frame RMSE {first:.4f}; temporal only {y_temporal:.4f} (ratio "
          f"{y_temporal / first:.3f}); temporal + a-trous defaults {y_filtered:.4f} (ratio "
          f"{y_filtered / first:.3f})", flush=True)
    rows = []
    for it, sl, below, fb in itertools.product(ITERATIONS, SIGMA_LUMINANCE, SPATIAL_BELOW, FEEDBACK):
        chain = S.Chain(tp, S.params(iterations=it, sigma_luminance=sl, spatial_below=below), fb)
        for c in frames:
            out, _, _ = chain.frame(c, g, None)
        rows.append((R.rmse(out, ref, mask), it, sl, below, fb))
    rows.sort()
    print("| iterations | sigma_luminance | spatial_below | feedback | RMSE | ratio to the first raw frame |")
    print("|---|---|---|---|---|---|")
    for e, it, sl, below, fb in rows:
        print(f"| {it} | {sl:g} | {below} | {'on' if fb else 'off'} | {e:.4f} | {e / first:.3f} |")
    e, it, sl, below, fb = rows[0]
    print(json.dumps(dict(size=n, ref_spp=a.ref_spp, spp=SPP, seeds=list(S.QUALITY_SEEDS),
                          first_raw_rmse=first, temporal_only_rmse=y_temporal,
                          temporal_atrous_rmse=y_filtered,
                          best=dict(iterations=it, sigma_luminance=sl, spatial_below=below,
                                    feedback=fb), best_rmse=e, best_ratio=e / first,
                          beats_both=bool(e < y_temporal and e < y_filtered), rows=len(rows))))


if __name__ == "__main__":
    main()
