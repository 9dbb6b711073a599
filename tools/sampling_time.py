#!/usr/bin/env python3
"""Cost and quality of the cosine-weighted bounce against the default uniform one on one GPU
(rvcp_set_sampling).

Cost: the Cornell box at SIZE^2 (default 1024), SPP = 30, the automatic schedule (the
scene-specialised path kernel), one context per mode rendered alternately; after WARMUP untimed
rounds, per mode the median, minimum and maximum of REPEATS (default 25, at least 20) device
times of a frame (rvcp_stats_t.kernel_ms, HIP events) and the traversals of a frame.

Quality, at 64^2: the error of one SPP = 4 frame per seed (times 5.0 .. 12.0) against the
mode's OWN mean of 32 frames x SPP 64 at other seeds (the two modes do not converge to the same
image on the open box), as the RMSE of colours clipped to [0, 1] and as the L2 of the unclipped
linear colours, averaged over the seeds; and the same at equal time -- cosine at SPP = 8 against
uniform at SPP = round(8 x ms_cosine / ms_uniform).  Prints one JSON line and, with --out, writes
it to a file (profiles/sampling_time_1024sq.json is this tool's output).

    timeout -k 10 300 python tools/sampling_time.py [--size 1024] [--repeats 25] [--warmup 5] [--out F]

(one process, a few seconds; run it under a time limit like every step that uses the GPU)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rvcp_amd                 # noqa: E402
from rvcp_amd import abi        # noqa: E402

SPP = 30
Q_SIZE, Q_SPP, Q_EQUAL_SPP = 64, 4, 8
Q_SEEDS = tuple(5.0 + i for i in range(8))
REF_TIMES = tuple(300.0 + i for i in range(32))
MODES = (("uniform", abi.SAMPLING_UNIFORM), ("cosine", abi.SAMPLING_COSINE))


def errors(frames, mean):
    clipped, unclipped = [], []
    for f in frames:
        d = np.clip(f.astype(np.float64), 0, 1) - np.clip(mean, 0, 1)
        clipped.append(float(np.sqrt(np.mean(d * d))))
        d = f.astype(np.float64) - mean
        unclipped.append(float(np.sqrt(np.mean(d * d))))
    return float(np.mean(clipped)), float(np.mean(unclipped))


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
    res = dict(size=n, spp=SPP, repeats=a.repeats, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), version=abi.load().rvcp_version().decode())

    def tracer(mode, spp):
        rt = rvcp_amd.RayTracer(spp=spp)
        rt.sampling = mode
        rt.upload_scene(sc)
        return rt

    # ---- cost: alternating frames of the two modes
    rts = {name: tracer(mode, SPP) for name, mode in MODES}
    ms = {name: [] for name, _ in MODES}
    trav = {}
    for r in range(a.warmup + a.repeats):
        for name, _ in MODES:
            rts[name].render(n, n, float(r % 1000))
            if r >= a.warmup:
                ms[name].append(float(rts[name].last_stats["kernel_ms"]))
                trav.setdefault(name, []).append(int(rts[name].last_stats["traversals"]))
    for name, _ in MODES:
        res[f"{name}_ms"] = statistics.median(ms[name])
        res[f"{name}_ms_min"], res[f"{name}_ms_max"] = min(ms[name]), max(ms[name])
        res[f"{name}_traversals_per_frame"] = statistics.median(trav[name])
        res[f"{name}_kernel_variant"] = int(rts[name].last_stats["kernel_variant"])
        rts[name].close()
    res["cosine_vs_uniform_ms"] = res["cosine_ms"] / res["uniform_ms"]
    res["cosine_vs_uniform_traversals"] = (res["cosine_traversals_per_frame"] /
                                           res["uniform_traversals_per_frame"])
    res["cosine_vs_uniform_ms_per_traversal"] = (res["cosine_vs_uniform_ms"] /
                                                 res["cosine_vs_uniform_traversals"])

    # ---- quality at 64^2: equal samples, then equal time
    q = Q_SIZE
    equal_spp = {"cosine": Q_EQUAL_SPP,
                 "uniform": max(1, int(round(Q_EQUAL_SPP * res["cosine_vs_uniform_ms"])))}
    res["equal_time_spp"] = equal_spp
    for name, mode in MODES:
        with tracer(mode, 64) as rt:
            mean = np.zeros((q, q, 3), np.float64)
            for t in REF_TIMES:
                mean += rt.render(q, q, t, want_linear=True)[1]
            mean /= len(REF_TIMES)
        res[f"{name}_mean_of_reference"] = float(mean.mean())
        for label, spp in (("spp4", Q_SPP), ("equal_time", equal_spp[name])):
            with tracer(mode, spp) as rt:
                frames = [rt.render(q, q, t, want_linear=True)[1] for t in Q_SEEDS]
                trav_q = int(rt.last_stats["traversals"])
            c, u = errors(frames, mean)
            res[f"{name}_{label}_rmse_clipped"] = c
            res[f"{name}_{label}_l2_unclipped"] = u
            res[f"{name}_{label}_traversals"] = trav_q
    for label in ("spp4", "equal_time"):
        res[f"{label}_l2_ratio"] = res[f"cosine_{label}_l2_unclipped"] / res[f"uniform_{label}_l2_unclipped"]
        res[f"{label}_rmse_ratio"] = res[f"cosine_{label}_rmse_clipped"] / res[f"uniform_{label}_rmse_clipped"]
    res["spp4_variance_ratio"] = res["spp4_l2_ratio"] ** 2
    res["brightness_cosine_vs_uniform"] = res["cosine_mean_of_reference"] / res["uniform_mean_of_reference"]
    line = json.dumps(res, allow_nan=False)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
