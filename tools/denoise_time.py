#!/usr/bin/env python3
"""Device times of the G-buffer render and the a-trous denoiser on one GPU.

Cornell box at SIZE^2 (default 1024).  After WARMUP untimed rounds, the median of REPEATS
(default 25, at least 20) HIP-event timings of
  gbuffer_ms            rvcp_render_gbuffer_async (events on the call's stream)
  denoise_ms            rvcp_denoise_async at the default parameters, its own events
                        (rvcp_denoise_wait), RGBA8 store included
  denoise_pass_ms[i]    pass i (step 2^i): the filter with i + 1 passes minus the filter with i
                        passes (no RGBA8 store), for i < PASSES (default 5)
  render_ms             the same run's plain frame at SPP = 30 and at the SPP the defaults were
                        chosen for (TARGET_SPP = 4), rvcp_stats_t.kernel_ms
and, per pass, the achieved bytes/s against the minimum traffic of a pass -- 12 B colour + 32 B
guide read and 12 B written per pixel, 56 B x W x H -- as a fraction of the 8 TB/s HBM peak.
Prints one JSON line.

    python tools/denoise_time.py [--size 1024] [--repeats 25] [--warmup 5] [--passes 5]
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

HBM_PEAK = 8.0e12               # bytes/s, the peak DESIGN.md §4.4 uses
TARGET_SPP = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    import torch
    n = a.size
    sc = rvcp_amd.Scene.default()
    push = sc.push_constant(123.0)
    d_rgba = torch.zeros(n * n, dtype=torch.int32, device="cuda")
    d_lin = torch.zeros(n * n * 3, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(n * n * 3, dtype=torch.float32, device="cuda")
    d_g = torch.zeros(n * n * 8, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    med = statistics.median
    res = dict(size=n, repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               version=abi.load().rvcp_version().decode())

    def rounds(f):
        for _ in range(a.warmup):
            f()
        return [f() for _ in range(a.repeats)]

    render_ms = {}
    for spp in (30, TARGET_SPP):
        with rvcp_amd.RayTracer(spp=spp) as rt:
            rt.upload_scene(sc)

            def render():
                rt.render_async(push, n, n, d_rgba.data_ptr(), d_lin.data_ptr(),
                                stream=stream.cuda_stream)
                return float(rt.wait()["kernel_ms"])
            render_ms[spp] = med(rounds(render))

            if spp != TARGET_SPP:
                continue
            # the G-buffer and the filter of the TARGET_SPP frame left in d_lin

            def gbuffer():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rt.render_gbuffer_async(push, n, n, d_g.data_ptr(), stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)
            res["gbuffer_ms"] = med(rounds(gbuffer))

            def denoise(params, rgba):
                def f():
                    rt.denoise_async(d_lin.data_ptr(), d_g.data_ptr(), n, n, d_out.data_ptr(),
                                     d_rgba.data_ptr() if rgba else 0, params,
                                     stream=stream.cuda_stream)
                    return rt.denoise_wait()
                return med(rounds(f))
            defaults = abi.make_denoise_params()
            # (an infinite sigma_color as the string "inf": strict JSON has no Infinity)
            res["params"] = {k: float(defaults[k]) if np.isfinite(defaults[k]) else str(float(defaults[k]))
                             for k in defaults.dtype.names}
            res["denoise_ms"] = denoise(defaults, True)
            chain = [0.0] + [denoise(abi.make_denoise_params(iterations=k), False)
                             for k in range(1, a.passes + 1)]
            res["denoise_chain_ms"] = chain[1:]
            res["denoise_pass_ms"] = [chain[k + 1] - chain[k] for k in range(a.passes)]
    res["render_spp30_ms"] = render_ms[30]
    res["render_target_spp"] = TARGET_SPP
    res["render_target_ms"] = render_ms[TARGET_SPP]
    min_bytes = 56.0 * n * n
    res["pass_min_bytes"] = min_bytes
    res["pass_bytes_per_s"] = [min_bytes / (ms * 1e-3) if ms > 0 else None
                               for ms in res["denoise_pass_ms"]]
    res["pass_fraction_of_hbm_peak"] = [b / HBM_PEAK if b else None for b in res["pass_bytes_per_s"]]
    res["gbuffer_plus_denoise_ms"] = res["gbuffer_ms"] + res["denoise_ms"]
    res["cheaper_than_spp30_frame"] = res["gbuffer_plus_denoise_ms"] < res["render_spp30_ms"]
    print(json.dumps(res, allow_nan=False))


if __name__ == "__main__":
    main()
