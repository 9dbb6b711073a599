#!/usr/bin/env python3
"""Device times of the temporal accumulation step on one GPU.

Cornell box at SIZE^2 (default 1024), SPP = TARGET_SPP (4).  After WARMUP untimed rounds, the
median of REPEATS (default 25, at least 20) HIP-event timings of
  temporal_identity_ms      rvcp_temporal_accumulate_async, camera not moved (one tap), its own
                            events (rvcp_temporal_wait), no RGBA8 store
  temporal_reproject_ms     the same through the view of a camera moved by (60, 20, 0): four taps
  temporal_no_history_ms    the same without history (the floor: 44 B read, 16 B written)
  temporal_rgba_ms          the reprojection with the RGBA8 store
  denoise_pass_ms[2]        the yardstick: the direct a-trous pass (step 4) of the same run, the
                            filter with 3 passes minus the filter with 2 (tools/denoise_time.py)
  render_ms                 the plain frame, rvcp_stats_t.kernel_ms
and, end to end on the host clock (render + G-buffer + step [+ filter] + copies to the host),
rvcp_render_temporal with and without the spatial pass against rvcp_render_denoised and
rvcp_render of the same run.  For the step, the achieved bytes/s against its minimum traffic --
44 B of the current frame and 48 B of history read, 16 B written per pixel, 108 B x W x H (60 B
without history) -- as a fraction of the 8 TB/s HBM peak.  Prints one JSON line.

    timeout -k 10 300 python tools/temporal_time.py [--size 1024] [--repeats 25] [--warmup 5]

(one process, a few seconds; run it under a time limit like every step that uses the GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rvcp_amd                 # noqa: E402
from rvcp_amd import abi        # noqa: E402

HBM_PEAK = 8.0e12               # bytes/s, the peak DESIGN.md §4.4 uses
TARGET_SPP = 4
MOVE = (60.0, 20.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    import torch
    n = a.size
    sc = rvcp_amd.Scene.default()
    moved = rvcp_amd.Scene.default()
    moved.camera.position = (moved.camera.position + np.asarray(MOVE, np.float32)).astype(np.float32)
    push_prev, push_cur = sc.push_constant(123.0), moved.push_constant(124.0)
    i32, f32 = torch.int32, torch.float32
    d_rgba = torch.zeros(n * n, dtype=i32, device="cuda")
    d_lin = [torch.zeros(n * n * 3, dtype=f32, device="cuda") for _ in range(2)]     # prev, cur
    d_g = [torch.zeros(n * n * 8, dtype=i32, device="cuda") for _ in range(2)]
    d_len = [torch.zeros(n * n, dtype=i32, device="cuda") for _ in range(2)]         # prev, out
    d_out = torch.zeros(n * n * 3, dtype=f32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    med = statistics.median
    res = dict(size=n, repeats=a.repeats, warmup=a.warmup, spp=TARGET_SPP,
               device=torch.cuda.get_device_name(0), version=abi.load().rvcp_version().decode())

    def rounds(f):
        for _ in range(a.warmup):
            f()
        return [f() for _ in range(a.repeats)]

    with rvcp_amd.RayTracer(spp=TARGET_SPP) as rt:
        rt.upload_scene(sc)
        s = stream.cuda_stream

        def render(push, k):
            rt.render_async(push, n, n, d_rgba.data_ptr(), d_lin[k].data_ptr(), stream=s)
            ms = float(rt.wait()["kernel_ms"])
            rt.render_gbuffer_async(push, n, n, d_g[k].data_ptr(), stream=s)
            return ms
        render(push_prev, 0)
        res["render_ms"] = med(rounds(lambda: render(push_cur, 1)))
        # the previous frame's history: every filterable pixel at length 1
        rt.temporal_accumulate_async(None, d_lin[0].data_ptr(), d_g[0].data_ptr(), 0, 0, 0, n, n,
                                     d_out.data_ptr(), d_len[0].data_ptr(), stream=s)
        rt.temporal_wait()
        d_lin[0].copy_(d_out)
        torch.cuda.synchronize()

        def step(view, history, rgba):
            def f():
                rt.temporal_accumulate_async(
                    view, d_lin[1].data_ptr(), d_g[1].data_ptr(),
                    d_lin[0].data_ptr() if history else 0, d_g[0].data_ptr() if history else 0,
                    d_len[0].data_ptr() if history else 0, n, n, d_out.data_ptr(),
                    d_len[1].data_ptr(), d_rgba.data_ptr() if rgba else 0, stream=s)
                return rt.temporal_wait()
            return med(rounds(f))
        view = abi.temporal_view(push_prev, n, n)
        # identity: the current frame as its own history (the lengths stay the previous frame's, so
        # a pixel that frame could not filter has no history here either)
        keep = d_lin[0].clone(), d_g[0].clone()
        d_lin[0].copy_(d_lin[1])
        d_g[0].copy_(d_g[1])
        torch.cuda.synchronize()
        res["temporal_identity_ms"] = step(None, True, False)
        res["identity_continued"] = float((d_len[1] == 2).float().mean())
        d_lin[0].copy_(keep[0])
        d_g[0].copy_(keep[1])
        torch.cuda.synchronize()
        res["temporal_reproject_ms"] = step(view, True, False)
        res["reproject_continued"] = float((d_len[1] == 2).float().mean())
        res["temporal_rgba_ms"] = step(view, True, True)
        res["temporal_no_history_ms"] = step(None, False, False)

        def denoise(k):
            def f():
                rt.denoise_async(d_lin[1].data_ptr(), d_g[1].data_ptr(), n, n, d_out.data_ptr(), 0,
                                 abi.make_denoise_params(iterations=k), stream=s)
                return rt.denoise_wait()
            return med(rounds(f))
        chain = [0.0] + [denoise(k) for k in (1, 2, 3)]
        res["denoise_pass_ms"] = [chain[k + 1] - chain[k] for k in range(3)]

        # end to end, host clock around the synchronous calls
        def wall(f):
            def g():
                t0 = time.perf_counter()
                f()
                return (time.perf_counter() - t0) * 1e3
            return med(rounds(g))
        seeds = iter(range(10 ** 6))
        tp, dp = abi.make_temporal_params(), abi.make_denoise_params()
        res["e2e_render_ms"] = wall(lambda: rt.render(n, n, float(next(seeds) % 1000)))
        res["e2e_render_denoised_ms"] = wall(
            lambda: rt.render_denoised(n, n, float(next(seeds) % 1000), dp))
        res["e2e_render_temporal_ms"] = wall(
            lambda: rt.render_temporal(n, n, float(next(seeds) % 1000), tp))
        res["e2e_render_temporal_step_ms"] = rt.last_temporal_ms
        res["e2e_render_temporal_denoised_ms"] = wall(
            lambda: rt.render_temporal(n, n, float(next(seeds) % 1000), tp, dp))
    for key, nbytes in (("identity", 108.0), ("reproject", 108.0), ("no_history", 60.0)):
        ms = res[f"temporal_{key}_ms"]
        res[f"{key}_min_bytes"] = nbytes * n * n
        res[f"{key}_bytes_per_s"] = nbytes * n * n / (ms * 1e-3) if ms > 0 else None
        res[f"{key}_fraction_of_hbm_peak"] = (res[f"{key}_bytes_per_s"] / HBM_PEAK
                                              if res[f"{key}_bytes_per_s"] else None)
    res["yardstick_direct_pass_ms"] = res["denoise_pass_ms"][2]
    res["cheaper_than_direct_pass"] = res["temporal_reproject_ms"] < res["denoise_pass_ms"][2]
    print(json.dumps(res, allow_nan=False))


if __name__ == "__main__":
    main()
